// frs_window_row.h -- one output of a windowed resample from its taps: WinParams (the geometry of a call) and
// WinRow<MODE, T, Mask> (what a destination row needs of the y axis, and one output of that row), written once for the
// host and the device.  Includes nothing from HIP: a plain C++ compiler builds it, hipcc builds the same text as
// __host__ __device__.  Needs -ffp-contract=off like the rest of the library.  Users: window_group in frs_window.hip,
// which stores the outputs in the source dtype, and render_group in frs_render.h, which maps them to 8-bit colour.
//
// WinRow::output computes one output and hands it to a result policy: out.hit(v) for a value computed from data,
// out.miss() where there is none (an axis is invalid, masked nearest hit a nodata tap, a masked output has no valid
// weight).  WinRow::pixel is output under WinFill (miss() is `fill`): what frs_resample_window* stores.  WinRow::sample
// is output under WinFlag: the value and whether it has data, `has` being false exactly where pixel returns `fill`.
#pragma once
#include <stdint.h>

#include "frs_nodata.h"
#include "frs_window_map.h"

namespace frs {

struct WinParams {
    int64_t src_h, src_w, dst_h, dst_w;
    int64_t src_row_stride, src_band_stride, dst_row_stride, dst_band_stride;
    double x0, y0, width, height, fill;
};

// one output: the value in the dtype, and whether it was computed from data (v means nothing without)
template <typename T> struct WinSample {
    T v;
    bool has;
};
// the result policies of WinRow::output
template <typename T> struct WinFill {
    using type = T;
    T fill;
    FRS_HD T hit(T v) const { return v; }
    FRS_HD T miss() const { return fill; }
};
template <typename T> struct WinFlag {
    using type = WinSample<T>;
    FRS_HD WinSample<T> hit(T v) const { return WinSample<T>{v, true}; }
    FRS_HD WinSample<T> miss() const { return WinSample<T>{(T)0, false}; }
};
// a masked windowed value in the dtype: win_result and the integer nudge where the valid weight is above 0
template <typename T, typename Out>
FRS_HD inline typename Out::type nd_win_output(const NdValue &r, T nd, const Out &out) {
    return r.valid ? out.hit(nd_nudge(win_result<T>(r.v), nd)) : out.miss();
}

// What a destination row needs of the y axis, and one output of that row.  `mask` is NoNodata, or Nodata<T>: then a
// nodata tap is left out of the output, and an output without a valid tap has no data.
template <int MODE, typename T, typename Mask> struct WinRow;

template <typename T, typename Mask> struct WinRow<kWindowNearest, T, Mask> {
    const T *s0;
    bool valid;
    Mask mask;
    FRS_HD WinRow(const T *src, const WinParams &P, const WinAxis &ay, int64_t r, const Mask &mask_) : mask(mask_) {
        const WinNearest n = win_nearest(ay, r);
        valid = n.valid, s0 = src + n.i * P.src_row_stride;
    }
    template <typename Out> FRS_HD typename Out::type output(const WinAxis &ax, int64_t x, const Out &out) const {
        const WinNearest n = win_nearest(ax, x);
        if (!(valid && n.valid)) return out.miss();
        const T v = s0[n.i];
        if constexpr (Mask::masked) return nd_is(v, mask.nd) ? out.miss() : out.hit(v);
        else return out.hit(v);
    }
    FRS_HD T pixel(const WinAxis &ax, int64_t x, T fill) const { return output(ax, x, WinFill<T>{fill}); }
    FRS_HD WinSample<T> sample(const WinAxis &ax, int64_t x) const { return output(ax, x, WinFlag<T>{}); }
};

template <typename T, typename Mask> struct WinRow<kWindowBilinear, T, Mask> {
    const T *s0, *s1;
    double t;
    bool valid;
    Mask mask;
    FRS_HD WinRow(const T *src, const WinParams &P, const WinAxis &ay, int64_t r, const Mask &mask_) : mask(mask_) {
        const WinLinear l = win_linear(ay, r);
        valid = l.valid, t = l.t;
        s0 = src + l.i0 * P.src_row_stride, s1 = src + l.i1 * P.src_row_stride;
    }
    template <typename Out> FRS_HD typename Out::type output(const WinAxis &ax, int64_t x, const Out &out) const {
        const WinLinear l = win_linear(ax, x);
        if (!(valid && l.valid)) return out.miss();
        if constexpr (Mask::masked) {
            const T a = s0[l.i0], b = s0[l.i1], c = s1[l.i0], d = s1[l.i1], nd = mask.nd;
            return nd_win_output<T>(nd_bilinear((double)a, (double)b, (double)c, (double)d, !nd_is(a, nd),
                                                !nd_is(b, nd), !nd_is(c, nd), !nd_is(d, nd), l.t, t),
                                    nd, out);
        } else {
            const double a = (double)s0[l.i0], b = (double)s0[l.i1], c = (double)s1[l.i0], d = (double)s1[l.i1];
            return out.hit(win_result<T>(win_bilinear_value(a, b, c, d, l.t, t)));
        }
    }
    FRS_HD T pixel(const WinAxis &ax, int64_t x, T fill) const { return output(ax, x, WinFill<T>{fill}); }
    FRS_HD WinSample<T> sample(const WinAxis &ax, int64_t x) const { return output(ax, x, WinFlag<T>{}); }
};

template <typename T, typename Mask> struct WinRow<kWindowAverage, T, Mask> {
    const T *src;
    int64_t row_stride;
    WinArea ry;
    Mask mask;
    FRS_HD WinRow(const T *src_, const WinParams &P, const WinAxis &ay, int64_t r, const Mask &mask_)
        : src(src_), row_stride(P.src_row_stride), ry(win_area(ay, r)), mask(mask_) {}
    template <typename Out> FRS_HD typename Out::type output(const WinAxis &ax, int64_t x, const Out &out) const {
        const WinArea rx = win_area(ax, x);
        if (!(ry.valid && rx.valid)) return out.miss();
        if constexpr (Mask::masked) {
            NdArea acc;
            for (int64_t j = ry.i0; j < ry.i1; j++) {
                const T *s = src + j * row_stride;
                for (int64_t i = rx.i0; i < rx.i1; i++) {
                    const T v = s[i];
                    acc.tap(win_area_weight(rx, i), (double)v, !nd_is(v, mask.nd));
                }
                acc.end_row(win_area_weight(ry, j));
            }
            return nd_win_output<T>(acc.value(rx, ry), mask.nd, out);
        } else {
            double sum = 0.0;
            for (int64_t j = ry.i0; j < ry.i1; j++) {
                const T *s = src + j * row_stride;
                double row = 0.0;
                for (int64_t i = rx.i0; i < rx.i1; i++) row = row + win_area_weight(rx, i) * (double)s[i];
                sum = sum + win_area_weight(ry, j) * row;
            }
            return out.hit(win_result<T>(win_area_value(sum, rx, ry)));
        }
    }
    FRS_HD T pixel(const WinAxis &ax, int64_t x, T fill) const { return output(ax, x, WinFill<T>{fill}); }
    FRS_HD WinSample<T> sample(const WinAxis &ax, int64_t x) const { return output(ax, x, WinFlag<T>{}); }
};

}  // namespace frs
