// frs_nodata.h -- the scalar arithmetic of the nodata-aware forms of the pyramid step (frs_downsample2_nodata*) and of
// the windowed resample (frs_resample_window_nodata*), written once for the host and the device.  Includes nothing from
// HIP, only the two headers whose arithmetic it extends: a plain C++ compiler builds it (tests/test_nodata_host.py
// compares it with exact integers and with the numpy restatement in tests/nodata_ref.py, bit for bit), hipcc builds the
// same text as __host__ __device__.  Needs -ffp-contract=off like the rest of the library: every operator below is one
// IEEE operation.  Users: downsample_group in frs_pyramid.hip and window_group in frs_window.hip under their Nodata<T>
// policy (at the end of this file); they keep their own loads, stores and loops.
//
// The definitions are the project's own (no parity with GDAL's or any other library's masked resampling is claimed).
//
// Nodata predicate.  nd is a double; ndT = (T)nd is what the dtype holds.  Integer dtypes: nd must be an integer value
// inside the dtype's range (nd_representable; the entry points reject anything else), a pixel is nodata iff v == ndT.
// Float dtypes: a pixel is nodata iff v == ndT or both are NaN; +-inf is allowed; -0.0 matches 0.0.
//
// Masked 2x average.  The block is frs_resample.h's: n = 4, 2 or 1 source pixels, never padded.  Its m <= n valid
// pixels v1 .. vm are taken in the order a, b, c, d.
//   m = 0      ndT
//   integers   floor((2 s + m) / (2 m)) of the exact 64-bit sum s of the valid pixels: the mean rounded half towards
//              +infinity, frs_resample.h's rule with m in place of n (m = 3 is a true floor division by 6).
//   floats     m = 4: ((v1 + v2) + (v3 + v4)) * 0.25; m = 3: ((v1 + v2) + v3) / 3; m = 2: (v1 + v2) * 0.5; m = 1: v1.
//              Every operation is rounded in the dtype.
// With every pixel of the block valid this is resample_avg4 / resample_avg2, bit for bit (before the nudge).
// Integer nudge: a mean (m > 0, m = n included) that equals ndT becomes ndT + 1, or ndT - 1 when ndT is the dtype's
// maximum, so that no hole appears where data exists.  Floats are not nudged: a float mean that hits ndT exactly needs
// a contrived input (the valid pixels, none of which is ndT, averaging to it to the last bit).
// Nearest is unchanged: the pixel (2r, 2x) is copied, nodata or not.
//
// Masked windowed resample.  Indices, weights and axis validity are frs_window_map.h's, unchanged.  An output whose
// valid weight is zero (it lies outside the source, all its taps are nodata, or its only valid taps have weight 0) gets
// `fill`, converted by win_result.
//   nearest    a nodata tap gives fill
//   bilinear   weights w00 = (1-tx)(1-ty), w01 = tx(1-ty), w10 = (1-tx)ty, w11 = tx ty.  All four taps valid:
//              win_bilinear_value, as without nodata.  Otherwise num and den start from 0.0 and the valid taps are
//              accumulated in the order 00, 01, 10, 11: num = num + w v, den = den + w; den == 0 gives fill, else
//              num / den.
//   average    per row, over its valid taps with columns ascending: row = row + wx v, roww = roww + wx; then with rows
//              ascending sum = sum + wy row, wsum = wsum + wy roww.  No tap nodata: win_area_value(sum, rx, ry), as
//              without nodata.  Otherwise wsum == 0 gives fill, else sum / wsum.
// Integer results take win_result; when the valid weight is above 0 and the result equals ndT the same +-1 nudge
// applies.  fill must be finite; for float dtypes it may also be NaN (a NaN-nodata raster filled with NaN).
#pragma once
#include <stdint.h>

#include "frs_resample.h"
#include "frs_window_map.h"

namespace frs {

template <typename T> struct NdFloat { static constexpr bool value = false; };
template <> struct NdFloat<float> { static constexpr bool value = true; };
template <> struct NdFloat<double> { static constexpr bool value = true; };

// may nd be the nodata value of a raster of T?  (integers: an integer inside the range; NaN fails both comparisons)
template <typename T> FRS_HD inline bool nd_representable(double nd) {
    if constexpr (NdFloat<T>::value) return true;
    else return nd >= WinLimits<T>::lo && nd <= WinLimits<T>::hi && __builtin_floor(nd) == nd;
}
// may `fill` be the fill value of a masked windowed resample of T?
template <typename T> FRS_HD inline bool nd_fill_ok(double fill) {
    return fill - fill == 0.0 || (NdFloat<T>::value && fill != fill);
}

// ndT = (T)nd (nd is representable)
template <typename T> FRS_HD inline T nd_cast(double nd) {
    if constexpr (NdFloat<T>::value) return (T)nd;
    else return (T)(int64_t)nd;
}

// the predicate
template <typename T> FRS_HD inline bool nd_is(T v, T nd) {
    if constexpr (NdFloat<T>::value) return v == nd || (v != v && nd != nd);
    else return v == nd;
}

// the integer nudge of a result computed from at least one valid pixel (floats: unchanged)
template <typename T> FRS_HD inline T nd_nudge(T r, T nd) {
    if constexpr (NdFloat<T>::value) return r;
    else {
        if (r != nd) return r;
        return (double)nd == WinLimits<T>::hi ? (T)(nd - 1) : (T)(nd + 1);
    }
}

// floor(a / 6)
FRS_HD inline int64_t nd_floor_div6(int64_t a) {
    const int64_t q = a / 6;
    return a - q * 6 < 0 ? q - 1 : q;
}

// the masked mean of the m (0 .. 4) valid pixels v[0 .. m), in block order
template <typename T> FRS_HD inline T nd_mean(const T *v, int m, T nd) {
    if (m == 0) return nd;
    if constexpr (NdFloat<T>::value) {
        if (m == 4) return resample_avg4(v[0], v[1], v[2], v[3]);
        if (m == 3) return ((v[0] + v[1]) + v[2]) / (T)3;
        if (m == 2) return resample_avg2(v[0], v[1]);
        return v[0];
    } else {
        int64_t s = 0;
        for (int i = 0; i < m; i++) s += (int64_t)v[i];
        // floor((2 s + m) / (2 m)): a shift for m = 1, 2, 4
        const int64_t q = m == 3 ? nd_floor_div6(2 * s + 3) : resample_round_shift(s, m >> 1);
        return nd_nudge((T)q, nd);
    }
}

// the masked average of a block of n = 4 (a, b, c, d), 2 (a, b) or 1 (a) pixels
template <typename T> FRS_HD inline T nd_avg(T a, T b, T c, T d, int n, T nd) {
    T v[4];
    int m = 0;
    if (!nd_is(a, nd)) v[m++] = a;
    if (n >= 2 && !nd_is(b, nd)) v[m++] = b;
    if (n == 4 && !nd_is(c, nd)) v[m++] = c;
    if (n == 4 && !nd_is(d, nd)) v[m++] = d;
    return nd_mean(v, m, nd);
}

// a masked windowed value before its conversion to the dtype: `valid` is "the valid weight is above 0"
struct NdValue {
    double v;
    bool valid;
};

// bilinear: taps a, b (upper row), c, d as doubles, oa .. od say which are valid (not nodata)
FRS_HD inline NdValue nd_bilinear(double a, double b, double c, double d, bool oa, bool ob, bool oc, bool od, double tx,
                                  double ty) {
    NdValue r;
    if (oa && ob && oc && od) {
        r.v = win_bilinear_value(a, b, c, d, tx, ty), r.valid = true;
        return r;
    }
    const double w00 = (1.0 - tx) * (1.0 - ty), w01 = tx * (1.0 - ty), w10 = (1.0 - tx) * ty, w11 = tx * ty;
    double num = 0.0, den = 0.0;
    if (oa) num = num + w00 * a, den = den + w00;
    if (ob) num = num + w01 * b, den = den + w01;
    if (oc) num = num + w10 * c, den = den + w10;
    if (od) num = num + w11 * d, den = den + w11;
    r.valid = !(den == 0.0);
    r.v = r.valid ? num / den : 0.0;
    return r;
}

// average: the accumulators of one output.  tap() per tap of a row with columns ascending, end_row() after each row
// with rows ascending, value() at the end.
struct NdArea {
    double sum = 0.0, wsum = 0.0, row = 0.0, roww = 0.0;
    bool masked = false;  // a tap was nodata
    FRS_HD void tap(double wx, double v, bool ok) {
        if (ok) row = row + wx * v, roww = roww + wx;
        else masked = true;
    }
    FRS_HD void end_row(double wy) {
        sum = sum + wy * row, wsum = wsum + wy * roww;
        row = 0.0, roww = 0.0;
    }
    FRS_HD NdValue value(const WinArea &rx, const WinArea &ry) const {
        NdValue r;
        if (!masked) r.v = win_area_value(sum, rx, ry), r.valid = true;
        else r.valid = !(wsum == 0.0), r.v = r.valid ? sum / wsum : 0.0;
        return r;
    }
};

// the value in the dtype: fill when the valid weight is zero, else win_result and the integer nudge
template <typename T> FRS_HD inline T nd_win_result(const NdValue &r, T fill, T nd) {
    return r.valid ? nd_nudge(win_result<T>(r.v), nd) : fill;
}

// The mask policy of the lane functions (downsample_group, window_group): NoNodata compiles the forms of
// frs_resample.h / frs_window_map.h alone, Nodata<T> the forms above with nd = ndT.
struct NoNodata {
    static constexpr bool masked = false;
};
template <typename T> struct Nodata {
    static constexpr bool masked = true;
    T nd;
};

}  // namespace frs
