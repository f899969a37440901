// frs_composite.h -- the arithmetic and the lane function of the three-band colour composite of a windowed read
// (frs_render_composite_window*), written once for the host and the device.  Includes nothing from HIP, only
// frs_render.h, whose quantiser, chunk type and launch constants it uses: a plain C++ compiler builds it
// (tests/test_composite_host.py runs composite_group lane by lane against tests/render_ref.py applied per plane, bit for
// bit), hipcc builds the same text as __host__ __device__.  Needs -ffp-contract=off like the rest of the library.  User:
// k_render_composite_window in frs_composite.hip, which only places the LUT and calls composite_group.
//
// The definition is frs_render.h's, three times.  The source is band-planar: plane c starts c * src_band_stride elements
// after plane 0 and shares its shape and row stride.  For c in {0, 1, 2}, v_c and has_data_c are exactly what
// render_group computes for plane c alone (WinRow::output of frs_window_row.h: the same taps, weights, rounding, nudge
// and NaN rule), i_c = render_index(range[c], (double)v_c), and byte c of the pixel is byte c of lut[i_c]: R from the R
// bytes, G from the G bytes, B from the B bytes.  A = 255.  A pixel where any plane has no data is nodata_rgba, whole.
// The destination is pixel-interleaved R, G, B, A (four channels only) and the store contract is render_rows': aligned
// 16-byte chunks inside a row, bytes at its head and tail.
//
// What is shared.  An output's indices, weights and validity depend on the mapping and the output position alone, not
// on the plane: CompRow computes them once per destination row (y axis) and once per output (x axis) and reads the taps
// of the three planes at the same offsets.  Per plane only the loads, the accumulation and the quantiser remain; each
// plane's operations come in WinRow's order, so the values are WinRow's bit for bit.
#pragma once
#include <stdint.h>

#include "frs_render.h"

namespace frs {

struct CompParams {
    HistRange range[3];    // lo, hi, scale and n of each channel
    const uint32_t *lut;   // n packed entries
    uint32_t nodata_rgba;
};

// byte c of the entry that plane c's value selects, ORed into rgba; false for a NaN (no data)
template <typename T> FRS_HD inline bool comp_channel(const CompParams &R, int c, T v, uint32_t &rgba) {
    if constexpr (NdFloat<T>::value) {
        if (v != v) return false;
    }
    rgba |= R.lut[render_index(R.range[c], (double)v)] & (0xffu << (8 * c));
    return true;
}

// What a destination row needs of the y axis, and one composite pixel of that row: WinRow<MODE, T, Mask> over three
// planes with the axis arithmetic done once.
template <int MODE, typename T, typename Mask> struct CompRow;

template <typename T, typename Mask> struct CompRow<kWindowNearest, T, Mask> {
    const T *s0;
    int64_t bs;
    bool valid;
    Mask mask;
    FRS_HD CompRow(const T *src, const WinParams &P, const WinAxis &ay, int64_t r, const Mask &mask_)
        : bs(P.src_band_stride), mask(mask_) {
        const WinNearest n = win_nearest(ay, r);
        valid = n.valid, s0 = src + n.i * P.src_row_stride;
    }
    FRS_HD uint32_t pixel(const WinAxis &ax, int64_t x, const CompParams &R) const {
        const WinNearest n = win_nearest(ax, x);
        if (!(valid && n.valid)) return R.nodata_rgba;
        uint32_t rgba = 0xff000000u;
        bool has = true;
        FRS_UNROLL
        for (int c = 0; c < 3; c++) {
            const T v = s0[c * bs + n.i];
            if constexpr (Mask::masked) has = has && !nd_is(v, mask.nd);
            has = comp_channel(R, c, v, rgba) && has;
        }
        return has ? rgba : R.nodata_rgba;
    }
};

template <typename T, typename Mask> struct CompRow<kWindowBilinear, T, Mask> {
    const T *s0, *s1;
    int64_t bs;
    double t;
    bool valid;
    Mask mask;
    FRS_HD CompRow(const T *src, const WinParams &P, const WinAxis &ay, int64_t r, const Mask &mask_)
        : bs(P.src_band_stride), mask(mask_) {
        const WinLinear l = win_linear(ay, r);
        valid = l.valid, t = l.t;
        s0 = src + l.i0 * P.src_row_stride, s1 = src + l.i1 * P.src_row_stride;
    }
    FRS_HD uint32_t pixel(const WinAxis &ax, int64_t x, const CompParams &R) const {
        const WinLinear l = win_linear(ax, x);
        if (!(valid && l.valid)) return R.nodata_rgba;
        uint32_t rgba = 0xff000000u;
        bool has = true;
        FRS_UNROLL
        for (int c = 0; c < 3; c++) {
            const T *p0 = s0 + c * bs, *p1 = s1 + c * bs;
            const T a = p0[l.i0], b = p0[l.i1], cc = p1[l.i0], d = p1[l.i1];
            T v;
            if constexpr (Mask::masked) {
                const T nd = mask.nd;
                const NdValue r = nd_bilinear((double)a, (double)b, (double)cc, (double)d, !nd_is(a, nd), !nd_is(b, nd),
                                              !nd_is(cc, nd), !nd_is(d, nd), l.t, t);
                has = has && r.valid;
                v = nd_nudge(win_result<T>(r.v), nd);
            } else {
                v = win_result<T>(win_bilinear_value((double)a, (double)b, (double)cc, (double)d, l.t, t));
            }
            has = comp_channel(R, c, v, rgba) && has;
        }
        return has ? rgba : R.nodata_rgba;
    }
};

template <typename T, typename Mask> struct CompRow<kWindowAverage, T, Mask> {
    const T *src;
    int64_t row_stride, bs;
    WinArea ry;
    Mask mask;
    FRS_HD CompRow(const T *src_, const WinParams &P, const WinAxis &ay, int64_t r, const Mask &mask_)
        : src(src_), row_stride(P.src_row_stride), bs(P.src_band_stride), ry(win_area(ay, r)), mask(mask_) {}
    FRS_HD uint32_t pixel(const WinAxis &ax, int64_t x, const CompParams &R) const {
        const WinArea rx = win_area(ax, x);
        if (!(ry.valid && rx.valid)) return R.nodata_rgba;
        uint32_t rgba = 0xff000000u;
        bool has = true;
        if constexpr (Mask::masked) {
            NdArea acc[3];
            for (int64_t j = ry.i0; j < ry.i1; j++) {
                const T *s = src + j * row_stride;
                for (int64_t i = rx.i0; i < rx.i1; i++) {
                    const double wx = win_area_weight(rx, i);
                    FRS_UNROLL
                    for (int c = 0; c < 3; c++) {
                        const T v = s[c * bs + i];
                        acc[c].tap(wx, (double)v, !nd_is(v, mask.nd));
                    }
                }
                const double wy = win_area_weight(ry, j);
                FRS_UNROLL
                for (int c = 0; c < 3; c++) acc[c].end_row(wy);
            }
            FRS_UNROLL
            for (int c = 0; c < 3; c++) {
                const NdValue r = acc[c].value(rx, ry);
                has = has && r.valid;
                has = comp_channel(R, c, nd_nudge(win_result<T>(r.v), mask.nd), rgba) && has;
            }
        } else {
            double sum[3] = {0.0, 0.0, 0.0};
            for (int64_t j = ry.i0; j < ry.i1; j++) {
                const T *s = src + j * row_stride;
                double row[3] = {0.0, 0.0, 0.0};
                for (int64_t i = rx.i0; i < rx.i1; i++) {
                    const double wx = win_area_weight(rx, i);
                    FRS_UNROLL
                    for (int c = 0; c < 3; c++) row[c] = row[c] + wx * (double)s[c * bs + i];
                }
                const double wy = win_area_weight(ry, j);
                FRS_UNROLL
                for (int c = 0; c < 3; c++) sum[c] = sum[c] + wy * row[c];
            }
            FRS_UNROLL
            for (int c = 0; c < 3; c++)
                has = comp_channel(R, c, win_result<T>(win_area_value(sum[c], rx, ry)), rgba) && has;
        }
        return has ? rgba : R.nodata_rgba;
    }
};

// One lane's share of a work-group: lane tid of work-group (bx of gx, by of gy), render_rows<.., 4> of frs_render.h
// with a composite pixel in place of a colour.  P's destination strides are bytes, its source band stride elements.
// (Plain C++, so that a host program can run it lane by lane against a direct evaluation.)
template <int MODE, typename T, typename Mask>
FRS_HD inline void composite_group(const T *__restrict__ src, uint8_t *__restrict__ dst, const WinParams &P,
                                   const CompParams &R, const Mask &mask, int64_t bx, int64_t gx, int64_t by,
                                   int64_t gy, uint32_t tid) {
    const int64_t wb = P.dst_w * 4;  // bytes of a row
    const WinAxis ax = win_axis(P.x0, P.width, P.dst_w, P.src_w);
    const WinAxis ay = win_axis(P.y0, P.height, P.dst_h, P.src_h);
    for (int64_t r = by; r < P.dst_h; r += gy) {
        const CompRow<MODE, T, Mask> row(src, P, ay, r, mask);
        uint8_t *d = dst + r * P.dst_row_stride;
        const int64_t first = (int64_t)(reinterpret_cast<uintptr_t>(d) & 15);
        const int64_t cpr = (first + wb + 15) / 16;    // chunks the row touches
        const int shift = (int)((4 - first % 4) % 4);  // bytes of the chunk's first pixel that lie before it
        for (int64_t k = bx * kRenderBlock + tid; k < cpr; k += gx * kRenderBlock) {
            // chunk k holds the row's bytes [b0, b0 + 16); its first byte belongs to pixel p0
            const int64_t b0 = k * 16 - first;
            const int64_t p0 = (b0 - shift) / 4;       // (b0 - shift is a multiple of 4: exact, also below 0)
            uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};      // pixels p0 .. p0 + 4
            FRS_UNROLL
            for (int e = 0; e < 5; e++) {
                const int64_t x = p0 + e;
                if ((e < 4 || shift) && x >= 0 && x < P.dst_w) w[e] = row.pixel(ax, x, R);
            }
            RenderVec v;
            FRS_UNROLL
            for (int i = 0; i < 4; i++) v.w[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> (8 * shift));
            if (b0 >= 0 && b0 + 16 <= wb) {  // a whole chunk: d + b0 is 16-byte aligned
                *reinterpret_cast<RenderVec *>(d + b0) = v;
            } else {  // head or tail of the row
                FRS_UNROLL
                for (int j = 0; j < 16; j++) {
                    const int64_t b = b0 + j;
                    if (b >= 0 && b < wb) d[b] = (uint8_t)(v.w[j / 4] >> (8 * (j % 4)));
                }
            }
        }
    }
}

}  // namespace frs
