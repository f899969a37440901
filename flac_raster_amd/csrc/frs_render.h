// frs_render.h -- the arithmetic and the lane function of the 8-bit render of a windowed read (frs_render_window*),
// written once for the host and the device.  Includes nothing from HIP, only the headers whose arithmetic it uses: a
// plain C++ compiler builds it (tests/test_render_host.py compares the quantiser and render_group, run lane by lane,
// with the numpy restatement in tests/render_ref.py, bit for bit), hipcc builds the same text as __host__ __device__.
// Needs -ffp-contract=off like the rest of the library: every operator below is one IEEE fp64 operation.  User:
// k_render_window in frs_render.hip, which only places the LUT and calls render_group.
//
// The definition is the project's own.  One output pixel comes from one resampled value v in the source dtype T and a
// flag has_data.
//
// v and has_data.  v is what frs_resample_window* (the _nodata form with a nodata value) writes for the pixel: it
// comes from WinRow::output (frs_window_row.h), the code WinRow::pixel is expressed through.  has_data is false exactly
// where that kernel writes `fill` (an axis is invalid, masked nearest hit a nodata tap, a masked output has no valid
// weight) and, for float rasters, where v is NaN.  +-inf are data.
//
// Quantise.  scale = (double)n / (hi - lo), computed once; lo and hi finite, hi > lo, n the LUT length (1 .. 4096).
// x = (double)v < lo gives index 0, x > hi gives n - 1, otherwise min((int64)floor((x - lo) * scale), n - 1).  This is
// the bin rule of frs_stats.h (hist_range, hist_bin: the same functions), with `below` and `above` clamped to the ends.
//
// Colour.  rgba = lut[index], lut holding n packed R, G, B, A bytes (one little-endian 32-bit word per entry:
// R | G << 8 | B << 16 | A << 24).  A pixel without data takes nodata_rgba, packed the same way.
//
// Channels.  C in {1, 2, 4}, pixel-interleaved uint8 [H][W][C] with a row stride in bytes: R; R, A; R, G, B, A.
//
// The lane function.  render_group has window_group's shape (frs_window.hip): work-group (bx of gx, by of gy) owns
// destination rows by, by + gy, ... and, of each, the 16-byte chunks bx * 256 + lane, striding gx * 256.  A row of
// w * C bytes is cut at the 16-byte boundaries of the destination.  A chunk wholly inside the row leaves as one aligned
// 16-byte store; the chunks the row begins or ends in go byte by byte, only the bytes inside the row.  When the row
// starts on a multiple of C a chunk holds 16 / C whole pixels.  When it does not (a destination whose origin or row
// stride is not a multiple of C), the chunk's first and last pixel straddle its boundaries: the lane computes 16 / C + 1
// pixels and shifts their bytes into place, and the lane of the neighbouring chunk computes the straddling pixel again.
#pragma once
#include <stdint.h>

#include "frs_stats.h"
#include "frs_window_row.h"

// (a plain host compiler does not know the pragma)
#ifdef __clang__
#define FRS_UNROLL _Pragma("unroll")
#else
#define FRS_UNROLL
#endif

namespace frs {

constexpr int kRenderBlock = 256;       // threads per work-group
constexpr int kRenderMaxGridY = 32768;  // destination rows beyond this are strided over
constexpr int kRenderMaxLut = 4096;     // LUT entries at most

// the LUT index of a value that is data (x is never NaN)
FRS_HD inline int32_t render_index(const HistRange &r, double x) {
    const int32_t b = hist_bin(r, x);
    return b == kHistBelow ? 0 : b == kHistAbove ? r.nbins - 1 : b;
}

struct RenderParams {
    HistRange range;       // lo, hi, scale and n
    const uint32_t *lut;   // n packed entries
    uint32_t nodata_rgba;
    int32_t channels;
};

// The result policy of WinRow::output (frs_window_row.h) that gives the packed colour of an output: has_data is
// "hit, and not NaN".
template <typename T> struct RenderOut {
    using type = uint32_t;
    const RenderParams &R;
    FRS_HD uint32_t hit(T v) const {
        if constexpr (NdFloat<T>::value) {
            if (v != v) return R.nodata_rgba;
        }
        return R.lut[render_index(R.range, (double)v)];
    }
    FRS_HD uint32_t miss() const { return R.nodata_rgba; }
};

// the C bytes of a pixel, in the low bits of a word: R; R, A; R, G, B, A
template <int C> FRS_HD inline uint32_t render_channels(uint32_t rgba) {
    if constexpr (C == 1) return rgba & 0xffu;
    else if constexpr (C == 2) return (rgba & 0xffu) | ((rgba >> 24) << 8);
    else return rgba;
}

// one aligned 16-byte chunk of the destination
struct alignas(16) RenderVec {
    uint32_t w[4];
};

// One lane's share of the rows of a work-group, for C channels.  P's destination strides are bytes.
template <int MODE, typename T, typename Mask, int C>
FRS_HD inline void render_rows(const T *__restrict__ src, uint8_t *__restrict__ dst, const WinParams &P,
                               const RenderParams &R, const Mask &mask, int64_t bx, int64_t gx, int64_t by, int64_t gy,
                               uint32_t tid) {
    constexpr int VE = 16 / C;            // whole pixels per chunk
    constexpr int PW = 4 / C;             // pixels per 32-bit word
    const int64_t wb = P.dst_w * C;       // bytes of a row
    const WinAxis ax = win_axis(P.x0, P.width, P.dst_w, P.src_w);
    const WinAxis ay = win_axis(P.y0, P.height, P.dst_h, P.src_h);
    for (int64_t r = by; r < P.dst_h; r += gy) {
        const WinRow<MODE, T, Mask> row(src, P, ay, r, mask);
        uint8_t *d = dst + r * P.dst_row_stride;
        const int64_t first = (int64_t)(reinterpret_cast<uintptr_t>(d) & 15);
        const int64_t cpr = (first + wb + 15) / 16;           // chunks the row touches
        const int shift = (int)((C - first % C) % C);         // bytes of the chunk's first pixel that lie before it
        for (int64_t k = bx * kRenderBlock + tid; k < cpr; k += gx * kRenderBlock) {
            // chunk k holds the row's bytes [b0, b0 + 16); its first byte belongs to pixel p0
            const int64_t b0 = k * 16 - first;
            const int64_t p0 = (b0 - shift) / C;              // (b0 - shift is a multiple of C: exact, also below 0)
            uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};             // the bytes of pixels p0 .. p0 + VE
            FRS_UNROLL
            for (int e = 0; e < VE + 1; e++) {
                const int64_t x = p0 + e;
                if ((e < VE || shift) && x >= 0 && x < P.dst_w)
                    w[e / PW] |= render_channels<C>(row.output(ax, x, RenderOut<T>{R})) << (8 * C * (e % PW) & 31);
            }
            RenderVec v;
            FRS_UNROLL
            for (int i = 0; i < 4; i++)
                v.w[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> (8 * shift));
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

// One lane's share of a work-group: lane tid of work-group (bx of gx, by of gy).  `mask` is NoNodata or Nodata<T>.
// (Plain C++, so that a host program can run it lane by lane against a direct evaluation.)
template <int MODE, typename T, typename Mask>
FRS_HD inline void render_group(const T *__restrict__ src, uint8_t *__restrict__ dst, const WinParams &P,
                                const RenderParams &R, const Mask &mask, int64_t bx, int64_t gx, int64_t by, int64_t gy,
                                uint32_t tid) {
    if (R.channels == 1) render_rows<MODE, T, Mask, 1>(src, dst, P, R, mask, bx, gx, by, gy, tid);
    else if (R.channels == 2) render_rows<MODE, T, Mask, 2>(src, dst, P, R, mask, bx, gx, by, gy, tid);
    else render_rows<MODE, T, Mask, 4>(src, dst, P, R, mask, bx, gx, by, gy, tid);
}

}  // namespace frs
