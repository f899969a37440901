// frs_shade.h -- the arithmetic and the lane functions of the hillshaded render of a windowed read
// (frs_render_shaded_window*), written once for the host and the device.  Includes nothing from HIP, only the headers
// whose arithmetic it uses: a plain C++ compiler builds it (tests/test_shade_host.py compares shade_level and the two
// lane functions, run lane by lane over every work-group, with the numpy restatement in tests/shade_ref.py, bit for
// bit), hipcc builds the same text as __host__ __device__.  Needs -ffp-contract=off like the rest of the library: every
// operator below is one IEEE fp64 operation.  User: k_render_shaded_window in frs_shade.hip, which places the tables
// and the tile in LDS and calls shade_fill, a barrier, shade_emit.
//
// The definition is the project's own.  The gradient is Horn's, as in gdaldem hillshade; no parity with GDAL is claimed.
//
// Samples.  For an output pixel (x, y) the nine samples z[dy][dx], dx, dy in {-1, 0, +1}, are what WinRow<MODE, T,
// Mask>::sample (frs_window_row.h) gives at output positions (x + dx, y + dy) under the call's own WinAxis.  Positions
// -1 and dst_w / dst_h are included: win_centre, win_lo and win_hi are plain arithmetic in j, so the apron comes from
// the raster and not from replication.  Each sample is converted to double.  A sample has no data where `has` is false
// or the value is NaN; +-inf are data.  A centre without data gives nodata_rgba, exactly as in frs_render_window*.  A
// neighbour without data is replaced by the centre's value.
//
// Gradient.  Rows grow southwards; 2z is z + z, every sum left to right as written:
//   gx = (z[-1][+1] + (z[0][+1] + z[0][+1]) + z[+1][+1]) - (z[-1][-1] + (z[0][-1] + z[0][-1]) + z[+1][-1])
//   gy = (z[+1][-1] + (z[+1][0] + z[+1][0]) + z[+1][+1]) - (z[-1][-1] + (z[-1][0] + z[-1][0]) + z[-1][+1])
//   p = gx * kx,  q = gy * ky
// kx = z_factor / (8 cell_x) and ky = z_factor / (8 cell_y) come from the caller, cell_x and cell_y being the ground
// size of an OUTPUT pixel.
//
// Shade.  (lx, ly, lz) is the unit vector towards the light: lx = sin A cos h, ly = cos A cos h, lz = sin h, A the
// azimuth clockwise from north, h the altitude; the trigonometry is the caller's.
//   num = (lz - p * lx) + q * ly
//   den = sqrt((1.0 + p * p) + q * q)          sqrt correctly rounded
//   s = num / den
//   k = 0 when s > 0 is false (NaN included), otherwise min((int)floor(s * 256.0), 255)
// With the light in the north-west a slope that descends westwards (p > 0) and one that descends northwards (q > 0) are
// both brighter than flat ground.
//
// Colour.  rgba = lut[render_index(range, (double)v)] from the centre value v: the plain render's colour.  m = table[k],
// a 256-byte table from the caller (strength and ambient light live in it, as gamma lives in the LUT).  R, G and B each
// become (c * m + 127) / 255 in integer arithmetic; A is untouched.  C = 1 stores the shaded R, C = 2 the shaded R and
// A, C = 4 R, G, B, A.  With m = 255 the result is the plain render's pixel.
//
// The lane functions.  A work-group of 256 lanes owns a tile of the destination: kShadeRows rows and, of each, the 16
// aligned 16-byte chunks tx * 16 .. tx * 16 + 15 (the chunks are cut at the 16-byte boundaries of the destination, as in
// frs_render.h).  shade_tile gives the tile's rows [r0, r1) and the pixel columns [xa, xb) its chunks touch (the same
// on every lane).  Phase 1, shade_fill: the lanes compute the samples of rows r0 - 1 .. r1 and columns xa - 1 .. xb
// through WinRow::sample and store them as doubles, NaN coding "no data" (an integer never converts to NaN, a float
// NaN is no data anyway).  Phase 2, shade_emit: lane tid owns chunk tid % 16 of row r0 + tid / 16, reads its 3 x 3
// neighbourhoods from the tile, shades, colours and stores under frs_render_window*'s contract: one aligned 16-byte
// store for a chunk wholly inside the row, bytes for the row's head and tail, no byte outside [H][W * C].  A row that
// does not start on a multiple of C shifts its pixels' bytes into place as render_rows does.
#pragma once
#include <stdint.h>

#include "frs_render.h"
#include "frs_window_row.h"

namespace frs {

constexpr int kShadeBlock = kRenderBlock;  // threads per work-group
constexpr int kShadeRows = 16;             // destination rows of a tile
constexpr int kShadeChunks = 16;           // 16-byte chunks of a tile's row: kShadeRows * kShadeChunks lanes
constexpr int kShadeMaxGrid = 65535;       // tiles beyond this, on either axis, are strided over

struct ShadeParams {
    double lx, ly, lz, kx, ky;
    const uint8_t *table;  // 256 entries
};

FRS_HD inline double shade_sqrt(double x) { return __builtin_sqrt(x); }

// the shade level 0 .. 255 of a 3 x 3 neighbourhood z[dy + 1][dx + 1] whose nine values are all data
FRS_HD inline int shade_level(const double z[3][3], const ShadeParams &S) {
    const double gx = (z[0][2] + (z[1][2] + z[1][2]) + z[2][2]) - (z[0][0] + (z[1][0] + z[1][0]) + z[2][0]);
    const double gy = (z[2][0] + (z[2][1] + z[2][1]) + z[2][2]) - (z[0][0] + (z[0][1] + z[0][1]) + z[0][2]);
    const double p = gx * S.kx;
    const double q = gy * S.ky;
    const double num = (S.lz - p * S.lx) + q * S.ly;
    const double den = shade_sqrt((1.0 + p * p) + q * q);
    const double s = num / den;
    if (!(s > 0.0)) return 0;
    const double f = __builtin_floor(s * 256.0);
    return f >= 255.0 ? 255 : (int)f;
}

// R, G and B of a packed colour scaled by m / 255, rounded; A as it is
FRS_HD inline uint32_t shade_pixel(uint32_t rgba, uint32_t m) {
    const uint32_t r = ((rgba & 0xffu) * m + 127u) / 255u;
    const uint32_t g = (((rgba >> 8) & 0xffu) * m + 127u) / 255u;
    const uint32_t b = (((rgba >> 16) & 0xffu) * m + 127u) / 255u;
    return r | g << 8 | b << 16 | (rgba & 0xff000000u);
}

// columns of the tile's sample array, apron included.  A row's chunk tx * 16 begins at most 15 bytes and one straddling
// pixel before the tile's first whole pixel, and its last chunk may end in one more straddling pixel:
// 256 / C + ceil((15 + C - 1) / C) + 1 columns at most, and two for the apron.
template <int C> struct ShadeShape {
    static constexpr int TW = kShadeChunks * 16 / C;      // pixels of a tile's row when rows start on a chunk boundary
    static constexpr int LW = TW + 16 / C + 4;             // the sample array's row pitch (276, 140, 72)
    static constexpr int LH = kShadeRows + 2;
    static constexpr int samples = LW * LH;                // doubles: 39744, 20160 and 10368 bytes
};

// first byte offset of destination row r within its 16-byte chunk
FRS_HD inline int64_t shade_first(const uint8_t *dst, const WinParams &P, int64_t r) {
    return (int64_t)(reinterpret_cast<uintptr_t>(dst + r * P.dst_row_stride) & 15);
}

// tiles per axis of a destination (the longest row may touch one chunk more than its bytes fill)
template <int C> FRS_HD inline int64_t shade_tiles_x(const WinParams &P) {
    return ((P.dst_w * C + 15) / 16 + 1 + kShadeChunks - 1) / kShadeChunks;
}
FRS_HD inline int64_t shade_tiles_y(const WinParams &P) { return (P.dst_h + kShadeRows - 1) / kShadeRows; }

// tile (tx, ty): destination rows [r0, r1) and the pixel columns [xa, xb) their chunks tx * 16 .. tx * 16 + 15 touch,
// clipped to the destination (xb <= xa: none)
struct ShadeTile {
    int64_t tx, r0, r1, xa, xb;
};
template <int C> FRS_HD inline ShadeTile shade_tile(const uint8_t *dst, const WinParams &P, int64_t tx, int64_t ty) {
    ShadeTile t;
    t.tx = tx, t.r0 = ty * kShadeRows;
    t.r1 = t.r0 + kShadeRows < P.dst_h ? t.r0 + kShadeRows : P.dst_h;
    int64_t xa = P.dst_w, xb = 0;
    for (int64_t r = t.r0; r < t.r1; r++) {
        const int64_t first = shade_first(dst, P, r);
        const int64_t shift = (C - first % C) % C;
        const int64_t lo = (tx * kShadeChunks * 16 - first - shift) / C;  // (exact, also below 0)
        const int64_t hi = lo + ShadeShape<C>::TW + (shift ? 1 : 0);
        xa = lo < xa ? lo : xa, xb = hi > xb ? hi : xb;
    }
    t.xa = xa < 0 ? 0 : xa, t.xb = xb > P.dst_w ? P.dst_w : xb;
    return t;
}

FRS_HD inline double shade_nan() { return __builtin_nan(""); }

// Phase 1: lane tid's share of the tile's samples, rows t.r0 - 1 .. t.r1 and columns t.xa - 1 .. t.xb, into
// tile[row * LW + column]
template <int MODE, typename T, typename Mask, int C>
FRS_HD inline void shade_fill(const T *__restrict__ src, const WinParams &P, const Mask &mask, const ShadeTile &t,
                              double *__restrict__ tile, uint32_t tid) {
    if (t.xb <= t.xa) return;
    const WinAxis ax = win_axis(P.x0, P.width, P.dst_w, P.src_w);
    const WinAxis ay = win_axis(P.y0, P.height, P.dst_h, P.src_h);
    const uint32_t cols = (uint32_t)(t.xb - t.xa + 2), rows = (uint32_t)(t.r1 - t.r0 + 2);
    for (uint32_t i = tid; i < rows * cols; i += (uint32_t)kShadeBlock) {
        const uint32_t ry = i / cols, cx = i - ry * cols;
        const WinRow<MODE, T, Mask> row(src, P, ay, t.r0 - 1 + (int64_t)ry, mask);
        const WinSample<T> s = row.sample(ax, t.xa - 1 + (int64_t)cx);
        tile[ry * (uint32_t)ShadeShape<C>::LW + cx] = s.has ? (double)s.v : shade_nan();
    }
}

// the packed colour of the pixel whose 3 x 3 samples are the columns a, b, c (west, centre, east; rows north to south)
FRS_HD inline uint32_t shade_colour(const double a[3], const double b[3], const double c[3], const RenderParams &R,
                                    const ShadeParams &S) {
    const double v = b[1];
    if (v != v) return R.nodata_rgba;
    double z[3][3];
    FRS_UNROLL
    for (int j = 0; j < 3; j++) {
        z[j][0] = a[j] != a[j] ? v : a[j];
        z[j][1] = b[j] != b[j] ? v : b[j];
        z[j][2] = c[j] != c[j] ? v : c[j];
    }
    return shade_pixel(R.lut[render_index(R.range, v)], S.table[shade_level(z, S)]);
}

// Phase 2: lane tid's chunk of the tile, from the samples of phase 1
template <int C>
FRS_HD inline void shade_emit(uint8_t *__restrict__ dst, const WinParams &P, const RenderParams &R,
                              const ShadeParams &S, const ShadeTile &t, const double *__restrict__ tile,
                              uint32_t tid) {
    constexpr int VE = 16 / C;            // whole pixels per chunk
    constexpr int PW = 4 / C;             // pixels per 32-bit word
    constexpr int LW = ShadeShape<C>::LW;
    const int64_t r = t.r0 + (int64_t)(tid / (uint32_t)kShadeChunks);
    if (r >= t.r1) return;
    const int64_t wb = P.dst_w * C;       // bytes of a row
    uint8_t *d = dst + r * P.dst_row_stride;
    const int64_t first = shade_first(dst, P, r);
    const int64_t k = t.tx * kShadeChunks + (int64_t)(tid % (uint32_t)kShadeChunks);
    if (k >= (first + wb + 15) / 16) return;  // past the chunks the row touches
    const int shift = (int)((C - first % C) % C);  // bytes of the chunk's first pixel that lie before it
    const int64_t b0 = k * 16 - first;             // the chunk holds the row's bytes [b0, b0 + 16)
    const int64_t p0 = (b0 - shift) / C;           // its first byte belongs to pixel p0 (exact, also below 0)
    // the samples of pixel x: rows (r - r0) .. (r - r0) + 2 of the array, columns (x - xa) .. (x - xa) + 2
    const double *base = tile + (r - t.r0) * LW;
    const auto column = [&](int64_t x, double col[3]) {  // the three samples of output column x
        const bool in = x >= t.xa - 1 && x <= t.xb;
        const int64_t cx = in ? x - (t.xa - 1) : 0;
        FRS_UNROLL
        for (int j = 0; j < 3; j++) col[j] = in ? base[j * LW + cx] : 0.0;
    };
    double a[3], b[3], c[3];
    column(p0 - 1, a);
    column(p0, b);
    uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};  // the bytes of pixels p0 .. p0 + VE
    FRS_UNROLL
    for (int e = 0; e < VE + 1; e++) {
        const int64_t x = p0 + e;
        if (e < VE || shift) {
            column(x + 1, c);
            if (x >= 0 && x < P.dst_w)
                w[e / PW] |= render_channels<C>(shade_colour(a, b, c, R, S)) << (8 * C * (e % PW) & 31);
            FRS_UNROLL
            for (int j = 0; j < 3; j++) a[j] = b[j], b[j] = c[j];
        }
    }
    RenderVec v;
    FRS_UNROLL
    for (int i = 0; i < 4; i++) v.w[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> (8 * shift));
    if (b0 >= 0 && b0 + 16 <= wb) {  // a whole chunk: d + b0 is 16-byte aligned
        *reinterpret_cast<RenderVec *>(d + b0) = v;
    } else {  // head or tail of the row
        FRS_UNROLL
        for (int j = 0; j < 16; j++) {
            const int64_t bb = b0 + j;
            if (bb >= 0 && bb < wb) d[bb] = (uint8_t)(v.w[j / 4] >> (8 * (j % 4)));
        }
    }
}

}  // namespace frs
