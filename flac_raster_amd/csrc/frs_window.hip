// frs_window.hip -- resample a rectangle of a band-planar raster onto a destination grid of any size
// (frs_resample_window*), by the arithmetic of frs_window_map.h (nearest, bilinear, or the area-weighted average) and,
// with a nodata value, of frs_nodata.h (nodata taps left out of an output, an output without a valid tap filled).
//
// There is no reference path: the reference reads whole tiles at the one resolution a file holds.  It is the last
// stage of streaming.read_window: the tiles a bounding box needs are decoded and placed into a device window
// (frs_decode_tiles_window_device), this kernel maps the box onto the W x H pixels the caller asked for, and only those
// cross to the host.
//
//   k_resample_window          grid (gx, gy, nbands), 256 threads.  Work-group (bx, by, band) owns destination rows
//   k_resample_window_nodata   by, by + gy, ... of the band and, of each, the 16-byte chunks bx * 256 + lane, striding
//                              gx * 256.  Row and band come from the block index alone: the row's taps, weights and
//                              validity (win_nearest / win_linear / win_area of the y axis), the source row pointers
//                              and the row's alignment are uniform over the work-group.
//
// Both kernels are one lane function, window_group, with a mask policy (frs_nodata.h): NoNodata, or Nodata<T> with the
// nodata value.  The policy reaches only WinRow::pixel (frs_window_row.h, shared with frs_render.hip), what one output
// is computed from its taps; the mapping, the chunks and the stores do not know of it.
//
// Store side, as in frs_place.hip and frs_pyramid.hip: a destination row is cut at the 16-byte boundaries of the
// DESTINATION; a chunk that lies wholly inside the row leaves as one aligned 16-byte store per lane, the first and last
// chunk of a row that starts or ends off a boundary go element by element.  Destination elements outside
// [height][width] are never written.  Load side: the taps of neighbouring outputs lie `step` source pixels apart, a
// number only known at run time, so each tap is one element-sized global load (a lane's 16 / ES outputs read
// neighbouring addresses, the lines stay in the vector L1 between them).  Every tap index comes out of frs_window_map.h
// inside [0, N): nothing is read outside the source's [H][W].  The average's tap loops are not capped (a 150x reduction
// reads 150 x 150 taps per output).  No LDS, no atomics, no init pass.
//
// One instantiation per (dtype, mode, policy): the conversion to double and the rounding differ per dtype, and there
// is no per-element switch on any of the three.
#include <algorithm>

#include "frs_internal.h"
#include "frs_nodata.h"
#include "frs_window_map.h"
#include "frs_window_row.h"

namespace frs {

constexpr int kWinBlock = 256;        // threads per work-group
constexpr int kWinMaxGridY = 32768;   // destination rows beyond this are strided over

// One lane's share of a work-group: lane tid of work-group (bx of gx, by of gy) of one band (src / dst are the band's
// origins).  (Plain C++, so that a host program can run it lane by lane against a direct evaluation.)
template <int MODE, typename T, typename Mask>
__host__ __device__ inline void window_group(const T *__restrict__ src, T *__restrict__ dst, const WinParams &P,
                                             const Mask &mask, int64_t bx, int64_t gx, int64_t by, int64_t gy,
                                             uint32_t tid) {
    constexpr int ES = (int)sizeof(T);
    constexpr int VE = 16 / ES;  // outputs per 16-byte chunk
    const int64_t w = P.dst_w;
    const WinAxis ax = win_axis(P.x0, P.width, P.dst_w, P.src_w);
    const WinAxis ay = win_axis(P.y0, P.height, P.dst_h, P.src_h);
    const T fill = win_result<T>(P.fill);
    for (int64_t r = by; r < P.dst_h; r += gy) {
        const WinRow<MODE, T, Mask> row(src, P, ay, r, mask);
        T *d = dst + r * P.dst_row_stride;
        const int64_t first = (int64_t)(reinterpret_cast<uintptr_t>(d) & 15) / ES;
        const int64_t cpr = (first + w + VE - 1) / VE;  // chunks the row touches
        for (int64_t k = bx * kWinBlock + tid; k < cpr; k += gx * kWinBlock) {
            // chunk k holds the row's outputs [pa, pb)
            const int64_t p0 = k * VE - first;
            const int64_t pa = p0 < 0 ? 0 : p0, pb = std::min<int64_t>(p0 + VE, w);
            T o[VE];
#pragma unroll
            for (int e = 0; e < VE; e++) {
                const int64_t x = p0 + e;
                o[e] = x >= pa && x < pb ? row.pixel(ax, x, fill) : fill;
            }
            if (pb - pa == VE) {  // a whole chunk: d + pa is 16-byte aligned
                uint4 v;
                __builtin_memcpy(&v, o, 16);
                *reinterpret_cast<uint4 *>(d + pa) = v;
            } else {  // head or tail of the row
#pragma unroll
                for (int e = 0; e < VE; e++) {
                    const int64_t x = p0 + e;
                    if (x >= pa && x < pb) d[x] = o[e];
                }
            }
        }
    }
}

// The two kernels differ in their arguments alone.
template <int MODE, typename T>
__global__ void __launch_bounds__(kWinBlock) k_resample_window(const T *__restrict__ src, T *__restrict__ dst,
                                                               WinParams P) {
    const int64_t band = blockIdx.z;
    window_group<MODE, T>(src + band * P.src_band_stride, dst + band * P.dst_band_stride, P, NoNodata{}, blockIdx.x,
                          gridDim.x, blockIdx.y, gridDim.y, threadIdx.x);
}

template <int MODE, typename T>
__global__ void __launch_bounds__(kWinBlock) k_resample_window_nodata(const T *__restrict__ src, T *__restrict__ dst,
                                                                      WinParams P, T nd) {
    const int64_t band = blockIdx.z;
    window_group<MODE, T>(src + band * P.src_band_stride, dst + band * P.dst_band_stride, P, Nodata<T>{nd},
                          blockIdx.x, gridDim.x, blockIdx.y, gridDim.y, threadIdx.x);
}

// nodata: null without one
template <int MODE, typename T>
static void launch_window_mode(hipStream_t st, dim3 grid, const void *src, void *dst, const WinParams &P,
                               const double *nodata) {
    const T *s = static_cast<const T *>(src);
    T *d = static_cast<T *>(dst);
    if (nodata) k_resample_window_nodata<MODE, T><<<grid, kWinBlock, 0, st>>>(s, d, P, nd_cast<T>(*nodata));
    else k_resample_window<MODE, T><<<grid, kWinBlock, 0, st>>>(s, d, P);
}

template <typename T>
static void launch_window(hipStream_t st, dim3 grid, int32_t mode, const void *src, void *dst, const WinParams &P,
                          const double *nodata) {
    if (mode == FRS_RESAMPLE_NEAREST) launch_window_mode<kWindowNearest, T>(st, grid, src, dst, P, nodata);
    else if (mode == FRS_RESAMPLE_BILINEAR) launch_window_mode<kWindowBilinear, T>(st, grid, src, dst, P, nodata);
    else launch_window_mode<kWindowAverage, T>(st, grid, src, dst, P, nodata);
}

// The arguments are already validated (window_entry below), the nodata value for the dtype as well (null: none).
// Synchronous on the context stream.
static int window_job(frs_ctx *ctx, const frs_raster_desc *s, const void *src_dev, const frs_raster_desc *d,
                      void *dst_dev, const frs_window_map *map, int32_t mode, const double *nodata) {
    const int es = dtype_size(d->dtype);
    WinParams P;
    P.src_h = s->height, P.src_w = s->width, P.dst_h = d->height, P.dst_w = d->width;
    P.src_row_stride = s->row_stride, P.src_band_stride = s->band_stride;
    P.dst_row_stride = d->row_stride, P.dst_band_stride = d->band_stride;
    P.x0 = map->x0, P.y0 = map->y0, P.width = map->width, P.height = map->height, P.fill = map->fill;
    // chunks of the longest row (one more when it starts off a boundary); whole steps only, the rest is strided over
    const int64_t cpr = (d->width + 16 / es - 1) / (16 / es) + 1;
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(cpr / kWinBlock, 65535));
    const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(d->height, kWinMaxGridY), (unsigned)d->nbands);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "resample", &ev);
    switch (d->dtype) {
    case FRS_DT_U8: launch_window<uint8_t>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    case FRS_DT_U16: launch_window<uint16_t>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    case FRS_DT_I16: launch_window<int16_t>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    case FRS_DT_I32: launch_window<int32_t>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    case FRS_DT_U32: launch_window<uint32_t>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    case FRS_DT_F32: launch_window<float>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    default: launch_window<double>(st, grid, mode, src_dev, dst_dev, P, nodata); break;
    }
    prof_end(ctx, "resample", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FRS_OK;
}

// elements from a raster's origin to the end of its last row, or -1 when that does not fit 63 bits (with room for the
// element size)
int64_t window_extent(const frs_raster_desc *d) {
    int64_t x, y;
    if (__builtin_mul_overflow((int64_t)d->nbands - 1, d->nbands > 1 ? d->band_stride : 0, &x) ||
        __builtin_mul_overflow(d->height - 1, d->row_stride, &y) || __builtin_add_overflow(x, y, &x) ||
        __builtin_add_overflow(x, d->width, &x) || x > (INT64_MAX >> 4))
        return -1;
    return x;
}

// argument checks of frs_resample_window*, before anything is sized, copied or launched (the descriptor's and the
// mapping's are frs_render_window*'s as well: frs_internal.h)
int check_window_desc(frs_ctx *ctx, const frs_raster_desc *d) {
    if (!d) { ctx->err = "null desc"; return FRS_E_ARG; }
    if (d->height < 1 || d->width < 1) { ctx->err = "resample: height and width must be >= 1"; return FRS_E_ARG; }
    if (d->row_stride < d->width) { ctx->err = "row_stride < width"; return FRS_E_ARG; }
    if (d->nbands < 1 || d->nbands > kMaxChannels) { ctx->err = "nbands must be 1..8"; return FRS_E_ARG; }
    if (dtype_size(d->dtype) == 0) { ctx->err = "bad dtype"; return FRS_E_ARG; }
    if (window_extent(d) < 0) { ctx->err = "resample: raster extent overflows"; return FRS_E_ARG; }
    if (d->nbands > 1 && d->band_stride < (d->height - 1) * d->row_stride + d->width) {
        ctx->err = "band_stride too small";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

static bool window_coord_ok(double v) { return v == v && v > -4503599627370496.0 && v < 4503599627370496.0; }  // 2^52

// mode and rectangle, and the fill unless it is ignored
int check_window_map(frs_ctx *ctx, const frs_window_map *map, int32_t mode, bool with_fill) {
    if (mode != FRS_RESAMPLE_NEAREST && mode != FRS_RESAMPLE_AVERAGE && mode != FRS_RESAMPLE_BILINEAR) {
        ctx->err = "resample: bad mode";
        return FRS_E_ARG;
    }
    if (!map) { ctx->err = "null map"; return FRS_E_ARG; }
    // (a non-finite value fails window_coord_ok: NaN compares false, +-inf is out of range)
    if (!window_coord_ok(map->x0) || !window_coord_ok(map->y0) || !window_coord_ok(map->width) ||
        !window_coord_ok(map->height) || !window_coord_ok(map->x0 + map->width) ||
        !window_coord_ok(map->y0 + map->height)) {
        ctx->err = "resample: the rectangle must be finite, with coordinates below 2^52 in magnitude";
        return FRS_E_ARG;
    }
    if (with_fill && !(map->fill - map->fill == 0.0)) { ctx->err = "resample: fill must be finite"; return FRS_E_ARG; }
    if (!(map->width > 0.0) || !(map->height > 0.0)) {
        ctx->err = "resample: the rectangle's width and height must be > 0";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

static int check_window_args(frs_ctx *ctx, const frs_raster_desc *src, const frs_raster_desc *dst,
                             const frs_window_map *map, int32_t mode) {
    if (int rc = check_window_desc(ctx, src)) return rc;
    if (int rc = check_window_desc(ctx, dst)) return rc;
    if (src->dtype != dst->dtype || src->nbands != dst->nbands) {
        ctx->err = "resample: source and destination differ in dtype or nbands";
        return FRS_E_ARG;
    }
    return check_window_map(ctx, map, mode, true);
}

// frs_resample_window_nodata*: the same checks, but a float raster may be filled with NaN, and the nodata value must be
// one the dtype holds
static int check_window_nodata_args(frs_ctx *ctx, const frs_raster_desc *src, const frs_raster_desc *dst,
                                    const frs_window_map *map, int32_t mode, double nodata) {
    frs_window_map m;
    const bool nan_fill =
        map && dst && map->fill != map->fill && (dst->dtype == FRS_DT_F32 || dst->dtype == FRS_DT_F64);
    if (nan_fill) m = *map, m.fill = 0.0;
    if (int rc = check_window_args(ctx, src, dst, nan_fill ? &m : map, mode)) return rc;
    if (!nodata_ok(dst->dtype, nodata)) {
        ctx->err = "resample: nodata must be an integer inside the dtype's range";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

static size_t window_bytes(const frs_raster_desc *d) { return (size_t)window_extent(d) * (size_t)dtype_size(d->dtype); }

// null, misaligned or overlapping rasters
static int check_window_pointers(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst,
                                 const void *dp) {
    const uintptr_t es = (uintptr_t)dtype_size(dst->dtype);
    const uintptr_t a = reinterpret_cast<uintptr_t>(sp), b = reinterpret_cast<uintptr_t>(dp);
    if (!sp || !dp || a % es || b % es) {
        ctx->err = "resample: null or element-misaligned pointer";
        return FRS_E_ARG;
    }
    if (a < b + window_bytes(dst) && b < a + window_bytes(src)) {
        ctx->err = "resample: source and destination overlap";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

// frs_resample_window*: every check, then the job between the device rasters `sp` / `dp`, or (host) between staged
// copies of the host rasters they point at.  nodata: null without one.
static int window_entry(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst, void *dp,
                        const frs_window_map *map, int32_t mode, const double *nodata, bool host) {
    if (!ctx) return FRS_E_ARG;
    if (int rc = check_unsynced(ctx)) return rc;
    if (int rc = nodata ? check_window_nodata_args(ctx, src, dst, map, mode, *nodata)
                        : check_window_args(ctx, src, dst, map, mode))
        return rc;
    if (int rc = check_window_pointers(ctx, src, sp, dst, dp)) return rc;
    FRS_HIP(hipSetDevice(ctx->device));
    if (!host) return window_job(ctx, src, sp, dst, dp, map, mode, nodata);
    return run_staged(ctx, sp, window_bytes(src), dp, window_bytes(dst), [&](const void *src_dev, void *dst_dev) {
        return window_job(ctx, src, src_dev, dst, dst_dev, map, mode, nodata);
    });
}

}  // namespace frs

extern "C" {

int frs_resample_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                               const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map, int32_t mode) {
    return frs::window_entry(ctx, src, src_dev, dst, dst_dev, map, mode, nullptr, false);
}

int frs_resample_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host, const frs_raster_desc *dst,
                        void *dst_host, const frs_window_map *map, int32_t mode) {
    return frs::window_entry(ctx, src, src_host, dst, dst_host, map, mode, nullptr, true);
}

int frs_resample_window_nodata_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                      const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map,
                                      int32_t mode, double nodata) {
    return frs::window_entry(ctx, src, src_dev, dst, dst_dev, map, mode, &nodata, false);
}

int frs_resample_window_nodata(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host,
                               const frs_raster_desc *dst, void *dst_host, const frs_window_map *map, int32_t mode,
                               double nodata) {
    return frs::window_entry(ctx, src, src_host, dst, dst_host, map, mode, &nodata, true);
}

}  // extern "C"
