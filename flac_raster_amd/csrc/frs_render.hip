// frs_render.hip -- a rectangle of one band as stretched 8-bit colour (frs_render_window*): the windowed resample of
// frs_window.hip fused with a quantiser, a colour look-up table and an alpha for "no data" (csrc/frs_render.h holds the
// arithmetic and the lane function, render_group; csrc/frs_window_row.h the output of a resample from its taps, shared
// with frs_window.hip).  It is the last stage of streaming.render_window: the decoded device window leaves the device
// as the W x H x C bytes a viewer shows.
//
//   k_render_window   grid (gx, gy), 256 threads: k_resample_window's.  Work-group (bx, by) owns destination rows by,
//                     by + gy, ... and, of each, the 16-byte chunks bx * 256 + lane, striding gx * 256.
//
// One kernel, templated on the mode, the dtype, the mask policy and where the LUT is read from.  Store side as in
// frs_window.hip: aligned 16-byte stores for the chunks wholly inside a row, bytes for its head and tail, nothing
// outside [H][W * C].  No atomics, no init pass.
//
// Where the LUT lives.  The grid gives most work-groups ONE row segment of 256 chunks (4 KB of output): a table loaded
// into LDS per work-group must be paid for by those.  A table of n <= 256 entries is one dword per lane, one coalesced
// load (every work-group reads the same 1 KB: it stays in L2) and one barrier: it goes to LDS, where a wave's 64
// scattered look-ups cost 2 LDS cycles and no vector-memory instruction.  A longer table (up to 16 KB, 16 loads per
// lane per work-group, four times the bytes the work-group stores for C = 4) stays in global memory and is gathered
// through the read-only path: it is L2-resident after the first touch and half of the vector L1's 32 KB at most.
// FRS_RENDER_LUT=global in the environment reads a short table from global memory as well (measurements only).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "frs_internal.h"
#include "frs_render.h"

namespace frs {

constexpr int kRenderLdsLut = kRenderBlock;  // entries up to which the table is copied to LDS: one per lane

template <int MODE, typename T, typename Mask, bool LDS>
__global__ void __launch_bounds__(kRenderBlock) k_render_window(const T *__restrict__ src, uint8_t *__restrict__ dst,
                                                                WinParams P, RenderParams R, Mask mask) {
    if constexpr (LDS) {
        __shared__ uint32_t s_lut[kRenderLdsLut];
        if ((int)threadIdx.x < R.range.nbins) s_lut[threadIdx.x] = R.lut[threadIdx.x];
        __syncthreads();
        R.lut = s_lut;
    }
    render_group<MODE, T>(src, dst, P, R, mask, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y, threadIdx.x);
}

template <int MODE, typename T, typename Mask>
static void launch_render_mask(hipStream_t st, dim3 grid, const T *s, uint8_t *d, const WinParams &P,
                               const RenderParams &R, const Mask &mask, bool lds) {
    if (lds) k_render_window<MODE, T, Mask, true><<<grid, kRenderBlock, 0, st>>>(s, d, P, R, mask);
    else k_render_window<MODE, T, Mask, false><<<grid, kRenderBlock, 0, st>>>(s, d, P, R, mask);
}

// nodata: null without one
template <int MODE, typename T>
static void launch_render_mode(hipStream_t st, dim3 grid, const T *s, uint8_t *d, const WinParams &P,
                               const RenderParams &R, const double *nodata, bool lds) {
    if (nodata) launch_render_mask<MODE, T>(st, grid, s, d, P, R, Nodata<T>{nd_cast<T>(*nodata)}, lds);
    else launch_render_mask<MODE, T>(st, grid, s, d, P, R, NoNodata{}, lds);
}

template <typename T>
static void launch_render(hipStream_t st, dim3 grid, int32_t mode, const void *src, void *dst, const WinParams &P,
                          const RenderParams &R, const double *nodata, bool lds) {
    const T *s = static_cast<const T *>(src);
    uint8_t *d = static_cast<uint8_t *>(dst);
    if (mode == FRS_RESAMPLE_NEAREST) launch_render_mode<kWindowNearest, T>(st, grid, s, d, P, R, nodata, lds);
    else if (mode == FRS_RESAMPLE_BILINEAR) launch_render_mode<kWindowBilinear, T>(st, grid, s, d, P, R, nodata, lds);
    else launch_render_mode<kWindowAverage, T>(st, grid, s, d, P, R, nodata, lds);
}

// The arguments are already validated (render_entry below).  Synchronous on the context stream.
static int render_job(frs_ctx *ctx, const frs_raster_desc *s, const void *src_dev, const frs_raster_desc *d,
                      void *dst_dev, const frs_window_map *map, int32_t mode, const double *nodata,
                      const frs_render_params *rp) {
    const int C = rp->channels;
    WinParams P;
    P.src_h = s->height, P.src_w = s->width, P.dst_h = d->height, P.dst_w = d->width;
    P.src_row_stride = s->row_stride, P.src_band_stride = 0;
    P.dst_row_stride = d->row_stride, P.dst_band_stride = 0;
    P.x0 = map->x0, P.y0 = map->y0, P.width = map->width, P.height = map->height, P.fill = 0.0;
    const size_t lut_bytes = (size_t)rp->n * 4;
    FRS_HIP(ctx->render_lut.ensure(lut_bytes));
    FRS_HIP(hipMemcpyAsync(ctx->render_lut.ptr, rp->lut, lut_bytes, hipMemcpyHostToDevice, ctx->stream));
    RenderParams R;
    R.range = hist_range(rp->lo, rp->hi, rp->n);
    R.lut = ctx->render_lut.as<uint32_t>();
    R.nodata_rgba = rp->nodata_rgba, R.channels = C;
    const char *where = getenv("FRS_RENDER_LUT");
    const bool lds = rp->n <= kRenderLdsLut && !(where && !strcmp(where, "global"));
    // chunks of the longest row (one more when it starts off a boundary); whole steps only, the rest is strided over
    const int64_t cpr = (d->width * C + 15) / 16 + 1;
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(cpr / kRenderBlock, 65535));
    const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(d->height, kRenderMaxGridY), 1u);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "render", &ev);
    switch (s->dtype) {
    case FRS_DT_U8: launch_render<uint8_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_U16: launch_render<uint16_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_I16: launch_render<int16_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_I32: launch_render<int32_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_U32: launch_render<uint32_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_F32: launch_render<float>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    default: launch_render<double>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    }
    prof_end(ctx, "render", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FRS_OK;
}

// bytes from the destination's origin to the end of its last row, or -1 when that does not fit 63 bits
int64_t render_dst_bytes(const frs_raster_desc *d, int C) {
    int64_t x, y;
    if (__builtin_mul_overflow(d->height - 1, d->row_stride, &y) || __builtin_mul_overflow(d->width, (int64_t)C, &x) ||
        __builtin_add_overflow(x, y, &x))
        return -1;
    return x;
}

// argument checks of frs_render_window* (and of frs_render_shaded_window*, frs_shade.hip), before anything is sized,
// copied or launched
int check_render_args(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst,
                      const void *dp, const frs_window_map *map, int32_t mode, const double *nodata,
                      const frs_render_params *rp) {
    if (int rc = check_window_desc(ctx, src)) return rc;
    if (int rc = check_window_desc(ctx, dst)) return rc;
    if (src->nbands != 1 || dst->nbands != 1) { ctx->err = "render: nbands must be 1"; return FRS_E_ARG; }
    if (dst->dtype != FRS_DT_U8) { ctx->err = "render: the destination must be uint8"; return FRS_E_ARG; }
    if (int rc = check_window_map(ctx, map, mode, false)) return rc;
    if (nodata && !nodata_ok(src->dtype, *nodata)) {
        ctx->err = "render: nodata must be an integer inside the dtype's range";
        return FRS_E_ARG;
    }
    if (!rp) { ctx->err = "render: null render parameters"; return FRS_E_ARG; }
    if (rp->channels != 1 && rp->channels != 2 && rp->channels != 4) {
        ctx->err = "render: channels must be 1, 2 or 4";
        return FRS_E_ARG;
    }
    if (rp->n < 1 || rp->n > kRenderMaxLut) { ctx->err = "render: the LUT length must be 1..4096"; return FRS_E_ARG; }
    if (!rp->lut) { ctx->err = "render: null LUT"; return FRS_E_ARG; }
    const double span = rp->hi - rp->lo;
    if (!(rp->lo - rp->lo == 0.0) || !(rp->hi - rp->hi == 0.0) || !(span - span == 0.0)) {
        ctx->err = "render: lo, hi and hi - lo must be finite";
        return FRS_E_ARG;
    }
    if (!(rp->hi > rp->lo)) { ctx->err = "render: hi must be > lo"; return FRS_E_ARG; }
    const int64_t dbytes = render_dst_bytes(dst, rp->channels);
    if (dbytes < 0) { ctx->err = "render: raster extent overflows"; return FRS_E_ARG; }
    if (dst->row_stride < dst->width * rp->channels) {
        ctx->err = "render: row_stride (bytes) < width * channels";
        return FRS_E_ARG;
    }
    const uintptr_t es = (uintptr_t)dtype_size(src->dtype);
    const uintptr_t a = reinterpret_cast<uintptr_t>(sp), b = reinterpret_cast<uintptr_t>(dp);
    if (!sp || !dp || a % es) { ctx->err = "render: null or element-misaligned pointer"; return FRS_E_ARG; }
    if (a < b + (uintptr_t)dbytes && b < a + (uintptr_t)window_extent(src) * es) {
        ctx->err = "render: source and destination overlap";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

// frs_render_window*: every check, then the job between the device rasters `sp` / `dp`, or (host) between staged copies
// of the host rasters they point at
static int render_entry(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst, void *dp,
                        const frs_window_map *map, int32_t mode, const double *nodata, const frs_render_params *rp,
                        bool host) {
    if (!ctx) return FRS_E_ARG;
    if (int rc = check_unsynced(ctx)) return rc;
    if (int rc = check_render_args(ctx, src, sp, dst, dp, map, mode, nodata, rp)) return rc;
    FRS_HIP(hipSetDevice(ctx->device));
    if (!host) return render_job(ctx, src, sp, dst, dp, map, mode, nodata, rp);
    const size_t sbytes = (size_t)window_extent(src) * (size_t)dtype_size(src->dtype);
    return run_staged(ctx, sp, sbytes, dp, (size_t)render_dst_bytes(dst, rp->channels),
                      [&](const void *src_dev, void *dst_dev) {
                          return render_job(ctx, src, src_dev, dst, dst_dev, map, mode, nodata, rp);
                      });
}

}  // namespace frs

extern "C" {

int frs_render_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev, const frs_raster_desc *dst,
                             void *dst_dev, const frs_window_map *map, int32_t mode, const double *nodata,
                             const frs_render_params *render) {
    return frs::render_entry(ctx, src, src_dev, dst, dst_dev, map, mode, nodata, render, false);
}

int frs_render_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host, const frs_raster_desc *dst,
                      void *dst_host, const frs_window_map *map, int32_t mode, const double *nodata,
                      const frs_render_params *render) {
    return frs::render_entry(ctx, src, src_host, dst, dst_host, map, mode, nodata, render, true);
}

}  // extern "C"
