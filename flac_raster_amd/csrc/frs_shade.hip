// frs_shade.hip -- a rectangle of one band as hillshaded 8-bit colour (frs_render_shaded_window*): the render of
// frs_render.hip with Horn's 3 x 3 gradient taken on the OUTPUT grid (csrc/frs_shade.h holds the definition, the
// arithmetic and the two lane functions).
//
//   k_render_shaded_window   grid (gx, gy) of tiles, 256 threads.  A work-group owns tiles (bx + i gx, by + j gy); a tile
//                            is 16 destination rows by 16 aligned 16-byte chunks, one chunk per lane.
//
// Every other kernel of the read side maps one output to a set of source taps.  This one needs the eight neighbours of
// an output on the output grid, each a full resample: the work-group computes the samples of its tile and a one-pixel
// apron once (shade_fill), keeps them as doubles in LDS, and after ONE barrier every lane reads the 3 x 3 neighbourhoods
// of its chunk's pixels from there (shade_emit).  When a work-group has a further tile a second barrier keeps its fill
// from overtaking the emit.  The apron comes from the raster (positions -1 and w / h are plain arithmetic), so two
// neighbouring map tiles shade identically along their seam when the decoded window reaches that far.
//
// LDS: the sample array (ShadeShape<C>::samples doubles: 39744, 20160, 10368 bytes for C = 1, 2, 4), the 256-byte shade
// table, and the colour LUT when it has n <= 256 entries (1 KB; a longer one is gathered from global memory, as in
// frs_render.hip, here chosen at run time through one pointer).  No atomics, no init pass, no scratch.
#include <math.h>

#include <algorithm>

#include "frs_internal.h"
#include "frs_shade.h"

namespace frs {

constexpr int kShadeLdsLut = kShadeBlock;  // entries up to which the colour table is copied to LDS: one per lane

template <int MODE, typename T, typename Mask, int C>
__global__ void __launch_bounds__(kShadeBlock) k_render_shaded_window(const T *__restrict__ src,
                                                                      uint8_t *__restrict__ dst, WinParams P,
                                                                      RenderParams R, ShadeParams S, Mask mask) {
    __shared__ double s_tile[ShadeShape<C>::samples];
    __shared__ uint32_t s_lut[kShadeLdsLut];
    __shared__ uint8_t s_table[256];
    s_table[threadIdx.x] = S.table[threadIdx.x];
    S.table = s_table;
    if (R.range.nbins <= kShadeLdsLut) {
        if ((int)threadIdx.x < R.range.nbins) s_lut[threadIdx.x] = R.lut[threadIdx.x];
        R.lut = s_lut;
    }
    const int64_t ntx = shade_tiles_x<C>(P), nty = shade_tiles_y(P);
    bool again = false;
    for (int64_t ty = blockIdx.y; ty < nty; ty += gridDim.y)
        for (int64_t tx = blockIdx.x; tx < ntx; tx += gridDim.x) {
            if (again) __syncthreads();  // the previous tile's emit has read the samples
            again = true;
            const ShadeTile t = shade_tile<C>(dst, P, tx, ty);
            shade_fill<MODE, T, Mask, C>(src, P, mask, t, s_tile, threadIdx.x);
            __syncthreads();  // (the first one also publishes the tables)
            shade_emit<C>(dst, P, R, S, t, s_tile, threadIdx.x);
        }
}

template <int MODE, typename T, typename Mask>
static void launch_shade_mask(hipStream_t st, const T *s, uint8_t *d, const WinParams &P, const RenderParams &R,
                              const ShadeParams &S, const Mask &mask) {
    const auto grid = [&](int64_t ntx) {
        return dim3((unsigned)std::min<int64_t>(ntx, kShadeMaxGrid),
                    (unsigned)std::min<int64_t>(shade_tiles_y(P), kShadeMaxGrid), 1u);
    };
    if (R.channels == 1)
        k_render_shaded_window<MODE, T, Mask, 1><<<grid(shade_tiles_x<1>(P)), kShadeBlock, 0, st>>>(s, d, P, R, S, mask);
    else if (R.channels == 2)
        k_render_shaded_window<MODE, T, Mask, 2><<<grid(shade_tiles_x<2>(P)), kShadeBlock, 0, st>>>(s, d, P, R, S, mask);
    else
        k_render_shaded_window<MODE, T, Mask, 4><<<grid(shade_tiles_x<4>(P)), kShadeBlock, 0, st>>>(s, d, P, R, S, mask);
}

// nodata: null without one
template <int MODE, typename T>
static void launch_shade_mode(hipStream_t st, const T *s, uint8_t *d, const WinParams &P, const RenderParams &R,
                              const ShadeParams &S, const double *nodata) {
    if (nodata) launch_shade_mask<MODE, T>(st, s, d, P, R, S, Nodata<T>{nd_cast<T>(*nodata)});
    else launch_shade_mask<MODE, T>(st, s, d, P, R, S, NoNodata{});
}

template <typename T>
static void launch_shade(hipStream_t st, int32_t mode, const void *src, void *dst, const WinParams &P,
                         const RenderParams &R, const ShadeParams &S, const double *nodata) {
    const T *s = static_cast<const T *>(src);
    uint8_t *d = static_cast<uint8_t *>(dst);
    if (mode == FRS_RESAMPLE_NEAREST) launch_shade_mode<kWindowNearest, T>(st, s, d, P, R, S, nodata);
    else if (mode == FRS_RESAMPLE_BILINEAR) launch_shade_mode<kWindowBilinear, T>(st, s, d, P, R, S, nodata);
    else launch_shade_mode<kWindowAverage, T>(st, s, d, P, R, S, nodata);
}

// The arguments are already validated (shade_entry below).  Synchronous on the context stream.
static int shade_job(frs_ctx *ctx, const frs_raster_desc *s, const void *src_dev, const frs_raster_desc *d,
                     void *dst_dev, const frs_window_map *map, int32_t mode, const double *nodata,
                     const frs_render_params *rp, const frs_shade_params *sp) {
    WinParams P;
    P.src_h = s->height, P.src_w = s->width, P.dst_h = d->height, P.dst_w = d->width;
    P.src_row_stride = s->row_stride, P.src_band_stride = 0;
    P.dst_row_stride = d->row_stride, P.dst_band_stride = 0;
    P.x0 = map->x0, P.y0 = map->y0, P.width = map->width, P.height = map->height, P.fill = 0.0;
    // the colour table, then the shade table, in the context's table buffer
    const size_t lut_bytes = (size_t)rp->n * 4;
    FRS_HIP(ctx->render_lut.ensure(lut_bytes + 256));
    FRS_HIP(hipMemcpyAsync(ctx->render_lut.ptr, rp->lut, lut_bytes, hipMemcpyHostToDevice, ctx->stream));
    FRS_HIP(hipMemcpyAsync(ctx->render_lut.at<uint8_t>(lut_bytes), sp->table, 256, hipMemcpyHostToDevice,
                           ctx->stream));
    RenderParams R;
    R.range = hist_range(rp->lo, rp->hi, rp->n);
    R.lut = ctx->render_lut.as<uint32_t>();
    R.nodata_rgba = rp->nodata_rgba, R.channels = rp->channels;
    ShadeParams S;
    S.lx = sp->lx, S.ly = sp->ly, S.lz = sp->lz, S.kx = sp->kx, S.ky = sp->ky;
    S.table = ctx->render_lut.at<uint8_t>(lut_bytes);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "render_shaded", &ev);
    switch (s->dtype) {
    case FRS_DT_U8: launch_shade<uint8_t>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    case FRS_DT_U16: launch_shade<uint16_t>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    case FRS_DT_I16: launch_shade<int16_t>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    case FRS_DT_I32: launch_shade<int32_t>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    case FRS_DT_U32: launch_shade<uint32_t>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    case FRS_DT_F32: launch_shade<float>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    default: launch_shade<double>(st, mode, src_dev, dst_dev, P, R, S, nodata); break;
    }
    prof_end(ctx, "render_shaded", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FRS_OK;
}

// frs_render_shaded_window*: frs_render_window*'s checks and the shade parameters', then the job between the device
// rasters `sp` / `dp`, or (host) between staged copies of the host rasters they point at
static int shade_entry(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst, void *dp,
                       const frs_window_map *map, int32_t mode, const double *nodata, const frs_render_params *rp,
                       const frs_shade_params *shade, bool host) {
    if (!ctx) return FRS_E_ARG;
    if (int rc = check_unsynced(ctx)) return rc;
    if (int rc = check_render_args(ctx, src, sp, dst, dp, map, mode, nodata, rp)) return rc;
    if (!shade || !shade->table) { ctx->err = "render_shaded: null shade parameters or table"; return FRS_E_ARG; }
    for (const double v : {shade->lx, shade->ly, shade->lz, shade->kx, shade->ky})
        if (!(v - v == 0.0)) { ctx->err = "render_shaded: lx, ly, lz, kx and ky must be finite"; return FRS_E_ARG; }
    FRS_HIP(hipSetDevice(ctx->device));
    if (!host) return shade_job(ctx, src, sp, dst, dp, map, mode, nodata, rp, shade);
    const size_t sbytes = (size_t)window_extent(src) * (size_t)dtype_size(src->dtype);
    return run_staged(ctx, sp, sbytes, dp, (size_t)render_dst_bytes(dst, rp->channels),
                      [&](const void *src_dev, void *dst_dev) {
                          return shade_job(ctx, src, src_dev, dst, dst_dev, map, mode, nodata, rp, shade);
                      });
}

}  // namespace frs

extern "C" {

int frs_render_shaded_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                    const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map, int32_t mode,
                                    const double *nodata, const frs_render_params *render,
                                    const frs_shade_params *shade) {
    return frs::shade_entry(ctx, src, src_dev, dst, dst_dev, map, mode, nodata, render, shade, false);
}

int frs_render_shaded_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host,
                             const frs_raster_desc *dst, void *dst_host, const frs_window_map *map, int32_t mode,
                             const double *nodata, const frs_render_params *render, const frs_shade_params *shade) {
    return frs::shade_entry(ctx, src, src_host, dst, dst_host, map, mode, nodata, render, shade, true);
}

}  // extern "C"
