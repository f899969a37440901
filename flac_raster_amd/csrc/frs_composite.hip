// frs_composite.hip -- a rectangle of THREE bands as one stretched 8-bit colour image (frs_render_composite_window*):
// the render of frs_render.hip with a plane per colour channel (csrc/frs_composite.h holds the definition, the
// arithmetic and the lane function, composite_group).  It is the last stage of streaming.render_window(bands=(r, g, b)):
// the three decoded planes of a band-planar device window leave the device as the W x H x 4 bytes a viewer shows, in one
// pass instead of three renders and an interleave.
//
//   k_render_composite_window   grid (gx, gy), 256 threads: k_render_window's.  Work-group (bx, by) owns destination
//                               rows by, by + gy, ... and, of each, the 16-byte chunks bx * 256 + lane, striding gx * 256.
//
// One kernel, templated on the mode, the dtype, the mask policy and where the LUT is read from.  The store side is
// k_render_window's for four channels.  No atomics, no init pass.
//
// Where the LUT lives.  As in frs_render.hip, and for its reasons: the packed table is the same size and a work-group
// still owns one row segment of 256 chunks (4 KB of output), which is what a table loaded per work-group must be paid
// for by.  n <= 256 entries: one dword per lane, one coalesced load and one barrier put it into LDS, where the three
// look-ups of a pixel are LDS reads.  A longer table (up to 16 KB: 16 loads per lane per work-group, four times the
// bytes the work-group stores) stays in global memory and is gathered through the read-only path; three gathers per
// pixel instead of one make its L1 residency matter more, and it still takes at most half of the vector L1.
#include <algorithm>

#include "frs_composite.h"
#include "frs_internal.h"

namespace frs {

constexpr int kCompLdsLut = kRenderBlock;  // entries up to which the table is copied to LDS: one per lane

template <int MODE, typename T, typename Mask, bool LDS>
__global__ void __launch_bounds__(kRenderBlock)
    k_render_composite_window(const T *__restrict__ src, uint8_t *__restrict__ dst, WinParams P, CompParams R,
                              Mask mask) {
    if constexpr (LDS) {
        __shared__ uint32_t s_lut[kCompLdsLut];
        if ((int)threadIdx.x < R.range[0].nbins) s_lut[threadIdx.x] = R.lut[threadIdx.x];
        __syncthreads();
        R.lut = s_lut;
    }
    composite_group<MODE, T>(src, dst, P, R, mask, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y, threadIdx.x);
}

template <int MODE, typename T, typename Mask>
static void launch_comp_mask(hipStream_t st, dim3 grid, const T *s, uint8_t *d, const WinParams &P,
                             const CompParams &R, const Mask &mask, bool lds) {
    if (lds) k_render_composite_window<MODE, T, Mask, true><<<grid, kRenderBlock, 0, st>>>(s, d, P, R, mask);
    else k_render_composite_window<MODE, T, Mask, false><<<grid, kRenderBlock, 0, st>>>(s, d, P, R, mask);
}

// nodata: null without one
template <int MODE, typename T>
static void launch_comp_mode(hipStream_t st, dim3 grid, const T *s, uint8_t *d, const WinParams &P,
                             const CompParams &R, const double *nodata, bool lds) {
    if (nodata) launch_comp_mask<MODE, T>(st, grid, s, d, P, R, Nodata<T>{nd_cast<T>(*nodata)}, lds);
    else launch_comp_mask<MODE, T>(st, grid, s, d, P, R, NoNodata{}, lds);
}

template <typename T>
static void launch_comp(hipStream_t st, dim3 grid, int32_t mode, const void *src, void *dst, const WinParams &P,
                        const CompParams &R, const double *nodata, bool lds) {
    const T *s = static_cast<const T *>(src);
    uint8_t *d = static_cast<uint8_t *>(dst);
    if (mode == FRS_RESAMPLE_NEAREST) launch_comp_mode<kWindowNearest, T>(st, grid, s, d, P, R, nodata, lds);
    else if (mode == FRS_RESAMPLE_BILINEAR) launch_comp_mode<kWindowBilinear, T>(st, grid, s, d, P, R, nodata, lds);
    else launch_comp_mode<kWindowAverage, T>(st, grid, s, d, P, R, nodata, lds);
}

// The arguments are already validated (composite_entry below).  Synchronous on the context stream.
static int composite_job(frs_ctx *ctx, const frs_raster_desc *s, const void *src_dev, const frs_raster_desc *d,
                         void *dst_dev, const frs_window_map *map, int32_t mode, const double *nodata,
                         const frs_composite_params *cp) {
    WinParams P;
    P.src_h = s->height, P.src_w = s->width, P.dst_h = d->height, P.dst_w = d->width;
    P.src_row_stride = s->row_stride, P.src_band_stride = s->band_stride;
    P.dst_row_stride = d->row_stride, P.dst_band_stride = 0;
    P.x0 = map->x0, P.y0 = map->y0, P.width = map->width, P.height = map->height, P.fill = 0.0;
    const size_t lut_bytes = (size_t)cp->n * 4;
    FRS_HIP(ctx->render_lut.ensure(lut_bytes));
    FRS_HIP(hipMemcpyAsync(ctx->render_lut.ptr, cp->lut, lut_bytes, hipMemcpyHostToDevice, ctx->stream));
    CompParams R;
    for (int c = 0; c < 3; c++) R.range[c] = hist_range(cp->lo[c], cp->hi[c], cp->n);
    R.lut = ctx->render_lut.as<uint32_t>();
    R.nodata_rgba = cp->nodata_rgba;
    const bool lds = cp->n <= kCompLdsLut;
    // chunks of the longest row (one more when it starts off a boundary); whole steps only, the rest is strided over
    const int64_t cpr = (d->width * 4 + 15) / 16 + 1;
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(cpr / kRenderBlock, 65535));
    const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(d->height, kRenderMaxGridY), 1u);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "render_composite", &ev);
    switch (s->dtype) {
    case FRS_DT_U8: launch_comp<uint8_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_U16: launch_comp<uint16_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_I16: launch_comp<int16_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_I32: launch_comp<int32_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_U32: launch_comp<uint32_t>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    case FRS_DT_F32: launch_comp<float>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    default: launch_comp<double>(st, grid, mode, src_dev, dst_dev, P, R, nodata, lds); break;
    }
    prof_end(ctx, "render_composite", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FRS_OK;
}

// argument checks of frs_render_composite_window*, before anything is sized, copied or launched: check_render_args'
// rules on plane 0 with each channel's lo / hi in turn, three planes, and the overlap of the destination with all three
static int check_composite_args(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst,
                                const void *dp, const frs_window_map *map, int32_t mode, const double *nodata,
                                const frs_composite_params *cp) {
    // (a band stride smaller than the plane's extent fails here)
    if (int rc = check_window_desc(ctx, src)) return rc;
    if (src->nbands != 3) { ctx->err = "render_composite: the source must have 3 bands"; return FRS_E_ARG; }
    if (!cp) { ctx->err = "render_composite: null parameters"; return FRS_E_ARG; }
    frs_raster_desc plane = *src;
    plane.nbands = 1;
    for (int c = 0; c < 3; c++) {
        const frs_render_params rp = {cp->lo[c], cp->hi[c], cp->lut, cp->n, cp->nodata_rgba, 4};
        if (int rc = check_render_args(ctx, &plane, sp, dst, dp, map, mode, nodata, &rp)) return rc;
    }
    const uintptr_t es = (uintptr_t)dtype_size(src->dtype);
    const uintptr_t a = reinterpret_cast<uintptr_t>(sp), b = reinterpret_cast<uintptr_t>(dp);
    if (a < b + (uintptr_t)render_dst_bytes(dst, 4) && b < a + (uintptr_t)window_extent(src) * es) {
        ctx->err = "render_composite: source and destination overlap";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

// frs_render_composite_window*: every check, then the job between the device rasters `sp` / `dp`, or (host) between
// staged copies of the host rasters they point at
static int composite_entry(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst,
                           void *dp, const frs_window_map *map, int32_t mode, const double *nodata,
                           const frs_composite_params *cp, bool host) {
    if (!ctx) return FRS_E_ARG;
    if (int rc = check_unsynced(ctx)) return rc;
    if (int rc = check_composite_args(ctx, src, sp, dst, dp, map, mode, nodata, cp)) return rc;
    FRS_HIP(hipSetDevice(ctx->device));
    if (!host) return composite_job(ctx, src, sp, dst, dp, map, mode, nodata, cp);
    const size_t sbytes = (size_t)window_extent(src) * (size_t)dtype_size(src->dtype);
    return run_staged(ctx, sp, sbytes, dp, (size_t)render_dst_bytes(dst, 4),
                      [&](const void *src_dev, void *dst_dev) {
                          return composite_job(ctx, src, src_dev, dst, dst_dev, map, mode, nodata, cp);
                      });
}

}  // namespace frs

extern "C" {

int frs_render_composite_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                       const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map,
                                       int32_t mode, const double *nodata, const frs_composite_params *composite) {
    return frs::composite_entry(ctx, src, src_dev, dst, dst_dev, map, mode, nodata, composite, false);
}

int frs_render_composite_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host,
                                const frs_raster_desc *dst, void *dst_host, const frs_window_map *map, int32_t mode,
                                const double *nodata, const frs_composite_params *composite) {
    return frs::composite_entry(ctx, src, src_host, dst, dst_host, map, mode, nodata, composite, true);
}

}  // extern "C"
