// frs_internal.h -- host-side context, device buffers and launcher entry points.
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/flac_raster_amd.h"
#include "frs_common.h"

// Grow-only device buffer owned by a context.
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (ptr) hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        size_t want = need + need / 8 + 4096;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (ptr) hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(ptr); }
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(static_cast<char *>(ptr) + off); }
};

// pinned host staging (small per-call H2D tables and the packed D2H results of the fast encode path): one
// allocation reused across calls, so the copies are DMA transfers instead of staged pageable copies
struct HostPin {
    void *ptr = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (ptr) hipHostFree(ptr);
        ptr = nullptr;
        bytes = 0;
        size_t want = need + need / 8 + 4096;
        hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocDefault);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (ptr) hipHostFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(static_cast<char *>(ptr) + off); }
};

struct ProfEntry {
    double total_ms = 0.0;
    int count = 0;
};

// Cached job geometry of the fast encode paths: the tile table (partial frames marked), the analysis wave table, the
// partial-frame list and the frame -> tile map stay on the device while the descriptor's geometry repeats (a bench or
// a server encoding same-shaped jobs skips their rebuild and uploads).
struct EncodeGeometry {
    std::vector<int64_t> key;           // descriptor geometry the cache holds (empty: nothing cached)
    std::vector<frs::TileGeom> tiles;   // host tile table, partial frames marked
    std::vector<int64_t> plist;         // partial-frame list
    int64_t nframes = 0;
    int nwaves = 0;
    // the device allocations each table was last uploaded into (a grown DevBuf is a new allocation: upload again)
    void *dev_tiles = nullptr, *dev_wave_tab = nullptr, *dev_plist = nullptr, *dev_frame_tile = nullptr;
};

struct frs_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    std::string err;
    // encode scratch
    DevBuf tiles, norms, analysis, slots, frame_bytes, frame_off, window, tile_sizes, luts, status, frame_tile,
        hdr_tab, wave_tab, plist, sub_slots, sub_bits, mc_bytes;
    int hdr_tab_n = -1, hdr_tab_sr = -1;  // cached frame-header table (fast encode path)
    bool force_generic = false;  // testing: route every job through the generic kernels
    // host staging (pinned)
    DevBuf raster_stage, arena_stage;  // device copies for the host-pointer entry points
    HostPin pin;                       // pinned staging of the fast encode path (tiles, wave table, results)
    HostPin ring[2];                   // pinned upload ring of the batched host-pointer encode (frs_encode_tiles)
    hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;  // its copy engines' streams (created on first use)
    DevBuf host_pack;                  // device side of the packed fast-path results
    // decode scratch
    DevBuf dec_cand, dec_count, dec_pcm, dec_soff, dec_next, dec_status, dec_fb, dec_sel, dec_chass, dec_crc;
    int decode_lane = -1;    // FRS_DECODE_LANE=0/1 (tests): force the pipelined / lane-per-frame decoder
    bool pipe_opt = true;    // FRS_PIPE_OPT=0 (tests): no optimistic small-range decode (read once, not per query)
    uint32_t dec_epoch = 0;  // call counter tagging the candidate selection's look-back words (24 bits, never 0)
    // profiling
    bool prof = false;
    std::map<std::string, ProfEntry> prof_tab;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> ev_pending;
    // cached window (blocksize)
    int window_bs = 0;
    EncodeGeometry geo;  // cached job geometry of the fast encode paths
    // subdivide_tukey levels (6..8): LPC candidates per coded signal, the tukey(0.5 / parts) window; loose mid/side:
    // per-frame assignment of the group leaders and the leader frame list
    DevBuf lpc_cand, window_hi, loose_assign, loose_lead;
    int window_hi_bs = 0, window_hi_parts = 0;
    DevBuf sub_est, st_pick;  // two-channel fast path: subframe estimates (L, R, M, S), the assignment per frame
    DevBuf zero_sub;          // raw-frames tiles: all-zero subframe flags (k_zero_subframes)
    // compare (frs_compare*): per-work-group partial records, their pinned host copy, the second raster's staging
    DevBuf cmp_part, cmp_stage;
    HostPin cmp_pin;
    // placement (frs_place_tiles_device, frs_decode_tiles_window*): the tile table and its pinned host copy, the
    // decoders' interleaved output that frs_decode_tiles_window* places from
    DevBuf place_tab, place_stage;
    HostPin place_pin;
    // band statistics and histogram (frs_band_stats*, frs_band_histogram*): per-work-group partial records, the
    // histogram's per-work-group counter slabs and per-band counts, the pinned host copy of the results
    DevBuf st_part, st_slab, st_counts;
    HostPin st_pin;
    DevBuf render_lut;  // render (frs_render_window*): the call's colour look-up table
    // page-locked host allocations of this context (frs_host_malloc): a C5 decode whose output lies in one returns
    // when the kernel's last work-group has published it, before the stream's completion signal (`unsynced` then
    // makes the next call check the stream for an asynchronous fault first)
    std::vector<std::pair<uintptr_t, size_t>> host_allocs;
    bool unsynced = false;
    bool is_host_alloc(const void *p, size_t n) const {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        for (const auto &r : host_allocs)
            if (a >= r.first && a + n <= r.first + r.second) return true;
        return false;
    }
};

#define FRS_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);              \
            return FRS_E_HIP;                                                          \
        }                                                                              \
    } while (0)

namespace frs {
// A call after an early-returning C5 decode (frs_ctx::unsynced): a fault of that kernel surfaces here, in the next
// call on the context, instead of in some later unrelated HIP call.
inline int check_unsynced(frs_ctx *ctx) {
    if (!ctx->unsynced) return FRS_OK;
    ctx->unsynced = false;
    const hipError_t e = hipStreamQuery(ctx->stream);
    if (e != hipSuccess && e != hipErrorNotReady) {
        ctx->err = std::string("an earlier decode's kernel failed: ") + hipGetErrorString(e);
        return FRS_E_HIP;
    }
    return FRS_OK;
}
// Kernel timing helpers (no-ops unless ctx->prof).
void prof_begin(frs_ctx *ctx, const char *name, hipEvent_t *start, hipStream_t s = nullptr);
void prof_end(frs_ctx *ctx, const char *name, hipEvent_t start, hipStream_t s = nullptr);
void prof_collect(frs_ctx *ctx);

int encode_job(frs_ctx *ctx, const frs_encode_desc *d, const void *raster_dev, void *arena_dev, int64_t arena_cap,
               int64_t *tile_off, double *tile_min, double *tile_max, int32_t *stream_bps);
// Decode the frames of nstreams streams.  out_dev == nullptr: int32 PCM into pcm_dev.  Otherwise the samples are
// de-normalised in the decode kernels (converter.py:88-110) with per-stream dmin/dmax into out_dev (out_dtype),
// and pcm_dev is only an optional int32 scratch (multi-channel / wide streams).
int decode_job(frs_ctx *ctx, const uint8_t *blob_dev, int64_t blob_bytes, const int64_t *stream_off,
               int32_t nstreams, int32_t channels, int32_t bps, int32_t blocksize, int32_t *pcm_dev,
               const int64_t *pcm_off, const double *dmin = nullptr, const double *dmax = nullptr,
               int32_t out_dtype = 0, void *out_dev = nullptr);
int denormalize_job(frs_ctx *ctx, const int32_t *pcm_dev, int64_t n, int pcm_bps, double dmin, double dmax,
                    int32_t out_dtype, void *out_dev);
int64_t arena_bound(const frs_encode_desc *d);
int synth_job(frs_ctx *ctx, int16_t *dev, int bands, int64_t height, int64_t width, int64_t row0, int64_t full_height,
              uint64_t seed);
int dtype_size(int dt);
// Difference statistics of two device rasters (frs_compare.hip); the descriptor is already validated.
int compare_job(frs_ctx *ctx, const frs_compare_desc *d, const void *a_dev, const void *b_dev, frs_compare_band *out);
// Place ntiles decoded tiles into a device raster (frs_place.hip); the arguments are already validated.
int place_job(frs_ctx *ctx, const frs_raster_desc *d, const void *tiles_dev, const int64_t *pcm_off,
              const frs_tile_window *win, int32_t ntiles, void *dst_dev);
// One 2x reduction step between two device rasters (frs_pyramid.hip); the arguments are already validated.  `nodata`
// is null, or points at the nodata value (the masked average of frs_nodata.h; nearest is the same with and without).
int downsample_job(frs_ctx *ctx, const frs_raster_desc *s, const void *src, const frs_raster_desc *d, void *dst,
                   int32_t mode, const double *nodata);
// The checks frs_resample_window* and frs_render_window* share (frs_window.hip): a raster descriptor; the mode and the
// rectangle of a mapping, and its fill unless with_fill is false; elements from a raster's origin to the end of its
// last row (-1: that does not fit 63 bits with room for the element size).
int check_window_desc(frs_ctx *ctx, const frs_raster_desc *d);
int check_window_map(frs_ctx *ctx, const frs_window_map *map, int32_t mode, bool with_fill);
int64_t window_extent(const frs_raster_desc *d);
// The checks frs_render_window* and frs_render_shaded_window* share (frs_render.hip): every argument of a render; bytes
// from a uint8 destination's origin to the end of its last row of C channels (-1: that does not fit 63 bits).
int check_render_args(frs_ctx *ctx, const frs_raster_desc *src, const void *sp, const frs_raster_desc *dst,
                      const void *dp, const frs_window_map *map, int32_t mode, const double *nodata,
                      const frs_render_params *rp);
int64_t render_dst_bytes(const frs_raster_desc *d, int C);
// May `nd` be the nodata value of a raster of dtype `dt` (frs_nodata.h: nd_representable)?
bool nodata_ok(int dt, double nd);

// The host-pointer form of a job between two rasters (frs_downsample2*, frs_resample_window*): both rasters go up to
// the context's staging buffers, job(src_dev, dst_dev) runs on them, the destination comes back.
template <typename Job>
int run_staged(frs_ctx *ctx, const void *src_host, size_t sbytes, void *dst_host, size_t dbytes, Job job) {
    FRS_HIP(ctx->raster_stage.ensure(sbytes));
    FRS_HIP(ctx->arena_stage.ensure(dbytes));
    FRS_HIP(hipMemcpyAsync(ctx->raster_stage.ptr, src_host, sbytes, hipMemcpyHostToDevice, ctx->stream));
    // the destination goes up first: its row and band padding comes back as it was
    FRS_HIP(hipMemcpyAsync(ctx->arena_stage.ptr, dst_host, dbytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = job(ctx->raster_stage.ptr, ctx->arena_stage.ptr)) return rc;
    FRS_HIP(hipMemcpyAsync(dst_host, ctx->arena_stage.ptr, dbytes, hipMemcpyDeviceToHost, ctx->stream));
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    return FRS_OK;
}
// The host-pointer form of a job that reads one raster and returns its results to the host itself (frs_band_stats,
// frs_band_histogram): the raster goes up to the context's staging buffer, job(src_dev) runs on it and synchronises.
// The copy keeps the host raster's position within a 16-byte window, so that a job whose summation order depends on
// the alignment gives the host raster's bits for it.
template <typename Job> int run_staged(frs_ctx *ctx, const void *src_host, size_t sbytes, Job job) {
    const size_t phase = reinterpret_cast<uintptr_t>(src_host) & 15u;
    FRS_HIP(ctx->raster_stage.ensure(sbytes + 16));
    void *dev = ctx->raster_stage.at<char>(phase);
    FRS_HIP(hipMemcpyAsync(dev, src_host, sbytes, hipMemcpyHostToDevice, ctx->stream));
    return job(dev);
}
}  // namespace frs
