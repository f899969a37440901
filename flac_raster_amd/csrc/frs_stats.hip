// frs_stats.hip -- statistics and histogram of the bands of one raster (frs_band_stats*, frs_band_histogram*): each is
// one streaming pass over every band.
//
// The reference (Youssef-Harby/flac-raster) has no such call; a caller of it downloads the raster and runs numpy's
// min / max / mean / std / histogram / percentile over it, several whole-array passes.  frs_stats.h holds the
// definitions (validity, exact integer sums, the bin rule, the centred square sum) and the lane function.
//
//   k_band_stats       grid (gx, nbands), kStBlock threads.  Work-group (g, band) walks its share of the band's 16-byte
//                      windows (stats_fold), reduces lane -> wave (shuffles, a fixed xor tree) -> work-group (LDS, waves
//                      in order) and writes ONE StatsPartial record.  No atomics, no init pass: the host adds the gx
//                      records of a band in work-group order.
//   k_band_histogram   grid (gx, nbands), kHistBlock threads, nbins * copies u32 counters in LDS.  Lanes count with LDS
//                      atomic adds (a lane merges equal bins that follow one another into one add; for nbins <=
//                      kHistCopyBins every wave has a copy of the counters to itself), keep below / above / m2 in
//                      registers, and the work-group writes its counters to a slab of its own plus one HistPartial.
//   k_hist_reduce      one thread per bin adds a band's gx slabs into a u64.
//
// Both grids are functions of (height, width, nbands, dtype, layout) only -- never of the CU count or the environment --
// so the float sums, whose value depends on the summation tree, reproduce run to run and machine to machine.
//
// Integer exactness: stats_job rejects shapes in which one work-group would fold more than kStatsMaxPerGroup = 2^30
// elements, the bound frs_stats.h's widths are argued from (and the bound of a u32 LDS counter).  The host adds the
// partials in __int128 / with add_u128 and converts to double once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "frs_internal.h"
#include "frs_stats.h"

namespace frs {

constexpr int kStBlock = 256;        // threads per work-group of k_band_stats
constexpr int kStUnroll = 4;         // 16-byte loads in flight per lane
constexpr int kStMaxGroups = 2048;   // cap of gx * nbands (grid-stride beyond it)
constexpr int kHistBlock = 512;      // threads per work-group of k_band_histogram
constexpr int kHistUnroll = 4;
constexpr int kHistMaxGroups = 1024;
constexpr int kHistMaxBins = 16384;  // 64 KB of u32 counters: two work-groups share a CU's 160 KB of LDS
constexpr int kHistCopyBins = 512;   // up to here every wave counts into a copy of its own (8 x 512 x 4 B = 16 KB)
constexpr int64_t kStatsMaxPerGroup = (int64_t)1 << 30;
// (flac_raster_amd/_native.py mirrors these for the tests' shape arithmetic)

union StatsVal {
    int64_t i;  // integer dtypes
    double f;   // float dtypes
};

// one work-group's partial of one band (first pass)
struct StatsPartial {
    int64_t n_valid, n_nodata, n_nan;
    StatsVal mn, mx, sum;
    uint64_t sq_hi, sq_lo;
};
// one work-group's partial of one band (second pass)
struct HistPartial {
    uint64_t below, above;
    double m2;
};

template <typename V> __device__ inline V st_wave_sum(V v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <typename V> __device__ inline V st_wave_min(V v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const V w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
template <typename V> __device__ inline V st_wave_max(V v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const V w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ inline void st_wave_sum_u128(unsigned long long &hi, unsigned long long &lo) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t xh = __shfl_xor(hi, o), xl = __shfl_xor(lo, o);
        uint64_t h = hi, l = lo;
        add_u128(h, l, xh, xl);
        hi = h, lo = l;
    }
}

template <typename T, bool MASKED>
__global__ void __launch_bounds__(kStBlock) k_band_stats(const T *A, StatsParams P, int64_t band_stride, T nd,
                                                        StatsPartial *out) {
    constexpr bool F = std::is_floating_point_v<T>;
    const int band = blockIdx.y, gx = gridDim.x, g = blockIdx.x, tid = threadIdx.x;
    StatsAcc<T, MASKED> acc;
    acc.nd = nd;
    stats_fold<kStBlock, kStUnroll>(acc, A + (int64_t)band * band_stride, P, g, gx, tid);

    // ---- lane -> wave -> work-group
    StatsPartial r;
    r.n_valid = st_wave_sum((int64_t)acc.n_valid);
    r.n_nodata = st_wave_sum((int64_t)acc.n_nodata);
    r.n_nan = st_wave_sum((int64_t)acc.n_nan);
    if constexpr (F) {
        r.mn.f = st_wave_min(acc.mn), r.mx.f = st_wave_max(acc.mx);
        r.sum.f = st_wave_sum(acc.sum);
        r.sq_hi = 0, r.sq_lo = 0;
    } else {
        r.mn.i = st_wave_min((int64_t)acc.mn), r.mx.i = st_wave_max((int64_t)acc.mx);
        r.sum.i = st_wave_sum(acc.sum);
        unsigned long long hi = acc.sq_hi, lo = acc.sq_lo;
        st_wave_sum_u128(hi, lo);
        r.sq_hi = hi, r.sq_lo = lo;
    }
    __shared__ StatsPartial wp[kStBlock / 64];
    if ((tid & 63) == 0) wp[tid >> 6] = r;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kStBlock / 64; w++) {  // waves in order
            const StatsPartial q = wp[w];
            r.n_valid += q.n_valid, r.n_nodata += q.n_nodata, r.n_nan += q.n_nan;
            if constexpr (F) {
                r.mn.f = q.mn.f < r.mn.f ? q.mn.f : r.mn.f;
                r.mx.f = q.mx.f > r.mx.f ? q.mx.f : r.mx.f;
                r.sum.f = r.sum.f + q.sum.f;
            } else {
                r.mn.i = q.mn.i < r.mn.i ? q.mn.i : r.mn.i;
                r.mx.i = q.mx.i > r.mx.i ? q.mx.i : r.mx.i;
                r.sum.i += q.sum.i;
                add_u128(r.sq_hi, r.sq_lo, q.sq_hi, q.sq_lo);
            }
        }
        out[(int64_t)band * gx + g] = r;
    }
}

// the device's counter sink: an LDS atomic add
struct LdsSink {
    uint32_t *bins;
    __host__ __device__ inline void add(int32_t b, uint32_t n) {
#ifdef __HIP_DEVICE_COMPILE__
        atomicAdd(&bins[b], n);
#else
        bins[b] += n;
#endif
    }
};

extern __shared__ __attribute__((aligned(16))) uint32_t hist_lds[];  // nbins * copies counters (>= kHistLdsMin bytes)
constexpr size_t kHistLdsMin = (kHistBlock / 64) * sizeof(HistPartial);

template <typename T, bool MASKED>
__global__ void __launch_bounds__(kHistBlock) k_band_histogram(const T *A, StatsParams P, int64_t band_stride, T nd,
                                                              HistRange R, double centre, int copies, uint32_t *slabs,
                                                              HistPartial *out) {
    const int band = blockIdx.y, gx = gridDim.x, g = blockIdx.x, tid = threadIdx.x;
    const int nbins = R.nbins;
    for (int i = tid; i < nbins * copies; i += kHistBlock) hist_lds[i] = 0u;
    __syncthreads();
    HistAcc<T, MASKED, LdsSink> acc;
    acc.r = R, acc.centre = centre, acc.nd = nd;
    acc.sink.bins = hist_lds + ((tid >> 6) % copies) * nbins;
    stats_fold<kHistBlock, kHistUnroll>(acc, A + (int64_t)band * band_stride, P, g, gx, tid);
    __syncthreads();
    uint32_t *slab = slabs + ((int64_t)band * gx + g) * nbins;
    for (int b = tid; b < nbins; b += kHistBlock) {
        uint32_t s = 0;
        for (int c = 0; c < copies; c++) s += hist_lds[c * nbins + b];
        slab[b] = s;
    }
    __syncthreads();  // the counters are out: their LDS now holds the waves' partials

    HistPartial r;
    r.below = (uint64_t)st_wave_sum((int64_t)acc.below);
    r.above = (uint64_t)st_wave_sum((int64_t)acc.above);
    r.m2 = st_wave_sum(acc.m2);
    HistPartial *wp = reinterpret_cast<HistPartial *>(hist_lds);
    if ((tid & 63) == 0) wp[tid >> 6] = r;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kHistBlock / 64; w++) {  // waves in order
            r.below += wp[w].below, r.above += wp[w].above;
            r.m2 = r.m2 + wp[w].m2;
        }
        out[(int64_t)band * gx + g] = r;
    }
}

// counts[band][b] = the sum of the band's gx slabs at b
__global__ void __launch_bounds__(256) k_hist_reduce(const uint32_t *slabs, int gx, int nbins, uint64_t *counts) {
    const int b = blockIdx.x * 256 + threadIdx.x, band = blockIdx.y;
    if (b >= nbins) return;
    const uint32_t *p = slabs + (int64_t)band * gx * nbins + b;
    uint64_t s = 0;
    for (int g = 0; g < gx; g++) s += p[(int64_t)g * nbins];
    counts[(int64_t)band * nbins + b] = s;
}

// Work-groups per band: one per step of block * unroll windows, capped so that gx * nbands stays near max_groups.
static int64_t stats_groups(int64_t items, int nbands, int block, int unroll, int max_groups) {
    const int64_t chunk = (int64_t)block * unroll;
    const int64_t want = (items + chunk - 1) / chunk;
    const int64_t cap = std::max<int64_t>(1, max_groups / nbands);
    return std::max<int64_t>(1, std::min(want, cap));
}

template <typename T> static T stats_nd(const double *nodata) {
    if (!nodata) return (T)0;
    return nd_cast<T>(*nodata);
}

template <typename T>
static void launch_stats(hipStream_t st, dim3 grid, const void *a, const StatsParams &P, int64_t bs, const double *nodata,
                         StatsPartial *out) {
    if (nodata) k_band_stats<T, true><<<grid, kStBlock, 0, st>>>(static_cast<const T *>(a), P, bs, stats_nd<T>(nodata), out);
    else k_band_stats<T, false><<<grid, kStBlock, 0, st>>>(static_cast<const T *>(a), P, bs, (T)0, out);
}

template <typename T>
static void launch_hist(hipStream_t st, dim3 grid, size_t lds, const void *a, const StatsParams &P, int64_t bs,
                        const double *nodata, const HistRange &R, double centre, int copies, uint32_t *slabs,
                        HistPartial *out) {
    if (nodata)
        k_band_histogram<T, true><<<grid, kHistBlock, lds, st>>>(static_cast<const T *>(a), P, bs, stats_nd<T>(nodata), R,
                                                                 centre, copies, slabs, out);
    else
        k_band_histogram<T, false><<<grid, kHistBlock, lds, st>>>(static_cast<const T *>(a), P, bs, (T)0, R, centre,
                                                                  copies, slabs, out);
}

static StatsParams stats_params(const frs_raster_desc *d) {
    StatsParams P;
    P.height = d->height, P.width = d->width, P.row_stride = d->row_stride;
    P.dense = d->row_stride == d->width ? 1 : 0;
    return P;
}

// the shape's work-group count, or 0 with FRS_E_ARG's message set when a work-group's share exceeds the exactness bound
static int stats_grid(frs_ctx *ctx, const frs_raster_desc *d, int block, int unroll, int max_groups) {
    const int es = dtype_size(d->dtype);
    const int64_t items = stats_items(d->height, d->width, d->row_stride == d->width, es);
    const int64_t gx = stats_groups(items, d->nbands, block, unroll, max_groups);
    if (stats_group_share(items, gx, (int64_t)block * unroll, es) > kStatsMaxPerGroup) {
        ctx->err = "stats: more than 2^30 elements per work-group (a 64-bit partial sum could overflow)";
        return 0;
    }
    return (int)gx;
}

// The arguments are already validated (stats_entry below).  Synchronous on the context stream.
static int stats_job(frs_ctx *ctx, const frs_raster_desc *d, const void *dev, const double *nodata,
                     frs_band_stats_out *out) {
    const int nb = d->nbands;
    const int gx = stats_grid(ctx, d, kStBlock, kStUnroll, kStMaxGroups);
    if (gx == 0) return FRS_E_ARG;
    const StatsParams P = stats_params(d);
    const int64_t bs = nb > 1 ? d->band_stride : 0;
    const size_t bytes = (size_t)nb * gx * sizeof(StatsPartial);
    FRS_HIP(ctx->st_part.ensure(bytes));  // every record is written by its work-group: no init pass
    FRS_HIP(ctx->st_pin.ensure(bytes));
    StatsPartial *dpart = ctx->st_part.as<StatsPartial>();
    const dim3 grid((unsigned)gx, (unsigned)nb);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "band_stats", &ev);
    switch (d->dtype) {
    case FRS_DT_U8: launch_stats<uint8_t>(st, grid, dev, P, bs, nodata, dpart); break;
    case FRS_DT_U16: launch_stats<uint16_t>(st, grid, dev, P, bs, nodata, dpart); break;
    case FRS_DT_I16: launch_stats<int16_t>(st, grid, dev, P, bs, nodata, dpart); break;
    case FRS_DT_I32: launch_stats<int32_t>(st, grid, dev, P, bs, nodata, dpart); break;
    case FRS_DT_U32: launch_stats<uint32_t>(st, grid, dev, P, bs, nodata, dpart); break;
    case FRS_DT_F32: launch_stats<float>(st, grid, dev, P, bs, nodata, dpart); break;
    default: launch_stats<double>(st, grid, dev, P, bs, nodata, dpart); break;
    }
    prof_end(ctx, "band_stats", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipMemcpyAsync(ctx->st_pin.ptr, dpart, bytes, hipMemcpyDeviceToHost, st));
    FRS_HIP(hipStreamSynchronize(st));
    prof_collect(ctx);

    const bool is_float = d->dtype == FRS_DT_F32 || d->dtype == FRS_DT_F64;
    const StatsPartial *hp = ctx->st_pin.at<StatsPartial>(0);
    for (int b = 0; b < nb; b++) {
        const StatsPartial *p = hp + (size_t)b * gx;
        frs_band_stats_out o;
        memset(&o, 0, sizeof(o));
        for (int g = 0; g < gx; g++) o.n_valid += p[g].n_valid, o.n_nodata += p[g].n_nodata, o.n_nan += p[g].n_nan;
        if (is_float) {
            double mn = INFINITY, mx = -INFINITY, sum = 0.0;
            for (int g = 0; g < gx; g++) {  // work-group order
                mn = p[g].mn.f < mn ? p[g].mn.f : mn;
                mx = p[g].mx.f > mx ? p[g].mx.f : mx;
                sum = sum + p[g].sum.f;
            }
            o.min = mn, o.max = mx, o.sum = sum;
        } else {
            int64_t mn = INT64_MAX, mx = INT64_MIN;
            __int128 sum = 0;
            uint64_t qh = 0, ql = 0;
            for (int g = 0; g < gx; g++) {
                mn = std::min(mn, p[g].mn.i), mx = std::max(mx, p[g].mx.i);
                sum += p[g].sum.i;
                add_u128(qh, ql, p[g].sq_hi, p[g].sq_lo);
            }
            o.min = (double)mn, o.max = (double)mx;
            o.sum = (double)sum;  // one rounding
            o.isum_hi = (int64_t)(sum >> 64), o.isum_lo = (uint64_t)sum;
            o.isq_hi = qh, o.isq_lo = ql;
        }
        if (o.n_valid == 0) o.min = o.max = __builtin_nan("");
        out[b] = o;
    }
    return FRS_OK;
}

static int hist_job(frs_ctx *ctx, const frs_raster_desc *d, const void *dev, const double *nodata,
                    const frs_hist_params *hp, uint64_t *counts, frs_band_hist_out *out) {
    const int nb = d->nbands, nbins = hp->nbins;
    const int gx = stats_grid(ctx, d, kHistBlock, kHistUnroll, kHistMaxGroups);
    if (gx == 0) return FRS_E_ARG;
    const StatsParams P = stats_params(d);
    const int64_t bs = nb > 1 ? d->band_stride : 0;
    const HistRange R = hist_range(hp->lo, hp->hi, nbins);
    const int copies = nbins <= kHistCopyBins ? kHistBlock / 64 : 1;
    const size_t lds = std::max((size_t)nbins * copies * sizeof(uint32_t), kHistLdsMin);
    const size_t pbytes = (size_t)nb * gx * sizeof(HistPartial), cbytes = (size_t)nb * nbins * sizeof(uint64_t);
    FRS_HIP(ctx->st_part.ensure(pbytes));
    FRS_HIP(ctx->st_slab.ensure((size_t)nb * gx * nbins * sizeof(uint32_t)));  // every slab is written whole
    FRS_HIP(ctx->st_counts.ensure(cbytes));
    FRS_HIP(ctx->st_pin.ensure(pbytes + cbytes));
    HistPartial *dpart = ctx->st_part.as<HistPartial>();
    uint32_t *slabs = ctx->st_slab.as<uint32_t>();
    const dim3 grid((unsigned)gx, (unsigned)nb);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "band_hist", &ev);
    switch (d->dtype) {
    case FRS_DT_U8: launch_hist<uint8_t>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    case FRS_DT_U16: launch_hist<uint16_t>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    case FRS_DT_I16: launch_hist<int16_t>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    case FRS_DT_I32: launch_hist<int32_t>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    case FRS_DT_U32: launch_hist<uint32_t>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    case FRS_DT_F32: launch_hist<float>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    default: launch_hist<double>(st, grid, lds, dev, P, bs, nodata, R, hp->centre, copies, slabs, dpart); break;
    }
    k_hist_reduce<<<dim3((unsigned)((nbins + 255) / 256), (unsigned)nb), 256, 0, st>>>(slabs, gx, nbins,
                                                                                      ctx->st_counts.as<uint64_t>());
    prof_end(ctx, "band_hist", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipMemcpyAsync(ctx->st_pin.ptr, dpart, pbytes, hipMemcpyDeviceToHost, st));
    FRS_HIP(hipMemcpyAsync(ctx->st_pin.at<char>(pbytes), ctx->st_counts.ptr, cbytes, hipMemcpyDeviceToHost, st));
    FRS_HIP(hipStreamSynchronize(st));
    prof_collect(ctx);

    const bool is_float = d->dtype == FRS_DT_F32 || d->dtype == FRS_DT_F64;
    memcpy(counts, ctx->st_pin.at<char>(pbytes), cbytes);
    const HistPartial *pp = ctx->st_pin.at<HistPartial>(0);
    for (int b = 0; b < nb; b++) {
        frs_band_hist_out o;
        o.below = 0, o.above = 0, o.m2 = 0.0;
        for (int g = 0; g < gx; g++) {  // work-group order
            const HistPartial &q = pp[(size_t)b * gx + g];
            o.below += q.below, o.above += q.above;
            if (is_float) o.m2 = o.m2 + q.m2;
        }
        out[b] = o;
    }
    return FRS_OK;
}

// elements from a raster's origin to the end of its last row, or -1 when that does not fit 63 bits (with room for the
// element size)
static int64_t stats_extent(const frs_raster_desc *d) {
    int64_t x, y;
    if (__builtin_mul_overflow((int64_t)d->nbands - 1, d->nbands > 1 ? d->band_stride : 0, &x) ||
        __builtin_mul_overflow(d->height - 1, d->row_stride, &y) || __builtin_add_overflow(x, y, &x) ||
        __builtin_add_overflow(x, d->width, &x) || x > (INT64_MAX >> 4))
        return -1;
    return x;
}

// the descriptor rules of frs_resample_window* (check_window_desc in frs_window.hip), before anything is sized, copied
// or launched
static int check_stats_desc(frs_ctx *ctx, const frs_raster_desc *d) {
    if (!d) { ctx->err = "null desc"; return FRS_E_ARG; }
    if (d->height < 1 || d->width < 1) { ctx->err = "stats: height and width must be >= 1"; return FRS_E_ARG; }
    if (d->row_stride < d->width) { ctx->err = "row_stride < width"; return FRS_E_ARG; }
    if (d->nbands < 1 || d->nbands > kMaxChannels) { ctx->err = "nbands must be 1..8"; return FRS_E_ARG; }
    if (dtype_size(d->dtype) == 0) { ctx->err = "bad dtype"; return FRS_E_ARG; }
    if (stats_extent(d) < 0) { ctx->err = "stats: raster extent overflows"; return FRS_E_ARG; }
    if (d->nbands > 1 && d->band_stride < (d->height - 1) * d->row_stride + d->width) {
        ctx->err = "band_stride too small";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

static int check_stats_args(frs_ctx *ctx, const frs_raster_desc *d, const void *ptr, const double *nodata,
                            const void *out) {
    if (int rc = check_stats_desc(ctx, d)) return rc;
    if (!ptr || !out || reinterpret_cast<uintptr_t>(ptr) % (uintptr_t)dtype_size(d->dtype)) {
        ctx->err = "stats: null or element-misaligned pointer";
        return FRS_E_ARG;
    }
    if (nodata && !nodata_ok(d->dtype, *nodata)) {
        ctx->err = "stats: nodata must be an integer inside the dtype's range";
        return FRS_E_ARG;
    }
    return FRS_OK;
}

static bool stats_finite(double v) { return v - v == 0.0; }

// frs_band_stats*: every check, then the job on the device raster `ptr`, or (host) on a staged copy of the host raster
static int stats_entry(frs_ctx *ctx, const frs_raster_desc *d, const void *ptr, const double *nodata,
                       frs_band_stats_out *out, bool host) {
    if (!ctx) return FRS_E_ARG;
    if (int rc = check_unsynced(ctx)) return rc;
    if (int rc = check_stats_args(ctx, d, ptr, nodata, out)) return rc;
    if (stats_grid(ctx, d, kStBlock, kStUnroll, kStMaxGroups) == 0) return FRS_E_ARG;
    FRS_HIP(hipSetDevice(ctx->device));
    if (!host) return stats_job(ctx, d, ptr, nodata, out);
    return run_staged(ctx, ptr, (size_t)stats_extent(d) * (size_t)dtype_size(d->dtype),
                      [&](const void *dev) { return stats_job(ctx, d, dev, nodata, out); });
}

static int hist_entry(frs_ctx *ctx, const frs_raster_desc *d, const void *ptr, const double *nodata,
                      const frs_hist_params *hp, uint64_t *counts, frs_band_hist_out *out, bool host) {
    if (!ctx) return FRS_E_ARG;
    if (int rc = check_unsynced(ctx)) return rc;
    if (int rc = check_stats_args(ctx, d, ptr, nodata, out)) return rc;
    if (!hp || !counts) { ctx->err = "stats: null or element-misaligned pointer"; return FRS_E_ARG; }
    if (hp->nbins < 1 || hp->nbins > kHistMaxBins) { ctx->err = "histogram: nbins must be 1..16384"; return FRS_E_ARG; }
    if (!stats_finite(hp->lo) || !stats_finite(hp->hi) || !stats_finite(hp->centre) || !(hp->hi > hp->lo) ||
        !stats_finite(hp->hi - hp->lo) || !stats_finite((double)hp->nbins / (hp->hi - hp->lo))) {
        ctx->err = "histogram: lo, hi, hi - lo, nbins / (hi - lo) and centre must be finite, with hi > lo";
        return FRS_E_ARG;
    }
    if (stats_grid(ctx, d, kHistBlock, kHistUnroll, kHistMaxGroups) == 0) return FRS_E_ARG;
    FRS_HIP(hipSetDevice(ctx->device));
    if (!host) return hist_job(ctx, d, ptr, nodata, hp, counts, out);
    return run_staged(ctx, ptr, (size_t)stats_extent(d) * (size_t)dtype_size(d->dtype),
                      [&](const void *dev) { return hist_job(ctx, d, dev, nodata, hp, counts, out); });
}

}  // namespace frs

extern "C" {

int frs_band_stats_device(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_dev, const double *nodata,
                          frs_band_stats_out *out_host) {
    return frs::stats_entry(ctx, desc, raster_dev, nodata, out_host, false);
}

int frs_band_stats(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_host, const double *nodata,
                   frs_band_stats_out *out_host) {
    return frs::stats_entry(ctx, desc, raster_host, nodata, out_host, true);
}

int frs_band_histogram_device(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_dev, const double *nodata,
                              const frs_hist_params *params, uint64_t *counts_host, frs_band_hist_out *out_host) {
    return frs::hist_entry(ctx, desc, raster_dev, nodata, params, counts_host, out_host, false);
}

int frs_band_histogram(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_host, const double *nodata,
                       const frs_hist_params *params, uint64_t *counts_host, frs_band_hist_out *out_host) {
    return frs::hist_entry(ctx, desc, raster_host, nodata, params, counts_host, out_host, true);
}

}  // extern "C"
