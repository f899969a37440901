// frs_compare.hip -- fused difference statistics of two rasters (frs_compare*): one streaming pass over both.
//
// Reference path replaced (Youssef-Harby/flac-raster): compare.py:55-78 -- np.array_equal, np.max(np.abs(a-b)),
// np.mean(np.abs(a-b)), np.sqrt(np.mean((a-b)**2)), np.min / np.max of each file, overall and per band: about twenty
// whole-array numpy passes with temporaries.  Here every band is read once.
//
//   k_compare   grid (gx, nbands), 256 threads.  Work-group (g, band) walks the band's 16-byte vector pairs in chunks
//               of kCmpUnroll x 256 vectors with stride gx chunks (grid-stride), then its share of the elements the
//               vectors do not cover (head / tail of a run, or everything when the runs are not 16-byte aligned),
//               reduces lane -> wave (shuffles) -> work-group (LDS) and writes ONE CmpPartial record.  No atomics, no
//               hand-off between work-groups: the host adds the gx records of a band in work-group order.
//
// The grid is a function of (height, width, nbands, dtype) only -- never of the CU count or the environment -- so the
// float sums (whose value depends on the summation tree) reproduce run to run and machine to machine.
//
// Integer exactness: every per-element term (the wrapped |a-b| and (a-b)^2 in T, the true |a-b|) has magnitude
// <= 2^32, and compare_job rejects shapes in which one work-group would fold more than kCmpMaxPerGroup = 2^30 elements,
// so a work-group's int64 partial has magnitude <= 2^62 and cannot overflow.  The host adds the partials in __int128
// and converts to double once: the result is the correctly rounded exact sum.
#include <algorithm>
#include <limits>
#include <type_traits>

#include "frs_internal.h"

namespace frs {

constexpr int kCmpBlock = 256;           // threads per work-group
constexpr int kCmpUnroll = 4;            // 16-byte loads in flight per lane and raster
constexpr int kCmpMaxGroups = 2048;      // cap of gx * nbands (grid-stride beyond it)
constexpr int kCmpChunkVecs = kCmpBlock * kCmpUnroll;          // 16-byte vectors per work-group step
constexpr int64_t kCmpMaxPerGroup = (int64_t)1 << 30;          // elements one work-group may fold (see above)
// (flac_raster_amd/_native.py mirrors kCmpBlock / kCmpUnroll / kCmpMaxGroups for the tests' shape arithmetic)

template <int DT> struct CmpElem;
template <> struct CmpElem<FRS_DT_U8> { using T = uint8_t; };
template <> struct CmpElem<FRS_DT_U16> { using T = uint16_t; };
template <> struct CmpElem<FRS_DT_I16> { using T = int16_t; };
template <> struct CmpElem<FRS_DT_I32> { using T = int32_t; };
template <> struct CmpElem<FRS_DT_U32> { using T = uint32_t; };
template <> struct CmpElem<FRS_DT_F32> { using T = float; };
template <> struct CmpElem<FRS_DT_F64> { using T = double; };

union CmpVal {
    int64_t i;  // integer dtypes
    double f;   // float dtypes
};

// one work-group's partial of one band
struct CmpPartial {
    int64_t n_diff;
    int64_t first_diff;  // smallest row * width + col with a != b, INT64_MAX when none
    CmpVal a_min, a_max, b_min, b_max;
    CmpVal np_max;       // max of the wrapped |a - b| (a value of T)
    CmpVal np_sum_abs, np_sum_sq;
    CmpVal max_abs, sum_abs;  // true |a - b|
    int64_t nan;         // float dtypes: bit 0 a holds a NaN, bit 1 b holds one, bit 2 some a - b is NaN
};

struct CmpParams {
    int64_t height, width;
    int64_t a_row_stride, a_band_stride, b_row_stride, b_band_stride;
    int32_t dense;  // both rasters dense: a band is one flat run of height * width elements
};

typedef short cmp_v2i16 __attribute__((ext_vector_type(2)));
typedef unsigned short cmp_v2u16 __attribute__((ext_vector_type(2)));

// per-lane accumulators
template <typename T, bool F = std::is_floating_point_v<T>> struct CmpAcc;

template <typename T> struct CmpAcc<T, false> {
    static constexpr bool kSmall = sizeof(T) <= 2;
    static constexpr int VE = 16 / (int)sizeof(T);
    using U = std::make_unsigned_t<T>;
    using W = std::conditional_t<kSmall, int32_t, int64_t>;  // holds any true |a - b|
    using M = std::conditional_t<kSmall, int32_t, T>;        // holds any value of T (min / max, the wrapped |a - b|)
    using V = std::conditional_t<std::is_signed_v<T>, cmp_v2i16, cmp_v2u16>;
    using E16 = std::conditional_t<std::is_signed_v<T>, short, unsigned short>;
    uint32_t nd = 0;  // <= kCmpMaxPerGroup per lane
    int64_t first = INT64_MAX;
    bool any_equal = false;  // some vector pair had equal bits (its zero terms were skipped)
    M amin = std::numeric_limits<T>::max(), amax = std::numeric_limits<T>::lowest();
    M bmin = std::numeric_limits<T>::max(), bmax = std::numeric_limits<T>::lowest();
    M npmax = std::numeric_limits<T>::lowest();
    W tmax = 0;
    int64_t s_abs = 0, s_sq = 0, s_true = 0;
    // packed 16-bit min / max of the vector path (8/16-bit dtypes; u8 widened into 16-bit halves: exact)
    V pamin = (V)(E16)std::numeric_limits<E16>::max(), pamax = (V)(E16)std::numeric_limits<E16>::lowest();
    V pbmin = (V)(E16)std::numeric_limits<E16>::max(), pbmax = (V)(E16)std::numeric_limits<E16>::lowest();

    // difference terms of one element pair (a - b, |.| and the square all wrap in T as numpy's do)
    template <typename S> __host__ __device__ inline void diff(T a, T b, int64_t lin, S &sa, S &sq, S &st) {
        const bool ne = a != b;
        nd += ne ? 1u : 0u;
        if (ne && lin < first) first = lin;
        const T d = (T)((U)a - (U)b);
        T ad = d;
        if constexpr (std::is_signed_v<T>) ad = d < 0 ? (T)((U)0 - (U)d) : d;  // abs(min) stays min
        const T dd = (T)((uint32_t)(U)d * (uint32_t)(U)d);
        W t = (W)a - (W)b;
        t = t < 0 ? -t : t;
        npmax = (M)ad > npmax ? (M)ad : npmax;
        tmax = t > tmax ? t : tmax;
        sa += (S)ad;
        sq += (S)dd;
        st += (S)t;
    }
    __host__ __device__ inline void elem(T a, T b, int64_t lin) {
        amin = (M)a < amin ? (M)a : amin;
        amax = (M)a > amax ? (M)a : amax;
        bmin = (M)b < bmin ? (M)b : bmin;
        bmax = (M)b > bmax ? (M)b : bmax;
        diff(a, b, lin, s_abs, s_sq, s_true);
    }
    __host__ __device__ inline void fold16(uint32_t w, V &mn, V &mx) {
        if constexpr (sizeof(T) == 2) {
            const V v = __builtin_bit_cast(V, w);
            mn = __builtin_elementwise_min(mn, v);
            mx = __builtin_elementwise_max(mx, v);
        } else {
            const V lo = __builtin_bit_cast(V, w & 0x00FF00FFu), hi = __builtin_bit_cast(V, (w >> 8) & 0x00FF00FFu);
            mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(lo, hi));
            mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(lo, hi));
        }
    }
    // one 16-byte vector pair whose first element has linear index lin
    __host__ __device__ inline void vec(const uint4 &qa, const uint4 &qb, int64_t lin) {
        T ea[VE], eb[VE];
        __builtin_memcpy(ea, &qa, 16);
        __builtin_memcpy(eb, &qb, 16);
        if constexpr (kSmall) {
            fold16(qa.x, pamin, pamax), fold16(qa.y, pamin, pamax), fold16(qa.z, pamin, pamax), fold16(qa.w, pamin, pamax);
            fold16(qb.x, pbmin, pbmax), fold16(qb.y, pbmin, pbmax), fold16(qb.z, pbmin, pbmax), fold16(qb.w, pbmin, pbmax);
        } else {
#pragma unroll
            for (int k = 0; k < VE; k++) {
                amin = (M)ea[k] < amin ? (M)ea[k] : amin;
                amax = (M)ea[k] > amax ? (M)ea[k] : amax;
                bmin = (M)eb[k] < bmin ? (M)eb[k] : bmin;
                bmax = (M)eb[k] > bmax ? (M)eb[k] : bmax;
            }
        }
        // integer vectors with equal bits differ nowhere: every difference term is 0 (np_max's 0 is folded at the end)
        if (((qa.x ^ qb.x) | (qa.y ^ qb.y) | (qa.z ^ qb.z) | (qa.w ^ qb.w)) == 0) {
            any_equal = true;
            return;
        }
        if constexpr (kSmall) {
            int32_t sa = 0, sq = 0, st = 0;  // <= 16 terms of magnitude <= 2^16
#pragma unroll
            for (int k = 0; k < VE; k++) diff(ea[k], eb[k], lin + k, sa, sq, st);
            s_abs += sa;
            s_sq += sq;
            s_true += st;
        } else {
#pragma unroll
            for (int k = 0; k < VE; k++) diff(ea[k], eb[k], lin + k, s_abs, s_sq, s_true);
        }
    }
    __host__ __device__ inline void finish() {
        if (any_equal && npmax < 0) npmax = 0;  // the skipped terms' |0| (npmax can only be below 0 for signed T)
        if constexpr (kSmall) {
            amin = min(amin, min((int32_t)pamin.x, (int32_t)pamin.y));
            amax = max(amax, max((int32_t)pamax.x, (int32_t)pamax.y));
            bmin = min(bmin, min((int32_t)pbmin.x, (int32_t)pbmin.y));
            bmax = max(bmax, max((int32_t)pbmax.x, (int32_t)pbmax.y));
        }
    }
};

template <typename T> struct CmpAcc<T, true> {
    static constexpr int VE = 16 / (int)sizeof(T);
    uint32_t nd = 0;
    int64_t first = INT64_MAX;
    int32_t nan = 0;
    // NaN-ignoring min / max plus the NaN flags: the host turns a flagged band's values into NaN (np.min propagates)
    double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
    double npmax = -INFINITY, tmax = -INFINITY;
    double s_abs = 0.0, s_sq = 0.0, s_true = 0.0;
    __host__ __device__ inline void elem(T a, T b, int64_t lin) {
        nan |= (a != a ? 1 : 0) | (b != b ? 2 : 0);
        amin = fmin(amin, (double)a);
        amax = fmax(amax, (double)a);
        bmin = fmin(bmin, (double)b);
        bmax = fmax(bmax, (double)b);
        const bool ne = a != b;  // NaN differs from everything, -0.0 == 0.0
        nd += ne ? 1u : 0u;
        if (ne && lin < first) first = lin;
        const T d = a - b;       // in T
        const T ad = d < 0 ? -d : d;
        const T dd = d * d;      // in T (-ffp-contract=off: a separate rounded product)
        nan |= d != d ? 4 : 0;
        double t = (double)a - (double)b;
        t = t < 0 ? -t : t;
        npmax = fmax(npmax, (double)ad);
        tmax = fmax(tmax, t);
        s_abs += (double)ad;     // a NaN term makes the sum NaN, as numpy's
        s_sq += (double)dd;
        s_true += t;
    }
    __host__ __device__ inline void vec(const uint4 &qa, const uint4 &qb, int64_t lin) {
        T ea[VE], eb[VE];
        __builtin_memcpy(ea, &qa, 16);
        __builtin_memcpy(eb, &qb, 16);
#pragma unroll
        for (int k = 0; k < VE; k++) elem(ea[k], eb[k], lin + k);
    }
    __host__ __device__ inline void finish() {}
};

__device__ inline int64_t cmp_wave_sum(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline double cmp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int64_t cmp_wave_min(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ inline int64_t cmp_wave_max(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ inline double cmp_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ inline double cmp_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// One lane's share of a band: work-group g of gx, lane tid.  a0 / b0 are the band's origins.  (Plain C++, so that a
// host program can run it element for element against a direct evaluation.)
template <typename T>
__host__ __device__ inline void cmp_fold(CmpAcc<T> &acc, const T *a0, const T *b0, const CmpParams &P, int g, int gx,
                                         int tid) {
    constexpr int ES = (int)sizeof(T), VE = 16 / ES;
    // runs: the whole band when dense, else its rows
    const int64_t seg_len = P.dense ? P.height * P.width : P.width;
    const int64_t nseg = P.dense ? 1 : P.height;
    const int64_t a_ss = P.dense ? 0 : P.a_row_stride, b_ss = P.dense ? 0 : P.b_row_stride;
    const unsigned ma = (unsigned)(reinterpret_cast<uintptr_t>(a0) & 15), mb = (unsigned)(reinterpret_cast<uintptr_t>(b0) & 15);
    // 16-byte loads need both runs aligned at the same element: a dense band after a scalar head when A and B are
    // misaligned alike; rows when every row start of both rasters is aligned.  Anything else takes the scalar loop.
    const bool vec_ok = P.dense ? ma == mb
                                : (ma == 0 && mb == 0 && (P.a_row_stride * ES) % 16 == 0 && (P.b_row_stride * ES) % 16 == 0);
    int64_t head = seg_len;
    if (vec_ok) {
        head = ((16 - ma) & 15) / ES;
        head = head < seg_len ? head : seg_len;
    }
    const int64_t nvec = (seg_len - head) / VE;       // vectors per run
    const int64_t body_end = head + nvec * VE;
    const int64_t per_s = seg_len - nvec * VE;        // scalar elements per run (head + tail)
    const int64_t V = nseg * nvec, S = nseg * per_s;  // vector / scalar items of the band

    // ---- vector body
    auto load = [&](int64_t idx, uint4 &qa, uint4 &qb) -> int64_t {
        int64_t seg = 0, v = idx;
        if (nseg > 1) {
            seg = idx / nvec;
            v = idx - seg * nvec;
        }
        const int64_t p = head + v * VE;
        qa = *reinterpret_cast<const uint4 *>(a0 + seg * a_ss + p);
        qb = *reinterpret_cast<const uint4 *>(b0 + seg * b_ss + p);
        return seg * seg_len + p;
    };
    for (int64_t base = (int64_t)g * kCmpChunkVecs; base < V; base += (int64_t)gx * kCmpChunkVecs) {
        if (base + kCmpChunkVecs <= V) {
            uint4 qa[kCmpUnroll], qb[kCmpUnroll];
            int64_t lin[kCmpUnroll];
#pragma unroll
            for (int u = 0; u < kCmpUnroll; u++) lin[u] = load(base + u * kCmpBlock + tid, qa[u], qb[u]);
#pragma unroll
            for (int u = 0; u < kCmpUnroll; u++) acc.vec(qa[u], qb[u], lin[u]);
        } else {
            for (int64_t idx = base + tid; idx < V; idx += kCmpBlock) {
                uint4 qa, qb;
                const int64_t lin = load(idx, qa, qb);
                acc.vec(qa, qb, lin);
            }
        }
    }
    // ---- scalar items: head and tail of every run (everything when the runs are not vectorised)
    for (int64_t s = (int64_t)g * kCmpBlock + tid; s < S; s += (int64_t)gx * kCmpBlock) {
        int64_t seg = 0, j = s;
        if (nseg > 1) {
            seg = s / per_s;
            j = s - seg * per_s;
        }
        const int64_t p = j < head ? j : body_end + (j - head);
        acc.elem(a0[seg * a_ss + p], b0[seg * b_ss + p], seg * seg_len + p);
    }
    acc.finish();
}

template <int DT>
__global__ void __launch_bounds__(kCmpBlock) k_compare(const typename CmpElem<DT>::T *A, const typename CmpElem<DT>::T *B,
                                                      CmpParams P, CmpPartial *out) {
    using T = typename CmpElem<DT>::T;
    constexpr bool F = std::is_floating_point_v<T>;
    const int band = blockIdx.y;
    const int gx = gridDim.x, g = blockIdx.x, tid = threadIdx.x;
    const T *a0 = A + (int64_t)band * P.a_band_stride;
    const T *b0 = B + (int64_t)band * P.b_band_stride;
    CmpAcc<T> acc;
    cmp_fold(acc, a0, b0, P, g, gx, tid);

    // ---- lane -> wave -> work-group
    CmpPartial r;
    r.n_diff = cmp_wave_sum((int64_t)acc.nd);
    r.first_diff = cmp_wave_min(acc.first);
    if constexpr (F) {
        r.a_min.f = cmp_wave_min(acc.amin), r.a_max.f = cmp_wave_max(acc.amax);
        r.b_min.f = cmp_wave_min(acc.bmin), r.b_max.f = cmp_wave_max(acc.bmax);
        r.np_max.f = cmp_wave_max(acc.npmax), r.max_abs.f = cmp_wave_max(acc.tmax);
        r.np_sum_abs.f = cmp_wave_sum(acc.s_abs), r.np_sum_sq.f = cmp_wave_sum(acc.s_sq);
        r.sum_abs.f = cmp_wave_sum(acc.s_true);
        // (the max of a bit set is not its OR: fold the three flags separately)
        r.nan = cmp_wave_max((int64_t)(acc.nan & 1)) | cmp_wave_max((int64_t)(acc.nan & 2)) |
                cmp_wave_max((int64_t)(acc.nan & 4));
    } else {
        r.a_min.i = cmp_wave_min((int64_t)acc.amin), r.a_max.i = cmp_wave_max((int64_t)acc.amax);
        r.b_min.i = cmp_wave_min((int64_t)acc.bmin), r.b_max.i = cmp_wave_max((int64_t)acc.bmax);
        r.np_max.i = cmp_wave_max((int64_t)acc.npmax), r.max_abs.i = cmp_wave_max((int64_t)acc.tmax);
        r.np_sum_abs.i = cmp_wave_sum(acc.s_abs), r.np_sum_sq.i = cmp_wave_sum(acc.s_sq);
        r.sum_abs.i = cmp_wave_sum(acc.s_true);
        r.nan = 0;
    }
    __shared__ CmpPartial wp[kCmpBlock / 64];
    if ((tid & 63) == 0) wp[tid >> 6] = r;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kCmpBlock / 64; w++) {  // waves in order
            const CmpPartial q = wp[w];
            r.n_diff += q.n_diff;
            r.first_diff = q.first_diff < r.first_diff ? q.first_diff : r.first_diff;
            r.nan |= q.nan;
            if constexpr (F) {
                r.a_min.f = fmin(r.a_min.f, q.a_min.f), r.a_max.f = fmax(r.a_max.f, q.a_max.f);
                r.b_min.f = fmin(r.b_min.f, q.b_min.f), r.b_max.f = fmax(r.b_max.f, q.b_max.f);
                r.np_max.f = fmax(r.np_max.f, q.np_max.f), r.max_abs.f = fmax(r.max_abs.f, q.max_abs.f);
                r.np_sum_abs.f += q.np_sum_abs.f, r.np_sum_sq.f += q.np_sum_sq.f, r.sum_abs.f += q.sum_abs.f;
            } else {
                r.a_min.i = q.a_min.i < r.a_min.i ? q.a_min.i : r.a_min.i;
                r.a_max.i = q.a_max.i > r.a_max.i ? q.a_max.i : r.a_max.i;
                r.b_min.i = q.b_min.i < r.b_min.i ? q.b_min.i : r.b_min.i;
                r.b_max.i = q.b_max.i > r.b_max.i ? q.b_max.i : r.b_max.i;
                r.np_max.i = q.np_max.i > r.np_max.i ? q.np_max.i : r.np_max.i;
                r.max_abs.i = q.max_abs.i > r.max_abs.i ? q.max_abs.i : r.max_abs.i;
                r.np_sum_abs.i += q.np_sum_abs.i, r.np_sum_sq.i += q.np_sum_sq.i, r.sum_abs.i += q.sum_abs.i;
            }
        }
        out[(int64_t)band * gx + g] = r;
    }
}

template <int DT>
static void launch_compare(hipStream_t st, dim3 grid, const void *a, const void *b, const CmpParams &P, CmpPartial *out) {
    using T = typename CmpElem<DT>::T;
    k_compare<DT><<<grid, kCmpBlock, 0, st>>>(static_cast<const T *>(a), static_cast<const T *>(b), P, out);
}

// Work-groups per band: one per chunk of kCmpChunkVecs 16-byte vectors, capped so that gx * nbands stays near
// kCmpMaxGroups.  A function of the shape and the element size only.
static int64_t compare_groups(int64_t count, int nbands, int es) {
    const int64_t chunk = (int64_t)kCmpChunkVecs * (16 / es);
    const int64_t want = (count + chunk - 1) / chunk;
    const int64_t cap = std::max<int64_t>(1, kCmpMaxGroups / nbands);
    return std::max<int64_t>(1, std::min(want, cap));
}

int compare_job(frs_ctx *ctx, const frs_compare_desc *d, const void *a_dev, const void *b_dev, frs_compare_band *out) {
    const int es = dtype_size(d->dtype);
    const int nb = d->nbands;
    const int64_t count = d->height * d->width;
    const int gx = (int)compare_groups(count, nb, es);
    // a work-group folds at most this many elements (its grid-stride share of the vectors and of the scalar items,
    // each rounded up to a whole step): the int64 partial sums then stay below 2^62 (file header)
    const int64_t per_group = (count + gx - 1) / gx + (int64_t)kCmpChunkVecs * (16 / es) + kCmpBlock;
    if (per_group > kCmpMaxPerGroup) {
        ctx->err = "compare: more than 2^30 elements per work-group (a 64-bit partial sum could overflow)";
        return FRS_E_ARG;
    }
    CmpParams P;
    P.height = d->height, P.width = d->width;
    P.a_row_stride = d->a_row_stride, P.a_band_stride = d->a_band_stride;
    P.b_row_stride = d->b_row_stride, P.b_band_stride = d->b_band_stride;
    auto dense = [&](int64_t rs, int64_t bs) { return rs == d->width && (nb == 1 || bs == count); };
    P.dense = dense(d->a_row_stride, d->a_band_stride) && dense(d->b_row_stride, d->b_band_stride);
    const size_t nrec = (size_t)nb * gx, bytes = nrec * sizeof(CmpPartial);
    FRS_HIP(ctx->cmp_part.ensure(bytes));  // every record is written by its work-group: no init pass
    FRS_HIP(ctx->cmp_pin.ensure(bytes));
    CmpPartial *dpart = ctx->cmp_part.as<CmpPartial>();
    const dim3 grid((unsigned)gx, (unsigned)nb);
    hipEvent_t ev;
    prof_begin(ctx, "compare", &ev);
    switch (d->dtype) {
    case FRS_DT_U8: launch_compare<FRS_DT_U8>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    case FRS_DT_U16: launch_compare<FRS_DT_U16>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    case FRS_DT_I16: launch_compare<FRS_DT_I16>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    case FRS_DT_I32: launch_compare<FRS_DT_I32>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    case FRS_DT_U32: launch_compare<FRS_DT_U32>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    case FRS_DT_F32: launch_compare<FRS_DT_F32>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    default: launch_compare<FRS_DT_F64>(ctx->stream, grid, a_dev, b_dev, P, dpart); break;
    }
    prof_end(ctx, "compare", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipMemcpyAsync(ctx->cmp_pin.ptr, dpart, bytes, hipMemcpyDeviceToHost, ctx->stream));
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);

    const bool is_float = d->dtype == FRS_DT_F32 || d->dtype == FRS_DT_F64;
    const CmpPartial *hp = ctx->cmp_pin.at<CmpPartial>(0);
    for (int b = 0; b < nb; b++) {
        const CmpPartial *p = hp + (size_t)b * gx;
        frs_compare_band &o = out[b];
        o.count = count;
        int64_t nd = 0, first = INT64_MAX;
        for (int g = 0; g < gx; g++) {
            nd += p[g].n_diff;
            first = std::min(first, p[g].first_diff);
        }
        o.n_diff = nd;
        o.first_diff = first == INT64_MAX ? -1 : first;
        if (is_float) {
            double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY, npm = -INFINITY, tm = -INFINITY;
            double sa = 0.0, sq = 0.0, st = 0.0;
            int64_t nan = 0;
            for (int g = 0; g < gx; g++) {  // work-group order
                amin = std::min(amin, p[g].a_min.f), amax = std::max(amax, p[g].a_max.f);
                bmin = std::min(bmin, p[g].b_min.f), bmax = std::max(bmax, p[g].b_max.f);
                npm = std::max(npm, p[g].np_max.f), tm = std::max(tm, p[g].max_abs.f);
                sa += p[g].np_sum_abs.f, sq += p[g].np_sum_sq.f, st += p[g].sum_abs.f;
                nan |= p[g].nan;
            }
            const double qnan = __builtin_nan("");
            o.a_min = nan & 1 ? qnan : amin, o.a_max = nan & 1 ? qnan : amax;
            o.b_min = nan & 2 ? qnan : bmin, o.b_max = nan & 2 ? qnan : bmax;
            o.np_max_abs = nan & 4 ? qnan : npm, o.max_abs = nan & 4 ? qnan : tm;
            o.np_sum_abs = sa, o.np_sum_sq = sq, o.sum_abs = st;
        } else {
            int64_t amin = INT64_MAX, amax = INT64_MIN, bmin = INT64_MAX, bmax = INT64_MIN, npm = INT64_MIN, tm = 0;
            __int128 sa = 0, sq = 0, st = 0;
            for (int g = 0; g < gx; g++) {
                amin = std::min(amin, p[g].a_min.i), amax = std::max(amax, p[g].a_max.i);
                bmin = std::min(bmin, p[g].b_min.i), bmax = std::max(bmax, p[g].b_max.i);
                npm = std::max(npm, p[g].np_max.i), tm = std::max(tm, p[g].max_abs.i);
                sa += p[g].np_sum_abs.i, sq += p[g].np_sum_sq.i, st += p[g].sum_abs.i;
            }
            o.a_min = (double)amin, o.a_max = (double)amax, o.b_min = (double)bmin, o.b_max = (double)bmax;
            o.np_max_abs = (double)npm, o.max_abs = (double)tm;
            o.np_sum_abs = (double)sa, o.np_sum_sq = (double)sq, o.sum_abs = (double)st;  // one rounding each
        }
    }
    return FRS_OK;
}

}  // namespace frs
