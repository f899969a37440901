// frs_stats.h -- the arithmetic of the band statistics and of the band histogram (frs_band_stats*, frs_band_histogram*),
// written once for the host and the device.  Includes nothing from HIP, only the header whose predicate it uses: a plain
// C++ compiler builds it (tests/test_stats_host.py compares the bin rule, the 128-bit carries and the lane functions,
// run lane by lane, with the restatement in tests/stats_ref.py), hipcc builds the same text as __host__ __device__.
// Needs -ffp-contract=off like the rest of the library: every operator below is one IEEE operation.  Users:
// k_band_stats and k_band_histogram in frs_stats.hip, which keep their own wave and work-group reductions.
//
// The definitions are the project's own.
//
// Validity.  With a nodata value nd given (ndT = (T)nd, frs_nodata.h), a pixel v with nd_is(v, ndT) is NODATA.
// Otherwise, for a float dtype, v != v makes it NAN.  Otherwise it is VALID; +-inf are valid values.  Without a nodata
// value no pixel is nodata.  The three classes are counted; everything else below is over the valid pixels alone.
//
// Per-pixel accumulation.  min and max are kept in the dtype (widened: exact).  Integer dtypes: the sum s and the sum of
// squares q are exact.  A lane, a wave and a work-group fold at most 2^30 elements (the entry points reject larger
// shares), so s, of terms below 2^32 in magnitude, fits an int64; q of an 8/16-bit dtype (terms < 2^32) fits a uint64;
// a 32-bit v^2 reaches 2^64, so there q is an unsigned 128-bit value kept as two 64-bit words (hi, lo) with an explicit
// carry: add_u128(hi, lo, x), the one function the lane, wave, work-group and host steps all use.  Float dtypes: an fp64
// sum of (double)v, sum = sum + (double)v, in the order the lane meets the pixels; no sum of squares (see below).
//
// Bin rule.  Given finite doubles lo < hi with hi - lo finite, and nbins >= 1: scale = (double)nbins / (hi - lo),
// computed once.  For a valid pixel x = (double)v:  x < lo counts in `below`;  x > hi counts in `above`;  otherwise
// b = (int64)floor((x - lo) * scale), and b >= nbins becomes nbins - 1 (x == hi, or a product that rounded up).
// With lo = m, hi = M + 1, nbins = M - m + 1 for integers m <= M, scale is exactly 1 and every integer value m .. M has
// a bin of its own.
//
// Centred square sum.  Float dtypes only: m2 = m2 + (x - centre) * (x - centre) over the valid pixels, in the lane's
// order (the second pass, with centre = the mean of the first: sqrt(m2 / n) is the population deviation without the
// cancellation of q / n - mean^2).  Integer dtypes have the exact q instead; their m2 is 0.
//
// The lane function.  stats_fold walks one lane's share of one band and hands every pixel inside [height][width] to an
// accumulator, and nothing else: a band is a set of runs (its rows, or the whole band when it is dense), a run is cut
// at the 16-byte boundaries of memory into windows, and window c of run r is item r * C + c, C being the windows a run
// can touch whatever its alignment.  Work-group g of gx takes the items [g, g + gx, ...) * BLOCK * UNROLL + u * BLOCK +
// tid, u ascending.  A window wholly inside its run is read with one aligned 16-byte load; a window the run begins or
// ends in (head and tail) is read element by element, only the elements inside the run.
#pragma once
#include <stdint.h>

#include "frs_nodata.h"

namespace frs {

// ---- validity
constexpr int kStatsValid = 0, kStatsNodata = 1, kStatsNan = 2;

template <typename T, bool MASKED> FRS_HD inline int stats_class(T v, T nd) {
    if (MASKED && nd_is(v, nd)) return kStatsNodata;
    if constexpr (NdFloat<T>::value) {
        if (v != v) return kStatsNan;
    }
    return kStatsValid;
}

// ---- 128-bit unsigned accumulation: (hi, lo) += x
FRS_HD inline void add_u128(uint64_t &hi, uint64_t &lo, uint64_t x) {
    lo = lo + x;
    hi = hi + (lo < x ? 1u : 0u);
}
// (hi, lo) += (xhi, xlo)
FRS_HD inline void add_u128(uint64_t &hi, uint64_t &lo, uint64_t xhi, uint64_t xlo) {
    hi = hi + xhi;
    add_u128(hi, lo, xlo);
}

// ---- the bin rule
struct HistRange {
    double lo, hi, scale;
    int32_t nbins;
};
FRS_HD inline HistRange hist_range(double lo, double hi, int32_t nbins) {
    HistRange r;
    r.lo = lo, r.hi = hi, r.nbins = nbins;
    r.scale = (double)nbins / (hi - lo);
    return r;
}
constexpr int32_t kHistBelow = -1, kHistAbove = -2;
// the bin of a valid pixel's x (never NaN), or kHistBelow / kHistAbove
FRS_HD inline int32_t hist_bin(const HistRange &r, double x) {
    if (x < r.lo) return kHistBelow;
    if (x > r.hi) return kHistAbove;
    // lo <= x <= hi: the product is at most nbins (1 + 2^-52), so the rule's (int64)floor(.) fits 32 bits
    const int32_t b = (int32_t)__builtin_floor((x - r.lo) * r.scale);
    return b >= r.nbins ? r.nbins - 1 : b;
}

// ---- per-dtype types: M holds any value of T (min / max)
template <typename T> struct StatsTraits;
template <> struct StatsTraits<uint8_t> { using M = int32_t; static constexpr bool wide = false; };
template <> struct StatsTraits<uint16_t> { using M = int32_t; static constexpr bool wide = false; };
template <> struct StatsTraits<int16_t> { using M = int32_t; static constexpr bool wide = false; };
template <> struct StatsTraits<int32_t> { using M = int32_t; static constexpr bool wide = true; };
template <> struct StatsTraits<uint32_t> { using M = uint32_t; static constexpr bool wide = true; };

// one aligned 16-byte window of memory
struct alignas(16) StatsVec {
    uint32_t x, y, z, w;
};

// ---- the accumulators of the first pass (one lane's)
template <typename T, bool MASKED, bool F = NdFloat<T>::value> struct StatsAcc;

template <typename T, bool MASKED> struct StatsAcc<T, MASKED, false> {
    static constexpr int VE = 16 / (int)sizeof(T);
    using M = typename StatsTraits<T>::M;
    T nd = 0;
    uint32_t n_valid = 0, n_nodata = 0;  // <= 2^30 per lane
    static constexpr uint32_t n_nan = 0;
    M mn = (M)WinLimits<T>::hi, mx = (M)WinLimits<T>::lo;
    int64_t sum = 0;
    uint64_t sq_hi = 0, sq_lo = 0;
    // (branch-free: a pixel that is not valid contributes 0 to every sum and leaves min / max alone)
    FRS_HD inline void elem(T v) {
        const bool ok = stats_class<T, MASKED>(v, nd) == kStatsValid;
        n_valid += ok ? 1u : 0u;
        n_nodata += ok ? 0u : 1u;
        mn = ok && (M)v < mn ? (M)v : mn;
        mx = ok && (M)v > mx ? (M)v : mx;
        if constexpr (StatsTraits<T>::wide) {
            const int64_t w = ok ? (int64_t)v : 0;
            sum += w;
            add_u128(sq_hi, sq_lo, (uint64_t)w * (uint64_t)w);  // |w| <= 2^32 - 1: the product is w^2 mod 2^64 = w^2
        } else {
            const uint32_t w = ok ? (uint32_t)(int32_t)v : 0u;
            sum += (int64_t)(int32_t)w;
            sq_lo += (uint64_t)(uint32_t)(w * w);  // w^2 < 2^32 for every 8/16-bit value (two's complement: exact)
        }
    }
    // one window: the 8/16-bit dtypes add its <= 16 terms in 32 bits first (|sum| < 2^20; the squares stay 64-bit)
    FRS_HD inline void vec(const StatsVec &q) {
        T e[VE];
        __builtin_memcpy(e, &q, 16);
        if constexpr (StatsTraits<T>::wide) {
            for (int k = 0; k < VE; k++) elem(e[k]);
        } else {
            int32_t s = 0;
            uint32_t nv = 0;
            for (int k = 0; k < VE; k++) {
                const bool ok = stats_class<T, MASKED>(e[k], nd) == kStatsValid;
                const int32_t w = ok ? (int32_t)e[k] : 0;
                nv += ok ? 1u : 0u;
                mn = ok && w < mn ? w : mn;
                mx = ok && w > mx ? w : mx;
                s += w;
                sq_lo += (uint64_t)((uint32_t)w * (uint32_t)w);
            }
            n_valid += nv, n_nodata += (uint32_t)VE - nv;
            sum += (int64_t)s;
        }
    }
    FRS_HD inline void finish() {}
};

template <typename T, bool MASKED> struct StatsAcc<T, MASKED, true> {
    static constexpr int VE = 16 / (int)sizeof(T);
    T nd = 0;
    uint32_t n_valid = 0, n_nodata = 0, n_nan = 0;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    double sum = 0.0;
    FRS_HD inline void elem(T v) {
        const int c = stats_class<T, MASKED>(v, nd);
        if (c != kStatsValid) {
            if (c == kStatsNodata) n_nodata += 1u;
            else n_nan += 1u;
            return;
        }
        const double x = (double)v;
        n_valid += 1u;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        sum = sum + x;
    }
    FRS_HD inline void vec(const StatsVec &q) {
        T e[VE];
        __builtin_memcpy(e, &q, 16);
        for (int k = 0; k < VE; k++) elem(e[k]);
    }
    FRS_HD inline void finish() {}
};

// ---- the accumulators of the second pass (one lane's).  Sink takes the counts: sink.add(bin, n) adds n to the bin's
// counter (the device's is an LDS atomic, a host program's a plain array).  Equal bins that follow one another in the
// lane's order are merged into one add.
template <typename T, bool MASKED, typename Sink> struct HistAcc {
    static constexpr int VE = 16 / (int)sizeof(T);
    HistRange r;
    double centre = 0.0;
    T nd = 0;
    Sink sink;
    uint32_t below = 0, above = 0;  // <= 2^30 per lane
    double m2 = 0.0;
    int32_t run_bin = kHistBelow;   // the pending run: run_n pixels of run_bin
    uint32_t run_n = 0;
    FRS_HD inline void flush() {
        if (run_n) sink.add(run_bin, run_n);
        run_n = 0;
    }
    // (one branch per pixel, the flush of a finished run: everything else is selects.  A pixel that is not counted
    // into a bin takes lo's place in the bin arithmetic, so that the conversion below always has an operand in range.)
    FRS_HD inline void elem(T v) {
        const bool ok = stats_class<T, MASKED>(v, nd) == kStatsValid;
        const double x = (double)v;
        if constexpr (NdFloat<T>::value) {
            const double d = x - centre;
            m2 = ok ? m2 + d * d : m2;
        }
        const bool lt = ok && x < r.lo, gt = ok && x > r.hi;
        const bool in = ok && !lt && !gt;
        below += lt ? 1u : 0u;
        above += gt ? 1u : 0u;
        const int32_t b = hist_bin(r, in ? x : r.lo);
        if (in && b != run_bin) {
            flush();
            run_bin = b;
        }
        run_n += in ? 1u : 0u;
    }
    FRS_HD inline void vec(const StatsVec &q) {
        T e[VE];
        __builtin_memcpy(e, &q, 16);
        for (int k = 0; k < VE; k++) elem(e[k]);
    }
    FRS_HD inline void finish() { flush(); }
};

// ---- the lane function
struct StatsParams {
    int64_t height, width;
    int64_t row_stride;
    int32_t dense;  // row_stride == width: the band is one run of height * width elements
};

// 16-byte windows a run of seg_len elements of ES bytes can touch, whatever its start's alignment
FRS_HD inline int64_t stats_windows(int64_t seg_len, int es) {
    const int64_t ve = 16 / es;
    return (seg_len + 2 * ve - 2) / ve;
}
// items (windows of all runs) of a band
FRS_HD inline int64_t stats_items(int64_t height, int64_t width, bool dense, int es) {
    return dense ? stats_windows(height * width, es) : height * stats_windows(width, es);
}

// One lane's share of a band whose first element is at band0: work-group g of gx, lane tid of BLOCK.
template <int BLOCK, int UNROLL, typename T, typename Acc>
FRS_HD inline void stats_fold(Acc &acc, const T *band0, const StatsParams &P, int g, int gx, int tid) {
    constexpr int ES = (int)sizeof(T), VE = 16 / ES;
    const int64_t seg_len = P.dense ? P.height * P.width : P.width;
    const int64_t nseg = P.dense ? 1 : P.height;
    const int64_t C = stats_windows(seg_len, ES);
    const int64_t items = nseg * C;
    constexpr int64_t kChunk = (int64_t)BLOCK * UNROLL;

    // item idx: its window's first element, as an index e0 of the run (negative in a head), and the run
    auto locate = [&](int64_t idx, const T *&run, int64_t &e0) {
        int64_t seg = 0, c = idx;
        if (nseg > 1) {
            seg = idx / C;
            c = idx - seg * C;
        }
        run = band0 + seg * P.row_stride;
        const int64_t off = (int64_t)((reinterpret_cast<uintptr_t>(run) & 15u) / (unsigned)ES);
        e0 = c * VE - off;
    };
    auto partial = [&](const T *run, int64_t e0) {
        const int64_t k0 = e0 < 0 ? 0 : e0;
        const int64_t k1 = e0 + VE < seg_len ? e0 + VE : seg_len;
        for (int64_t k = k0; k < k1; k++) acc.elem(run[k]);
    };
    for (int64_t base = (int64_t)g * kChunk; base < items; base += (int64_t)gx * kChunk) {
        if (base + kChunk <= items) {
            const T *run[UNROLL];
            int64_t e0[UNROLL];
            bool full[UNROLL];
            StatsVec q[UNROLL];
            for (int u = 0; u < UNROLL; u++) {
                locate(base + (int64_t)u * BLOCK + tid, run[u], e0[u]);
                full[u] = e0[u] >= 0 && e0[u] + VE <= seg_len;
                if (full[u]) q[u] = *reinterpret_cast<const StatsVec *>(run[u] + e0[u]);
            }
            for (int u = 0; u < UNROLL; u++) {
                if (full[u]) acc.vec(q[u]);
                else partial(run[u], e0[u]);
            }
        } else {
            for (int64_t idx = base + tid; idx < items; idx += BLOCK) {
                const T *run;
                int64_t e0;
                locate(idx, run, e0);
                if (e0 >= 0 && e0 + VE <= seg_len) acc.vec(*reinterpret_cast<const StatsVec *>(run + e0));
                else partial(run, e0);
            }
        }
    }
    acc.finish();
}

// elements one work-group folds at most: its grid-stride steps, each a whole step of windows
FRS_HD inline int64_t stats_group_share(int64_t items, int64_t gx, int64_t chunk, int es) {
    const int64_t steps = (items + gx * chunk - 1) / (gx * chunk);
    return steps * chunk * (16 / es);
}

}  // namespace frs
