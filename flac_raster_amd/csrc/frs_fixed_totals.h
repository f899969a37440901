// frs_fixed_totals.h -- the fixed-predictor totals of one lane's 64 samples, on packed int16 pairs
// (LanePairs::totals of k_encode_v4 and of the multi-channel kernels).
// Includes nothing from HIP: a plain C++ compiler builds it (tests/test_fixed_totals_host.py), hipcc builds the same
// text as __host__ __device__; the device pass takes the five instructions named below, the host pass their plain
// C++ restatements.
//
// fixed.c FLAC__fixed_compute_best_predictor sums |e_k(i)|, k = 0..4, e_0 = x, e_{k+1}(i) = e_k(i) - e_k(i - 1).
// The lane holds E[4 + m] = (x[2m], x[2m+1]) as int16 pairs (low half first) and E[0..3] = the eight samples before
// them (zeros on lane 0).  Per pair:
//  * A = E[4 + m], O = (x[2m-1], x[2m]) by one byte-select; Ab, Ob = A, O with 0x8000 flipped in both halves, which
//    keep their order as unsigned 16-bit values
//  * t0 += |x[2m]| + |x[2m+1]| = sad_u16(Ab, 0x80008000); t1 += |e1(2m)| + |e1(2m+1)| = sad_u16(Ab, Ob)
//  * y1(i) = e1(i) + 2^30 = dot2((x[i-1], x[i]), (-1, +1)) + 2^30: O for the even sample, A for the odd one
//  * y2(i) = (y1(i-1) ^ 0x7FFFFFFF) + y1(i) = y1(i) - y1(i-1) - 1 + 2^31 = e2(i) + 2^31 - 1 in one xor-add, and
//    y3(i) = (y2(i-1) ^ 0x7FFFFFFF) + y2(i) = e3(i) + 2^31 - 1 likewise.  The offset of a level is the same for every
//    i, so it cancels in |y_k(i) - y_k(i-1)| = |e_{k+1}(i)|, and |e_k| <= 2^20 keeps every y far from a wrap
//  * t2, t3, t4 += sad_u32(y_k(i), y_k(i-1)), k = 1..3
// which is 8.5 lane-instructions per sample: 1.5 for O, Ab, Ob, 1 for t0 and t1, 3 for y1..y3, 3 sads.
#pragma once
#include <stdint.h>

#ifndef FRS_HD
#ifdef __HIPCC__
#define FRS_HD __host__ __device__
#else
#define FRS_HD
#endif
#endif

#ifdef __HIPCC__
#define FRS_FT_UNROLL _Pragma("unroll")
#else
#define FRS_FT_UNROLL
#endif

namespace frs {

constexpr uint32_t kFtBias16 = 0x80008000u;  // int16 pair -> order-preserving unsigned halves
constexpr uint32_t kFtBias = 0x40000000u;    // y1 = e1 + kFtBias
constexpr uint32_t kFtNext = 0x7FFFFFFFu;    // (p ^ kFtNext) + y = y - p - 1 + 2^31

// (lo's high half, hi's low half): the pair one sample earlier than hi.  v_perm_b32 hi, lo, 0x05040302
FRS_HD inline uint32_t ft_mid_pair(uint32_t hi, uint32_t lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x05040302u);
#else
    return (lo >> 16) | (hi << 16);
#endif
}
// |a.lo - b.lo| + |a.hi - b.hi| + c on unsigned halves.  v_sad_u16
FRS_HD inline uint32_t ft_sad_u16(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u16(a, b, c);
#else
    const uint32_t al = a & 0xFFFFu, bl = b & 0xFFFFu, ah = a >> 16, bh = b >> 16;
    return c + (al > bl ? al - bl : bl - al) + (ah > bh ? ah - bh : bh - ah);
#endif
}
// |a - b| + c on unsigned operands.  v_sad_u32
FRS_HD inline uint32_t ft_sad_u32(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
#else
    return c + (a > b ? a - b : b - a);
#endif
}
// hi - lo + 2^30 of a signed int16 pair.  v_dot2_i32_i16 pair, (-1, +1), 2^30: the VOP3P form, whose accumulator is
// an inline constant (2^30 is the bit pattern of 2.0f; the VOP2 form v_dot2c adds into its destination, which costs a
// move per use)
FRS_HD inline uint32_t ft_diff_biased(uint32_t pair) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_dot2_i32_i16 %0, %1, %2, 0x40000000" : "=v"(d) : "v"(pair), "s"(0x0001FFFFu));
    return d;
#else
    return (uint32_t)((int32_t)(int16_t)(pair >> 16) - (int32_t)(int16_t)(pair & 0xFFFFu)) + kFtBias;
#endif
}
// y - p - 1 + 2^31: the next difference level of two values that carry the same offset.  v_xad_u32 p, 0x7FFFFFFF, y
FRS_HD inline uint32_t ft_next_level(uint32_t y, uint32_t p) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_xad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(p), "s"(kFtNext), "v"(y));
    return d;
#else
    return (p ^ kFtNext) + y;
#endif
}

// tk[k]: this lane's sum of |e_k(i)| over its 64 samples, lane 0 (l0) from sample 4 on, as the frame's totals start
// there; hk[k]: the sum over k <= i < 4 (lane 0 adds it to tk[k] for the fixed candidate's Rice sum, which runs from
// the warm-up on); hk[4] = 0.
FRS_HD inline void fixed_totals_pairs(const uint32_t *E, bool l0, uint32_t *tk, uint32_t *hk) {
    // the three levels at the sample before the lane's first, from the four before it (h4, h3 | h2, h1 = E[2], E[3])
    uint32_t p1, p2, p3;
    {
        const uint32_t d1 = ft_diff_biased(E[3]), d2 = ft_diff_biased(ft_mid_pair(E[3], E[2])), d3 = ft_diff_biased(E[2]);
        const uint32_t s1 = ft_next_level(d1, d2), s2 = ft_next_level(d2, d3);
        p1 = d1, p2 = s1, p3 = ft_next_level(s1, s2);
    }
    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    // ---- samples 0..3: lane 0 keeps them out of the totals
    {
        uint32_t y1[4], y2[4], y3[4], a0 = 0, a1 = 0;
        FRS_FT_UNROLL
        for (int m = 0; m < 2; m++) {
            const uint32_t A = E[4 + m], O = ft_mid_pair(A, E[3 + m]);
            a0 = ft_sad_u16(A ^ kFtBias16, kFtBias16, a0);
            a1 = ft_sad_u16(A ^ kFtBias16, O ^ kFtBias16, a1);
            y1[2 * m] = ft_diff_biased(O);
            y1[2 * m + 1] = ft_diff_biased(A);
        }
        uint32_t q1 = p1, q2 = p2;
        FRS_FT_UNROLL
        for (int j = 0; j < 4; j++) {
            y2[j] = ft_next_level(y1[j], q1);
            y3[j] = ft_next_level(y2[j], q2);
            q1 = y1[j], q2 = y2[j];
        }
        hk[0] = a0;
        hk[1] = ft_sad_u32(y1[3], kFtBias, ft_sad_u32(y1[2], kFtBias, ft_sad_u32(y1[1], kFtBias, 0)));
        hk[2] = ft_sad_u32(y1[3], y1[2], ft_sad_u32(y1[2], y1[1], 0));
        hk[3] = ft_sad_u32(y2[3], y2[2], 0);
        hk[4] = 0;
        const uint32_t a2 = ft_sad_u32(y1[1], y1[0], ft_sad_u32(y1[0], p1, hk[2]));
        const uint32_t a3 = ft_sad_u32(y2[2], y2[1], ft_sad_u32(y2[1], y2[0], ft_sad_u32(y2[0], p2, hk[3])));
        const uint32_t a4 = ft_sad_u32(y3[3], y3[2], ft_sad_u32(y3[2], y3[1],
                                       ft_sad_u32(y3[1], y3[0], ft_sad_u32(y3[0], p3, 0))));
        t0 = l0 ? 0u : a0, t1 = l0 ? 0u : a1, t2 = l0 ? 0u : a2, t3 = l0 ? 0u : a3, t4 = l0 ? 0u : a4;
        p1 = y1[3], p2 = y2[3], p3 = y3[3];
    }
    // ---- samples 4..63
    FRS_FT_UNROLL
    for (int m = 2; m < 32; m++) {
        const uint32_t A = E[4 + m], O = ft_mid_pair(A, E[3 + m]);
        const uint32_t Ab = A ^ kFtBias16;
        t0 = ft_sad_u16(Ab, kFtBias16, t0);
        t1 = ft_sad_u16(Ab, O ^ kFtBias16, t1);
        const uint32_t y1e = ft_diff_biased(O), y1o = ft_diff_biased(A);
        const uint32_t y2e = ft_next_level(y1e, p1), y2o = ft_next_level(y1o, y1e);
        const uint32_t y3e = ft_next_level(y2e, p2), y3o = ft_next_level(y2o, y2e);
        t2 = ft_sad_u32(y1o, y1e, ft_sad_u32(y1e, p1, t2));
        t3 = ft_sad_u32(y2o, y2e, ft_sad_u32(y2e, p2, t3));
        t4 = ft_sad_u32(y3o, y3e, ft_sad_u32(y3e, p3, t4));
        p1 = y1o, p2 = y2o, p3 = y3o;
    }
    tk[0] = t0, tk[1] = t1, tk[2] = t2, tk[3] = t3, tk[4] = t4;
}

}  // namespace frs
