// frs_normalize.h -- the scalar arithmetic of the tile normalisation (converter.py:56-86:
// ((2.0*(x-min))/(max-min) - 1.0) * 32767 with numpy-2 dtype wrap of x-min and max-min and the x86 truncating cast),
// written once for the host and the device.  Includes nothing from HIP: a plain C++ compiler builds it
// (tests/test_normalize_host.py, which checks the reciprocal form against the division for every 0 <= d <= den <= 65535,
// the mode choice at its cut-offs and udiv_inv at the multiples of its divisor), hipcc builds the same text as
// __host__ __device__.  Both need -ffp-contract=off: every multiply, add and divide below is one IEEE operation, and
// the only fused operations are the two spelled __builtin_fma.  Users, all in frs_encode.hip: Normalizer::operator(),
// norm_fast, norm_chunk, lut_entry and ana_norm, which keep their own loads, LDS and loops, and the row division of
// the fast kernels (udiv_inv).  tile_norm_finalize holds a copy of norm_mode_of's text (the call changed its code).
#pragma once
#include <stdint.h>

#ifndef FRS_HD
#ifdef __HIPCC__
#define FRS_HD __host__ __device__
#else
#define FRS_HD
#endif
#endif

namespace frs {

constexpr int kNormLut = 0;      // pcm = lut[x - min] (R + 1 <= kLutCap entries, built once per tile)
constexpr int kNormFastDiv = 1;  // no wrap, den <= 65535: RN(2d/den) by reciprocal + 2 FMA (exhaustively exact)
constexpr int kNormSlow = 2;     // anything else (wrapping int16, 32-bit dtypes, floats): IEEE division
constexpr int kNormZero = 3;     // max == min: zeros
constexpr int kLutCap = 4096;    // LUT entries per tile

// numpy's float64 -> int32 cast as compiled on x86-64 (cvttsd2si): truncation, out of range or NaN
// gives INT32_MIN ("integer indefinite").  The gfx950 v_cvt_i32_f64 saturates instead, so guard it.
FRS_HD inline int32_t cast_f64_i32_x86(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return INT32_MIN;
    return (int32_t)v;
}

// RN(a / den) from rinv = RN(1 / den) by one Newton step in two FMAs.  Equal to a / den bit for bit for a = 2 d,
// every integer 0 <= d <= den <= 65535 (all 2 147 516 415 pairs: tests/test_normalize_host.py).
FRS_HD inline double norm_quot_recip(double a, double den, double rinv) {
    const double q0 = a * rinv;
    const double r = __builtin_fma(-q0, den, a);
    return __builtin_fma(r, rinv, q0);
}

// the 16-bit sample of d = x - min (wrapped to the dtype by the caller) over den = max - min: the exact division
FRS_HD inline int32_t norm16_div(double d, double den) {
    return (int32_t)(int16_t)cast_f64_i32_x86(((2.0 * d) / den - 1.0) * 32767.0);
}
// the same from a = 2 d by the reciprocal (kNormLut / kNormFastDiv tiles only: 0 <= d <= den <= 65535)
FRS_HD inline int32_t norm16_recip(double a, double den, double rinv) {
    return (int32_t)(int16_t)cast_f64_i32_x86((norm_quot_recip(a, den, rinv) - 1.0) * 32767.0);
}
// norm16_recip without the cast's range guard: for 0 <= a <= 2 den the product lies in [-32767, 32767], where the
// plain cast is the guarded one (the chunk loops of norm_chunk and ana_norm, which spend no compare on it)
FRS_HD inline int32_t norm16_recip_inrange(double a, double den, double rinv) {
    return (int32_t)(int16_t)(int32_t)((norm_quot_recip(a, den, rinv) - 1.0) * 32767.0);
}

// v wrapped to an integer dtype of `bits` (8, 16, 32) bits: numpy 2 same-kind arithmetic (NEP 50)
FRS_HD inline int64_t norm_wrap(int64_t v, int bits, bool is_signed) {
    switch (bits) {
    case 8: return is_signed ? (int64_t)(int8_t)v : (int64_t)(uint8_t)v;
    case 16: return is_signed ? (int64_t)(int16_t)v : (int64_t)(uint16_t)v;
    default: return is_signed ? (int64_t)(int32_t)v : (int64_t)(uint32_t)v;
    }
}

// how the fast kernels normalise an integer tile of extremes imin <= imax (kNorm*).  norm_mode 0 is converter.py's
// map (1: spatial_encoder.py's, which has no modes), scale_bits 16 the 16-bit streams.  x - min and max - min cannot
// wrap in the dtype exactly when the range R does not: then d = x - min is the true difference, 0 <= d <= R, and the
// LUT (R + 1 <= kLutCap entries) or the reciprocal (R <= 65535) applies; anything else takes the division.
// (tile_norm_finalize in frs_encode.hip restates these lines: change both together.)
FRS_HD inline int norm_mode_of(int64_t imin, int64_t imax, int bits, bool is_signed, int norm_mode, int scale_bits) {
    int mode = kNormSlow;
    const int64_t R = imax - imin;
    const bool nowrap = norm_wrap(R, bits, is_signed) == R;
    if (norm_mode == 0 && scale_bits == 16) {
        if (!(imax > imin)) mode = kNormZero;
        else if (nowrap && R + 1 <= kLutCap) mode = kNormLut;
        else if (nowrap && R <= 65535) mode = kNormFastDiv;
    }
    return mode;
}

// n / d for n < 2^32 via a double reciprocal (inv = 1.0 / d): the estimate is off by at most one, fixed up
// (tests/test_normalize_host.py: at and beside the multiples of every d <= 70000)
FRS_HD inline uint32_t udiv_inv(uint32_t n, uint32_t d, double inv) {
    uint32_t q = (uint32_t)((double)n * inv);
    const int64_t r = (int64_t)n - (int64_t)q * d;
    q = r < 0 ? q - 1 : (r >= (int64_t)d ? q + 1 : q);
    return q;
}

}  // namespace frs
