// frs_resample.h -- the scalar arithmetic of one 2x reduction step of the overview pyramid (frs_downsample2*), written
// once for the host and the device.  Includes nothing from HIP: a plain C++ compiler builds it
// (tests/test_resample_host.py, which checks the integer average against exact integer arithmetic at every edge value
// of every dtype and the float forms against the same expressions in numpy), hipcc builds the same text as
// __host__ __device__.  Needs -ffp-contract=off like the rest of the library (no operation below could fuse, but the
// rule is one IEEE operation per operator).  User: downsample_group in frs_pyramid.hip, which keeps its own loads,
// stores and loops.
//
// One step takes an H x W band to ceil(H/2) x ceil(W/2).  Output pixel (r, x) covers source rows 2r .. min(2r+1, H-1)
// and columns 2x .. min(2x+1, W-1): n = 4, 2 or 1 source pixels (edge blocks of odd sizes are partial, never padded).
//   nearest            the source pixel (2r, 2x)
//   average, integers  floor((2 s + n) / (2 n)) of the exact 64-bit block sum s: the mean rounded half towards
//                      +infinity; for n = 4 that is (s + 2) >> 2 with an arithmetic shift (-1,-1,-1,-2 -> -1;
//                      -1,-2 -> -1; -3,-2 -> -2).  |s| <= 4 * 2^32, so nothing here can overflow.
//   average, floats    n = 4: ((a + b) + (c + d)) * 0.25 with a = (2r, 2x), b = (2r, 2x+1), c = (2r+1, 2x),
//                      d = (2r+1, 2x+1); n = 2: (a + b) * 0.5; n = 1: a.  Every operation is rounded in the dtype; NaN
//                      and +-inf fall out of the expression.
// The definition is the project's own (no parity with any other library's "average" is claimed).
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

constexpr int kResampleNearest = 0;  // FRS_RESAMPLE_NEAREST
constexpr int kResampleAverage = 1;  // FRS_RESAMPLE_AVERAGE

// floor((2 s + n) / (2 n)) for n = 1, 2, 4 (log2n = 0, 1, 2): add half the divisor, shift arithmetically
FRS_HD inline int64_t resample_round_shift(int64_t s, int log2n) {
    return (s + (((int64_t)1 << log2n) >> 1)) >> log2n;
}

// integer dtypes (u8, u16, i16, i32, u32): the sum in 64 bits, the result back in T (it lies between the block's
// smallest and largest value, so the narrowing is exact)
template <typename T> FRS_HD inline T resample_avg4(T a, T b, T c, T d) {
    return (T)resample_round_shift(((int64_t)a + (int64_t)b) + ((int64_t)c + (int64_t)d), 2);
}
template <typename T> FRS_HD inline T resample_avg2(T a, T b) {
    return (T)resample_round_shift((int64_t)a + (int64_t)b, 1);
}
// floats: the expressions of the header comment, each operation rounded in the dtype
FRS_HD inline float resample_avg4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }
FRS_HD inline float resample_avg2(float a, float b) { return (a + b) * 0.5f; }
FRS_HD inline double resample_avg4(double a, double b, double c, double d) { return ((a + b) + (c + d)) * 0.25; }
FRS_HD inline double resample_avg2(double a, double b) { return (a + b) * 0.5; }

// size of one level from the previous one
FRS_HD inline int64_t resample_half(int64_t n) { return (n + 1) >> 1; }

}  // namespace frs
