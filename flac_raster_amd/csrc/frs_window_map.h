// frs_window_map.h -- the scalar arithmetic of a windowed resample (frs_resample_window*): a rectangle of a source
// buffer, given in fractional pixel coordinates, onto a destination grid of any size, written once for the host and the
// device.  Includes nothing from HIP: a plain C++ compiler builds it (tests/test_window_map_host.py compares every
// index, weight, validity flag and rounded result with the numpy restatement in tests/window_ref.py, bit for bit), hipcc
// builds the same text as __host__ __device__.  Needs -ffp-contract=off like the rest of the library: every operator
// below is one IEEE fp64 operation.  User: window_group in frs_window.hip, which keeps its own loads, stores and loops.
//
// The definition is the project's own (no parity with GDAL's or any other library's resampling is claimed).
//
// The source rectangle is x0, y0, width, height in pixel-EDGE coordinates of the source buffer: pixel i covers
// [i, i + 1).  It may reach outside the buffer.  Per axis, with N the source extent, n the destination extent and span
// the rectangle's width or height:
//   step = span / n,  lo(j) = x0 + j * step,  hi(j) = x0 + (j + 1) * step,  centre(j) = x0 + (j + 0.5) * step
// (one multiply and one add each; j, j + 1 and j + 0.5 are exact doubles).
//   nearest    i = floor(centre); valid iff 0 <= i < N.
//   bilinear   valid iff 0 <= floor(centre) < N.  u = centre - 0.5, i0 = floor(u), t = u - i0; taps i0 and i0 + 1, each
//              clamped to [0, N - 1], weights 1 - t and t.  Value (a (1 - tx) + b tx) (1 - ty) + (c (1 - tx) + d tx) ty
//              with a, b on the upper row.
//   average    clo = max(lo, 0), chi = min(hi, N); valid iff chi > clo (on both axes).  Taps i = floor(clo) ..
//              ceil(chi) - 1 with weight min(chi, i + 1) - max(clo, i) (always > 0).  Value
//              (sum over rows ascending of wy * (sum over columns ascending of wx * v)) / ((chi_x - clo_x) (chi_y - clo_y)),
//              both sums starting from 0.0.  The tap count is not capped.
// Source values are converted to double (exact for every dtype).  Results: integer dtypes round half to even, clamp to
// the dtype's range, cast; float32 narrows the double; float64 keeps it.  NaN and +-inf come out as the expression
// gives them.  A pixel that is not valid gets `fill`, a double converted by the same rule.
//
// Two consequences:
//   * With x0 = y0 = 0, width = W = w and height = H = h every mode returns a finite source unchanged (step is exactly 1;
//     the average's single tap has weight 1 and divisor 1, bilinear's t is 0).  "Unchanged" is by value: a float -0.0
//     comes back as +0.0 from the average (0.0 + -0.0), and an inf next to a pixel turns bilinear's 0-weight tap into
//     NaN, as the expression gives it.
//   * The integer average rounds half to EVEN.  The pyramid's FRS_RESAMPLE_AVERAGE (frs_resample.h) rounds half towards
//     +infinity.  They are different calls with different definitions.
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

constexpr int kWindowNearest = 0;   // FRS_RESAMPLE_NEAREST
constexpr int kWindowAverage = 1;   // FRS_RESAMPLE_AVERAGE
constexpr int kWindowBilinear = 2;  // FRS_RESAMPLE_BILINEAR

// one axis of the mapping: source extent N, the rectangle's origin and the step per destination pixel
struct WinAxis {
    double x0, step;
    int64_t N;
};
FRS_HD inline WinAxis win_axis(double x0, double span, int64_t n, int64_t N) {
    WinAxis a;
    a.x0 = x0, a.step = span / (double)n, a.N = N;
    return a;
}
FRS_HD inline double win_lo(const WinAxis &a, int64_t j) { return a.x0 + (double)j * a.step; }
FRS_HD inline double win_hi(const WinAxis &a, int64_t j) { return a.x0 + (double)(j + 1) * a.step; }
FRS_HD inline double win_centre(const WinAxis &a, int64_t j) { return a.x0 + ((double)j + 0.5) * a.step; }

FRS_HD inline int64_t win_clamp_index(int64_t i, int64_t N) { return i < 0 ? 0 : i > N - 1 ? N - 1 : i; }

// nearest: the tap (meaningful only when valid)
struct WinNearest {
    int64_t i;
    bool valid;
};
FRS_HD inline WinNearest win_nearest(const WinAxis &a, int64_t j) {
    const double f = __builtin_floor(win_centre(a, j));
    WinNearest r;
    r.valid = f >= 0.0 && f < (double)a.N;
    r.i = r.valid ? (int64_t)f : 0;
    return r;
}

// bilinear: the two clamped taps, the weight t of the second (the first has 1 - t)
struct WinLinear {
    int64_t i0, i1;
    double t;
    bool valid;
};
FRS_HD inline WinLinear win_linear(const WinAxis &a, int64_t j) {
    const double c = win_centre(a, j);
    const double f = __builtin_floor(c);
    const double u = c - 0.5;
    const double f0 = __builtin_floor(u);
    WinLinear r;
    r.valid = f >= 0.0 && f < (double)a.N;
    r.t = u - f0;
    const int64_t i = r.valid ? (int64_t)f0 : 0;  // (valid: -1 <= f0 < N)
    r.i0 = win_clamp_index(i, a.N), r.i1 = win_clamp_index(i + 1, a.N);
    return r;
}
FRS_HD inline double win_bilinear_value(double a, double b, double c, double d, double tx, double ty) {
    return (a * (1.0 - tx) + b * tx) * (1.0 - ty) + (c * (1.0 - tx) + d * tx) * ty;
}

// average: the clipped interval [clo, chi) and its taps i0 .. i1 - 1 (i0 = i1 = 0 when not valid)
struct WinArea {
    double clo, chi;
    int64_t i0, i1;
    bool valid;
};
FRS_HD inline WinArea win_area(const WinAxis &a, int64_t j) {
    const double lo = win_lo(a, j), hi = win_hi(a, j), n = (double)a.N;
    WinArea r;
    r.clo = lo > 0.0 ? lo : 0.0;
    r.chi = hi < n ? hi : n;
    r.valid = r.chi > r.clo;
    r.i0 = r.valid ? (int64_t)__builtin_floor(r.clo) : 0;
    r.i1 = r.valid ? (int64_t)__builtin_ceil(r.chi) : 0;
    return r;
}
// weight of tap i: min(chi, i + 1) - max(clo, i)
FRS_HD inline double win_area_weight(const WinArea &r, int64_t i) {
    const double a = (double)i, b = (double)(i + 1);
    return (r.chi < b ? r.chi : b) - (r.clo > a ? r.clo : a);
}
FRS_HD inline double win_area_value(double sum, const WinArea &x, const WinArea &y) {
    return sum / ((x.chi - x.clo) * (y.chi - y.clo));
}

// the result in the dtype: integers round half to even, clamp, cast (NaN, which only `fill` could be and the entry
// points reject, would go to 0); float narrows; double is kept
template <typename T> struct WinLimits;
template <> struct WinLimits<uint8_t> { static constexpr double lo = 0.0, hi = 255.0; };
template <> struct WinLimits<uint16_t> { static constexpr double lo = 0.0, hi = 65535.0; };
template <> struct WinLimits<int16_t> { static constexpr double lo = -32768.0, hi = 32767.0; };
template <> struct WinLimits<int32_t> { static constexpr double lo = -2147483648.0, hi = 2147483647.0; };
template <> struct WinLimits<uint32_t> { static constexpr double lo = 0.0, hi = 4294967295.0; };

template <typename T> FRS_HD inline T win_result(double v) {
    const double r = __builtin_rint(v);
    if (!(r >= WinLimits<T>::lo)) return r != r ? (T)0 : (T)WinLimits<T>::lo;
    if (r > WinLimits<T>::hi) return (T)WinLimits<T>::hi;
    return (T)(int64_t)r;
}
template <> FRS_HD inline float win_result<float>(double v) { return (float)v; }
template <> FRS_HD inline double win_result<double>(double v) { return v; }

}  // namespace frs
