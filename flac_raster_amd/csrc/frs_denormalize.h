// frs_denormalize.h -- the scalar arithmetic of the de-normalisation (converter.py:88-110 after pyflac + soundfile's
// PCM_16 WAV round trip: v = float32(pcm16 / 32768), out = round(((v + 1) / 2) * float32(max - min) + float32(min)) in
// fp32, round half to even, cast to the raster dtype; float dtypes get v itself), written once for the host and the
// device.  Includes nothing from HIP: a plain C++ compiler builds it (tests/test_denormalize_host.py, which holds the
// two-operation rewrite equal to the four-operation sequence for every range of uint8 / int16 / uint16 and every PCM
// value, and the four-operation value equal to numpy's), hipcc builds the same text as __host__ __device__.  Both need
// -ffp-contract=off: every multiply, add and divide below is one IEEE operation.  Users, all in frs_decode.hip: dn_store,
// dn_bits_t, the dn1 lambda and the dfast loop of k_decode_frames_pipe, k_denormalize, and the (range, min) pair of
// stage_decode_tables and denormalize_job; they keep their own loads, LDS, packing and stores.
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

// per stream: (float32(data_max - data_min), float32(data_min)).  The difference is taken in double first (Python
// floats), then each value is cast to float32 (NEP 50: a Python float beside a float32 array is a float32)
struct DnPair {
    float rng, mn;
};
FRS_HD inline DnPair dn_pair(double dmin, double dmax) { return {(float)(dmax - dmin), (float)dmin}; }

// the 16-bit sample that the WAV round trip keeps: 32-bit streams (shift 16) lose their low half (libsndfile int ->
// short), every other stream is unchanged (shift 0)
FRS_HD inline int32_t dn_pcm16(int32_t pcm, int shift) { return pcm >> shift; }

// v = float32(p16 / 32768): the division is by a power of two, so it is the exact product
FRS_HD inline float dn_unit(int32_t p16) { return (float)p16 * (1.0f / 32768.0f); }

// the reference's four operations on v, each rounded to fp32
FRS_HD inline float dn_value4(float v, float rng, float mn) {
    float a = v + 1.0f;
    a = a / 2.0f;
    a = a * rng;
    a = a + mn;
    return a;
}

// The same value in two operations, for <= 16-bit outputs.  With h = x << wasted (|h| < 2^24), v = h / 32768 and
// (v + 1) / 2 = (h + 32768) 2^-16 exactly; scaling rng by 2^-16 instead (dn_rng16) is exact too, so one product and
// one sum round as the reference's last two operations do.  x: the sample before its wasted-bit shift.
FRS_HD inline float dn_rng16(float rng) { return rng * (1.0f / 65536.0f); }
FRS_HD inline float dn_value2(int32_t x, int wasted, float rng16, float mn) {
    const float a = (float)((int32_t)((uint32_t)x << wasted) + 32768) * rng16;
    return a + mn;
}

// round half to even, then the cast: int64 serves every integer dtype (uint32 included); int32 where the rounded
// value is within a <= 16-bit dtype
FRS_HD inline int64_t dn_round64(float a) { return (int64_t)__builtin_rintf(a); }
FRS_HD inline int32_t dn_round32(float a) { return (int32_t)__builtin_rintf(a); }

}  // namespace frs
