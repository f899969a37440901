// frs_store_select.h -- byte selectors of the frame store (k_encode_v4's resolve_and_store).
// Includes nothing from HIP: a plain C++ compiler builds it (tests/test_gpu_encode_store_path.py), hipcc builds the
// same text as __host__ __device__.
//
// A frame sits in its bit buffer as big-endian 32-bit words: stream byte 4 i + j (j = 0..3) is bits 31 - 8 j .. 24 - 8 j
// of word i.  The store writes 16-byte chunks that begin r = 0..3 bytes into a word, so output word i (little-endian in
// memory) holds the stream bytes 4 i + r .. 4 i + r + 3: a byte swap and a byte alignment over the pair
// {w[i + 1], w[i]}, which is one byte-select.  v_perm_b32 D, S0, S1, sel numbers the bytes of {S0, S1} 0..7 from the
// least significant byte of S1; byte k of sel (< 8) picks the byte that lands in byte k of D.
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

// selector for perm(S0 = w[i + 1], S1 = w[i]): stream byte j (= r + k) of the pair is byte 3 - j of w[i] for j < 4
// and byte 7 - j of w[i + 1], numbered 11 - j in the pair, for j >= 4.  r = 0 is the plain byte swap 0x00010203.
FRS_HD constexpr uint32_t store_select(uint32_t r) {
    uint32_t sel = 0;
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t j = (r & 3u) + k;
        sel |= (j < 4 ? 3u - j : 11u - j) << (8 * k);
    }
    return sel;
}
static_assert(store_select(0) == 0x00010203u && store_select(1) == 0x07000102u && store_select(2) == 0x06070001u &&
                  store_select(3) == 0x05060700u,
              "the four selectors");

// v_perm_b32 for selector bytes below 8 (what store_select gives), for the host
FRS_HD inline uint32_t perm_bytes(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t pair = ((uint64_t)s0 << 32) | s1;
    uint32_t d = 0;
    for (int k = 0; k < 4; k++) d |= (uint32_t)((pair >> (8 * ((sel >> (8 * k)) & 7u))) & 0xFFu) << (8 * k);
    return d;
}

}  // namespace frs
