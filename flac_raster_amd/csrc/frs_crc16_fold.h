// frs_crc16_fold.h -- FLAC's frame CRC-16 (polynomial P = x^16 + x^15 + x^2 + 1, init 0, MSB first) without a table.
// Includes nothing from HIP: a plain C++ compiler builds it (tests/test_crc16_fold.py), hipcc builds the same text as
// __host__ __device__.  User: k_encode_v4 (crc16_column over a lane's column of the frame buffer; crc16_xpow for the
// host's table of the column factors).
//
// P = (x + 1) Q with Q = x^15 + x + 1, so a value mod P is fixed by its residue mod Q and its residue mod x + 1,
// which is the parity of the message bits.  Q is a trinomial: x^15 = x + 1, and by squaring x^(15 * 2^k) =
// x^(2^k) + 1, so hi x^(15 * 2^k) + lo reduces to lo ^ hi ^ (hi << 2^k).  At k = 5 and 6 that moves whole words:
// x^480 = x^32 + 1 and x^960 = x^64 + 1.  A message of 32-bit words therefore collapses into 15 accumulator words
// by XORs alone (crc16_fold_word), those 480 bits into 15 by eight shift-and-XOR folds (crc16_residue), and the
// residue and the parity give the CRC (crc16_finish).
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
#define FRS_UNROLL _Pragma("unroll")
#else
#define FRS_UNROLL
#endif

namespace frs {

constexpr int kCrcFoldSpan = 45;  // words one pass of crc16_fold_word spans (k / 15 <= 2)
constexpr int kCrcAcc = 17;       // accumulator words: 15, and two that crc16_fold_carry takes home

// Word w of a message, with k (< kCrcFoldSpan) words after it, into the accumulators: w x^(32 k) mod Q with
// k = 15 q + r is w x^(32 r) for q = 0, w (x^32 + 1) x^(32 r) for q = 1, w (x^64 + 1) x^(32 r) for q = 2.
// (k is a constant wherever the caller's loop is unrolled, so A stays in registers on the device.)
FRS_HD inline void crc16_fold_word(uint32_t *A, int k, uint32_t w) {
    const int q = k / 15, r = k % 15;
    A[r] ^= w;
    if (q) A[r + q] ^= w;
}

// A[15] x^480 = A[15] (x^32 + 1), A[16] x^512 = A[16] (x^64 + x^32)
FRS_HD inline void crc16_fold_carry(uint32_t *A) {
    A[0] ^= A[15];
    A[1] ^= A[15] ^ A[16];
    A[2] ^= A[16];
    A[15] = A[16] = 0;
}

// word j of V >> S; V has N words, word 0 the lowest
template <int N, int S>
FRS_HD inline uint32_t crc16_shr_word(const uint32_t *V, int j) {
    constexpr int ws = S / 32, bs = S % 32;
    const int i = j + ws;
    const uint32_t lo = i < N ? V[i] : 0u;
    if constexpr (bs == 0) {
        return lo;
    } else {
        const uint32_t hi = i + 1 < N ? V[i + 1] : 0u;
        return (lo >> bs) | (hi << (32 - bs));
    }
}

// One fold of V (N words) at B = 15 T bits, T = 2^k < 32: V = hi x^B + lo becomes R = lo ^ hi ^ (hi << T), in M
// words.  hi may be longer than B bits (the identity holds for any hi); R is max(B, bits(V) - B + T) bits long.
template <int N, int M, int B, int T>
FRS_HD inline void crc16_fold_bits(const uint32_t *V, uint32_t *R) {
    static_assert(B == 15 * T && T < 32 && 32 * M >= B, "fold point and multiplier");
    FRS_UNROLL
    for (int j = 0; j < M; j++) {
        uint32_t lo = 0;
        if (32 * (j + 1) <= B) lo = V[j];
        else if (32 * j < B) lo = V[j] & ((1u << (B - 32 * j)) - 1u);
        uint32_t h2 = crc16_shr_word<N, B - T>(V, j);  // (V >> B) << T, but for the T bits below
        if (j == 0) h2 &= ~((1u << T) - 1u);
        R[j] = lo ^ crc16_shr_word<N, B>(V, j) ^ h2;
    }
}

// the 15 accumulator words (480 bits) mod Q: 480 -> 256 -> 144 -> 88 -> 60 -> 46 -> 32 -> 18 -> 15 bits
FRS_HD inline uint32_t crc16_residue(const uint32_t *A) {
    uint32_t a[8], b[5], c[3], d[2], e[2], f[1], g[1], h[1];
    crc16_fold_bits<15, 8, 240, 16>(A, a);
    crc16_fold_bits<8, 5, 120, 8>(a, b);
    crc16_fold_bits<5, 3, 60, 4>(b, c);
    crc16_fold_bits<3, 2, 30, 2>(c, d);
    crc16_fold_bits<2, 2, 15, 1>(d, e);
    crc16_fold_bits<2, 1, 15, 1>(e, f);
    crc16_fold_bits<1, 1, 15, 1>(f, g);
    crc16_fold_bits<1, 1, 15, 1>(g, h);
    return h[0];
}

FRS_HD inline uint32_t crc16_parity(uint32_t v) { return (uint32_t)__builtin_popcount(v) & 1u; }

// The value below x^16 that is `res` mod Q and has parity `par`: res or res ^ Q (Q has three terms, so the two
// differ in parity; res < 2^15, so either stays below 2^16).
FRS_HD inline uint32_t crc16_join(uint32_t res, uint32_t par) {
    return res ^ (crc16_parity(res) != par ? 0x8003u : 0u);
}

// CRC-16 of a message M from M mod Q and the XOR of M's words (any value of M's parity): the CRC is M x^16 mod P,
// x^16 = x^2 + x mod Q, and a factor x^16 keeps the parity.
FRS_HD inline uint32_t crc16_finish(uint32_t res, uint32_t x) {
    uint32_t t[1] = {(res << 2) ^ (res << 1)}, r[1];
    crc16_fold_bits<1, 1, 15, 1>(t, r);
    return crc16_join(r[0], crc16_parity(x));
}

// v mod P for a polynomial of up to 64 bits
FRS_HD inline uint32_t crc16_reduce64(uint64_t v) {
    uint32_t a[2] = {(uint32_t)v, (uint32_t)(v >> 32)}, b[2], c[2], d[1];
    crc16_fold_bits<2, 2, 30, 2>(a, b);  // 64 -> 36 bits
    crc16_fold_bits<2, 2, 15, 1>(b, c);  // -> 22 (one word)
    crc16_fold_bits<1, 1, 15, 1>(c, d);  // -> 15
    return crc16_join(d[0], crc16_parity(a[0] ^ a[1]));
}

// CRC-16 `crc` of a message, extended by the t (0..3) bytes in the top bytes of `word`
FRS_HD inline uint32_t crc16_tail(uint32_t crc, uint32_t word, int t) {
    if (t == 0) return crc;
    return crc16_reduce64(((uint64_t)crc << (8 * t)) ^ ((uint64_t)(word >> (32 - 8 * t)) << 16));
}

// CRC-16 of the N-word message whose first c words are p[0], p[stride], ..., p[(c - 1) stride] and whose other
// words are zero (N <= kCrcFoldSpan).  Rows are read in groups of G: every row below min(N, c rounded up to G) is
// read, so those past c must be readable and hold zeros.
template <int N, int G = 1>
FRS_HD inline uint32_t crc16_column(const uint32_t *p, int stride, int c) {
    static_assert(N <= kCrcFoldSpan, "one fold pass");
    uint32_t A[kCrcAcc] = {0}, x = 0;
    FRS_UNROLL
    for (int i = 0; i < N; i++) {
        if (i % G == 0 && i >= c) break;
        const uint32_t w = p[i * stride];
        x ^= w;
        crc16_fold_word(A, N - 1 - i, w);
    }
    crc16_fold_carry(A);
    return crc16_finish(crc16_residue(A), x);
}

// CRC-16 of n big-endian 32-bit words p[0], p[stride], ...: the first n - 15 b words (at most kCrcFoldSpan) in one
// pass, then b blocks of 15 words, each after a multiplication of the accumulators by x^480 = x^32 + 1
FRS_HD inline uint32_t crc16_words(const uint32_t *p, long stride, long n) {
    uint32_t A[kCrcAcc] = {0}, x = 0;
    const long nb = n > kCrcFoldSpan ? (n - kCrcFoldSpan + 14) / 15 : 0, t = n - 15 * nb;
    FRS_UNROLL
    for (int k = kCrcFoldSpan - 1; k >= 0; k--) {
        if (k < t) {
            const uint32_t w = p[(t - 1 - k) * stride];
            x ^= w;
            crc16_fold_word(A, k, w);
        }
    }
    crc16_fold_carry(A);
    const uint32_t *q = p + t * stride;
    for (long b = 0; b < nb; b++, q += 15 * stride) {
        const uint32_t carry = A[14];  // A[14] x^32 = carry x^480
        FRS_UNROLL
        for (int r = 14; r >= 1; r--) {
            const uint32_t w = q[(14 - r) * stride];
            x ^= w;
            A[r] ^= A[r - 1] ^ w;
        }
        const uint32_t w = q[14 * stride];
        x ^= w;
        A[0] ^= carry ^ w;
        A[1] ^= carry;
    }
    return crc16_finish(crc16_residue(A), x);
}

// a b mod P (a, b below x^16)
FRS_HD inline uint32_t crc16_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^e mod P, e of either sign: P(0) = 1, so x has the inverse x^15 + x^14 + x (x times it is P + 1)
FRS_HD inline uint32_t crc16_xpow(long e) {
    uint32_t r = 1, s = e < 0 ? 0xC002u : 2u;
    for (unsigned long m = e < 0 ? 0ul - (unsigned long)e : (unsigned long)e; m; m >>= 1) {
        if (m & 1) r = crc16_mulmod(r, s);
        s = crc16_mulmod(s, s);
    }
    return r;
}

}  // namespace frs
