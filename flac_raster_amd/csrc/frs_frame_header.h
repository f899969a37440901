// frs_frame_header.h -- the FLAC frame header (RFC 9639 9.1; libFLAC FLAC__frame_add_header), written once for
// the host and the device.  Includes nothing from HIP: a plain C++ compiler builds it (tests/test_frame_header.py),
// hipcc builds the same text as __host__ __device__.  Users: k_encode_frames, k_zero_frames_emit, k_mc_frame_bytes and
// k_mc_assemble (frame_header with c_crc8), the host's header table of the mono fast path (frame_header with a table
// it builds), and k_encode_v4 (sample_rate_code and frame_header_bytes only: it packs the header's bits itself when a
// frame number lies beyond that table); the decoder's selection and frame decoders (parse_header with d_crc8,
// header_ok_regs: the readers at the end of this file).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FRS_HD __host__ __device__
#define FRS_UNROLL _Pragma("unroll")
#else
#define FRS_HD
#define FRS_UNROLL
#endif

namespace frs {

// CRC-8 table (polynomial x^8 + x^2 + x + 1) of the header's last byte
inline void crc8_table(uint8_t *t) {
    for (int i = 0; i < 256; i++) {
        uint8_t c = (uint8_t)i;
        for (int k = 0; k < 8; k++) c = (c & 0x80) ? (uint8_t)((c << 1) ^ 0x07) : (uint8_t)(c << 1);
        t[i] = c;
    }
}

// src: the header's 4-bit code; srx: 12 / 13 / 14 when the rate follows the frame number (kHz in 8 bits, Hz in 16,
// Hz / 10 in 16), else 0
FRS_HD inline void sample_rate_code(int sr, int &src, int &srx) {  // RFC 9639 9.1.2
    srx = 0;
    switch (sr) {
    case 88200: src = 1; break;
    case 176400: src = 2; break;
    case 192000: src = 3; break;
    case 8000: src = 4; break;
    case 16000: src = 5; break;
    case 22050: src = 6; break;
    case 24000: src = 7; break;
    case 32000: src = 8; break;
    case 44100: src = 9; break;
    case 48000: src = 10; break;
    case 96000: src = 11; break;
    default:
        if (sr <= 255000 && sr % 1000 == 0) src = srx = 12;
        else if (sr % 10 == 0 && sr / 10 <= 65535) src = srx = 14;
        else src = srx = 13;
    }
}

// bsc: the 4-bit code; bsx: 6 / 7 when blocksize - 1 follows the frame number in 8 / 16 bits, else 0
FRS_HD inline void block_size_code(int n, int &bsc, int &bsx) {  // RFC 9639 9.1.1
    bsx = 0;
    switch (n) {
    case 192: bsc = 1; break;
    case 576: bsc = 2; break;
    case 1152: bsc = 3; break;
    case 2304: bsc = 4; break;
    case 4608: bsc = 5; break;
    case 256: bsc = 8; break;
    case 512: bsc = 9; break;
    case 1024: bsc = 10; break;
    case 2048: bsc = 11; break;
    case 4096: bsc = 12; break;
    case 8192: bsc = 13; break;
    case 16384: bsc = 14; break;
    case 32768: bsc = 15; break;
    default: bsc = bsx = (n <= 256 ? 6 : 7); break;
    }
}

// the "UTF-8" coded number of RFC 9639 9.1.5 (up to 6 bytes here: frame numbers are 32-bit); returns its bytes
FRS_HD inline int utf8_number(uint8_t *h, uint32_t v) {
    const int nb = v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : 6;
    if (nb == 1) {
        h[0] = (uint8_t)v;
        return 1;
    }
    h[0] = (uint8_t)((0xFF00u >> nb) | (v >> (6 * (nb - 1))));  // nb leading ones, a zero, the top bits
    for (int i = 1; i < nb; i++) h[i] = (uint8_t)(0x80 | ((v >> (6 * (nb - 1 - i))) & 0x3F));
    return nb;
}

// bytes of a fixed-blocksize (4096) frame header incl. CRC-8: sync/codes (4) + UTF-8 frame number + rate ext
FRS_HD inline uint32_t frame_header_bytes(uint32_t v, int srx) {
    const uint32_t u = v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : 6;
    return 4 + u + (srx == 12 ? 1 : (srx == 13 || srx == 14) ? 2 : 0) + 1;
}

// Header of a fixed-blocksize stream's frame into h (at most 16 bytes): sync, block size and sample rate codes,
// channel assignment code (channels - 1 independent; 8 left-side, 9 right-side, 10 mid-side), sample size code, the
// frame number, the block size and sample rate that their codes announce, CRC-8 by the caller's table.  Returns the
// header's bytes.
FRS_HD inline int frame_header(uint8_t *h, int blocksize, int sample_rate, int bps, int channel_code, uint32_t frame_no,
                               const uint8_t *crc8) {
    int bsc, bsx, src, srx;
    block_size_code(blocksize, bsc, bsx);
    sample_rate_code(sample_rate, src, srx);
    const int bpc = bps == 8 ? 1 : bps == 12 ? 2 : bps == 16 ? 4 : bps == 20 ? 5 : bps == 24 ? 6 : bps == 32 ? 7 : 0;
    int hb = 0;
    h[hb++] = 0xFF;
    h[hb++] = 0xF8;
    h[hb++] = (uint8_t)((bsc << 4) | src);
    h[hb++] = (uint8_t)((channel_code << 4) | (bpc << 1));
    hb += utf8_number(h + hb, frame_no);
    if (bsx == 6) h[hb++] = (uint8_t)(blocksize - 1);
    else if (bsx == 7) { h[hb++] = (uint8_t)((blocksize - 1) >> 8); h[hb++] = (uint8_t)(blocksize - 1); }
    if (srx == 12) h[hb++] = (uint8_t)(sample_rate / 1000);
    else if (srx == 13) { h[hb++] = (uint8_t)(sample_rate >> 8); h[hb++] = (uint8_t)sample_rate; }
    else if (srx == 14) { h[hb++] = (uint8_t)((sample_rate / 10) >> 8); h[hb++] = (uint8_t)(sample_rate / 10); }
    uint8_t c = 0;
    for (int i = 0; i < hb; i++) c = crc8[c ^ h[i]];
    h[hb++] = c;
    return hb;
}

// ------------------------------------------------------------------------------------------------ the readers
// Two forms of one acceptance test (RFC 9639 9.1: sync code, reserved codes, coded frame number, CRC-8, channel
// count): parse_header reads the header from memory and returns its fields (the frame decoders; the selection's
// fallback at a window's edge), header_ok_regs reads it from 16 bytes in registers and only accepts or rejects (the
// selection's fast path).  The header's shape -- the reserved codes, the lead byte's class, the extension bytes -- is
// header_tail; each form keeps its own byte access, bounds and CRC-8 walk.  header_ok_regs calls header_tail;
// parse_header holds a COPY of it in its own text (calling it gave the selection kernels and the frame decoders that
// inline parse_header other register figures), and tests/test_frame_header.py holds the copy equal: it runs both
// forms over every (byte 2, byte 3) pair and every lead-byte class.
// The one documented difference is the bound: parse_header stops at `end`, the end of the containing stream;
// header_ok_regs at `avail`, the bytes up to the end of the blob (at most 16).  A header that runs past its stream's
// end but not the blob's is accepted by the register form alone; it is only a candidate then, and the frame decoders'
// parse_header rejects it.

struct FrameHdr {
    int32_t ok;
    int32_t frame_no;  // frame number from the header
    int32_t bs;        // block size
    int32_t hdr_len;   // header bytes incl. CRC-8
    int32_t chass;     // channel assignment
    int32_t bps;       // sample size
};

// What follows the lead byte of the coded number: `extra` continuation bytes (-1: the header is rejected), then
// `bsx` bytes of block size (bsc 6 / 7) and `srx` bytes of sample rate (src 12 / 13, 14)
struct HeaderTail {
    int extra, bsx, srx;
};

// The fixed part of a header: byte 2 (block size and sample rate codes), byte 3 (channel assignment, sample size
// code, reserved bit) and the lead byte of the coded number (0xC0 .. 0xFC announce 1 .. 5 continuation bytes; 0x80 ..
// 0xBF and 0xFE, 0xFF are rejected: frame numbers are below 2^31)
FRS_HD inline HeaderTail header_tail(uint32_t b2, uint32_t b3, uint32_t lead) {
    const uint32_t bsc = b2 >> 4, src = b2 & 15, chass = b3 >> 4, ssc = (b3 >> 1) & 7;
    HeaderTail t = {-1, 0, 0};
    if (bsc == 0 || src == 15 || chass > 10 || ssc == 3 || (b3 & 1)) return t;
    int extra = 0;
    if (lead & 0x80) {
        if ((lead & 0xE0) == 0xC0) extra = 1;
        else if ((lead & 0xF0) == 0xE0) extra = 2;
        else if ((lead & 0xF8) == 0xF0) extra = 3;
        else if ((lead & 0xFC) == 0xF8) extra = 4;
        else if ((lead & 0xFE) == 0xFC) extra = 5;
        else return t;
    }
    t.extra = extra;
    t.bsx = bsc == 6 ? 1 : bsc == 7 ? 2 : 0;
    t.srx = src == 12 ? 1 : (src == 13 || src == 14) ? 2 : 0;
    return t;
}

// Parse + CRC-8-check (table crc8) a frame header at blob[p]; end = end of the containing stream.
FRS_HD inline FrameHdr parse_header(const uint8_t *blob, int64_t p, int64_t end, int channels, int stream_bps,
                                    const uint8_t *crc8) {
    FrameHdr h;
    h.ok = 0;
    if (p + 6 > end) return h;
    if (blob[p] != 0xFF || (blob[p + 1] & 0xFE) != 0xF8) return h;
    const uint8_t b2 = blob[p + 2], b3 = blob[p + 3];
    const int bsc = b2 >> 4, src = b2 & 15, chass = b3 >> 4, ssc = (b3 >> 1) & 7;
    // (from here to the CRC-8: a copy of header_tail, mixed with this form's reads)
    if (bsc == 0 || src == 15 || chass > 10 || ssc == 3 || (b3 & 1)) return h;
    int64_t q = p + 4;
    uint32_t v = blob[q++];
    int extra = 0;
    if (v & 0x80) {
        if ((v & 0xE0) == 0xC0) { extra = 1; v &= 0x1F; }
        else if ((v & 0xF0) == 0xE0) { extra = 2; v &= 0x0F; }
        else if ((v & 0xF8) == 0xF0) { extra = 3; v &= 0x07; }
        else if ((v & 0xFC) == 0xF8) { extra = 4; v &= 0x03; }
        else if ((v & 0xFE) == 0xFC) { extra = 5; v &= 0x01; }
        else return h;
    }
    for (int i = 0; i < extra; i++) {
        if (q >= end) return h;
        const uint8_t c = blob[q++];
        if ((c & 0xC0) != 0x80) return h;
        v = (v << 6) | (c & 0x3F);
    }
    int bs;
    if (bsc == 1) bs = 192;
    else if (bsc >= 2 && bsc <= 5) bs = 576 << (bsc - 2);
    else if (bsc == 6) { if (q >= end) return h; bs = blob[q++] + 1; }
    else if (bsc == 7) { if (q + 1 >= end) return h; bs = ((blob[q] << 8) | blob[q + 1]) + 1; q += 2; }
    else bs = 256 << (bsc - 8);
    if (src == 12) q += 1;
    else if (src == 13 || src == 14) q += 2;
    if (q >= end) return h;
    uint8_t c = 0;
    for (int64_t i = p; i < q; i++) c = crc8[c ^ blob[i]];
    if (c != blob[q]) return h;
    const int nch = chass < 8 ? chass + 1 : 2;
    if (nch != channels) return h;
    h.ok = 1;
    h.frame_no = (int32_t)v;
    h.bs = bs;
    h.hdr_len = (int32_t)(q + 1 - p);
    h.chass = chass;
    h.bps = ssc == 1 ? 8 : ssc == 2 ? 12 : ssc == 4 ? 16 : ssc == 5 ? 20 : ssc == 6 ? 24 : ssc == 7 ? 32 : stream_bps;
    return h;
}

// CRC-8 (poly 0x07) of one byte folded into c, bitwise (no table: the register form's check)
FRS_HD inline uint32_t crc8_byte(uint32_t c, uint32_t b) {
    c ^= b;
    FRS_UNROLL
    for (int k = 0; k < 8; k++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    return c;
}

// parse_header(...).ok on the 16 bytes h (little-endian dwords) that start at a sync code, `avail` bytes of the blob
// from there
FRS_HD inline bool header_ok_regs(const uint32_t *h, int64_t avail, int channels) {
    auto B = [&](int t) -> uint32_t { return (h[t >> 2] >> (8 * (t & 3))) & 0xFFu; };
    if (avail < 6) return false;
    const HeaderTail t = header_tail(B(2), B(3), B(4));
    if (t.extra < 0) return false;
    int q = 5;
    FRS_UNROLL
    for (int i = 0; i < 5; i++) {
        if (i < t.extra) {
            if (q >= avail || (B(5 + i) & 0xC0) != 0x80) return false;
            q++;
        }
    }
    q += t.bsx + t.srx;
    if (q >= avail) return false;  // (covers the extension bytes too) q <= 14: the CRC-8 byte is h's byte q
    uint32_t c = 0;
    FRS_UNROLL
    for (int i = 0; i < 15; i++)
        if (i < q) c = crc8_byte(c, B(i));
    if (c != B(q)) return false;
    const int chass = (int)(B(3) >> 4);
    return (chass < 8 ? chass + 1 : 2) == channels;
}

}  // namespace frs
