// frs_frame_header.h -- the FLAC frame header (RFC 9639 9.1; libFLAC FLAC__frame_add_header), written once for
// the host and the device.  Includes nothing from HIP: a plain C++ compiler builds it (tests/test_frame_header.py),
// hipcc builds the same text as __host__ __device__.  Users: k_encode_frames, k_zero_frames_emit, k_mc_frame_bytes and
// k_mc_assemble (frame_header with c_crc8), the host's header table of the mono fast path (frame_header with a table
// it builds), and k_encode_v4 (sample_rate_code and frame_header_bytes only: it packs the header's bits itself when a
// frame number lies beyond that table).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FRS_HD __host__ __device__
#else
#define FRS_HD
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

}  // namespace frs
