// frs_decode_plan.h -- what the host decides about one decode before it launches anything: the constants it decides
// with, the route (selection form, span check, frame decoder), the carves of the two-pass selection's scratch
// buffers, and the names of the counters word.  Includes nothing from HIP: a plain C++ compiler builds it
// (tests/test_decode_plan.py); frs_decode.hip's kernels take the constants and the counter names from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace frs {

// ---- candidate selection: a work-group of 4 waves takes kSelBytes, each wave kSelSteps steps of 1 KB
constexpr int kSelThreads = 256, kSelBytes = 64 * 1024;
constexpr int kSelSteps = kSelBytes / (kSelThreads / 64) / 1024;  // 16 steps of 1 KB per wave
static_assert(kSelSteps == 16, "64 KB blocks of 4 waves");
// small ranges (a C5 query's tile, <= 4 MB): 16 KB blocks of 4 waves x 4 steps, so a 0.5 MB tile spreads over 32
// work-groups instead of 8 (the one-pass selection is latency-bound there)
constexpr int kSelStepsSmall = 4;
constexpr int64_t kSelSmallBytes = (int64_t)kSelStepsSmall * 1024 * (kSelThreads / 64);
constexpr int64_t kSelOnePassBlocks = 256;  // up to 16 MB: the one-pass selection (latency: C5 queries)
constexpr int kSelBlkCap = 32;  // two-pass: candidates kept per 64 KB block (a C4 block holds ~8 frame starts)

// ---- frame decoders
constexpr int kDecResMax = 4096;          // residual buffer (LDS) of the fast subframe path: its largest block size
constexpr int64_t kLaneMinFrames = 4096;  // mono: this many frames take the lane-per-frame decoder
constexpr int64_t kMultiLaneMinFrames = 64;  // 2..8 channels: this many take the lane walk + k_interleave_dn
// range of the x^(8m) tables d_xpow_lo[256] x d_xpow_hi[4096] (crc_xpow): spans below this many bytes
constexpr int kDecXpowLo = 256, kDecXpowHi = 4096;
constexpr int64_t kDecXpowRange = (int64_t)kDecXpowHi * kDecXpowLo;

// ---- the counters word (frs_ctx::dec_count, ints): zeroed once, re-armed by the kernels
enum DecCounter {
    kCntCand = 0,      // candidates the selection found (may exceed the capacity: nothing is written past it)
    kCntValid = 1,     // frames decoded and verified
    kCntBroken = 2,    // k_chain_lds: a stream's frame chain broke
    kCntFallback = 3,  // frames the lane decoders queued for k_decode_frames_wave_list
    kCntTicket = 4,    // ints 4-5: the one-pass selection's ticket (64-bit)
    kCntDecline = 6,   // optimistic decode: declined (a false sync, a frame for the one-lane decoder)
    kCntOptValid = 7,  // optimistic decode: frames decoded and verified
    kCntRearm = 8,     // optimistic decode: work-groups finished; the last one re-arms it to 0
    kCntHostWords = 8,  // the host reads ints [0, 8) back; the word has 16 (frs_ctx::dec_count)
};

enum class SelForm { OnePassSmall, OnePass, TwoPass };  // k_sync_select<4>, k_sync_select<16>, count + scan + scatter
enum class SpanForm { Pcrc, Lane, Wave };               // k_span_pcrc, k_span_crc_lane, k_span_crc_wave
enum class FrameDec { Pipe, Lane, MultiLane, Wave };    // k_decode_frames_pipe / _lane / _lane<.., true> / _wave

struct DecodeRoute {
    SelForm sel;
    SpanForm span;
    FrameDec dec;
    // pipe_opt: the optimistic pipe decode runs first; span check, chain and decoder only if it declines.  planar16:
    // MultiLane with >= 3 independent channels of <= 16 bits (two: the side channel is 17 bits).  tabs_by_arg: the
    // per-call tables ride in k_sync_select's arguments.  fused: the decoders de-normalise into the caller's output
    bool pipe_opt, planar16, tabs_by_arg, fused;
    // the selection's block size and blocks; two-pass: the blocks whose 64 KB lie inside the range (the unguarded
    // instance; the last, partial block has its own)
    int64_t sel_bytes, nblocks, nfull;
    int64_t cand_cap;      // candidate capacity
    int64_t max_frame;     // bound of one frame's bytes
    int64_t planar_words;  // MultiLane: the channel-planar int32 scratch
};

// decode_lane: -1, or 0 / 1 to force the pipelined / lane-per-frame decoder; span_mode: 0, or 1 / 2 to force the
// reading / prefix-CRC span check of a two-pass selection (the other selections ignore it); frames > 0
inline DecodeRoute plan_decode_route(int channels, int bps, int blocksize, int64_t frames, int nstreams,
                                     int64_t blob_bytes, int lead, bool force_generic, int decode_lane, bool pipe_opt,
                                     int span_mode, bool fused) {
    DecodeRoute r;
    // the selection reads from the 16-byte boundary at or below the blob (`lead` = the pointer's low four bits)
    const int64_t lead_bytes = blob_bytes + lead;
    const bool small = (lead_bytes + kSelSmallBytes - 1) / kSelSmallBytes <= kSelOnePassBlocks;
    r.sel_bytes = small ? kSelSmallBytes : (int64_t)kSelBytes;
    r.nblocks = (lead_bytes + r.sel_bytes - 1) / r.sel_bytes;
    r.sel = small ? SelForm::OnePassSmall : r.nblocks <= kSelOnePassBlocks ? SelForm::OnePass : SelForm::TwoPass;
    r.nfull = r.sel == SelForm::TwoPass ? (lead_bytes / kSelBytes < r.nblocks ? lead_bytes / kSelBytes : r.nblocks) : 0;
    r.fused = fused;
    r.max_frame = (int64_t)blocksize * channels * 5 + 4096;
    // Candidate capacity: every true frame plus false syncs (a sync pattern with a CRC-8-correct header inside
    // frame data, ~1e-7 per byte) with a wide margin; a crafted stream with more is rejected (nothing is written
    // past the cap).  Indices stay below 2^31.
    const int64_t cap = 2 * frames + blob_bytes / 1024 + 4096;
    r.cand_cap = cap < (int64_t)0x7FFFFFF0 ? cap : (int64_t)0x7FFFFFF0;
    // the fast subframe path: <= 16 bits, a block that fits its LDS residual buffer; force_generic (tests): every
    // frame through the one-lane wave decoder
    const bool fast = bps <= 16 && blocksize <= kDecResMax && !force_generic;
    const bool mono = fast && channels == 1;
    // many mono frames: the lane-per-frame throughput decoder (the pipelined one is latency-optimised: ~2 work-groups
    // per CU at 62 KB of LDS each)
    const bool lane = mono && (decode_lane >= 0 ? decode_lane == 1 : frames >= kLaneMinFrames);
    // multi-channel streams: the lane decoder walks each frame's subframes into a channel-planar int32 scratch,
    // k_interleave_dn interleaves (and de-normalises); the wave decoder takes the rest
    const bool mcl = fast && channels >= 2 && channels <= 8 && frames >= kMultiLaneMinFrames && decode_lane != 0;
    r.dec = lane ? FrameDec::Lane : mcl ? FrameDec::MultiLane : mono ? FrameDec::Pipe : FrameDec::Wave;
    r.planar16 = mcl && channels >= 3;
    r.planar_words = mcl ? frames * channels * (int64_t)blocksize : 0;
    // Pipe implies max_frame <= 24576: its spans are within the x^(8m) tables, which k_span_crc_wave and the
    // optimistic decode's CRC need, and no span check for longer frames exists beside the lane form
    static_assert((int64_t)kDecResMax * 1 * 5 + 4096 < kDecXpowRange, "a Pipe frame is within the x^(8m) tables");
    r.pipe_opt = r.dec == FrameDec::Pipe && pipe_opt;
    // The span check from the prefix CRCs that the two-pass selection folds, within the x^(8m) table range:
    // multi-channel lane decodes by default (mono keeps the reading form: DESIGN.md 4.4), span_mode 1 / 2 forces
    const bool pcrc = span_mode != 1 && (span_mode == 2 || mcl) && r.sel == SelForm::TwoPass &&
                      r.dec != FrameDec::Pipe && r.max_frame < kDecXpowRange;
    // batched mono, or long multi-channel / 32-bit frames (which the wave form would walk on one lane past its LDS
    // stage): one lane per candidate; Pipe: one wave per candidate
    r.span = pcrc ? SpanForm::Pcrc : r.dec != FrameDec::Pipe ? SpanForm::Lane : SpanForm::Wave;
    // one stream through the one-pass selection (a bbox query)
    r.tabs_by_arg = nstreams == 1 && r.sel != SelForm::TwoPass;
    return r;
}

// ---- carves of the two-pass selection's scratch: byte offsets of the regions, in order, and the allocation's size
// frs_ctx::dec_sel: bcount int32 per block (its candidate count) | bbase int64 per block + 1 (exclusive scan of the
// counts) | bpos int64 kSelBlkCap per block (the positions a block kept)
struct SelLayout {
    size_t bcount, bbase, bpos, total;
};
inline SelLayout sel_layout(int64_t nblocks) {
    const size_t nb = (size_t)nblocks, bbase = 8 * ((nb + 1) / 2 + 1);
    return {0, bbase, bbase + 8 * (nb + 1), 8 * (2 * nb + 4 + (size_t)kSelBlkCap * nb)};
}

// frs_ctx::dec_crc (SpanForm::Pcrc): bp uint32 per block + 1 (prefix CRC at the block's first byte) | bfirst uint32 per
// block (first stream boundary in it) | bcrc uint16 per block (CRC of its 64 KB) | bipc uint16 kSelBlkCap per block
// (in-block prefix CRC of each kept candidate) | sbib uint16 per stream + 1 (in-block prefix CRC at the stream's
// boundary) | pcrc uint16 per candidate (prefix CRC at the candidate)
struct PcrcLayout {
    size_t bp, bfirst, bcrc, bipc, sbib, pcrc, total;
};
inline PcrcLayout pcrc_layout(int64_t nblocks, int nstreams, int64_t cand_cap) {
    const size_t nb = (size_t)nblocks, bfirst = 4 * (nb + 1), bcrc = bfirst + 4 * nb, bipc = bcrc + 2 * nb,
                 sbib = bipc + 2 * (size_t)kSelBlkCap * nb, pcrc = sbib + 2 * ((size_t)nstreams + 1);
    return {0, bfirst, bcrc, bipc, sbib, pcrc, pcrc + 2 * (size_t)cand_cap + 64};
}

}  // namespace frs
