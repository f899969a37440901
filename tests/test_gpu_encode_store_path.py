"""The mono fast encoder's store path (resolve_and_store of k_encode_v4): the look-back's sum, the 16-byte store with
its byte-select, and the re-zeroing of the wave's bit buffer.

A frame's bytes leave the bit buffer as head bytes up to 16-byte alignment, 16-byte chunks whose words are one
byte-select of a word pair (the selector depends on the frame's offset mod 4), and tail bytes; the buffer's C rows
(C = ceil(words / 64), 1..34) are then zeroed for the wave's next frame.  The jobs below put frames at every offset
residue, use the smallest and the largest C, follow a large frame by a small one in one wave's buffer, span more than
one look-back window, and send a partial frame through the copy path; bytes, offsets and min / max must equal the
oracle's.  The selector itself is checked on the CPU against the big-endian word stream.
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_store_select.h"

T = 64  # a 64 x 64 tile is one 4096-sample frame
CONSTANT, FIXED, LPC, VERBATIM = 0, 1, 2, 3


def _tile(kind, rng, dtype):
    """a 64 x 64 tile that codes as a CONSTANT, FIXED, LPC or VERBATIM subframe; the random draws vary its size"""
    dt = np.dtype(dtype)
    if dt == np.uint8:
        if kind == CONSTANT:
            return np.full((T, T), int(rng.integers(0, 256)), dt)
        if kind == FIXED:  # a ramp along the frame with a few steps: FIXED, a few dozen to a few hundred bytes
            v = int(rng.integers(0, 60)) + np.arange(T * T) // int(rng.integers(24, 64))
            return v.reshape(T, T).astype(dt)
        if kind == LPC:
            y, x = np.meshgrid(np.linspace(0, 1, T), np.linspace(0, 1, T), indexing="ij")
            return (120 + 80 * np.sin(6 * x) * np.cos(4 * y) + int(rng.integers(4, 40)) * rng.random((T, T))).astype(dt)
        return rng.integers(0, 256, size=(T, T), dtype=dt)
    lo, hi = (0, 65536) if dt == np.uint16 else (-32768, 32768)
    mid = (lo + hi) // 2
    if kind == CONSTANT:
        return np.full((T, T), mid + int(rng.integers(-500, 500)), dt)
    if kind == FIXED:  # a per-column ramp
        return np.broadcast_to((mid + int(rng.integers(0, 2000)) + int(rng.integers(5, 20)) * np.arange(T)).astype(dt),
                               (T, T)).copy()
    if kind == LPC:  # smooth plus noise of 0.2 to 2.5 % of the range (the tile's range is stretched to 16 bits)
        y, x = np.meshgrid(np.linspace(0, 1, T), np.linspace(0, 1, T), indexing="ij")
        return (mid + 1000 + 3000 * np.sin(6 * x) * np.cos(4 * y) + int(rng.integers(10, 150)) * rng.random((T, T))).astype(dt)
    return rng.integers(lo, hi, size=(T, T), dtype=dt)


def _row(kinds, seed, dtype):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.concatenate([_tile(k, rng, dtype) for k in kinds], axis=1))


def _subframe_codes(o_arena, o_off):
    """the subframe type code of each one-frame tile's first frame (frame 0: a 6-byte frame header)"""
    return [int(o_arena[o + 6]) >> 1 for o in o_off[:-1]]


def _kind_of(code):
    return CONSTANT if code == 0 else VERBATIM if code == 1 else FIXED if 8 <= code < 16 else LPC


def _check(ctx, band, tile, oracle=None, threads=1):
    H, W = band.shape
    d = ctx.make_desc(H, W, band.dtype, tile_h=tile, tile_w=tile, sample_rate=44100, bits_per_sample=16)
    arena, off, mn, mx, bps = ctx.encode_tiles_host(band, d)
    o_arena, o_off, o_mn, o_mx = oracle if oracle is not None else O.encode_tiles(band, tile, threads=threads)
    assert bps == 16
    assert list(off) == list(o_off)
    assert len(arena) == int(o_off[-1])
    assert arena.tobytes() == o_arena.tobytes()
    assert list(mn) == list(o_mn) and list(mx) == list(o_mx)
    return o_off, o_arena


# ---- offset residues: 32 one-frame tiles, the four kinds in a scrambled order.  The seeds were chosen on the CPU so
# that the oracle's offsets alone meet the residue conditions asserted below.
RESIDUE_KINDS = [CONSTANT, FIXED, LPC, VERBATIM, FIXED, CONSTANT, LPC, FIXED] * 4
RESIDUE_SEED = {"int16": 7, "uint16": 3, "uint8": 5}  # each: all 16 residues mod 16


def _residue_job(dtype):
    band = _row(RESIDUE_KINDS, RESIDUE_SEED[np.dtype(dtype).name], dtype)
    return band, O.encode_tiles(band, T)


@pytest.mark.parametrize("dtype", ["int16", "uint16", "uint8"])
def test_offset_residues_oracle(dtype):
    """(CPU) the oracle's frames of the residue job start at all four residues mod 4 and at least 8 mod 16, and all
    four subframe kinds occur"""
    band, (o_arena, o_off, _, _) = _residue_job(dtype)
    assert len(o_off) == len(RESIDUE_KINDS) + 1 >= 25
    starts = [int(o) for o in o_off[:-1]]
    assert {s % 4 for s in starts} == {0, 1, 2, 3}
    assert len({s % 16 for s in starts}) >= 8
    kinds = {_kind_of(c) for c in _subframe_codes(o_arena, o_off)}
    assert kinds == {CONSTANT, FIXED, LPC, VERBATIM}
    sizes = np.diff(np.asarray(o_off))
    assert sizes.min() < 16  # a CONSTANT frame: no 16-byte chunk at all, head bytes only


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "uint16", "uint8"])
def test_offset_residues(gpu_ctx, dtype):
    band, oracle = _residue_job(dtype)
    o_arena, o_off = oracle[0], oracle[1]
    starts = [int(o) for o in o_off[:-1]]
    assert {s % 4 for s in starts} == {0, 1, 2, 3} and len({s % 16 for s in starts}) >= 8
    _check(gpu_ctx, band, T, oracle=oracle)


def _columns(nbytes):
    """C of the frame's buffer layout: ceil(words / 64) over the words the frame may touch (its bytes, rounded up to
    words, and one more)"""
    return max(1, ((int(nbytes) + 3) // 4 + 1 + 63) // 64)


@pytest.mark.gpu
def test_column_counts_in_one_row(gpu_ctx):
    """C = 1 (CONSTANT), a middle value (smooth LPC) and 33-34 (16-bit VERBATIM) side by side in tickets of 8"""
    kinds = [VERBATIM, CONSTANT, LPC, VERBATIM, VERBATIM, CONSTANT, FIXED, LPC, CONSTANT, VERBATIM, LPC, CONSTANT]
    band = _row(kinds, 77, np.int16)
    oracle = O.encode_tiles(band, T)
    sizes = np.diff(np.asarray(oracle[1]))
    cs = [_columns(s) for s in sizes]
    assert min(cs) == 1 and max(cs) in (33, 34) and any(4 <= c <= 28 for c in cs), cs
    _check(gpu_ctx, band, T, oracle=oracle)


@pytest.mark.gpu
def test_small_frame_after_large_in_one_wave_buffer(gpu_ctx):
    """4,096 VERBATIM frames (C = 33) fill one ticket of every work-group the grid can hold (2 per CU x 256 CUs x 8
    waves), so each of the 64 frames after them -- CONSTANT (C = 1) and smooth LPC by turns -- is coded by a wave
    whose buffer last held a 33-row frame: rows that the re-zeroing left behind would be ORed into the next frame or
    read by its CRC."""
    rng = np.random.default_rng(78)
    n_big, n_small = 4096, 64
    big = rng.integers(-32768, 32768, size=(T, T * n_big), dtype=np.int16)
    small = _row([CONSTANT, LPC] * (n_small // 2), 79, np.int16)
    band = np.ascontiguousarray(np.concatenate([big, small], axis=1))
    oracle = O.encode_tiles(band, T, threads=16)
    sizes = np.diff(np.asarray(oracle[1]))
    assert all(_columns(s) >= 33 for s in sizes[:n_big])
    assert all(_columns(s) == 1 for s in sizes[n_big::2]) and all(2 <= _columns(s) <= 28 for s in sizes[n_big + 1::2])
    _check(gpu_ctx, band, T, oracle=oracle)


@pytest.mark.gpu
def test_look_back_span(gpu_ctx):
    """200 one-frame tiles whose first 72 frames are long (VERBATIM): more than one 64-lane look-back window, and
    inclusive prefixes far above 2^16 next to aggregates of a dozen bytes"""
    kinds = [VERBATIM] * 72 + [CONSTANT, FIXED, LPC, VERBATIM, CONSTANT, CONSTANT, LPC, FIXED] * 16
    assert len(kinds) == 200
    band = _row(kinds, 80, np.int16)
    oracle = O.encode_tiles(band, T, threads=8)
    o_off, o_arena = _check(gpu_ctx, band, T, oracle=oracle)
    assert int(o_off[72]) > 72 * 8192 and len(o_arena) == int(o_off[-1])


@pytest.mark.gpu
def test_copy_path_beside_full_frames(gpu_ctx):
    """Tiles of 64 x 96 = one full frame and a partial one (2,048 samples, coded by the generic kernels and copied
    into the look-back chain): frames 1, 3, 5, 7 of the first ticket are copies beside full frames."""
    rng = np.random.default_rng(81)
    H, W, tw = T, 5 * 96, 96
    y, x = np.meshgrid(np.linspace(0, 7, H), np.linspace(0, 33, W), indexing="ij")
    band = (1000 + 300 * np.sin(x * 0.8) * np.cos(y * 0.3) + 50 * rng.random((H, W))).astype(np.int16)
    d = gpu_ctx.make_desc(H, W, band.dtype, tile_h=T, tile_w=tw, sample_rate=44100, bits_per_sample=16)
    arena, off, mn, mx, bps = gpu_ctx.encode_tiles_host(band, d)
    assert bps == 16
    # the oracle's tiles are square: a band of one 64 x 96 tile at tile = 96 is that tile's stream
    chunks, o_off, o_mn, o_mx = [], [0], [], []
    for c0 in range(0, W, tw):
        a, o, lo, hi = O.encode_tiles(np.ascontiguousarray(band[:, c0:c0 + tw]), tw)
        assert len(o) == 2
        chunks.append(np.asarray(a).tobytes())
        o_off.append(o_off[-1] + int(o[1]))
        o_mn.append(lo[0])
        o_mx.append(hi[0])
    assert list(off) == o_off
    assert arena.tobytes() == b"".join(chunks)
    assert list(mn) == o_mn and list(mx) == o_mx


# ---- the selector, on the CPU

_PROGRAM = r"""
#include "frs_store_select.h"
#include <cstdio>
#include <cstring>
#include <random>
int main() {
    std::mt19937 g(12345);
    const uint32_t want[4] = {0x00010203u, 0x07000102u, 0x06070001u, 0x05060700u};
    long bad = 0, n = 0;
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t sel = frs::store_select(r);
        if (sel != want[r]) bad++;
        for (int t = 0; t < 4000; t++) {
            uint32_t w[6];
            for (uint32_t &x : w) x = g();
            if (t < 8) for (int i = 0; i < 6; i++) w[i] = 0x00010203u + 0x04040404u * (uint32_t)i;  // byte b holds b
            unsigned char stream[24];  // the big-endian word stream
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 4; j++) stream[4 * i + j] = (unsigned char)(w[i] >> (24 - 8 * j));
            for (int i = 0; i < 5; i++) {
                const uint32_t o = frs::perm_bytes(w[i + 1], w[i], sel);  // pair {w[i + 1], w[i]}
                unsigned char mem[4];
                for (int k = 0; k < 4; k++) mem[k] = (unsigned char)(o >> (8 * k));  // memory order of a stored word
                if (memcmp(mem, stream + 4 * i + r, 4)) bad++;
                n++;
            }
        }
    }
    printf("%ld %ld\n", n, bad);
    return bad != 0;
}
"""


def test_store_selector_matches_the_big_endian_stream(tmp_path):
    """frs_store_select.h built by the host compiler: for r = 0..3 and 4,000 random runs of six words each, the
    byte-select of {w[i + 1], w[i]} is stream bytes 4 i + r .. 4 i + r + 3 in memory order"""
    (tmp_path / "t.cpp").write_text(_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(HEADER.parent), "-o", str(tmp_path / "t"),
                    str(tmp_path / "t.cpp")], check=True)
    p = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    n, bad = (int(v) for v in p.stdout.split())
    assert n == 4 * 4000 * 5 and bad == 0
