"""GPU encode parity where the mono fast encoder's work-group width shows: k_encode_v4 runs work-groups of 8 waves on
16-bit single-band jobs, so a ticket is 8 consecutive frames (wave = frame) that share one LUT tile.

The shapes put tile boundaries, idle waves, partial frames, the repack path and the deferred store on wave indices
4..7 and on tickets that mix up to eight tiles; bytes, offsets and min / max must equal the oracle's.
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

T = 64  # a 64 x 64 tile is one 4096-sample frame


def _check(ctx, band, tile, threads=1):
    H, W = band.shape
    d = ctx.make_desc(H, W, band.dtype, tile_h=tile, tile_w=tile, sample_rate=44100, bits_per_sample=16)
    arena, off, mn, mx, bps = ctx.encode_tiles_host(band, d)
    o_arena, o_off, o_mn, o_mx = O.encode_tiles(band, tile, threads=threads)
    assert bps == 16
    assert list(off) == list(o_off)
    assert arena.tobytes() == o_arena.tobytes()
    assert list(mn) == list(o_mn) and list(mx) == list(o_mx)
    return o_off, o_arena


def _one_frame_tile(kind, rng):
    """a 64 x 64 int16 tile that codes as a CONSTANT, FIXED, LPC or VERBATIM subframe"""
    if kind == 0:
        return np.full((T, T), int(rng.integers(-500, 500)), np.int16)
    if kind == 1:  # a per-column ramp: FIXED
        return np.broadcast_to((int(rng.integers(0, 2000)) + 12 * np.arange(T)).astype(np.int16), (T, T)).copy()
    if kind == 2:  # smooth plus noise: LPC
        y, x = np.meshgrid(np.linspace(0, 1, T), np.linspace(0, 1, T), indexing="ij")
        return (1000 + 30 * np.sin(6 * x) * np.cos(4 * y) + 50 * rng.random((T, T))).astype(np.int16)
    return rng.integers(-32768, 32768, size=(T, T), dtype=np.int16)  # VERBATIM


@pytest.mark.parametrize("ntiles", [7, 8, 9, 17])
def test_one_frame_tiles_in_rows(gpu_ctx, ntiles):
    """Rows of 7, 8, 9 and 17 one-frame tiles: a ticket with one idle wave, a full ticket, a ticket of one frame with
    seven idle waves; eight different tiles in a ticket, seven of them off the work-group's LUT."""
    rng = np.random.default_rng(1000 + ntiles)
    band = np.ascontiguousarray(np.concatenate([_one_frame_tile(i % 4, rng) for i in range(ntiles)], axis=1))
    assert band.shape == (T, T * ntiles)
    o_off, o_arena = _check(gpu_ctx, band, T)
    assert len(o_off) == ntiles + 1
    # the recipe still gives the intended kinds (the byte after the 6-byte frame header: the subframe type code)
    codes = [int(o_arena[o + 6]) >> 1 for o in o_off[:-1]]
    for i, c in enumerate(codes):
        k = i % 4
        assert (c == 0) if k == 0 else (8 <= c < 16) if k == 1 else (c >= 32) if k == 2 else (c == 1), (i, c)


def _encode_rect(ctx, band, tile_h, tile_w):
    """GPU encode at a rectangular tile against the oracle run tile by tile (its tiles are square: a band of one
    tile_h x tile_w tile at tile = max(tile_h, tile_w) is that tile's stream)"""
    H, W = band.shape
    d = ctx.make_desc(H, W, band.dtype, tile_h=tile_h, tile_w=tile_w, sample_rate=44100, bits_per_sample=16)
    arena, off, mn, mx, bps = ctx.encode_tiles_host(band, d)
    assert bps == 16
    chunks, o_off, o_mn, o_mx = [], [0], [], []
    for r0 in range(0, H, tile_h):
        for c0 in range(0, W, tile_w):
            t = np.ascontiguousarray(band[r0:r0 + tile_h, c0:c0 + tile_w])
            a, o, lo, hi = O.encode_tiles(t, max(tile_h, tile_w))
            assert len(o) == 2
            chunks.append(np.asarray(a).tobytes())
            o_off.append(o_off[-1] + int(o[1]))
            o_mn.append(lo[0])
            o_mx.append(hi[0])
    assert list(off) == o_off
    assert arena.tobytes() == b"".join(chunks)
    assert list(mn) == o_mn and list(mx) == o_mx


def test_three_frame_tiles(gpu_ctx):
    """Six tiles of 128 x 96 = 12,288 samples, three full frames each: tile boundaries fall inside tickets (18 frames
    in tickets of 8 + 8 + 2), and rows of 96 samples take the gather load."""
    rng = np.random.default_rng(31)
    H, W = 128, 6 * 96
    y, x = np.meshgrid(np.linspace(0, 9, H), np.linspace(0, 40, W), indexing="ij")
    band = (800 + 400 * np.sin(x * 0.7) * np.cos(y * 0.4) + 40 * rng.random((H, W))).astype(np.int16)
    _encode_rect(gpu_ctx, band, 128, 96)


def test_partial_frames_on_every_other_wave(gpu_ctx):
    """Five tiles of 96 x 96 = two full frames and a partial one: 15 frames, the partial ones (the early return that
    only joins the look-back) are frames 2, 5, 8, 11, 14 -- waves 2 and 5 of the first ticket, then 0, 3, 6."""
    rng = np.random.default_rng(32)
    H, W = 96, 5 * 96
    y, x = np.meshgrid(np.linspace(0, 20, H), np.linspace(0, 33, W), indexing="ij")
    band = (1000 + 300 * np.sin(x * 0.8) * np.cos(y * 0.3) + 50 * rng.random((H, W))).astype(np.int16)
    o_off, _ = _check(gpu_ctx, band, 96)
    assert len(o_off) == 6


def test_more_frames_than_the_resident_grid(gpu_ctx):
    """3072 x 5632 at tile 512: 66 tiles, 4,224 frames, more than one pass of a grid of 2 work-groups per CU with 8
    frames each (256 CUs: 4,096): work-groups loop, reload the LUT and carry the deferred store across tickets."""
    rng = np.random.default_rng(33)
    H, W = 3072, 5632
    y, x = np.meshgrid(np.linspace(0, 30, H, dtype=np.float32), np.linspace(0, 55, W, dtype=np.float32),
                       indexing="ij")
    band = (3000 + 1500 * np.sin(x) * np.cos(y) + 60 * rng.random((H, W), dtype=np.float32)).astype(np.int16)
    o_off, _ = _check(gpu_ctx, band, 512, threads=16)
    assert len(o_off) == 67


@pytest.mark.parametrize("layout", ["own_tile", "lut_tile"])
def test_lane_segment_overflow_in_wave_5(gpu_ctx, layout):
    """A lane whose 64 codes outgrow its private column of 1,088 bits makes the wave repack the frame; here that
    frame is the sixth of its ticket (wave 5).  Lane 20's samples alternate between the extremes around a smooth
    field, so a predictor fitted to the field leaves residuals near 2^16 there: with the Rice parameter at most 14 a
    code of zigzag value >= 2^16 takes >= 4 + 1 + 14 = 19 bits, 64 of them 1,216 bits.  own_tile: eight one-frame
    tiles (the frame is off the work-group's LUT); lut_tile: one 256 x 256 tile of 16 frames (frames 5 and 13, wave 5
    of both tickets, on the LUT)."""
    rng = np.random.default_rng(34)
    if layout == "own_tile":
        H, W, tile = T, 8 * T, T
    else:
        H, W, tile = 256, 256, 256
    y, x = np.meshgrid(np.linspace(0, 6, H), np.linspace(0, 6, W), indexing="ij")
    band = (2000 + 900 * np.sin(x) * np.cos(y) + 20 * rng.random((H, W))).astype(np.int16)
    burst = np.where(np.arange(64) & 1, 32000, -32000).astype(np.int16) + rng.integers(-700, 700, 64).astype(np.int16)
    spiked = []
    if layout == "own_tile":
        t = np.ascontiguousarray(band[:, 5 * T:6 * T])
        t.flat[64 * 20:64 * 21] = burst
        band[:, 5 * T:6 * T] = t
        spiked = [5]
    else:
        for f in (5, 13):
            band.flat[f * 4096 + 64 * 20:f * 4096 + 64 * 21] = burst
    o_off, o_arena = _check(gpu_ctx, band, tile, threads=4)
    for t in spiked:  # still a predicted subframe (FIXED or LPC), not VERBATIM
        assert (int(o_arena[o_off[t] + 6]) >> 1) >= 8
