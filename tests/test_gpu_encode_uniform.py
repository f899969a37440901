"""GPU encode parity on the branches the fast encoder takes on wave-uniform (scalar) frame state.

k_encode_v4 keeps a frame's index and everything decoded from it -- tile geometry, normaliser, analysis, header row,
field positions, look-back bounds -- in scalar registers, and branches on them with scalar branches: the idle waves
of the last ticket, the partial-frame early return, a frame of another tile than the work-group's LUT, the subframe
type, the candidates.  The shapes here put each of those on both sides at least once; bytes, offsets and min / max
must equal the oracle's (as tests/test_gpu_encode_parity.py checks the common paths).
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _check(ctx, band, tile):
    H, W = band.shape
    d = ctx.make_desc(H, W, band.dtype, tile_h=tile, tile_w=tile, sample_rate=44100, bits_per_sample=16)
    arena, off, mn, mx, bps = ctx.encode_tiles_host(band, d)
    o_arena, o_off, o_mn, o_mx = O.encode_tiles(band, tile)
    assert bps == 16
    assert list(off) == list(o_off)
    assert arena.tobytes() == o_arena.tobytes()
    assert list(mn) == list(o_mn) and list(mx) == list(o_mx)
    return o_off, o_arena


def subframe_types_band():
    """64 x 448 int16, seven one-frame tiles of 64 x 64, one subframe kind each"""
    rng = np.random.default_rng(7)
    T = 64
    tiles = []
    t = np.full((T, T), 100, np.int16)      # order-1 total 0 from sample 4 on, yet not constant: LPC order 1
    t[0, :3] = (90, 110, 95)
    tiles.append(t)
    tiles.append(np.full((T, T), -7, np.int16))                                   # CONSTANT
    flat = np.arange(T * T)
    tiles.append((5 + (flat & 1)).astype(np.int16).reshape(T, T))                 # +-32767: the largest fixed totals
    tiles.append((5 + ((flat >> 1) & 1)).astype(np.int16).reshape(T, T))          # 5, 5, 6, 6, ...
    y, x = np.meshgrid(np.linspace(0, 1, T), np.linspace(0, 1, T), indexing="ij")
    tiles.append((1000 + 30 * np.sin(6 * x) * np.cos(4 * y) + 50 * rng.random((T, T))).astype(np.int16))
    tiles.append(np.broadcast_to((1000 + 12 * np.arange(T)).astype(np.int16), (T, T)).copy())  # per-column ramp
    tiles.append(rng.integers(-32768, 32768, size=(T, T), dtype=np.int16))        # VERBATIM
    return np.ascontiguousarray(np.concatenate(tiles, axis=1))


def test_one_frame_tiles_of_every_subframe_type(gpu_ctx):
    """A ticket's four frames sit in four tiles (three of them not the work-group's LUT tile), the last ticket has
    idle waves; the tiles code as LPC, CONSTANT, LPC, LPC, LPC, FIXED and VERBATIM subframes."""
    band = subframe_types_band()
    assert band.shape == (64, 448)
    o_off, o_arena = _check(gpu_ctx, band, 64)
    # the recipe still produces the intended kinds: the oracle's frame sizes and subframe type codes (the byte after
    # the 6-byte frame header: LPC order 1, CONSTANT, LPC 2, LPC 4, LPC 5, FIXED 1, VERBATIM)
    assert np.diff(np.asarray(o_off)).tolist() == [698, 11, 531, 537, 7963, 7155, 8201]
    assert [int(o_arena[o + 6]) >> 1 for o in o_off[:-1]] == [32, 0, 33, 35, 36, 9, 1]


def test_partial_last_frames_and_odd_width(gpu_ctx):
    """96 x 288 at tile 96: three tiles of 9216 samples = two full frames and a partial one (the early return that
    only joins the look-back), rows of 96 samples (no multiple of 64: the gather load and the row / column division)"""
    rng = np.random.default_rng(8)
    H, W = 96, 288
    y, x = np.meshgrid(np.linspace(0, 20, H), np.linspace(0, 20, W), indexing="ij")
    band = (1000 + 300 * np.sin(x * 0.8) * np.cos(y * 0.3) + 50 * rng.random((H, W))).astype(np.int16)
    o_off, _ = _check(gpu_ctx, band, 96)
    assert len(o_off) == 4


def test_wasted_bits_block_at_tile_64(gpu_ctx):
    band = np.full((128, 128), 7, dtype=np.int16)
    band[64:, :] = 9
    band[:, 100:] = 4000            # min/max spread so normalised samples have wasted bits in places
    _check(gpu_ctx, band, 64)
