"""GPU encode parity over the shapes the frame CRC-16 of k_encode_v4 works on.

The fast encoder lays a frame out in 64 columns of C = ceil(words / 64) rows and every lane folds its column into a
CRC-16 without a table (csrc/frs_crc16_fold.h: a column is a message of 34 words, the rows past C being zeros that
are never read), then the lanes' values are joined with x^(8m) factors.  What changes from frame to frame is C, the
number of tail bytes behind the last whole word (body & 3) and how much of the last data column is filled.  The
one-frame tiles here run from a CONSTANT frame of 11 bytes to a VERBATIM frame of 8201, and the conditions on C, the
tail and the last column are asserted on the oracle's frame sizes alone; bytes, offsets and min / max must equal the
oracle's.

C = 2 cannot occur on the fast path: its frames are full blocks of 4096 samples, and a subframe that is not CONSTANT
spends at least one bit per residual, so a body is either about 9 bytes (C = 1) or more than 512 (C >= 3).  C = 34
cannot occur either: the largest 16-bit mono frame is the VERBATIM one (8201 bytes, C = 33).
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

T = 64
EXPECTED_C = [1] + list(range(3, 34))


def column_shape(frame_bytes: int):
    """(C, body & 3, whole words in the last data column) of a fast-path frame of this size (k_encode_v4: body =
    bytes before the CRC-16 footer, the layout holds the body, the footer and a spare word)"""
    body = frame_bytes - 2
    words = ((8 * body + 23) >> 5) + 2
    c = (words + 63) // 64
    nfw = body >> 2
    return c, body & 3, (nfw - 1) % c + 1


def graded_band():
    """64 x 4928 int16: 77 one-frame tiles whose frames grow from 11 to 8201 bytes.  A tile's samples are scaled to
    the full 16-bit range by its own minimum and maximum, so the size is set by how well a tile predicts: a constant;
    the alternating pair (an exact order-2 prediction, one bit per residual); ramps that stay exact lines after the
    scaling (range 32767, slope 7), with a one added to a share p of the samples; then a ramp under uniform noise
    whose amplitude doubles every 4.3 tiles.  (Ranges stay below 32768: the reference's int16 difference wraps.)"""
    rng = np.random.default_rng(5)
    n = np.arange(T * T)
    tiles = [np.full(T * T, 123), 5 + (n & 1)]
    for p in (0.0, 0.01, 0.03, 0.06):
        v = -16000 + 7 * n + (rng.random(T * T) < p)
        v[-1] = -16000 + 32767
        tiles.append(v)
    ramp = np.linspace(-16000, 16000, T * T)
    for i in range(71):
        a = 0.2 * 2.0 ** (16.5 * i / 70)
        v = ramp * max(0.0, 1 - a / 16000) + rng.uniform(-a, a, T * T)
        tiles.append(np.clip(np.rint(v), -16383, 16383))
    return np.ascontiguousarray(np.concatenate([np.asarray(t).astype(np.int16).reshape(T, T) for t in tiles], axis=1))


def terrain_band(side):
    """C4-like data: smooth relief under a little noise"""
    rng = np.random.default_rng(12)
    y = np.linspace(0, 20, side, dtype=np.float32)[:, None]
    x = np.linspace(0, 20, side, dtype=np.float32)[None, :]
    base = 3000 + 1200 * np.sin(x * 0.7) * np.cos(y * 0.3) + 400 * np.sin(1.3 * x) * np.sin(1.1 * y)
    return (base + 60 * rng.random((side, side), dtype=np.float32)).astype(np.int16)


def _check(ctx, band, tile):
    H, W = band.shape
    d = ctx.make_desc(H, W, band.dtype, tile_h=tile, tile_w=tile, sample_rate=44100, bits_per_sample=16)
    ctx.profile(True)
    ctx.profile_reset()
    arena, off, mn, mx, bps = ctx.encode_tiles_host(band, d)
    compact_ms = ctx.profile_avg_ms("compact")
    ctx.profile(False)
    assert compact_ms < 0, "expected the fast path, got the generic kernels"
    o_arena, o_off, o_mn, o_mx = O.encode_tiles(band, tile)
    assert bps == 16
    assert list(off) == list(o_off)
    assert arena.tobytes() == o_arena.tobytes()
    assert list(mn) == list(o_mn) and list(mx) == list(o_mx)
    return o_off


def test_one_frame_tiles_of_every_column_shape(gpu_ctx):
    band = graded_band()
    assert band.shape == (64, 64 * 77)
    o_off = _check(gpu_ctx, band, T)
    sizes = np.diff(np.asarray(o_off)).tolist()
    assert min(sizes) == 11 and max(sizes) == 8201
    shapes = [column_shape(s) for s in sizes]
    assert sorted({c for c, _, _ in shapes}) == EXPECTED_C
    assert {t for _, t, _ in shapes} == {0, 1, 2, 3}
    # the last data column holds a single word / is full (C = 1 is both at once: asked of the taller layouts)
    assert any(c > 1 and last == 1 for c, _, last in shapes)
    assert any(c > 1 and last == c for c, _, last in shapes)


@pytest.mark.parametrize("side", [512, 768])
def test_multi_frame_tile(gpu_ctx, side):
    """One tile of side^2 / 4096 frames: 64 at 512 (frame numbers of one byte), 144 at 768 (two bytes from frame 128
    on, so the header is a byte longer and the body's alignment in the layout moves)"""
    _check(gpu_ctx, terrain_band(side), side)
