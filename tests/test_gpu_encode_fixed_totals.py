"""The fixed-predictor totals of the fast encoders (csrc/frs_fixed_totals.h) where lane 0's first four samples carry the
weight: frames that code FIXED although a full-scale step sits inside samples 0..3.

The totals that choose the fixed order run over samples 4..4095, so the step is outside them, while the fixed
candidate's Rice sum runs from the warm-up on, so lane 0 adds its terms at order <= i < 4 (hk) -- a full-scale step
there is the largest value those terms can take.  The signals after the step are sums of noise (walks) and integer
piecewise polynomials (block-wise constant differences with Thue-Morse signs, summed up), which the oracle codes as
FIXED of several orders; the CPU tests below hold that on the oracle's bytes alone, and the GPU tests compare bytes,
offsets and min / max with the oracle: rows of one-frame 64 x 64 tiles in three dtypes (17 tiles: a ticket of eight
frames holds several kinds), the same signals with one and three wasted bits, and as two-band (L / R / M units) and
three-band (subframe units) streams.

A one-frame tile holds its own extremes, which normalise to -32767 and 32767, so it never has wasted bits: the
wasted-bits signals are frames 1..3 of 128 x 128 tiles whose frame 0 is an anchor, and frames after an anchor frame
in the streams, as in tests/encode_cells.py; they are uint16, the dtype whose normalisation can be steered to chosen
samples (C.to_u16).
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import encode_cells as C

T = 64
FRAME = C.FRAME
LO, HI = C.LO, C.HI
L, H, _ = "lo", "hi", None
# what samples 0..3 hold: the low extreme, the high extreme, or the signal
STEPS = {"a": (L, H, _, _), "b": (_, _, L, H), "c": (H, H, L, L), "d": (_, L, H, H), "e": (L, _, _, H),
         "f": (H, L, H, L)}
THUE_MORSE = (1, -1, -1, 1, -1, 1, 1, -1)


def _stepped(x, step, lo, hi):
    x = np.array(x, dtype=np.int64)
    for i, s in enumerate(STEPS[step]):
        if s is not None:
            x[i] = lo if s == L else hi
    return x


def _poly_levels(order, c, block):
    """8-bit levels whose (order - 1)-th difference is +-c, constant over blocks of `block` samples with Thue-Morse
    signs (2^(order - 1) blocks sum to nothing in every moment below order - 1, so the sums stay bounded):
    polynomial pieces of degree order - 1, whose order-th difference is 0 but at the block edges"""
    d = np.repeat(np.resize(np.asarray(THUE_MORSE[:max(1, 1 << (order - 1))]), -(-FRAME // block)), block)[:FRAME] * c
    x = d.astype(np.int64)
    for _ in range(order - 1):
        x = np.cumsum(x)
    x = x - (int(x.max()) + int(x.min())) // 2 + 128
    assert 1 <= x.min() and x.max() <= 254, (order, c, block, int(x.min()), int(x.max()))
    return x


# (kind, parameters, step): "walk" = (order, step amplitude, peak) in 16-bit samples (C.walk), "poly" = (order, c, block)
# in 8-bit levels.  Seventeen one-frame tiles.
TILES = [
    ("walk", (1, 2.0, 20000), "a"), ("poly", (2, 5, 40), "b"), ("walk", (0, 3, 3), "c"), ("walk", (2, 0.5, 30000), "a"),
    ("poly", (3, 1, 12), "d"), ("walk", (1, 30, 30000), "f"), ("poly", (2, 3, 60), "e"), ("walk", (0, 40, 40), "b"),
    ("walk", (3, 0.01, 30000), "c"), ("poly", (4, 1, 5), "a"), ("walk", (1, 2.0, 20000), "d"), ("poly", (3, 1, 10), "f"),
    ("walk", (2, 5, 30000), "b"), ("walk", (0, 3, 3), "e"), ("poly", (2, 7, 30), "c"), ("walk", (3, 1.0, 30000), "d"),
    ("walk", (1, 30, 30000), "b"),
]


def _tile_u16(t, seed):
    """the uint16 samples of tile t (4096): both extremes sit in samples 0..3"""
    kind, par, step = TILES[t]
    if kind == "poly":
        return (_stepped(_poly_levels(*par), step, 0, 255) * 257).astype(np.uint16)
    order, step_amp, amp = par
    x = C.walk(step_amp, seed * 100 + t, order, amp=amp)(FRAME) if order else C.noise(int(step_amp), seed * 100 + t)(FRAME)
    return C.to_u16(_stepped(x, step, LO, HI))[0]


def _as_dtype(u16, dtype):
    """uint16 as it is; int16 halved and recentred (the reference's int16 arithmetic wraps on a wider range), uint8 the
    8-bit levels: as tests/encode_cells.py does.  The int16 and uint8 tiles normalise to other samples of the same
    shape; what they code as is asserted per dtype."""
    if dtype == "uint16":
        return u16
    if dtype == "int16":
        return ((u16 >> 1).astype(np.int32) - 16383).astype(np.int16)
    return (u16 // 257).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _row(dtype, seed=1):
    band = np.concatenate([_as_dtype(_tile_u16(t, seed), dtype).reshape(T, T) for t in range(len(TILES))], axis=1)
    band = np.ascontiguousarray(band)
    band.setflags(write=False)
    return band, O.encode_tiles(band, T, C.RATE)


def _census_tiles(ref, per_tile):
    arena, off = ref[0].tobytes(), [int(o) for o in ref[1]]
    return [O.subframe_census(arena[off[t]:off[t + 1]], 1, 16, per_tile) for t in range(len(off) - 1)]


@pytest.mark.parametrize("dtype", ["uint16", "int16", "uint8"])
def test_oracle_codes_the_stepped_tiles_fixed(dtype):
    """(CPU) the oracle codes at least 12 of the 17 tiles FIXED, with at least three different orders, and the step
    is there: each tile's first four samples hold both of its extremes"""
    band, ref = _row(dtype)
    span = {"uint16": 65534, "int16": 32767, "uint8": 254}[dtype]
    for t in range(len(TILES)):
        tile = band[:, t * T:(t + 1) * T].reshape(-1).astype(np.int64)
        assert tile[:4].min() == tile.min() and tile[:4].max() == tile.max(), t
        assert int(tile.max()) - int(tile.min()) >= span, t
    subs = [c[0] for c in _census_tiles(ref, FRAME)]
    fixed = [c["order"] for c in subs if c["kind"] == "fixed"]
    print(dtype, [f"{c['kind'][0]}{c['order']}" for c in subs])
    assert len(fixed) >= 12 and len(set(fixed)) >= 3, fixed
    # in one ticket of eight frames: more than one kind of frame
    assert len({(c["kind"], c["order"]) for c in subs[:8]}) >= 3


# ---- wasted bits: 128 x 128 tiles, frame 0 an anchor with both extremes, frames 1..3 three of the signals << w
def _wasted_signal(t, w, seed):
    kind, par, step = TILES[t]
    lo, hi = -(HI >> w), HI >> w
    if kind == "poly":
        x = (_poly_levels(*par) - 128) * (64 >> w)
    else:
        order, step_amp, amp = par
        x = (C.walk(step_amp, seed * 100 + t, order, amp=amp)(FRAME) if order else
             C.noise(int(step_amp), seed * 100 + t)(FRAME)) >> w
    return _stepped(x, step, lo, hi) << w


def _anchor():
    x = C.walk(30, 7, 1)(FRAME).copy()
    x[100], x[200] = LO, HI
    return x


WASTED_TILES = [0, 1, 3, 4, 5, 7, 8, 9, 12]   # three 128 x 128 tiles' frames 1..3


@functools.lru_cache(maxsize=None)
def _wasted_band(dtype, w, seed=1):
    cols = []
    for g in range(0, len(WASTED_TILES), 3):
        frames = [_anchor()] + [_wasted_signal(t, w, seed) for t in WASTED_TILES[g:g + 3]]
        raw = np.concatenate([C.to_u16(x)[0] for x in frames])
        cols.append(_as_dtype(raw, dtype).reshape(128, 128))
    band = np.ascontiguousarray(np.concatenate(cols, axis=1))
    band.setflags(write=False)
    return band, O.encode_tiles(band, 128, C.RATE)


@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("dtype", ["uint16"])
def test_oracle_codes_the_wasted_bits_tiles_fixed(dtype, w):
    """(CPU) frames 1..3 of every tile have exactly w wasted bits; at least six of the nine are FIXED, of at least
    three orders"""
    band, ref = _wasted_band(dtype, w)
    subs = [c for tile in _census_tiles(ref, 4 * FRAME) for c in tile[1:]]
    print(dtype, w, [f"{c['kind'][0]}{c['order']}w{c['wasted']}" for c in subs])
    assert len(subs) == len(WASTED_TILES) and all(c["wasted"] == w for c in subs)
    fixed = [c["order"] for c in subs if c["kind"] == "fixed"]
    assert len(fixed) >= 6 and len(set(fixed)) >= 3, fixed


# ---- streams: [bands, 64 * frames, 64], frame 0 an anchor in every band, then the signals (w wasted bits)
@functools.lru_cache(maxsize=None)
def _stream(bands, w, seed=1):
    sig = [_wasted_signal(t, w, seed) for t in range(len(TILES))]
    n = len(sig)
    if bands == 2:   # a signal beside its successor: L, R, mid and the 17-bit side of two stepped frames
        chans = [[_anchor()] + sig, [_anchor()] + sig[1:] + sig[:1]]
    else:            # every band holds all of them, band b starting a b-th of the way in
        chans = [[_anchor()] + sig[b * n // bands:] + sig[:b * n // bands] for b in range(bands)]
    arr = np.stack([np.concatenate([C.to_u16(x)[0] for x in ch]).reshape(-1, T) for ch in chans])
    arr.setflags(write=False)
    pcm, mn, mx, bps = O.normalize(arr.transpose(1, 2, 0).reshape(-1, bands))
    assert bps == 16
    return arr, (O.encode_frames(pcm, bps, C.RATE), pcm, mn, mx)


@pytest.mark.parametrize("w", [0, 1, 3])
@pytest.mark.parametrize("bands", [2, 3])
def test_oracle_codes_the_streams_fixed(bands, w):
    """(CPU) after the anchor frame: w wasted bits in every L / R (or band) subframe, FIXED of at least three orders"""
    arr, (frames, pcm, mn, mx) = _stream(bands, w)
    subs = [c for c in O.subframe_census(frames, bands, 16, len(pcm)) if c["frame"] > 0]
    print(bands, w, [f"{c['assignment']}:{c['kind'][0]}{c['order']}w{c['wasted']}" for c in subs])
    assert len(subs) == bands * len(TILES)
    if bands == 3:
        assert all(c["wasted"] == w for c in subs)
    else:
        assert all(c["wasted"] >= w for c in subs) and sum(c["wasted"] == w for c in subs) >= len(TILES)
    fixed = [c["order"] for c in subs if c["kind"] == "fixed"]
    assert len(fixed) >= bands * 6 and len(set(fixed)) >= 3, fixed


# ---------------------------------------------------------------------------------------------------------- the GPU
def _check_tiles(ctx, band, tile, ref):
    Hh, W = band.shape
    d = ctx.make_desc(Hh, W, band.dtype, tile_h=tile, tile_w=tile, sample_rate=C.RATE, bits_per_sample=16)
    arena, off, mn, mx, bps = ctx.encode_tiles_host(np.ascontiguousarray(band), d)
    o_arena, o_off, o_mn, o_mx = ref
    assert bps == 16
    assert list(off) == list(o_off)
    assert arena.tobytes() == o_arena.tobytes()
    assert list(mn) == list(o_mn) and list(mx) == list(o_mx)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint16", "int16", "uint8"])
def test_stepped_tiles(gpu_ctx, dtype):
    band, ref = _row(dtype)
    _check_tiles(gpu_ctx, band, T, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("dtype", ["uint16"])
def test_stepped_tiles_with_wasted_bits(gpu_ctx, dtype, w):
    band, ref = _wasted_band(dtype, w)
    _check_tiles(gpu_ctx, band, 128, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [0, 1, 3])
@pytest.mark.parametrize("bands", [2, 3])
def test_stepped_streams(gpu_ctx, bands, w):
    """two bands: the L / R / M units (and the wide side); three bands: the subframe units"""
    arr, (frames, pcm, r_mn, r_mx) = _stream(bands, w)
    Hh, W = arr.shape[-2:]
    d = gpu_ctx.make_desc(Hh, W, arr.dtype, nbands=bands, tile_h=Hh, tile_w=W, sample_rate=C.RATE, bits_per_sample=16)
    gpu_ctx.profile(True)
    gpu_ctx.profile_reset()
    arena, off, mn, mx, bps = gpu_ctx.encode_tiles_host(np.ascontiguousarray(arr), d)
    compact = gpu_ctx.profile_avg_ms("compact")
    gpu_ctx.profile(False)
    assert compact < 0, "expected the multi-channel fast path"
    assert bps == 16 and len(off) == 2 and int(off[0]) == 0 and int(off[1]) == len(frames)
    assert arena.tobytes() == frames
    assert (mn[0], mx[0]) == (r_mn, r_mx)
