"""The tile normalisation on the GPU at every range edge, on every encode path.

Rasters of ramp tiles: every tile holds EVERY value from min to min + R (asserted: the coverage is the tests' own
precondition), for R on both sides of each cut-off of tile_norm_finalize (LUT up to R = 4095, reciprocal up to 65535
while x - min cannot wrap, the division otherwise), with min at the dtype's minimum, at 0 and at max - R.  Two
arrangements per tile: the ramp ascending and repeated, and a slow triangle wave whose samples are shuffled within a
few positions (the same values, +- a few of the wave): frames whose LPC decisions depend on the normalised samples.

Per raster, three exact assertions:
 1. the GPU's frames decoded (decode_frames_host, pinned by test_gpu_decode_layouts.py) equal NUMPY's expression on
    each tile -- not the oracle: this ties the encoder's samples to numpy directly;
 2. arena and tile offsets equal the oracle's.  The analysis normalises with copies of its own (ana_norm, the LUT
    k_analyze_v3 builds in LDS), whose errors change decisions (predictor, precision, and the wasted-bits count,
    through which a gross error there reaches the samples too): this is the only check that sees them, and it is
    weak against a single wrong sample there, because one sample rarely moves a quantised coefficient;
 3. the reported min / max equal the tile's true extremes.
Each test asserts its route through the per-kernel profile the way the older tests do ("stats" is timed only when the
separate statistics kernels run, "compact" only on the generic kernels, "assemble" on the multi-channel fast paths).
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_normalize_host import _numpy_normalize

gpu = pytest.mark.gpu

LIMITS = {np.dtype(np.uint8): (0, 255), np.dtype(np.uint16): (0, 65535), np.dtype(np.int16): (-32768, 32767)}
CUT_R = (1, 2, 3, 7, 4093, 4094, 4095, 4096, 4097, 8191, 8192, 32766, 32767, 32768, 32769, 65521, 65534, 65535)
EXTRA_R = tuple(int(r) for r in np.random.default_rng(20261019).integers(8, 65521, 8))  # drawn once: the seed is fixed


def tile_size(R):
    """the smallest tiles that hold the whole ramp: one frame, sixteen frames"""
    return 64 if R <= 4095 else 256


def mins_for(dtype, R):
    lo, hi = LIMITS[np.dtype(dtype)]
    return [m for m in sorted({lo, 0, hi - R}) if lo <= m and m + R <= hi]


def ramp(n, R, smooth, seed):
    """n >= R + 1 values that include every integer of 0..R"""
    assert n >= R + 1
    if not smooth:
        return np.arange(n, dtype=np.int64) % (R + 1)
    # triangle wave of h monotone passes over 0..R (each at least R + 1 samples long: slope <= 1, no integer skipped).
    # A handful of levels (R <= 7) makes no slow wave that a predictor gains on, so there the passes are R + 1 long: a
    # wave of period 2 R + 2 whose normalised samples obey x[n] = -x[n - R - 1], which LPC follows and no fixed
    # predictor does
    fastwave = R <= 7
    h = n // (R + 1) if fastwave else max(1, min(6, n // (2 * (R + 1))))
    edges = np.linspace(0, n, h + 1).astype(np.int64)
    parts = []
    for p in range(h):
        seg = np.rint(np.linspace(0, R, int(edges[p + 1] - edges[p]))).astype(np.int64)
        parts.append(seg if p % 2 == 0 else seg[::-1])
    v = np.concatenate(parts)
    rng = np.random.default_rng(seed)
    if fastwave:  # dither: about n / 64 swaps of neighbours
        for i in rng.choice(n - 1, n // 64, replace=False):
            v[i], v[i + 1] = v[i + 1], v[i]
        return v
    # dither: shuffle within a window of positions that spans about +-3 values of the wave (the values stay the same)
    w = int(np.clip(round(3.0 * n / (h * (R + 1))), 2, 64))
    return v[np.argsort(np.arange(n) + rng.uniform(0, w, n), kind="stable")]


def ramp_tile(dtype, T, mn, R, smooth, seed):
    return (ramp(T * T, R, smooth, seed) + mn).astype(dtype).reshape(T, T)


def specs_for(dtype, T):
    """(R, min, smooth) of every tile of the dtype's raster of tile size T"""
    dtype = np.dtype(dtype)
    Rs = range(1, 256) if dtype == np.uint8 else sorted(set(CUT_R + EXTRA_R))
    return [(R, mn, smooth) for R in Rs if tile_size(R) == T for mn in mins_for(dtype, R) for smooth in (False, True)]


@functools.lru_cache(maxsize=None)
def raster(dtype, T):
    """-> (band, specs): the tiles side by side, row-major; the last row is filled up with copies of the first tiles"""
    specs = specs_for(dtype, T)
    ncol = 8 if len(specs) <= 128 else 32
    while len(specs) % ncol:
        specs.append(specs[len(specs) % ncol])
    band = np.empty((len(specs) // ncol * T, ncol * T), dtype)
    for i, (R, mn, smooth) in enumerate(specs):
        r, c = divmod(i, ncol)
        band[r * T:(r + 1) * T, c * T:(c + 1) * T] = ramp_tile(dtype, T, mn, R, smooth, i)
    band.setflags(write=False)
    return band, specs


def tiles_of(band, T):
    return [band[r:r + T, c:c + T] for r in range(0, band.shape[0], T) for c in range(0, band.shape[1], T)]


@functools.lru_cache(maxsize=None)
def oracle_tiles(dtype, T):
    return O.encode_tiles(raster(dtype, T)[0], T, threads=8)


def lpc_fraction(arena, off, tiles, pick):
    """share of LPC subframes among the frames of the picked tiles (oracle decode of the given frames)"""
    lpc = total = 0
    for t, tile in enumerate(tiles):
        if pick[t]:
            types = O.subframe_types(arena[off[t]:off[t + 1]].tobytes(), 1, 16, tile.size)[:, 0]
            lpc += int(np.count_nonzero(types >= 32))
            total += types.size
    return lpc / total


RASTERS = [(np.uint16, 64), (np.uint16, 256), (np.int16, 64), (np.int16, 256), (np.uint8, 64)]


@pytest.mark.parametrize("dtype,T", RASTERS)
def test_ramp_rasters_cover_their_ranges_and_smooth_tiles_are_lpc(dtype, T):
    """CPU: every tile holds all R + 1 values at its min; the cut-offs are present on both sides; and the oracle codes
    more than half of the smooth tiles' frames as LPC (so their bytes depend on the analysis' normalised samples)."""
    band, specs = raster(dtype, T)
    tiles = tiles_of(band, T)
    assert len(tiles) == len(specs)
    for tile, (R, mn, smooth) in zip(tiles, specs):
        assert np.unique(tile).size == R + 1 and int(tile.min()) == mn and int(tile.max()) == mn + R, (R, mn, smooth)
    if np.dtype(dtype) != np.uint8:
        have = {R for R, _, _ in specs}
        assert have == {R for R in set(CUT_R + EXTRA_R) if tile_size(R) == T} and len(set(EXTRA_R)) == 8
        lo, hi = LIMITS[np.dtype(dtype)]
        assert {mn for _, mn, _ in specs} >= {lo, 0} and any(mn + R == hi and mn != lo for R, mn, _ in specs)
    else:
        assert {R for R, _, _ in specs} == set(range(1, 256))
    arena, off, _, _ = oracle_tiles(dtype, T)
    assert lpc_fraction(arena, off, tiles, [s[2] for s in specs]) > 0.5


def _encode(ctx, band, T=None, nbands=1, bits=16):
    """encode (T: square tiles; None: the whole raster as one tile) -> (encode_tiles_host's tuple, profile entries)"""
    H, W = band.shape[-2:]
    view = not band.flags.c_contiguous
    d = ctx.make_desc(H, W, band.dtype, nbands=nbands, tile_h=T or H, tile_w=T or W, sample_rate=44100,
                      bits_per_sample=bits, row_stride=band.strides[-2] // band.itemsize if view else None)
    ctx.profile(True)
    ctx.profile_reset()
    out = ctx.encode_tiles_host(band, d)
    prof = {k: ctx.profile_avg_ms(k) for k in ("stats", "compact", "assemble")}
    ctx.profile(False)
    return out, prof


def _check_tiles(ctx, got, band, T, ref, bps=16):
    """the three assertions, for a single-band raster of tiles"""
    arena, off, mn, mx, sbps = got
    o_arena, o_off, _, _ = ref
    tiles = tiles_of(band, T)
    assert sbps == bps
    pcm = ctx.decode_frames_host(arena, off, [t.size for t in tiles], channels=1, bps=bps)[:, 0]
    pos = 0
    for i, tile in enumerate(tiles):                                          # 1. samples == numpy
        want = _numpy_normalize(np.ascontiguousarray(tile).reshape(-1))
        bad = np.flatnonzero(pcm[pos:pos + tile.size] != want)
        assert bad.size == 0, (i, int(tile.min()), int(tile.max()), bad[:4], pcm[pos + bad[:4]], want[bad[:4]])
        pos += tile.size
    assert list(off) == list(o_off)                                           # 2. decisions == oracle
    assert arena.tobytes() == o_arena.tobytes()
    if band.dtype.kind != "f":                                                # 3. extremes
        assert list(mn) == [float(t.min()) for t in tiles] and list(mx) == [float(t.max()) for t in tiles]


@gpu
@pytest.mark.parametrize("dtype,T", RASTERS[:4])
def test_fused_stats_fast_path(gpu_ctx, dtype, T):
    """16-bit samples, 16-byte aligned rows, tiles of <= 64 frames: min / max, the mode and the LUT come from
    k_analyze_v3<..., STATS> itself (tile_norm_finalize and lut_entry in the analysis launch)."""
    band, _ = raster(dtype, T)
    got, prof = _encode(gpu_ctx, band, T)
    assert prof["stats"] <= 0 and prof["compact"] < 0, prof
    _check_tiles(gpu_ctx, got, band, T, oracle_tiles(dtype, T))


@gpu
@pytest.mark.parametrize("dtype,T", RASTERS[:4])
def test_separate_stats_rows_not_16_byte_runs(gpu_ctx, dtype, T):
    """The same tiles as a window of a raster 4 samples wider: rows start on 8-byte boundaries only, so k_tile_stats,
    k_tile_finalize and k_build_lut run before the analysis."""
    band, _ = raster(dtype, T)
    wide = np.zeros((band.shape[0], band.shape[1] + 4), band.dtype)
    wide[:, :-4] = band
    got, prof = _encode(gpu_ctx, wide[:, :-4], T)
    assert prof["stats"] > 0 and prof["compact"] < 0, prof
    _check_tiles(gpu_ctx, got, band, T, oracle_tiles(dtype, T))


@gpu
@pytest.mark.parametrize("dtype,mn,smooth", [(np.uint16, 0, False), (np.uint16, 0, True), (np.int16, -32768, True)])
def test_separate_stats_tile_of_256_frames(gpu_ctx, dtype, mn, smooth):
    """One 1024 x 1024 tile (more than 64 frames: never fused) holding a 65535 ramp: the reciprocal for uint16, the
    wrapping division for int16."""
    band = ramp_tile(dtype, 1024, mn, 65535, smooth, 5)
    assert np.unique(band).size == 65536
    got, prof = _encode(gpu_ctx, band, 1024)
    assert prof["stats"] > 0 and prof["compact"] < 0, prof
    _check_tiles(gpu_ctx, got, band, 1024, O.encode_tiles(band, 1024, threads=8))


@gpu
def test_separate_stats_uint8(gpu_ctx):
    """uint8 never takes the fused form; every R from 1 to 255 (all LUT tiles)."""
    band, _ = raster(np.uint8, 64)
    got, prof = _encode(gpu_ctx, band, 64)
    assert prof["stats"] > 0 and prof["compact"] < 0, prof
    _check_tiles(gpu_ctx, got, band, 64, oracle_tiles(np.uint8, 64))


@gpu
@pytest.mark.parametrize("dtype,T", RASTERS)
def test_generic_kernels(gpu_ctx, dtype, T, monkeypatch):
    """A context created under FRS_FORCE_GENERIC=1: Normalizer::operator() and its reciprocal branch (k_analyze*,
    k_encode_frames, k_compact)."""
    from flac_raster_amd import _native
    monkeypatch.setenv("FRS_FORCE_GENERIC", "1")
    band, _ = raster(dtype, T)
    with _native.Context(0) as ctx:
        got, prof = _encode(ctx, band, T)
        assert prof["compact"] > 0, prof
        _check_tiles(gpu_ctx, got, band, T, oracle_tiles(dtype, T))


def _band_ramps(dtype, nb, H, W, mn, R, smooth):
    """nb bands, each a ramp over its own part of min..min + R; together they reach both ends"""
    span = R // 2
    bands = []
    for b in range(nb):
        lo = mn + (R - span) * b // (nb - 1)
        bands.append((ramp(H * W, span, smooth, 40 + b) + lo).astype(dtype).reshape(H, W))
    data = np.stack(bands)
    assert int(data.min()) == mn and int(data.max()) == mn + R
    assert all(np.unique(b).size == span + 1 for b in bands)
    return data


# 4095 / 4096: the LUT cut-off.  4096 is a power of two, where the reciprocal is exact by itself; 4430 is the second
# range above it with 2 R * RN(1 / R) < 2 (4237 is the first): there only the correction step makes the top value 32767
MULTI = [(dt, mn, R, smooth) for dt in (np.uint16, np.int16) for R in (4095, 4096, 4430) for smooth in (False, True)
         for mn in mins_for(dt, R)[:1] + mins_for(dt, R)[-1:]]


def _check_stream(ctx, data, got, prof, fast_key):
    """one stream of interleaved bands (converter.py:185-216): min / max over all bands, as O.normalize takes them"""
    arena, off, mn, mx, bps = got
    nb, H, W = data.shape
    inter = np.ascontiguousarray(data.transpose(1, 2, 0).reshape(-1, nb))
    assert prof["compact"] < 0 and (fast_key is None or prof[fast_key] > 0), prof
    pcm = ctx.decode_frames_host(arena, [0, len(arena)], [H * W], channels=nb, bps=16)
    assert np.array_equal(pcm, _numpy_normalize(inter))                       # 1. samples == numpy
    o_pcm, o_mn, o_mx, o_bps = O.normalize(inter)
    assert bps == o_bps == 16
    assert arena[:off[-1]].tobytes() == O.encode_frames(o_pcm, o_bps, 44100)  # 2. decisions == oracle
    assert (mn[0], mx[0]) == (float(data.min()), float(data.max())) == (o_mn, o_mx)   # 3. extremes


@gpu
@pytest.mark.parametrize("dtype,mn,R,smooth", MULTI)
def test_three_band_convert(gpu_ctx, dtype, mn, R, smooth):
    """Plain convert of three bands as one stream on the multi-channel fast path, on either side of the LUT cut-off."""
    data = _band_ramps(dtype, 3, 64, 128, mn, R, smooth)
    got, prof = _encode(gpu_ctx, data, nbands=3)
    _check_stream(gpu_ctx, data, got, prof, "assemble")


@gpu
@pytest.mark.parametrize("dtype,mn,R,smooth", MULTI)
def test_two_band_stream(gpu_ctx, dtype, mn, R, smooth):
    """Two bands: libFLAC forms mid and side from the NORMALISED samples (orc_encode_frames_level through
    O.encode_frames); 16-bit streams stay on the fast two-channel kernels."""
    data = _band_ramps(dtype, 2, 64, 128, mn, R, smooth)
    got, prof = _encode(gpu_ctx, data, nbands=2)
    _check_stream(gpu_ctx, data, got, prof, None)


def _wide_rasters():
    """name -> (band, tile): 32-bit scale (8388607, int32 samples, 32-bit streams), |x| < 256 for the floats"""
    rng = np.random.default_rng(7)
    T = 272                                                    # 73984 samples: the smallest square over 70001
    i32 = np.concatenate([ramp_tile(np.int32, T, m, 70000, s, 3) for m in (-2 ** 31, -7, 2 ** 31 - 1 - 70000)
                          for s in (False, True)], axis=1)
    u32 = np.concatenate([ramp_tile(np.uint32, T, m, 70000, s, 4) for m in (0, 2 ** 32 - 1 - 70000)
                          for s in (False, True)], axis=1)
    over = rng.integers(-2 ** 30, 2 ** 30 + 6, (128, 256)).astype(np.int32)
    over[0, :2] = over[64, 128:130] = [-2 ** 30, 2 ** 30 + 5]  # range 2^31 + 5 in either tile: max - min wraps
    ufull = rng.integers(0, 2 ** 32, (128, 256)).astype(np.uint32)
    ufull[0, :2] = ufull[64, 128:130] = [0, 2 ** 32 - 1]
    t = np.linspace(0, 40, 128 * 256)
    f = (120 * np.sin(t) + rng.normal(0, 0.5, t.size)).clip(-255.9, 255.9)
    f[:4] = [-255.99, 255.99, 0.0, -0.0]
    f = f.reshape(128, 256)
    return {"i32_ramps": (i32, T), "u32_ramps": (u32, T), "i32_over_2^31": (over, 128), "u32_full": (ufull, 128),
            "f32": (f.astype(np.float32), 128), "f64": (f.astype(np.float64), 128)}


@gpu
@pytest.mark.parametrize("name", list(_wide_rasters()))
def test_32_bit_scale(gpu_ctx, name):
    """int32, uint32 and float rasters on the generic kernels (the fast paths are 16-bit).  Floats of |x| >= 256 are
    left out here: they give INT32_MIN samples, which tests/wide_cells.py places frame by frame (NaN, +-inf, 257.0,
    -300.0) and tests/test_gpu_wide_cells.py compares with the oracle's restatement of libFLAC's limit_residual
    routines."""
    band, T = _wide_rasters()[name]
    if name.endswith("ramps"):
        assert all(np.unique(t).size == 70001 for t in tiles_of(band, T))
    got, prof = _encode(gpu_ctx, band, T, bits=24)
    assert prof["compact"] > 0, prof
    _check_tiles(gpu_ctx, got, band, T, O.encode_tiles(band, T, threads=8), bps=32)
