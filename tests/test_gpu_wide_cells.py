"""The generic 32-bit encode path (int32, uint32, float32 and float64 rasters: bits_per_sample 24, stream bps 32), byte
for byte against the oracle on the corpus of tests/wide_cells.py, and the oracle's streams through the wave decoder.

tests/test_wide_cells_host.py holds (on the CPU) that the oracle's output on these rasters reaches every coded form:
VERBATIM, FIXED and LPC under wasted bits on both sides of subframe_bps 28 (where libFLAC changes the fixed-predictor
estimator), CONSTANT below 28 and FIXED 1 for a constant block from 28 on, FIXED 0..4 with ties and totals past 2^32,
INT32_MIN samples (NaN, +-inf, |x| > 256) that put fixed orders and LPC candidates out, LPC 1..12 at precision 15 with
clamped coefficients on full-scale samples, partition orders 0..6, both Rice methods up to parameter 30, every
two-band assignment with sides of 27, 28 and 33 bits, and last frames of 1024, 11 and 3 samples.  Here k_analyze<WIDE>,
k_analyze_fixed_wide, k_analyze_lpc_hi<WIDE> and k_encode_frames (int64 samples for the 33-bit side) code the same
rasters and must write the oracle's arena bytes, tile offsets, min / max and bps 32.  Every assertion is exact equality.
"""
import numpy as np
import pytest

from flac_raster_amd import geotiff
from flac_raster_amd.converter import RasterFLACConverter
from oracle import oracle as O
from oracle import pipeline as P
from tests import wide_cells as W
from tests.test_gpu_decode import _decoder_ctx

pytestmark = pytest.mark.gpu

PROFILE = ("stats", "partial", "assemble", "compact")


def _encode(ctx, arr, tile=None, level=5):
    """arr [H, W] at `tile` (an int, or (th, tw)), or [bands, H, W] as one stream -> (encode_tiles_host's tuple,
    profile entries)"""
    bands = arr.shape[0] if arr.ndim == 3 else 1
    H, W_ = arr.shape[-2:]
    th, tw = (H, W_) if tile is None else (tile, tile) if isinstance(tile, int) else tile
    d = ctx.make_desc(H, W_, arr.dtype, nbands=bands, tile_h=th, tile_w=tw, sample_rate=W.RATE, bits_per_sample=24,
                      compression_level=level)
    ctx.profile(True)
    ctx.profile_reset()
    out = ctx.encode_tiles_host(np.ascontiguousarray(arr), d)
    prof = {k: ctx.profile_avg_ms(k) for k in PROFILE}
    ctx.profile(False)
    assert prof["compact"] >= 0, f"expected the generic kernels: {prof}"
    return out


def _first_difference(data, ref, bands, nsamples, names):
    """the first subframe, by the oracle's census of its own stream, whose frame holds a differing byte"""
    if data == ref:
        return None
    at = next((i for i, (a, b) in enumerate(zip(data, ref)) if a != b), min(len(data), len(ref)))
    cen = O.subframe_census(ref, bands, 32, nsamples)
    starts = [i for i in range(len(ref) - 1) if ref[i] == 0xFF and ref[i + 1] == 0xF8]   # (sync codes; may overcount)
    frame = max(0, sum(1 for s in starts if s <= at) - 1)
    here = [c for c in cen if c["frame"] == min(frame, cen[-1]["frame"])]
    return (f"byte {at} of {len(ref)} (GPU {len(data)}), about frame {frame}: "
            + "; ".join(f"{names[c['frame'] * bands + c['channel']] if names else ''} {c['kind']} {c['order']} "
                        f"w{c['wasted']} po{c['porder']} shift {c['shift']}" for c in here))


def _same(a, b):
    """extremes equal value for value; a tile or stream that holds a NaN has NaN for both (np.min / np.max)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _check_tiles(got, ref, samples_per_tile, names, what):
    arena, off, mn, mx, bps = got
    data, r_off, r_mn, r_mx = ref
    assert bps == 32, what
    bad = []
    ntiles = len(r_off) - 1
    per = len(names) // ntiles
    for t in range(ntiles):
        mine = arena[int(off[t]):int(off[t + 1])].tobytes() if t + 1 < len(off) else b""
        diff = _first_difference(mine, data[r_off[t]:r_off[t + 1]], 1, samples_per_tile, names[t * per:(t + 1) * per])
        if diff:
            bad.append(f"{what} tile {t}: {diff}")
    assert not bad, f"{len(bad)} tiles differ\n" + "\n".join(bad[:40])
    assert [int(o) for o in off] == r_off and arena.tobytes() == data, what
    assert _same(mn, r_mn), (what, "min", list(mn), r_mn)
    assert _same(mx, r_mx), (what, "max", list(mx), r_mx)


def _check_stream(got, ref, bands, names, what):
    arena, off, mn, mx, bps = got
    frames, pcm, r_mn, r_mx = ref
    assert bps == 32 and len(off) == 2 and int(off[0]) == 0, (what, list(off))
    diff = _first_difference(arena[:int(off[1])].tobytes(), frames, bands, len(pcm), names)
    assert diff is None, f"{what}: {diff}"
    assert int(off[1]) == len(frames) == len(arena), (what, list(off), len(frames), len(arena))
    assert _same([mn[0], mx[0]], [r_mn, r_mx]), (what, mn[0], mx[0], r_mn, r_mx)


# ------------------------------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("dtype", ["float64", "float32", "int32", "uint32"])
def test_mono_tiles_at_level_5(gpu_ctx, dtype):
    got = _encode(gpu_ctx, W.mono_band(dtype), W.TILE)
    _check_tiles(got, W.tiles_reference("mono", dtype), 4 * W.FRAME, W.mono_names(dtype), dtype)


@pytest.mark.parametrize("level", [0, 8])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mono_tiles_at_levels_0_and_8(gpu_ctx, dtype, level):
    """level 0: fixed predictors only, partition orders to 3; level 8: k_analyze_lpc_hi's window candidates, LPC
    orders to 12, partition orders to 6"""
    got = _encode(gpu_ctx, W.mono_band(dtype), W.TILE, level=level)
    _check_tiles(got, W.tiles_reference("mono", dtype, level), 4 * W.FRAME, W.mono_names(dtype), f"{dtype} level {level}")


def test_partial_last_frames(gpu_ctx):
    """96 x 96 tiles (1024-sample tails), and one-row tiles of a frame and 11 or 3 samples"""
    got = _encode(gpu_ctx, W.partial_band(), W.PTILE)
    _check_tiles(got, W.tiles_reference("partial"), W.PTILE ** 2, [n for n, _ in W.partial_frames()], "partial")
    for tail in (11, 3):
        band = W.tiny_band(tail)
        got = _encode(gpu_ctx, band, (1, band.shape[1]))
        _check_tiles(got, W.tiles_reference(f"tiny{tail}"), band.shape[1], W.tiny_names(), f"tail {tail}")


def test_three_band_stream(gpu_ctx):
    got = _encode(gpu_ctx, W.multi_raster(3))
    _check_stream(got, W.stream_reference(3), 3, W.multi_names(3), "three bands")


@pytest.mark.parametrize("level", [4, 5, 8])
def test_two_band_stream(gpu_ctx, level):
    """left, right, mid and the 33-bit side in int64; level 4: loose mid/side; level 8: window candidates per signal"""
    got = _encode(gpu_ctx, W.stereo_raster(), level=level)
    _check_stream(got, W.stream_reference(2, level), 2, W.stereo_names(), f"two bands level {level}")


# ------------------------------------------------------------------------------------------------------ decode
def _decode_tiles(ctx, ref, per):
    data, off = ref[0], ref[1]
    counts = [per] * (len(off) - 1)
    want = np.concatenate([O.decode_frames(data[off[t]:off[t + 1]], 1, 32, per) for t in range(len(counts))])
    got = ctx.decode_frames_host(np.frombuffer(data, dtype=np.uint8), off, counts, channels=1, bps=32)
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (bad.size, "first at sample", int(bad[0]), "frame", int(bad[0]) // W.FRAME)


def test_wave_decoder_reads_the_mono_corpus(monkeypatch):
    """The oracle's streams at level 5 and level 8 (LPC orders to 12, partition order 6), and the 96 x 96 tiles"""
    ctx = _decoder_ctx("wave", monkeypatch)
    try:
        _decode_tiles(ctx, W.tiles_reference("mono", "float64"), 4 * W.FRAME)
        _decode_tiles(ctx, W.tiles_reference("mono", "float64", 8), 4 * W.FRAME)
        _decode_tiles(ctx, W.tiles_reference("mono", "float32"), 4 * W.FRAME)
        _decode_tiles(ctx, W.tiles_reference("partial"), W.PTILE ** 2)
    finally:
        ctx.close()


@pytest.mark.parametrize("bands", [2, 3])
def test_wave_decoder_reads_the_multi_band_corpus(bands, monkeypatch):
    """Two bands: every assignment, sides of 27, 28 and 33 bits; three bands: the corpus dealt over them"""
    frames, pcm, mn, mx = W.stream_reference(bands)
    ctx = _decoder_ctx("wave", monkeypatch)
    try:
        got = ctx.decode_frames_host(np.frombuffer(frames, dtype=np.uint8), [0, len(frames)], [len(pcm)],
                                     channels=bands, bps=32).reshape(-1, bands)
        bad = np.flatnonzero((got != pcm).any(1))
        assert bad.size == 0, (bands, bad.size, "frames", np.unique(bad // W.FRAME).tolist()[:20])
    finally:
        ctx.close()


def test_default_context_sends_32_bit_streams_to_the_wave_decoder(gpu_ctx):
    gpu_ctx.profile(True)
    gpu_ctx.profile_reset()
    try:
        _decode_tiles(gpu_ctx, W.tiles_reference("mono", "float64"), 4 * W.FRAME)
        ran = {n: gpu_ctx.profile_avg_ms(n) for n in ("decode", "decode_frames", "lane_fallback_frames")}
    finally:
        gpu_ctx.profile(False)
    assert ran["decode_frames"] >= 0 and ran["lane_fallback_frames"] < 0, ran      # (no lane decoder ran)


# --------------------------------------------------------------------------------------------------- file level
def test_float32_dem_file_matches_the_oracle_pipeline(gpu_ctx, tmp_path):
    """A float32 DEM of whole-metre elevations in [32, 256) with a flat lake: every sample carries 5 or more wasted
    bits, the lake's frames are CONSTANT and the slopes go through the plain estimator."""
    H, Wd = 130, 300
    y, x = np.mgrid[0:H, 0:Wd]
    dem = np.rint(120.0 + 70.0 * np.sin(x / 37.0) * np.cos(y / 23.0) + W._rng(60).normal(0, 1.5, (H, Wd)))
    dem = np.clip(dem, 32, 255)
    dem[20:75, :] = 64.0                                       # the lake: 55 rows of 300, frames 2..4 entirely
    arr = dem.astype(np.float32)[None]
    t = geotiff.Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4000000.0)
    src = tmp_path / "dem.tif"
    geotiff.write(src, arr, t, 32636)
    r = geotiff.read(src)
    assert r.data.dtype == np.float32 and np.array_equal(r.data, arr)
    ref, _ = P.plain_convert(r.data, list(r.transform), r.crs_string, r.nodata, embed=True)
    pcm = W.samples(arr.reshape(-1))
    cen = O.subframe_census(O.encode_frames(pcm, 32, O.sample_rate_for(1, H)), 1, 32, pcm.size)
    assert all(c["wasted"] >= 5 for c in cen) and {"constant", "fixed"} <= {c["kind"] for c in cen}, \
        [(c["kind"], c["wasted"]) for c in cen]
    out = tmp_path / "dem.flac"
    RasterFLACConverter(gpu_ctx).tiff_to_flac(src, out)
    data = out.read_bytes()
    if data != ref:
        n = len(ref) - len(O.encode_frames(pcm, 32, O.sample_rate_for(1, H)))
        raise AssertionError(_first_difference(data[n:], ref[n:], 1, pcm.size, None))
