"""Every path of the GPU that codes subframes, byte for byte against the oracle on the corpus of tests/encode_cells.py.

tests/test_encode_cells_host.py holds (on the CPU) that the oracle's output on these inputs reaches every coded form:
FIXED 0..4 and LPC 1..8, partition orders 0..5 under both, Rice parameters 0..14, wasted bits under every subframe
kind, LPC shifts 7..14 and both clamped coefficient codes, ties of the fixed totals and of the two-channel choice, all
four assignments with CONSTANT, VERBATIM and wasted-bits sides.  Here each path encodes the same inputs -- the mono
fast path in three dtypes, partial last frames, the three- and eight-band subframe instances, the two-band L / R / M
and wide side instances, the generic kernels at level 5 and at level 8 -- and must write the oracle's arena bytes, tile
offsets and min / max; then the oracle's streams go through every decoder.  Every assertion is exact equality.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import encode_cells as C
from tests.test_gpu_decode import DECODERS, _decoder_ctx
from tests.test_gpu_tiny_frames import _ctx

pytestmark = pytest.mark.gpu

PROFILE = ("stats", "partial", "assemble", "compact")
DTYPES = ("uint16", "int16", "uint8")


def _encode(ctx, arr, tile=None, level=5):
    """arr [H, W] at `tile` x `tile`, or [bands, H, W] as one stream -> (encode_tiles_host's tuple, profile entries)"""
    bands = arr.shape[0] if arr.ndim == 3 else 1
    H, W = arr.shape[-2:]
    th, tw = (tile, tile) if tile else (H, W)
    d = ctx.make_desc(H, W, arr.dtype, nbands=bands, tile_h=th, tile_w=tw, sample_rate=C.RATE, bits_per_sample=16,
                      compression_level=level)
    ctx.profile(True)
    ctx.profile_reset()
    out = ctx.encode_tiles_host(np.ascontiguousarray(arr), d)
    prof = {k: ctx.profile_avg_ms(k) for k in PROFILE}
    ctx.profile(False)
    return out, prof


def _first_difference(data, ref, bands, nsamples, names):
    """the first subframe, by the oracle's census of its own stream, whose frame holds a differing byte"""
    if data == ref:
        return None
    at = next((i for i, (a, b) in enumerate(zip(data, ref)) if a != b), min(len(data), len(ref)))
    cen = O.subframe_census(ref, bands, 16, nsamples)
    starts = [i for i in range(len(ref) - 1) if ref[i] == 0xFF and ref[i + 1] == 0xF8]   # (sync codes; may overcount)
    frame = max(0, sum(1 for s in starts if s <= at) - 1)
    here = [c for c in cen if c["frame"] == min(frame, cen[-1]["frame"])]
    return (f"byte {at} of {len(ref)} (GPU {len(data)}), about frame {frame}: "
            + "; ".join(f"{names[c['frame'] * bands + c['channel']] if names else ''} {c['kind']} {c['order']} "
                        f"w{c['wasted']} po{c['porder']} shift {c['shift']}" for c in here))


def _check_tiles(got, ref, samples_per_tile, names, what):
    arena, off, mn, mx, bps = got
    data, r_off, r_mn, r_mx = ref
    assert bps == 16, what
    bad = []
    ntiles = len(r_off) - 1
    per = len(names) // ntiles
    for t in range(ntiles):
        mine = arena[int(off[t]):int(off[t + 1])].tobytes() if t + 1 < len(off) else b""
        diff = _first_difference(mine, data[r_off[t]:r_off[t + 1]], 1, samples_per_tile, names[t * per:(t + 1) * per])
        if diff:
            bad.append(f"{what} tile {t}: {diff}")
    assert not bad, "\n".join(bad[:10])
    assert [int(o) for o in off] == r_off and arena.tobytes() == data, what
    assert list(mn) == r_mn and list(mx) == r_mx, what


def _check_stream(got, ref, bands, names, what):
    arena, off, mn, mx, bps = got
    frames, pcm, r_mn, r_mx = ref
    assert bps == 16 and len(off) == 2 and int(off[0]) == 0, (what, list(off))
    diff = _first_difference(arena[:int(off[1])].tobytes(), frames, bands, len(pcm), names)
    assert diff is None, f"{what}: {diff}"
    assert int(off[1]) == len(frames) == len(arena), (what, list(off), len(frames), len(arena))
    assert (mn[0], mx[0]) == (r_mn, r_mx), what


def _mono_names():
    return [n for n, _ in C.frames()]


def _stereo_names():
    return [f"{n}/{ch}" for n, _, _ in C.stereo_frames() for ch in "LR"]


# ------------------------------------------------------------------------------------------------- 1. mono fast path
@pytest.mark.parametrize("tile", [C.TILE, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_mono_fast_path(gpu_ctx, dtype, tile):
    """Four-frame tiles (the corpus' cells as the host test counts them) and one-frame tiles (every frame normalised
    by its own extremes: other samples, the same kernels)."""
    got, prof = _encode(gpu_ctx, C.mono_band(dtype, tile), tile)
    assert prof["compact"] < 0, f"expected the fast path: {prof}"
    per = tile * tile // C.FRAME
    names = _mono_names()
    _check_tiles(got, C.tiles_reference("mono", dtype, tile), tile * tile, names[:len(names) // per * per], dtype)


# ------------------------------------------------------------------------------------------ 2. partial last frames
@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_last_frames(gpu_ctx, dtype):
    """96 x 96 tiles: k_analyze_partial and k_encode_frames on the 1024-sample tails, inside a fast job"""
    got, prof = _encode(gpu_ctx, C.partial_band(dtype), C.PTILE)
    assert prof["partial"] > 0 and prof["compact"] < 0, prof
    _check_tiles(got, C.tiles_reference("partial", dtype, C.PTILE), C.PTILE ** 2, [n for n, _ in C.partial_frames()],
                 dtype)


# -------------------------------------------------------------------------------- 3. three and eight bands, 4. two
@pytest.mark.parametrize("bands,dtype", [(3, "uint16"), (3, "uint8"), (8, "uint16"), (8, "int16")])
def test_subframe_instances_of_multi_band_streams(gpu_ctx, bands, dtype):
    got, prof = _encode(gpu_ctx, C.multi_raster(bands, dtype))
    assert prof["assemble"] > 0 and prof["compact"] < 0, f"expected the multi-channel fast path: {prof}"
    _check_stream(got, C.stream_reference(bands, dtype), bands, C.multi_names(bands), f"{bands} bands {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_band_streams(gpu_ctx, dtype):
    """L, R, M as packed pairs, the 17-bit side, st_pick: all four assignments, the ties, CONSTANT / VERBATIM /
    wasted-bits sides, and every corpus frame beside its successor"""
    got, prof = _encode(gpu_ctx, C.stereo_raster(dtype))
    assert prof["compact"] < 0, f"expected the fast stereo path: {prof}"
    _check_stream(got, C.stream_reference(2, dtype), 2, _stereo_names(), f"two bands {dtype}")


# -------------------------------------------------------------------------------------- 5. generic kernels, level 5
def test_generic_kernels_at_level_5(monkeypatch):
    ctx = _ctx(monkeypatch, FRS_FORCE_GENERIC="1")
    try:
        got, prof = _encode(ctx, C.mono_band("uint16"), C.TILE)
        assert prof["compact"] >= 0, prof
        _check_tiles(got, C.tiles_reference("mono", "uint16"), 4 * C.FRAME, _mono_names(), "generic mono")
        got, prof = _encode(ctx, C.partial_band("uint16"), C.PTILE)
        assert prof["compact"] >= 0, prof
        _check_tiles(got, C.tiles_reference("partial", "uint16", C.PTILE), C.PTILE ** 2,
                     [n for n, _ in C.partial_frames()], "generic partial")
        got, prof = _encode(ctx, C.stereo_raster("uint16"))
        assert prof["compact"] >= 0, prof
        _check_stream(got, C.stream_reference(2), 2, _stereo_names(), "generic two bands")
        got, prof = _encode(ctx, C.multi_raster(3, "uint16"))
        assert prof["compact"] >= 0, prof
        _check_stream(got, C.stream_reference(3), 3, C.multi_names(3), "generic three bands")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- 6. level 8
def _print_added(five, eight, what):
    added = sorted((c for c in eight if c not in five and c[0] in ("type", "porder", "shift", "coef")), key=str)
    print(f"\nlevel 8, {what}, adds: " + ", ".join(f"{' '.join(str(v) for v in c)} ({eight[c]})" for c in added))


def test_level_8_mono(gpu_ctx):
    got, prof = _encode(gpu_ctx, C.mono_band("uint16"), C.TILE, level=8)
    ref = C.tiles_reference("mono", "uint16", C.TILE, 8)
    names = _mono_names()
    _print_added(C.cells_of(C.census_of_tiles(C.tiles_reference("mono", "uint16"), 4 * C.FRAME, names)),
                 C.cells_of(C.census_of_tiles(ref, 4 * C.FRAME, names)), "mono")
    assert prof["compact"] >= 0, prof
    _check_tiles(got, ref, 4 * C.FRAME, names, "level 8 mono")


def test_level_8_two_bands(gpu_ctx):
    got, prof = _encode(gpu_ctx, C.stereo_raster("uint16"), level=8)
    ref = C.stream_reference(2, "uint16", 8)
    five = C.stream_reference(2)
    names = _stereo_names()
    _print_added(C.cells_of(C.census_of_stream(five[0], 2, len(five[1]), names)),
                 C.cells_of(C.census_of_stream(ref[0], 2, len(ref[1]), names)), "two bands")
    assert prof["compact"] >= 0, prof
    _check_stream(got, ref, 2, names, "level 8 two bands")


# ---------------------------------------------------------------------------------------------------- decoders
@pytest.mark.parametrize("kind", list(DECODERS))
def test_decoders_read_the_mono_corpus(kind, monkeypatch):
    """The oracle's streams of the four-frame tiles and of the 96 x 96 tiles (short last frames), one call each"""
    ctx = _decoder_ctx(kind, monkeypatch)
    try:
        for what, per in (("mono", 4 * C.FRAME), ("partial", C.PTILE ** 2)):
            data, off, mn, mx = C.tiles_reference(what, "uint16", C.TILE if what == "mono" else C.PTILE)
            counts = [per] * (len(off) - 1)
            want = np.concatenate([O.decode_frames(data[off[t]:off[t + 1]], 1, 16, per) for t in range(len(counts))])
            got = ctx.decode_frames_host(np.frombuffer(data, dtype=np.uint8), off, counts, channels=1, bps=16)
            bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            assert bad.size == 0, (kind, what, bad.size, "first at sample", int(bad[0]))
    finally:
        ctx.close()


@pytest.mark.parametrize("bands", [2, -3])
@pytest.mark.parametrize("kind", ["lane", "wave"])
def test_decoders_read_the_multi_band_corpus(kind, bands, monkeypatch):
    """Two bands (every assignment, the sides of the host test) and three bands holding the whole corpus each"""
    frames, pcm, mn, mx = C.stream_reference(bands)
    ch = abs(bands)
    want = O.decode_frames(frames, ch, 16, len(pcm))
    assert np.array_equal(want, pcm)
    ctx = _decoder_ctx(kind, monkeypatch)
    try:
        got = ctx.decode_frames_host(np.frombuffer(frames, dtype=np.uint8), [0, len(frames)], [len(pcm)], channels=ch,
                                     bps=16).reshape(-1, ch)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, (kind, ch, bad.size, "frames", np.unique(bad // C.FRAME).tolist()[:20])
    finally:
        ctx.close()
