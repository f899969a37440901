"""Tiny tiles and tail frames (1..576 samples) on every codec path of the GPU.

The inputs are tests/tiny_frames.py's: rasters whose tiles are streams of one n-sample frame ("single") or of a full
frame and an n-sample tail ("tail"), for every n of LENGTHS; tests/test_tiny_frames_host.py holds, with the oracle
alone, that they contain the frames meant (VERBATIM up to 4 samples, CONSTANT from 5, FIXED with partitions, LPC, every
block-size code form, every channel assignment).  Encodes are compared byte for byte with the oracle's stream of each
tile, with tile offsets, min / max and the stream's sample size; decodes of the ORACLE's streams with the samples that
went in.  Every assertion is exact equality.  A test collects the cases that differ and names them all.
"""
import json
import struct

import numpy as np
import pytest

from flac_raster_amd import geotiff, streaming
from oracle import oracle as O
from oracle import pipeline as P
from tests import tiny_frames as TF
from tests.pyramid_ref import np_pyramid
from tests.test_gpu_decode import DECODERS, _decoder_ctx
from tests.test_normalize_host import _numpy_normalize

pytestmark = pytest.mark.gpu

PROFILE = ("stats", "partial", "assemble", "compact")
SWITCHES = ("FRS_FORCE_GENERIC", "FRS_DECODE_LANE", "FRS_PIPE_OPT", "FRS_SPAN_READ", "FRS_ANA_PF")


def _ctx(monkeypatch, **env):
    """a context of its own, created under the given switches (as tests/test_gpu_decode_routes.py's)"""
    from flac_raster_amd import _native
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _native.Context(0)


def _encode(ctx, arr, bits=16, level=5, norm_mode=0):
    """arr ([bands,] 8, W) at tile (1, W): one stream per row -> (encode_tiles_host's tuple, profile entries)"""
    bands = arr.shape[0] if arr.ndim == 3 else 1
    W = arr.shape[-1]
    d = ctx.make_desc(8, W, arr.dtype, nbands=bands, tile_h=1, tile_w=W, sample_rate=TF.RATE, bits_per_sample=bits,
                      compression_level=level, norm_mode=norm_mode)
    ctx.profile(True)
    ctx.profile_reset()
    out = ctx.encode_tiles_host(arr, d)
    prof = {k: ctx.profile_avg_ms(k) for k in PROFILE}
    ctx.profile(False)
    return out, prof


def _differences(got, ref, what):
    """the tiles of one encode that differ from their reference, as text"""
    arena, off, mn, mx, bps = got
    bad = []
    data = arena.tobytes()
    if len(off) != 9 or int(off[0]) != 0 or int(off[-1]) != len(data):
        bad.append(f"{what}: tile_off {list(off)} over {len(data)} bytes")
        return bad
    pos = 0
    for r, (pcm, omn, omx, obps, fr) in enumerate(ref):
        frames = data[int(off[r]):int(off[r + 1])]
        if int(off[r]) != pos:
            bad.append(f"{what} tile {r}: offset {int(off[r])} != {pos}")
        if frames != fr:
            bad.append(f"{what} tile {r}: {frames[:24].hex()} ({len(frames)} B) != {fr[:24].hex()} ({len(fr)} B)")
        if bps != obps:
            bad.append(f"{what}: stream_bps {bps} != {obps}")
        if omn is not None and (mn[r] != omn or mx[r] != omx):
            bad.append(f"{what} tile {r}: min / max {mn[r]}, {mx[r]} != {omn}, {omx}")
        pos += len(fr)
    return bad


# name -> (bands, dtype, bits_per_sample, level, spatial, route)
PATHS = {
    "mono_i16": (1, np.int16, 16, 5, False, "fast"),
    "mono_u16": (1, np.uint16, 16, 5, False, "fast"),
    "mono_u8": (1, np.uint8, 16, 5, False, "fast"),
    "mono_i16_forced_generic": (1, np.int16, 16, 5, False, "forced"),
    "three_bands_i16": (3, np.int16, 16, 5, False, "multi"),
    "two_bands_i16": (2, np.int16, 16, 5, False, "multi"),
    "mono_i32_24bit": (1, np.int32, 24, 5, False, "generic"),
    "spatial_one_band": (1, np.int16, 16, 5, True, "generic"),
    "spatial_two_bands": (2, np.int16, 16, 5, True, "generic"),
    "spatial_three_bands": (3, np.int16, 16, 5, True, "generic"),   # (k_zero_frames_emit with three subframes)
    "mono_i16_level0": (1, np.int16, 16, 0, False, "generic"),
    "mono_i16_level3": (1, np.int16, 16, 3, False, "generic"),
    "mono_i16_level6": (1, np.int16, 16, 6, False, "generic"),
    "mono_i16_level8": (1, np.int16, 16, 8, False, "generic"),
    "two_bands_i16_level1": (2, np.int16, 16, 1, False, "generic"),
}


def _route_ok(route, prof, dtype, W):
    """the profile names of the route, asserted the way the older tests do"""
    if route == "fast":
        # 16-bit rows that are 16-byte runs: the statistics are fused into the analysis; else the stats kernels run
        fused = np.dtype(dtype).itemsize == 2 and W % 8 == 0
        return prof["partial"] > 0 and prof["compact"] < 0 and (prof["stats"] <= 0) == fused
    if route == "multi":
        return prof["partial"] > 0 and prof["assemble"] > 0 and prof["compact"] < 0
    return prof["compact"] >= 0


@pytest.mark.parametrize("form", TF.FORMS)
@pytest.mark.parametrize("path", list(PATHS))
def test_encode_matches_oracle_at_every_length(gpu_ctx, monkeypatch, path, form):
    bands, dtype, bits, level, spatial, route = PATHS[path]
    ctx = _ctx(monkeypatch, FRS_FORCE_GENERIC="1") if route == "forced" else gpu_ctx
    bad = []
    try:
        for n in TF.LENGTHS:
            arr = TF.spatial_raster(bands, form, n) if spatial else TF.raster_of(bands, form, n, dtype)
            got, prof = _encode(ctx, arr, bits, level, 1 if spatial else 0)
            if not _route_ok(route, prof, dtype, arr.shape[-1]):
                bad.append(f"n {n}: route {prof}")
            bad += _differences(got, TF.reference(bands, form, n, dtype, level, spatial), f"n {n}")
    finally:
        if ctx is not gpu_ctx:
            ctx.close()
    assert not bad, f"{path} {form}: {len(bad)} differences\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("form", TF.FORMS)
def test_encoded_samples_are_numpys(gpu_ctx, form):
    """Not through the oracle's encoder or normalisation: the GPU's bytes of the int16 mono fast path, decoded by the
    oracle, are numpy's expression of each tile (assertion 1 of tests/test_gpu_normalize_ramps.py)."""
    bad = []
    for n in TF.LENGTHS:
        arr = TF.raster(form, n, np.int16)
        (arena, off, _, _, _), _ = _encode(gpu_ctx, arr)
        data = arena.tobytes()
        for r in range(8):
            pcm = O.decode_frames(data[int(off[r]):int(off[r + 1])], 1, 16, arr.shape[1])
            if not np.array_equal(pcm[:, 0], _numpy_normalize(np.ascontiguousarray(arr[r]))):
                bad.append((n, r))
    assert not bad, bad


def test_wasted_bits_in_the_side_of_a_three_sample_frame(gpu_ctx):
    """All four signals VERBATIM, and the side's two wasted bits make left-side the cheapest pair."""
    arr = TF.wasted_side_pair()
    got, prof = _encode(gpu_ctx, arr)
    ref = []
    for r in range(8):
        pcm, mn, mx, bps = O.normalize(TF.tile_samples(arr, r))
        ref.append((pcm, mn, mx, bps, O.encode_frames(pcm, bps, TF.RATE)))
    assert TF.header_fields(ref[4][4])[1] == 8
    bad = _differences(got, ref, "n 3")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("form", TF.FORMS)
@pytest.mark.parametrize("path", ["mono_i16", "mono_i16_forced_generic", "three_bands_i16", "two_bands_i16"])
def test_table_block_size_codes_on_short_frames(gpu_ctx, monkeypatch, path, form):
    """Frames of 512, 1024, 1152, 2048 and 2304 samples, alone and as tails: the header names the length by a table
    code, like LENGTHS' 192, 256 and 576 (tests/test_tiny_frames_host.py holds the nibbles)."""
    bands, dtype, bits, level, spatial, route = PATHS[path]
    ctx = _ctx(monkeypatch, FRS_FORCE_GENERIC="1") if route == "forced" else gpu_ctx
    bad = []
    try:
        for n in TF.TABLE_LENGTHS:
            arr = TF.raster_of(bands, form, n, dtype)
            got, prof = _encode(ctx, arr, bits, level)
            if not _route_ok(route, prof, dtype, arr.shape[-1]):
                bad.append(f"n {n}: route {prof}")
            bad += _differences(got, TF.reference(bands, form, n, dtype, level), f"n {n}")
    finally:
        if ctx is not gpu_ctx:
            ctx.close()
    assert not bad, f"{path} {form}: {len(bad)} differences\n" + "\n".join(bad[:40])


# ------------------------------------------------------------------------------------- two-dimensional edge tiles
@pytest.mark.parametrize("name", list(TF.GRIDS))
def test_edge_tiles_of_a_grid_match_oracle(gpu_ctx, name):
    """131 x 67 at tile 65: tiles of 65 x 65 (a full frame and 129 samples), 1 x 65, 65 x 2 and 1 x 2; 513 x 513 at
    tile 512: 64 full frames, a 512-sample frame (a table block-size code) twice, and the 12-byte 1 x 1 stream.  The
    second encode on the same context takes the cached geometry."""
    H, W, T = TF.GRIDS[name]
    band = TF.grid_band(name)
    o_arena, o_off, o_mn, o_mx = TF.grid_reference(name)
    for again in (False, True):
        d = gpu_ctx.make_desc(H, W, band.dtype, tile_h=T, tile_w=T, sample_rate=TF.RATE, bits_per_sample=16)
        gpu_ctx.profile(True)
        gpu_ctx.profile_reset()
        arena, off, mn, mx, bps = gpu_ctx.encode_tiles_host(band, d)
        prof = {k: gpu_ctx.profile_avg_ms(k) for k in PROFILE}
        gpu_ctx.profile(False)
        assert prof["partial"] > 0 and prof["compact"] < 0, (again, prof)
        assert bps == 16 and list(off) == list(o_off), again
        for t in range(len(o_mn)):
            assert arena[off[t]:off[t + 1]].tobytes() == o_arena[o_off[t]:o_off[t + 1]].tobytes(), (again, t)
        assert arena.tobytes() == o_arena.tobytes(), again
        assert list(mn) == list(o_mn) and list(mx) == list(o_mx), again


# ------------------------------------------------------------------------------------------------------- decode
# the stages a decode runs, by profile name (tests/test_gpu_decode_routes.py), per decoder kind: (all of, none of).
# Mono streams take all four kinds; two and three bands the lane walk ("lane": 64 frames or more in the call) or the
# one-lane wave decoder.
DECODE_STAGES = ("decode_span", "decode_frames", "decode_fallback", "lane_fallback_frames")
ROUTES = {"pipe": ({"decode_frames"}, {"decode_span", "decode_fallback", "lane_fallback_frames"}),
          "pipe_chain": ({"decode_span", "decode_frames"}, {"decode_fallback", "lane_fallback_frames"}),
          "lane": ({"decode_span", "lane_fallback_frames"}, {"decode_fallback"}),
          "wave": ({"decode_span", "decode_frames"}, {"decode_fallback", "lane_fallback_frames"})}


def _batch(bands, order, forms=("single",), dtype=np.int16):
    """The oracle's streams of every length in `order`, eight per length and form: (blob, stream offsets, sample
    counts, [pcm], mins, maxs, [the tile's source samples where the reference's round trip returns them, else None],
    dtype)"""
    streams, counts, pcms, mins, maxs, sources = [], [], [], [], [], []
    for n in order:
        for form in forms:
            keep = TF.lossless_tiles(form, n, dtype) if bands == 1 else ()
            arr = TF.raster_of(bands, form, n, dtype)
            for r, (pcm, mn, mx, bps, fr) in enumerate(TF.reference(bands, form, n, dtype)):
                assert bps == 16
                streams.append(fr)
                counts.append(len(pcm))
                pcms.append(pcm)
                mins.append(mn)
                maxs.append(mx)
                sources.append(TF.tile_samples(arr, r) if r in keep else None)
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    return np.frombuffer(b"".join(streams), dtype=np.uint8), off, counts, pcms, mins, maxs, sources, np.dtype(dtype)


def _check_decodes(ctx, kind, bands, batch, what):
    blob, off, counts, pcms, mins, maxs, sources, dtype = batch
    want = np.concatenate(pcms)
    ctx.profile(True)
    ctx.profile_reset()
    got = ctx.decode_frames_host(blob, off, counts, channels=bands, bps=16).reshape(-1, bands)
    ran = {k for k in DECODE_STAGES if ctx.profile_avg_ms(k) >= 0}
    ctx.profile(False)
    assert ROUTES[kind][0] <= ran and not ROUTES[kind][1] & ran, (kind, what, ran)
    ends = np.cumsum(counts)
    bad = [(what, "pcm", s, counts[s]) for s in range(len(counts))
           if not np.array_equal(got[ends[s] - counts[s]:ends[s]], pcms[s])]
    assert not bad and np.array_equal(got, want), bad[:20]
    # the fused de-normalisation against the oracle's two steps, and against the source where those return it
    vals = ctx.decode_tiles_host(blob, off, counts, channels=bands, bps=16, data_min=mins, data_max=maxs,
                                 dtype=dtype).reshape(-1, bands)
    bad = [(what, "values", s, counts[s]) for s in range(len(counts))
           if not np.array_equal(vals[ends[s] - counts[s]:ends[s]], O.denormalize_i16(pcms[s], mins[s], maxs[s], dtype))]
    bad += [(what, "source", s, counts[s]) for s in range(len(counts))
            if sources[s] is not None and not np.array_equal(vals[ends[s] - counts[s]:ends[s]], sources[s])]
    assert not bad, bad[:20]


@pytest.mark.parametrize("kind", list(DECODERS))
def test_decode_batches_of_one_frame_streams(kind, monkeypatch):
    """8 x 29 mono streams of one frame each in one call, ascending (the blob begins with a 12-byte stream of one
    sample) and descending (it ends with the last byte of one); then the two-frame tail streams mixed in; then the
    ascending batches of the uint16 and uint8 rasters (their de-normalisation).  The values are compared with the
    oracle's everywhere and with the source on the tiles the reference's own round trip returns."""
    up = _batch(1, TF.LENGTHS)
    down = _batch(1, TF.LENGTHS[::-1])
    assert up[2][0] == 1 and down[2][-1] == 1 and int(up[1][1]) == 12 and int(down[1][-1] - down[1][-2]) == 12
    assert len(up[2]) == 8 * len(TF.LENGTHS) and sum(s is not None for s in up[6]) > len(up[2]) // 2
    mixed = _batch(1, TF.LENGTHS, ("single", "tail"))
    ctx = _decoder_ctx(kind, monkeypatch)
    try:
        _check_decodes(ctx, kind, 1, up, "ascending")
        _check_decodes(ctx, kind, 1, down, "descending")
        _check_decodes(ctx, kind, 1, mixed, "mixed")
        for dtype in (np.uint16, np.uint8):
            _check_decodes(ctx, kind, 1, _batch(1, TF.LENGTHS, ("single", "tail"), dtype), np.dtype(dtype).name)
    finally:
        ctx.close()


@pytest.mark.parametrize("bands", [2, 3])
@pytest.mark.parametrize("kind", ["lane", "wave"])
def test_decode_batches_of_multi_band_streams(kind, bands, monkeypatch):
    up = _batch(bands, TF.LENGTHS)
    down = _batch(bands, TF.LENGTHS[::-1])
    mixed = _batch(bands, TF.LENGTHS, ("single", "tail"))
    ctx = _decoder_ctx(kind, monkeypatch)
    try:
        _check_decodes(ctx, kind, bands, up, "ascending")
        _check_decodes(ctx, kind, bands, down, "descending")
        _check_decodes(ctx, kind, bands, mixed, "mixed")
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
def test_single_tile_query_of_every_one_frame_stream(gpu_ctx, dtype):
    """frs_decode_tile_device (the bbox query's call) on each stream of the ascending batch in turn, in place in the
    device blob: into page-locked host memory that was poisoned before the call -- the samples are the oracle's and
    the 32 elements after them keep the poison -- and, for the first and the last stream, into device memory."""
    blob_h, off, counts, pcms, mins, maxs, sources, dt = _batch(1, TF.LENGTHS, dtype=dtype)
    poison = dt.type(0x5A)
    cap = max(counts) + 32
    blob = gpu_ctx.alloc(len(blob_h))
    hb = gpu_ctx.host_buffer(cap * dt.itemsize)
    out = gpu_ctx.alloc(cap * dt.itemsize)
    bad = []
    try:
        blob.upload(blob_h)
        host = hb.array.view(dt)
        for s, n in enumerate(counts):
            want = O.denormalize_i16(pcms[s], mins[s], maxs[s], dt).reshape(-1)
            host[:] = poison
            gpu_ctx.decode_tile_device(blob, int(off[s]), int(off[s + 1]), n, 1, 16, mins[s], maxs[s], dt, hb)
            if not np.array_equal(host[:n], want):
                bad.append((s, n, "values"))
            if not (host[n:n + 32] == poison).all():
                bad.append((s, n, "wrote past the tile"))
            if s in (0, len(counts) - 1):
                gpu_ctx.decode_tile_device(blob, int(off[s]), int(off[s + 1]), n, 1, 16, mins[s], maxs[s], dt, out)
                if not np.array_equal(out.download(n * dt.itemsize).view(dt), want):
                    bad.append((s, n, "device output"))
    finally:
        blob.close()
        hb.close()
        out.close()
    assert not bad, bad[:20]


# ---------------------------------------------------------------------------------------------------- placement
def _grid_want(name):
    """the oracle's decode + de-normalise of every tile of the grid, at its window"""
    H, W, _ = TF.GRIDS[name]
    arena, off, mins, maxs = TF.grid_reference(name)
    want = np.zeros((H, W), dtype=np.int16)
    for t, (c, r, w, h) in enumerate(TF.grid_windows(name)):
        pcm = O.decode_frames(arena[off[t]:off[t + 1]].tobytes(), 1, 16, w * h)
        want[r:r + h, c:c + w] = O.denormalize_i16(pcm, mins[t], maxs[t], np.int16).reshape(h, w)
    return want


@pytest.mark.parametrize("name", list(TF.GRIDS))
def test_decode_into_windows_of_a_sentinel_filled_raster(gpu_ctx, name):
    H, W, _ = TF.GRIDS[name]
    arena, off, mins, maxs = TF.grid_reference(name)
    wins = TF.grid_windows(name)
    want = _grid_want(name)
    assert np.array_equal(want, TF.grid_band(name))  # (every tile survives the round trip: the host test holds it)
    sentinel = np.int16(-12345)
    assert not (want == sentinel).any()
    out = np.full((1, H, W), sentinel, dtype=np.int16)
    got = gpu_ctx.decode_tiles_window_host(arena, off, wins, 16, mins, maxs, np.int16, out=out)
    assert got is out and np.array_equal(out[0], want)
    # rows padded to 520 elements (513 x 513 only: the width must fit): the padding keeps the sentinel
    rs = 520 if W <= 520 else W + 7
    blob, dst = gpu_ctx.alloc(len(arena) + 16), gpu_ctx.alloc(H * rs * 2)
    try:
        blob.upload(arena)
        dst.upload(np.full(H * rs, sentinel, dtype=np.int16))
        gpu_ctx.decode_tiles_window_device(blob, off, wins, 16, mins, maxs, np.int16, dst, (1, H, W), row_stride=rs)
        back = dst.download().view(np.int16).reshape(H, rs)
    finally:
        blob.close()
        dst.close()
    assert np.array_equal(back[:, :W], want)
    assert (back[:, W:] == sentinel).all()


# -------------------------------------------------------------------------------------------------------- files
FT = geotiff.Affine(0.25, 0.0, -106.0, 0.0, -0.25, 41.0)   # (exact in binary: bbox edges land on pixel edges)
CRS = "EPSG:4326"
MODES = ["average", "nearest"]


@pytest.fixture(scope="module")
def files(gpu_ctx, tmp_path_factory):
    """mode (None: no overviews) -> path of the 129 x 193 band's streaming file at tile 64.  Written once."""
    d = tmp_path_factory.mktemp("tiny_files")
    out = {None: d / "plain.flac"}
    streaming.create_streaming_array(TF.file_band(), FT, CRS, out[None], TF.FILE_TILE, ctx=gpu_ctx)
    for mode in MODES:
        out[mode] = d / f"{mode}.flac"
        streaming.create_streaming_array(TF.file_band(), FT, CRS, out[mode], TF.FILE_TILE, ctx=gpu_ctx, overviews=True,
                                         resampling=mode)
    return out


def test_file_is_the_oracle_pipelines(files):
    assert files[None].read_bytes() == P.create_streaming(TF.file_band(), list(FT), CRS, TF.FILE_TILE)


@pytest.mark.parametrize("mode", MODES)
def test_file_levels_are_the_oracle_pipelines(files, mode):
    """every overview level's tile section is what create-streaming writes for that level's raster"""
    raw = files[mode].read_bytes()
    n = struct.unpack(">I", raw[:4])[0]
    index, body = json.loads(raw[4:4 + n]), raw[4 + n:]
    plain = files[None].read_bytes()
    pn = struct.unpack(">I", plain[:4])[0]
    assert body[:len(plain) - 4 - pn] == plain[4 + pn:]
    pos = len(plain) - 4 - pn
    pyr = np_pyramid(TF.file_band(), TF.FILE_SHAPES, mode)
    assert [(lv["height"], lv["width"]) for lv in index["overviews"]["levels"]] == TF.FILE_SHAPES
    for k, lv in enumerate(index["overviews"]["levels"], start=1):
        ref = P.create_streaming(pyr[k], streaming.level_transform(list(FT), k), CRS, TF.FILE_TILE)
        rn = struct.unpack(">I", ref[:4])[0]
        ref_body = ref[4 + rn:]
        assert body[pos:pos + len(ref_body)] == ref_body, k
        pos += len(ref_body)
    assert pos == len(body)


def test_file_extract_all_and_verify(gpu_ctx, files, tmp_path):
    out = tmp_path / "all.tif"
    streaming.extract_all(files[None], out, ctx=gpu_ctx)
    assert np.array_equal(geotiff.read(out).data[0], TF.file_band())
    res = streaming.verify_streaming(files[None], TF.file_band(), ctx=gpu_ctx)
    assert res["n_different"] == 0 and res["first_difference"] is None
    for mode in MODES:
        res = streaming.verify_streaming(files[mode], TF.file_band(), ctx=gpu_ctx)
        assert res["levels_checked"] == 3 and res["n_different"] == 0 and res["first_difference"] is None
        assert [x["n_different"] for x in res["levels"]] == [0, 0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_file_reconstruct_every_level(gpu_ctx, files, mode):
    for k, want in enumerate(np_pyramid(TF.file_band(), TF.FILE_SHAPES, mode)):
        arr, tr = streaming.reconstruct(files[mode], ctx=gpu_ctx, level=k)
        assert arr.dtype == want.dtype and np.array_equal(arr[0], want), k


def test_file_reads_of_the_last_column(gpu_ctx, files):
    """A bbox over the last column alone, the 1 x 64 tiles and the 1 x 1 corner.  extract_bbox_mosaic decodes just those
    three tiles (129 samples in one call); read_window adds its one-pixel margin, so the 64-wide neighbours come too,
    and returns the column at its native size."""
    H, W = TF.FILE_H, TF.FILE_W
    column = TF.file_band()[:, W - 1]
    index = streaming.read_index(files[None])[1]
    inside = [FT.c + FT.a * (W - 0.75), FT.f + FT.e * H, FT.c + FT.a * W, FT.f]
    thin = [(1, 64), (1, 64), (1, 1)]
    assert [(f["window"]["width"], f["window"]["height"]) for f in streaming.intersecting(index, inside)] == thin
    arr, win, _ = streaming.extract_bbox_mosaic(files[None], inside, ctx=gpu_ctx)
    assert win == {"col_off": W - 1, "row_off": 0, "width": 1, "height": H}
    assert arr.shape == (1, H, 1) and np.array_equal(arr[0, :, 0], column)
    bbox = [FT.c + FT.a * (W - 1), FT.f + FT.e * H, FT.c + FT.a * W, FT.f]
    req = streaming.window_request(index, bbox, 1, H, 0)
    assert [(f["window"]["width"], f["window"]["height"]) for f in req["frames"]
            if f["window"]["col_off"] == W - 1] == thin
    for mode in ("nearest", "average"):
        arr, _ = streaming.read_window(files[None], bbox, 1, H, resampling=mode, level=0, ctx=gpu_ctx)
        assert arr.shape == (1, H, 1) and np.array_equal(arr[0, :, 0], column), mode
