"""Tile placement on the GPU (csrc/frs_place.hip): frs_place_tiles_device against a numpy restatement, the window
decode against the per-tile decode placed by numpy, the mosaic against the host loop it replaces, the multi-band
convert against decode + transpose, and the commands built on them."""
import ctypes
import os

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, container, geotiff, streaming
from flac_raster_amd.cli import app
from flac_raster_amd.converter import RasterFLACConverter

pytestmark = pytest.mark.gpu
runner = CliRunner()

ALL_DTYPES = [np.uint8, np.uint16, np.int16, np.int32, np.uint32, np.float32, np.float64]


# ------------------------------------------------------------------------------------------------ placement alone
def _sentinel(dtype):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(np.dtype(dtype))[0]


def _distinct(n, dtype):
    """np.arange-style distinct values (they wrap for the 8/16-bit types, never in step with a row or a tile)."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (np.arange(n, dtype=np.float64) * 0.5 + 1.0).astype(dt)
    return (np.arange(n, dtype=np.uint64) * 7 + 3).astype(dt)


def _place(ctx, dtype, C, H, W, wins, row_stride=None, band_stride=None, lead=0, pcm_gap=0):
    """Run frs_place_tiles_device on distinct tile contents and a sentinel-filled destination whose origin lies `lead`
    elements into its buffer.  Returns (got, want): the whole destination buffer and its numpy restatement."""
    dt = np.dtype(dtype)
    rs = W if row_stride is None else row_stride
    bs = rs * H if band_stride is None else band_stride
    ext = lead + (C - 1) * bs + (H - 1) * rs + W
    poff, p = [], pcm_gap
    for (_, _, w, h) in wins:
        poff.append(p)
        p += w * h + pcm_gap
    src = _distinct(max(p, 1) * C, dt)
    want = np.full(ext, _sentinel(dt), dtype=dt)
    view = np.lib.stride_tricks.as_strided(want[lead:], shape=(C, H, W), strides=(bs * dt.itemsize, rs * dt.itemsize,
                                                                                    dt.itemsize))
    for (c0, r0, w, h), po in zip(wins, poff):
        tile = src[po * C:(po + w * h) * C].reshape(h, w, C)
        ys, ye, xs, xe = max(0, -r0), min(h, H - r0), max(0, -c0), min(w, W - c0)
        if ys < ye and xs < xe:
            for c in range(C):
                view[c, r0 + ys:r0 + ye, c0 + xs:c0 + xe] = tile[ys:ye, xs:xe, c]
    tb, db = ctx.alloc(src.nbytes), ctx.alloc(ext * dt.itemsize)
    try:
        tb.upload(src)
        db.upload(np.full(ext, _sentinel(dt), dtype=dt))
        d = ctx.make_raster_desc(H, W, dt, nbands=C, row_stride=rs, band_stride=bs)
        ctx.place_tiles_device(tb.ptr, poff, wins, d, db.ptr + lead * dt.itemsize)
        got = np.empty(ext, dtype=dt)
        db.download(out=got)
    finally:
        tb.close()
        db.close()
    return got, want


def _grid(w, h, co=3, ro=1):
    """2 x 2 tiles of w x h from (co, ro), the right column 5 px narrower and the bottom row 1 px lower (so the
    per-tile sample counts differ), in a destination that is odd in elements and 4 px wider and 2 px higher."""
    w2, h2 = max(1, w - 5), h + 1
    wins = [(co, ro, w, h), (co + w, ro, w2, h), (co, ro + h, w, h2), (co + w, ro + h, w2, h2)]
    W = co + w + w2 + 4
    W += 1 - W % 2
    return wins, ro + h + h2 + 2, W


def _check(ctx, dtype, C, w, h, co=3, pad=3, slack=5):
    wins, H, W = _grid(w, h, co)
    rs = W + pad
    got, want = _place(ctx, dtype, C, H, W, wins, row_stride=rs, band_stride=rs * H + slack)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_place_every_dtype(gpu_ctx, dtype):
    _check(gpu_ctx, dtype, 1, 100, 3)
    _check(gpu_ctx, dtype, 3, 100, 3)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8])
def test_place_channels(gpu_ctx, C):
    _check(gpu_ctx, np.int16, C, 100, 3)


@pytest.mark.parametrize("w", [1, 7, 64, 100, 512])
@pytest.mark.parametrize("C", [1, 3])
def test_place_tile_widths(gpu_ctx, w, C):
    _check(gpu_ctx, np.int16, C, w, 3)


@pytest.mark.parametrize("h", [1, 3, 512])
@pytest.mark.parametrize("C", [1, 3])
def test_place_tile_heights(gpu_ctx, h, C):
    _check(gpu_ctx, np.int16, C, 100, h)  # h = 512: several row blocks per tile


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("slack", [0, 5, 8])
def test_place_strides(gpu_ctx, pad, slack):
    """row_stride = width and width + 3 (the padding keeps the sentinel); band planes dense and with slack, which puts
    the planes after the first at other offsets from a 16-byte boundary."""
    _check(gpu_ctx, np.int16, 1, 100, 3, pad=pad, slack=slack)
    _check(gpu_ctx, np.int16, 3, 100, 3, pad=pad, slack=slack)


@pytest.mark.parametrize("co", [0, 1, 3, 8])
@pytest.mark.parametrize("dtype,C", [(np.int16, 1), (np.uint8, 1), (np.int16, 4)])
def test_place_column_offsets(gpu_ctx, co, dtype, C):
    _check(gpu_ctx, dtype, C, 100, 3, co=co)


@pytest.mark.parametrize("dtype,C,w", [(np.float64, 4, 512), (np.float64, 5, 512), (np.uint8, 3, 512), (np.int32, 2, 7)])
def test_place_rows_wider_than_a_work_group(gpu_ctx, dtype, C, w):
    """512 px x 8 bytes x 4 channels is one 16 KiB row per work-group; x 5 channels is more than one work-group's share."""
    _check(gpu_ctx, dtype, C, w, 3)


@pytest.mark.parametrize("lead", [0, 1, 5])
def test_place_destination_origin_off_a_16_byte_boundary(gpu_ctx, lead):
    wins, H, W = _grid(100, 3)
    got, want = _place(gpu_ctx, np.int16, 1, H, W, wins, lead=lead, pcm_gap=3)
    assert np.array_equal(got, want)
    got, want = _place(gpu_ctx, np.uint8, 2, H, W, wins, lead=lead, pcm_gap=1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype,C", [(np.int16, 1), (np.int16, 3), (np.uint8, 1), (np.float32, 5)])
def test_place_clips_tiles_to_the_destination(gpu_ctx, dtype, C):
    """A 3 x 3 set of 60 x 50 tiles from (-25, -20) over a 120 x 100 destination: the outer eight overhang all four
    edges and corners, the centre tile lies wholly inside; one more tile lies wholly outside."""
    wins = [(-25 + 60 * i, -20 + 50 * j, 60, 50) for j in range(3) for i in range(3)] + [(500, 10, 60, 50)]
    got, want = _place(gpu_ctx, dtype, C, 100, 120, wins, row_stride=123, band_stride=123 * 100 + 1)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # only tiles that lie outside: nothing is written
    far = [(-60, 0, 60, 50), (0, 100, 60, 50), (120, -50, 60, 50), (1 << 40, -(1 << 40), 60, 50)]
    got, want = _place(gpu_ctx, dtype, C, 100, 120, far)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and np.all(got == _sentinel(dtype))


def test_place_no_tiles_and_any_tile_order(gpu_ctx):
    got, want = _place(gpu_ctx, np.int16, 2, 9, 33, [])
    assert np.array_equal(got, want) and np.all(got == _sentinel(np.int16))
    wins, H, W = _grid(100, 3)
    for order in ([3, 0, 2, 1], [1, 3, 0, 2]):
        got, want = _place(gpu_ctx, np.int16, 1, H, W, [wins[i] for i in order])
        assert np.array_equal(got, want)


def test_place_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    tb, db = ctx.alloc(4096), ctx.alloc(4096)
    poff = np.zeros(2, dtype=np.int64)
    pp = poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def call(desc, wins, n=None, tiles=None, dst=None):
        arr = _native.tile_window_array(wins)
        return ctx.lib.frs_place_tiles_device(ctx.handle, ctypes.byref(desc), ctypes.c_void_p(tiles or tb.ptr), pp, arr,
                                              len(wins) if n is None else n, ctypes.c_void_p(dst or db.ptr))

    good = lambda **kw: ctx.make_raster_desc(8, 16, np.int16, **kw)  # noqa: E731
    one = [(0, 0, 4, 4)]
    try:
        assert call(good(), one) == 0
        assert call(good(), [], n=0) == 0
        assert call(good(), one, n=-1) == -1
        assert call(good(), [(0, 0, 0, 4)]) == -1 and call(good(), [(0, 0, 4, 0)]) == -1
        assert call(good(), [(0, 0, 4, 4), (4, 0, -1, 4)]) == -1
        assert call(ctx.make_raster_desc(0, 16, np.int16), one) == -1
        assert call(ctx.make_raster_desc(8, 0, np.int16), one) == -1
        assert call(good(row_stride=15), one) == -1
        for nb in (0, 9, -1):
            d = good()
            d.nbands = nb
            assert call(d, one) == -1
        for code in (0, 8, -3):
            d = good()
            d.dtype = code
            assert call(d, one) == -1
        assert call(good(), one, dst=db.ptr + 1) == -1 and call(good(), one, tiles=tb.ptr + 1) == -1
        assert "FRS_E_ARG" in _native.STATUS[-1]
        with pytest.raises(_native.FrsError):
            ctx.place_tiles_device(tb.ptr, [0], [(0, 0, 0, 4)], good(), db.ptr)
    finally:
        tb.close()
        db.close()


# ------------------------------------------------------------------------------------------------ decode into a window
def gpu_device() -> int:
    return int(os.environ.get("FRS_DEVICE", "0"))


@pytest.fixture(scope="module")
def streamed(gpu_ctx, golden, tmp_path_factory):
    """sample_dem at tile 200 and sample_rgb (band 1) at tile 100 as streaming files, with their source bands."""
    d = tmp_path_factory.mktemp("place")
    out = {}
    for name, tile in (("sample_dem", 200), ("sample_rgb", 100)):
        f = d / f"{name}.flac"
        streaming.create_streaming(golden / f"{name}.tif", f, tile, ctx=gpu_ctx)
        r = geotiff.read(golden / f"{name}.tif")
        r.data.setflags(write=False)
        out[name] = (f, r)
    return out


def _placed_by_numpy(ctx, path):
    """The per-tile decode (TileDecoder.decode_streams) placed into the full raster by numpy."""
    n, index = streaming.read_index(path)
    dec = streaming.TileDecoder(ctx).decode_streams(streaming.fetch_tiles(path, index["frames"], n))
    out = np.zeros((1, index["height"], index["width"]), dtype=dec[0][0].dtype)
    for f, (arr, _) in zip(index["frames"], dec):
        w = f["window"]
        out[0, w["row_off"]:w["row_off"] + w["height"], w["col_off"]:w["col_off"] + w["width"]] = arr[0]
    return out


@pytest.mark.parametrize("name", ["sample_dem", "sample_rgb"])
def test_reconstruct_equals_the_source_band(gpu_ctx, streamed, name):
    path, r = streamed[name]
    arr, tr = streaming.reconstruct(path, ctx=gpu_ctx)
    assert arr.shape == (1, r.height, r.width) and arr.dtype == r.data.dtype
    assert np.array_equal(arr[0], r.data[0])
    assert np.array_equal(arr, _placed_by_numpy(gpu_ctx, path))
    assert list(tr)[:6] == list(r.transform)[:6]


@pytest.mark.parametrize("lane", ["0", "1"])
def test_reconstruct_through_either_mono_decoder(streamed, monkeypatch, lane):
    monkeypatch.setenv("FRS_DECODE_LANE", lane)
    with _native.Context(gpu_device()) as ctx:
        for name in ("sample_dem", "sample_rgb"):
            path, r = streamed[name]
            arr, _ = streaming.reconstruct(path, ctx=ctx)
            assert np.array_equal(arr[0], r.data[0]), (name, lane)


def test_window_host_call_keeps_what_no_tile_covers(gpu_ctx, streamed):
    """frs_decode_tiles_window (host pointers): two of the tiles, decoded into a sentinel-filled window that starts
    inside the first; the rest of the window comes back untouched."""
    path, r = streamed["sample_dem"]
    n, index = streaming.read_index(path)
    frames = [index["frames"][0], index["frames"][4]]
    datas = streaming.fetch_tiles(path, frames, n)
    metas = [container.parse_metadata(s) for s in datas]
    mds = [container.read_raster_tags(m) for m in metas]
    blob = np.concatenate([np.frombuffer(s, dtype=np.uint8)[m.audio_offset:] for s, m in zip(datas, metas)])
    soff = np.cumsum([0] + [len(s) - m.audio_offset for s, m in zip(datas, metas)])
    c0, r0, h, w = 37, 11, 300, 333
    out = np.full((1, h, w), 12345, dtype=r.data.dtype)
    got = gpu_ctx.decode_tiles_window_host(blob, soff, streaming.tile_windows(frames, (c0, r0)), metas[0].bps,
                                           [m["data_min"] for m in mds], [m["data_max"] for m in mds], r.data.dtype,
                                           out=out)
    assert got is out
    want = np.full((1, h, w), 12345, dtype=r.data.dtype)
    for f in frames:
        k = f["window"]
        ya, yb = max(k["row_off"], r0), min(k["row_off"] + k["height"], r0 + h)
        xa, xb = max(k["col_off"], c0), min(k["col_off"] + k["width"], c0 + w)
        want[0, ya - r0:yb - r0, xa - c0:xb - c0] = r.data[0, ya:yb, xa:xb]
    assert np.array_equal(out, want)


# ------------------------------------------------------------------------------------------------ mosaic
def _host_loop_mosaic(ctx, path, bbox, crop):
    """streaming.extract_bbox_mosaic as it was before the placement kernel: zeros, place tile by tile, crop."""
    n, index = streaming.read_index(path)
    hits = streaming.intersecting(index, bbox)
    dec = streaming.TileDecoder(ctx).decode_streams(streaming.fetch_tiles(path, hits, n))
    c0 = min(f["window"]["col_off"] for f in hits)
    r0 = min(f["window"]["row_off"] for f in hits)
    c1 = max(f["window"]["col_off"] + f["window"]["width"] for f in hits)
    r1 = max(f["window"]["row_off"] + f["window"]["height"] for f in hits)
    out = np.zeros((1, r1 - r0, c1 - c0), dtype=dec[0][0].dtype)
    for f, (arr, _) in zip(hits, dec):
        w = f["window"]
        out[0, w["row_off"] - r0:w["row_off"] - r0 + w["height"], w["col_off"] - c0:w["col_off"] - c0 + w["width"]] = arr[0]
    t = geotiff.Affine(*index["transform"][:6])
    win = {"col_off": c0, "row_off": r0, "width": c1 - c0, "height": r1 - r0}
    if crop and t.b == 0 and t.d == 0:
        cw = streaming.bbox_pixel_window(t, bbox, int(index["width"]), int(index["height"]))
        a0, b0 = max(cw["col_off"], c0), max(cw["row_off"], r0)
        a1 = min(cw["col_off"] + cw["width"], c1)
        b1 = min(cw["row_off"] + cw["height"], r1)
        out = np.ascontiguousarray(out[:, b0 - r0:max(b1, b0) - r0, a0 - c0:max(a1, a0) - c0])
        win = {"col_off": a0, "row_off": b0, "width": max(a1 - a0, 0), "height": max(b1 - b0, 0)}
    return out, win, list(geotiff.window_transform(t, win["col_off"], win["row_off"]))


# pixel boxes (col0, row0, col1, row1) of the tile-200 sample_dem file, None for the raster's own bounds
MOSAIC_BOXES = {
    "inside_one_tile": (20.3, 30.2, 150.7, 120.6),
    "four_tiles_off_grid": (150.5, 180.3, 260.25, 230.8),
    "full_extent": None,
    "over_the_upper_left_edge": (-50.0, -30.5, 100.5, 250.4),
    "over_the_lower_right_edge": (-30.5, -40.25, 45.0, 60.0),  # measured from the raster's lower right corner
}


@pytest.mark.parametrize("crop", [True, False])
@pytest.mark.parametrize("box", list(MOSAIC_BOXES))
def test_mosaic_equals_the_host_loop(gpu_ctx, streamed, box, crop):
    path, r = streamed["sample_dem"]
    t = r.transform
    px = MOSAIC_BOXES[box]
    if px is None:
        px = (0, 0, r.width, r.height)
    elif box == "over_the_lower_right_edge":
        px = (r.width + px[0], r.height + px[1], r.width + px[2], r.height + px[3])
    xs, ys = (t.c + t.a * px[0], t.c + t.a * px[2]), (t.f + t.e * px[1], t.f + t.e * px[3])
    bbox = [min(xs), min(ys), max(xs), max(ys)]
    arr, win, tr = streaming.extract_bbox_mosaic(path, bbox, ctx=gpu_ctx, crop=crop)
    ref, rwin, rtr = _host_loop_mosaic(gpu_ctx, path, bbox, crop)
    assert win == rwin and tr == rtr
    assert arr.dtype == ref.dtype and arr.shape == ref.shape and np.array_equal(arr, ref)
    assert arr.flags.c_contiguous
    assert np.array_equal(arr[0], r.data[0, win["row_off"]:win["row_off"] + win["height"],
                                          win["col_off"]:win["col_off"] + win["width"]])


# ------------------------------------------------------------------------------------------------ multi-band convert
def test_convert_sample_rgb_flac_still_equals_the_fixture(gpu_ctx, golden, tmp_path):
    src = tmp_path / "sample_rgb.flac"
    src.write_bytes((golden / "sample_rgb.flac").read_bytes())
    src.with_suffix(".json").write_text((golden / "sample_rgb.json").read_text())
    out = tmp_path / "rec.tif"
    RasterFLACConverter(gpu_ctx).flac_to_tiff(src, out)
    assert np.array_equal(geotiff.read(out).data, geotiff.read(golden / "sample_rgb_reconstructed.tif").data)


@pytest.mark.parametrize("bands", [4, 2])
def test_multiband_decode_equals_decode_plus_transpose(gpu_ctx, bands):
    """256 x 300: the width is no multiple of 64 and the last frame is partial (76800 samples, blocksize 4096)."""
    H, W = 256, 300
    y, x = np.mgrid[0:H, 0:W]
    data = np.stack([(1000 + 300 * np.sin(x * (0.05 + 0.03 * b)) * np.cos(y * 0.03) + 7 * ((x * 31 + y * 17 + b) % 13))
                     .astype(np.int16) for b in range(bands)])
    conv = RasterFLACConverter(gpu_ctx)
    frames, dmin, dmax, sbps, sr = conv.encode_array(data)
    md = {"width": W, "height": H, "count": bands, "dtype": "int16", "data_min": dmin, "data_max": dmax}
    got, _ = conv.decode_bytes(container.bare_header(bands, sbps, sr) + frames, metadata=md)
    flat = gpu_ctx.decode_tiles_host(np.frombuffer(frames, dtype=np.uint8), [0, len(frames)], [H * W], channels=bands,
                                     bps=sbps, data_min=[dmin], data_max=[dmax], dtype=np.int16)
    want = np.ascontiguousarray(flat.reshape(H, W, bands).transpose(2, 0, 1))
    assert got.shape == (bands, H, W) and got.dtype == np.int16 and got.flags.c_contiguous
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ commands
def test_cli_create_streaming_verify(golden, tmp_path):
    out = tmp_path / "dem_streaming.flac"
    r = runner.invoke(app, ["create-streaming", str(golden / "sample_dem.tif"), "-o", str(out), "--tile-size", "200",
                            "--verify"])
    assert r.exit_code == 0, r.output
    assert "VERIFY: lossless" in r.output and out.exists()
    # float32 samples go through a 24-bit quantisation and back as they are: not lossless
    tif = tmp_path / "f32.tif"
    geotiff.write(tif, np.random.default_rng(1).random((1, 64, 64), dtype=np.float32))
    r = runner.invoke(app, ["create-streaming", str(tif), "-o", str(tmp_path / "f32.flac"), "--tile-size", "48",
                            "--verify"])
    assert r.exit_code == 3, r.output
    assert "VERIFY: differs (n_different=" in r.output and (tmp_path / "f32.flac").exists()


def test_cli_extract_streaming_all(streamed, tmp_path):
    path, r = streamed["sample_dem"]
    out = tmp_path / "all.tif"
    res = runner.invoke(app, ["extract-streaming", str(path), "--all", "-o", str(out)])
    assert res.exit_code == 0, res.output
    got = geotiff.read(out)
    assert got.data.shape == (1, r.height, r.width) and np.array_equal(got.data[0], r.data[0])
    assert got.transform.to_tuple() == r.transform.to_tuple() and got.epsg == r.epsg
