"""The render through the streaming path, on files: streaming.render_window and the render command against
lut[quantise(read_window(...))].  A 300 x 260 int16 raster whose inner block holds 100..3000, with a 20-pixel -9999
collar and a hole, written in tiles of 64 with overviews, its nodata value and its statistics."""
import os

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, geotiff, render, stats, streaming
from flac_raster_amd.cli import app
from tests import render_ref as RR
from tests.render_cases import read_png

pytestmark = pytest.mark.gpu
runner = CliRunner()

H, W, TILE, ND = 300, 260, 64, -9999
T = geotiff.Affine(0.001, 0.0, -106.0, 0.0, -0.001, 41.0)
CRS = "EPSG:4326"
FULL = [-106.0, 41.0 - H * 0.001, -106.0 + W * 0.001, 41.0]
# the whole raster and a margin around it, the collar's corner at a fractional scale, an inner piece
BOXES = {"all_and_margin": ([-106.01, 40.69, -105.73, 41.01], 50, 60),
         "corner": ([-105.999, 40.9503, -105.9521, 40.9997], 33, 17),
         "inner": ([-105.9, 40.8, -105.8, 40.9], 7, 5)}
NODATA_RGBA = (10, 20, 30, 0)


def _band():
    rng = np.random.default_rng(61)
    a = np.full((H, W), ND, dtype=np.int16)
    a[20:-20, 20:-20] = rng.integers(100, 3000, size=(H - 40, W - 40), endpoint=True)
    a[120:150, 100:130] = ND  # a hole
    return a


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_ctx):
    d = tmp_path_factory.mktemp("render_files")
    band = _band()
    index = streaming.create_streaming_array(band, T, CRS, d / "dem.flac", tile_size=TILE, ctx=gpu_ctx, overviews=True,
                                             nodata=ND, stats=True)
    streaming.create_streaming_array(band, T, CRS, d / "nostats.flac", tile_size=TILE, ctx=gpu_ctx, overviews=True,
                                     nodata=ND)
    assert "statistics" in index and streaming.overview_levels(index) == [0, 1, 2, 3]
    return {"dir": d, "band": band, "path": d / "dem.flac", "nostats": d / "nostats.flac", "index": index}


@pytest.fixture(scope="module")
def prof_ctx():
    """a context of its own with profiling on: its entries say which kernels a call ran"""
    ctx = _native.Context(int(os.environ.get("FRS_DEVICE", "0")))
    ctx.profile(True)
    yield ctx
    ctx.close()


def _expected(path, bbox, w, h, mode, lo, hi, lut, channels, ctx, level=None, nodata="index"):
    """lut[quantise(read_window)], alpha and colour of `no data` exactly where two fills differ"""
    a, tr = streaming.read_window(path, bbox, w, h, resampling=mode, level=level, fill=0, ctx=ctx, nodata=nodata)
    b, _ = streaming.read_window(path, bbox, w, h, resampling=mode, level=level, fill=1, ctx=ctx, nodata=nodata)
    return RR.colours(a[0], a[0] == b[0], lo, hi, lut, NODATA_RGBA, channels), tr, a[0] == b[0]


@pytest.mark.parametrize("mode", streaming.RESAMPLING_READ)
def test_render_window_is_the_lut_of_read_window(files, gpu_ctx, mode):
    file_stats = streaming.index_statistics(files["index"])
    for name, (bbox, w, h) in BOXES.items():
        for stretch, cmap, kw, channels in (("percentile:2,98", "gray", {}, 4), ("range:500,2500", "terrain", {}, 2),
                                            ("minmax", "heat", {"gamma": 2.2}, 1), ("stddev:2", "diverging",
                                                                                    {"transfer": "log"}, 4)):
            lo, hi = render.stretch_limits(file_stats, stretch)
            lut = render.build_lut(cmap, render.default_lut_size(**kw), **kw)
            assert len(lut) == (4096 if kw else 256)
            want, tr, has = _expected(files["path"], bbox, w, h, mode, lo, hi, lut, channels, gpu_ctx)
            got, gtr = streaming.render_window(files["path"], bbox, w, h, stretch=stretch, stats_from="file",
                                               colormap=cmap, resampling=mode, channels=channels,
                                               nodata_rgba=NODATA_RGBA, ctx=gpu_ctx, **kw)
            assert got.dtype == np.uint8 and got.shape == (h, w, channels) and gtr == tr
            assert np.array_equal(got, want), (name, stretch)
            assert has.any() and (name == "inner" or not has.all())  # data and no data both occur
            if channels > 1:  # alpha is 0 exactly where there is no data
                assert np.array_equal(got[..., -1] == 0, ~has)


def test_levels(files, gpu_ctx):
    bbox, w, h = FULL, 52, 60  # scale 5: level 2
    assert streaming.window_request(files["index"], bbox, w, h)["level"] == 2
    lo, hi = 500.0, 2500.0
    lut = render.build_lut("gray", 256)
    for level in (None, 0, 1):
        want, _, _ = _expected(files["path"], bbox, w, h, "average", lo, hi, lut, 4, gpu_ctx, level=level)
        got, _ = streaming.render_window(files["path"], bbox, w, h, stretch="range:500,2500", level=level,
                                         nodata_rgba=NODATA_RGBA, ctx=gpu_ctx)
        assert np.array_equal(got, want), level
    with pytest.raises(LookupError):
        streaming.render_window(files["path"], bbox, w, h, stretch="range:500,2500", level=7, ctx=gpu_ctx)


def test_stats_from_file_and_window(files, gpu_ctx):
    lut = render.build_lut("gray", 256)
    file_stats = streaming.index_statistics(files["index"])
    # the whole raster at level 0: the decoded window is the band, so "window" must see the band's own statistics
    w, h = 65, 75
    own = stats.band_statistics(files["band"], nodata=ND, bins=256, ctx=gpu_ctx)[0]
    for stretch in ("percentile:2,98", "minmax", "stddev:1"):
        for source, st in (("file", file_stats), ("window", own)):
            lo, hi = render.stretch_limits(st, stretch)
            want, _, _ = _expected(files["path"], FULL, w, h, "average", lo, hi, lut, 4, gpu_ctx, level=0)
            got, _ = streaming.render_window(files["path"], FULL, w, h, stretch=stretch, stats_from=source, level=0,
                                             nodata_rgba=NODATA_RGBA, ctx=gpu_ctx)
            assert np.array_equal(got, want), (stretch, source)
    # an inner window's own values stretch differently from the file's
    bbox, w, h = [-105.95, 40.75, -105.9, 40.8], 20, 20
    a, _ = streaming.render_window(files["path"], bbox, w, h, stretch="minmax", stats_from="file", ctx=gpu_ctx)
    b, _ = streaming.render_window(files["path"], bbox, w, h, stretch="minmax", stats_from="window", ctx=gpu_ctx)
    assert a.shape == b.shape and (a[..., 3] == 255).all() and (b[..., 3] == 255).all()
    req = streaming.window_request(files["index"], bbox, w, h)
    win = req["window"]
    assert req["level"] == 1
    # auto: the file's where it applies, the window's where it does not
    got, _ = streaming.render_window(files["path"], bbox, w, h, stretch="minmax", stats_from="auto", ctx=gpu_ctx)
    assert np.array_equal(got, a)
    got, _ = streaming.render_window(files["nostats"], bbox, w, h, stretch="minmax", stats_from="auto", ctx=gpu_ctx)
    assert np.array_equal(got, b) and win["width"] > 0
    got, _ = streaming.render_window(files["path"], bbox, w, h, stretch="minmax", stats_from="auto", nodata=None,
                                     ctx=gpu_ctx)
    want, _ = streaming.render_window(files["path"], bbox, w, h, stretch="minmax", stats_from="window", nodata=None,
                                      ctx=gpu_ctx)
    assert np.array_equal(got, want)
    # the errors of "file"
    with pytest.raises(LookupError, match='no "statistics"'):
        streaming.render_window(files["nostats"], bbox, w, h, stats_from="file", ctx=gpu_ctx)
    for nd in (None, -1):
        with pytest.raises(ValueError, match="statistics were taken with nodata"):
            streaming.render_window(files["path"], bbox, w, h, stats_from="file", nodata=nd, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="stats_from must be one of"):
        streaming.render_window(files["path"], bbox, w, h, stats_from="level", ctx=gpu_ctx)
    # a range needs none of it
    streaming.render_window(files["nostats"], bbox, w, h, stretch="range:0,1", stats_from="file", ctx=gpu_ctx)


def test_range_runs_no_statistics_pass(files, prof_ctx):
    bbox, w, h = BOXES["corner"]
    ran = lambda name: prof_ctx.profile_avg_ms(name) >= 0.0  # noqa: E731
    prof_ctx.profile_reset()
    streaming.render_window(files["nostats"], bbox, w, h, stretch="range:500,2500", ctx=prof_ctx)
    assert ran("render") and not ran("band_stats") and not ran("band_hist") and not ran("resample")
    prof_ctx.profile_reset()
    streaming.render_window(files["path"], bbox, w, h, stretch="percentile:2,98", stats_from="file", ctx=prof_ctx)
    assert ran("render") and not ran("band_stats") and not ran("band_hist")
    prof_ctx.profile_reset()
    streaming.render_window(files["path"], bbox, w, h, stretch="percentile:2,98", stats_from="window", ctx=prof_ctx)
    assert ran("render") and ran("band_stats") and ran("band_hist")


def test_bbox_outside_the_raster(files, prof_ctx):
    prof_ctx.profile_reset()
    for channels, want in ((1, [10]), (2, [10, 0]), (4, [10, 20, 30, 0])):
        got, tr = streaming.render_window(files["path"], [-100.0, 10.0, -99.0, 11.0], 9, 4, channels=channels,
                                          nodata_rgba=NODATA_RGBA, ctx=prof_ctx)
        assert got.shape == (4, 9, channels) and (got == np.array(want, dtype=np.uint8)).all()
        assert tr == [1.0 / 9, 0.0, -100.0, 0.0, -0.25, 11.0]
    assert prof_ctx.profile_avg_ms("render") < 0.0  # no GPU call


def test_render_command(files, gpu_ctx):
    d = files["dir"]
    bbox, w, h = BOXES["corner"]
    box = ",".join(str(v) for v in bbox)
    want, tr = streaming.render_window(files["path"], bbox, w, h, colormap="terrain", ctx=gpu_ctx)
    r = runner.invoke(app, ["render", str(files["path"]), "--bbox", box, "--out-size", f"{w}x{h}", "-o",
                            str(d / "x.png"), "--colormap", "terrain"])
    assert r.exit_code == 0, r.output
    assert np.array_equal(read_png((d / "x.png").read_bytes()), want)
    r = runner.invoke(app, ["render", str(files["path"]), "--bbox", box, "--out-size", f"{w}x{h}", "-o",
                            str(d / "x.tif"), "--colormap", "terrain"])
    assert r.exit_code == 0, r.output
    g = geotiff.read(d / "x.tif")
    assert g.data.shape == (4, h, w) and np.array_equal(g.data.transpose(1, 2, 0), want)
    assert list(g.transform)[:6] == streaming.window_request(files["index"], bbox, w, h)["transform"] == tr
    assert g.crs_string == CRS
    # an existing output needs --force
    r = runner.invoke(app, ["render", str(files["path"]), "--max-size", "40", "-o", str(d / "x.png")])
    assert r.exit_code == 1 and "use --force" in r.output
    # --max-size keeps the aspect ratio of the box (here the raster's bounds: 260 x 300 pixels), the colormap file, 2 channels
    ramp = d / "ramp.txt"
    ramp.write_text(render.format_colormap(render.COLORMAPS["heat"]))
    for n, shape in ((40, (40, 35)), (1, (1, 1)), (300, (300, 260))):
        r = runner.invoke(app, ["render", str(files["path"]), "--max-size", str(n), "-o", str(d / "x.png"), "--force",
                                "--colormap", str(ramp), "--channels", "2", "--resampling", "bilinear"])
        assert r.exit_code == 0, r.output
        got = read_png((d / "x.png").read_bytes())
        assert got.shape == shape + (2,)
        want, _ = streaming.render_window(files["path"], FULL, shape[1], shape[0], colormap="heat", channels=2,
                                          resampling="bilinear", ctx=gpu_ctx)
        assert np.array_equal(got, want)
    r = runner.invoke(app, ["render", str(files["nostats"]), "--max-size", "40", "-o", str(d / "y.png"),
                            "--stats-from", "file"])
    assert r.exit_code == 1 and 'no "statistics"' in r.output and not (d / "y.png").exists()
