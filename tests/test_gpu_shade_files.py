"""The hillshaded render through files: streaming.render_window(hillshade=...) and `render --hillshade` on a 256 x 256
int16 ramp-and-bump raster with a nodata collar, tile 64, overviews.  The seam: the halves of a box, rendered on their
own, equal the halves of the whole byte for byte, which needs the decoded window to reach one output pixel beyond the
box (window_request's margin)."""
import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import geotiff, render, streaming
from flac_raster_amd.cli import app
from tests import shade_ref as SR
from tests.render_cases import read_png

pytestmark = pytest.mark.gpu
runner = CliRunner()

N, TILE, ND, COLLAR = 256, 64, -9999, 8
T = geotiff.Affine(1.0, 0.0, 0.0, 0.0, -1.0, float(N))  # one ground unit per pixel, pixel edges on integers
CRS = "EPSG:32613"
FULL = (0.0, 0.0, float(N), float(N))
STRETCH = "range:0,2200"
HS = (315.0, 45.0)


def _terrain():
    y, x = np.mgrid[0:N, 0:N].astype(np.float64)
    z = 3.0 * x + 2.0 * y + 600.0 * np.exp(-((x - 128.0) ** 2 + (y - 120.0) ** 2) / 900.0)
    band = np.rint(z).astype(np.int16)
    band[:COLLAR], band[-COLLAR:], band[:, :COLLAR], band[:, -COLLAR:] = ND, ND, ND, ND
    return band


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_ctx):
    d = tmp_path_factory.mktemp("shade_files")
    band = _terrain()
    index = streaming.create_streaming_array(band, T, CRS, d / "dem.flac", tile_size=TILE, ctx=gpu_ctx, overviews=True,
                                             nodata=ND)
    assert "statistics" not in index and len(streaming.overview_levels(index)) > 1
    return {"dir": d, "band": band, "path": d / "dem.flac", "index": index}


def _restated(window, req, w, h, bbox, mode, channels=4, shade_only=False, strength=1.0):
    """the restatement's image of a decoded window under a request"""
    lut = render.build_lut([(0, 255, 255, 255), (1, 255, 255, 255)], 1) if shade_only else render.build_lut("gray", 256)
    lo, hi = (0.0, 1.0) if shade_only else (0.0, 2200.0)
    kx, ky = render.shade_scales((bbox[2] - bbox[0]) / w, (bbox[3] - bbox[1]) / h, 1.0)
    return SR.render_shaded(window, req["rect"], (h, w), mode, ND, lo, hi, lut, 0, channels,
                            render.light_vector(*HS), kx, ky, render.shade_table(strength))


def _window(band, req):
    win = req["window"]
    return band[win["row_off"]:win["row_off"] + win["height"], win["col_off"]:win["col_off"] + win["width"]]


@pytest.mark.parametrize("mode", ["average", "bilinear"])
def test_the_halves_of_a_box_equal_the_halves_of_the_whole(files, gpu_ctx, mode):
    """boxes on integer pixel edges, power-of-two sizes, level 0 at two source pixels per output pixel: the apron of a
    half lies two source pixels beyond its box, one more than a plain read decodes"""
    kw = dict(stretch=STRETCH, resampling=mode, level=0, hillshade=HS, ctx=gpu_ctx)
    whole, _ = streaming.render_window(files["path"], (64.0, 64.0, 192.0, 192.0), 64, 64, **kw)
    halves = {"left": ((64.0, 64.0, 128.0, 192.0), 32, 64, whole[:, :32]),
              "right": ((128.0, 64.0, 192.0, 192.0), 32, 64, whole[:, 32:]),
              "top": ((64.0, 128.0, 192.0, 192.0), 64, 32, whole[:32]),
              "bottom": ((64.0, 64.0, 192.0, 128.0), 64, 32, whole[32:])}
    for name, (bbox, w, h, want) in halves.items():
        # first: the restatement on the window a plain read decodes (no margin) differs along the seam, and on the
        # widened window it gives the whole's half: the test cannot pass without the margin
        plain = streaming.window_request(files["index"], bbox, w, h, level=0)
        wide = streaming.window_request(files["index"], bbox, w, h, level=0, margin=1)
        a = _restated(_window(files["band"], plain), plain, w, h, bbox, mode)
        b = _restated(_window(files["band"], wide), wide, w, h, bbox, mode)
        assert np.array_equal(b, want), name
        seam = {"left": a[:, -1] != want[:, -1], "right": a[:, 0] != want[:, 0], "top": a[-1] != want[-1],
                "bottom": a[0] != want[0]}[name]
        assert seam.any(), name
        got, _ = streaming.render_window(files["path"], bbox, w, h, **kw)
        assert np.array_equal(got, want), name
    # and at the level the request picks by itself
    kw.pop("level")
    whole, _ = streaming.render_window(files["path"], (64.0, 64.0, 192.0, 192.0), 64, 64, **kw)
    left, _ = streaming.render_window(files["path"], (64.0, 64.0, 128.0, 192.0), 32, 64, **kw)
    lower, _ = streaming.render_window(files["path"], (64.0, 64.0, 192.0, 128.0), 64, 32, **kw)
    assert np.array_equal(left, whole[:, :32]) and np.array_equal(lower, whole[32:])


def test_shade_only_needs_no_statistics(files, gpu_ctx):
    with pytest.raises(LookupError):
        streaming.render_window(files["path"], FULL, 64, 64, stats_from="file", ctx=gpu_ctx)
    img, _ = streaming.render_window(files["path"], FULL, N, N, resampling="nearest", hillshade=HS, shade_only=True,
                                     channels=2, ctx=gpu_ctx)
    req = streaming.window_request(files["index"], FULL, N, N, margin=1)
    want = _restated(_window(files["band"], req), req, N, N, FULL, "nearest", channels=2, shade_only=True)
    assert np.array_equal(img, want)
    inside = img[COLLAR + 2:-COLLAR - 2, COLLAR + 2:-COLLAR - 2]
    assert (inside[..., 1] == 255).all() and len(np.unique(inside[..., 0])) > 20  # grey levels of the shade alone


def test_a_nodata_collar_stays_transparent_and_its_neighbours_are_shaded_from_valid_pixels(files, gpu_ctx):
    img, _ = streaming.render_window(files["path"], FULL, N, N, stretch=STRETCH, resampling="nearest", hillshade=HS,
                                     ctx=gpu_ctx)
    assert (img[:COLLAR] == 0).all() and (img[-COLLAR:] == 0).all() and (img[:, :COLLAR] == 0).all() \
        and (img[:, -COLLAR:] == 0).all()
    assert (img[COLLAR:-COLLAR, COLLAR:-COLLAR, 3] == 255).all()
    req = streaming.window_request(files["index"], FULL, N, N, margin=1)
    want = _restated(files["band"], req, N, N, FULL, "nearest")
    assert np.array_equal(img, want)
    # the ring beside the collar: the centre stands in for the missing neighbours, so the plane's slope is halved
    # there and the shade differs from the interior's but is no outlier (not black, not the nodata colour)
    ring, interior = img[COLLAR, 40:60, 0].astype(int), img[COLLAR + 3, 40:60, 0].astype(int)
    assert (ring > 0).all() and (np.abs(ring - interior) < 80).all()


def test_cli_writes_the_functions_pixels(files, gpu_ctx):
    d = files["dir"]
    box, bbox, w, h = "32,32,224,160", (32.0, 32.0, 224.0, 160.0), 96, 64
    want, tr = streaming.render_window(files["path"], bbox, w, h, stretch=STRETCH, colormap="terrain",
                                       hillshade=(300.0, 40.0), z_factor=2.0, shade_strength=0.75, ctx=gpu_ctx)
    args = ["render", str(files["path"]), "--bbox", box, "--out-size", f"{w}x{h}", "--stretch", STRETCH, "--colormap",
            "terrain", "--hillshade", "300,40", "--z-factor", "2", "--shade-strength", "0.75", "-o"]
    r = runner.invoke(app, args + [str(d / "s.png")])
    assert r.exit_code == 0, r.output
    assert "SUCCESS" in r.output and "hillshade 300,40" in r.output
    assert np.array_equal(read_png((d / "s.png").read_bytes()), want)
    r = runner.invoke(app, args + [str(d / "s.tif")])
    assert r.exit_code == 0, r.output
    g = geotiff.read(d / "s.tif")
    assert np.array_equal(g.data.transpose(1, 2, 0), want) and list(g.transform)[:6] == tr
    # --hillshade alone is 315,45; --shade-only on a file without statistics
    r = runner.invoke(app, ["render", str(files["path"]), "--max-size", "64", "--hillshade", "--shade-only", "-o",
                            str(d / "o.png")])
    assert r.exit_code == 0, r.output
    want, _ = streaming.render_window(files["path"], FULL, 64, 64, hillshade=HS, shade_only=True, ctx=gpu_ctx)
    assert np.array_equal(read_png((d / "o.png").read_bytes()), want)
    r = runner.invoke(app, ["render", str(files["path"]), "--max-size", "64", "--stretch", STRETCH, "-o",
                            str(d / "h.png"), "--hillshade"])
    assert r.exit_code == 0, r.output
    want, _ = streaming.render_window(files["path"], FULL, 64, 64, stretch=STRETCH, hillshade=HS, ctx=gpu_ctx)
    assert np.array_equal(read_png((d / "h.png").read_bytes()), want)


def test_render_without_hillshade_is_what_it_was(files, gpu_ctx):
    d = files["dir"]
    r = runner.invoke(app, ["render", str(files["path"]), "--max-size", "80", "--stretch", STRETCH, "--colormap",
                            "heat", "-o", str(d / "p.png")])
    assert r.exit_code == 0, r.output
    assert "hillshade" not in r.output
    want, _ = streaming.render_window(files["path"], FULL, 80, 80, stretch=STRETCH, colormap="heat", ctx=gpu_ctx)
    assert np.array_equal(read_png((d / "p.png").read_bytes()), want)
    # and the function itself against the plain device call on the window a plain read decodes
    req = streaming.window_request(files["index"], FULL, 80, 80)
    src = streaming.Source(files["path"])
    buf, dtype = streaming.decode_into_window(
        streaming.fetch_tiles(src, req["frames"], streaming.read_index(src)[0]),
        req["frames"], (req["window"]["col_off"], req["window"]["row_off"]),
        (req["window"]["height"], req["window"]["width"]), gpu_ctx)
    dst = gpu_ctx.alloc(80 * 80 * 4)
    try:
        gpu_ctx.render_window_device(buf.ptr, gpu_ctx.make_raster_desc(req["window"]["height"], req["window"]["width"],
                                                                        dtype), dst.ptr, 80, 80, req["rect"],
                                     "average", 0.0, 2200.0, render.build_lut("heat", 256), nodata_rgba=0, channels=4,
                                     nodata=ND)
        got = np.empty((80, 80, 4), dtype=np.uint8)
        dst.download(out=got)
    finally:
        buf.close()
        dst.close()
    assert np.array_equal(got, want)
