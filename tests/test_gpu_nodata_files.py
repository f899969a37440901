"""Nodata through the streaming path, on files: create_streaming_array(nodata=...) with overviews, verify_streaming,
reconstruct, read_window and the CLI, against tests/nodata_ref.py applied to the numpy levels.  A 300 x 200 int16 raster
whose inner block holds 100..3000, with a 20-pixel -9999 collar and a few holes, in tiles of 64."""
import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import container, geotiff, streaming
from flac_raster_amd.cli import app
from tests import nodata_ref as N
from tests import window_ref as R
from tests.pyramid_ref import np_pyramid

pytestmark = pytest.mark.gpu
runner = CliRunner()

H, W, TILE, ND = 200, 300, 64, -9999
LO, HI = 100, 3000
T = geotiff.Affine(0.001, 0.0, -106.0, 0.0, -0.001, 41.0)
CRS = "EPSG:4326"
# three boxes: the whole raster and a margin around it, the collar's corner at a fractional scale, an inner piece
BOXES = {"all_and_margin": ([-106.01, 40.79, -105.69, 41.01], 50, 40),
         "corner": ([-105.999, 40.9503, -105.9521, 40.9997], 33, 17),
         "inner": ([-105.9, 40.85, -105.8, 40.95], 7, 5)}


def _band():
    rng = np.random.default_rng(51)
    a = np.full((H, W), ND, dtype=np.int16)
    a[20:-20, 20:-20] = rng.integers(LO, HI, size=(H - 40, W - 40), endpoint=True)
    a[50:53, 60:70] = ND
    a[100, 150] = ND
    a[120:140, 200:203] = ND
    a[64:128, 64:128][::2, ::2] = ND  # a sieve over one whole tile
    return a


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_ctx):
    """the band; a file without nodata and one with nodata and overviews, with their indexes; the masked pyramid"""
    d = tmp_path_factory.mktemp("nodata_files")
    band = _band()
    plain, masked = d / "plain.flac", d / "masked.flac"
    pi = streaming.create_streaming_array(band, T, CRS, plain, TILE, gpu_ctx)
    mi = streaming.create_streaming_array(band, T, CRS, masked, TILE, gpu_ctx, overviews=True, nodata=ND)
    shapes = streaming.overview_shapes(H, W, TILE)
    return {"dir": d, "band": band, "plain": plain, "plain_index": pi, "masked": masked, "masked_index": mi,
            "pyramid": N.np_pyramid_nodata(band, shapes, "average", ND), "shapes": shapes}


def test_without_nodata_the_file_is_what_it_was(files, gpu_ctx):
    again = files["dir"] / "again.flac"
    idx = streaming.create_streaming_array(files["band"], T, CRS, again, TILE, gpu_ctx, nodata=None)
    assert again.read_bytes() == files["plain"].read_bytes()
    assert "nodata" not in idx and "nodata" not in files["plain_index"] and idx == files["plain_index"]
    ov, ov2 = files["dir"] / "ov.flac", files["dir"] / "ov2.flac"
    i1 = streaming.create_streaming_array(files["band"], T, CRS, ov, TILE, gpu_ctx, overviews=True)
    i2 = streaming.create_streaming_array(files["band"], T, CRS, ov2, TILE, gpu_ctx, overviews=True, nodata=None)
    assert ov.read_bytes() == ov2.read_bytes() and i1 == i2
    assert "nodata" not in i1 and "nodata_aware" not in i1["overviews"]


def test_index_keys_and_tile_tags(files):
    idx = files["masked_index"]
    n, on_disk = streaming.read_index(files["masked"])
    assert on_disk == idx
    assert idx["nodata"] == ND and idx["overviews"]["nodata_aware"] is True
    assert idx["overviews"]["resampling"] == "average"
    assert [(lv["height"], lv["width"]) for lv in idx["overviews"]["levels"]] == files["shapes"]
    for k in streaming.overview_levels(idx):
        li = streaming.level_index(idx, k)
        assert li["nodata"] == ND
        for fr, data in zip(li["frames"], streaming.fetch_tiles(files["masked"], li["frames"], n)):
            meta = container.parse_metadata(data)
            assert meta.tag("GEOSPATIAL_NODATA") == str(float(ND)) == "-9999.0"
            assert container.read_raster_tags(meta)["nodata"] == float(ND)


def test_level0_frames_are_those_of_the_file_without_nodata(files):
    n0, pi = streaming.read_index(files["plain"])
    n1, mi = streaming.read_index(files["masked"])
    a = streaming.fetch_tiles(files["plain"], pi["frames"], n0)
    b = streaming.fetch_tiles(files["masked"], mi["frames"], n1)
    assert len(a) == len(b) == len(streaming.tile_grid(H, W, TILE))
    for x, y in zip(a, b):
        mx, my = container.parse_metadata(x), container.parse_metadata(y)
        assert x[mx.audio_offset:] == y[my.audio_offset:] and len(x) - mx.audio_offset > 0
        assert mx.tag("GEOSPATIAL_NODATA") == "None"


def test_every_level_is_the_masked_pyramid_and_holds_no_invented_value(files, gpu_ctx):
    pyr = files["pyramid"]
    plain_pyr = np_pyramid(files["band"], files["shapes"], "average")
    for k, want in enumerate(pyr):
        got, tr = streaming.reconstruct(files["masked"], gpu_ctx, level=k)
        assert np.array_equal(got[0], want), k
        assert list(tr)[:6] == streaming.level_transform(list(T)[:6], k)
        assert (((got >= LO) & (got <= HI)) | (got == ND)).all(), k
        if k:  # the unmasked pyramid, in contrast, invents values along the collar
            assert not (((plain_pyr[k] >= LO) & (plain_pyr[k] <= HI)) | (plain_pyr[k] == ND)).all()
    res = streaming.verify_streaming(files["masked"], files["band"], gpu_ctx)
    assert res["n_different"] == 0 and res["levels_checked"] == len(pyr)
    assert all(lv["n_different"] == 0 for lv in res["levels"])


@pytest.mark.parametrize("mode", R.MODES)
def test_read_window_equals_the_restatement_on_the_numpy_level(files, gpu_ctx, mode):
    idx = files["masked_index"]
    for name, (bbox, ow, oh) in BOXES.items():
        req = streaming.window_request(idx, bbox, ow, oh)
        win = req["window"]
        level = files["pyramid"][req["level"]]
        window = level[win["row_off"]:win["row_off"] + win["height"], win["col_off"]:win["col_off"] + win["width"]]
        got, tr = streaming.read_window(files["masked"], bbox, ow, oh, mode, ctx=gpu_ctx)
        want = N.resample_nodata(window, req["rect"], (oh, ow), mode, ND, ND)
        assert got.shape == (1, oh, ow) and tr == req["transform"]
        assert np.array_equal(got[0], want), (name, mode)
        assert (((got >= LO) & (got <= HI)) | (got == ND)).all(), (name, mode)
        # another fill; and masking switched off gives today's blend of the same window
        got7, _ = streaming.read_window(files["masked"], bbox, ow, oh, mode, ctx=gpu_ctx, fill=7)
        assert np.array_equal(got7[0], N.resample_nodata(window, req["rect"], (oh, ow), mode, 7, ND)), (name, mode)
        off, _ = streaming.read_window(files["masked"], bbox, ow, oh, mode, ctx=gpu_ctx, nodata=None)
        assert np.array_equal(off[0], R.resample(window, req["rect"], (oh, ow), mode, 0)), (name, mode)
    # a file without the key reads as it always did, and a box that misses the raster is all fill
    bbox, ow, oh = BOXES["corner"]
    a, _ = streaming.read_window(files["plain"], bbox, ow, oh, mode, ctx=gpu_ctx)
    req = streaming.window_request(files["plain_index"], bbox, ow, oh)
    win = req["window"]
    window = files["band"][win["row_off"]:win["row_off"] + win["height"], win["col_off"]:win["col_off"] + win["width"]]
    assert np.array_equal(a[0], R.resample(window, req["rect"], (oh, ow), mode, 0))
    miss, _ = streaming.read_window(files["masked"], [10.0, 10.0, 11.0, 11.0], 4, 3, mode, ctx=gpu_ctx)
    assert (miss == ND).all()
    miss0, _ = streaming.read_window(files["plain"], [10.0, 10.0, 11.0, 11.0], 4, 3, mode, ctx=gpu_ctx)
    assert (miss0 == 0).all()


def test_cli_source_nodata_through_to_a_tagged_window(files, tmp_path):
    tif, flac, out = tmp_path / "dem.tif", tmp_path / "dem.flac", tmp_path / "out.tif"
    geotiff.write(tif, files["band"][None], transform=T, epsg=4326, nodata=ND)
    r = runner.invoke(app, ["create-streaming", str(tif), "-o", str(flac), "--tile-size", str(TILE), "--nodata",
                            "source", "--overviews", "--verify"])
    assert r.exit_code == 0, r.output
    assert "NODATA: -9999" in r.output and "VERIFY: lossless" in r.output
    _, idx = streaming.read_index(flac)
    assert idx["nodata"] == ND and idx["overviews"]["nodata_aware"] is True
    assert idx["frames"] == files["masked_index"]["frames"] and idx["overviews"] == files["masked_index"]["overviews"]
    r = runner.invoke(app, ["info", str(flac)])
    assert r.exit_code == 0 and "Nodata: -9999" in r.output, r.output
    bbox = "-106.01,40.79,-105.69,41.01"
    r = runner.invoke(app, ["extract-streaming", str(flac), "--bbox", bbox, "--out-size", "50x40", "-o", str(out)])
    assert r.exit_code == 0, r.output
    back = geotiff.read(out)
    assert back.nodata == float(ND) and back.data.shape == (1, 40, 50)
    assert (((back.data >= LO) & (back.data <= HI)) | (back.data == ND)).all()
    want, _ = streaming.read_window(files["masked"], [float(v) for v in bbox.split(",")], 50, 40)
    assert np.array_equal(back.data, want)
    # --nodata none: today's blended result, which does hold invented values, and no tag
    out2 = tmp_path / "out2.tif"
    r = runner.invoke(app, ["extract-streaming", str(flac), "--bbox", bbox, "--out-size", "50x40", "--nodata", "none",
                            "-o", str(out2)])
    assert r.exit_code == 0, r.output
    blended = geotiff.read(out2)
    off, _ = streaming.read_window(files["masked"], [float(v) for v in bbox.split(",")], 50, 40, nodata=None)
    assert blended.nodata is None and np.array_equal(blended.data, off)
    assert not (((off >= LO) & (off <= HI)) | (off == ND) | (off == 0)).all()
    # the tag in the other selection modes, and the override
    for sel in (["--all"], ["--tile-id", "0"], ["--bbox", bbox, "--mosaic"], ["--all", "--level", "1"]):
        o = tmp_path / "sel.tif"
        r = runner.invoke(app, ["extract-streaming", str(flac), "-o", str(o)] + sel)
        assert r.exit_code == 0 and geotiff.read(o).nodata == float(ND), (sel, r.output)
        r = runner.invoke(app, ["extract-streaming", str(flac), "-o", str(o), "--nodata", "none"] + sel)
        assert r.exit_code == 0 and geotiff.read(o).nodata is None, (sel, r.output)
        r = runner.invoke(app, ["extract-streaming", str(flac), "-o", str(o), "--nodata", "-1"] + sel)
        assert r.exit_code == 0 and geotiff.read(o).nodata == -1.0, (sel, r.output)
    # a GeoTIFF without the tag cannot be its own source
    geotiff.write(tif, files["band"][None], transform=T, epsg=4326)
    r = runner.invoke(app, ["create-streaming", str(tif), "-o", str(flac), "--force", "--nodata", "source"])
    assert r.exit_code == 1 and "no GDAL_NODATA tag" in r.output
