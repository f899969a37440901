"""Multi-band streaming files on the GPU: a 3-band int16 GeoTIFF of 150 x 130 (tile 64: partial edge tiles, two overview
levels), the bands with different value ranges and a nodata hole each in a different place.  The format (every stored
band's tiles are those of the file written from that band alone), the readers (bands=), the statistics, --verify, and
the render of a band and of a three-band composite."""
import json
import struct

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import geotiff, render, stats, streaming
from flac_raster_amd.cli import app
from tests import composite_ref as CR
from tests.render_cases import read_png

pytestmark = pytest.mark.gpu
runner = CliRunner()

H, W, TILE, ND = 130, 150, 64, -9999
T = geotiff.Affine(0.5, 0.0, -106.0, 0.0, -0.25, 41.0)
CRS = "EPSG:4326"
FULL = [-106.0, 41.0 - H * 0.25, -106.0 + W * 0.5, 41.0]
OPTS = dict(overviews=True, nodata=ND, stats=True)


def _source():
    rng = np.random.default_rng(81)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([(20 * x + 3 * y + rng.integers(0, 40, (H, W))),                # 0 .. ~3400
                  (-2000 + 9 * y + 2 * x + rng.integers(0, 15, (H, W))),         # ~-2000 .. ~-500
                  (rng.integers(100, 160, (H, W)) + (x // 16) * 5)]).astype(np.int16)  # ~100 .. ~205
    a[0, 10:30, 20:50] = ND
    a[1, 60:100, 90:140] = ND
    a[2, 100:, :40] = ND
    return a


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_ctx):
    d = tmp_path_factory.mktemp("bands_files")
    a = _source()
    geotiff.write(d / "src.tif", a, transform=T, epsg=4326, nodata=ND, planar=2)
    out = {"dir": d, "data": a, "tif": d / "src.tif", "multi": d / "multi.flac"}
    out["index"] = streaming.create_streaming(d / "src.tif", d / "multi.flac", TILE, ctx=gpu_ctx, bands="all", **OPTS)
    for b in (1, 2, 3):  # the file the same call writes from band b alone, as a single-band raster
        out[b] = d / f"band{b}.flac"
        streaming.create_streaming_array(a[b - 1], T, CRS, out[b], tile_size=TILE, ctx=gpu_ctx, **OPTS)
    return out


def _read(path):
    data = path.read_bytes()
    n = struct.unpack(">I", data[:4])[0]
    return json.loads(data[4:4 + n]), data[4 + n:]


def _tiles(index, body):
    """per level: [(window, bbox, the tile's bytes)]"""
    return [[(f["window"], f["bbox"], body[f["byte_offset"]:f["byte_offset"] + f["byte_size"]])
             for f in streaming.level_index(index, k)["frames"]] for k in streaming.overview_levels(index)]


# ------------------------------------------------------------------------------------------------ the format
def test_every_band_is_stored_as_the_single_band_file_of_that_band(files):
    index, body = _read(files["multi"])
    assert index == files["index"] and streaming.bands_of(index) == [1, 2, 3] and index["bands"]["count"] == 3
    total, fid = 0, 0
    for b in (1, 2, 3):
        bi = streaming.band_index(index, b)
        si, sbody = _read(files[b])
        assert streaming.overview_levels(bi) == streaming.overview_levels(si) == [0, 1, 2]
        got, want = _tiles(bi, body), _tiles(si, sbody)
        assert got == want, b  # windows, bboxes, headers and frames, level by level
        assert any(w["width"] < TILE for w, _, _ in got[0]) and any(w["height"] < TILE for w, _, _ in got[0])
        assert streaming.index_statistics(bi) == streaming.index_statistics(si)
        # frame ids and byte offsets run on through the file: band after band, level after level
        for k in streaming.overview_levels(bi):
            for f in streaming.level_index(bi, k)["frames"]:
                assert (f["frame_id"], f["byte_offset"]) == (fid, total)
                fid, total = fid + 1, total + f["byte_size"]
        assert len(sbody) == sum(len(t) for lv in want for _, _, t in lv)
    # the file's length is the sum of its parts
    head = 4 + struct.unpack(">I", files["multi"].read_bytes()[:4])[0]
    assert files["multi"].stat().st_size == head + total == head + sum(len(_read(files[b])[1]) for b in (1, 2, 3))


def test_the_index_minus_bands_is_the_band_1_index_key_for_key(files):
    index, _ = _read(files["multi"])
    single, _ = _read(files[1])
    top = {k: v for k, v in index.items() if k != "bands"}
    assert list(index)[-1] == "bands" and list(top) == list(single)
    assert top == single  # frames included: the offsets are relative to the body
    entries = index["bands"]["entries"]
    assert [e["band"] for e in entries] == [2, 3]
    assert all(list(e) == ["band", "frames", "overviews", "statistics"] for e in entries)
    assert all(e["overviews"]["nodata_aware"] is True and e["overviews"]["resampling"] == "average" for e in entries)


def test_optional_keys_follow_the_top_level_ones_and_the_order_given_is_the_file_order(files, gpu_ctx):
    out = files["dir"] / "plain31.flac"
    index = streaming.create_streaming(files["tif"], out, TILE, ctx=gpu_ctx, bands=[3, 1])
    assert streaming.bands_of(index) == [1, 3] and index["bands"]["count"] == 3
    assert list(index) == ["crs", "transform", "width", "height", "tile_size", "frames", "bands"]
    assert [list(e) for e in index["bands"]["entries"]] == [["band", "frames"]]
    arr, _ = streaming.reconstruct(out, gpu_ctx, bands=[3, 1])
    assert np.array_equal(arr, files["data"][[2, 0]])
    planes = streaming.create_streaming_bands_array(files["data"][[1, 0]], [2, 1], T, CRS, files["dir"] / "arr.flac",
                                                    tile_size=TILE, ctx=gpu_ctx, source_count=7)
    assert streaming.bands_of(planes) == [1, 2] and planes["bands"]["count"] == 7
    assert np.array_equal(streaming.reconstruct(files["dir"] / "arr.flac", gpu_ctx, bands="all")[0], files["data"][:2])


def test_a_call_without_bands_writes_what_it_always_wrote(files, gpu_ctx):
    a, b = files["dir"] / "nobands.flac", files["dir"] / "band1_array.flac"
    for kw in ({}, OPTS):
        streaming.create_streaming(files["tif"], a, TILE, ctx=gpu_ctx, **kw)
        streaming.create_streaming_array(files["data"][0], T, CRS, b, tile_size=TILE, ctx=gpu_ctx, **kw)
        assert a.read_bytes() == b.read_bytes() and "bands" not in _read(a)[0]
    assert a.read_bytes() == files[1].read_bytes()


# ------------------------------------------------------------------------------------------------ the readers
def test_extract_all_and_verify_give_the_source_bands_exactly(files, gpu_ctx):
    out = files["dir"] / "all.tif"
    streaming.extract_all(files["multi"], out, ctx=gpu_ctx, bands="all")
    back = geotiff.read(out)
    assert np.array_equal(back.data, files["data"]) and back.nodata == ND
    for k, shape in ((1, (3, 65, 75)), (2, (3, 33, 38))):
        arr, _ = streaming.reconstruct(files["multi"], gpu_ctx, level=k, bands="all")
        assert arr.shape == shape
        for i, b in enumerate((1, 2, 3)):
            assert np.array_equal(arr[i], streaming.reconstruct(files[b], gpu_ctx, level=k)[0][0])
    # no band named: band 1, as ever
    assert np.array_equal(streaming.reconstruct(files["multi"], gpu_ctx)[0], files["data"][:1])
    for b in (1, 2, 3):
        ex = streaming.verify_streaming(files["multi"], files["data"][b - 1], gpu_ctx, band_number=b)
        assert ex["n_different"] == 0 and ex["levels_checked"] == 3
    assert streaming.verify_streaming(files["multi"], files["data"][0], gpu_ctx, band_number=2)["n_different"] > 0


def test_cli_create_verify_extract_info_and_stats(files):
    out = files["dir"] / "cli.flac"
    r = runner.invoke(app, ["create-streaming", str(files["tif"]), "-o", str(out), "--tile-size", str(TILE), "--bands",
                            "1,2,3", "--overviews", f"--nodata={ND}", "--stats", "--verify"])
    assert r.exit_code == 0 and "VERIFY: lossless (bands 1,2,3, levels 0..2)" in r.output, r.output
    assert "BANDS: 1,2,3 of 3" in r.output
    assert out.read_bytes() == files["multi"].read_bytes()
    r = runner.invoke(app, ["create-streaming", str(files["tif"]), "-o", str(out), "--tile-size", str(TILE), "--force",
                            "--bands", "all", "--verify"])
    assert r.exit_code == 0 and "VERIFY: lossless (bands 1,2,3)" in r.output, r.output
    tif = files["dir"] / "cli.tif"
    r = runner.invoke(app, ["extract-streaming", str(files["multi"]), "--all", "--bands", "3,1", "-o", str(tif)])
    assert r.exit_code == 0, r.output
    assert np.array_equal(geotiff.read(tif).data, files["data"][[2, 0]])
    bbox = [-100.0, 15.0, -60.0, 35.0]
    r = runner.invoke(app, ["extract-streaming", str(files["multi"]), "--bbox", ",".join(map(str, bbox)), "--mosaic",
                            "--bands", "all", "-o", str(tif)])
    assert r.exit_code == 0, r.output
    arr, win, _ = streaming.extract_bbox_mosaic(files["multi"], bbox, bands="all")
    assert np.array_equal(geotiff.read(tif).data, arr)
    sl = np.s_[win["row_off"]:win["row_off"] + win["height"], win["col_off"]:win["col_off"] + win["width"]]
    assert arr.shape[0] == 3 and arr.size and np.array_equal(arr, files["data"][(slice(None),) + sl])
    r = runner.invoke(app, ["extract-streaming", str(files["multi"]), "--bbox", ",".join(map(str, bbox)), "--out-size",
                            "40x30", "--bands", "2,3", "-o", str(tif)])
    assert r.exit_code == 0, r.output
    assert np.array_equal(geotiff.read(tif).data, streaming.read_window(files["multi"], bbox, 40, 30, bands=(2, 3))[0])
    r = runner.invoke(app, ["extract-streaming", str(files["multi"]), "--tile-id", "0", "--bands", "2", "-o", str(tif)])
    assert r.exit_code == 1 and "Tile ID 0 not found" in r.output  # band 2's ids run on from band 1's
    first = streaming.band_index(files["index"], 2)["frames"][0]["frame_id"]
    r = runner.invoke(app, ["extract-streaming", str(files["multi"]), "--tile-id", str(first), "--bands", "2", "-o",
                            str(tif)])
    assert r.exit_code == 0 and np.array_equal(geotiff.read(tif).data[0], files["data"][1][:TILE, :TILE]), r.output
    r = runner.invoke(app, ["extract-streaming", str(files["multi"]), "--all", "--bands", "4", "-o", str(tif)])
    assert r.exit_code == 1 and "band 4 not in this file (bands present: [1, 2, 3])" in r.output
    r = runner.invoke(app, ["info", str(files["multi"])])
    assert r.exit_code == 0 and "Bands stored: 1,2,3 of 3" in r.output and "Band 3:" in r.output, r.output
    r = runner.invoke(app, ["stats", str(files["multi"]), "--json"])
    assert r.exit_code == 0 and json.loads(r.output)["band_numbers"] == [1, 2, 3], r.output
    r = runner.invoke(app, ["stats", str(files["multi"]), "--band", "2"])
    assert r.exit_code == 0 and "Band 2:" in r.output and "Band 1:" not in r.output, r.output


@pytest.mark.parametrize("mode", streaming.RESAMPLING_READ)
def test_read_window_of_two_bands_is_the_two_single_band_reads_stacked(files, gpu_ctx, mode):
    for bbox, (w, h) in (([-100.0, 15.0, -60.0, 35.0], (37, 23)), (FULL, (40, 30)),
                         ([-110.0, 30.0, -90.0, 45.0], (16, 16))):  # level 0, an overview level, over the edge
        for nodata in ("index", None):
            got, tr = streaming.read_window(files["multi"], bbox, w, h, resampling=mode, ctx=gpu_ctx, nodata=nodata,
                                            bands=(3, 1))
            want = [streaming.read_window(files[b], bbox, w, h, resampling=mode, ctx=gpu_ctx, nodata=nodata)
                    for b in (3, 1)]
            assert got.shape == (2, h, w) and tr == want[0][1]
            assert np.array_equal(got, np.concatenate([x[0] for x in want])), (bbox, nodata)
            one, _ = streaming.read_window(files["multi"], bbox, w, h, resampling=mode, ctx=gpu_ctx, nodata=nodata)
            assert np.array_equal(one, want[1][0])  # no band named: band 1
    miss, _ = streaming.read_window(files["multi"], [0.0, 0.0, 1.0, 1.0], 4, 3, resampling=mode, bands=(3, 1))
    assert miss.shape == (2, 3, 4) and (miss == ND).all()


def test_only_the_named_bands_tiles_are_fetched(files, gpu_ctx, monkeypatch):
    index = files["index"]
    asked = []
    real = streaming.fetch_tiles

    def spy(src, frames, index_size):
        asked.extend((f["byte_offset"], f["byte_size"]) for f in frames)
        return real(src, frames, index_size)

    monkeypatch.setattr(streaming, "fetch_tiles", spy)

    def ranges(b):
        bi = streaming.band_index(index, b)
        return {(f["byte_offset"], f["byte_size"]) for k in streaming.overview_levels(bi)
                for f in streaming.level_index(bi, k)["frames"]}

    streaming.read_window(files["multi"], [-100.0, 15.0, -60.0, 35.0], 37, 23, ctx=gpu_ctx, bands=(3, 1))
    assert asked and set(asked) <= ranges(3) | ranges(1) and set(asked) & ranges(3) and set(asked) & ranges(1)
    assert not set(asked) & ranges(2)
    del asked[:]
    streaming.render_window(files["multi"], FULL, 30, 26, ctx=gpu_ctx, bands=(3, 2, 3))
    assert asked and set(asked) <= ranges(3) | ranges(2) and not set(asked) & ranges(1)
    del asked[:]
    streaming.reconstruct(files["multi"], gpu_ctx, bands=[2])
    assert set(asked) == {(f["byte_offset"], f["byte_size"]) for f in streaming.band_index(index, 2)["frames"]}


def test_stats_of_the_file_are_the_stats_of_the_sources_bands(files, gpu_ctx):
    got = stats.raster_file_statistics(files["multi"], ctx=gpu_ctx)
    want = stats.raster_file_statistics(files["tif"], ctx=gpu_ctx)
    assert got["band_numbers"] == want["band_numbers"] == [1, 2, 3] and got["nodata"] == want["nodata"] == ND
    assert got["bands"] == want["bands"] and len(got["bands"]) == 3
    assert [b["nodata_count"] for b in got["bands"]] == [20 * 30, 40 * 50, 30 * 40]
    one = stats.raster_file_statistics(files["multi"], ctx=gpu_ctx, band=3)
    assert one["band_numbers"] == [3] and one["bands"] == want["bands"][2:]
    assert stats.raster_file_statistics(files["tif"], ctx=gpu_ctx, band=2)["bands"] == want["bands"][1:2]
    # and what create-streaming --stats stored per band is what a 256-bin read gives
    for b in (1, 2, 3):
        stored = streaming.index_statistics(streaming.band_index(files["index"], b))
        assert stored == stats.statistics_from_index(stats.statistics_to_index(want["bands"][b - 1]))
    with pytest.raises(LookupError, match="band 4 not in this file"):
        stats.raster_file_statistics(files["multi"], ctx=gpu_ctx, band=4)


# ------------------------------------------------------------------------------------------------ the render
def _planes(files, req, bands):
    win = req["window"]
    return files["data"][[b - 1 for b in bands], win["row_off"]:win["row_off"] + win["height"],
                         win["col_off"]:win["col_off"] + win["width"]]


@pytest.mark.parametrize("mode", ["average", "bilinear", "nearest"])
def test_composite_render_equals_the_reference_on_the_decoded_planes(files, gpu_ctx, mode):
    bands = (1, 2, 3)
    index = files["index"]
    for bbox, (w, h), level, gamma in (([-100.0, 15.0, -60.0, 35.0], (37, 23), 0, 1.0), (FULL, (50, 40), None, 2.2)):
        req = streaming.window_request(index, bbox, w, h, level)
        planes = _planes(files, req, bands) if req["level"] == 0 else np.concatenate(
            [streaming.reconstruct(files[b], gpu_ctx, level=req["level"])[0] for b in bands])[
                (slice(None),) + np.s_[req["window"]["row_off"]:req["window"]["row_off"] + req["window"]["height"],
                                       req["window"]["col_off"]:req["window"]["col_off"] + req["window"]["width"]]]
        lut = render.build_lut("gray", render.default_lut_size(gamma, "linear"), gamma, "linear")
        for stats_from in ("file", "window"):
            if stats_from == "file":
                st = [streaming.index_statistics(streaming.band_index(index, b)) for b in bands]
            else:
                st = stats.band_statistics(np.ascontiguousarray(planes), nodata=ND, bins=256, ctx=gpu_ctx)
            lim = [render.stretch_limits(s, "percentile:2,98") for s in st]
            lo3, hi3 = [x[0] for x in lim], [x[1] for x in lim]
            assert len(set(lim)) == 3  # each band its own stretch
            want = CR.composite(planes, req["rect"], (h, w), mode, ND, lo3, hi3, lut, (9, 8, 7, 0))
            got, tr = streaming.render_window(files["multi"], bbox, w, h, resampling=mode, level=level, gamma=gamma,
                                              stats_from=stats_from, nodata_rgba=(9, 8, 7, 0), ctx=gpu_ctx, bands=bands)
            assert got.shape == (h, w, 4) and tr == req["transform"]
            assert np.array_equal(got, want), (bbox, stats_from)
            assert (got[..., 3] == 0).any() and (got[..., 3] == 255).any()  # holes of single bands show
    # range:lo,hi applies to all three; a permutation of the bands permutes the planes
    got, _ = streaming.render_window(files["multi"], FULL, 30, 26, stretch="range:-2000,3000", resampling=mode,
                                     ctx=gpu_ctx, bands=(3, 1, 2), level=0)
    req = streaming.window_request(index, FULL, 30, 26, 0)
    want = CR.composite(_planes(files, req, (3, 1, 2)), req["rect"], (26, 30), mode, ND, [-2000.0] * 3, [3000.0] * 3,
                        render.build_lut("gray", 256), 0)
    assert np.array_equal(got, want)


def test_composite_of_a_box_that_misses_the_raster_and_of_a_missing_band(files):
    img, _ = streaming.render_window(files["multi"], [0.0, 0.0, 1.0, 1.0], 5, 4, nodata_rgba=(1, 2, 3, 4), bands=(1, 2, 3))
    assert img.shape == (4, 5, 4) and (img == (1, 2, 3, 4)).all()
    with pytest.raises(LookupError, match="band 4 not in this file"):
        streaming.render_window(files["multi"], FULL, 5, 4, bands=(1, 2, 4))
    with pytest.raises(LookupError, match="band 2 not in this file"):
        streaming.render_window(files[1], FULL, 5, 4, bands=(1, 2, 3))


def test_cli_composite_png_reads_back_as_the_array(files, gpu_ctx):
    png = files["dir"] / "rgb.png"
    bbox = [-100.0, 15.0, -60.0, 35.0]
    r = runner.invoke(app, ["render", str(files["multi"]), "--bands", "3,2,1", "--bbox", ",".join(map(str, bbox)),
                            "--out-size", "48x31", "--gamma", "1.8", "-o", str(png)])
    assert r.exit_code == 0 and "bands 3,2,1" in r.output, r.output
    want, _ = streaming.render_window(files["multi"], bbox, 48, 31, gamma=1.8, ctx=gpu_ctx, bands=(3, 2, 1))
    assert np.array_equal(read_png(png.read_bytes()), want)
    assert len({tuple(p) for p in want.reshape(-1, 4)[:, :3]}) > 50 and (want[..., 0] != want[..., 2]).any()  # colour
    tif = files["dir"] / "rgb.tif"
    r = runner.invoke(app, ["render", str(files["multi"]), "--bands", "3,2,1", "--max-size", "40", "-o", str(tif)])
    assert r.exit_code == 0, r.output
    assert geotiff.read(tif).data.shape[0] == 4


def test_render_of_band_2_is_the_render_of_the_file_made_from_band_2(files, gpu_ctx):
    for kw in (dict(), dict(stats_from="window", resampling="bilinear"), dict(hillshade=(315.0, 45.0), z_factor=0.01),
               dict(stretch="minmax", colormap="terrain", channels=2)):
        got, _ = streaming.render_window(files["multi"], FULL, 60, 52, ctx=gpu_ctx, band=2, **kw)
        want, _ = streaming.render_window(files[2], FULL, 60, 52, ctx=gpu_ctx, **kw)
        assert np.array_equal(got, want), kw
        base, _ = streaming.render_window(files["multi"], FULL, 60, 52, ctx=gpu_ctx, **kw)
        assert np.array_equal(base, streaming.render_window(files[1], FULL, 60, 52, ctx=gpu_ctx, **kw)[0])
        assert not np.array_equal(base, got)
    png = files["dir"] / "b2.png"
    r = runner.invoke(app, ["render", str(files["multi"]), "--band", "2", "--out-size", "60x52", "-o", str(png)])
    assert r.exit_code == 0 and "band 2" in r.output, r.output
    assert np.array_equal(read_png(png.read_bytes()), streaming.render_window(files[2], FULL, 60, 52, ctx=gpu_ctx)[0])
