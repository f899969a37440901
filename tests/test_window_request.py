"""The pure half of the windowed read: streaming.pick_level_for_scale and streaming.window_request on a hand-made
index (transform [0.5, 0, 100, 0, -0.5, 200], 300 x 420, tile 64, levels 0..3), and the CLI's --out-size option
conflicts, all rejected before anything is read.  No GPU."""
import math

import pytest
from typer.testing import CliRunner

from flac_raster_amd import streaming
from flac_raster_amd.cli import app

runner = CliRunner()

W, H, TILE = 300, 420, 64
TRANSFORM = [0.5, 0.0, 100.0, 0.0, -0.5, 200.0]


def _frames(width, height, transform, id0=0):
    a, _, c, _, e, f = transform
    out = []
    for i, (col, row, w, h) in enumerate(streaming.tile_grid(height, width, TILE)):
        out.append({"frame_id": id0 + i, "window": {"col_off": col, "row_off": row, "width": w, "height": h},
                    "bbox": [c + col * a, f + (row + h) * e, c + (col + w) * a, f + row * e],
                    "byte_offset": 1000 * (id0 + i), "byte_size": 1000})
    return out


def _index(levels=3, transform=TRANSFORM):
    index = {"crs": "EPSG:32633", "transform": list(transform), "width": W, "height": H, "tile_size": TILE,
             "frames": _frames(W, H, transform)}
    lv = []
    for k, (h, w) in enumerate(streaming.overview_shapes(H, W, TILE, levels), start=1):
        t = streaming.level_transform(transform, k)
        lv.append({"level": k, "factor": 2 ** k, "width": w, "height": h, "transform": t,
                   "frames": _frames(w, h, t, id0=1000 * k)})
    if lv:
        index["overviews"] = {"resampling": "average", "levels": lv}
    return index


INDEX = _index()


def test_the_index_has_levels_0_to_3():
    assert streaming.overview_levels(INDEX) == [0, 1, 2, 3]
    assert [(lv["width"], lv["height"]) for lv in INDEX["overviews"]["levels"]] == [(150, 210), (75, 105), (38, 53)]


@pytest.mark.parametrize("scale,level", [(0.3, 0), (1, 0), (1.99, 0), (2, 1), (7.9, 2), (8, 3), (1000, 3)])
def test_pick_level_for_scale(scale, level):
    assert streaming.pick_level_for_scale(INDEX, scale) == level


@pytest.mark.parametrize("scale", [0.3, 1, 2, 8, 1000])
def test_pick_level_for_scale_without_overviews(scale):
    assert streaming.pick_level_for_scale(_index(levels=0), scale) == 0


def _bbox(c0, r0, c1, r1, transform=TRANSFORM):
    """the bbox of level-0 pixel-edge columns c0..c1 and rows r0..r1"""
    a, _, c, _, e, f = transform
    return [c + c0 * a, f + r1 * e, c + c1 * a, f + r0 * e]


def _brute_frames(index, level, win):
    c0, r0 = win["col_off"], win["row_off"]
    cols, rows = set(range(c0, c0 + win["width"])), set(range(r0, r0 + win["height"]))
    out = []
    for fr in streaming.level_index(index, level)["frames"]:
        w = fr["window"]
        if cols & set(range(w["col_off"], w["col_off"] + w["width"])) and \
                rows & set(range(w["row_off"], w["row_off"] + w["height"])):
            out.append(fr["frame_id"])
    return out


def test_source_window_and_margin_at_level_0():
    # columns 70.25 .. 130.75, rows 100.5 .. 161: scale 60.5 / 64 < 1
    req = streaming.window_request(INDEX, _bbox(70.25, 100.5, 130.75, 161.0), 64, 64)
    assert req["level"] == 0 and req["scale"] == pytest.approx(60.5 / 64)
    assert req["window"] == {"col_off": 69, "row_off": 99, "width": 132 - 69, "height": 162 - 99}
    assert req["rect"] == (70.25 - 69, 100.5 - 99, 60.5, 60.5)
    assert [f["frame_id"] for f in req["frames"]] == _brute_frames(INDEX, 0, req["window"]) == [6, 7, 11, 12]
    assert (req["out_w"], req["out_h"]) == (64, 64)


def test_window_on_whole_pixels_still_gets_its_margin():
    req = streaming.window_request(INDEX, _bbox(64, 128, 128, 192), 64, 64)
    assert req["level"] == 0
    assert req["window"] == {"col_off": 63, "row_off": 127, "width": 66, "height": 66}
    assert req["rect"] == (1.0, 1.0, 64.0, 64.0)
    assert [f["frame_id"] for f in req["frames"]] == _brute_frames(INDEX, 0, req["window"])
    assert len(req["frames"]) == 9  # the margin reaches into the eight tiles around tile (2, 1)


def test_level_is_picked_from_the_larger_axis_scale():
    # 200 x 80 level-0 pixels as 50 x 40: scales 4 and 2 -> level 2
    req = streaming.window_request(INDEX, _bbox(40, 40, 240, 120), 50, 40)
    assert req["scale"] == 4.0 and req["level"] == 2
    # in level 2 (pixel size 2.0): columns 10 .. 60, rows 10 .. 30
    assert req["window"] == {"col_off": 9, "row_off": 9, "width": 61 - 9, "height": 31 - 9}
    assert req["rect"] == (1.0, 1.0, 50.0, 20.0)
    assert [f["frame_id"] for f in req["frames"]] == _brute_frames(INDEX, 2, req["window"])


@pytest.mark.parametrize("bbox,window", [
    (_bbox(-10.5, 50, 20, 80), {"col_off": 0, "row_off": 49, "width": 21, "height": 32}),        # left
    (_bbox(280, 50, 310.5, 80), {"col_off": 279, "row_off": 49, "width": 21, "height": 32}),     # right
    (_bbox(50, -7.25, 80, 20), {"col_off": 49, "row_off": 0, "width": 32, "height": 21}),        # top
    (_bbox(50, 400, 80, 431), {"col_off": 49, "row_off": 399, "width": 32, "height": 21}),       # bottom
    (_bbox(-5, -5, 305, 425), {"col_off": 0, "row_off": 0, "width": 300, "height": 420}),        # all four
], ids=["left", "right", "top", "bottom", "all"])
def test_clipping_at_the_raster_edges(bbox, window):
    req = streaming.window_request(INDEX, bbox, 400, 500, level=0)
    assert req["window"] == window
    a, _, c, _, e, f = TRANSFORM
    x, y = (bbox[0] - c) / a, (bbox[3] - f) / e
    assert req["rect"] == (x - window["col_off"], y - window["row_off"], (bbox[2] - bbox[0]) / a,
                           (bbox[1] - bbox[3]) / e)
    assert [fr["frame_id"] for fr in req["frames"]] == _brute_frames(INDEX, 0, window)


@pytest.mark.parametrize("bbox", [_bbox(302, 10, 340, 50), _bbox(-50, 10, -2, 50), _bbox(10, 422, 50, 470),
                                  _bbox(10, -60, 50, -1.5), _bbox(1000, 1000, 1100, 1100)])
def test_a_bbox_outside_the_raster_gives_no_frames(bbox):
    req = streaming.window_request(INDEX, bbox, 32, 32)
    assert req["frames"] == [] and req["window"]["width"] == 0 and req["window"]["height"] == 0


def test_a_bbox_within_the_margin_of_the_raster_reads_the_edge_pixels():
    # one pixel to the right of the raster: the margin still touches column 299, the resample will find nothing valid
    req = streaming.window_request(INDEX, _bbox(300.5, 10, 310, 20), 8, 8)
    assert req["window"]["col_off"] == 299 and req["window"]["width"] == 1 and len(req["frames"]) == 1


def test_frames_equal_a_brute_force_intersection_on_every_level():
    for level in range(4):
        for bbox in (_bbox(3.3, 7.7, 290.1, 410.9), _bbox(63.9, 63.9, 64.1, 64.1), _bbox(120, 200, 200, 330)):
            req = streaming.window_request(INDEX, bbox, 16, 16, level=level)
            ids = [f["frame_id"] for f in req["frames"]]
            assert ids == _brute_frames(INDEX, level, req["window"]) and ids == sorted(ids) and ids


def test_output_transform():
    bbox = [110.25, 60.5, 171.0, 150.125]
    req = streaming.window_request(INDEX, bbox, 37, 21)
    assert req["transform"] == [(171.0 - 110.25) / 37, 0.0, 110.25, 0.0, -(150.125 - 60.5) / 21, 150.125]


def test_a_forced_level():
    bbox = _bbox(70.25, 100.5, 130.75, 161.0)
    assert streaming.window_request(INDEX, bbox, 64, 64)["level"] == 0
    req = streaming.window_request(INDEX, bbox, 64, 64, level=2)
    assert req["level"] == 2
    x, y, w, h = 70.25 / 4, 100.5 / 4, 60.5 / 4, 60.5 / 4
    win = {"col_off": math.floor(x) - 1, "row_off": math.floor(y) - 1}
    win["width"] = math.ceil(x + w) + 1 - win["col_off"]
    win["height"] = math.ceil(y + h) + 1 - win["row_off"]
    assert req["window"] == win
    assert req["rect"] == (x - win["col_off"], y - win["row_off"], w, h)
    assert all(f["frame_id"] >= 2000 for f in req["frames"])
    with pytest.raises(LookupError):
        streaming.window_request(INDEX, bbox, 64, 64, level=4)


def test_a_rotated_transform_is_rejected():
    for t in ([0.5, 0.1, 100.0, 0.0, -0.5, 200.0], [0.5, 0.0, 100.0, -0.2, -0.5, 200.0]):
        with pytest.raises(ValueError, match="north-up"):
            streaming.window_request(_index(transform=t), _bbox(10, 10, 50, 50), 8, 8)


def test_bad_sizes_and_boxes_are_rejected():
    with pytest.raises(ValueError):
        streaming.window_request(INDEX, _bbox(10, 10, 50, 50), 0, 8)
    with pytest.raises(ValueError):
        streaming.window_request(INDEX, [120.0, 150.0, 110.0, 160.0], 8, 8)


def test_read_window_names_the_three_modes(tmp_path):
    assert streaming.RESAMPLING_READ == ("nearest", "bilinear", "average")
    assert streaming.RESAMPLING == ("average", "nearest")
    with pytest.raises(ValueError, match="nearest, bilinear, average"):
        streaming.read_window(tmp_path / "never_opened.flac", [0, 0, 1, 1], 4, 4, resampling="cubic")


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra", [
    ["--out-size", "64x64"],                                                   # needs --bbox
    ["--bbox", "0,0,1,1", "--out-size", "64x64", "--mosaic"],
    ["--out-size", "64x64", "--all"],
    ["--bbox", "0,0,1,1", "--out-size", "64x64", "--tile-id", "0"],
    ["--bbox", "0,0,1,1", "--out-size", "64x64", "--center"],
    ["--bbox", "0,0,1,1", "--out-size", "64x64", "--last"],
    ["--bbox", "0,0,1,1", "--out-size", "64x64", "--max-size", "100"],
    ["--bbox", "0,0,1,1", "--out-size", "64"],
    ["--bbox", "0,0,1,1", "--out-size", "0x5"],
    ["--bbox", "0,0,1,1", "--out-size", "ax3"],
    ["--bbox", "0,0,1,1", "--out-size", "64x64", "--resampling", "cubic"],
    ["--bbox", "0,0,1,1", "--resampling", "nearest"],                          # without --out-size
    ["--bbox", "0,0,1,1", "--fill", "5"],
    ["--bbox", "0,0,1,1", "--mosaic", "--resampling", "average"],
], ids=lambda e: " ".join(e))
def test_out_size_option_conflicts_exit_1_before_anything_is_read(tmp_path, extra):
    out = tmp_path / "o.tif"
    # the file does not exist: an option conflict must be reported before the missing file is
    r = runner.invoke(app, ["extract-streaming", str(tmp_path / "missing.flac"), "-o", str(out), *extra])
    assert r.exit_code == 1, r.output
    assert "missing.flac" not in r.output and "No such file" not in r.output
    assert "--out-size" in r.output or "--resampling" in r.output
    assert not out.exists()


def test_out_size_with_level_passes_the_option_checks(tmp_path):
    r = runner.invoke(app, ["extract-streaming", str(tmp_path / "missing.flac"), "-o", str(tmp_path / "o.tif"),
                            "--bbox", "0,0,1,1", "--out-size", "8x8", "--level", "1", "--resampling", "bilinear",
                            "--fill", "-1"])
    assert r.exit_code == 1 and "--out-size" not in r.output  # it got as far as opening the file
