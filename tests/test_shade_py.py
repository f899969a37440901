"""The pure Python side of the hillshade: render.light_vector, render.shade_table, render.parse_hillshade and
streaming.window_request's margin.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

from flac_raster_amd import render as rn
from flac_raster_amd import streaming as S


def test_light_vector_is_the_unit_vector_towards_the_light():
    assert rn.light_vector() == rn.light_vector(315.0, 45.0)
    lx, ly, lz = rn.light_vector(315, 45)
    assert lx < 0 < ly and abs(lx + 0.5) < 1e-15 and abs(ly - 0.5) < 1e-15 and abs(lz - math.sqrt(0.5)) < 1e-15
    assert rn.light_vector(0, 90)[2] == 1.0 and abs(rn.light_vector(123, 90)[0]) < 1e-16
    e = rn.light_vector(90, 30)
    assert abs(e[0] - math.cos(math.radians(30))) < 1e-15 and abs(e[1]) < 1e-15 and abs(e[2] - 0.5) < 1e-15
    for az, alt in ((0, 10), (200, 60), (-45, 45), (720, 1)):
        assert abs(sum(v * v for v in rn.light_vector(az, alt)) - 1.0) < 1e-15
    for az, alt in ((0, 0), (0, -5), (0, 90.5), (float("nan"), 45), (float("inf"), 45), (0, float("nan"))):
        with pytest.raises(ValueError):
            rn.light_vector(az, alt)


def test_shade_table():
    assert (rn.shade_table(0) == 255).all() and (rn.shade_table(0.0) == 255).all()
    t = rn.shade_table(1.0)
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert t[0] == 0 and t[255] == 255  # 255 / 512 rounds to 0, 255 * 511 / 512 to 255
    for s in (1.0, 0.5, 0.25, Fraction(1, 3)):
        t = rn.shade_table(s)
        assert (np.diff(t.astype(int)) >= 0).all()
        f = Fraction(s) if isinstance(s, Fraction) else Fraction(repr(s))
        for k in (0, 1, 127, 128, 255):
            exact = 255 * (1 - f + f * Fraction(2 * k + 1, 512))
            assert abs(int(t[k]) - exact) <= Fraction(1, 2)
    # ties go to the even value.  m[k] = 255 - 255 s (511 - 2k) / 512; with s = 256 / 765 that is 255 - (511 - 2k) / 6,
    # a half-integer at k = 254 - 3j: 254.5, 253.5, 252.5, 251.5
    t = rn.shade_table(Fraction(256, 765))
    assert [int(t[k]) for k in (254, 251, 248, 245)] == [254, 254, 252, 252]
    for bad in (-0.1, 1.5, float("nan"), "1", None):
        with pytest.raises(ValueError):
            rn.shade_table(bad)


def test_parse_hillshade():
    assert rn.parse_hillshade("315,45") == (315.0, 45.0)
    assert rn.parse_hillshade("0,90") == (0.0, 90.0)
    assert rn.parse_hillshade("-30.5, 0.25") == (-30.5, 0.25)
    for bad in ("", "315", "315,45,1", "a,b", "315,0", "315,-1", "315,90.01", "nan,45", "inf,45", "315,nan"):
        with pytest.raises(ValueError):
            rn.parse_hillshade(bad)


def _index(W=1000, H=800, tile=100):
    frames = [{"window": {"col_off": c, "row_off": r, "width": min(tile, W - c), "height": min(tile, H - r)},
               "byte_offset": 0, "byte_size": 1}
              for r in range(0, H, tile) for c in range(0, W, tile)]
    return {"transform": [2.0, 0.0, 100.0, 0.0, -2.0, 5000.0], "width": W, "height": H, "frames": frames}


BOXES = [((100.0, 3400.0, 2100.0, 5000.0), 500, 400), ((500.0, 4000.0, 900.0, 4400.0), 256, 256),
         ((101.5, 4500.25, 350.75, 4800.0), 77, 91), ((0.0, 4000.0, 300.0, 5200.0), 64, 64),
         ((5000.0, 4000.0, 5300.0, 4400.0), 16, 16)]


def test_margin_zero_is_the_call_without_the_keyword():
    ix = _index()
    for bbox, w, h in BOXES:
        assert S.window_request(ix, bbox, w, h, margin=0) == S.window_request(ix, bbox, w, h)
    with pytest.raises(ValueError):
        S.window_request(ix, BOXES[0][0], 8, 8, margin=-1)


def test_margin_one_covers_the_widened_rectangle_clipped_to_the_raster():
    ix = _index()
    for bbox, w, h in BOXES:
        a, b = S.window_request(ix, bbox, w, h), S.window_request(ix, bbox, w, h, margin=1)
        assert (a["level"], a["transform"], a["out_w"], a["out_h"]) == (b["level"], b["transform"], b["out_w"],
                                                                       b["out_h"])
        wa, wb = a["window"], b["window"]
        if wb["width"] == 0:
            assert wa["width"] == 0
            continue
        # the same rectangle in raster coordinates
        assert a["rect"][2:] == b["rect"][2:]
        x, y = b["rect"][0] + wb["col_off"], b["rect"][1] + wb["row_off"]
        if wa["width"]:
            assert (x, y) == (a["rect"][0] + wa["col_off"], a["rect"][1] + wa["row_off"])
        sx, sy = b["rect"][2] / w, b["rect"][3] / h
        # one output step beyond each side, and a source pixel more, unless the raster ends first
        assert wb["col_off"] <= max(math.floor(x - sx) - 1, 0)
        assert wb["row_off"] <= max(math.floor(y - sy) - 1, 0)
        assert wb["col_off"] + wb["width"] >= min(math.ceil(x + b["rect"][2] + sx) + 1, 1000)
        assert wb["row_off"] + wb["height"] >= min(math.ceil(y + b["rect"][3] + sy) + 1, 800)
        assert wb["col_off"] >= 0 and wb["row_off"] >= 0
        assert wb["col_off"] + wb["width"] <= 1000 and wb["row_off"] + wb["height"] <= 800
        if wa["width"]:
            assert wb["col_off"] <= wa["col_off"] and wb["width"] >= wa["width"]
        for fr in a["frames"]:
            assert fr in b["frames"]
    # the widening shows: a box well inside the raster gets a larger window
    a, b = S.window_request(ix, BOXES[1][0], 16, 16), S.window_request(ix, BOXES[1][0], 16, 16, margin=1)
    assert b["window"]["width"] > a["window"]["width"] and b["window"]["height"] > a["window"]["height"]


def test_cli_rejects_every_broken_rule_before_the_file_is_opened(tmp_path):
    from typer.testing import CliRunner
    from flac_raster_amd.cli import app
    runner = CliRunner()
    base = ["render", str(tmp_path / "missing.flac"), "--max-size", "64", "-o", str(tmp_path / "o.png")]
    for extra, word in ((["--z-factor", "2"], "--z-factor needs --hillshade"),
                        (["--shade-strength", "0.5"], "--shade-strength needs --hillshade"),
                        (["--shade-only"], "--shade-only needs --hillshade"),
                        (["--hillshade", "315,0"], "altitude"), (["--hillshade", "315,91"], "altitude"),
                        (["--hillshade", "315"], "AZ,ALT"), (["--hillshade", "1,2,3"], "AZ,ALT"),
                        (["--hillshade", "nan,45"], "azimuth"),
                        (["--hillshade", "--z-factor", "0"], "--z-factor"),
                        (["--hillshade", "--z-factor", "inf"], "--z-factor"),
                        (["--hillshade", "--shade-strength", "1.5"], "--shade-strength"),
                        (["--hillshade", "--shade-strength", "-0.1"], "--shade-strength"),
                        (["--hillshade", "--shade-only", "--colormap", "heat"], "--shade-only"),
                        (["--hillshade", "--shade-only", "--stretch", "minmax"], "--shade-only"),
                        (["--hillshade", "--shade-only", "--stats-from", "window"], "--shade-only")):
        r = runner.invoke(app, base + extra)
        assert r.exit_code == 1 and word in r.output and "missing.flac" not in r.output, (extra, r.output)
    # with every rule kept the command gets as far as the file, which is not there
    for extra in (["--hillshade"], ["--hillshade", "300,30", "--z-factor", "2", "--shade-strength", "0.5"],
                  ["--hillshade", "--shade-only"], []):
        r = runner.invoke(app, base + extra)
        assert r.exit_code == 1 and "missing.flac" in r.output, (extra, r.output)


def test_render_window_rejects_shade_options_without_hillshade():
    for kw in ({"z_factor": 2.0}, {"shade_strength": 0.5}, {"shade_only": True}):
        with pytest.raises(ValueError):
            S.render_window("/nonexistent/file.flac", (0, 0, 1, 1), 4, 4, **kw)
    for kw in ({"hillshade": (315, 0)}, {"hillshade": (315, 45), "z_factor": 0.0},
               {"hillshade": (315, 45), "shade_strength": 2.0}):
        with pytest.raises(ValueError):
            S.render_window("/nonexistent/file.flac", (0, 0, 1, 1), 4, 4, **kw)
