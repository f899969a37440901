"""The pure host side of the render: render.stretch_limits and render.build_lut, the colormap files, png.write_png,
geotiff.write's alpha keyword (and its absence: byte-identical files), the ctypes surface, and the argument rules of the
render command.  No GPU."""
import ctypes
import struct
import subprocess
import zlib
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, geotiff, png, render
from flac_raster_amd.cli import app
from tests import stats_ref as S
from tests.render_cases import read_png as _read_png

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
runner = CliRunner()


# ------------------------------------------------------------------------------------------------ stretch
def _per_value_stats(values):
    """the statistics entry of an integer band with a bin per value"""
    v = np.asarray(values, dtype=np.int64)
    lo, hi = int(v.min()), int(v.max())
    return {"valid": len(v), "nodata_count": 0, "nan": 0, "min": lo, "max": hi, "mean": float(v.mean()),
            "std": float(v.std()),
            "histogram": {"lo": lo, "hi": hi + 1, "counts": np.bincount(v - lo, minlength=hi - lo + 1).tolist(),
                          "below": 0, "above": 0, "per_value": True}}


def test_stretch_limits_every_spec():
    rng = np.random.default_rng(3)
    v = rng.integers(-300, 900, size=5000)
    st = _per_value_stats(v)
    assert render.stretch_limits(st, "minmax") == (float(v.min()), float(v.max()))
    for p, q in ((2, 98), (0, 100), (25, 75), (0.5, 99.5)):
        want = (float(S.percentile_sorted(v.tolist(), Fraction(p))), float(S.percentile_sorted(v.tolist(), Fraction(q))))
        assert render.stretch_limits(st, f"percentile:{p},{q}") == want
    assert render.stretch_limits(st) == render.stretch_limits(st, "percentile:2,98")
    m, s = st["mean"], st["std"]
    assert render.stretch_limits(st, "stddev:1.5") == (m - 1.5 * s, m + 1.5 * s)
    assert render.stretch_limits(st, "stddev:100") == (float(v.min()), float(v.max()))  # clipped to [min, max]
    assert render.stretch_limits(None, "range:-5,12.5") == (-5.0, 12.5)
    assert render.stretch_limits(st, "range:-5,12.5") == (-5.0, 12.5)


def test_stretch_limits_degenerate_results():
    flat = _per_value_stats([7] * 40)
    for spec in ("minmax", "percentile:2,98", "stddev:2"):
        assert render.stretch_limits(flat, spec) == (7.0, 8.0)
    assert render.stretch_limits(None, "range:3,3") == (3.0, 4.0)
    assert render.stretch_limits(None, "range:3,1") == (3.0, 4.0)
    empty = {"valid": 0, "nodata_count": 12, "nan": 0, "min": None, "max": None, "mean": None, "std": None,
             "histogram": None}
    for spec in ("minmax", "percentile:2,98", "stddev:2"):
        assert render.stretch_limits(empty, spec) == (0.0, 1.0)
    with pytest.raises(ValueError, match="needs the band's statistics"):
        render.stretch_limits(None, "minmax")
    # a float band with infinities: minmax falls back to the histogram's finite range, stddev has no finite answer
    inf = {"valid": 10, "min": float("-inf"), "max": float("inf"), "mean": float("nan"), "std": float("nan"),
           "histogram": {"lo": -2.5, "hi": 4.0, "counts": [5, 3], "below": 1, "above": 1, "per_value": False}}
    assert render.stretch_limits(inf, "minmax") == (-2.5, 4.0)
    with pytest.raises(ValueError, match="not finite"):
        render.stretch_limits(inf, "stddev:2")


@pytest.mark.parametrize("spec", ["", "min", "minmax:1", "percentile", "percentile:2", "percentile:98,2",
                                  "percentile:-1,50", "percentile:2,101", "percentile:a,b", "stddev:0", "stddev:-1",
                                  "stddev:1,2", "range:1", "range:1,2,3", "range:nan,1", "range:0,inf", "gamma:2"])
def test_stretch_specs_rejected(spec):
    with pytest.raises(ValueError, match="--stretch"):
        render.parse_stretch(spec)


# ------------------------------------------------------------------------------------------------ LUT
def test_gray_is_the_identity_ramp():
    lut = render.build_lut("gray", 256)
    assert lut.dtype == np.uint8 and lut.shape == (256, 4)
    assert np.array_equal(lut[:, 0], np.arange(256)) and np.array_equal(lut[:, 1], lut[:, 0])
    assert np.array_equal(lut[:, 2], lut[:, 0]) and (lut[:, 3] == 255).all()
    assert np.array_equal(render.build_lut("gray_r", 256)[:, 0], np.arange(255, -1, -1))


@pytest.mark.parametrize("name", sorted(render.COLORMAPS))
@pytest.mark.parametrize("n", [1, 2, 256, 4096])
def test_named_ramps_end_at_their_end_control_points(name, n):
    pts = render.check_colormap(render.COLORMAPS[name])
    lut = render.build_lut(name, n).astype(int)
    # entry 0 is the ramp at 1 / 2n, the last at 1 - 1 / 2n: half a step from the end, over which a piecewise-linear
    # ramp moves by at most its steepest segment's slope times 1 / 2n; and the rounding's half
    for entry, p in ((lut[0], pts[0]), (lut[-1], pts[-1])):
        for c in range(3):
            slope = max(abs(b[1 + c] - a[1 + c]) / float(b[0] - a[0]) for a, b in zip(pts, pts[1:]))
            assert abs(entry[c] - p[1 + c]) <= slope / (2 * n) + 0.5, (entry, p)
    assert (lut[:, 3] == 255).all()
    # exact rational interpolation, rounded half up, at every entry
    for i in (0, n // 3, n // 2, n - 1):
        t = Fraction(2 * i + 1, 2 * n)
        k = max(j for j, p in enumerate(pts[:-1]) if p[0] <= t)
        f = (t - pts[k][0]) / (pts[k + 1][0] - pts[k][0])
        want = [int((pts[k][c] + (pts[k + 1][c] - pts[k][c]) * f + Fraction(1, 2)) // 1) for c in (1, 2, 3)]
        assert lut[i, :3].tolist() == want


def test_gamma_and_log_are_monotone_and_bend_the_ramp():
    lin = render.build_lut("gray", 4096)[:, 0].astype(int)
    for kw in ({"gamma": 2.2}, {"gamma": 0.5}, {"transfer": "log"}):
        g = render.build_lut("gray", 4096, **kw)[:, 0].astype(int)
        assert (np.diff(g) >= 0).all() and g[0] <= 40 and g[-1] == 255
        brighter = kw != {"gamma": 0.5}
        assert (g >= lin).all() if brighter else (g <= lin).all()
    assert render.default_lut_size() == 256 and render.default_lut_size(2.2) == 4096
    assert render.default_lut_size(1.0, "log") == 4096
    # entry i of a gamma ramp: the grey of t ** (1 / gamma), from the double the expression gives
    g = render.build_lut("gray", 1000, gamma=2.2)
    for i in (0, 17, 500, 999):
        u = Fraction(float(Fraction(2 * i + 1, 2000)) ** (1.0 / 2.2))
        assert g[i, 0] == int((255 * u + Fraction(1, 2)) // 1)
    for bad in ({"n": 0}, {"n": 4097}, {"gamma": 0}, {"gamma": float("inf")}, {"transfer": "sqrt"},
                {"colormap": "viridis"}):
        with pytest.raises(ValueError):
            render.build_lut(**{"colormap": "gray", "n": 16, **bad})


def test_colormap_file_round_trip_and_rejections(tmp_path):
    pts = [(0, 1, 2, 3), ("0.25", 10, 20, 30, 40), (0.5, 0, 255, 0), (1, 255, 254, 253, 0)]
    f = tmp_path / "ramp.txt"
    f.write_text("# a ramp\n\n" + render.format_colormap(pts) + "   # trailing comment\n")
    got = render.load_colormap(f)
    assert got == [(Fraction(0), 1, 2, 3, 255), (Fraction(1, 4), 10, 20, 30, 40), (Fraction(1, 2), 0, 255, 0, 255),
                   (Fraction(1), 255, 254, 253, 0)]
    assert np.array_equal(render.build_lut(got, 64), render.build_lut(pts, 64))
    # the last entry lies 63/64 of the way from (0, 255, 0, 255) to (255, 254, 253, 0): alpha is interpolated too
    assert render.build_lut(got, 64)[-1].tolist() == [251, 254, 249, 4]
    for text, msg in (("0 0 0 0\n", "at least two"), ("0 0 0 0\n0.5 1 1\n", "t r g b"),
                      ("0 0 0 0\n1.5 1 1 1\n", r"\[0, 1\]"), ("0.5 0 0 0\n0.5 1 1 1\n", "ascend"),
                      ("0.5 0 0 0\n0.25 1 1 1\n", "ascend"), ("0 0 0 0\n1 256 0 0\n", "0..255"),
                      ("0 0 0 0\n1 1.5 0 0\n", "0..255"), ("0 0 0 0\nx 1 1 1\n", "must be a number"),
                      ("0 0 0 0\n1 -1 0 0\n", "0..255")):
        f.write_text(text)
        with pytest.raises(ValueError, match=msg):
            render.load_colormap(f)


def test_max_size_shape():
    assert render.max_size_shape(300.0, 260.0, 100) == (100, 87)
    assert render.max_size_shape(260.0, 300.0, 100) == (87, 100)
    assert render.max_size_shape(1000.0, 1.0, 64) == (64, 1)
    assert render.max_size_shape(2.0, 2.0, 1) == (1, 1)
    assert render.max_size_shape(3.0, 1.0, 3) == (3, 1) and render.max_size_shape(2.0, 1.0, 5) == (5, 3)  # half up
    with pytest.raises(ValueError):
        render.max_size_shape(1.0, 1.0, 0)


# ------------------------------------------------------------------------------------------------ PNG
@pytest.mark.parametrize("c", [1, 2, 4])
def test_write_png_round_trip(tmp_path, c):
    rng = np.random.default_rng(c)
    for h, w in ((1, 1), (3, 130), (40, 9)):
        a = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
        png.write_png(tmp_path / "a.png", a)
        assert np.array_equal(_read_png((tmp_path / "a.png").read_bytes()), a)
    png.write_png(tmp_path / "g.png", a[:, :, 0] if c == 1 else a)
    assert _read_png((tmp_path / "g.png").read_bytes()).shape == a.shape
    for bad in (a.astype(np.uint16), np.zeros((2, 2, 3), np.uint8), np.zeros((0, 2, 1), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            png.write_png(tmp_path / "bad.png", bad)


def test_write_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    for c, mode in ((1, "L"), (2, "LA"), (4, "RGBA")):
        a = rng.integers(0, 256, size=(13, 21, c), dtype=np.uint8)
        png.write_png(tmp_path / "p.png", a)
        with Image.open(tmp_path / "p.png") as im:
            assert im.mode == mode and np.array_equal(np.asarray(im).reshape(13, 21, c), a)


# ------------------------------------------------------------------------------------------------ GeoTIFF
def _golden_array():
    return (np.arange(4 * 5 * 7, dtype=np.uint32).reshape(4, 5, 7) * 37 % 251).astype(np.uint8)


def test_geotiff_write_without_the_keyword_is_byte_identical(tmp_path):
    """tests/golden/render_geotiff_4band_parent.tif was written by this call before the keyword existed"""
    tr = geotiff.Affine(0.5, 0.0, -106.0, 0.0, -0.25, 41.0)
    geotiff.write(tmp_path / "a.tif", _golden_array(), transform=tr, epsg=4326)
    want = (GOLDEN / "render_geotiff_4band_parent.tif").read_bytes()
    assert (tmp_path / "a.tif").read_bytes() == want
    geotiff.write(tmp_path / "b.tif", _golden_array(), transform=tr, epsg=4326, alpha=False)
    assert (tmp_path / "b.tif").read_bytes() == want


def _tags(path):
    """tag -> values of a little-endian classic TIFF's first directory (SHORT and LONG entries)"""
    d = Path(path).read_bytes()
    assert d[:4] == b"II*\x00"
    off = struct.unpack("<I", d[4:8])[0]
    out = {}
    for i in range(struct.unpack("<H", d[off:off + 2])[0]):
        tag, typ, cnt, val = struct.unpack("<HHI4s", d[off + 2 + 12 * i:off + 14 + 12 * i])
        if typ in (3, 4):
            size, fmt = (2, "H") if typ == 3 else (4, "I")
            raw = val[:cnt * size] if cnt * size <= 4 else d[struct.unpack("<I", val)[0]:][:cnt * size]
            out[tag] = list(struct.unpack("<" + fmt * cnt, raw))
    return out


def test_geotiff_write_alpha_keyword(tmp_path):
    a = _golden_array()
    tr = geotiff.Affine(0.5, 0.0, -106.0, 0.0, -0.25, 41.0)
    geotiff.write(tmp_path / "rgba.tif", a, transform=tr, epsg=4326, alpha=True)
    t = _tags(tmp_path / "rgba.tif")
    assert t[262] == [2] and t[277] == [4] and t[338] == [2]          # RGB + unassociated alpha
    geotiff.write(tmp_path / "la.tif", a[:2], transform=tr, epsg=4326, alpha=True)
    t = _tags(tmp_path / "la.tif")
    assert t[262] == [1] and t[277] == [2] and t[338] == [2]          # grey + unassociated alpha
    geotiff.write(tmp_path / "plain.tif", a, transform=tr, epsg=4326)
    t = _tags(tmp_path / "plain.tif")
    assert t[262] == [1] and t[338] == [0, 0, 0]
    for name, bands in (("rgba.tif", 4), ("la.tif", 2)):
        r = geotiff.read(tmp_path / name)
        assert np.array_equal(r.data, a[:bands]) and tuple(r.transform)[:6] == tuple(tr)[:6]
    with pytest.raises(ValueError, match="at least two bands"):
        geotiff.write(tmp_path / "one.tif", a[0], alpha=True)


# ------------------------------------------------------------------------------------------------ ABI surface
def test_render_prototypes_and_structure_match_the_header(tmp_path):
    hdr = ROOT / "include" / "flac_raster_amd.h"
    proto = ("int (*p%d)(frs_ctx *, const frs_raster_desc *, const void *, const frs_raster_desc *, void *, "
             "const frs_window_map *, int32_t, const double *, const frs_render_params *) = %s;\n")
    (tmp_path / "t.c").write_text(f'#include "{hdr}"\n' + "".join(
        proto % (i, name) for i, name in enumerate(("frs_render_window_device", "frs_render_window"))))
    subprocess.run(["gcc", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")], check=True)
    (tmp_path / "v.c").write_text(
        f'#include "{hdr}"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){{printf("%zu %zu %zu %zu %zu %zu\\n", '
        "sizeof(frs_render_params), offsetof(frs_render_params, hi), offsetof(frs_render_params, lut), "
        "offsetof(frs_render_params, n), offsetof(frs_render_params, nodata_rgba), "
        "offsetof(frs_render_params, channels));return 0;}\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "v"), str(tmp_path / "v.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "v")], capture_output=True, text=True, check=True).stdout.split()]
    P = _native.RenderParams
    assert out == [ctypes.sizeof(P), P.hi.offset, P.lut.offset, P.n.offset, P.nodata_rgba.offset, P.channels.offset]
    assert {"frs_render_window_device", "frs_render_window"} <= set(_native.EXPORTS)
    assert _native.RENDER_MAX_LUT == render.MAX_LUT == 4096


def test_library_exports_the_render_entry_points():
    L = _native.load_library()
    rdp, vp = ctypes.POINTER(_native.RasterDesc), ctypes.c_void_p
    want = [vp, rdp, vp, rdp, vp, ctypes.POINTER(_native.WindowMap), ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(_native.RenderParams)]
    for name in ("frs_render_window_device", "frs_render_window"):
        fn = getattr(L, name)
        assert fn.argtypes == want and fn.restype is ctypes.c_int32
    assert L.frs_abi_version() == 1


def test_pack_rgba():
    assert _native.pack_rgba((1, 2, 3, 4)) == 0x04030201 and _native.pack_rgba(0) == 0
    assert _native.pack_rgba(0xFFFFFFFF) == 0xFFFFFFFF
    for bad in ((256, 0, 0, 0), (0, 0, 0, -1), -1, 1 << 32):
        with pytest.raises(ValueError):
            _native.pack_rgba(bad)


# ------------------------------------------------------------------------------------------------ CLI rejections
def test_render_argument_rules_are_checked_before_anything_is_read(tmp_path):
    f, out = str(tmp_path / "missing.flac"), str(tmp_path / "o.png")
    ok = ["render", f, "-o", out, "--out-size", "8x8"]
    bad_ramp = tmp_path / "bad.txt"
    bad_ramp.write_text("0 0 0 0\n")
    exists = tmp_path / "exists.png"
    exists.write_bytes(b"x")
    for args, msg in (
            (["render", f, "-o", out], "exactly one of --out-size WxH and --max-size N"),
            (ok + ["--max-size", "8"], "exactly one of --out-size WxH and --max-size N"),
            (["render", f, "-o", out, "--out-size", "8"], "--out-size must be WxH"),
            (["render", f, "-o", out, "--out-size", "0x8"], "--out-size must be WxH"),
            (["render", f, "-o", out, "--max-size", "0"], "--max-size must be >= 1"),
            (["render", f, "-o", str(tmp_path / "o.jpg"), "--out-size", "8x8"], "must be .png or .tif"),
            (ok + ["--channels", "3"], "--channels must be 1, 2 or 4"),
            (ok + ["--stats-from", "level"], "--stats-from must be one of"),
            (ok + ["--resampling", "cubic"], "--resampling must be one of"),
            (ok + ["--transfer", "sqrt"], "--transfer must be one of"),
            (ok + ["--gamma", "0"], "--gamma must be"),
            (ok + ["--stretch", "percentile:98,2"], "--stretch percentile"),
            (ok + ["--stretch", "sigma:2"], "--stretch must be"),
            (ok + ["--nodata", "abc"], "--nodata must be a number or 'none'"),
            (ok + ["--bbox", "1,2,3"], "Invalid bbox format"),
            (ok + ["--bbox", "3,0,1,2"], "Invalid bbox format"),
            (ok + ["--colormap", "viridis"], "--colormap must be one of"),
            (ok + ["--colormap", str(bad_ramp)], "at least two"),
            (["render", f, "-o", str(exists), "--out-size", "8x8"], "use --force"),
    ):
        r = runner.invoke(app, args)
        assert r.exit_code == 1 and msg in r.output, (args, r.output)
        assert "missing.flac" not in r.output.replace(f, ""), r.output  # the input was never opened
    assert not Path(out).exists() and exists.read_bytes() == b"x"
    # with every rule met the command reaches the input
    r = runner.invoke(app, ok + ["--stretch", "range:0,1", "--colormap", "heat", "--channels", "2"])
    assert r.exit_code == 1 and "Invalid bbox" not in r.output and "must be" not in r.output
