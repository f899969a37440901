"""Host side of the multi-band streaming format: the pure index functions (bands_of, band_index, parse_bands,
select_bands) on hand-built index dicts, the command-line rules of --bands / --band, each checked before a file is
opened, and the composite's C-ABI surface against the header.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, geotiff, streaming
from flac_raster_amd.cli import app

runner = CliRunner()
ROOT = Path(__file__).resolve().parents[1]


def _frames(id0, off0, tile=64, width=150, height=130, a=0.5, e=-0.25, c=-106.0, f=41.0):
    out, off = [], off0
    k = id0
    for row in range(0, height, tile):
        for col in range(0, width, tile):
            w, h = min(tile, width - col), min(tile, height - row)
            x0, y1 = c + col * a, f + row * e
            out.append({"frame_id": k, "bbox": [x0, y1 + h * e, x0 + w * a, y1],
                        "window": {"col_off": col, "row_off": row, "width": w, "height": h},
                        "byte_offset": off, "byte_size": 100 + k})
            off += 100 + k
            k += 1
    return out, k, off


def _stats(v):
    return {"valid": v, "nodata_count": 1, "nan": 0, "min": 0, "max": v, "mean": 1.5, "std": 0.5, "histogram": None}


def _index(bands=(1, 2, 3), overviews=True, stats=True, nodata=-7):
    """an index as create_streaming_bands_array lays it out: 150 x 130, tile 64, one overview level of 75 x 65"""
    tr = [0.5, 0.0, -106.0, 0.0, -0.25, 41.0]
    k, off = 0, 0
    index, entries = {}, []
    for b in bands:
        fr0, k, off = _frames(k, off)
        fr1, k, off = _frames(k, off, width=75, height=65, a=1.0, e=-0.5)
        if b == 1:
            e = index
            index.update({"crs": "EPSG:4326", "transform": tr, "width": 150, "height": 130, "tile_size": 64,
                          "frames": fr0})
            if nodata is not None:
                index["nodata"] = nodata
        else:
            e = {"band": b, "frames": fr0}
            entries.append(e)
        if overviews:
            e["overviews"] = {"resampling": "average", "levels": [
                {"level": 1, "factor": 2, "width": 75, "height": 65, "transform": [1.0, 0.0, -106.0, 0.0, -0.5, 41.0],
                 "frames": fr1}]}
        if stats:
            e["statistics"] = _stats(1000 * b)
    if len(bands) > 1:
        index["bands"] = {"count": 4, "entries": entries}
    return index


# ------------------------------------------------------------------------------------------------ pure index functions
def test_bands_of():
    assert streaming.bands_of(_index((1,))) == [1]
    assert streaming.bands_of(_index((1, 2, 3))) == [1, 2, 3]
    assert streaming.bands_of(_index((1, 4, 2))) == [1, 4, 2]  # file order
    assert streaming.bands_of({"frames": []}) == [1]


def test_band_index_of_band_1_is_the_index_without_its_bands_key():
    index = _index()
    before = repr(index)
    b1 = streaming.band_index(index, 1)
    assert "bands" not in b1 and b1 == {k: v for k, v in index.items() if k != "bands"}
    assert list(b1) == ["crs", "transform", "width", "height", "tile_size", "frames", "nodata", "overviews",
                        "statistics"]
    assert b1["overviews"] is index["overviews"] and b1["statistics"] == _stats(1000) and b1["nodata"] == -7
    assert repr(index) == before  # pure
    single = _index((1,))
    assert streaming.band_index(single, 1) == single and streaming.band_index(single) == single


def test_band_index_of_another_band():
    index = _index()
    before = repr(index)
    b3 = streaming.band_index(index, 3)
    e3 = index["bands"]["entries"][1]
    assert list(b3) == ["crs", "transform", "width", "height", "tile_size", "frames", "nodata", "overviews",
                        "statistics"]
    assert b3["frames"] is e3["frames"] and b3["overviews"] is e3["overviews"]
    assert (b3["crs"], b3["transform"], b3["width"], b3["height"], b3["tile_size"], b3["nodata"]) == \
        ("EPSG:4326", index["transform"], 150, 130, 64, -7)
    assert streaming.index_statistics(b3)["valid"] == 3000 and streaming.index_nodata(b3) == -7.0
    assert repr(index) == before
    # the optional keys are present exactly when the file has them
    plain = streaming.band_index(_index(overviews=False, stats=False, nodata=None), 2)
    assert list(plain) == ["crs", "transform", "width", "height", "tile_size", "frames"]


def test_band_index_lookup_error_names_the_bands_present():
    with pytest.raises(LookupError, match=r"band 4 not in this file \(bands present: \[1, 2, 3\]\)"):
        streaming.band_index(_index(), 4)
    with pytest.raises(LookupError, match=r"band 2 not in this file \(bands present: \[1\]\)"):
        streaming.band_index(_index((1,)), 2)


def test_the_selection_functions_work_on_a_bands_dict():
    index = _index()
    b2 = streaming.band_index(index, 2)
    assert streaming.overview_levels(b2) == [0, 1]
    l1 = streaming.level_index(b2, 1)
    assert l1["frames"] is index["bands"]["entries"][0]["overviews"]["levels"][0]["frames"] and l1["nodata"] == -7
    bbox = [-106.0 + 10 * 0.5, 41.0 - 100 * 0.25, -106.0 + 100 * 0.5, 41.0 - 20 * 0.25]
    req1 = streaming.window_request(streaming.band_index(index, 1), bbox, 45, 40)
    req2 = streaming.window_request(b2, bbox, 45, 40)
    assert req2["level"] == req1["level"] == 1 and req2["window"] == req1["window"] and req2["rect"] == req1["rect"]
    # the same tiles of the level, the other band's entries: ids and offsets run on through the file
    assert [f["window"] for f in req2["frames"]] == [f["window"] for f in req1["frames"]]
    assert all(f2["frame_id"] > f1["frame_id"] and f2["byte_offset"] > f1["byte_offset"]
               for f1, f2 in zip(req1["frames"], req2["frames"]))
    req0 = streaming.window_request(b2, bbox, 90, 80, level=0)
    assert req0["frames"] and all(f in b2["frames"] for f in req0["frames"])
    hits = streaming.intersecting(b2, bbox)
    assert hits and streaming.select_frame(b2, bbox=bbox) is hits[0]
    assert streaming.select_frame(b2, tile_id=b2["frames"][1]["frame_id"]) is b2["frames"][1]
    assert streaming.pick_level(b2, 150, 130, 80) == 1


def test_parse_and_select_bands():
    assert streaming.parse_bands("all") == "all" and streaming.parse_bands(" ALL ") == "all"
    assert streaming.parse_bands("1,2,3") == [1, 2, 3] and streaming.parse_bands("3, 1") == [3, 1]
    for bad in ("", "1,,2", "a", "1,b", "1.5", "-1", "1;2", "0", "1,0", "2,2", "1,2,1"):
        with pytest.raises(ValueError):
            streaming.parse_bands(bad)
    assert streaming.select_bands("all", 4) == [1, 2, 3, 4]
    assert streaming.select_bands([3, 1], 4) == [3, 1] and streaming.select_bands("1,4", 4) == [1, 4]
    with pytest.raises(ValueError, match="band 1 must be among"):
        streaming.select_bands([2, 3], 4)
    with pytest.raises(ValueError, match="band 5 is not one of the source's 4"):
        streaming.select_bands([1, 5], 4)
    with pytest.raises(ValueError, match="named twice"):
        streaming.select_bands([1, 2, 2], 4)
    with pytest.raises(ValueError):
        streaming.select_bands([1, 0], 4)
    with pytest.raises(ValueError):
        streaming.select_bands([1, 2.5], 4)


def test_decode_into_window_checks_its_plane_before_any_gpu_work():
    with pytest.raises(ValueError, match="plane"):
        streaming.decode_into_window([b""], [{}], (0, 0), (4, 4), ctx=object(), plane=2, planes=2)
    with pytest.raises(ValueError, match="plane"):
        streaming.decode_into_window([b""], [{}], (0, 0), (4, 4), ctx=object(), plane=-1)


# ------------------------------------------------------------------------------------------------ CLI rules
def _rejected(args, msg, never):
    r = runner.invoke(app, args)
    assert r.exit_code == 1 and msg in r.output, (args, r.output)
    assert Path(never).name not in r.output.replace(never, ""), r.output  # the input was never opened


def test_create_streaming_bands_rules_are_checked_before_any_file_is_opened(tmp_path):
    missing = str(tmp_path / "missing.tif")
    ok = ["create-streaming", missing]
    for value, msg in (("2,3", "--bands must name band 1"), ("1,2,2", "named twice"), ("1,0", "band numbers start at 1"),
                       ("abc", "--bands must be 'all' or band numbers"), ("1,,2", "--bands must be 'all' or band numbers"),
                       ("1.5", "--bands must be 'all' or band numbers"), ("", "--bands must be 'all' or band numbers")):
        _rejected(ok + ["--bands", value], msg, missing)
    for extra in (["--gpus", "2"], ["--distributed"]):
        _rejected(ok + ["--bands", "1,2"] + extra, "--bands runs on one GPU", missing)
        _rejected(ok + ["--bands", "all"] + extra, "--bands runs on one GPU", missing)
    # with every rule met the command reaches the input
    r = runner.invoke(app, ok + ["--bands", "1,2"])
    assert r.exit_code == 1 and "Input file does not exist" in r.output


def test_create_streaming_rejects_a_band_beyond_the_source_before_anything_is_written(tmp_path):
    a = np.arange(3 * 6 * 5, dtype=np.int16).reshape(3, 6, 5)
    geotiff.write(tmp_path / "three.tif", a, transform=geotiff.Affine(1.0, 0.0, 0.0, 0.0, -1.0, 6.0), epsg=4326)
    out = tmp_path / "out.flac"
    r = runner.invoke(app, ["create-streaming", str(tmp_path / "three.tif"), "-o", str(out), "--bands", "1,4"])
    assert r.exit_code == 1 and "band 4 is not one of the source's 3 band(s)" in r.output and not out.exists()


def test_render_bands_rules_are_checked_before_anything_is_read(tmp_path):
    f, out = str(tmp_path / "missing.flac"), str(tmp_path / "o.png")
    ok = ["render", f, "-o", out, "--out-size", "8x8"]
    for extra, msg in ((["--bands", "1,2"], "--bands takes three band numbers"),
                       (["--bands", "1,2,3,4"], "--bands takes three band numbers"),
                       (["--bands", "1,2,x"], "--bands takes three band numbers"),
                       (["--bands", "1,2,0"], "--bands takes three band numbers"),
                       (["--bands", "3,2,1", "--hillshade"], "--bands cannot be combined with --hillshade"),
                       (["--bands", "3,2,1", "--hillshade", "300,40"], "--bands cannot be combined with --hillshade"),
                       (["--bands", "3,2,1", "--channels", "1"], "--channels must stay 4"),
                       (["--bands", "3,2,1", "--channels", "2"], "--channels must stay 4"),
                       (["--bands", "3,2,1", "--colormap", "heat"], "--bands keeps --colormap gray"),
                       (["--bands", "3,2,1", "--band", "2"], "give --band or --bands, not both"),
                       (["--band", "0"], "--band numbers start at 1")):
        _rejected(ok + extra, msg, f)
    assert not Path(out).exists()
    for extra in (["--bands", "3,2,1", "--gamma", "2.2", "--transfer", "log"], ["--band", "2", "--hillshade"]):
        r = runner.invoke(app, ok + extra + ["--stretch", "range:0,1"])
        assert r.exit_code == 1 and "--band" not in r.output  # every rule met: the command reaches the input


def test_extract_streaming_bands_rules_are_checked_before_anything_is_read(tmp_path):
    f, out = str(tmp_path / "missing.flac"), str(tmp_path / "o.tif")
    ok = ["extract-streaming", f, "-o", out]
    one = "--bands must name exactly one band"
    for extra, msg in ((["--tile-id", "0", "--bands", "1,2"], one), (["--center", "--bands", "all"], one),
                       (["--last", "--bands", "2,3"], one), (["--bbox", "0,0,1,1", "--bands", "1,2"], one),
                       (["--all", "--bands", "1,1"], "named twice"), (["--all", "--bands", "0"], "start at 1"),
                       (["--all", "--bands", "x"], "--bands must be 'all' or band numbers")):
        _rejected(ok + extra, msg, f)
    for extra in (["--all", "--bands", "all"], ["--bbox", "0,0,1,1", "--mosaic", "--bands", "3,1"],
                  ["--bbox", "0,0,1,1", "--out-size", "4x4", "--bands", "1,2,3"], ["--tile-id", "0", "--bands", "2"]):
        r = runner.invoke(app, ok + extra)
        assert r.exit_code == 1 and "--bands" not in r.output  # every rule met: the command reaches the input
    assert not Path(out).exists()


def test_stats_band_rule(tmp_path):
    r = runner.invoke(app, ["stats", str(tmp_path / "missing.flac"), "--band", "0"])
    assert r.exit_code == 1 and "--band numbers start at 1" in r.output


# ------------------------------------------------------------------------------------------------ python rules
def test_render_window_rejects_composite_options_before_the_file_is_opened(tmp_path):
    f = tmp_path / "missing.flac"
    box = [0.0, 0.0, 1.0, 1.0]
    for kw, msg in ((dict(bands=(1, 2)), "three bands"), (dict(bands=(1, 2, 3, 4)), "three bands"),
                    (dict(bands=(1, 2, 3), hillshade=(315.0, 45.0)), "cannot be hillshaded"),
                    (dict(bands=(1, 2, 3), channels=1), "4 channels"),
                    (dict(bands=(1, 2, 3), colormap="heat"), '"gray" colormap'),
                    (dict(bands=(1, 2, 3), band=2), "band or bands")):
        with pytest.raises(ValueError, match=msg):
            streaming.render_window(f, box, 4, 4, **kw)


def test_create_streaming_bands_array_checks_before_any_gpu_work(tmp_path):
    a = np.zeros((2, 4, 4), dtype=np.int16)
    tr = geotiff.Affine(1.0, 0.0, 0.0, 0.0, -1.0, 4.0)
    out = tmp_path / "o.flac"
    with pytest.raises(ValueError, match="band 1 must be among"):
        streaming.create_streaming_bands_array(a, [2, 3], tr, "EPSG:4326", out, ctx=object())
    with pytest.raises(ValueError, match="one band number per plane"):
        streaming.create_streaming_bands_array(a, [1, 2, 3], tr, "EPSG:4326", out, ctx=object())
    with pytest.raises(ValueError, match="one shape and dtype"):
        streaming.create_streaming_bands_array([a[0], a[1, :2]], [1, 2], tr, "EPSG:4326", out, ctx=object())
    assert not out.exists()


# ------------------------------------------------------------------------------------------------ ABI surface
def test_composite_prototypes_and_structure_match_the_header(tmp_path):
    hdr = ROOT / "include" / "flac_raster_amd.h"
    proto = ("int (*p%d)(frs_ctx *, const frs_raster_desc *, const void *, const frs_raster_desc *, void *, "
             "const frs_window_map *, int32_t, const double *, const frs_composite_params *) = %s;\n")
    names = ("frs_render_composite_window_device", "frs_render_composite_window")
    (tmp_path / "t.c").write_text(f'#include "{hdr}"\n' + "".join(proto % (i, n) for i, n in enumerate(names)))
    subprocess.run(["gcc", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")], check=True)
    (tmp_path / "v.c").write_text(
        f'#include "{hdr}"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){{printf("%zu %zu %zu %zu %zu\\n", '
        "sizeof(frs_composite_params), offsetof(frs_composite_params, hi), offsetof(frs_composite_params, lut), "
        "offsetof(frs_composite_params, n), offsetof(frs_composite_params, nodata_rgba));return 0;}\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "v"), str(tmp_path / "v.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "v")], capture_output=True, text=True, check=True).stdout.split()]
    P = _native.CompositeParams
    assert out == [ctypes.sizeof(P), P.hi.offset, P.lut.offset, P.n.offset, P.nodata_rgba.offset]
    assert set(names) <= set(_native.EXPORTS)


def test_library_exports_the_composite_entry_points():
    L = _native.load_library()
    rdp, vp = ctypes.POINTER(_native.RasterDesc), ctypes.c_void_p
    want = [vp, rdp, vp, rdp, vp, ctypes.POINTER(_native.WindowMap), ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(_native.CompositeParams)]
    for name in ("frs_render_composite_window_device", "frs_render_composite_window"):
        fn = getattr(L, name)
        assert fn.argtypes == want and fn.restype is ctypes.c_int32
