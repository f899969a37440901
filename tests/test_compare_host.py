"""The host side of the compare feature (reference compare.py:15-149, cli.py:247-290): structure layouts against the
C header, the pure combination of band records into the reference's result dict, the shape-mismatch path, and the
command-line validation.  Nothing here needs a GPU."""
import ctypes
import json
import math
import subprocess
from pathlib import Path

import numpy as np
from typer.testing import CliRunner

from flac_raster_amd import geotiff
from flac_raster_amd.cli import app

ROOT = Path(__file__).resolve().parents[1]
runner = CliRunner()

HEADER_KEYS = ["file1", "file2", "shape_match", "dtype_match", "crs_match", "file1_shape", "file2_shape", "file1_dtype",
               "file2_dtype", "file1_crs", "file2_crs"]
STAT_KEYS = ["arrays_equal", "max_difference", "mean_difference", "rmse", "file1_min", "file1_max", "file2_min",
             "file2_max"]
BAND_KEYS = ["band", "equal", "max_diff", "mean_diff", "file1_range", "file2_range", "exact"]
EXACT_KEYS = ["n_different", "max_difference", "mean_difference", "first_difference"]


def test_compare_struct_layouts_match_header(tmp_path):
    """ctypes CompareDesc / CompareBand against frs_compare_desc / frs_compare_band (offsets from a tiny C program)."""
    from flac_raster_amd._native import CompareBand, CompareDesc
    dfields = [n for n, _ in CompareDesc._fields_]
    bfields = [n for n, _ in CompareBand._fields_]
    items = ["sizeof(frs_compare_desc)"] + [f"offsetof(frs_compare_desc, {n})" for n in dfields]
    items += ["sizeof(frs_compare_band)"] + [f"offsetof(frs_compare_band, {n})" for n in bfields]
    fmt = " ".join(["%zu"] * len(items))
    prog = (f'#include "{ROOT / "include" / "flac_raster_amd.h"}"\n#include <stdio.h>\n#include <stddef.h>\n'
            f'int main(void){{printf("{fmt}\\n", {", ".join(items)});return 0;}}\n')
    c = tmp_path / "t.c"
    c.write_text(prog)
    subprocess.run(["gcc", "-o", str(tmp_path / "t"), str(c)], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = [ctypes.sizeof(CompareDesc)] + [getattr(CompareDesc, n).offset for n in dfields]
    want += [ctypes.sizeof(CompareBand)] + [getattr(CompareBand, n).offset for n in bfields]
    assert out == want
    assert dfields == ["height", "width", "nbands", "dtype", "a_row_stride", "a_band_stride", "b_row_stride",
                       "b_band_stride"]
    assert bfields == ["count", "n_diff", "first_diff", "a_min", "a_max", "b_min", "b_max", "np_max_abs", "np_sum_abs",
                       "np_sum_sq", "max_abs", "sum_abs"]


def _header(shape=(2, 4, 5)):
    return {"file1": "a.tif", "file2": "b.tif", "shape_match": True, "dtype_match": True, "crs_match": False,
            "file1_shape": shape, "file2_shape": shape, "file1_dtype": "uint8", "file2_dtype": "uint8",
            "file1_crs": "EPSG:4326", "file2_crs": "None"}


def _bands():
    # band 1 equal; band 2: 3 elements differ, first at linear index 13 = row 2, col 3 of a 4 x 5 band
    b1 = dict(count=20, n_diff=0, first_diff=-1, a_min=1.0, a_max=9.0, b_min=1.0, b_max=9.0, np_max_abs=0.0,
              np_sum_abs=0.0, np_sum_sq=0.0, max_abs=0.0, sum_abs=0.0)
    b2 = dict(count=20, n_diff=3, first_diff=13, a_min=0.0, a_max=200.0, b_min=2.0, b_max=100.0, np_max_abs=251.0,
              np_sum_abs=300.0, np_sum_sq=90.0, max_abs=7.0, sum_abs=12.0)
    return [b1, b2]


def test_results_from_bands_keys_values_and_json():
    from flac_raster_amd.compare import results_from_bands
    res = results_from_bands(_header(), _bands(), True)
    assert list(res) == HEADER_KEYS + STAT_KEYS + ["bands", "exact"]
    assert res["arrays_equal"] is False
    assert res["max_difference"] == 251.0           # max of the band maxes
    assert res["mean_difference"] == 300.0 / 40     # summed sums over summed counts
    assert res["rmse"] == math.sqrt(90.0 / 40)
    assert (res["file1_min"], res["file1_max"], res["file2_min"], res["file2_max"]) == (0.0, 200.0, 1.0, 100.0)
    assert [list(b) for b in res["bands"]] == [BAND_KEYS, BAND_KEYS]
    assert [b["band"] for b in res["bands"]] == [1, 2]
    assert [b["equal"] for b in res["bands"]] == [True, False]
    assert res["bands"][1]["max_diff"] == 251.0 and res["bands"][1]["mean_diff"] == 15.0
    assert res["bands"][1]["file1_range"] == [0.0, 200.0] and res["bands"][1]["file2_range"] == [2.0, 100.0]
    assert list(res["exact"]) == EXACT_KEYS
    assert res["exact"] == {"n_different": 3, "max_difference": 7.0, "mean_difference": 12.0 / 40,
                            "first_difference": [1, 2, 3]}
    assert res["bands"][0]["exact"]["first_difference"] is None
    assert res["bands"][1]["exact"] == {"n_different": 3, "max_difference": 7.0, "mean_difference": 12.0 / 20,
                                        "first_difference": [1, 2, 3]}
    back = json.loads(json.dumps(res, indent=2))
    assert list(back) == list(res) and back["file1_shape"] == [2, 4, 5]


def test_results_from_bands_no_bands_equal_and_nan():
    from flac_raster_amd.compare import results_from_bands
    res = results_from_bands(_header(), _bands(), False)
    assert list(res) == HEADER_KEYS + STAT_KEYS + ["exact"]
    eq = results_from_bands(_header(), [_bands()[0], _bands()[0]], True)
    assert eq["arrays_equal"] is True and eq["exact"]["first_difference"] is None
    assert eq["max_difference"] == 0.0 and eq["mean_difference"] == 0.0 and eq["rmse"] == 0.0
    # a NaN band makes the whole-raster max / min NaN (np.max propagates) and the first difference is in band 0
    nb = dict(_bands()[1], a_min=float("nan"), a_max=float("nan"), np_max_abs=float("nan"), np_sum_abs=float("nan"),
              np_sum_sq=float("nan"), max_abs=float("nan"), sum_abs=float("nan"), first_diff=0)
    nn = results_from_bands(_header(), [nb, _bands()[0]], True)
    assert nn["arrays_equal"] is False
    assert all(math.isnan(nn[k]) for k in ("max_difference", "mean_difference", "rmse", "file1_min", "file1_max"))
    assert nn["file2_min"] == 1.0 and nn["exact"]["first_difference"] == [0, 0, 0]
    # shapes differ: header keys only, whatever the band list
    h = dict(_header(), shape_match=False, file2_shape=(2, 4, 6))
    assert list(results_from_bands(h, [], True)) == HEADER_KEYS


def test_compare_tiffs_shape_mismatch_needs_no_gpu(tmp_path):
    from flac_raster_amd.compare import compare_tiffs, display_comparison_table
    a = np.arange(3 * 8 * 9, dtype=np.uint8).reshape(3, 8, 9)
    b = np.arange(3 * 8 * 10, dtype=np.uint8).reshape(3, 8, 10)
    geotiff.write(tmp_path / "a.tif", a, epsg=4326)
    geotiff.write(tmp_path / "b.tif", b, epsg=4326)
    res = compare_tiffs(tmp_path / "a.tif", tmp_path / "b.tif")
    assert list(res) == HEADER_KEYS
    assert res["shape_match"] is False and res["dtype_match"] is True and res["crs_match"] is True
    assert (res["file1"], res["file2"]) == ("a.tif", "b.tif")
    assert res["file1_shape"] == (3, 8, 9) and res["file2_shape"] == (3, 8, 10)
    assert res["file1_dtype"] == "uint8" and res["file1_crs"] == "EPSG:4326"
    from rich.console import Console
    con = Console(record=True, width=200)
    display_comparison_table(res, con)
    text = con.export_text()
    assert "TIFF Comparison Results" in text
    assert "Cannot compute detailed statistics - shapes don't match!" in text
    r = runner.invoke(app, ["compare", str(tmp_path / "a.tif"), str(tmp_path / "b.tif")])
    assert r.exit_code == 0 and "shapes don't match" in r.output.replace("\n", "")


def test_display_prints_the_five_tables():
    from rich.console import Console

    from flac_raster_amd.compare import display_comparison_table, results_from_bands
    con = Console(record=True, width=200)
    display_comparison_table(results_from_bands(_header(), _bands(), True), con)
    text = con.export_text()
    for title in ("TIFF Comparison Results", "Statistical Comparison", "Data Ranges", "Per-Band Statistics",
                  "Exact Differences"):
        assert title in text
    for label in ("Shape", "Data Type", "CRS", "Arrays Equal", "Max Difference", "Mean Difference", "RMSE"):
        assert label in text
    assert "251.000000" in text and "[0.0, 200.0]" in text


def test_compare_arrays_rejects_unsupported_common_type():
    """int32 vs uint32 promote to int64, which no kernel handles: ValueError before any device is looked for."""
    import pytest

    from flac_raster_amd.compare import compare_arrays
    with pytest.raises(ValueError):
        compare_arrays(np.zeros((2, 2), np.int32), np.zeros((2, 2), np.uint32))


def _flat(out: str) -> str:
    return " ".join(out.split())


def test_cli_compare_validation(tmp_path):
    a = tmp_path / "a.tif"
    geotiff.write(a, np.zeros((1, 4, 4), np.uint8))
    r = runner.invoke(app, ["compare", str(a), str(tmp_path / "missing.tif")])
    assert r.exit_code == 1
    assert "Error: File does not exist:" in _flat(r.output) and "missing.tif" in r.output.replace("\n", "")
    txt = tmp_path / "b.txt"
    txt.write_text("x")
    r = runner.invoke(app, ["compare", str(a), str(txt)])
    assert r.exit_code == 1 and "is not a TIFF file" in _flat(r.output)


def test_cli_convert_verify_rejections(tmp_path):
    flac = tmp_path / "x.flac"
    flac.write_bytes(b"fLaC")
    r = runner.invoke(app, ["convert", str(flac), "--verify"])
    assert r.exit_code == 1 and "--verify applies to plain TIFF to FLAC conversion" in _flat(r.output)
    tif = tmp_path / "x.tif"
    geotiff.write(tif, np.zeros((1, 4, 4), np.uint8))
    r = runner.invoke(app, ["convert", str(tif), "--spatial", "--verify"])
    assert r.exit_code == 1 and "--verify applies to plain TIFF to FLAC conversion" in _flat(r.output)
    assert flac.read_bytes() == b"fLaC"  # rejected before any work: the existing output was not touched
