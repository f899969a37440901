"""Raster comparison (reference compare.py:15-149): are two rasters equal, and if not, by how much.

Every sample goes through one fused GPU pass (frs_compare, csrc/frs_compare.hip) that returns one record per band;
this module only combines those records into the reference's result dict and prints its tables.  There is no CPU
fallback: without the library or a gfx950 device the comparison raises, like every other entry point of the package.

Values follow numpy's, quirks included, because that is what the reference reports: ``a - b``, ``abs`` and ``** 2``
are evaluated in the rasters' dtype, so they wrap for integers (uint8: 5 - 10 = 251).  The ``exact`` key adds what a
user of 8-bit data needs: the differences without wrap.

Accumulation: integer sums are exact (the mean and RMSE equal numpy's whenever the exact sum is below 2**53, beyond
that they are the correctly rounded exact value).  For float rasters the per-element terms are formed in the dtype, as
numpy forms them, but ``mean_difference`` and ``rmse`` are accumulated in float64.  For float32 rasters numpy's own
pairwise float32 accumulation can differ from that in the low bits.
"""
from __future__ import annotations

import logging
import math
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from . import geotiff
from ._native import DTYPE_CODES, Context, default_context

log = logging.getLogger("flac_raster.compare")

HEADER_KEYS = ("file1", "file2", "shape_match", "dtype_match", "crs_match", "file1_shape", "file2_shape",
               "file1_dtype", "file2_dtype", "file1_crs", "file2_crs")


def _nanmax(vals) -> float:
    """np.max of a list: NaN if any entry is NaN."""
    vals = [float(v) for v in vals]
    return float("nan") if any(math.isnan(v) for v in vals) else max(vals)


def _nanmin(vals) -> float:
    vals = [float(v) for v in vals]
    return float("nan") if any(math.isnan(v) for v in vals) else min(vals)


def _exact(bands: List[Dict], width: int, band0: Optional[int] = None) -> Dict:
    """The un-wrapped differences of a list of band records (`band0`: the index of a single band)."""
    count = sum(int(b["count"]) for b in bands)
    first = None
    for i, b in enumerate(bands):
        if int(b["first_diff"]) >= 0:
            lin = int(b["first_diff"])
            first = [i if band0 is None else band0, lin // width, lin % width]
            break
    return {"n_different": sum(int(b["n_diff"]) for b in bands),
            "max_difference": _nanmax(b["max_abs"] for b in bands),
            "mean_difference": sum(float(b["sum_abs"]) for b in bands) / count,
            "first_difference": first}


def results_from_bands(header: Dict, bands: List[Dict], show_bands: bool = True) -> Dict:
    """The reference's result dict (compare.py:39-78: its keys, in its order, with its values) from the per-band
    records of frs_compare, followed by the extension key ``exact``.  `header` holds the eleven file / shape / dtype /
    CRS keys; the width of a row comes from ``file1_shape``.  Pure host code."""
    res = {k: header[k] for k in HEADER_KEYS}
    if not res["shape_match"]:
        return res
    width = int(res["file1_shape"][-1])
    count = sum(int(b["count"]) for b in bands)
    res["arrays_equal"] = all(int(b["n_diff"]) == 0 for b in bands)
    res["max_difference"] = _nanmax(b["np_max_abs"] for b in bands)
    res["mean_difference"] = sum(float(b["np_sum_abs"]) for b in bands) / count
    sum_sq = sum(float(b["np_sum_sq"]) for b in bands)  # wrapped squares of a signed dtype can sum below zero:
    res["rmse"] = float("nan") if sum_sq < 0 else math.sqrt(sum_sq / count)  # np.sqrt gives NaN there
    res["file1_min"] = _nanmin(b["a_min"] for b in bands)
    res["file1_max"] = _nanmax(b["a_max"] for b in bands)
    res["file2_min"] = _nanmin(b["b_min"] for b in bands)
    res["file2_max"] = _nanmax(b["b_max"] for b in bands)
    if show_bands:
        res["bands"] = []
        for i, b in enumerate(bands):
            res["bands"].append({
                "band": i + 1,
                "equal": int(b["n_diff"]) == 0,
                "max_diff": float(b["np_max_abs"]),
                "mean_diff": float(b["np_sum_abs"]) / int(b["count"]),
                "file1_range": [float(b["a_min"]), float(b["a_max"])],
                "file2_range": [float(b["b_min"]), float(b["b_max"])],
                "exact": _exact([b], width, band0=i),
            })
    res["exact"] = _exact(bands, width)
    return res


def _header(name1: str, name2: str, a: np.ndarray, b: np.ndarray, crs1, crs2) -> Dict:
    return {"file1": name1, "file2": name2, "shape_match": a.shape == b.shape, "dtype_match": a.dtype == b.dtype,
            "crs_match": crs1 == crs2, "file1_shape": tuple(a.shape), "file2_shape": tuple(b.shape),
            "file1_dtype": str(a.dtype), "file2_dtype": str(b.dtype), "file1_crs": str(crs1), "file2_crs": str(crs2)}


def compare_arrays(a: np.ndarray, b: np.ndarray, ctx: Optional[Context] = None, show_bands: bool = True) -> Dict:
    """Compare two rasters, (bands, h, w) or (h, w), on the GPU.  Different dtypes are both cast to
    ``np.result_type(a.dtype, b.dtype)`` first, which is what numpy's ``a - b`` does; a result type outside the seven
    supported dtypes raises ValueError.  Returns the dict of :func:`results_from_bands`; when the shapes differ only
    its header keys, and the GPU is not touched."""
    a, b = np.asarray(a), np.asarray(b)
    return _compare(_header("a", "b", a, b, None, None), a, b, ctx, show_bands)


def _compare(header: Dict, a: np.ndarray, b: np.ndarray, ctx: Optional[Context], show_bands: bool) -> Dict:
    if a.shape != b.shape:
        return results_from_bands(header, [], show_bands)
    if a.ndim not in (2, 3):
        raise ValueError("rasters must be (bands, height, width) or (height, width)")
    rt = np.result_type(a.dtype, b.dtype)
    if rt not in DTYPE_CODES:
        raise ValueError(f"cannot compare {a.dtype} with {b.dtype}: their common type {rt} is not one of "
                         f"{', '.join(str(k) for k in DTYPE_CODES)}")
    if a.dtype != rt:
        a = a.astype(rt)
    if b.dtype != rt:
        b = b.astype(rt)
    bands = (ctx or default_context()).compare_host(a, b)
    return results_from_bands(header, bands, show_bands)


def compare_tiffs(file1, file2, show_bands: bool = True) -> Dict:
    """compare.py:15-80: compare two TIFF files and return the comparison statistics."""
    file1, file2 = Path(file1), Path(file2)
    log.info(f"Comparing {file1} and {file2}")
    r1, r2 = geotiff.read(file1), geotiff.read(file2)
    header = _header(file1.name, file2.name, r1.data, r2.data, r1.crs_string, r2.crs_string)
    return _compare(header, r1.data, r2.data, None, show_bands)


def display_comparison_table(results: Dict, console=None) -> None:
    """compare.py:83-149: the four tables of the reference, then the un-wrapped differences."""
    from rich.console import Console
    from rich.table import Table
    con = console or Console()
    yn = lambda v: "YES" if v else "NO"  # noqa: E731
    t = Table(title="TIFF Comparison Results", show_header=True)
    t.add_column("Property", style="cyan")
    t.add_column(results["file1"], style="green")
    t.add_column(results["file2"], style="yellow")
    t.add_column("Match", style="bold")
    t.add_row("Shape", str(results["file1_shape"]), str(results["file2_shape"]), yn(results["shape_match"]))
    t.add_row("Data Type", results["file1_dtype"], results["file2_dtype"], yn(results["dtype_match"]))
    t.add_row("CRS", results["file1_crs"], results["file2_crs"], yn(results["crs_match"]))
    con.print(t)
    if not results.get("shape_match"):
        con.print("[red]Cannot compute detailed statistics - shapes don't match![/red]")
        return
    s = Table(title="Statistical Comparison", show_header=True)
    s.add_column("Metric", style="cyan")
    s.add_column("Value", style="bold")
    s.add_row("Arrays Equal", yn(results["arrays_equal"]))
    s.add_row("Max Difference", f"{results['max_difference']:.6f}")
    s.add_row("Mean Difference", f"{results['mean_difference']:.6f}")
    s.add_row("RMSE", f"{results['rmse']:.6f}")
    con.print(s)
    r = Table(title="Data Ranges", show_header=True)
    r.add_column("File", style="cyan")
    r.add_column("Min", style="blue")
    r.add_column("Max", style="red")
    r.add_row(results["file1"], f"{results['file1_min']:.2f}", f"{results['file1_max']:.2f}")
    r.add_row(results["file2"], f"{results['file2_min']:.2f}", f"{results['file2_max']:.2f}")
    con.print(r)
    if "bands" in results:
        bt = Table(title="Per-Band Statistics", show_header=True)
        bt.add_column("Band", style="cyan")
        bt.add_column("Equal", style="bold")
        bt.add_column("Max Diff", style="yellow")
        bt.add_column("Mean Diff", style="yellow")
        bt.add_column(f"{results['file1']} Range", style="green")
        bt.add_column(f"{results['file2']} Range", style="blue")
        for b in results["bands"]:
            bt.add_row(str(b["band"]), yn(b["equal"]), f"{b['max_diff']:.3f}", f"{b['mean_diff']:.6f}",
                       f"\\[{b['file1_range'][0]:.1f}, {b['file1_range'][1]:.1f}]",
                       f"\\[{b['file2_range'][0]:.1f}, {b['file2_range'][1]:.1f}]")
        con.print(bt)
    if "exact" in results:
        e = Table(title="Exact Differences", show_header=True)
        e.add_column("Scope", style="cyan")
        e.add_column("Different", style="bold")
        e.add_column("Max |a-b|", style="yellow")
        e.add_column("Mean |a-b|", style="yellow")
        e.add_column("First (band, row, col)", style="green")

        def row(label, x):
            f = x["first_difference"]
            e.add_row(label, f"{x['n_different']:,}", f"{x['max_difference']:.6f}", f"{x['mean_difference']:.6f}",
                      "-" if f is None else f"({f[0] + 1}, {f[1]}, {f[2]})")
        row("All bands", results["exact"])
        for b in results.get("bands", []):
            row(f"Band {b['band']}", b["exact"])
        con.print(e)
