"""Restatement of the band statistics and the band histogram (csrc/frs_stats.h), written from the definition: Python
integers for the integer sums, the bin rule as numpy fp64 expressions (not np.histogram, whose edge rule differs), and
the percentile rule on a sorted list."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit roundoff of fp64


def gamma(k: int) -> float:
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a sum of k + 1 terms in ANY order."""
    return k * U / (1.0 - k * U) if k > 0 else 0.0


def classes(a: np.ndarray, nodata=None):
    """(valid, nodata, nan) boolean masks of a band."""
    a = np.asarray(a)
    isf = a.dtype.kind == "f"
    if nodata is None:
        nd = np.zeros(a.shape, dtype=bool)
    elif isf:
        ndt = a.dtype.type(nodata)
        nd = (a == ndt) | (np.isnan(a) & bool(np.isnan(ndt)))
    else:
        nd = a == a.dtype.type(int(nodata))
    nan = (np.isnan(a) & ~nd) if isf else np.zeros(a.shape, dtype=bool)
    return ~nd & ~nan, nd, nan


def band_stats(a: np.ndarray, nodata=None) -> dict:
    """One band's first pass.  Integers: isum, isq exact Python integers.  Floats: fsum = math.fsum of the valid values
    and abs_sum = math.fsum of their magnitudes (the scale of the sum's error bound)."""
    a = np.asarray(a)
    valid, nd, nan = classes(a, nodata)
    v = a[valid]
    out = {"n_valid": int(valid.sum()), "n_nodata": int(nd.sum()), "n_nan": int(nan.sum())}
    if v.size == 0:
        out.update(min=None, max=None, isum=0, isq=0, fsum=0.0, abs_sum=0.0)
        return out
    if a.dtype.kind in "iu" and a.dtype.itemsize <= 2 and v.size < 2 ** 30:
        w = v.astype(np.int64).ravel()  # |v| < 2^16 and fewer than 2^30 terms: the int64 sums are exact
        out.update(min=int(w.min()), max=int(w.max()), isum=int(w.sum()), isq=int((w * w).sum()))
    elif a.dtype.kind in "iu":
        vals = [int(x) for x in v.ravel()]
        out.update(min=min(vals), max=max(vals), isum=sum(vals), isq=sum(x * x for x in vals))
    else:
        x = v.astype(np.float64).ravel()
        with np.errstate(invalid="ignore"):
            out.update(min=float(x.min()), max=float(x.max()), isum=0, isq=0)
        fin = x[np.isfinite(x)]
        with np.errstate(invalid="ignore"):
            out["fsum"] = math.fsum(fin) if fin.size == x.size else float(np.sum(x))
        out["abs_sum"] = math.fsum(np.abs(fin))
    return out


def histogram(a: np.ndarray, lo: float, hi: float, nbins: int, nodata=None, centre: float = 0.0) -> dict:
    """One band's second pass: counts (int64[nbins]), below, above, and for float dtypes the terms (x - centre)^2 of
    m2 as fp64 values (each operator one rounding, as the kernel's)."""
    a = np.asarray(a)
    valid, _, _ = classes(a, nodata)
    x = a[valid].astype(np.float64).ravel()
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(nbins) / (hi - lo)
    below, above = x < lo, x > hi
    inside = x[~below & ~above]
    with np.errstate(invalid="ignore"):
        b = np.floor((inside - lo) * scale).astype(np.int64)
    b = np.where(b >= nbins, nbins - 1, b)
    counts = np.bincount(b, minlength=nbins).astype(np.int64)
    out = {"counts": counts, "below": int(below.sum()), "above": int(above.sum())}
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore", over="ignore"):
            d = x - np.float64(centre)
            out["m2_terms"] = d * d
    return out


def bin_index(x: float, lo: float, hi: float, nbins: int) -> int:
    """The bin rule for one value: -1 below, -2 above, else the bin."""
    x, lo, hi = np.float64(x), np.float64(lo), np.float64(hi)
    scale = np.float64(nbins) / (hi - lo)
    if x < lo:
        return -1
    if x > hi:
        return -2
    b = int(np.floor((x - lo) * scale))
    return nbins - 1 if b >= nbins else b


def percentile_sorted(values, q) -> object:
    """sorted(values)[k - 1] with k = max(1, ceil(q n / 100)) in exact rational arithmetic."""
    s = sorted(values)
    k = max(1, math.ceil(Fraction(q) * len(s) / 100))
    return s[k - 1]


def mean_std(values) -> tuple:
    """(mean, population deviation) of integers as exact Fractions (the deviation's SQUARE: the variance)."""
    vals = [int(v) for v in values]
    n = len(vals)
    mean = Fraction(sum(vals), n)
    var = Fraction(sum(v * v for v in vals), n) - mean * mean
    return mean, var


def is_nearest_sqrt(f: float, var: Fraction) -> bool:
    """Is the double f the correctly rounded (to nearest) square root of the rational var >= 0?"""
    if var == 0:
        return f == 0.0
    if not f > 0:
        return False
    lo = (Fraction(f) + Fraction(np.nextafter(f, -np.inf))) / 2
    hi = (Fraction(f) + Fraction(np.nextafter(f, np.inf))) / 2
    return lo * lo <= var <= hi * hi
