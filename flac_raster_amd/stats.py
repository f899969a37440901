"""Band statistics and histograms on the GPU (extension: the reference has none; `gdalinfo -stats -hist` is the model).

Two passes over a band that is already in device memory, or goes there once: frs_band_stats* (counts of valid / nodata /
NaN pixels, min, max, the sum -- exact 128-bit sums and sums of squares for the integer dtypes) and frs_band_histogram*
(the counts under the bin rule of csrc/frs_stats.h and, for float dtypes, the square sum centred on the mean).  What is
left for the host is arithmetic on a few numbers per band: the mean and deviation, and percentiles read off the
histogram.  The rules (`histogram_range`, `mean_std_from_sums`, `percentile`) are pure and need no GPU.
"""
from __future__ import annotations

import math
from fractions import Fraction
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

MAX_BINS = 16384  # _native.HIST_MAX_BINS: 64 KB of LDS counters


def histogram_range(dtype, vmin, vmax, bins: int) -> Tuple[float, float, int]:
    """(lo, hi, nbins) of the histogram of a band of `dtype` whose valid values span vmin .. vmax, with at most `bins`
    bins.  An integer dtype whose range fits gets a bin per value (lo = vmin, hi = vmax + 1, nbins = vmax - vmin + 1:
    the bin rule's scale is then exactly 1).  Otherwise lo = vmin, hi = vmax (hi = lo + 1 when they are equal) and
    nbins = bins."""
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must be 1..{MAX_BINS}, got {bins}")
    if np.dtype(dtype).kind in "iu":
        m, M = int(vmin), int(vmax)
        if M - m + 1 <= bins:
            return float(m), float(M + 1), M - m + 1
    lo, hi = float(vmin), float(vmax)
    if hi == lo:
        hi = lo + 1.0
    return lo, hi, bins


def _sqrt_fraction(v: Fraction) -> float:
    """sqrt of a non-negative rational, rounded once (to nearest): an integer square root with 128 spare bits, and a
    sticky bit below them when it is not exact."""
    if v == 0:
        return 0.0
    num, den = v.numerator * v.denominator, v.denominator  # sqrt(p / q) = sqrt(p q) / q
    k = 128
    x = num << (2 * k)
    r = math.isqrt(x)
    if r * r != x:
        r, k = 2 * r + 1, k + 1
    return float(Fraction(r, den << k))


def mean_std_from_sums(n: int, isum: int, isq: int) -> Tuple[float, float]:
    """(mean, population deviation) of n integers with exact sum `isum` and exact sum of squares `isq`, in exact
    rational arithmetic, each rounded once at the end."""
    n, isum, isq = int(n), int(isum), int(isq)
    mean = Fraction(isum, n)
    var = Fraction(n * isq - isum * isum, n * n)
    return float(mean), _sqrt_fraction(var)


def percentile(hist: Dict, q) -> Optional[Union[int, float]]:
    """The q-th percentile (0 <= q <= 100) read off a histogram {lo, hi, counts, per_value}.  n is the sum of the
    counts (pixels below lo or above hi are not in it), k = max(1, ceil(q n / 100)) in exact rational arithmetic, and
    b the first bin whose cumulative count reaches k.  A histogram with a bin per value returns lo + b: exactly
    sorted(valid)[k - 1], numpy's method="inverted_cdf".  Any other returns the bin's centre,
    lo + (b + 0.5) (hi - lo) / nbins: within half a bin width of that value.  None for an empty histogram."""
    counts = [int(c) for c in hist["counts"]]
    n = sum(counts)
    if n == 0:
        return None
    qf = Fraction(q)
    if not 0 <= qf <= 100:
        raise ValueError(f"a percentile must be 0..100, got {q!r}")
    k = max(1, math.ceil(qf * n / 100))
    cum, b = 0, 0
    for b, c in enumerate(counts):
        cum += c
        if cum >= k:
            break
    lo, hi = hist["lo"], hist["hi"]
    if hist.get("per_value"):
        return int(lo) + b
    return float(lo) + (b + 0.5) * (float(hi) - float(lo)) / len(counts)


def _finite(v) -> bool:
    return v is not None and math.isfinite(v)


def band_statistics(a=None, *, ptr: Optional[int] = None, desc=None, nodata=None, bins: int = 256, ctx=None
                    ) -> List[Dict]:
    """Statistics of every band of a host raster `a` ((bands, h, w) or (h, w)), or of the device raster at `ptr` laid
    out as the RasterDesc `desc` (at most 8 bands either way).  `nodata` (a number, or None) masks the pixels that hold
    it.  Per band: valid, nodata_count, nan, min, max, mean, std (population, ddof = 0) and histogram {lo, hi, counts,
    below, above, per_value} with at most `bins` bins (histogram_range).  A host raster goes up once for both passes.

    Integer dtypes: min, max and the counts are exact; mean and std come from the exact 128-bit sums
    (mean_std_from_sums).  Float dtypes: mean = sum / n with the kernel's fp64 sum, std = sqrt(m2 / n) with the second
    pass's square sum centred on that mean.  A band without a valid pixel has min = max = mean = std = None and no
    histogram (None); no second pass runs for it.

    A float band that holds +-inf has a non-finite min or max; its histogram takes the finite valid range, found by one
    more first pass per infinite end with that infinity as the nodata value: the pass's min / max is then over
    everything but that infinity and NaN.  When a finite nodata value is in force as well, that extra pass cannot mask
    it too, so the range is the hull of the finite valid values and the nodata value: wider at most, and the counts are
    unaffected, because the histogram pass masks nodata again.  The infinities are counted in below / above.  The
    mean, std and m2 of such a band are what IEEE arithmetic gives (inf or NaN)."""
    from ._native import DTYPE_CODES, default_context
    ctx = ctx or default_context()
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must be 1..{MAX_BINS}, got {bins}")
    buf = None
    try:
        if ptr is None:
            a = np.ascontiguousarray(a)
            if a.ndim not in (2, 3) or a.dtype not in DTYPE_CODES or a.size == 0:
                raise ValueError("band_statistics needs a non-empty (bands, h, w) or (h, w) array of a raster dtype")
            nb = a.shape[0] if a.ndim == 3 else 1
            desc = ctx.make_raster_desc(a.shape[-2], a.shape[-1], a.dtype, nbands=nb)
            buf = ctx.alloc(a.nbytes)
            buf.upload(a)
            ptr = buf.ptr
        return _device_statistics(ctx, ptr, desc, nodata, bins)
    finally:
        if buf is not None:
            buf.close()


def _dtype_of(desc) -> np.dtype:
    from ._native import DTYPE_CODES
    return next(dt for dt, code in DTYPE_CODES.items() if code == desc.dtype)


def _band_desc(ctx, desc, b: int):
    """(descriptor, element offset) of band b alone"""
    d = ctx.make_raster_desc(desc.height, desc.width, _dtype_of(desc), nbands=1, row_stride=desc.row_stride)
    return d, b * int(desc.band_stride) if desc.nbands > 1 else 0


def _device_statistics(ctx, ptr: int, desc, nodata, bins: int) -> List[Dict]:
    dtype = _dtype_of(desc)
    is_int = dtype.kind in "iu"
    first = ctx.band_stats_device(ptr, desc, nodata=nodata)
    out = []
    for b, s in enumerate(first):
        n = int(s["n_valid"])
        r = {"valid": n, "nodata_count": int(s["n_nodata"]), "nan": int(s["n_nan"]), "min": None, "max": None,
             "mean": None, "std": None, "histogram": None}
        out.append(r)
        if n == 0:
            continue
        vmin, vmax = s["min"], s["max"]
        r["min"], r["max"] = (int(vmin), int(vmax)) if is_int else (float(vmin), float(vmax))
        bd, off = _band_desc(ctx, desc, b)
        bptr = ptr + off * dtype.itemsize
        fmin, fmax = vmin, vmax
        if not is_int and not (math.isfinite(vmin) and math.isfinite(vmax)):
            if vmax == math.inf:
                fmax = ctx.band_stats_device(bptr, bd, nodata=math.inf)[0]["max"]
            if vmin == -math.inf:
                fmin = ctx.band_stats_device(bptr, bd, nodata=-math.inf)[0]["min"]
            if not (_finite(fmin) and _finite(fmax)) or fmin > fmax:  # no finite valid pixel
                fmin, fmax = 0.0, 0.0
        lo, hi, nbins = histogram_range(dtype, fmin, fmax, bins)
        if is_int:
            r["mean"], r["std"] = mean_std_from_sums(n, s["isum"], s["isq"])
            centre = 0.0
        else:
            r["mean"] = float(np.float64(s["sum"]) / np.float64(n))
            centre = r["mean"] if math.isfinite(r["mean"]) else 0.0
        counts, ho = ctx.band_histogram_device(bptr, bd, lo, hi, nbins, nodata=nodata, centre=centre)
        if not is_int:
            with np.errstate(invalid="ignore"):
                r["std"] = float(np.sqrt(np.float64(ho[0]["m2"]) / np.float64(n))) if math.isfinite(r["mean"]) \
                    else math.nan
        r["histogram"] = {"lo": int(lo) if is_int else lo, "hi": int(hi) if is_int else hi,
                          "counts": [int(c) for c in counts[0]], "below": ho[0]["below"], "above": ho[0]["above"],
                          "per_value": bool(is_int and hi - lo == nbins)}
    return out


def _file_nodata(word, own):
    """The nodata value a statistics read uses: the file's own ("file", the default), none (None or "none"), or a
    number that overrides it."""
    if word is None or (isinstance(word, str) and word == "none"):
        return None
    if isinstance(word, str):
        if word != "file":
            raise ValueError(f"nodata must be a number, None, 'none' or 'file', got {word!r}")
        return own
    return float(word)


def raster_file_statistics(path, level: int = 0, nodata="file", bins: int = 256, ctx=None, band=None) -> Dict:
    """Statistics of a raster file: {"file", "kind", "dtype", "width", "height", "level", "nodata", "bands": [...]} with
    one band_statistics entry per band.  A GeoTIFF gives every band: the bands go up once, more than 8 in groups of 8,
    and the nodata value is the file's GDAL_NODATA tag.  A streaming .flac gives the raster of overview level `level`
    through reconstruct_device -- decoded into device memory and never downloaded -- and the nodata value is the
    index's.  `nodata`: "file" (the default), None / "none" to read without one, or a number that overrides it.
    A streaming file of several bands gives every stored band, one reconstruction at a time.  `band` (1-based) selects
    one band of either kind of file; "band_numbers" names the bands the entries of "bands" describe."""
    from . import geotiff, streaming
    from ._native import default_context
    p = Path(path)
    suffix = p.suffix.lower()
    level = int(level)
    if suffix in (".tif", ".tiff"):
        if level != 0:
            raise ValueError("--level applies to streaming FLAC files: a TIFF has one level")
        r = geotiff.read(p)
        dtype = np.dtype(r.dtype)
        nd = _file_nodata(nodata, r.nodata)
        if nd is not None:
            nd = streaming.nodata_for_dtype(nd, dtype)
        data = r.data if r.data.ndim == 3 else r.data[None]
        numbers = list(range(1, data.shape[0] + 1))
        if band is not None:
            if not 1 <= int(band) <= data.shape[0]:
                raise LookupError(f"band {band} not in this file (bands present: {numbers})")
            data, numbers = data[int(band) - 1:int(band)], [int(band)]
        data = np.ascontiguousarray(data)
        bands: List[Dict] = []
        ctx = ctx or default_context()
        buf = ctx.alloc(data.nbytes)
        try:
            buf.upload(data)
            h, w = data.shape[-2:]
            for b0 in range(0, data.shape[0], 8):
                nb = min(8, data.shape[0] - b0)
                d = ctx.make_raster_desc(h, w, dtype, nbands=nb)
                bands += _device_statistics(ctx, buf.ptr + b0 * h * w * dtype.itemsize, d, nd, int(bins))
        finally:
            buf.close()
        kind, width, height = "tiff", w, h
    elif suffix == ".flac":
        _, index = streaming.read_index(p)
        if level not in streaming.overview_levels(index):
            raise LookupError(f"level {level} is not in the file (levels: {streaming.overview_levels(index)})")
        ctx = ctx or default_context()
        numbers = streaming.bands_of(index) if band is None else [int(band)]
        bands = []
        for b in numbers:  # one band in device memory at a time
            dst, dtype, li = streaming.reconstruct_device(p, ctx, level, bands=None if b == 1 else [b])
            dtype = np.dtype(dtype)
            try:
                nd = _file_nodata(nodata, streaming.index_nodata(index))
                if nd is not None:
                    nd = streaming.nodata_for_dtype(nd, dtype)
                height, width = int(li["height"]), int(li["width"])
                d = ctx.make_raster_desc(height, width, dtype)
                bands += _device_statistics(ctx, dst.ptr, d, nd, int(bins))
            finally:
                dst.close()
        kind = "streaming"
    else:
        raise ValueError(f"Unsupported file format: {suffix}")
    return {"file": str(path), "kind": kind, "dtype": str(dtype), "width": width, "height": height, "level": level,
            "nodata": nd, "bands": bands, "band_numbers": numbers}


def with_percentiles(band: Dict, qs: Sequence) -> Dict:
    """The band's entry with "percentiles": {str(q): value} read off its histogram (empty without one)."""
    h = band.get("histogram")
    return dict(band, percentiles={} if h is None else {str(q): percentile(h, q) for q in qs})


# ---- the streaming index's "statistics" key
def _num_to_index(v):
    """A number as the index holds it: itself, or "nan" / "inf" / "-inf" (streaming._nodata_to_index's rule)."""
    if v is None or isinstance(v, (bool, int)):
        return v
    return v if math.isfinite(v) else str(float(v))


def _num_from_index(v):
    return float(v) if isinstance(v, str) else v


_NUMERIC = ("min", "max", "mean", "std")


def statistics_to_index(band: Dict) -> Dict:
    """One band's statistics as the index's "statistics" value (JSON-safe: non-finite numbers as words)."""
    out = {k: band[k] for k in ("valid", "nodata_count", "nan")}
    for k in _NUMERIC:
        out[k] = _num_to_index(band[k])
    h = band.get("histogram")
    out["histogram"] = None if h is None else dict(h, lo=_num_to_index(h["lo"]), hi=_num_to_index(h["hi"]))
    return out


def statistics_from_index(value: Optional[Dict]) -> Optional[Dict]:
    """The inverse of statistics_to_index (None for None)."""
    if value is None:
        return None
    out = dict(value)
    for k in _NUMERIC:
        out[k] = _num_from_index(value.get(k))
    h = value.get("histogram")
    if h is not None:
        out["histogram"] = dict(h, lo=_num_from_index(h["lo"]), hi=_num_from_index(h["hi"]))
    return out


def format_band(i: int, band: Dict, qs: Sequence = ()) -> List[str]:
    """The text lines of one band's statistics (the `stats` and `info` commands)."""
    lines = [f"Band {i}:",
             f"  Valid pixels: {band['valid']}  (nodata {band['nodata_count']}, NaN {band['nan']})"]
    if band["valid"]:
        lines.append(f"  Minimum: {band['min']}  Maximum: {band['max']}")
        lines.append(f"  Mean: {band['mean']}  StdDev: {band['std']}")
        h = band.get("histogram")
        if h is not None:
            lines.append(f"  Histogram: {len(h['counts'])} bins over [{h['lo']}, {h['hi']}]"
                         f"{' (one per value)' if h.get('per_value') else ''}, below {h['below']}, above {h['above']}")
            for q in qs:
                lines.append(f"  Percentile {q}: {percentile(h, q)}")
    return lines
