"""frs_band_stats* and frs_band_histogram* on the GPU against the restatement tests/stats_ref.py.

Integers: every field is exact.  Floats: the counts, min, max, the histogram counts, below and above are exact; the sum
is within gamma(n - 1) * sum|v| of math.fsum (u = 2^-53: the bound no summation order of n terms exceeds, so it is
derived, not measured), m2 within the same bound on its own terms plus one rounding per term."""
import ctypes
import math

import numpy as np
import pytest

from flac_raster_amd import _native
from tests import stats_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.int16, np.int32, np.uint32, np.float32, np.float64]
IDS = [np.dtype(d).name for d in DTYPES]


def _as3(x):
    return x if x.ndim == 3 else x[None]


def rand_band(rng, dtype, shape, spread=1000):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(shape) * spread).astype(dt)
    ii = np.iinfo(dt)
    lo = max(int(ii.min), -spread // 2)
    return rng.integers(lo, min(int(ii.max), lo + spread) + 1, shape).astype(dt)


def check_stats(got, a, nodata):
    """Every field of every band's frs_band_stats_out against the restatement on the dense array a."""
    a = _as3(a)
    assert len(got) == a.shape[0]
    for r, band in zip(got, a):
        w = R.band_stats(band, nodata)
        print("stats", band.dtype, band.shape, nodata, r)
        assert (r["n_valid"], r["n_nodata"], r["n_nan"]) == (w["n_valid"], w["n_nodata"], w["n_nan"])
        if w["n_valid"] == 0:
            assert math.isnan(r["min"]) and math.isnan(r["max"])
            assert r["sum"] == 0.0 and r["isum"] == 0 and r["isq"] == 0
            continue
        assert r["min"] == w["min"] and r["max"] == w["max"]
        if band.dtype.kind in "iu":
            assert r["isum"] == w["isum"] and r["isq"] == w["isq"]
            assert r["sum"] == float(w["isum"])  # the exact sum rounded once (int -> float rounds to nearest)
        else:
            assert r["isum"] == 0 and r["isq"] == 0
            if np.isfinite(band[R.classes(band, nodata)[0]]).all():
                err, bound = abs(r["sum"] - w["fsum"]), R.gamma(w["n_valid"] - 1) * w["abs_sum"]
                print("  sum error", err, "bound", bound)
                assert err <= bound


def check_hist(counts, outs, a, lo, hi, nbins, nodata, centre=0.0):
    a = _as3(a)
    assert counts.shape == (a.shape[0], nbins) and len(outs) == a.shape[0]
    for c, o, band in zip(counts, outs, a):
        w = R.histogram(band, lo, hi, nbins, nodata, centre)
        assert c.tolist() == w["counts"].tolist()
        assert (o["below"], o["above"]) == (w["below"], w["above"])
        if band.dtype.kind in "iu":
            assert o["m2"] == 0.0
        elif np.isfinite(band[R.classes(band, nodata)[0]]).all():
            t = w["m2_terms"]
            err, bound = abs(o["m2"] - math.fsum(t)), (R.gamma(max(t.size - 1, 0)) + R.U) * math.fsum(t)
            print("  m2 error", err, "bound", bound)
            assert err <= bound


def both_passes(ctx, a, nodata, lo, hi, nbins, centre=0.0):
    check_stats(ctx.band_stats(a, nodata=nodata), a, nodata)
    counts, outs = ctx.band_histogram(a, lo, hi, nbins, nodata=nodata, centre=centre)
    check_hist(counts, outs, a, lo, hi, nbins, nodata, centre)


def mid_range(a):
    """A range that leaves pixels below and above (when the band has more than a few values)."""
    v = a[np.isfinite(a)] if a.dtype.kind == "f" else a
    if v.size == 0:
        return 0.0, 1.0
    lo, hi = float(np.percentile(v, 15)), float(np.percentile(v, 85))
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


# ---- both kernels against the restatement
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shapes(gpu_ctx, dtype):
    rng = np.random.default_rng(1)
    k = 0
    for w in (1, 7, 8, 9, 33, 300):
        for h in (1, 5, 40):
            nb = 1 + k % 3
            k += 1
            a = rand_band(rng, dtype, (nb, h, w))
            nd = float(a[0, h // 2, w // 2])
            lo, hi = mid_range(a)
            for nodata in (None, nd):
                both_passes(gpu_ctx, a, nodata, lo, hi, 1 + (k * 37) % 300, centre=float(a.mean()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_misaligned_strided_sub_views(gpu_ctx, dtype):
    """Windows of a larger buffer whose surround holds sentinels below the minimum, above the maximum and equal to the
    nodata value: one element read outside [height][width] changes a count, min or max."""
    rng = np.random.default_rng(2)
    dt = np.dtype(dtype)
    es = dt.itemsize
    for nb, h, w, r0, c0, H, W in [(1, 5, 9, 1, 1, 8, 16), (2, 7, 33, 2, 3, 11, 41), (3, 4, 70, 0, 5, 6, 77),
                                   (2, 9, 1, 3, 7, 14, 9), (1, 6, 40, 1, 8 // es + 1, 9, 64)]:
        inner = rand_band(rng, dtype, (nb, h, w), spread=200)
        nd = float(inner[0, 0, 0])
        big = np.empty((nb, H, W), dtype=dt)
        flat = big.reshape(-1)
        flat[0::3] = dt.type(np.iinfo(dt).min if dt.kind in "iu" else -1e30)
        flat[1::3] = dt.type(np.iinfo(dt).max if dt.kind in "iu" else 1e30)
        flat[2::3] = dt.type(nd)
        big[:, r0:r0 + h, c0:c0 + w] = inner
        view = big[:, r0:r0 + h, c0:c0 + w]
        lo, hi = mid_range(inner)
        # the same layout in device memory, at the host view's position within a 16-byte window
        off = (r0 * W + c0) * es
        shift = (view.ctypes.data - off) % 16
        buf = gpu_ctx.alloc(big.nbytes + 16)
        try:
            gpu_ctx._check(gpu_ctx.lib.frs_memcpy_h2d(gpu_ctx.handle, buf.ptr + shift, _native._p(big), big.nbytes))
            d = gpu_ctx.make_raster_desc(h, w, dt, nbands=nb, row_stride=W, band_stride=H * W)
            for nodata in (None, nd):
                hs = gpu_ctx.band_stats(view, nodata=nodata)
                check_stats(hs, inner, nodata)
                hc, ho = gpu_ctx.band_histogram(view, lo, hi, 17, nodata=nodata, centre=1.5)
                check_hist(hc, ho, inner, lo, hi, 17, nodata, 1.5)
                # the _device variant: identical bits, twice
                for _ in range(2):
                    assert gpu_ctx.band_stats_device(buf.ptr + shift + off, d, nodata=nodata) == hs
                    dc, do = gpu_ctx.band_histogram_device(buf.ptr + shift + off, d, lo, hi, 17, nodata=nodata,
                                                           centre=1.5)
                    assert dc.tobytes() == hc.tobytes() and do == ho
        finally:
            buf.close()


# ---- masks
def nodata_values(dt):
    if dt.kind == "f":
        return [float(np.finfo(dt).min), float(np.finfo(dt).max), 0.0, float("nan"), float("-inf")]
    ii = np.iinfo(dt)
    return [float(ii.min), float(ii.max), 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masks(gpu_ctx, dtype):
    rng = np.random.default_rng(3)
    dt = np.dtype(dtype)
    h, w = 21, 37
    yy, xx = np.mgrid[0:h, 0:w]
    collar = (yy < 3) | (yy >= h - 2) | (xx < 4) | (xx >= w - 5)
    one = np.ones((h, w), dtype=bool)
    one[h // 2, w // 3] = False
    masks = {"none": np.zeros((h, w), dtype=bool), "all": np.ones((h, w), dtype=bool), "one valid": one,
             "collar": collar, "checkerboard": (yy + xx) % 2 == 0}
    for nd in nodata_values(dt):
        ndt = dt.type(nd)
        for name, m in masks.items():
            a = rand_band(rng, dtype, (h, w), spread=100)
            # no accidental nodata among the valid pixels
            hit = R.classes(a, nd)[1]
            a[hit] = dt.type(7)
            a[m] = ndt
            assert int(R.classes(a, nd)[1].sum()) == int(m.sum()), name
            lo, hi = mid_range(a[~m]) if (~m).any() else (0.0, 1.0)
            both_passes(gpu_ctx, a, nd, lo, hi, 33, centre=3.0)
            both_passes(gpu_ctx, a, None if (dt.kind == "f" and nd != nd) else nd, lo, hi, 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_rasters_with_nan_and_inf(gpu_ctx, dtype):
    rng = np.random.default_rng(4)
    a = rand_band(rng, dtype, (2, 13, 29), spread=10)
    a[0, ::3, ::4] = np.nan
    a[0, 1, 1], a[0, 5, 7], a[1, 2, 2] = np.inf, -np.inf, np.inf
    a[1, 7, :] = -0.0
    for nodata in (None, float("nan"), float("inf"), float("-inf"), 0.0):
        both_passes(gpu_ctx, a, nodata, -5.0, 5.0, 40)
        s = gpu_ctx.band_stats(a, nodata=nodata)
        w0 = R.band_stats(a[0], nodata)
        assert s[0]["n_nan"] == w0["n_nan"] and (s[0]["min"], s[0]["max"]) == (w0["min"], w0["max"])


# ---- histograms and shapes
@pytest.mark.parametrize("nbins", [1, 2, 255, 256, 4096, 16384])
def test_bin_counts(gpu_ctx, nbins):
    rng = np.random.default_rng(nbins)
    for dtype in (np.int16, np.float32, np.uint32):
        a = rand_band(rng, dtype, (2, 50, 123), spread=30000)
        lo, hi = mid_range(a)
        counts, outs = gpu_ctx.band_histogram(a, lo, hi, nbins, nodata=float(a[0, 0, 0]))
        check_hist(counts, outs, a, lo, hi, nbins, float(a[0, 0, 0]))
        assert outs[0]["below"] > 0 and outs[0]["above"] > 0


def test_per_value_bins(gpu_ctx):
    from flac_raster_amd.stats import histogram_range
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (3, 64, 200)).astype(np.uint8)
    a[0, 0, :2] = (0, 255)
    lo, hi, nbins = histogram_range(a.dtype, 0, 255, 256)
    counts, outs = gpu_ctx.band_histogram(a, lo, hi, nbins)
    for c, band in zip(counts, a):
        assert c.tolist() == np.bincount(band.ravel(), minlength=256).tolist()
    b = rng.integers(-8000, 8384, (1, 80, 333)).astype(np.int16)
    b[0, 0, :2] = (-8000, 8383)
    lo, hi, nbins = histogram_range(b.dtype, -8000, 8383, 16384)
    assert nbins == 16384 and hi - lo == nbins
    counts, outs = gpu_ctx.band_histogram(b, lo, hi, nbins)
    assert counts[0].tolist() == np.bincount(b.ravel().astype(np.int64) + 8000, minlength=16384).tolist()
    assert outs[0]["below"] == 0 and outs[0]["above"] == 0
    check_hist(counts, outs, b, lo, hi, nbins, None)


def test_two_work_groups_and_a_second_grid_stride_step(gpu_ctx):
    """A shape, chosen with the mirrored launch constants, on which both kernels run several work-groups per band and
    every work-group takes a second grid-stride step."""
    N = _native
    nb, h, w = 8, 2100, 2048
    items = N.stats_items(h, w, 1)
    for block, unroll, cap in ((N.STATS_BLOCK, N.STATS_UNROLL, N.STATS_MAX_GROUPS),
                               (N.HIST_BLOCK, N.HIST_UNROLL, N.HIST_MAX_GROUPS)):
        gx = N.stats_groups(items, nb, block, unroll, cap)
        assert gx >= 2 and items > gx * block * unroll  # more than one step per work-group
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (nb, h, w)).astype(np.uint8)
    a[:, :40, :] = 255  # a collar of nodata
    check_stats(gpu_ctx.band_stats(a, nodata=255.0), a, 255.0)
    counts, outs = gpu_ctx.band_histogram(a, 0.0, 255.0, 255, nodata=255.0)
    for c, o, band in zip(counts, outs, a):
        assert c.tolist() == np.bincount(band[40:].ravel(), minlength=256)[:255].tolist()
        assert (o["below"], o["above"], o["m2"]) == (0, 0, 0.0)


def test_32_bit_carries(gpu_ctx):
    a = np.full((1, 1, 8), -2 ** 31, dtype=np.int32)  # the squares add up to 2^65
    s = gpu_ctx.band_stats(a)[0]
    assert s["isq"] == 8 * 2 ** 62 and s["isum"] == -8 * 2 ** 31 and s["sum"] == -8.0 * 2 ** 31
    b = np.full((2, 37, 91), 2 ** 32 - 1, dtype=np.uint32)
    b[1, ::2] = 0
    check_stats(gpu_ctx.band_stats(b), b, None)
    assert gpu_ctx.band_stats(b)[0]["isq"] == 37 * 91 * (2 ** 32 - 1) ** 2 > 2 ** 64
    c = np.full((1, 300, 300), -2 ** 31, dtype=np.int32)
    c[0, 5, 5] = 2 ** 31 - 1
    check_stats(gpu_ctx.band_stats(c, nodata=0.0), c, 0.0)


# ---- exactness of repetition
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16], ids=["float32", "float64", "int16"])
def test_two_calls_and_both_variants_return_identical_bits(gpu_ctx, dtype):
    rng = np.random.default_rng(10)
    a = rand_band(rng, dtype, (3, 200, 301))
    nd = float(a[1, 1, 1])
    lo, hi = mid_range(a)
    hs = gpu_ctx.band_stats(a, nodata=nd, as_dicts=False)
    hc, ho = gpu_ctx.band_histogram(a, lo, hi, 100, nodata=nd, centre=0.25)
    buf = gpu_ctx.alloc(a.nbytes)
    try:
        buf.upload(a)
        d = gpu_ctx.make_raster_desc(200, 301, a.dtype, nbands=3)
        for _ in range(2):
            ds = gpu_ctx.band_stats_device(buf.ptr, d, nodata=nd, as_dicts=False)
            assert [bytes(x) for x in ds] == [bytes(x) for x in hs]
            dc, do = gpu_ctx.band_histogram_device(buf.ptr, d, lo, hi, 100, nodata=nd, centre=0.25)
            assert dc.tobytes() == hc.tobytes()
            assert [np.float64(x["m2"]).tobytes() for x in do] == [np.float64(x["m2"]).tobytes() for x in ho]
            assert do == ho
    finally:
        buf.close()
    assert [bytes(x) for x in gpu_ctx.band_stats(a, nodata=nd, as_dicts=False)] == [bytes(x) for x in hs]


# ---- argument errors
def test_argument_errors_leave_the_destination_untouched(gpu_ctx):
    ctx, L = gpu_ctx, gpu_ctx.lib
    a = np.arange(64 * 64, dtype=np.int16).reshape(1, 64, 64)
    buf = ctx.alloc(a.nbytes + 64)
    try:
        buf.upload(a)
        good = ctx.make_raster_desc(64, 64, np.int16)
        out = (_native.BandStatsOut * 8)()
        hout = (_native.BandHistOut * 8)()
        counts = np.full(8 * 16384, 0xABABABABABABABAB, dtype=np.uint64)
        ctypes.memset(out, 0xAB, ctypes.sizeof(out))
        ctypes.memset(hout, 0xAB, ctypes.sizeof(hout))
        before = (bytes(out), bytes(hout), counts.tobytes())
        cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        nd = lambda v: ctypes.byref(ctypes.c_double(v))  # noqa: E731
        hp = lambda lo, hi, n, c=0.0: ctypes.byref(_native.HistParams(lo, hi, n, c))  # noqa: E731
        ptr, host = ctypes.c_void_p(buf.ptr), _native._p(a)

        def desc(**kw):
            d = ctx.make_raster_desc(64, 64, np.int16)
            for k, v in kw.items():
                setattr(d, k, v)
            return ctypes.byref(d)

        huge = ctx.make_raster_desc(2 ** 31, 2 ** 11, np.uint8)  # 2^31 elements per work-group: past the exactness bound
        stats_cases = [
            (ctypes.byref(good), None, None), (ctypes.byref(good), ctypes.c_void_p(buf.ptr + 1), None),
            (ctypes.byref(good), ptr, nd(0.5)), (ctypes.byref(good), ptr, nd(40000.0)),
            (ctypes.byref(good), ptr, nd(float("nan"))), (None, ptr, None),
            (desc(height=0), ptr, None), (desc(width=0), ptr, None), (desc(row_stride=63), ptr, None),
            (desc(nbands=0), ptr, None), (desc(nbands=9), ptr, None), (desc(dtype=0), ptr, None),
            (desc(nbands=2, band_stride=100), ptr, None), (ctypes.byref(huge), ptr, None),
        ]
        for fn in (L.frs_band_stats_device, L.frs_band_stats):
            for d, p, n in stats_cases:
                if fn is L.frs_band_stats and p is ptr:
                    p = host
                if fn is L.frs_band_stats and d is not None and d._obj is huge:
                    continue  # (the host variant would be handed a host pointer for 2^42 elements: the device form covers it)
                assert fn(ctx.handle, d, p, n, out) == -1, ctx.last_error()
            assert fn(ctx.handle, ctypes.byref(good), ptr if fn is L.frs_band_stats_device else host, None, None) == -1
        hist_cases = [
            hp(0.0, 1.0, 0), hp(0.0, 1.0, -1), hp(0.0, 1.0, 16385), hp(float("nan"), 1.0, 4), hp(0.0, float("inf"), 4),
            hp(float("-inf"), 0.0, 4), hp(0.0, 1.0, 4, float("nan")), hp(0.0, 1.0, 4, float("inf")), hp(1.0, 1.0, 4),
            hp(2.0, 1.0, 4), hp(-1.7e308, 1.7e308, 4), None,
        ]
        for fn in (L.frs_band_histogram_device, L.frs_band_histogram):
            p = ptr if fn is L.frs_band_histogram_device else host
            for h in hist_cases:
                assert fn(ctx.handle, ctypes.byref(good), p, None, h, cp, hout) == -1, ctx.last_error()
            ok = hp(0.0, 100.0, 16)
            for d, pp, n in stats_cases[:6]:
                if pp is ptr:
                    pp = p
                assert fn(ctx.handle, d, pp, n, ok, cp, hout) == -1, ctx.last_error()
            assert fn(ctx.handle, ctypes.byref(good), p, None, ok, None, hout) == -1
            assert fn(ctx.handle, ctypes.byref(good), p, None, ok, cp, None) == -1
        assert L.frs_band_histogram_device(ctx.handle, ctypes.byref(huge), ptr, None, hp(0.0, 255.0, 16), cp, hout) == -1
        assert "2^30" in ctx.last_error()
        assert (bytes(out), bytes(hout), counts.tobytes()) == before
        # and the context still works
        check_stats(ctx.band_stats_device(buf.ptr, good), a, None)
    finally:
        buf.close()
    with pytest.raises(_native.FrsError):
        ctx.band_stats(np.zeros((9, 4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        ctx.band_stats(np.zeros((0, 4), dtype=np.uint8))
