"""frs_compare on the GPU against numpy itself: the reference's expressions (compare.py:55-78) restated here.

Integer cases assert exact equality: every sum below is under 2**53, where numpy's float64 mean of an integer array is
the exact sum divided by the count, and the library's is the correctly rounded exact sum divided by the count.  Float
sums are bounded by count * 2**-53 relative, the worst case of any summation order of non-negative terms."""
import json
import math

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, geotiff
from flac_raster_amd.cli import app
from flac_raster_amd.compare import compare_arrays, compare_tiffs

pytestmark = pytest.mark.gpu
runner = CliRunner()

INT_DTYPES = [np.uint8, np.uint16, np.int16, np.int32, np.uint32]
HEADER_KEYS = ["file1", "file2", "shape_match", "dtype_match", "crs_match", "file1_shape", "file2_shape", "file1_dtype",
               "file2_dtype", "file1_crs", "file2_crs"]
STAT_KEYS = ["arrays_equal", "max_difference", "mean_difference", "rmse", "file1_min", "file1_max", "file2_min",
             "file2_max"]


def _as3(x):
    return x if x.ndim == 3 else x[None]


def check_int(bands, a, b):
    """Every field of every band record against numpy on the (dense) arrays a, b of one integer dtype."""
    a, b = _as3(a), _as3(b)
    assert len(bands) == a.shape[0]
    with np.errstate(all="ignore"):
        for r, x, y in zip(bands, a, b):
            ne = (x != y).ravel()
            d = x - y  # wraps in the dtype
            t = np.abs(x.astype(np.int64) - y.astype(np.int64))
            got = {k: r[k] for k in r}
            print(x.dtype, x.shape, got)
            assert r["count"] == x.size
            assert r["n_diff"] == int(ne.sum())
            assert r["first_diff"] == (int(np.argmax(ne)) if ne.any() else -1)
            assert (r["a_min"], r["a_max"], r["b_min"], r["b_max"]) == (float(x.min()), float(x.max()), float(y.min()),
                                                                        float(y.max()))
            assert r["np_max_abs"] == float(np.max(np.abs(d)))
            assert r["np_sum_abs"] / r["count"] == float(np.mean(np.abs(d)))
            want_rmse = float(np.sqrt(np.mean(d ** 2)))
            ss = r["np_sum_sq"] / r["count"]
            got_rmse = math.sqrt(ss) if ss >= 0 else float("nan")
            assert got_rmse == want_rmse or (math.isnan(got_rmse) and math.isnan(want_rmse))
            assert r["max_abs"] == float(t.max())
            assert r["sum_abs"] == float(t.sum())


def _core(dtype):
    """(min, max), (max, min), (5, 10), (10, 5), (0, 0) and for int16 a difference of 300 (its square wraps)."""
    ii = np.iinfo(dtype)
    a = [ii.min, ii.max, 5, 10, 0]
    b = [ii.max, ii.min, 10, 5, 0]
    if dtype == np.int16:
        a.append(400)
        b.append(100)
    return np.array(a, dtype=dtype), np.array(b, dtype=dtype)


def test_numpy_quirks_the_kernel_reproduces():
    """The literals the cases rest on, from numpy itself (no GPU involved in this one)."""
    a, b = _core(np.uint8)
    assert float(np.max(np.abs(a - b))) == 255.0 and float(np.mean(np.abs(a - b))) == 102.4
    assert np.abs(np.int16(-32768)) == -32768
    assert (np.array([300], np.int16) ** 2)[0] == 24464


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_wrap_and_extreme_vectors(gpu_ctx, dtype):
    ca, cb = _core(dtype)
    check_int(gpu_ctx.compare_host(ca[None, :], cb[None, :]), ca[None, :], cb[None, :])  # the bare core
    rng = np.random.default_rng(5)
    ii = np.iinfo(dtype)
    # padded to 1 x 67: the core at the start, in the middle of the vector body and at the end
    a = rng.integers(ii.min, ii.max, size=(1, 67), dtype=dtype, endpoint=True)
    b = a.copy()
    b[0, 20:40] = rng.integers(ii.min, ii.max, size=20, dtype=dtype, endpoint=True)
    n = len(ca)
    for at in (0, 30, 67 - n):
        a[0, at:at + n], b[0, at:at + n] = ca, cb
    check_int(gpu_ctx.compare_host(a, b), a, b)
    if dtype == np.uint8:
        r = gpu_ctx.compare_host(ca[None, :], cb[None, :])[0]
        assert r["np_max_abs"] == 255.0 and r["np_sum_abs"] / r["count"] == 102.4 and r["max_abs"] == 255.0
    if dtype == np.int16:
        r = gpu_ctx.compare_host(np.array([[300]], np.int16), np.array([[0]], np.int16))[0]
        assert r["np_sum_sq"] == 24464.0 and r["np_max_abs"] == 300.0
        r = gpu_ctx.compare_host(np.array([[-32768, -32768]], np.int16), np.array([[0, 0]], np.int16))[0]
        assert r["np_max_abs"] == -32768.0 and r["max_abs"] == 32768.0  # abs(min) stays min in the dtype


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_shapes_small(gpu_ctx, dtype):
    rng = np.random.default_rng(11)
    ii = np.iinfo(dtype)
    a = rng.integers(ii.min, ii.max, size=(1, 1), dtype=dtype, endpoint=True)
    check_int(gpu_ctx.compare_host(a, a.copy()), a, a.copy())
    b = a.copy()
    b[0, 0] ^= 1
    check_int(gpu_ctx.compare_host(a, b), a, b)
    a = rng.integers(ii.min, ii.max, size=(3, 7, 13), dtype=dtype, endpoint=True)
    b = a.copy()
    m = rng.random(a.shape) < 0.3
    b[m] = rng.integers(ii.min, ii.max, size=int(m.sum()), dtype=dtype, endpoint=True)
    b[1] = a[1]  # one equal band
    check_int(gpu_ctx.compare_host(a, b), a, b)


def test_single_difference_in_second_band(gpu_ctx):
    rng = np.random.default_rng(3)
    a = rng.integers(-32768, 32767, size=(2, 257, 1031), dtype=np.int16, endpoint=True)
    b = a.copy()
    b[1, 200, 1000] = a[1, 200, 1000] ^ 0x55
    bands = gpu_ctx.compare_host(a, b)
    check_int(bands, a, b)
    assert bands[0]["n_diff"] == 0 and bands[0]["first_diff"] == -1
    assert bands[1]["n_diff"] == 1 and bands[1]["first_diff"] == 200 * 1031 + 1000
    res = compare_arrays(a, b, ctx=gpu_ctx)
    assert [x["equal"] for x in res["bands"]] == [True, False]
    assert res["arrays_equal"] is False and res["exact"]["first_difference"] == [1, 200, 1000]
    assert res["exact"]["n_different"] == 1 and res["exact"]["max_difference"] == float(abs(int(a[1, 200, 1000]) -
                                                                                           int(b[1, 200, 1000])))


def test_second_grid_stride_iteration_uint8(gpu_ctx):
    """One dense uint8 band just large enough that work-groups take a second grid-stride step: the group count is
    capped at COMPARE_MAX_GROUPS, each step covers COMPARE_BLOCK * COMPARE_UNROLL 16-byte vectors."""
    step = _native.COMPARE_BLOCK * _native.COMPARE_UNROLL * 16  # uint8 elements per work-group step
    n = _native.COMPARE_MAX_GROUPS * step + 2 * step + 7
    assert n <= 64 << 20
    assert _native.compare_groups(n, 1, 1) == _native.COMPARE_MAX_GROUPS
    assert -(-n // step) > _native.COMPARE_MAX_GROUPS  # more steps than groups: some group takes a second one
    rng = np.random.default_rng(9)
    a = rng.integers(0, 255, size=(1, 1, n), dtype=np.uint8, endpoint=True)
    b = a.copy()
    b[0, 0, -1] = a[0, 0, -1] ^ 0x80
    r = gpu_ctx.compare_host(a, b)[0]
    print(r)
    assert r["count"] == n and r["n_diff"] == 1 and r["first_diff"] == n - 1
    assert (r["a_min"], r["a_max"]) == (float(a.min()), float(a.max()))
    assert (r["b_min"], r["b_max"]) == (float(b.min()), float(b.max()))
    assert r["np_max_abs"] == 128.0 and r["np_sum_abs"] == 128.0 and r["max_abs"] == 128.0 and r["sum_abs"] == 128.0
    assert r["np_sum_sq"] == 0.0 == float((np.array([128], np.uint8) ** 2)[0])  # 128**2 wraps to 0 in uint8
    # and an unequal pair of the same size through the difference path of every step
    b2 = np.bitwise_xor(a, np.uint8(3))
    r2 = gpu_ctx.compare_host(a, b2)[0]
    d = a - b2
    assert r2["n_diff"] == n and r2["first_diff"] == 0
    assert r2["np_sum_abs"] == float(np.abs(d).sum(dtype=np.int64))
    assert r2["np_sum_sq"] == float((d ** 2).sum(dtype=np.int64))
    assert r2["sum_abs"] == float(np.abs(a.astype(np.int16) - b2.astype(np.int16)).sum(dtype=np.int64))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32])
def test_windows_of_larger_arrays(gpu_ctx, dtype):
    rng = np.random.default_rng(21)
    ii = np.iinfo(dtype)
    h, w = 37, 61
    big = rng.integers(ii.min, ii.max, size=(3, 50, 80), dtype=dtype, endpoint=True)
    win = big[:, 3:3 + h, 5:5 + w]
    assert not win.flags.c_contiguous
    other = np.ascontiguousarray(win).copy()
    m = rng.random(other.shape) < 0.1
    other[m] = rng.integers(ii.min, ii.max, size=int(m.sum()), dtype=dtype, endpoint=True)
    dense = gpu_ctx.compare_host(np.ascontiguousarray(win), other)
    check_int(dense, np.ascontiguousarray(win), other)
    assert gpu_ctx.compare_host(win, other) == dense           # A a window, B dense
    swapped = gpu_ctx.compare_host(other, np.ascontiguousarray(win))
    assert gpu_ctx.compare_host(other, win) == swapped         # the other way round
    # both windows, rows 16-byte aligned (the per-row vector path): 64-column windows of a 96-column parent
    big2 = rng.integers(ii.min, ii.max, size=(2, 40, 96), dtype=dtype, endpoint=True)
    big3 = big2.copy()
    big3[:, ::3, ::5] ^= 1
    wa, wb = big2[:, 2:35, 16:16 + 67], big3[:, 2:35, 16:16 + 67]
    da, db = np.ascontiguousarray(wa), np.ascontiguousarray(wb)
    check_int(gpu_ctx.compare_host(wa, wb), da, db)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_device_pointers_one_element_off_alignment(gpu_ctx, dtype):
    rng = np.random.default_rng(4)
    shape = (2, 33, 129)
    ii = np.iinfo(dtype)
    a = rng.integers(ii.min, ii.max, size=shape, dtype=dtype, endpoint=True)
    b = a.copy()
    b[:, ::2, ::3] ^= 5
    es = np.dtype(dtype).itemsize
    da, db = gpu_ctx.alloc(a.nbytes + 64), gpu_ctx.alloc(b.nbytes + 64)
    try:
        assert da.ptr % 16 == 0 and db.ptr % 16 == 0
        da.upload(a.view(np.uint8).ravel(), es)
        db.upload(b.view(np.uint8).ravel(), es)
        desc = gpu_ctx.make_compare_desc(shape[1], shape[2], dtype, nbands=shape[0])
        got = gpu_ctx.compare_device(da.ptr + es, db.ptr + es, desc)
        # B alone off by one element: A and B misaligned differently (scalar loop)
        db.upload(b.view(np.uint8).ravel(), 2 * es)
        got2 = gpu_ctx.compare_device(da.ptr + es, db.ptr + 2 * es, desc)
    finally:
        da.close()
        db.close()
    want = gpu_ctx.compare_host(a, b)
    assert got == want and got2 == want
    check_int(got, a, b)


def _float_pair(dtype, seed=7):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((2, 129, 257)).astype(dtype)
    b = rng.standard_normal((2, 129, 257)).astype(dtype)
    b[1, :64] = a[1, :64]  # first difference of band 2 is at row 64
    return a, b


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_floats_against_numpy(gpu_ctx, dtype):
    a, b = _float_pair(dtype)
    bands = gpu_ctx.compare_host(a, b)
    for r, x, y in zip(bands, a, b):
        ne = (x != y).ravel()
        d = x - y                     # in the dtype
        ad, sq = np.abs(d), d * d     # in the dtype
        assert sq.dtype == dtype
        n = x.size
        bound = n * 2.0 ** -53
        want_abs, want_sq = float(np.sum(ad, dtype=np.float64)), float(np.sum(sq, dtype=np.float64))
        want_true = float(np.sum(np.abs(x.astype(np.float64) - y.astype(np.float64))))
        print(dtype, "rel err abs/sq/true", abs(r["np_sum_abs"] - want_abs) / want_abs,
              abs(r["np_sum_sq"] - want_sq) / want_sq, abs(r["sum_abs"] - want_true) / want_true, "bound", bound)
        assert r["count"] == n and r["n_diff"] == int(ne.sum()) and r["first_diff"] == int(np.argmax(ne))
        assert (r["a_min"], r["a_max"], r["b_min"], r["b_max"]) == (float(x.min()), float(x.max()), float(y.min()),
                                                                    float(y.max()))
        assert r["np_max_abs"] == float(np.max(ad))
        assert r["max_abs"] == float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64))))
        assert abs(r["np_sum_abs"] - want_abs) <= bound * want_abs
        assert abs(r["np_sum_sq"] - want_sq) <= bound * want_sq
        assert abs(r["sum_abs"] - want_true) <= bound * want_true
    assert bands[1]["first_diff"] == 64 * 257


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_nan_and_signed_zero(gpu_ctx, dtype):
    a, b = _float_pair(dtype)
    b = a.copy()
    a[0, 77, 100] = np.nan
    res = compare_arrays(a, b, ctx=gpu_ctx)
    r = gpu_ctx.compare_host(a, b)
    assert res["arrays_equal"] is False and res["bands"][0]["equal"] is False and res["bands"][1]["equal"] is True
    for k in ("a_min", "a_max", "np_max_abs", "np_sum_abs", "np_sum_sq", "max_abs", "sum_abs"):
        assert math.isnan(r[0][k]), k
    assert r[0]["b_min"] == float(b[0].min()) and r[0]["b_max"] == float(b[0].max())
    assert r[0]["n_diff"] == 1 and r[0]["first_diff"] == 77 * 257 + 100
    assert r[1]["n_diff"] == 0 and r[1]["np_max_abs"] == 0.0 and not math.isnan(r[1]["a_min"])
    for k in ("max_difference", "mean_difference", "rmse", "file1_min", "file1_max"):
        assert math.isnan(res[k]), k
    assert res["file2_min"] == float(b.min())
    # -0.0 against 0.0 is equal
    z = np.zeros((1, 5, 9), dtype)
    r = gpu_ctx.compare_host(z, -z)[0]
    assert r["n_diff"] == 0 and r["first_diff"] == -1 and r["np_max_abs"] == 0.0 and r["sum_abs"] == 0.0


def test_float_results_are_bitwise_reproducible(gpu_ctx):
    a, b = _float_pair(np.float32, seed=8)
    first = gpu_ctx.compare_host(a, b, as_dicts=False)
    again = gpu_ctx.compare_host(a, b, as_dicts=False)
    assert [bytes(x) for x in first] == [bytes(x) for x in again]


def test_fixture_pairs_through_compare_tiffs(gpu_ctx, golden):
    res = compare_tiffs(golden / "sample_rgb.tif", golden / "sample_rgb_reconstructed.tif")
    assert list(res) == HEADER_KEYS + STAT_KEYS + ["bands", "exact"]
    assert res["arrays_equal"] is True and res["shape_match"] and res["dtype_match"]
    assert res["max_difference"] == 0.0 and res["mean_difference"] == 0.0 and res["rmse"] == 0.0
    assert len(res["bands"]) == 3 and all(b["equal"] and b["max_diff"] == 0.0 and b["mean_diff"] == 0.0
                                          for b in res["bands"])
    assert res["exact"] == {"n_different": 0, "max_difference": 0.0, "mean_difference": 0.0, "first_difference": None}
    a = geotiff.read(golden / "sample_rgb.tif").data
    assert (res["file1_min"], res["file1_max"]) == (float(a.min()), float(a.max()))

    # the lossy raw-frames pair
    res = compare_tiffs(golden / "sample_dem.tif", golden / "sample_dem_reconstructed.tif")
    a = geotiff.read(golden / "sample_dem.tif").data
    b = geotiff.read(golden / "sample_dem_reconstructed.tif").data
    assert res["arrays_equal"] is False
    assert res["max_difference"] == 50.0 == float(np.max(np.abs(a - b)))
    assert res["mean_difference"] == 16.67731475830078 == float(np.mean(np.abs(a - b)))
    assert res["rmse"] == 20.432674106503487 == float(np.sqrt(np.mean((a - b) ** 2)))
    assert res["exact"]["n_different"] == 256773 == int((a != b).sum())
    assert (res["file1_min"], res["file1_max"], res["file2_min"], res["file2_max"]) == (
        float(np.min(a)), float(np.max(a)), float(np.min(b)), float(np.max(b)))
    for i, bd in enumerate(res["bands"]):
        assert bd["band"] == i + 1 and bd["equal"] == bool(np.array_equal(a[i], b[i]))
        assert bd["max_diff"] == float(np.max(np.abs(a[i] - b[i])))
        assert bd["mean_diff"] == float(np.mean(np.abs(a[i] - b[i])))
        assert bd["file1_range"] == [float(a[i].min()), float(a[i].max())]
        assert bd["file2_range"] == [float(b[i].min()), float(b[i].max())]
    idx = np.argwhere(a != b)[0]
    assert res["exact"]["first_difference"] == [int(v) for v in idx]


def test_mixed_dtypes(gpu_ctx):
    rng = np.random.default_rng(2)
    a = rng.integers(0, 255, size=(2, 19, 23), dtype=np.uint8, endpoint=True)
    b = rng.integers(-300, 300, size=(2, 19, 23), dtype=np.int16, endpoint=True)
    res = compare_arrays(a, b, ctx=gpu_ctx)
    pa, pb = a.astype(np.int16), b
    assert np.result_type(a.dtype, b.dtype) == np.int16
    assert res["dtype_match"] is False and res["arrays_equal"] == bool(np.array_equal(a, b))
    assert res["max_difference"] == float(np.max(np.abs(a - b))) == float(np.max(np.abs(pa - pb)))
    assert res["mean_difference"] == float(np.mean(np.abs(a - b)))
    assert res["rmse"] == float(np.sqrt(np.mean((a - b) ** 2)))
    assert res["file1_min"] == float(a.min()) and res["file2_max"] == float(b.max())
    with pytest.raises(ValueError):
        compare_arrays(a.astype(np.int32), b.astype(np.uint32), ctx=gpu_ctx)


def test_cli_compare_and_export(gpu_ctx, golden, tmp_path):
    out = tmp_path / "cmp.json"
    r = runner.invoke(app, ["compare", str(golden / "sample_rgb.tif"), str(golden / "sample_rgb_reconstructed.tif"),
                            "--export", str(out)])
    assert r.exit_code == 0, r.output
    assert "Arrays Equal" in r.output and "YES" in r.output and "Exact Differences" in r.output
    back = json.loads(out.read_text())
    assert list(back) == HEADER_KEYS + STAT_KEYS + ["bands", "exact"]
    assert back["arrays_equal"] is True and back["file1_shape"] == [3, 256, 256]
    r = runner.invoke(app, ["compare", str(golden / "sample_rgb.tif"), str(golden / "sample_rgb_reconstructed.tif"),
                            "--no-bands", "--export", str(out)])
    assert r.exit_code == 0 and "Per-Band Statistics" not in r.output
    assert list(json.loads(out.read_text())) == HEADER_KEYS + STAT_KEYS + ["exact"]


def test_cli_convert_verify(gpu_ctx, golden, tmp_path):
    r = runner.invoke(app, ["convert", str(golden / "sample_rgb.tif"), "--verify", "-o", str(tmp_path / "rgb.flac")])
    assert r.exit_code == 0, r.output
    assert "VERIFY: lossless" in r.output
    # float32 samples go through a 24-bit quantisation and back as they are: not lossless
    tif = tmp_path / "f32.tif"
    geotiff.write(tif, np.random.default_rng(1).random((1, 64, 64), dtype=np.float32))
    r = runner.invoke(app, ["convert", str(tif), "--verify", "-o", str(tmp_path / "f32.flac")])
    assert r.exit_code == 3, r.output
    assert "VERIFY: differs (n_different=" in r.output and (tmp_path / "f32.flac").exists()


def test_argument_errors_are_rejected_on_the_host(gpu_ctx):
    a = np.zeros((1, 4, 8), np.int16)
    for kw in ({"a_row_stride": 7}, {"b_row_stride": 7}):
        desc = gpu_ctx.make_compare_desc(4, 8, np.int16, **kw)
        out = (_native.CompareBand * 1)()
        import ctypes
        rc = gpu_ctx.lib.frs_compare(gpu_ctx.handle, ctypes.byref(desc), a.ctypes.data_as(ctypes.c_void_p),
                                     a.ctypes.data_as(ctypes.c_void_p), out)
        assert rc == -1  # FRS_E_ARG, before any copy or launch
        buf = gpu_ctx.alloc(256)
        try:
            with pytest.raises(_native.FrsError) as e:
                gpu_ctx.compare_device(buf.ptr, buf.ptr, desc)
            assert e.value.code == -1
        finally:
            buf.close()
    # the last one: 2**42 uint8 elements in one band would put 2**31 elements on one work-group, past the bound that
    # keeps its 64-bit partial sums from overflowing -- rejected from the shape alone, nothing is read
    for bad in ({"height": 0}, {"width": 0}, {"nbands": 0}, {"dtype": 99},
                {"dtype": 1, "height": 1 << 21, "width": 1 << 21, "a_row_stride": 1 << 21, "b_row_stride": 1 << 21}):
        desc = gpu_ctx.make_compare_desc(4, 8, np.int16)
        for k, v in bad.items():
            setattr(desc, k, v)
        buf = gpu_ctx.alloc(256)
        try:
            with pytest.raises(_native.FrsError) as e:
                gpu_ctx.compare_device(buf.ptr, buf.ptr, desc)
            assert e.value.code == -1
        finally:
            buf.close()
