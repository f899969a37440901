"""frs_render_shaded_window* on the GPU against the numpy restatement (tests/shade_ref.py), bit for bit, on the shapes
of tests/test_shade_host.py (tests/shade_cases.py): destinations around the kernel's tile, rectangles over the raster's
edges, a one-byte lead with an odd row stride, every channel count and LUT length."""
import ctypes

import numpy as np
import pytest

from tests import shade_cases as SC
from tests.render_cases import PAD, SRC_H, SRC_W, limits, lut_of, nodata_of

pytestmark = pytest.mark.gpu

FULL = ("int16", "uint8", "float32", "float64")  # every mode; the others in one
COMBOS = [(d, m) for d in FULL for m in ("nearest", "bilinear", "average")] + \
         [("uint16", "bilinear"), ("int32", "average"), ("uint32", "nearest")]


@pytest.fixture(scope="module")
def ctx():
    from flac_raster_amd import _native
    with _native.Context(0) as c:
        yield c


def _upload_source(ctx, dt, masked):
    a = SC.source(dt.name, masked)
    srs = SRC_W + PAD
    flat = np.zeros((SRC_H - 1) * srs + SRC_W, dtype=dt)
    np.lib.stride_tricks.as_strided(flat, shape=(SRC_H, SRC_W), strides=(srs * dt.itemsize, dt.itemsize))[...] = a
    buf = ctx.alloc(flat.nbytes)
    buf.upload(flat)
    return buf, ctx.make_raster_desc(SRC_H, SRC_W, dt, row_stride=srs)


def _run_case(ctx, sbuf, sd, dt, mode, masked, case, tab, shaded=True):
    C, n, rgba, rect, h, w, drs, lead, want = case
    lo, hi = limits(dt)
    kx, ky = SC.scales(dt)
    host = np.full(len(want) + 16, 0xA5, dtype=np.uint8)
    dbuf = ctx.alloc(host.nbytes)
    try:
        dbuf.upload(host)
        nd = nodata_of(dt) if masked else None
        if shaded:
            ctx.render_shaded_window_device(sbuf.ptr, sd, dbuf.ptr + lead, h, w, rect, mode, lo, hi, lut_of(4096)[:n],
                                            SC.LIGHT, kx, ky, tab, nodata_rgba=rgba, channels=C, nodata=nd,
                                            dst_row_stride=drs)
        else:
            ctx.render_window_device(sbuf.ptr, sd, dbuf.ptr + lead, h, w, rect, mode, lo, hi, lut_of(4096)[:n],
                                     nodata_rgba=rgba, channels=C, nodata=nd, dst_row_stride=drs)
        dbuf.download(out=host)
    finally:
        dbuf.close()
    assert (host[len(want):] == 0xA5).all()
    return host[:len(want)]


@pytest.mark.parametrize("dtype,mode", COMBOS)
def test_device_call_equals_the_restatement(ctx, dtype, mode):
    dt = np.dtype(dtype)
    for masked in (False, True):
        sbuf, sd = _upload_source(ctx, dt, masked)
        try:
            for case in SC.cases(dt.name, mode, masked):
                got = _run_case(ctx, sbuf, sd, dt, mode, masked, case, SC.table())
                if not np.array_equal(got, case[-1]):
                    bad = int(np.flatnonzero(got != case[-1])[0])
                    raise AssertionError((masked, case[:8], bad, int(got[bad]), int(case[-1][bad])))
        finally:
            sbuf.close()


def test_strength_zero_equals_render_window_device(ctx):
    dt = np.dtype(np.int16)
    sbuf, sd = _upload_source(ctx, dt, True)
    try:
        for mode in ("nearest", "bilinear", "average"):
            for case in SC.cases(dt.name, mode, True):
                a = _run_case(ctx, sbuf, sd, dt, mode, True, case, np.full(256, 255, dtype=np.uint8))
                b = _run_case(ctx, sbuf, sd, dt, mode, True, case, None, shaded=False)
                assert np.array_equal(a, b), case[:8]
    finally:
        sbuf.close()


def test_lut_of_256_and_of_4096_entries(ctx):
    """the table in LDS and the table in global memory"""
    dt = np.dtype(np.float32)
    ns = {c[1] for c in SC.cases(dt.name, "bilinear", False)}
    assert {256, 4096} <= ns  # (compared in test_device_call_equals_the_restatement)
    sbuf, sd = _upload_source(ctx, dt, False)
    try:
        for case in SC.cases(dt.name, "bilinear", False):
            if case[1] in (256, 4096) and case[0] == 4:
                assert np.array_equal(_run_case(ctx, sbuf, sd, dt, "bilinear", False, case, SC.table()), case[-1])
    finally:
        sbuf.close()


def test_host_rasters_with_destination_padding_preserved(ctx):
    dt = np.dtype(np.int16)
    case = next(c for c in SC.cases(dt.name, "average", True) if c[0] == 2 and c[6] > c[5] * 2 and c[7] == 0)
    C, n, rgba, rect, h, w, drs, lead, want = case
    lo, hi = limits(dt)
    kx, ky = SC.scales(dt)
    out = np.full(len(want), 0xA5, dtype=np.uint8)
    got = ctx.render_shaded_window(SC.source(dt.name, True), rect, out, "average", lo, hi, lut_of(4096)[:n], SC.LIGHT,
                                   kx, ky, SC.table(), nodata_rgba=rgba, channels=C, nodata=nodata_of(dt),
                                   dst_row_stride=drs, out_shape=(h, w))
    assert np.array_equal(got, want)


def test_every_rejected_argument_leaves_the_destination_untouched(ctx):
    from flac_raster_amd import _native as N
    dt = np.dtype(np.int16)
    sbuf, sd = _upload_source(ctx, dt, False)
    h, w, C = 5, 7, 4
    host = np.full(h * w * C, 0xA5, dtype=np.uint8)
    dbuf = ctx.alloc(host.nbytes)
    lut = lut_of(256)
    tab = SC.table()
    good = dict(rect=(0.0, 0.0, float(SRC_W), float(SRC_H)), mode="average", lo=0.0, hi=10.0, lut=lut, light=SC.LIGHT,
                kx=0.1, ky=0.1, table=tab, channels=C)
    try:
        dbuf.upload(host)
        bad = []
        for name in ("kx", "ky"):
            for v in (np.inf, -np.inf, np.nan):
                bad.append({**good, name: v})
        for i in range(3):
            for v in (np.inf, np.nan):
                l = list(SC.LIGHT)
                l[i] = v
                bad.append({**good, "light": tuple(l)})
        bad += [{**good, "channels": 3}, {**good, "hi": 0.0}, {**good, "lo": np.nan},
                {**good, "rect": (0.0, 0.0, -1.0, 5.0)}, {**good, "lut": np.zeros((0, 4), dtype=np.uint8)}]
        E_ARG = -1
        for kw in bad:
            with pytest.raises(N.FrsError) as e:
                ctx.render_shaded_window_device(sbuf.ptr, sd, dbuf.ptr, h, w, **kw)
            assert e.value.code == E_ARG, kw
        # a null table, a null shade, a null render: straight through the C ABI
        rp, keep = ctx._render_params(0.0, 10.0, lut, 0, C)
        sp = N.ShadeParams(*SC.LIGHT, 0.1, 0.1, None)
        dd = ctx.make_raster_desc(h, w, np.uint8, row_stride=w * C)
        m = ctx._window_map(good["rect"], 0.0)
        call = lambda r, s: ctx.lib.frs_render_shaded_window_device(
            ctx.handle, ctypes.byref(sd), ctypes.c_void_p(sbuf.ptr), ctypes.byref(dd), ctypes.c_void_p(dbuf.ptr),
            ctypes.byref(m), N.RESAMPLE_AVERAGE, None, r, s)
        assert call(ctypes.byref(rp), ctypes.byref(sp)) == E_ARG
        assert call(ctypes.byref(rp), None) == E_ARG
        sp.table = tab.ctypes.data
        assert call(None, ctypes.byref(sp)) == E_ARG
        got = np.empty_like(host)
        dbuf.download(out=got)
        assert (got == 0xA5).all()
        assert call(ctypes.byref(rp), ctypes.byref(sp)) == 0  # (and the good call goes through)
        dbuf.download(out=got)
        assert not (got == 0xA5).all()
    finally:
        sbuf.close()
        dbuf.close()
