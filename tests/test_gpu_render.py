"""The 8-bit render on the GPU (k_render_window in csrc/frs_render.hip): frs_render_window_device against
tests/render_ref.py, byte for byte: seven dtypes x three modes x C in {1, 2, 4}, a 37 x 53 source as a strided sub-view
with sentinels, destinations one byte off a 16-byte boundary with row padding and sentinel bytes all around, four masks,
five rectangles, LUT lengths 1, 256 (the LDS table) and 4096 (the global gather) with a random LUT, and stretch limits
inside the data's range so that both clamps are hit; the argument rejections; the host variant."""
import ctypes

import numpy as np
import pytest

from flac_raster_amd import _native
from tests import render_ref as RR
from tests import window_ref as R
from tests.render_cases import (LEAD, LUT_SIZES, MASKS, PAD, RECTS, SIZES, SRC_H, SRC_W, limits, lut_of, make_source,
                                nodata_of)

pytestmark = pytest.mark.gpu

SLACK = 5  # sentinel bytes after the destination's last row


def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


class _Rig:
    """A source raster (37, 53) as a strided sub-view of a sentinel-filled device buffer, and a destination buffer of
    sentinel bytes per call (tests/test_gpu_window_nodata.py's arrangement, for one band and byte pixels)."""

    def __init__(self, ctx, dt):
        self.ctx, self.dt = ctx, np.dtype(dt)
        self.srs = SRC_W + PAD
        self.sext = LEAD + (SRC_H - 1) * self.srs + SRC_W + LEAD
        self.sb = ctx.alloc(self.sext * self.dt.itemsize)
        self.db = ctx.alloc(max(self._dst_layout(h, w, 4)[1] for h, w in SIZES))
        self.sd = ctx.make_raster_desc(SRC_H, SRC_W, self.dt, row_stride=self.srs)

    @staticmethod
    def _dst_layout(h, w, C):
        drs = w * C + PAD
        return drs, LEAD + (h - 1) * drs + w * C + SLACK

    def load(self, a):
        es = self.dt.itemsize
        src = np.full(self.sext, _sentinel(self.dt), dtype=self.dt)
        np.lib.stride_tricks.as_strided(src[LEAD:], shape=(SRC_H, SRC_W), strides=(self.srs * es, es))[...] = a
        self.sb.upload(src)

    def run(self, rect, h, w, mode, nd, lo, hi, lut, rgba, C, ref):
        """-> (whole destination buffer, what it must hold)"""
        drs, dext = self._dst_layout(h, w, C)
        blank = np.full(dext, 0xA5, dtype=np.uint8)
        want = blank.copy()
        np.lib.stride_tricks.as_strided(want[LEAD:], shape=(h, w * C), strides=(drs, 1))[...] = ref.reshape(h, w * C)
        self.db.upload(blank)
        self.ctx.render_window_device(self.sb.ptr + LEAD * self.dt.itemsize, self.sd, self.db.ptr + LEAD, h, w, rect,
                                      mode, lo, hi, lut, nodata_rgba=rgba, channels=C, nodata=nd, dst_row_stride=drs)
        got = np.empty(dext, dtype=np.uint8)
        self.db.download(dext, 0, out=got)
        return got, want

    def close(self):
        self.sb.close()
        self.db.close()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_equals_the_restatement_byte_for_byte(gpu_ctx, dtype, mode):
    """every mask (the unmasked kernel as well where nothing is masked), destination size, rectangle, channel count and
    LUT length; every sentinel survives"""
    rng = np.random.default_rng(51)
    dt = np.dtype(dtype)
    lut = lut_of(4096)
    lo, hi = limits(dt)
    rig = _Rig(gpu_ctx, dt)
    try:
        for mask in MASKS:
            a = make_source(rng, dt, mask, nodata_of(dt))
            rig.load(a)
            for nd in ((None, nodata_of(dt)) if mask == "none" else (nodata_of(dt),)):
                for h, w in SIZES:
                    rects = R.rects(SRC_W, SRC_H, w, h)
                    for rname in RECTS:
                        v, has = RR.resampled(a, rects[rname], (h, w), mode, nd)
                        if mask == "all" or rname == "outside_right":
                            assert not has.any()
                        elif rname == "scale_to_fit" and mask == "none" and dt.kind != "f":
                            assert has.all()
                        if mask == "none" and rname == "scale_to_fit" and (h, w) == (17, 33):
                            x = v[has].astype(np.float64)
                            assert (x < lo).any() and (x > hi).any() and ((x >= lo) & (x <= hi)).any()  # both clamps
                        for C in (1, 2, 4):
                            for n in LUT_SIZES:
                                rgba = 0x80402010 + n + C
                                ref = RR.colours(v, has, lo, hi, lut[:n], rgba, C)
                                got, want = rig.run(rects[rname], h, w, mode, nd, lo, hi, lut[:n], rgba, C, ref)
                                assert np.array_equal(got, want), (mask, nd, h, w, rname, C, n)
    finally:
        rig.close()


def test_dense_destination_and_tuple_nodata_colour(gpu_ctx):
    """the default layout (rows w * C bytes apart, 16-byte aligned origin) at a width of several whole chunks"""
    rng = np.random.default_rng(52)
    dt = np.dtype(np.int16)
    a = make_source(rng, dt, "collar", nodata_of(dt))
    lo, hi = limits(dt)
    src, dst = gpu_ctx.alloc(a.nbytes), gpu_ctx.alloc(64 * 1100 * 4)
    try:
        src.upload(a)
        sd = gpu_ctx.make_raster_desc(SRC_H, SRC_W, dt)
        for (h, w), C, n in (((64, 1100), 4, 256), ((3, 1029), 1, 4096), ((5, 515), 2, 256)):
            lut = lut_of(n, seed=n)
            rect = R.rects(SRC_W, SRC_H, w, h)["over_all_edges"]
            for mode in R.MODES:
                gpu_ctx.render_window_device(src.ptr, sd, dst.ptr, h, w, rect, mode, lo, hi, lut,
                                             nodata_rgba=(9, 8, 7, 6), channels=C, nodata=nodata_of(dt))
                got = np.empty((h, w, C), dtype=np.uint8)
                dst.download(got.nbytes, 0, out=got)
                want = RR.render(a, rect, (h, w), mode, nodata_of(dt), lo, hi, lut, (9, 8, 7, 6), C)
                assert np.array_equal(got, want), (h, w, C, n, mode)
    finally:
        src.close()
        dst.close()


def test_host_variant(gpu_ctx):
    rng = np.random.default_rng(53)
    for dtype, mode, shape, C, n in ((np.int16, "average", (5, 33), 4, 256), (np.float32, "bilinear", (40, 9), 2, 4096),
                                     (np.uint8, "nearest", (1, 7), 1, 1)):
        dt = np.dtype(dtype)
        a = make_source(rng, dt, "collar", nodata_of(dt))
        lo, hi = limits(dt)
        lut = lut_of(n)
        rect = R.rects(SRC_W, SRC_H, shape[1], shape[0])["over_all_edges"]
        for nd in (None, nodata_of(dt)):
            got = gpu_ctx.render_window(a, rect, shape, mode, lo, hi, lut, nodata_rgba=0x01020304, channels=C, nodata=nd)
            assert got.dtype == np.uint8 and got.shape == shape + (C,)
            assert np.array_equal(got, RR.render(a, rect, shape, mode, nd, lo, hi, lut, 0x01020304, C))


def test_argument_errors(gpu_ctx):
    """one rejection per rule, with its message; nothing is launched (the destination keeps its bytes)"""
    ctx = gpu_ctx
    buf = ctx.alloc(8192)
    try:
        buf.upload(np.full(8192, 0xA5, dtype=np.uint8))
        src, dst = buf.ptr, buf.ptr + 4096
        rect = (0.5, 0.5, 7.0, 3.0)
        lut = lut_of(16)
        i16 = np.dtype(np.int16)

        def call(dt=i16, nd=None, mode="average", sd=None, r=rect, s=src, d=dst, h=3, w=5, lo=0.0, hi=10.0, t=lut,
                 C=4, rs=None, dd=None, rp=None):
            sd = sd or ctx.make_raster_desc(5, 9, dt)
            if dd is None and rp is None:
                return ctx.render_window_device(s, sd, d, h, w, r, mode, lo, hi, t, channels=C, nodata=nd,
                                                dst_row_stride=rs)
            # a destination descriptor or render parameters the wrapper would not build
            dd = dd or ctx.make_raster_desc(h, w, np.uint8, row_stride=w * C)
            keep = np.ascontiguousarray(t)
            if rp is None:
                rp = _native.RenderParams(lo, hi, keep.ctypes.data, len(keep), 0, C)
            m = _native.WindowMap(*r, 0.0)
            ctx._check(ctx.lib.frs_render_window_device(
                ctx.handle, ctypes.byref(sd), ctypes.c_void_p(s), ctypes.byref(dd), ctypes.c_void_p(d), ctypes.byref(m),
                _native.WINDOW_RESAMPLE_CODES[mode], None, None if rp == "null" else ctypes.byref(rp)))

        def rejected(msg, **kw):
            with pytest.raises(_native.FrsError) as e:
                call(**kw)
            assert e.value.code == -1 and msg in str(e.value), e.value  # FRS_E_ARG
            return True

        for dtype in R.DTYPES:  # the call itself is accepted for every dtype and mode
            for mode in R.MODES:
                call(np.dtype(dtype), mode=mode)
                call(np.dtype(dtype), nd=nodata_of(dtype), mode=mode)
        buf.upload(np.full(8192, 0xA5, dtype=np.uint8))
        # what frs_resample_window* rejects
        assert rejected("row_stride < width", sd=ctx.make_raster_desc(5, 9, i16, row_stride=8))
        assert rejected("height and width must be >= 1", h=0)
        assert rejected("bad dtype", sd=_native.RasterDesc(5, 9, 9, 45, 9, 1))
        assert rejected("bad mode", mode=3)
        assert rejected("width and height must be > 0", r=(0.0, 0.0, 0.0, 3.0))
        assert rejected("rectangle must be finite", r=(float("nan"), 0.0, 1.0, 3.0))
        assert rejected("nodata must be an integer inside the dtype's range", nd=0.5)
        assert rejected("nodata must be an integer inside the dtype's range", nd=40000)
        assert rejected("null or element-misaligned pointer", s=0)
        assert rejected("null or element-misaligned pointer", s=src + 1)
        assert rejected("null or element-misaligned pointer", d=0)
        # the render's own
        assert rejected("nbands must be 1", sd=ctx.make_raster_desc(5, 9, i16, nbands=2))
        assert rejected("nbands must be 1", dd=ctx.make_raster_desc(3, 5, np.uint8, nbands=2, row_stride=20))
        for C in (0, 3, 5, 8):
            assert rejected("channels must be 1, 2 or 4", C=C, rs=64)
        assert rejected("LUT length must be 1..4096", t=np.zeros((0, 4), np.uint8))
        assert rejected("LUT length must be 1..4096", t=np.zeros((4097, 4), np.uint8))
        assert rejected("null LUT", rp=_native.RenderParams(0.0, 10.0, None, 16, 0, 4))
        assert rejected("null render parameters", rp="null")
        for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (-1.7e308, 1.7e308)):
            assert rejected("lo, hi and hi - lo must be finite", lo=lo, hi=hi)
        assert rejected("hi must be > lo", lo=1.0, hi=1.0) and rejected("hi must be > lo", lo=2.0, hi=1.0)
        assert rejected("destination must be uint8", dd=ctx.make_raster_desc(3, 5, np.uint16, row_stride=20))
        assert rejected("row_stride (bytes) < width * channels", rs=19)
        assert rejected("row_stride (bytes) < width * channels", C=2, rs=9)
        assert rejected("source and destination overlap", d=src + 2 * 10)
        assert rejected("source and destination overlap", s=dst + 16)
        # an unaligned destination is fine: it is bytes
        call(d=dst + 1)
        got = buf.download()
        assert (got[:4097] == 0xA5).all() and (got[4096 + 1 + 60:] == 0xA5).all()
    finally:
        buf.close()
