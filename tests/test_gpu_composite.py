"""The three-band composite on the GPU (k_render_composite_window in csrc/frs_composite.hip) against the single-band
render kernel, frs_render_window_device, which is the oracle here: byte c of every composite pixel equals the C = 1
render of plane c under a LUT whose R byte is channel c's curve, wherever all three planes have data; everywhere else the
pixel is nodata_rgba.  The shapes, rectangles, row paddings and masks are tests/render_cases.py's; the planes' holes
differ, a band stride leaves padding behind each plane, lo / hi differ per channel, n is 1, 256 (the LDS table) and 4096
(the global gather), and the destination's origin takes each of the 16 positions within a chunk, with marker bytes all
around.  Then the argument rejections and the host variant."""
import ctypes

import numpy as np
import pytest

from flac_raster_amd import _native
from tests import composite_ref as CR
from tests import window_ref as R
from tests.render_cases import LUT_SIZES, PAD, RECTS, SIZES, SRC_H, SRC_W, lut_of, nodata_of

pytestmark = pytest.mark.gpu

SLACK = 5  # marker bytes after the destination's last row


def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


class _Rig:
    """Three planes (37, 53) as strided sub-views of a sentinel-filled device buffer, a band stride apart with padding
    behind each, and destination buffers of marker bytes."""

    def __init__(self, ctx, dt):
        self.ctx, self.dt = ctx, np.dtype(dt)
        self.srs = SRC_W + PAD
        self.sbs = (SRC_H - 1) * self.srs + SRC_W + CR.BAND_PAD
        self.sext = 1 + 2 * self.sbs + (SRC_H - 1) * self.srs + SRC_W + 1
        self.sb = ctx.alloc(self.sext * self.dt.itemsize)
        top = max(15 + (h - 1) * (w * 4 + PAD) + w * 4 + SLACK for h, w in SIZES)
        self.db, self.ob = ctx.alloc(top), ctx.alloc(top)
        self.sd3 = ctx.make_raster_desc(SRC_H, SRC_W, self.dt, nbands=3, row_stride=self.srs, band_stride=self.sbs)
        self.sd1 = ctx.make_raster_desc(SRC_H, SRC_W, self.dt, row_stride=self.srs)

    def plane_ptr(self, c):
        return self.sb.ptr + (1 + c * self.sbs) * self.dt.itemsize

    def load(self, planes):
        es = self.dt.itemsize
        src = np.full(self.sext, _sentinel(self.dt), dtype=self.dt)
        for c in range(3):
            np.lib.stride_tricks.as_strided(src[1 + c * self.sbs:], shape=(SRC_H, SRC_W),
                                            strides=(self.srs * es, es))[...] = planes[c]
        self.sb.upload(src)

    def oracle(self, rect, h, w, mode, nd, lo3, hi3, lut, rgba):
        """what the destination's [h][w * 4] must hold, from the single-band kernel: per plane one C = 1 render under
        the LUT whose R byte is the channel's curve, and one under a one-entry table of 255 with a nodata colour of 0,
        which is has_data"""
        out = np.empty((h, w, 4), dtype=np.uint8)
        has_all = np.ones((h, w), dtype=bool)
        one = np.full((1, 4), 255, dtype=np.uint8)
        for c in range(3):
            curve = np.ascontiguousarray(np.repeat(lut[:, c:c + 1], 4, axis=1))
            for table, lo, hi, keep in ((curve, lo3[c], hi3[c], True), (one, 0.0, 1.0, False)):
                self.ctx.render_window_device(self.plane_ptr(c), self.sd1, self.ob.ptr, h, w, rect, mode, lo, hi, table,
                                              nodata_rgba=0, channels=1, nodata=nd)
                got = np.empty((h, w), dtype=np.uint8)
                self.ob.download(h * w, 0, out=got)
                if keep:
                    out[..., c] = got
                else:
                    has_all &= got == 255
        out[..., 3] = 255
        out[~has_all] = [rgba & 0xFF, (rgba >> 8) & 0xFF, (rgba >> 16) & 0xFF, rgba >> 24]
        return out, has_all

    def run(self, rect, h, w, mode, nd, lo3, hi3, lut, rgba, lead, ref):
        """-> (whole destination buffer, what it must hold)"""
        drs = w * 4 + PAD
        dext = lead + (h - 1) * drs + w * 4 + SLACK
        blank = np.full(dext, 0xA5, dtype=np.uint8)
        want = blank.copy()
        np.lib.stride_tricks.as_strided(want[lead:], shape=(h, w * 4), strides=(drs, 1))[...] = ref.reshape(h, w * 4)
        self.db.upload(blank)
        self.ctx.render_composite_window_device(self.plane_ptr(0), self.sd3, self.db.ptr + lead, h, w, rect, mode, lo3,
                                                hi3, lut, nodata_rgba=rgba, nodata=nd, dst_row_stride=drs)
        got = np.empty(dext, dtype=np.uint8)
        self.db.download(dext, 0, out=got)
        return got, want

    def close(self):
        for b in (self.sb, self.db, self.ob):
            b.close()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", CR.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_equals_three_single_band_renders(gpu_ctx, dtype, mode):
    rng = np.random.default_rng(71)
    dt = np.dtype(dtype)
    lut = lut_of(4096)
    lo3, hi3 = CR.channel_limits(dt)
    rig = _Rig(gpu_ctx, dt)
    case = 0
    some, none, mixed = False, False, False
    try:
        for masks in CR.PLANE_MASKS:
            planes = CR.make_planes(rng, dt, masks)
            rig.load(planes)
            for nd in ((None, nodata_of(dt)) if masks == CR.PLANE_MASKS[0] else (nodata_of(dt),)):
                for h, w in SIZES:
                    rects = R.rects(SRC_W, SRC_H, w, h)
                    for rname in RECTS:
                        for n in LUT_SIZES:
                            rgba = 0x80402010 + n
                            lead = CR.LEADS[case % 16]
                            case += 1
                            ref, has = rig.oracle(rects[rname], h, w, mode, nd, lo3, hi3, lut[:n], rgba)
                            some, none = some or bool(has.all()), none or not has.any()
                            mixed = mixed or (bool(has.any()) and not has.all())
                            got, want = rig.run(rects[rname], h, w, mode, nd, lo3, hi3, lut[:n], rgba, lead, ref)
                            assert np.array_equal(got, want), (masks, nd, h, w, rname, n, lead)
        assert some and none and mixed and case >= 16  # the rule is exercised both ways, every alignment was used
    finally:
        rig.close()


def test_oracle_and_restatement_agree_where_the_planes_holes_differ(gpu_ctx):
    """the any-plane rule, shown on one case against the numpy restatement: a pixel is nodata where a hole of ONE plane
    lies, and the other two planes' values there do not show"""
    rng = np.random.default_rng(72)
    dt = np.dtype(np.int16)
    planes = CR.make_planes(rng, dt, ("random30", "collar", "none"))
    lo3, hi3 = CR.channel_limits(dt)
    lut = lut_of(256)
    rect = (0.0, 0.0, float(SRC_W), float(SRC_H))
    got = gpu_ctx.render_composite_window(planes, rect, (SRC_H, SRC_W), "nearest", lo3, hi3, lut,
                                          nodata_rgba=(1, 2, 3, 4), nodata=nodata_of(dt))
    assert np.array_equal(got, CR.composite(planes, rect, (SRC_H, SRC_W), "nearest", nodata_of(dt), lo3, hi3, lut,
                                            (1, 2, 3, 4)))
    hole = (planes == nodata_of(dt)).any(axis=0)
    only_one = (planes == nodata_of(dt)).sum(axis=0) == 1
    assert only_one.any() and (got[hole] == (1, 2, 3, 4)).all() and (got[~hole][:, 3] == 255).all()


def test_dense_destination_and_host_variant(gpu_ctx):
    """the default layout (rows w * 4 bytes apart, 16-byte aligned origin) at a width of several work-group steps, on
    the device and through the host-staged call"""
    rng = np.random.default_rng(73)
    for dtype, mode, (h, w), n in ((np.int16, "average", (7, 1100), 256), (np.float32, "bilinear", (40, 9), 4096),
                                   (np.uint8, "nearest", (3, 515), 1)):
        dt = np.dtype(dtype)
        planes = CR.make_planes(rng, dt, ("collar", "none", "random30"))
        lo3, hi3 = CR.channel_limits(dt)
        lut = lut_of(n, seed=n)
        rect = R.rects(SRC_W, SRC_H, w, h)["over_all_edges"]
        for nd in (None, nodata_of(dt)):
            want = CR.composite(planes, rect, (h, w), mode, nd, lo3, hi3, lut, 0x01020304)
            got = gpu_ctx.render_composite_window(planes, rect, (h, w), mode, lo3, hi3, lut, nodata_rgba=0x01020304,
                                                  nodata=nd)
            assert got.dtype == np.uint8 and got.shape == (h, w, 4) and np.array_equal(got, want)
            src, dst = gpu_ctx.alloc(planes.nbytes), gpu_ctx.alloc(h * w * 4)
            try:
                src.upload(planes)
                sd = gpu_ctx.make_raster_desc(SRC_H, SRC_W, dt, nbands=3)
                gpu_ctx.render_composite_window_device(src.ptr, sd, dst.ptr, h, w, rect, mode, lo3, hi3, lut,
                                                       nodata_rgba=0x01020304, nodata=nd)
                out = np.empty((h, w, 4), dtype=np.uint8)
                dst.download(out=out)
                assert np.array_equal(out, want)
            finally:
                src.close()
                dst.close()


def test_profile_entry(gpu_ctx):
    planes = np.arange(3 * 4 * 5, dtype=np.int16).reshape(3, 4, 5)
    gpu_ctx.profile(True)
    try:
        gpu_ctx.profile_reset()
        gpu_ctx.render_composite_window(planes, (0.0, 0.0, 5.0, 4.0), (4, 5), "nearest", (0, 0, 0), (60, 60, 60),
                                        lut_of(16))
        assert gpu_ctx.profile_avg_ms("render_composite") >= 0.0
    finally:
        gpu_ctx.profile(False)


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
        lo3, hi3 = (0.0, 1.0, 2.0), (10.0, 11.0, 12.0)

        def call(dt=i16, nd=None, mode="average", sd=None, r=rect, s=src, d=dst, h=3, w=5, lo=lo3, hi=hi3, t=lut,
                 rs=None, dd=None, cp=None):
            sd = sd or ctx.make_raster_desc(5, 9, dt, nbands=3)
            if dd is None and cp is None:
                return ctx.render_composite_window_device(s, sd, d, h, w, r, mode, lo, hi, t, nodata=nd,
                                                          dst_row_stride=rs)
            # a destination descriptor or parameters the wrapper would not build
            dd = dd or ctx.make_raster_desc(h, w, np.uint8, row_stride=w * 4)
            keep = np.ascontiguousarray(t)
            d3 = ctypes.c_double * 3
            if cp is None:
                cp = _native.CompositeParams(d3(*lo), d3(*hi), keep.ctypes.data, len(keep), 0)
            m = _native.WindowMap(*r, 0.0)
            ctx._check(ctx.lib.frs_render_composite_window_device(
                ctx.handle, ctypes.byref(sd), ctypes.c_void_p(s), ctypes.byref(dd), ctypes.c_void_p(d), ctypes.byref(m),
                _native.WINDOW_RESAMPLE_CODES[mode], None, None if cp == "null" else ctypes.byref(cp)))

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
        # what frs_render_window* rejects
        assert rejected("row_stride < width", sd=ctx.make_raster_desc(5, 9, i16, nbands=3, row_stride=8))
        assert rejected("height and width must be >= 1", h=0)
        assert rejected("bad dtype", sd=_native.RasterDesc(5, 9, 9, 45, 9, 3))
        assert rejected("bad mode", mode=3)
        assert rejected("width and height must be > 0", r=(0.0, 0.0, 0.0, 3.0))
        assert rejected("rectangle must be finite", r=(float("nan"), 0.0, 1.0, 3.0))
        assert rejected("nodata must be an integer inside the dtype's range", nd=0.5)
        assert rejected("null or element-misaligned pointer", s=0)
        assert rejected("null or element-misaligned pointer", s=src + 1)
        assert rejected("null or element-misaligned pointer", d=0)
        assert rejected("nbands must be 1", dd=ctx.make_raster_desc(3, 5, np.uint8, nbands=2, row_stride=20))
        assert rejected("LUT length must be 1..4096", t=np.zeros((0, 4), np.uint8))
        assert rejected("LUT length must be 1..4096", t=np.zeros((4097, 4), np.uint8))
        d3 = ctypes.c_double * 3
        assert rejected("null LUT", cp=_native.CompositeParams(d3(*lo3), d3(*hi3), None, 16, 0))
        assert rejected("destination must be uint8", dd=ctx.make_raster_desc(3, 5, np.uint16, row_stride=20))
        assert rejected("row_stride (bytes) < width * channels", rs=19)
        # the composite's own: three planes, a band stride that holds a plane, every channel's lo / hi
        for nb in (1, 2, 4):
            assert rejected("the source must have 3 bands", sd=ctx.make_raster_desc(5, 9, i16, nbands=nb))
        assert rejected("band_stride too small", sd=ctx.make_raster_desc(5, 9, i16, nbands=3, band_stride=44))
        assert rejected("null parameters", cp="null")
        for c in range(3):
            for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (-1.7e308, 1.7e308)):
                lo_c, hi_c = list(lo3), list(hi3)
                lo_c[c], hi_c[c] = lo, hi
                assert rejected("lo, hi and hi - lo must be finite", lo=lo_c, hi=hi_c)
            hi_c = list(hi3)
            hi_c[c] = lo3[c]
            assert rejected("hi must be > lo", hi=hi_c)
        # the destination may not overlap any of the three planes (5 x 9 int16 each, 90 bytes apart)
        assert rejected("source and destination overlap", d=src + 2 * 10)
        assert rejected("source and destination overlap", d=src + 90 + 20)
        assert rejected("source and destination overlap", d=src + 180 + 20)
        assert rejected("source and destination overlap", s=dst + 16)
        # an unaligned destination is fine: it is bytes
        call(d=dst + 1)
        got = buf.download()
        assert (got[:4097] == 0xA5).all() and (got[4096 + 1 + 60:] == 0xA5).all()
    finally:
        buf.close()
