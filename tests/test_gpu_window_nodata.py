"""The nodata-aware windowed resample on the GPU (k_resample_window_nodata in csrc/frs_window.hip):
frs_resample_window_nodata_device against tests/nodata_ref.py, bit for bit: seven dtypes x three modes, a 37 x 53
source as a strided sub-view with sentinels, the rectangles of window_ref.rects (identity, ~9x reduction, partly and
wholly outside among them) at destination sizes below, on and above one and several 16-byte chunks, under four masks,
with a fill that is not the nodata value and a NaN fill for floats; the argument rejections; the host variant."""
import numpy as np
import pytest

from flac_raster_amd import _native
from tests import nodata_ref as N
from tests import window_ref as R

pytestmark = pytest.mark.gpu

SRC_H, SRC_W = 37, 53
SIZES = ((1, 1), (5, 7), (17, 33), (3, 130), (40, 9))  # (h, w)
RECTS = ("scale_to_fit", "1.37x", "9.3x", "0.4x_upsampling", "over_left_top", "over_all_edges", "outside_right",
         "lo_on_pixel_edges")
MASKS = ("none", "all", "random30", "collar")
FILL = 200.5  # half to even: 200 in every integer dtype; never a nodata value of this test
PAD, SLACK, LEAD = 3, 5, 1  # row padding, band slack, elements before the raster's origin


def nodata_values(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return [0.0, float("nan"), float("-inf")]
    ii = np.iinfo(dt)
    return sorted({ii.min, ii.max, 0})


def _values(rng, dtype, shape, nd):
    """values none of which is nodata; floats with a NaN and both infinities where those are not nodata"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(dt)
        v[:, 5, 7], v[:, 20, 30], v[:, 30, 2] = np.nan, np.inf, -np.inf
        v[N.nodata_mask(v, nd)] = dt.type(1.5)
        return v
    ii = np.iinfo(dt)
    v = rng.integers(ii.min, ii.max, size=shape, dtype=dt, endpoint=True)
    pick = rng.integers(0, 6, size=shape)
    v[pick == 0], v[pick == 1] = ii.min, ii.max
    v[v == dt.type(nd)] = dt.type(nd + 1 if nd < ii.max else nd - 1)
    return v


def _mask(rng, name, shape):
    m = np.zeros(shape, dtype=bool)
    if name == "all":
        m[...] = True
    elif name == "random30":
        m[...] = rng.random(shape) < 0.3
    elif name == "collar":
        m[...] = True
        m[:, 6:-6, 8:-8] = False
        m[:, 15:18, 20:26] = True  # and a hole
    return m


def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


def _same(got, want):
    if got.dtype.kind == "f":  # NaN payloads are the hardware's: NaN in the same places, the same bits elsewhere
        n = np.isnan(want)
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        return np.array_equal(np.isnan(got), n) and np.array_equal(got.view(u)[~n], want.view(u)[~n])
    return np.array_equal(got, want)


class _Rig:
    """A source raster (C, 37, 53) as a strided sub-view of a sentinel-filled device buffer, and a destination buffer
    laid out the same way per call (tests/test_gpu_window.py's arrangement)."""

    def __init__(self, ctx, dt, C):
        self.ctx, self.dt, self.C = ctx, np.dtype(dt), C
        self.srs, self.sbs, self.sext = self._layout(C, SRC_H, SRC_W)
        self.sb = ctx.alloc(self.sext * self.dt.itemsize)
        self.db = ctx.alloc(self._layout(C, max(h for h, _ in SIZES), max(w for _, w in SIZES))[2] * self.dt.itemsize)
        assert SRC_H <= max(h for h, _ in SIZES) and SRC_W <= max(w for _, w in SIZES)

    @staticmethod
    def _layout(C, h, w):
        rs = w + PAD
        bs = rs * h + SLACK
        return rs, bs, LEAD + (C - 1) * bs + (h - 1) * rs + w + LEAD

    def _view(self, buf, C, h, w, rs, bs):
        es = self.dt.itemsize
        return np.lib.stride_tricks.as_strided(buf[LEAD:], shape=(C, h, w), strides=(bs * es, rs * es, es))

    def load(self, a):
        src = np.full(self.sext, _sentinel(self.dt), dtype=self.dt)
        self._view(src, self.C, SRC_H, SRC_W, self.srs, self.sbs)[...] = a
        self.sb.upload(src)

    def run(self, C, rect, h, w, mode, fill, nd, ref):
        """bands [0, C) of the source -> (whole destination buffer, what it must hold)"""
        ctx, dt = self.ctx, self.dt
        drs, dbs, dext = self._layout(C, h, w)
        blank = np.full(dext, _sentinel(dt), dtype=dt)
        want = blank.copy()
        self._view(want, C, h, w, drs, dbs)[...] = ref[:C]
        self.db.upload(blank)
        sd = ctx.make_raster_desc(SRC_H, SRC_W, dt, nbands=C, row_stride=self.srs, band_stride=self.sbs)
        dd = ctx.make_raster_desc(h, w, dt, nbands=C, row_stride=drs, band_stride=dbs)
        ctx.resample_window_device(self.sb.ptr + LEAD * dt.itemsize, sd, self.db.ptr + LEAD * dt.itemsize, dd, rect,
                                   mode, fill, nodata=nd)
        got = np.empty(dext, dtype=dt)
        self.db.download(got.nbytes, 0, out=got.view(np.uint8))
        return got, want

    def close(self):
        self.sb.close()
        self.db.close()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_masked_kernel_equals_the_restatement_bit_for_bit(gpu_ctx, dtype, mode):
    """every nodata value, mask, destination size and rectangle, three bands and one, as strided sub-views one element
    off a 16-byte boundary; every sentinel survives; without a masked pixel the result is the unmasked call's"""
    rng = np.random.default_rng(41)
    dt = np.dtype(dtype)
    rig = _Rig(gpu_ctx, dt, 3)
    try:
        for nd in nodata_values(dtype):
            base = _values(rng, dtype, (3, SRC_H, SRC_W), nd)
            for name in MASKS:
                a = base.copy()
                m = _mask(rng, name, a.shape)
                a[m] = dt.type(nd)
                if dt.kind == "f" and nd == 0:  # -0.0 is nodata as well
                    a[m & (rng.random(a.shape) < 0.5)] = dt.type(-0.0)
                rig.load(a)
                for h, w in SIZES + ((SRC_H, SRC_W),):
                    rects = R.rects(SRC_W, SRC_H, w, h)
                    for rname in RECTS if (h, w) != (SRC_H, SRC_W) else ("scale_to_fit",):  # the last: the identity
                        ref = N.resample_nodata(a, rects[rname], (h, w), mode, FILL, nd)
                        if name == "all" or rname == "outside_right":
                            assert np.array_equal(ref, np.full_like(ref, R.to_dtype(FILL, dt)))
                        for C in (1, 3) if rname in ("1.37x", "over_all_edges") else (3,):  # (the last: all three bands)
                            got, want = rig.run(C, rects[rname], h, w, mode, FILL, nd, ref)
                            assert _same(got, want), (nd, name, h, w, rname, C)
                        if name == "none":  # the unmasked call's result, but for the integer nudge off nodata
                            plain, _ = rig.run(3, rects[rname], h, w, mode, FILL, None, ref)
                            if dt.kind != "f":  # (neither the sentinel nor FILL is a nodata value of this test)
                                plain = N.nudge(plain.astype(np.int64), dt.type(nd), dt).astype(dt)
                            assert _same(plain, want), (nd, h, w, rname)
    finally:
        rig.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_fill_on_float_rasters(gpu_ctx, dtype):
    rng = np.random.default_rng(42)
    dt = np.dtype(dtype)
    nd = float("nan")
    a = _values(rng, dtype, (3, SRC_H, SRC_W), nd)
    a[_mask(rng, "collar", a.shape)] = np.nan
    rig = _Rig(gpu_ctx, dt, 3)
    try:
        rig.load(a)
        for mode in R.MODES:
            for h, w in ((17, 33), (5, 7)):
                rect = R.rects(SRC_W, SRC_H, w, h)["over_all_edges"]
                ref = N.resample_nodata(a, rect, (h, w), mode, nd, nd)
                assert np.isnan(ref[:, 0, 0]).all() and not np.isnan(ref[:, h // 2, w // 2]).any()
                got, want = rig.run(3, rect, h, w, mode, nd, nd, ref)
                assert _same(got, want), (mode, h, w)
    finally:
        rig.close()


def test_fill_defaults_and_host_variant(gpu_ctx):
    rng = np.random.default_rng(43)
    for dtype, mode, shape, nd in ((np.int16, "average", (5, 33), -9999), (np.float32, "bilinear", (40, 9), -np.inf),
                                   (np.uint8, "nearest", (1, 7), 0)):
        a = _values(rng, dtype, (3, SRC_H, SRC_W), nd)
        a[_mask(rng, "collar", a.shape)] = np.dtype(dtype).type(nd)
        rect = R.rects(SRC_W, SRC_H, shape[1], shape[0])["over_all_edges"]
        for fill in (7, FILL):
            assert _same(gpu_ctx.resample_window(a, rect, shape, mode, fill, nodata=nd),
                         N.resample_nodata(a, rect, shape, mode, fill, nd))
            assert _same(gpu_ctx.resample_window(a[0], rect, shape, mode, fill, nodata=nd),
                         N.resample_nodata(a[0], rect, shape, mode, fill, nd))


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    buf = ctx.alloc(8192)
    try:
        buf.upload(np.zeros(8192, dtype=np.uint8))
        src, dst = buf.ptr, buf.ptr + 4096
        rect = (0.5, 0.5, 7.0, 3.0)

        def call(dt, nd, fill=0, mode="average", sd=None, dd=None, r=rect, s=src, d=dst):
            ctx.resample_window_device(s, sd or ctx.make_raster_desc(5, 9, dt), d, dd or ctx.make_raster_desc(3, 5, dt),
                                       r, mode, fill, nodata=nd)

        def rejected(*args, **kw):
            with pytest.raises(_native.FrsError) as e:
                call(*args, **kw)
            assert e.value.code == -1, e.value  # FRS_E_ARG
            return True

        for dtype in R.DTYPES:
            dt = np.dtype(dtype)
            for mode in R.MODES:
                for nd in nodata_values(dtype):
                    call(dt, nd, mode=mode)
                if dt.kind == "f":
                    call(dt, float("inf"), mode=mode)
                    call(dt, 0.0, fill=float("nan"), mode=mode)      # a float raster may be filled with NaN
                    assert rejected(dt, 0.0, fill=float("inf"), mode=mode)
                    assert rejected(dt, float("nan"), fill=float("-inf"), mode=mode)
                    continue
                ii = np.iinfo(dt)
                for nd in (ii.min - 1, ii.max + 1, 0.5, float("nan"), float("inf"), float("-inf")):
                    assert rejected(dt, nd, mode=mode), (dt, nd)
                assert rejected(dt, 0, fill=float("nan"), mode=mode)
                assert rejected(dt, 0, fill=float("inf"), mode=mode)
        # the unmasked call's rejections hold with a nodata value
        i16 = np.dtype(np.int16)
        assert rejected(i16, 0, dd=ctx.make_raster_desc(3, 5, np.uint16))
        assert rejected(i16, 0, sd=ctx.make_raster_desc(5, 9, i16, row_stride=8))
        assert rejected(i16, 0, mode=3)
        assert rejected(i16, 0, r=(0.0, 0.0, 0.0, 3.0)) and rejected(i16, 0, r=(float("nan"), 0.0, 1.0, 3.0))
        assert rejected(i16, 0, s=0) and rejected(i16, 0, d=dst + 1)
        assert rejected(i16, 0, d=src + 2 * 10)  # overlap
    finally:
        buf.close()
