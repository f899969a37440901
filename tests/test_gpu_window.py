"""The windowed resample on the GPU (csrc/frs_window.hip): frs_resample_window_device against the numpy restatement
tests/window_ref.py, bit for bit, on a 37 x 53 source and destination sizes that put a row below, on and above one and
several 16-byte chunks; strided sub-views with sentinels around the destination; every argument error; and the file
path, streaming.read_window and the CLI, against window_ref applied to the numpy pyramid."""
import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, geotiff, streaming
from flac_raster_amd.cli import app
from tests import window_ref as R
from tests.pyramid_ref import np_pyramid

pytestmark = pytest.mark.gpu
runner = CliRunner()

SRC_H, SRC_W = 37, 53
WIDTHS = (1, 7, 8, 9, 33, 300)
HEIGHTS = (1, 5, 40)
FILL = 200.5  # half to even: 200 in every integer dtype
PAD, SLACK, LEAD = 3, 5, 1  # row padding, band slack, elements before the raster's origin


def _values(rng, dtype, shape):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(dt)
        v[:, 5, 7], v[:, 20, 30], v[:, 30, 2] = np.nan, np.inf, -np.inf
        return v
    ii = np.iinfo(dt)
    v = rng.integers(ii.min, ii.max, size=shape, dtype=dt, endpoint=True)
    pick = rng.integers(0, 6, size=shape)
    v[pick == 0], v[pick == 1] = ii.min, ii.max
    return v


def _finite_values(rng, dtype, shape):
    v = _values(rng, dtype, shape)
    if v.dtype.kind == "f":
        v[~np.isfinite(v)] = 1.5
    return v


def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


def _same(got, want):
    if got.dtype.kind == "f":  # NaN payloads are the hardware's: NaN in the same places, the same bits elsewhere
        n = np.isnan(want)
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        return np.array_equal(np.isnan(got), n) and np.array_equal(got.view(u)[~n], want.view(u)[~n])
    return np.array_equal(got, want)


class _Rig:
    """A source raster (C, 37, 53) laid out as a strided sub-view of a sentinel-filled device buffer (row_stride =
    width + 3, band slack 5, origin one element in), and a destination buffer laid out the same way per call."""

    def __init__(self, ctx, a):
        self.ctx, self.a, self.dt = ctx, a, a.dtype
        C, H, W = a.shape
        self.srs, self.sbs, ext = self._layout(C, H, W)
        src = np.full(ext, _sentinel(self.dt), dtype=self.dt)
        self._view(src, C, H, W, self.srs, self.sbs)[...] = a
        self.sb = ctx.alloc(src.nbytes)
        self.sb.upload(src)
        self.db = ctx.alloc(self._layout(C, max(HEIGHTS + (H,)), max(WIDTHS + (W,)))[2] * self.dt.itemsize)

    @staticmethod
    def _layout(C, h, w):
        rs = w + PAD
        bs = rs * h + SLACK
        return rs, bs, LEAD + (C - 1) * bs + (h - 1) * rs + w + LEAD

    def _view(self, buf, C, h, w, rs, bs):
        es = self.dt.itemsize
        return np.lib.stride_tricks.as_strided(buf[LEAD:], shape=(C, h, w), strides=(bs * es, rs * es, es))

    def run(self, C, rect, h, w, mode, fill, ref):
        """bands [0, C) of the source -> (whole destination buffer, what it must hold)"""
        ctx, dt = self.ctx, self.dt
        H, W = self.a.shape[1:]
        drs, dbs, dext = self._layout(C, h, w)
        blank = np.full(dext, _sentinel(dt), dtype=dt)
        want = blank.copy()
        self._view(want, C, h, w, drs, dbs)[...] = ref[:C]
        self.db.upload(blank)
        sd = ctx.make_raster_desc(H, W, dt, nbands=C, row_stride=self.srs, band_stride=self.sbs)
        dd = ctx.make_raster_desc(h, w, dt, nbands=C, row_stride=drs, band_stride=dbs)
        ctx.resample_window_device(self.sb.ptr + LEAD * dt.itemsize, sd, self.db.ptr + LEAD * dt.itemsize, dd, rect,
                                   mode, fill)
        got = np.empty(dext, dtype=dt)
        self.db.download(got.nbytes, 0, out=got.view(np.uint8))
        return got, want

    def close(self):
        self.sb.close()
        self.db.close()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_equals_the_restatement_bit_for_bit(gpu_ctx, dtype, mode):
    """Every rectangle of the host test at every destination size, one band and three, as strided sub-views one
    element off a 16-byte boundary; floats with a NaN and both infinities; every sentinel survives."""
    rng = np.random.default_rng(21)
    a = _values(rng, dtype, (3, SRC_H, SRC_W))
    rig = _Rig(gpu_ctx, a)
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                for name, rect in R.rects(SRC_W, SRC_H, w, h).items():
                    ref = R.resample(a, rect, (h, w), mode, FILL)
                    for C in (1, 3):
                        got, want = rig.run(C, rect, h, w, mode, FILL, ref)
                        assert _same(got, want), (name, h, w, C)
    finally:
        rig.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_identity_rectangle_returns_the_source(gpu_ctx, dtype):
    rng = np.random.default_rng(22)
    a = _finite_values(rng, dtype, (3, SRC_H, SRC_W))
    rig = _Rig(gpu_ctx, a)
    try:
        for mode in R.MODES:
            for C in (1, 3):
                got, want = rig.run(C, (0.0, 0.0, float(SRC_W), float(SRC_H)), SRC_H, SRC_W, mode, FILL, a)
                assert np.array_equal(got, want), (mode, C)
    finally:
        rig.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_wholly_outside_rectangle_returns_fill(gpu_ctx, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(23)
    a = _values(rng, dtype, (3, SRC_H, SRC_W))
    rig = _Rig(gpu_ctx, a)
    try:
        for fill in (0, FILL, -3.5, 1e10, -1e300):
            if dt.kind == "f":
                with np.errstate(over="ignore"):
                    f = np.float64(fill).astype(dt)
            else:
                ii = np.iinfo(dt)
                f = dt.type(min(max(round(fill), ii.min), ii.max))
            for mode in R.MODES:
                for rect in ((SRC_W + 0.0, 0.0, 10.0, 10.0), (0.0, -10.0, 10.0, 10.0), (-1e6, -1e6, 5.0, 5.0)):
                    got, want = rig.run(3, rect, 5, 33, mode, fill, np.full((3, 5, 33), f, dtype=dt))
                    assert np.array_equal(got, want), (fill, mode, rect)
    finally:
        rig.close()


def test_rows_longer_than_one_step_and_more_rows_than_the_grid(gpu_ctx):
    """A row of more chunks than one work-group step covers (256 chunks; float64 has the fewest outputs per chunk), and
    more destination rows than the grid has (32768): the strides over both."""
    rng = np.random.default_rng(24)
    for dtype, h, w, mode in ((np.float64, 3, 1300, "average"), (np.int16, 2, 5000, "bilinear"),
                              (np.uint8, 33000, 3, "nearest"), (np.uint8, 33000, 3, "average")):
        a = _finite_values(rng, dtype, (1, SRC_H, SRC_W))
        rect = (-1.25, 0.5, SRC_W + 2.0, SRC_H - 1.0)
        want = R.resample(a, rect, (h, w), mode, 9)
        assert np.array_equal(gpu_ctx.resample_window(a, rect, (h, w), mode, 9), want), (dtype, h, w, mode)


def test_host_variant(gpu_ctx):
    rng = np.random.default_rng(25)
    for dtype, mode, shape in ((np.int16, "average", (5, 33)), (np.float32, "bilinear", (40, 9)),
                               (np.uint8, "nearest", (1, 7))):
        a = _values(rng, dtype, (3, SRC_H, SRC_W))
        rect = R.rects(SRC_W, SRC_H, shape[1], shape[0])["1.37x"]
        assert _same(gpu_ctx.resample_window(a, rect, shape, mode, FILL), R.resample(a, rect, shape, mode, FILL))
        assert _same(gpu_ctx.resample_window(a[0], rect, shape, mode, FILL), R.resample(a[0], rect, shape, mode, FILL))
    with pytest.raises(ValueError, match="nearest"):
        gpu_ctx.resample_window(a, rect, shape, "cubic")


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    dt = np.dtype(np.int16)
    buf = ctx.alloc(4096)
    try:
        buf.upload(np.zeros(2048, dtype=dt))
        src, dst = buf.ptr, buf.ptr + 2048
        good_rect = (0.5, 0.5, 7.0, 3.0)

        def desc(h, w, **kw):
            kw.setdefault("nbands", 1)
            dtype = kw.pop("dtype", dt)
            return ctx.make_raster_desc(h, w, dtype, **kw)

        def rejected(sd, dd, rect=good_rect, mode="average", s=src, d=dst, fill=0):
            with pytest.raises(_native.FrsError) as e:
                ctx.resample_window_device(s, sd, d, dd, rect, mode, fill)
            assert e.value.code == -1, e.value  # FRS_E_ARG
            return True

        good_s, good_d = desc(5, 9), desc(3, 5)
        ctx.resample_window_device(src, good_s, dst, good_d, good_rect, "average")  # the baseline is accepted
        # a size < 1
        assert rejected(desc(0, 9), good_d) and rejected(desc(5, 0), good_d) and rejected(desc(-1, 9), good_d)
        assert rejected(good_s, desc(0, 5)) and rejected(good_s, desc(3, 0)) and rejected(good_s, desc(3, -2))
        # row_stride < width, a band stride too small
        assert rejected(desc(5, 9, row_stride=8), good_d) and rejected(good_s, desc(3, 5, row_stride=4))
        assert rejected(desc(5, 9, nbands=2, band_stride=44), desc(3, 5, nbands=2))
        assert rejected(desc(5, 9, nbands=2), desc(3, 5, nbands=2, band_stride=14))
        # nbands outside 1..8, or unequal
        assert rejected(desc(5, 9, nbands=2), good_d) and rejected(good_s, desc(3, 5, nbands=2))
        assert rejected(desc(5, 9, nbands=9), desc(3, 5, nbands=9))
        zero_s, zero_d = desc(5, 9), desc(3, 5)
        zero_s.nbands = zero_d.nbands = 0
        assert rejected(zero_s, zero_d)
        # dtypes unequal or unknown
        bad, bad_d = desc(5, 9), desc(3, 5)
        bad.dtype = bad_d.dtype = 0
        assert rejected(bad, bad_d)
        bad.dtype = bad_d.dtype = 8
        assert rejected(bad, bad_d)
        assert rejected(good_s, desc(3, 5, dtype=np.uint16))
        # an extent that overflows 63 bits
        assert rejected(desc(5, 9, row_stride=2 ** 61), good_d) and rejected(good_s, desc(3, 5, row_stride=2 ** 61))
        assert rejected(desc(5, 9, nbands=2, band_stride=2 ** 62), desc(3, 5, nbands=2))
        # an unknown mode
        assert rejected(good_s, good_d, mode=3) and rejected(good_s, good_d, mode=-1)
        # a null or misaligned pointer
        assert rejected(good_s, good_d, s=0) and rejected(good_s, good_d, d=0)
        assert rejected(good_s, good_d, s=src + 1) and rejected(good_s, good_d, d=dst + 1)
        # overlapping byte ranges: the destination inside the source, each raster's last element
        assert rejected(good_s, good_d, d=src + 2 * 10)
        assert rejected(good_s, good_d, d=src + 2 * 44)
        assert rejected(good_s, good_d, s=dst + 2 * 14)
        # touching ranges are fine
        ctx.resample_window_device(src, good_s, src + 2 * 45, good_d, good_rect, "nearest")
        ctx.resample_window_device(dst + 2 * 15, good_s, dst, good_d, good_rect, "bilinear")
        # a non-finite map field
        for k in range(4):
            for v in (np.nan, np.inf, -np.inf):
                r = list(good_rect)
                r[k] = v
                assert rejected(good_s, good_d, rect=tuple(r))
        for v in (np.nan, np.inf, -np.inf):
            assert rejected(good_s, good_d, fill=v)
        # width <= 0 or height <= 0
        assert rejected(good_s, good_d, rect=(0.5, 0.5, 0.0, 3.0)) and rejected(good_s, good_d, rect=(0.5, 0.5, 7.0, 0.0))
        assert rejected(good_s, good_d, rect=(0.5, 0.5, -7.0, 3.0)) and rejected(good_s, good_d, rect=(0.5, 0.5, 7.0, -1.0))
        # a coordinate of magnitude >= 2^52
        big = 2.0 ** 52
        assert rejected(good_s, good_d, rect=(big, 0.5, 7.0, 3.0)) and rejected(good_s, good_d, rect=(-big, 0.5, 7.0, 3.0))
        assert rejected(good_s, good_d, rect=(0.5, big, 7.0, 3.0)) and rejected(good_s, good_d, rect=(0.5, -big, 7.0, 3.0))
        assert rejected(good_s, good_d, rect=(0.5, 0.5, big, 3.0)) and rejected(good_s, good_d, rect=(0.5, 0.5, 7.0, big))
        assert rejected(good_s, good_d, rect=(big / 2, 0.5, big / 2, 3.0))  # x0 + width
        # just below it, and wholly outside: FRS_OK, the destination is filled
        ctx.resample_window_device(src, good_s, dst, good_d, (big / 4, -big / 4, 7.0, 3.0), "average", 7)
        got = np.empty(15, dtype=dt)
        buf.download(30, 2048, out=got.view(np.uint8))
        assert np.array_equal(got, np.full(15, 7, dtype=dt))
        with pytest.raises(ValueError):
            ctx.resample_window_device(src, good_s, dst, good_d, good_rect, "cubic")
    finally:
        buf.close()


def test_downsample2_still_rejects_mode_2(gpu_ctx):
    ctx = gpu_ctx
    buf = ctx.alloc(4096)
    try:
        buf.upload(np.zeros(2048, dtype=np.int16))
        sd, dd = ctx.make_raster_desc(5, 9, np.int16), ctx.make_raster_desc(3, 5, np.int16)
        ctx.downsample2_device(buf.ptr, sd, buf.ptr + 2048, dd, 1)
        with pytest.raises(_native.FrsError) as e:
            ctx.downsample2_device(buf.ptr, sd, buf.ptr + 2048, dd, _native.RESAMPLE_BILINEAR)
        assert e.value.code == -1
        with pytest.raises(ValueError):
            ctx.downsample2_device(buf.ptr, sd, buf.ptr + 2048, dd, "bilinear")
    finally:
        buf.close()


# ------------------------------------------------------------------------------------------------ the file path
W, H, TILE = 300, 420, 64
T = geotiff.Affine(0.5, 0.0, 100.0, 0.0, -0.5, 200.0)
CRS = "EPSG:32633"
OUT_W, OUT_H = 12, 16


def _px_bbox(c0, r0, c1, r1):
    """the bbox of level-0 pixel-edge columns c0..c1 and rows r0..r1"""
    return [T.c + c0 * T.a, T.f + r1 * T.e, T.c + c1 * T.a, T.f + r0 * T.e]


# name -> (bbox, out_w, out_h, the level window_request must pick)
BOXES = {f"inside_scale_{s}": (_px_bbox(30.3, 50.7, 30.3 + OUT_W * s, 50.7 + OUT_H * s), OUT_W, OUT_H, k)
         for s, k in ((0.5, 0), (1.5, 0), (3, 1), (20, 3))}
BOXES["over_two_edges"] = (_px_bbox(-10.5, -7.25, 50.0, 40.0), 20, 15, 1)
BOXES["outside"] = (_px_bbox(400.0, 10.0, 450.0, 50.0), 9, 7, None)


@pytest.fixture(scope="module")
def band():
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:H, 0:W]
    base = 1000 + 300 * np.sin(0.05 * x) * np.cos(0.07 * y) + rng.integers(-40, 41, size=(H, W))
    b = np.round(base - 1200).astype(np.int16)
    b.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def stream_file(gpu_ctx, band, tmp_path_factory):
    """(path, index, [band, level 1, 2, 3] in numpy): written once; every level reads back as the numpy pyramid"""
    p = tmp_path_factory.mktemp("window") / "band.flac"
    index = streaming.create_streaming_array(band, T, CRS, p, tile_size=TILE, ctx=gpu_ctx, overviews=True)
    pyr = np_pyramid(band, streaming.overview_shapes(H, W, TILE), "average")
    assert len(pyr) == 4
    for k, a in enumerate(pyr):
        a.setflags(write=False)
        assert np.array_equal(streaming.reconstruct(p, gpu_ctx, level=k)[0][0], a), k
    return p, index, pyr


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", list(BOXES))
def test_read_window_equals_the_restatement_on_the_pyramid(gpu_ctx, stream_file, name, mode):
    path, index, pyr = stream_file
    bbox, ow, oh, level = BOXES[name]
    req = streaming.window_request(index, bbox, ow, oh)
    arr, tr = streaming.read_window(path, bbox, ow, oh, resampling=mode, fill=-7, ctx=gpu_ctx)
    assert arr.shape == (1, oh, ow) and arr.dtype == np.int16
    assert tr == req["transform"] == [(bbox[2] - bbox[0]) / ow, 0.0, bbox[0], 0.0, -(bbox[3] - bbox[1]) / oh, bbox[3]]
    if level is None:
        assert req["frames"] == [] and np.array_equal(arr, np.full((1, oh, ow), -7, dtype=np.int16))
        return
    assert req["level"] == level
    win = req["window"]
    sub = pyr[level][win["row_off"]:win["row_off"] + win["height"], win["col_off"]:win["col_off"] + win["width"]]
    assert sub.shape == (win["height"], win["width"])
    want = R.resample(sub, req["rect"], (oh, ow), mode, -7)
    assert np.array_equal(arr[0], want)
    if name == "over_two_edges":
        assert (want == -7).any() and (want != -7).any()


def test_read_window_with_a_forced_level(gpu_ctx, stream_file):
    path, index, pyr = stream_file
    bbox, ow, oh, _ = BOXES["inside_scale_3"]
    req = streaming.window_request(index, bbox, ow, oh, level=0)
    arr, _ = streaming.read_window(path, bbox, ow, oh, resampling="average", level=0, ctx=gpu_ctx)
    win = req["window"]
    sub = pyr[0][win["row_off"]:win["row_off"] + win["height"], win["col_off"]:win["col_off"] + win["width"]]
    assert np.array_equal(arr[0], R.resample(sub, req["rect"], (oh, ow), "average", 0))
    with pytest.raises(ValueError, match="nearest, bilinear, average"):
        streaming.read_window(path, bbox, ow, oh, resampling="cubic", ctx=gpu_ctx)


def test_cli_writes_the_window_as_a_geotiff(gpu_ctx, stream_file, tmp_path):
    path, index, pyr = stream_file
    bbox, ow, oh, level = BOXES["inside_scale_3"]
    out = tmp_path / "window.tif"
    r = runner.invoke(app, ["extract-streaming", str(path), "--bbox", ",".join(repr(v) for v in bbox), "--out-size",
                            f"{ow}x{oh}", "--resampling", "bilinear", "--fill", "-7", "-o", str(out)])
    assert r.exit_code == 0, r.output
    assert f"SUCCESS: window {ow}x{oh} (level {level}, bilinear) -> {out}" in r.output
    t = geotiff.read(out)
    want, tr = streaming.read_window(path, bbox, ow, oh, resampling="bilinear", fill=-7, ctx=gpu_ctx)
    assert t.data.shape == (1, oh, ow) and np.array_equal(t.data, want)
    assert list(t.transform)[:6] == pytest.approx(tr, rel=0, abs=0)
    assert t.crs_string == CRS
    # the default mode and a forced level
    r = runner.invoke(app, ["extract-streaming", str(path), "--bbox", ",".join(repr(v) for v in bbox), "--out-size",
                            f"{ow}x{oh}", "--level", "2", "-o", str(out)])
    assert r.exit_code == 0, r.output
    assert f"SUCCESS: window {ow}x{oh} (level 2, average) -> {out}" in r.output
    assert np.array_equal(geotiff.read(out).data, streaming.read_window(path, bbox, ow, oh, level=2, ctx=gpu_ctx)[0])
