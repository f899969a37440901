"""The 2x pyramid step on the GPU (csrc/frs_pyramid.hip): frs_downsample2_device against a numpy restatement of
csrc/frs_resample.h's definition, on the smallest shapes that reach every path of the kernel (partial blocks of odd
sizes, rows that start and end on and off a 16-byte boundary, one chunk more or less than a whole number of them),
strided sub-views with sentinels in all padding, every argument error, and the host variant."""
import numpy as np
import pytest

from flac_raster_amd import _native
from tests.pyramid_ref import np_downsample2

pytestmark = pytest.mark.gpu

ALL_DTYPES = [np.uint8, np.uint16, np.int16, np.int32, np.uint32, np.float32, np.float64]
MODES = ["nearest", "average"]

# (height, width) of the source.  Widths 2w and 2w - 1 give w = 15, 16, 17, 31, 32, 33 outputs: one less than, exactly
# and one more than one and two 16-byte chunks of uint8, two and four of the 16-bit dtypes, ... with even and odd heights
SMALL = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 37), (37, 1)]
EDGES = [(h, 2 * w - odd) for w in (15, 16, 17, 31, 32, 33) for odd in (0, 1) for h in (4, 5)]
SHAPES = SMALL + EDGES + [(203, 301)]


def _values(rng, dtype, shape):
    dt = np.dtype(dtype)
    C, H, W = shape
    if dt.kind == "f":
        v = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(dt)
        flat = v.reshape(-1)
        if flat.size >= 8:
            flat[rng.integers(0, flat.size, 3)] = [np.nan, np.inf, -np.inf]
        return v
    ii = np.iinfo(dt)
    v = rng.integers(ii.min, ii.max, size=shape, dtype=dt, endpoint=True)
    # a quarter of the elements at each extreme, then whole blocks of them and each extreme alone in each position
    pick = rng.integers(0, 4, size=shape)
    v[pick == 0], v[pick == 1] = ii.min, ii.max
    blocks = [(r, c) for r in range(0, H - 1, 2) for c in range(0, W - 1, 2)]
    fills = [(ii.max,) * 4, (ii.min,) * 4] + [tuple(e if k == p else o for k in range(4))
                                              for e, o in ((ii.max, ii.min), (ii.min, ii.max), (ii.min, -1 if ii.min else 1))
                                              for p in range(4)]
    for (r, c), f in zip(blocks, fills):
        v[:, r:r + 2, c:c + 2] = np.array(f, dtype=dt).reshape(2, 2)
    return v


def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


def _run(ctx, a, mode, pad=0, slack=0, lead=0):
    """frs_downsample2_device on `a` (C, H, W) laid out with row_stride = width + pad, band_stride = rows + slack and
    its origin `lead` elements into a sentinel-filled device buffer, into a destination laid out the same way.
    Returns (whole destination buffer, what it must hold)."""
    dt = a.dtype
    C, H, W = a.shape
    h, w = (H + 1) // 2, (W + 1) // 2

    def layout(hh, ww):
        rs = ww + pad
        bs = rs * hh + slack
        return rs, bs, lead + (C - 1) * bs + (hh - 1) * rs + ww + lead

    def view(buf, hh, ww, rs, bs):
        return np.lib.stride_tricks.as_strided(buf[lead:], shape=(C, hh, ww),
                                               strides=(bs * dt.itemsize, rs * dt.itemsize, dt.itemsize))
    srs, sbs, sext = layout(H, W)
    drs, dbs, dext = layout(h, w)
    src = np.full(sext, _sentinel(dt), dtype=dt)
    view(src, H, W, srs, sbs)[...] = a
    want = np.full(dext, _sentinel(dt), dtype=dt)
    view(want, h, w, drs, dbs)[...] = np_downsample2(a, mode)
    sb, db = ctx.alloc(src.nbytes), ctx.alloc(want.nbytes)
    try:
        sb.upload(src)
        db.upload(np.full(dext, _sentinel(dt), dtype=dt))
        sd = ctx.make_raster_desc(H, W, dt, nbands=C, row_stride=srs, band_stride=sbs)
        dd = ctx.make_raster_desc(h, w, dt, nbands=C, row_stride=drs, band_stride=dbs)
        ctx.downsample2_device(sb.ptr + lead * dt.itemsize, sd, db.ptr + lead * dt.itemsize, dd, mode)
        got = np.empty(dext, dtype=dt)
        db.download(out=got.view(np.uint8))
    finally:
        sb.close()
        db.close()
    return got, want


def _same(got, want):
    if got.dtype.kind == "f":  # NaN payloads are the hardware's: NaN in the same places, the same bits elsewhere
        n = np.isnan(want)
        assert np.array_equal(np.isnan(got), n)
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        return np.array_equal(got.view(u)[~n], want.view(u)[~n])
    return np.array_equal(got, want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_downsample_dense(gpu_ctx, dtype, mode):
    rng = np.random.default_rng(3)
    for H, W in SHAPES:
        for C in (1, 3):
            a = _values(rng, dtype, (C, H, W))
            got, want = _run(gpu_ctx, a, mode)
            assert _same(got, want), (H, W, C)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_downsample_strided_subviews_keep_every_sentinel(gpu_ctx, dtype, mode):
    """row_stride = width + 3 on both sides, band planes with slack, both origins one element past a 16-byte boundary
    of a larger buffer: the row and band padding and the elements before and after the rasters keep their sentinel."""
    rng = np.random.default_rng(4)
    for H, W in SHAPES:
        for C in (1, 3):
            a = _values(rng, dtype, (C, H, W))
            got, want = _run(gpu_ctx, a, mode, pad=3, slack=5, lead=1)
            assert _same(got, want), (H, W, C)


def test_downsample_row_longer_than_one_step(gpu_ctx):
    """A row of more chunks than one work-group step covers (2 x 256 chunks): several work-groups per row and the
    stride over what the whole steps leave; float64 has the fewest outputs per chunk."""
    rng = np.random.default_rng(6)
    for dtype, W in ((np.float64, 2 * 2600 + 1), (np.int16, 2 * 9000)):
        a = _values(rng, dtype, (1, 3, W))
        got, want = _run(gpu_ctx, a, "average", pad=1, lead=1)
        assert _same(got, want), (dtype, W)


def test_downsample_host_variant(gpu_ctx):
    rng = np.random.default_rng(8)
    for (H, W), dtype, mode in (((5, 33), np.int16, "average"), ((203, 301), np.float32, "average"),
                                ((4, 7), np.uint8, "nearest")):
        a = _values(rng, dtype, (3, H, W))
        assert _same(gpu_ctx.downsample2_host(a, mode), np_downsample2(a, mode))
        assert _same(gpu_ctx.downsample2_host(a[0], mode), np_downsample2(a[:1], mode)[0])


def test_downsample_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    dt = np.dtype(np.int16)
    buf = ctx.alloc(4096)
    try:
        buf.upload(np.zeros(2048, dtype=dt))
        src, dst = buf.ptr, buf.ptr + 2048

        def desc(h, w, **kw):
            kw.setdefault("nbands", 1)
            dtype = kw.pop("dtype", dt)
            return ctx.make_raster_desc(h, w, dtype, **kw)

        def rejected(sd, dd, mode="average", s=src, d=dst):
            with pytest.raises(_native.FrsError) as e:
                ctx.downsample2_device(s, sd, d, dd, mode)
            assert e.value.code == -1, e.value  # FRS_E_ARG
            return True

        good_s, good_d = desc(5, 9), desc(3, 5)
        ctx.downsample2_device(src, good_s, dst, good_d, "average")  # the baseline is accepted
        # sizes: not ceil(src / 2), below 1
        assert rejected(good_s, desc(2, 5)) and rejected(good_s, desc(3, 4)) and rejected(good_s, desc(3, 6))
        assert rejected(desc(0, 9), desc(0, 5)) and rejected(desc(5, 0), desc(3, 0))
        assert rejected(desc(-1, 9), desc(0, 5))
        # strides
        assert rejected(desc(5, 9, row_stride=8), good_d) and rejected(good_s, desc(3, 5, row_stride=4))
        assert rejected(desc(5, 9, nbands=2, band_stride=44), desc(3, 5, nbands=2))
        assert rejected(desc(5, 9, nbands=2), desc(3, 5, nbands=2, band_stride=14))
        # dtype, nbands, mode
        bad = desc(5, 9)
        bad.dtype = 0
        bad_d = desc(3, 5)
        bad_d.dtype = 0
        assert rejected(bad, bad_d)
        bad.dtype = bad_d.dtype = 8
        assert rejected(bad, bad_d)
        assert rejected(good_s, desc(3, 5, dtype=np.uint16))
        assert rejected(desc(5, 9, nbands=2), good_d)
        assert rejected(desc(5, 9, nbands=9), desc(3, 5, nbands=9))
        zero_s, zero_d = desc(5, 9), desc(3, 5)
        zero_s.nbands = zero_d.nbands = 0
        assert rejected(zero_s, zero_d)
        assert rejected(good_s, good_d, mode=2) and rejected(good_s, good_d, mode=-1)
        # pointers: null, not aligned to the element
        assert rejected(good_s, good_d, s=0) and rejected(good_s, good_d, d=0)
        assert rejected(good_s, good_d, s=src + 1) and rejected(good_s, good_d, d=dst + 1)
        # overlapping ranges: the destination inside the source, the source's last element, the destination's last
        assert rejected(good_s, good_d, d=src + 2 * 10)
        assert rejected(good_s, good_d, d=src + 2 * 44)
        assert rejected(good_s, good_d, s=dst + 2 * 14)
        # touching ranges are fine
        ctx.downsample2_device(src, good_s, src + 2 * 45, good_d, "nearest")
        ctx.downsample2_device(dst + 2 * 15, good_s, dst, good_d, "nearest")
        with pytest.raises(ValueError):
            ctx.downsample2_device(src, good_s, dst, good_d, "cubic")
    finally:
        buf.close()
