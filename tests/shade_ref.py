"""numpy restatement of the hillshaded render (csrc/frs_shade.h, frs_render_shaded_window*), written from the definition
in include/flac_raster_amd.h and not from the C++, on top of the unchanged restatements of the windowed resample and of
the render (tests/window_ref.py, tests/nodata_ref.py, tests/render_ref.py).  fp64 throughout, every numpy operation one
IEEE operation; np.sqrt is correctly rounded.

The samples at output positions -1 .. n come from window_ref itself: its `axis` is evaluated at j = -1 .. n with the
call's own step (span / n) while the unchanged resample code runs on an (h + 2, w + 2) grid."""
import contextlib

import numpy as np

from tests import render_ref as RR
from tests import window_ref as R


@contextlib.contextmanager
def _positions_minus_one_to_n():
    """window_ref.axis over n + 2 positions j = -1 .. n of an n-pixel axis (same expressions, same step)"""
    def axis(x0, span, n2, N):
        x0, step = np.float64(x0), np.float64(span) / np.float64(n2 - 2)
        j = np.arange(n2, dtype=np.float64) - 1.0
        return x0 + j * step, x0 + (j + 1.0) * step, x0 + (j + 0.5) * step
    keep = R.axis
    R.axis = axis
    try:
        yield
    finally:
        R.axis = keep


def samples(src, rect, out_shape, mode, nd):
    """float64 (h + 2, w + 2): the samples at output positions -1 .. h and -1 .. w, NaN where there is no data"""
    h, w = out_shape
    with _positions_minus_one_to_n():
        v, has = RR.resampled(src, rect, (h + 2, w + 2), mode, nd)
    return np.where(has, v.astype(np.float64), np.nan)


def level(z, light, kx, ky):
    """shade levels (int64) of neighbourhoods z[..., 3, 3] (rows north to south) whose values are all data"""
    z = np.asarray(z, dtype=np.float64)
    lx, ly, lz = (np.float64(v) for v in light)
    kx, ky = np.float64(kx), np.float64(ky)
    g = lambda dy, dx: z[..., dy + 1, dx + 1]
    with np.errstate(all="ignore"):
        gx = ((g(-1, 1) + (g(0, 1) + g(0, 1))) + g(1, 1)) - ((g(-1, -1) + (g(0, -1) + g(0, -1))) + g(1, -1))
        gy = ((g(1, -1) + (g(1, 0) + g(1, 0))) + g(1, 1)) - ((g(-1, -1) + (g(-1, 0) + g(-1, 0))) + g(-1, 1))
        p = gx * kx
        q = gy * ky
        num = (lz - p * lx) + q * ly
        den = np.sqrt((1.0 + p * p) + q * q)
        s = num / den
        pos = s > 0
        k = np.minimum(np.floor(np.where(pos, s, 0.0) * 256.0), 255.0).astype(np.int64)
    return np.where(pos, k, 0)


def neighbourhoods(zs):
    """(h, w, 3, 3) of the (h + 2, w + 2) samples, a neighbour without data replaced by the centre"""
    h, w = zs.shape[0] - 2, zs.shape[1] - 2
    out = np.empty((h, w, 3, 3), dtype=np.float64)
    centre = zs[1:h + 1, 1:w + 1]
    for dy in range(3):
        for dx in range(3):
            n = zs[dy:dy + h, dx:dx + w]
            out[:, :, dy, dx] = np.where(np.isnan(n), centre, n)
    return out


def shade_colours(zs, lo, hi, lut, nodata_rgba, channels, light, kx, ky, table):
    """uint8 (h, w, channels) from the (h + 2, w + 2) samples"""
    lut = np.asarray(lut, dtype=np.uint8)
    table = np.asarray(table, dtype=np.uint8)
    h, w = zs.shape[0] - 2, zs.shape[1] - 2
    centre = zs[1:h + 1, 1:w + 1]
    has = ~np.isnan(centre)
    k = level(np.where(has[..., None, None], neighbourhoods(zs), 0.0), light, kx, ky)
    m = table[k].astype(np.int64)
    idx = RR.quantise(np.where(has, centre, 0.0), lo, hi, len(lut))
    rgba = lut[idx].astype(np.int64)
    rgba[..., :3] = (rgba[..., :3] * m[..., None] + 127) // 255
    rgba = np.where(has[..., None], rgba, np.array(RR.unpack_rgba(nodata_rgba), dtype=np.int64))
    return np.ascontiguousarray(rgba[..., RR.CHANNELS[channels]]).astype(np.uint8)


def render_shaded(src, rect, out_shape, mode, nd, lo, hi, lut, nodata_rgba, channels, light, kx, ky, table):
    """src (H, W) -> uint8 (h, w, channels)"""
    return shade_colours(samples(src, rect, out_shape, mode, nd), lo, hi, lut, nodata_rgba, channels, light, kx, ky,
                         table)
