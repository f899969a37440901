"""numpy restatement of the 8-bit render (csrc/frs_render.h, frs_render_window*), written from the definition and not
from the C++, on top of the unchanged restatements of the windowed resample (tests/window_ref.py, tests/nodata_ref.py).

One output pixel comes from a resampled value v in the source dtype and a flag has_data.  v is what the resample gives;
has_data is false where the resample writes `fill` -- found here by resampling twice with two different fills and taking
the pixels where the two results agree -- and, for floats, where v is NaN.  Quantise: scale = n / (hi - lo) once;
x = float64(v) < lo gives 0, x > hi gives n - 1, else min(floor((x - lo) * scale), n - 1), every numpy operation one
IEEE fp64 operation.  Colour: lut[index], or nodata_rgba without data.  Channels: 1 = R, 2 = R, A, 4 = R, G, B, A."""
import numpy as np

from tests import nodata_ref as N
from tests import window_ref as R

CHANNELS = {1: [0], 2: [0, 3], 4: [0, 1, 2, 3]}


def quantise(v, lo, hi, n):
    """LUT indices (int64) of the values v, none of which is NaN"""
    x = np.asarray(v).astype(np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(n) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = ~(x < lo) & ~(x > hi)
        b = np.floor((np.where(inside, x, lo) - lo) * scale).astype(np.int64)
    b = np.minimum(b, n - 1)
    return np.where(x < lo, 0, np.where(x > hi, n - 1, b))


def unpack_rgba(rgba):
    """(r, g, b, a) of a packed value R | G << 8 | B << 16 | A << 24, or of such a tuple"""
    if isinstance(rgba, (int, np.integer)):
        rgba = int(rgba)
        return (rgba & 0xFF, (rgba >> 8) & 0xFF, (rgba >> 16) & 0xFF, (rgba >> 24) & 0xFF)
    return tuple(int(x) for x in rgba)


def resampled(src, rect, out_shape, mode, nd):
    """(v, has_data) of the (H, W) source: the resample's output and where it is not `fill`"""
    src = np.asarray(src)
    assert src.ndim == 2
    f = (lambda fill: R.resample(src, rect, out_shape, mode, fill)) if nd is None else \
        (lambda fill: N.resample_nodata(src, rect, out_shape, mode, fill, nd))
    a, b = f(0), f(1)
    if src.dtype.kind == "f":
        agree = (a == b) | (np.isnan(a) & np.isnan(b))
        return a, agree & ~np.isnan(a)
    return a, a == b


def colours(v, has_data, lo, hi, lut, nodata_rgba, channels):
    """uint8 (h, w, channels) of resampled values and their has_data flags"""
    lut = np.asarray(lut, dtype=np.uint8)
    assert lut.ndim == 2 and lut.shape[1] == 4
    idx = quantise(np.where(has_data, v, v.dtype.type(0)), lo, hi, len(lut))
    rgba = np.where(has_data[..., None], lut[idx], np.array(unpack_rgba(nodata_rgba), dtype=np.uint8))
    return np.ascontiguousarray(rgba[..., CHANNELS[channels]]).astype(np.uint8)


def render(src, rect, out_shape, mode, nd, lo, hi, lut, nodata_rgba, channels):
    """src (H, W) -> uint8 (h, w, channels)"""
    v, has = resampled(src, rect, out_shape, mode, nd)
    return colours(v, has, lo, hi, lut, nodata_rgba, channels)
