"""numpy restatement of the three-band composite (csrc/frs_composite.h, frs_render_composite_window*) and the cases its
host and GPU tests share.  The restatement is tests/render_ref.py applied per plane, plus the rule that a pixel where any
plane has no data is nodata_rgba, whole: for c in {0, 1, 2} byte c of the pixel is byte c of lut[index of plane c's value
under lo[c], hi[c]], and A is 255."""
import numpy as np

from tests import render_ref as RR
from tests.render_cases import limits, make_source, nodata_of

DTYPES = (np.int16, np.uint8, np.float32)
# the mask of each plane (tests/render_cases.make_source): the holes differ, so that "any plane" is exercised
PLANE_MASKS = (("none", "none", "none"), ("random30", "collar", "none"), ("collar", "random30", "random30"),
               ("none", "all", "random30"))
BAND_PAD = 5  # elements between the end of a plane and the start of the next
LEADS = tuple(range(16))  # destination origins: every position within a 16-byte chunk


def channel_limits(dtype):
    """((lo_r, lo_g, lo_b), (hi_r, hi_g, hi_b)): three different stretches inside the data's range"""
    lo, hi = limits(dtype)
    span = hi - lo
    return (lo, lo + 0.125 * span, lo), (hi, hi, hi - 0.25 * span)


def make_planes(rng, dtype, masks):
    """(3, 37, 53): one make_source per plane"""
    return np.stack([make_source(rng, dtype, m, nodata_of(dtype)) for m in masks])


def composite(planes, rect, out_shape, mode, nd, lo3, hi3, lut, nodata_rgba):
    """planes (3, H, W) -> uint8 (h, w, 4)"""
    planes = np.asarray(planes)
    assert planes.ndim == 3 and planes.shape[0] == 3
    h, w = out_shape
    out = np.empty((h, w, 4), dtype=np.uint8)
    has_all = np.ones((h, w), dtype=bool)
    for c in range(3):
        v, has = RR.resampled(planes[c], rect, out_shape, mode, nd)
        out[..., c] = RR.colours(v, has, lo3[c], hi3[c], lut, 0, 4)[..., c]
        has_all &= has
    out[..., 3] = 255
    out[~has_all] = np.array(RR.unpack_rgba(nodata_rgba), dtype=np.uint8)
    return out
