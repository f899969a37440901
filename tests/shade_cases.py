"""The cases tests/test_shade_host.py and tests/test_gpu_shade.py share: the 37 x 53 sources of tests/render_cases.py,
the destination sizes around the shade kernel's tile (16 rows x 256 / C pixels), the rectangles, and the expected
buffers from tests/shade_ref.py, computed once per (dtype, mode, nodata) and kept."""
import functools

import numpy as np

from tests import render_ref as RR
from tests import shade_ref as SR
from tests import window_ref as R
from tests.render_cases import PAD, SRC_H, SRC_W, limits, lut_of, make_source, nodata_of

TH = 16
LIGHT = (-0.5, 0.5, 0.7071067811865476)  # 315 degrees, 45 degrees


def TW(C):
    return 256 // C


def scales(dtype):
    """(kx, ky) that put p and q around 1 for the random sources"""
    dt = np.dtype(dtype)
    span = 400.0 if dt.kind == "f" else float(np.iinfo(dt).max) - float(np.iinfo(dt).min)
    return 2.0 / span, 3.0 / span


def table():
    return (255 - np.arange(256) * 3 // 4).astype(np.uint8)[::-1].copy()  # not the identity, ascending


def geometries(C):
    """(h, w, rect name, lead, row padding) of the destinations for C channels"""
    tw = TW(C)
    names = ("scale_to_fit", "1.37x", "0.4x_upsampling", "9.3x", "lo_on_pixel_edges")
    out = [(1, 1, "scale_to_fit", 0, 0)]
    k = 0
    for h in (TH - 1, TH, TH + 1):
        for w in (tw - 1, tw, tw + 1):
            out.append((h, w, names[k % len(names)], 0, 0 if k % 2 else 16 - (w * C) % 16))
            k += 1
    out.append((TH + 3, tw + 5, "scale_to_fit", 1, PAD if (tw + 5) * C % 2 == 0 else PAD + 1))  # odd row stride
    for name in ("over_left_top", "over_right_bottom", "over_all_edges", "outside_right"):
        out.append((TH + 1, 33, name, 0, PAD))
    return out


@functools.lru_cache(maxsize=None)
def source(dtype_name, masked):
    dt = np.dtype(dtype_name)
    rng = np.random.default_rng(91)
    return make_source(rng, dt, "collar" if masked else "none", nodata_of(dt))


@functools.lru_cache(maxsize=None)
def cases(dtype_name, mode, masked):
    """[(C, n, rgba, rect, h, w, drs, lead, expected buffer)] for one source; the buffer is lead + (h - 1) * drs + w * C
    bytes, 0xa5 outside the destination"""
    dt = np.dtype(dtype_name)
    a = source(dtype_name, masked)
    nd = nodata_of(dt) if masked else None
    lo, hi = limits(dt)
    kx, ky = scales(dt)
    out = []
    for C in (1, 2, 4):
        for i, (h, w, rname, lead, pad) in enumerate(geometries(C)):
            rect = R.rects(SRC_W, SRC_H, w, h)[rname]
            n = (256, 4096, 1)[i % 3] if i else 256
            rgba = 0x80402010 + n + C
            drs = w * C + pad
            zs = SR.samples(a, rect, (h, w), mode, nd)
            img = SR.shade_colours(zs, lo, hi, lut_of(4096)[:n], rgba, C, LIGHT, kx, ky, table())
            want = np.full(lead + (h - 1) * drs + w * C, 0xA5, dtype=np.uint8)
            np.lib.stride_tricks.as_strided(want[lead:], shape=(h, w * C), strides=(drs, 1))[...] = \
                img.reshape(h, w * C)
            out.append((C, n, rgba, rect, h, w, drs, lead, want))
    return out


def plain(dtype_name, mode, masked, C, rect, h, w, n, rgba):
    """the plain render's image of the same case"""
    dt = np.dtype(dtype_name)
    lo, hi = limits(dt)
    return RR.render(source(dtype_name, masked), rect, (h, w), mode, nodata_of(dt) if masked else None, lo, hi,
                     lut_of(4096)[:n], rgba, C)
