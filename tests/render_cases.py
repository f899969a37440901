"""The cases tests/test_gpu_render.py and tests/test_render_host.py share: a 37 x 53 source under four masks, the
destination sizes and rectangles, the LUT lengths, a random LUT, and stretch limits inside the data's range."""
import struct
import zlib

import numpy as np

SRC_H, SRC_W = 37, 53
SIZES = ((1, 1), (5, 7), (17, 33), (3, 130), (40, 9))  # (h, w)
RECTS = ("scale_to_fit", "9.3x", "0.4x_upsampling", "over_all_edges", "outside_right")
MASKS = ("none", "all", "random30", "collar")
LUT_SIZES = (1, 256, 4096)
PAD, LEAD = 3, 1  # row padding and bytes (source: elements) before the raster's origin


def nodata_of(dtype):
    """the nodata value the masked cases use"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return float("nan") if dt == np.float32 else 0.0
    return int(np.iinfo(dt).min) if dt.kind == "i" else 0


def limits(dtype):
    """(lo, hi) inside the data's range, so that both clamps are hit; neither is an integer for the wide dtypes"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return -5.25, 50.5
    ii = np.iinfo(dt)
    span = float(ii.max) - float(ii.min)
    return float(ii.min) + span * 0.25, float(ii.max) - span * 0.3125


def lut_of(n, seed=77):
    """a random LUT, so that a wrong index shows: uint8 (n, 4)"""
    return np.random.default_rng(seed).integers(0, 256, size=(n, 4), dtype=np.uint8)


def _is_nodata(v, nd):
    if v.dtype.kind == "f":
        return (v == v.dtype.type(nd)) | (np.isnan(v) & bool(np.isnan(nd)))
    return v == v.dtype.type(nd)


def make_source(rng, dtype, mask, nd):
    """(37, 53) values none of which is nodata (floats with NaN and both infinities where those are not nodata), then
    `nd` where the mask says so"""
    dt = np.dtype(dtype)
    shape = (SRC_H, SRC_W)
    if dt.kind == "f":
        v = (rng.standard_normal(shape) * 10.0 ** rng.integers(-1, 3, size=shape)).astype(dt)
        v[5, 7], v[20, 30], v[30, 2] = np.nan, np.inf, -np.inf
        v[_is_nodata(v, nd)] = dt.type(1.5)
    else:
        ii = np.iinfo(dt)
        v = rng.integers(ii.min, ii.max, size=shape, dtype=dt, endpoint=True)
        pick = rng.integers(0, 8, size=shape)
        v[pick == 0], v[pick == 1] = ii.min, ii.max
        v[v == dt.type(nd)] = dt.type(nd + 1 if nd < ii.max else nd - 1)
    m = np.zeros(shape, dtype=bool)
    if mask == "all":
        m[...] = True
    elif mask == "random30":
        m[...] = rng.random(shape) < 0.3
    elif mask == "collar":
        m[...] = True
        m[6:-6, 8:-8] = False
        m[15:18, 20:26] = True  # and a hole
    v[m] = dt.type(nd)
    return v


def read_png(data: bytes) -> np.ndarray:
    """a small reader: 8-bit colour types 0, 4 and 6, filter type 0 on every row, every chunk's CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    c = {0: 1, 4: 2, 6: 4}[ctype]
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + w * c)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, c)
