"""Rasters and memory layouts for the encoder's alignment classes, shared by tests/test_encode_layouts_host.py and
tests/test_gpu_encode_layouts.py.

The level-5 fast encoders load 64- (or 16-) sample row segments with the instruction their job's alignment class
allows (EncodeParams::vec_ok, flac_raster_amd._native.encode_align_class): 16-, 8- or 4-byte vector loads, or the
element gather.  The class follows from the address of the first band's origin, the row stride, the tile width and,
with several bands, the band stride; the output never depends on it.  So every content here is encoded from a set of
layouts -- a parent buffer and an element-strided view of it -- that reaches every class, and compared with the
oracle's bytes for the contiguous copy.

Contents (each small: every tile is one to a few 4096-sample frames, but the Sentinel-2 row's):
  mono     512 x 208 at 128 x 128 tiles: four tile rows of a 128-wide column (a multiple of 64: every kernel takes the
           class) and an 80-wide edge column (a multiple of 16 only: two frames and a 2048-sample tail; the slow analysis
           takes the class, the lean analysis and the encoder gather).  The tile grid is uniform with truncated edge
           tiles, so the edge column is what is left of the width after whole tiles.  Every normalisation mode of
           frs_normalize.h that the dtype allows occurs in both columns (MONO_MODES).
  stereo   two correlated bands, 256 x 64, one stream of four frames (FastStereo).
  multi    three bands, 256 x 64, one stream (FastMulti).
  raw      norm_mode 1 (32-bit streams, the generic path with k_zero_subframes): one and three bands, 128 x 64 at
           64 x 64 tiles: the first tile's frames are all-zero, the second's are not.  (Checked on the CPU only for
           now: see tests/test_gpu_encode_layouts.py.)
  s2row    a 64 x 10980 uint16 strip at 1024 x 1024 tiles: the Sentinel-2 row, whose dense rows (21960 bytes) are class 8.
Data stay strictly inside the dtype's range, so the parents' padding (alternately the dtype's minimum and maximum) lies
outside every tile's min..max: one element read from outside the view moves a tile's extremes or a sample.  The one
exception is raw uint8, whose only non-zero samples come from 0 and 255 (Content.inside is False there).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import oracle as O

RATE = 44100
FRAME = 4096
LUT, FASTDIV, SLOW, ZERO = 0, 1, 2, 3        # frs_normalize.h kNorm*
MODE_NAMES = {LUT: "lut", FASTDIV: "fastdiv", SLOW: "slow", ZERO: "zero"}

MONO_H, MONO_W, MONO_TILE = 512, 208, 128
# the mode of tile (tile row, column) per dtype: column 0 is 128 wide, column 1 the 80-wide edge
MONO_MODES = {
    "uint8": [(LUT, ZERO), (ZERO, LUT), (LUT, LUT), (LUT, LUT)],
    "uint16": [(LUT, FASTDIV), (FASTDIV, LUT), (ZERO, FASTDIV), (FASTDIV, ZERO)],
    "int16": [(LUT, FASTDIV), (FASTDIV, SLOW), (ZERO, LUT), (SLOW, ZERO)],
}
STREAM_H, STREAM_W = 256, 64
RAW_H, RAW_W, RAW_TILE = 128, 64, 64
S2_H, S2_W, S2_TILE = 64, 10980, 1024

Content = namedtuple("Content", "name kind dtype data tile_h tile_w norm_mode inside")
Layout = namedtuple("Layout", "name lead row_res band_res")  # bytes; the residues are mod 16
Placed = namedtuple("Placed", "parent view lead row_stride band_stride")  # strides in elements, lead in bytes


# ------------------------------------------------------------------------------------------------------- contents
def _smooth(n, rng, period):
    t = np.arange(n)
    return 0.5 + 0.35 * np.sin(t / period) + 0.1 * np.sin(t / 7.3) + rng.normal(0, 0.01, n)


def _mono_tile(mode, dtype, h, w, rng):
    """an h x w tile of `dtype` whose extremes give normalisation mode `mode`, strictly inside the dtype's range"""
    dt = np.dtype(dtype)
    centre = {"uint8": 120, "uint16": 30000, "int16": 500}[dt.name]
    span = {LUT: 150 if dt.itemsize == 1 else 1800, FASTDIV: 21000, SLOW: 60000, ZERO: 0}[mode]
    s = np.clip(_smooth(h * w, rng, 90.0), 0.0, 1.0)
    v = np.rint(centre - span / 2 + span * s).astype(np.int64)
    if mode != ZERO:                       # the extremes are attained, so the range is the intended one
        v[rng.integers(0, h * w)] = centre - span // 2
        v[rng.integers(0, h * w)] = centre - span // 2 + span
    return v.reshape(h, w).astype(dt)


@lru_cache(maxsize=None)
def mono(dtype):
    rng = np.random.default_rng(7100 + np.dtype(dtype).itemsize + (np.dtype(dtype).kind == "i"))
    a = np.empty((MONO_H, MONO_W), dtype=dtype)
    for tr, modes in enumerate(MONO_MODES[dtype]):
        for tc, mode in enumerate(modes):
            c0 = tc * MONO_TILE
            w = min(MONO_TILE, MONO_W - c0)
            a[tr * MONO_TILE:(tr + 1) * MONO_TILE, c0:c0 + w] = _mono_tile(mode, dtype, MONO_TILE, w, rng)
    a.setflags(write=False)
    return Content(f"mono-{dtype}", "mono", dtype, a, MONO_TILE, MONO_TILE, 0, True)


@lru_cache(maxsize=None)
def stream(bands, dtype):
    """`bands` correlated smooth-plus-noise bands whose four frames favour, in turn, independent, left-side, right-side
    and mid-side coding of the first two"""
    rng = np.random.default_rng(7200 + bands)
    n = STREAM_H * STREAM_W
    t = np.arange(n)
    base = 800 * np.sin(t / 300.0) + 200 * np.sin(t / 37.0)
    L, R = base.copy(), base.copy()
    for f in range(n // FRAME):
        sl = slice(f * FRAME, (f + 1) * FRAME)
        if f % 4 == 0:
            R[sl] = 600 * np.sin(t[sl] / 11.0 + f) + rng.normal(0, 30, FRAME)
            L[sl] += rng.normal(0, 2, FRAME)
        elif f % 4 == 1:
            R[sl] = L[sl] + rng.normal(0, 40, FRAME)
        elif f % 4 == 2:
            L[sl] = R[sl] + rng.normal(0, 40, FRAME)
        else:
            e = rng.normal(0, 20, FRAME)
            L[sl] += e
            R[sl] -= e
    sig = [L, R, 0.5 * (L + R) + 300 * np.sin(t / 23.0) + rng.normal(0, 10, n)][:bands]
    scale, offset = {"uint8": (1 / 16.0, 2000.0), "uint16": (8.0, 2000.0), "int16": (1.0, 300.0)}[dtype]
    a = ((np.stack(sig).reshape(bands, STREAM_H, STREAM_W) + offset) * scale).astype(dtype)
    a.setflags(write=False)
    kind = "stereo" if bands == 2 else "multi"
    return Content(f"{kind}-{dtype}", kind, dtype, a, STREAM_H, STREAM_W, 0, True)


# values that normalise to -1 / +1 under spatial_encoder.py's map and lie inside the dtype's range where one exists
_RAW_MARKS = {"uint8": (0, 255), "int16": (-32767, -32767), "int32": (-2147483600, 2147483600),
              "float32": (-2.0, 1.5)}


@lru_cache(maxsize=None)
def raw(bands, dtype):
    rng = np.random.default_rng(7300 + bands)
    dt = np.dtype(dtype)
    shape = (bands, RAW_H, RAW_W)
    if dt.kind == "f":
        a = rng.uniform(-0.9, 0.9, shape).astype(dt)
    else:
        info = np.iinfo(dt)
        q = (int(info.max) - int(info.min)) // 8
        a = rng.integers(int(info.min) + q, int(info.max) - q, size=shape).astype(dt)       # -> 0
    lo, hi = _RAW_MARKS[dt.name]
    # the second tile (rows 64..): a sprinkle of +-1 in the first and the last band; a middle band stays all-zero
    for b in sorted({0, bands - 1}):
        m = rng.random((RAW_TILE, RAW_W)) < 0.02
        half = a[b, RAW_TILE:]
        half[m] = np.where(rng.random(int(m.sum())) < 0.5, lo, hi).astype(dt)
    a.setflags(write=False)
    return Content(f"raw{bands}-{dtype}", "raw", dtype, a if bands > 1 else a[0], RAW_TILE, RAW_TILE, 1, dt.name != "uint8")


@lru_cache(maxsize=None)
def s2row():
    rng = np.random.default_rng(7400)
    y, x = np.mgrid[0:S2_H, 0:S2_W]
    a = (2000 + 900 * np.sin(x / 210.0) + 500 * np.cos(y / 9.0) + 300 * np.sin((x + 3 * y) / 31.0)
         + rng.integers(0, 24, size=(S2_H, S2_W))).astype(np.uint16)
    a.setflags(write=False)
    return Content("s2row-uint16", "mono", "uint16", a, S2_TILE, S2_TILE, 0, True)


CONTENTS = {}
for _dt in ("uint8", "uint16", "int16"):
    CONTENTS[f"mono-{_dt}"] = (mono, (_dt,))
    CONTENTS[f"stereo-{_dt}"] = (stream, (2, _dt))
    CONTENTS[f"multi-{_dt}"] = (stream, (3, _dt))
for _dt in ("uint8", "int16", "int32", "float32"):
    for _b in (1, 3):
        CONTENTS[f"raw{_b}-{_dt}"] = (raw, (_b, _dt))
CONTENTS["s2row-uint16"] = (s2row, ())


def content(name):
    fn, args = CONTENTS[name]
    return fn(*args)


def bands_of(c):
    return c.data.shape[0] if c.data.ndim == 3 else 1


def tile_boxes(c):
    """(r0, c0, h, w) of every tile in row-major tile order (edge tiles truncated)"""
    H, W = c.data.shape[-2:]
    return [(r, x, min(c.tile_h, H - r), min(c.tile_w, W - x))
            for r in range(0, H, c.tile_h) for x in range(0, W, c.tile_w)]


# -------------------------------------------------------------------------------------------------------- layouts
def layouts(c):
    """The layout table of a content.  e: the narrowest misalignment the dtype allows (its element size; 4-byte
    elements cannot leave class 4, so their fourth residue is 12 and class 0 does not exist for them)."""
    es = np.dtype(c.dtype).itemsize
    e = es if es < 4 else 12
    multi = bands_of(c) > 1
    out = [Layout("aligned", 0, 0, 0)]
    out += [Layout(f"lead{v}", v, 0, 0) for v in (8, 4, e) if v != 12]          # (a lead of 12 is class 4 again)
    out += [Layout(f"row{v}", 0, v, 0) for v in (8, 4, e)]
    if multi:
        out += [Layout(f"band{v}", 0, 0, v) for v in (8, 4, e)]                  # only the band stride is misaligned
    # combinations whose minimum is 8, 4 and the narrowest class (16 is `aligned`)
    out += [Layout("all8", 8, 8, 8 if multi else 0), Layout("mix4", 4, 8, 4 if multi else 0),
            Layout("mixe", e if e != 12 else 4, 4, 8 if multi else 0)]
    return out


def _stride_for(least, es, res):
    """the smallest stride (elements) >= least whose byte length is `res` mod 16"""
    s = least
    while (s * es) % 16 != res:
        s += 1
    return s


def sentinels(dtype):
    dt = np.dtype(dtype)
    info = np.finfo(dt) if dt.kind == "f" else np.iinfo(dt)
    return dt.type(info.min), dt.type(info.max)


def place(c, lay):
    """The content in a parent buffer by layout `lay`: every element of the parent outside the view alternates between
    the dtype's minimum and maximum."""
    dt = np.dtype(c.dtype)
    es = dt.itemsize
    B = bands_of(c)
    H, W = c.data.shape[-2:]
    rs = _stride_for(W, es, lay.row_res)
    bs = _stride_for(rs * H, es, lay.band_res) if B > 1 else rs * H
    lead = lay.lead // es
    assert lead * es == lay.lead
    n = lead + (B - 1) * bs + (H - 1) * rs + W + 16 // es + 1
    lo, hi = sentinels(dt)
    parent = np.empty(n, dtype=dt)
    parent[0::2] = lo
    parent[1::2] = hi
    shape, strides = ((B, H, W), (bs * es, rs * es, es)) if B > 1 else ((H, W), (rs * es, es))
    view = np.lib.stride_tricks.as_strided(parent[lead:], shape=shape, strides=strides)
    view[...] = c.data
    return Placed(parent, view, lay.lead, rs, bs)


def view_mask(c, p):
    """True for the parent's elements that belong to the view"""
    m = np.zeros(p.parent.shape, dtype=bool)
    es = p.parent.dtype.itemsize
    shape, strides = (p.view.shape, tuple(s // es for s in p.view.strides))
    np.lib.stride_tricks.as_strided(m[p.lead // es:], shape=shape, strides=strides)[...] = True
    return m


def align_class(c, p, base=0):
    """encode_align_class of placement p with the parent at address `base`"""
    from flac_raster_amd._native import encode_align_class
    return encode_align_class(base + p.lead, p.parent.dtype.itemsize, p.row_stride, p.band_stride, c.tile_w, bands_of(c))


# ------------------------------------------------------------------------------------------------------ reference
Reference = namedtuple("Reference", "data off mins maxs bps")  # bytes, tile offsets, per-tile extremes, stream bps


@lru_cache(maxsize=None)
def reference(name):
    """The oracle's encode of the contiguous content: computed once, the same for every layout."""
    c = content(name)
    a = np.ascontiguousarray(c.data)
    B = bands_of(c)
    if c.kind == "mono":
        arena, off, mn, mx = O.encode_tiles(a, c.tile_h, RATE)
        return Reference(arena.tobytes(), [int(o) for o in off], list(mn), list(mx), 16)
    if c.kind in ("stereo", "multi"):
        pcm, mn, mx, bps = O.normalize(a.transpose(1, 2, 0).reshape(-1, B))
        data = O.encode_frames(pcm, bps, RATE)
        return Reference(data, [0, len(data)], [mn], [mx], bps)
    parts, mins, maxs = [], [], []
    a3 = a.reshape(B, *a.shape[-2:])
    for r0, c0, h, w in tile_boxes(c):
        sub = np.ascontiguousarray(a3[:, r0:r0 + h, c0:c0 + w])
        pcm = O.normalize_spatial(np.ascontiguousarray(sub.reshape(B, -1).T))
        parts.append(O.encode_frames(pcm, 32, RATE))
        mins.append(float(sub.min()))
        maxs.append(float(sub.max()))
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    return Reference(b"".join(parts), off, mins, maxs, 32)


def reference_pcm(name):
    """per tile: the oracle's PCM [samples, bands] of the contiguous content"""
    c = content(name)
    B = bands_of(c)
    a3 = np.ascontiguousarray(c.data).reshape(B, *c.data.shape[-2:])
    out = []
    for r0, c0, h, w in tile_boxes(c):
        sub = np.ascontiguousarray(a3[:, r0:r0 + h, c0:c0 + w].reshape(B, -1).T)
        out.append(O.normalize_spatial(sub) if c.kind == "raw" else O.normalize(sub)[0])
    return out
