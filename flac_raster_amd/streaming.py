"""Streaming FLAC format (create-streaming / extract-streaming) on the MI355X codec.

Reference: cli.py:620-804 (create_streaming) and cli.py:875-1039 (extract_streaming).
File layout: ``[u32 BE index_len][compact JSON index][tile FLAC 0]...[tile FLAC N-1]``; every tile is a
complete FLAC stream of band 1 (cli.py:699) with the mutagen-embedded geospatial tags of its temporary
GeoTIFF (converter.py:315-349).

Differences from the reference are only in *how*: all tiles are encoded in one GPU call (the reference
loops tiles serially through two temporary files each), and extraction decodes any number of tiles in
one batched GPU call.  ``extract_bbox_mosaic`` is an extension: the reference returns
only the first intersecting tile.

Overviews (extension, ``create_streaming*(overviews=True)``): reduced-resolution levels of band 1, each a 2x
reduction of the one before (frs_downsample2_device), tiled and encoded exactly as a raster of its own would be.
Their tiles follow level 0's in the file -- ``[u32 index length][index][level-0 tiles][level-1 tiles]...`` -- and
the index gains one key after ``frames``::

    "overviews": {"resampling": "average", "levels": [
        {"level": 1, "factor": 2, "width": w, "height": h, "transform": [...], "frames": [...]}, ...]}

Everything a reader without overview support looks at (the top-level keys, ``frames``) is what it is without them.
``level_index`` turns a level into a dict of the top-level index's shape, on which the selection and decode
functions work unchanged.

Nodata (extension, ``create_streaming*(nodata=V)``): the index gains a top-level ``"nodata": V`` key (NaN and +-inf as
the JSON strings ``"nan"``, ``"inf"``, ``"-inf"``), every tile's ``GEOSPATIAL_NODATA`` tag carries ``str(float(V))``,
the overview levels are built with the masked step (frs_downsample2_nodata_device; ``"nodata_aware": true`` in
``overviews``) and ``read_window`` resamples with the masked kernel, so that a nodata collar or hole is never averaged
into its neighbours.  Level 0's frames are what they are without nodata.  A file without the key reads exactly as
before.

Statistics (extension, ``create_streaming*(stats=True)``): the index gains a top-level ``"statistics"`` key with the
level-0 band's valid / nodata / NaN counts, min, max, mean, std and a histogram of at most 256 bins
(``stats.band_statistics``; non-finite numbers as the same JSON strings), masked by the nodata value in force.  The
frames and every other key are what they are without it; ``index_statistics`` reads the key back.

Bands (extension, ``create_streaming*(bands=...)``): every selected band of the source is stored as mono tiles of its
own, band after band -- ``[u32 index length][index][band 1: level-0 tiles, overview tiles][next band: level-0 tiles,
overview tiles]...`` -- frame ids and byte offsets running on through the file.  Band 1 must be among them: every key
above keeps its meaning and describes band 1, so a reader that knows nothing of bands sees a valid single-band file.
One key follows the others::

    "bands": {"count": <bands in the source>, "entries": [
        {"band": b, "frames": [...], "overviews": {...}, "statistics": {...}}, ...]}

with one entry per stored band other than 1, in file order; ``overviews`` and ``statistics`` are present exactly when
the top-level ones are, and one ``nodata`` value serves every band.  ``bands_of`` lists the stored bands and
``band_index`` turns one into a dict of the index's own shape; the readers take ``bands=`` and fetch the named bands'
tiles only.  Without ``bands`` the file written and the path taken are what they always were.
"""
from __future__ import annotations

import json
import logging
import math
import os
import struct
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import container, geotiff
from ._native import Context, default_context
from .converter import audio_params, write_tiff_from_meta

log = logging.getLogger("flac_raster.streaming")


# ----------------------------------------------------------------------------- encode
def tile_grid(height: int, width: int, tile: int) -> List[Tuple[int, int, int, int]]:
    """cli.py:691-696: row-major (col_off, row_off, w, h) windows, edge tiles truncated."""
    out = []
    for row in range(0, height, tile):
        for col in range(0, width, tile):
            out.append((col, row, min(tile, width - col), min(tile, height - row)))
    return out


def tile_transform_and_bbox(transform: geotiff.Affine, col: int, row: int, w: int, h: int):
    """cli.py:702-706 with rasterio's window_transform."""
    tt = geotiff.window_transform(transform, col, row)
    xmin = tt.c
    ymax = tt.f
    xmax = xmin + (w * tt.a)
    ymin = ymax + (h * tt.e)
    return tt, [xmin, ymin, xmax, ymax]


RESAMPLING = ("average", "nearest")


def overview_shapes(height: int, width: int, tile_size: int, max_levels: Optional[int] = None) -> List[Tuple[int, int]]:
    """(height, width) of overview levels 1, 2, ...: each level halves the one before with ceil, as long as the one
    before does not fit in one tile; the last level does.  At most `max_levels` levels.  Pure host code."""
    h, w, t = int(height), int(width), int(tile_size)
    if h < 1 or w < 1 or t < 1:
        raise ValueError("height, width and tile_size must be >= 1")
    if max_levels is not None and max_levels < 0:
        raise ValueError("max_levels must be >= 0")
    out: List[Tuple[int, int]] = []
    while max(h, w) > t and (max_levels is None or len(out) < max_levels):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def level_transform(transform: Sequence[float], level: int) -> List[float]:
    """The affine transform of overview level `level`: pixel sizes times 2**level, the origin unchanged (a level's
    pixel (0, 0) starts where level 0's does).  The products are exact (a power of two)."""
    a, b, c, d, e, f0 = (float(v) for v in list(transform)[:6])
    f = float(2 ** int(level))
    return [a * f, b * f, c, d * f, e * f, f0]


def nodata_for_dtype(nd, dtype):
    """The nodata value `nd` as a raster of `dtype` holds it: a Python int for the integer dtypes, a float (narrowed
    through float32 for float32) for the float dtypes.  ValueError when an integer dtype cannot hold it: a non-integer
    value, one outside the dtype's range, NaN or +-inf.  Pure."""
    dt = np.dtype(dtype)
    v = float(nd)
    if dt.kind == "f":
        with np.errstate(over="ignore"):
            return float(dt.type(v))
    if dt.kind not in "iu":
        raise ValueError(f"nodata: {dt} is not a raster dtype")
    ii = np.iinfo(dt)
    if not math.isfinite(v) or v != math.floor(v) or not (ii.min <= v <= ii.max):
        raise ValueError(f"nodata {nd!r} is not an integer inside the range of {dt} [{ii.min}, {ii.max}]")
    return int(v)


def _nodata_to_index(v):
    """The index's "nodata" value: the number, or "nan" / "inf" / "-inf" (JSON has no such numbers)."""
    return v if math.isfinite(v) else str(float(v))


def index_nodata(index: Dict) -> Optional[float]:
    """The nodata value a streaming index carries (its "nodata" key), or None."""
    v = index.get("nodata")
    return None if v is None else float(v)


def index_statistics(index: Dict) -> Optional[Dict]:
    """The statistics of the level-0 band a streaming index carries (its "statistics" key, written by
    create_streaming*(stats=True)), as stats.band_statistics returns a band's, or None."""
    from .stats import statistics_from_index
    return statistics_from_index(index.get("statistics"))


def overview_levels(index: Dict) -> List[int]:
    """The levels a streaming index holds: 0 and its overview levels."""
    ov = index.get("overviews") or {}
    return [0] + [int(lv["level"]) for lv in ov.get("levels", [])]


def level_index(index: Dict, level: int = 0) -> Dict:
    """A dict of the streaming index's own shape (crs, transform, width, height, tile_size, frames) for one level;
    level 0 is the index itself.  select_frame, intersecting, first_intersecting, tile_windows and decode_into_window
    work on the result unchanged.  An index with a "nodata" key passes it on to every level.  LookupError (naming the
    levels present) for a level the file does not hold."""
    if int(level) == 0:
        return index
    for lv in (index.get("overviews") or {}).get("levels", []):
        if int(lv["level"]) == int(level):
            li = {"crs": index.get("crs"), "transform": list(lv["transform"]), "width": lv["width"],
                  "height": lv["height"], "tile_size": index.get("tile_size"), "frames": lv["frames"]}
            if "nodata" in index:
                li["nodata"] = index["nodata"]
            return li
    raise LookupError(f"level {level} not in this file (levels present: {overview_levels(index)})")


def bands_of(index: Dict) -> List[int]:
    """The band numbers (1-based, the source's) a streaming index holds, in file order: [1] for a file without a
    "bands" key.  Pure."""
    return [1] + [int(e["band"]) for e in (index.get("bands") or {}).get("entries", [])]


def band_index(index: Dict, band: int = 1) -> Dict:
    """A dict of the streaming index's own shape (crs, transform, width, height, tile_size, frames, and nodata /
    overviews / statistics where the file has them) for one stored band; band 1 is the index without its "bands" key.
    level_index, window_request, select_frame, intersecting, pick_level and index_statistics work on the result
    unchanged.  LookupError (naming the bands present) for a band the file does not hold.  Pure."""
    band = int(band)
    if band == 1:
        return {k: v for k, v in index.items() if k != "bands"} if "bands" in index else index
    for e in (index.get("bands") or {}).get("entries", []):
        if int(e["band"]) == band:
            bi = {"crs": index.get("crs"), "transform": list(index["transform"]), "width": index["width"],
                  "height": index["height"], "tile_size": index.get("tile_size"), "frames": e["frames"]}
            if "nodata" in index:
                bi["nodata"] = index["nodata"]
            for key in ("overviews", "statistics"):
                if key in e:
                    bi[key] = e[key]
            return bi
    raise LookupError(f"band {band} not in this file (bands present: {bands_of(index)})")


def parse_bands(text: str):
    """A --bands value: "all", or 1-based band numbers separated by commas ("1,2,3") as a list.  ValueError for
    anything else, a number below 1 and a number given twice.  Pure."""
    t = str(text).strip().lower()
    if t == "all":
        return "all"
    parts = [p.strip() for p in t.split(",")]
    if not parts or not all(p.isascii() and p.isdigit() for p in parts):
        raise ValueError(f"--bands must be 'all' or band numbers separated by commas, got {text!r}")
    nums = [int(p) for p in parts]
    if min(nums) < 1:
        raise ValueError(f"--bands: band numbers start at 1, got {text!r}")
    if len(set(nums)) != len(nums):
        raise ValueError(f"--bands: a band is named twice in {text!r}")
    return nums


def select_bands(bands, count: int) -> List[int]:
    """The bands create_streaming*(bands=...) stores of a source with `count` bands: "all" is 1 .. count, a sequence is
    checked (whole numbers 1 .. count, none twice) and must name band 1, whose frames the top-level keys of the index
    describe.  ValueError otherwise.  Pure."""
    count = int(count)
    if isinstance(bands, str):
        bands = parse_bands(bands)
        if bands == "all":
            return list(range(1, count + 1))
    nums = [int(b) for b in bands]
    if [float(b) for b in bands] != [float(b) for b in nums] or not nums:
        raise ValueError(f"bands must be whole band numbers, got {list(bands)!r}")
    if len(set(nums)) != len(nums):
        raise ValueError(f"a band is named twice in {nums}")
    bad = [b for b in nums if not 1 <= b <= count]
    if bad:
        raise ValueError(f"band {bad[0]} is not one of the source's {count} band(s)")
    if 1 not in nums:
        raise ValueError(f"band 1 must be among the stored bands (the index's top-level keys are band 1's), got {nums}")
    return nums


def _bands_to_read(index: Dict, bands) -> List[int]:
    """The bands a read returns: [1] for None, every stored band for "all", else the named bands, each of which the
    file must hold (LookupError) and none of which may be named twice."""
    if bands is None:
        return [1]
    if isinstance(bands, str):
        bands = parse_bands(bands)
        if bands == "all":
            return bands_of(index)
    nums = [int(b) for b in bands]
    if not nums or len(set(nums)) != len(nums):
        raise ValueError(f"bands must name at least one band and none twice, got {nums}")
    for b in nums:
        band_index(index, b)
    return nums


def pick_level(index: Dict, width_px: int, height_px: int, max_size: int) -> int:
    """The finest level at which a window of width_px x height_px level-0 pixels is at most `max_size` pixels on its
    longer side (a level-k window has ceil(n / 2**k) pixels); the coarsest level when none qualifies.  Pure."""
    if max_size < 1:
        raise ValueError("max_size must be >= 1")
    levels = sorted(overview_levels(index))
    longer = max(int(width_px), int(height_px))
    for k in levels:
        if -(-longer // (1 << k)) <= max_size:
            return k
    return levels[-1]


def tile_tags(crs: Optional[str], tt: geotiff.Affine, w: int, h: int, dtype, tmin: float, tmax: float,
              nodata: Optional[float] = None):
    """Tags of the per-tile FLAC (tiff_to_flac on the temporary 1-band GeoTIFF, cli.py:719-733)."""
    bounds = geotiff.GeoRaster(np.empty((1, h, w), dtype=np.uint8), tt).bounds
    md = {
        "width": w, "height": h, "count": 1, "dtype": str(np.dtype(dtype)), "crs": crs,
        "transform": list(tt),
        "bounds": {"left": bounds[0], "bottom": bounds[1], "right": bounds[2], "top": bounds[3]},
        "data_min": tmin, "data_max": tmax, "nodata": None if nodata is None else float(nodata), "driver": "GTiff",
    }
    return container.raster_tags(md)


class TileHeaderBuilder:
    """Per-tile FLAC headers of a streaming file, byte-identical to ``container.mutagen_header(..., tile_tags(...))``
    (the mutagen rewrite of each temporary tile FLAC, converter.py:315-349) at a few microseconds per tile: the
    constant tag entries are encoded once and the per-tile numbers (a C4 file has 6241 tiles but only 79 column
    and 79 row origins) are formatted through a cache.  Checked against the direct path in tests."""

    _PREFIX = (("TITLE", "Geospatial Raster Data"),
               ("DESCRIPTION", "TIFF raster converted to FLAC with geospatial metadata"),
               ("ENCODER", "FLAC-Raster v0.1.0"))

    def __init__(self, crs: Optional[str], dtype, stream_bps: int, sample_rate: int = 44100, blocksize: int = 4096,
                 nodata: Optional[float] = None):
        self._si = container.block(container.BLOCK_STREAMINFO,
                                   container.streaminfo(blocksize, sample_rate, 1, stream_bps), False)
        self._vendor = struct.pack("<I", len(container.VENDOR)) + container.VENDOR + struct.pack("<I", 14)
        ent = self._entry
        self._pre = b"".join(ent(k, v) for k, v in self._PREFIX) + ent("GEOSPATIAL_CRS", str(crs))
        self._mid = (ent("GEOSPATIAL_COUNT", "1") + ent("GEOSPATIAL_DTYPE", str(np.dtype(dtype))) +
                     ent("GEOSPATIAL_NODATA", "None" if nodata is None else str(float(nodata))))
        self._tail = ent("GEOSPATIAL_SPATIAL_TILING", "False")
        self._num: Dict[Tuple[type, object, bool], str] = {}
        self._ent: Dict[Tuple[str, str], bytes] = {}

    @staticmethod
    def _entry(k: str, v: str) -> bytes:
        c = k.encode("ascii") + b"=" + v.encode("utf-8")
        return struct.pack("<I", len(c)) + c

    def _js(self, x) -> str:
        """json.dumps of a number (float.__repr__ for finite floats), cached; -0.0 and 0.0 kept apart."""
        key = (type(x), x, math.copysign(1.0, x) < 0 if isinstance(x, float) else False)
        v = self._num.get(key)
        if v is None:
            v = self._num[key] = json.dumps(x)
        return v

    def _cached_entry(self, k: str, v: str) -> bytes:
        e = self._ent.get((k, v))
        if e is None:
            e = self._ent[(k, v)] = self._entry(k, v)
        return e

    def header(self, tt: geotiff.Affine, w: int, h: int, tmin: float, tmax: float, frame_bytes: int) -> bytes:
        js = self._js
        left, bottom, right, top = geotiff.bounds_of(tt, w, h)
        tr = "[" + ", ".join(js(v) for v in tt) + "]"
        bd = '{"left": ' + js(left) + ', "bottom": ' + js(bottom) + ', "right": ' + js(right) + ', "top": ' + \
             js(top) + "}"
        ent = self._entry
        body = b"".join((self._vendor, self._pre, self._cached_entry("GEOSPATIAL_WIDTH", str(w)),
                         self._cached_entry("GEOSPATIAL_HEIGHT", str(h)), self._mid,
                         self._cached_entry("GEOSPATIAL_DATA_MIN", str(tmin)),
                         self._cached_entry("GEOSPATIAL_DATA_MAX", str(tmax)),
                         ent("GEOSPATIAL_TRANSFORM", tr), ent("GEOSPATIAL_BOUNDS", bd), self._tail))
        vc = container.block(container.BLOCK_VORBIS_COMMENT, body, False)
        pad = container.mutagen_padding(86 - 4, len(self._si) + len(vc) + 4, frame_bytes)
        return b"".join((b"fLaC", self._si, vc, container.block(container.BLOCK_PADDING, bytes(pad), True)))


@dataclass
class EncodedTiles:
    """Output of one GPU encode of all band-1 tiles."""
    windows: List[Tuple[int, int, int, int]]
    frames: np.ndarray          # arena: all tiles' frames back to back
    tile_off: np.ndarray        # int64[n+1]
    tile_min: np.ndarray
    tile_max: np.ndarray
    stream_bps: int


def encode_band_tiles(band: np.ndarray, tile_size: int, ctx: Optional[Context] = None,
                      pinned: bool = False) -> EncodedTiles:
    """All band-1 tiles in one GPU launch sequence (the reference's tile loop, cli.py:690-763).  pinned=True: the
    frames land in page-locked memory owned by the returned arena array (Context.pinned: the DMA writes at full
    rate, and the buffer lives as long as any view of it)."""
    H, W = band.shape
    if H == 0 or W == 0:  # an empty shard (more ranks than tile rows): no tiles, nothing to launch
        z = np.zeros(0, dtype=np.float64)
        _, bps = audio_params(1, 1, band.dtype)
        return EncodedTiles([], np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), z, z,
                            16 if bps == 16 else 32)
    ctx = ctx or default_context()
    _, bps = audio_params(1, min(tile_size, H), band.dtype)
    d = ctx.make_desc(H, W, band.dtype, nbands=1, tile_h=tile_size, tile_w=tile_size, sample_rate=44100,
                      bits_per_sample=bps)
    arena, off, mn, mx, sbps = ctx.encode_tiles_host(np.ascontiguousarray(band), d, pinned=pinned)
    return EncodedTiles(tile_grid(H, W, tile_size), arena, off, mn, mx, sbps)


def streaming_headers(enc: EncodedTiles, transform: geotiff.Affine, crs: Optional[str], width: int, height: int,
                      tile_size: int, dtype, windows=None, frame_id0: int = 0, byte_offset0: int = 0,
                      nodata: Optional[float] = None):
    """Per-tile headers and index entries of `enc`'s tiles (cli.py:702-759): (headers, frames entries, bytes).
    `nodata` goes into every tile's GEOSPATIAL_NODATA tag."""
    windows = enc.windows if windows is None else windows
    hb = TileHeaderBuilder(crs, dtype, enc.stream_bps, nodata=nodata)
    headers: List[bytes] = []
    frames: List[Dict] = []
    total = byte_offset0
    tile_bytes = np.diff(enc.tile_off)
    for i, (col, row, w, h) in enumerate(windows):
        tt = geotiff.window_transform(transform, col, row)
        # sample rate of the tile: _calculate_audio_params on the (1, h, w) array -> shape0*shape1 = h
        if h >= 1000000:
            raise NotImplementedError("tile heights >= 1e6 rows change the sample rate; re-encode needed")
        fb = int(tile_bytes[i])
        hdr = hb.header(tt, w, h, float(enc.tile_min[i]), float(enc.tile_max[i]), fb)
        xmin, ymax = tt.c, tt.f
        frames.append({"frame_id": frame_id0 + i, "bbox": [xmin, ymax + (h * tt.e), xmin + (w * tt.a), ymax],
                       "window": {"col_off": col, "row_off": row, "width": w, "height": h},
                       "byte_offset": total, "byte_size": len(hdr) + fb})
        headers.append(hdr)
        total += len(hdr) + fb
    return headers, frames, total - byte_offset0


def streaming_head(index: Dict) -> bytes:
    """[u32 BE index length][compact JSON index] (cli.py:769-773)."""
    js = container.index_json(index)
    return struct.pack(">I", len(js)) + js


def assemble_streaming(enc: EncodedTiles, transform: geotiff.Affine, crs: Optional[str], width: int, height: int,
                       tile_size: int, dtype) -> Tuple[bytes, List[bytes], Dict]:
    """Index JSON + per-tile FLAC streams (header bytes + frames) -> (head, tile_streams, index)."""
    headers, frames, _ = streaming_headers(enc, transform, crs, width, height, tile_size, dtype)
    index = {"crs": str(crs), "transform": list(transform), "width": width, "height": height,
             "tile_size": tile_size, "frames": frames}
    streams = [hdr + enc.frames[enc.tile_off[i]:enc.tile_off[i + 1]].tobytes() for i, hdr in enumerate(headers)]
    return streaming_head(index), streams, index


def write_tiles(fd: int, offset: int, headers: Sequence[bytes], enc: EncodedTiles, threads: int = 8) -> None:
    """pwritev of (header, frames) pairs straight from the arena (no per-tile copies), tile ranges in parallel
    threads (os.pwritev releases the GIL); the tiles land back to back from file offset `offset`."""
    from concurrent.futures import ThreadPoolExecutor
    n = len(headers)
    if n == 0:
        return
    mv = memoryview(enc.frames)
    sizes = np.array([len(h) for h in headers], dtype=np.int64) + np.diff(enc.tile_off)
    starts = offset + np.concatenate(([0], np.cumsum(sizes)[:-1]))
    off = enc.tile_off

    def run(a: int, b: int):
        i = a
        while i < b:
            j = min(b, i + 512)  # 1024 iovecs per call (IOV_MAX)
            iov = []
            for k in range(i, j):
                iov.append(headers[k])
                iov.append(mv[off[k]:off[k + 1]])
            want = int(starts[j - 1] + sizes[j - 1] - starts[i])
            done = os.pwritev(fd, iov, int(starts[i]))
            if done != want:  # short write: finish byte-wise
                buf = b"".join(bytes(x) for x in iov)
                while done < want:
                    done += os.pwrite(fd, buf[done:], int(starts[i]) + done)
            i = j

    k = max(1, min(threads, n // 64 or 1))
    bounds = [n * t // k for t in range(k + 1)]
    with ThreadPoolExecutor(k) as ex:
        list(ex.map(lambda t: run(bounds[t], bounds[t + 1]), range(k)))


def encode_band_tiles_device(ctx: Context, raster_ptr: int, height: int, width: int, dtype, tile_size: int,
                             arena, pinned: bool = False) -> EncodedTiles:
    """encode_band_tiles for a dense band already in device memory: frs_encode_tiles_device into the device arena
    `arena` (at least the descriptor's arena bound), the frames brought back to the host."""
    _, bps = audio_params(1, min(tile_size, height), dtype)
    d = ctx.make_desc(height, width, dtype, nbands=1, tile_h=tile_size, tile_w=tile_size, sample_rate=44100,
                      bits_per_sample=bps)
    off, mn, mx, sbps = ctx.encode_tiles_device(raster_ptr, d, arena)
    n = int(off[-1])
    frames = ctx.pinned(n) if pinned and n else np.empty(n, dtype=np.uint8)
    if n:
        arena.download(n, 0, out=frames)
    return EncodedTiles(tile_grid(height, width, tile_size), frames, off, mn, mx, sbps)


def _create_streaming_overviews(band: np.ndarray, transform: geotiff.Affine, crs: Optional[str], output: Path,
                                tile_size: int, ctx: Optional[Context], tm: Dict[str, float], resampling: str,
                                max_levels: Optional[int], nodata=None, stats: bool = False) -> Dict:
    """create_streaming_array(overviews=True): the band goes up once; level k is made from level k - 1 on the device
    (frs_downsample2_device) and encoded there like a raster of its own.  Device memory held at any time: the band,
    two level buffers and one arena (sized for level 0, the largest).  With `nodata` (already in the dtype's terms) the
    step is the masked one.  With `stats` the uploaded band's statistics go into the index."""
    if resampling not in RESAMPLING:
        raise ValueError(f"resampling must be one of {RESAMPLING}, got {resampling!r}")
    ctx = ctx or default_context()
    t0 = time.perf_counter()
    H, W = band.shape
    dtype = band.dtype
    shapes = [(H, W)] + overview_shapes(H, W, tile_size, max_levels)
    _, bps0 = audio_params(1, min(tile_size, H), dtype)
    d0 = ctx.make_desc(H, W, dtype, nbands=1, tile_h=tile_size, tile_w=tile_size, sample_rate=44100,
                       bits_per_sample=bps0)
    bufs = [ctx.alloc(band.nbytes)]
    pyr_s = 0.0
    encs: List[EncodedTiles] = []
    band_stats = None
    try:
        bufs[0].upload(band)
        if stats:
            band_stats = _band_statistics_device(ctx, bufs[0].ptr, H, W, dtype, nodata)
        arena = ctx.alloc(ctx.arena_bound(d0))
        bufs.append(arena)
        # level k lives in lv[k % 2] (level 1 and 2 get a buffer each, level k + 2 fits in level k's)
        lv = [ctx.alloc(h * w * dtype.itemsize) for h, w in shapes[1:3]]
        bufs.extend(lv)
        cur, cur_desc = bufs[0], ctx.make_raster_desc(H, W, dtype)
        for k, (h, w) in enumerate(shapes):
            if k:
                tp = time.perf_counter()
                nxt = lv[(k - 1) % 2]
                cur_desc = ctx.downsample2_device(cur.ptr, cur_desc, nxt.ptr, mode=resampling, nodata=nodata)
                cur = nxt
                pyr_s += time.perf_counter() - tp
            # level 0 of a large job: frames back into page-locked memory, as without overviews
            encs.append(encode_band_tiles_device(ctx, cur.ptr, h, w, dtype, tile_size, arena,
                                                 pinned=k == 0 and band.nbytes >= (64 << 20)))
    finally:
        for b in bufs:
            b.close()
    t1 = time.perf_counter()
    tr6 = list(transform)[:6]
    parts = []  # (headers, enc) per level, in file order
    levels = []
    fid, total = 0, 0
    frames0: List[Dict] = []
    for k, ((h, w), enc) in enumerate(zip(shapes, encs)):
        lt = level_transform(tr6, k)
        tk = geotiff.Affine(*lt) if k else transform
        headers, frames, nbytes = streaming_headers(enc, tk, crs, w, h, tile_size, dtype, frame_id0=fid,
                                                    byte_offset0=total, nodata=nodata)
        parts.append((headers, enc, total))
        fid += len(frames)
        total += nbytes
        if k == 0:
            frames0 = frames
        else:
            levels.append({"level": k, "factor": 2 ** k, "width": w, "height": h, "transform": lt,
                           "frames": frames})
    index = {"crs": str(crs), "transform": list(transform), "width": W, "height": H, "tile_size": tile_size,
             "frames": frames0}
    if nodata is not None:
        index["nodata"] = _nodata_to_index(nodata)
    index["overviews"] = {"resampling": resampling, "levels": levels}
    if nodata is not None:
        index["overviews"]["nodata_aware"] = True
    if band_stats is not None:
        index["statistics"] = band_stats
    head = streaming_head(index)
    t2 = time.perf_counter()
    fd = os.open(output, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        os.ftruncate(fd, len(head) + total)
        t2b = time.perf_counter()
        os.pwrite(fd, head, 0)
        for headers, enc, start in parts:
            write_tiles(fd, len(head) + start, headers, enc)
    finally:
        os.close(fd)
    t3 = time.perf_counter()
    tm.update(encode_s=t1 - t0, pyramid_s=pyr_s, index_s=t2 - t1, write_s=t3 - t2, open_truncate_s=t2b - t2,
              total_s=t3 - t0)
    return index


STATS_INDEX_BINS = 256  # bins of the histogram create_streaming*(stats=True) stores at most


def _band_statistics_device(ctx: Context, ptr: int, height: int, width: int, dtype, nodata) -> Dict:
    """The index's "statistics" value of the dense band at device pointer `ptr`."""
    from .stats import _device_statistics, statistics_to_index
    d = ctx.make_raster_desc(height, width, dtype)
    return statistics_to_index(_device_statistics(ctx, ptr, d, nodata, STATS_INDEX_BINS)[0])


def _encode_band_tiles_with_statistics(band: np.ndarray, tile_size: int, ctx: Context, nodata):
    """create_streaming_array(stats=True) without overviews: the band goes up once, is encoded there
    (encode_band_tiles_device: the frames encode_band_tiles gives) and its statistics are taken from the same
    buffer.  Returns (EncodedTiles, the index's "statistics" value)."""
    H, W = band.shape
    if H == 0 or W == 0:
        raise ValueError("statistics of an empty band")
    _, bps = audio_params(1, min(tile_size, H), band.dtype)
    d = ctx.make_desc(H, W, band.dtype, nbands=1, tile_h=tile_size, tile_w=tile_size, sample_rate=44100,
                      bits_per_sample=bps)
    bufs = [ctx.alloc(band.nbytes)]
    try:
        bufs[0].upload(band)
        bufs.append(ctx.alloc(ctx.arena_bound(d)))
        enc = encode_band_tiles_device(ctx, bufs[0].ptr, H, W, band.dtype, tile_size, bufs[1],
                                       pinned=band.nbytes >= (64 << 20))
        return enc, _band_statistics_device(ctx, bufs[0].ptr, H, W, band.dtype, nodata)
    finally:
        for b in bufs:
            b.close()


def create_streaming_array(band: np.ndarray, transform: geotiff.Affine, crs: Optional[str], output: Path,
                           tile_size: int = 1024, ctx: Optional[Context] = None,
                           timings: Optional[Dict[str, float]] = None, overviews: bool = False,
                           resampling: str = "average", max_levels: Optional[int] = None, nodata=None,
                           stats: bool = False) -> Dict:
    """cli.py:620-804 on an in-memory band-1 array: one GPU encode of every tile, headers and index on the host,
    tiles written from the arena with parallel pwritev.  Returns the index; `timings` gets the stage seconds.
    overviews=True (extension) appends reduced-resolution levels (module docstring): `resampling` is "average" or
    "nearest", `max_levels` caps their number; `timings` then also gets pyramid_s (inside encode_s).  `nodata`
    (extension, a number the band's dtype holds: nodata_for_dtype) marks pixels without data (module docstring).
    stats=True (extension) puts the band's statistics (stats.band_statistics: counts, min, max, mean, std and a
    histogram of at most 256 bins, masked by the nodata value in force) into the index under "statistics"; the band
    then goes up once for the encode and the statistics together.  Without it the file and the path taken are what
    they are without the option."""
    tm = timings if timings is not None else {}
    if nodata is not None:
        nodata = nodata_for_dtype(nodata, band.dtype)
    if overviews:
        return _create_streaming_overviews(band, transform, crs, output, tile_size, ctx, tm, resampling, max_levels,
                                           nodata, stats)
    t0 = time.perf_counter()
    H, W = band.shape
    band_stats = None
    if stats:
        enc, band_stats = _encode_band_tiles_with_statistics(band, tile_size, ctx or default_context(), nodata)
    else:
        # large jobs: frames back into page-locked memory (DMA rate, no page faults) and written from there
        enc = encode_band_tiles(band, tile_size, ctx, pinned=band.nbytes >= (64 << 20))
    t1 = time.perf_counter()
    headers, frames, body = streaming_headers(enc, transform, crs, W, H, tile_size, band.dtype, nodata=nodata)
    index = {"crs": str(crs), "transform": list(transform), "width": W, "height": H, "tile_size": tile_size,
             "frames": frames}
    if nodata is not None:
        index["nodata"] = _nodata_to_index(nodata)
    if band_stats is not None:
        index["statistics"] = band_stats
    head = streaming_head(index)
    t2 = time.perf_counter()
    fd = os.open(output, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        os.ftruncate(fd, len(head) + body)
        t2b = time.perf_counter()  # (truncating an existing file frees its pages: part of the write cost)
        os.pwrite(fd, head, 0)
        write_tiles(fd, len(head), headers, enc)
    finally:
        os.close(fd)
    t3 = time.perf_counter()
    tm.update(encode_s=t1 - t0, index_s=t2 - t1, write_s=t3 - t2, open_truncate_s=t2b - t2, total_s=t3 - t0)
    return index


def create_streaming_bands_array(bands, band_numbers: Sequence[int], transform: geotiff.Affine, crs: Optional[str],
                                 output: Path, tile_size: int = 1024, ctx: Optional[Context] = None,
                                 timings: Optional[Dict[str, float]] = None, overviews: bool = False,
                                 resampling: str = "average", max_levels: Optional[int] = None, nodata=None,
                                 stats: bool = False, source_count: Optional[int] = None) -> Dict:
    """Extension: a streaming file of several bands (module docstring, "Bands").  `bands` is an (N, H, W) array or a
    sequence of N (H, W) arrays of one shape and dtype; band_numbers[k] is the 1-based number plane k has in its
    source, and band 1 must be among them (select_bands).  `source_count` (the "count" the index records) defaults to
    the largest number.  Every band is encoded as mono tiles by the path create_streaming_array takes for band 1 on the
    device (encode_band_tiles_device), gets overview levels of its own with `overviews` and statistics of its own with
    `stats`; one `nodata` value serves them all.  The bands go through the device one after the other: the band buffer,
    the two level buffers and the arena are allocated once, for one band.  Band 1's tiles come first, then the other
    bands' in the order given.  Returns the index; `timings` gets the stage seconds."""
    tm = timings if timings is not None else {}
    planes = [np.asarray(b) for b in bands]
    count = int(source_count) if source_count is not None else max(int(b) for b in band_numbers)
    nums = select_bands(list(band_numbers), count)
    if len(planes) != len(nums):
        raise ValueError("one band number per plane")
    H, W = planes[0].shape if planes[0].ndim == 2 else (0, 0)
    dtype = planes[0].dtype
    if H == 0 or W == 0 or any(p.shape != (H, W) or p.dtype != dtype for p in planes):
        raise ValueError("the bands must be non-empty (H, W) arrays of one shape and dtype")
    if overviews and resampling not in RESAMPLING:
        raise ValueError(f"resampling must be one of {RESAMPLING}, got {resampling!r}")
    if nodata is not None:
        nodata = nodata_for_dtype(nodata, dtype)
    ctx = ctx or default_context()
    t0 = time.perf_counter()
    shapes = [(H, W)] + (overview_shapes(H, W, tile_size, max_levels) if overviews else [])
    _, bps0 = audio_params(1, min(tile_size, H), dtype)
    d0 = ctx.make_desc(H, W, dtype, nbands=1, tile_h=tile_size, tile_w=tile_size, sample_rate=44100,
                       bits_per_sample=bps0)
    order = [nums.index(1)] + [k for k, b in enumerate(nums) if b != 1]
    bufs: List = []
    pyr_s = 0.0
    encoded = []  # (band number, EncodedTiles per level, statistics or None), in file order
    try:
        bufs.append(ctx.alloc(H * W * dtype.itemsize))
        bufs.append(ctx.alloc(ctx.arena_bound(d0)))
        band_buf, arena = bufs
        # level k lives in lv[k % 2], as in _create_streaming_overviews
        lv = [ctx.alloc(h * w * dtype.itemsize) for h, w in shapes[1:3]]
        bufs.extend(lv)
        for k in order:
            band_buf.upload(planes[k])
            band_stats = _band_statistics_device(ctx, band_buf.ptr, H, W, dtype, nodata) if stats else None
            cur, cur_desc = band_buf, ctx.make_raster_desc(H, W, dtype)
            encs: List[EncodedTiles] = []
            for level, (h, w) in enumerate(shapes):
                if level:
                    tp = time.perf_counter()
                    nxt = lv[(level - 1) % 2]
                    cur_desc = ctx.downsample2_device(cur.ptr, cur_desc, nxt.ptr, mode=resampling, nodata=nodata)
                    cur = nxt
                    pyr_s += time.perf_counter() - tp
                encs.append(encode_band_tiles_device(ctx, cur.ptr, h, w, dtype, tile_size, arena,
                                                     pinned=level == 0 and planes[k].nbytes >= (64 << 20)))
            encoded.append((nums[k], encs, band_stats))
    finally:
        for b in bufs:
            b.close()
    t1 = time.perf_counter()
    tr6 = list(transform)[:6]
    parts = []  # (headers, enc, body offset) per band and level, in file order
    fid, total = 0, 0
    index: Dict = {}
    entries: List[Dict] = []
    for num, encs, band_stats in encoded:
        frames0: List[Dict] = []
        levels = []
        for level, ((h, w), enc) in enumerate(zip(shapes, encs)):
            lt = level_transform(tr6, level)
            headers, frames, nbytes = streaming_headers(enc, geotiff.Affine(*lt) if level else transform, crs, w, h,
                                                        tile_size, dtype, frame_id0=fid, byte_offset0=total,
                                                        nodata=nodata)
            parts.append((headers, enc, total))
            fid += len(frames)
            total += nbytes
            if level == 0:
                frames0 = frames
            else:
                levels.append({"level": level, "factor": 2 ** level, "width": w, "height": h, "transform": lt,
                               "frames": frames})
        if num == 1:  # the keys a single-band file has, in its order
            entry = index
            index.update({"crs": str(crs), "transform": list(transform), "width": W, "height": H,
                          "tile_size": tile_size, "frames": frames0})
            if nodata is not None:
                index["nodata"] = _nodata_to_index(nodata)
        else:
            entry = {"band": num, "frames": frames0}
            entries.append(entry)
        if overviews:
            entry["overviews"] = {"resampling": resampling, "levels": levels}
            if nodata is not None:
                entry["overviews"]["nodata_aware"] = True
        if band_stats is not None:
            entry["statistics"] = band_stats
    index["bands"] = {"count": count, "entries": entries}
    head = streaming_head(index)
    t2 = time.perf_counter()
    fd = os.open(output, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        os.ftruncate(fd, len(head) + total)
        t2b = time.perf_counter()
        os.pwrite(fd, head, 0)
        for headers, enc, start in parts:
            write_tiles(fd, len(head) + start, headers, enc)
    finally:
        os.close(fd)
    t3 = time.perf_counter()
    tm.update(encode_s=t1 - t0, pyramid_s=pyr_s, index_s=t2 - t1, write_s=t3 - t2, open_truncate_s=t2b - t2,
              total_s=t3 - t0)
    return index


def create_streaming(input_file: Path, output_file: Path, tile_size: int = 1024,
                     ctx: Optional[Context] = None, timings: Optional[Dict[str, float]] = None,
                     materialize: bool = False, overviews: bool = False, resampling: str = "average",
                     max_levels: Optional[int] = None, nodata=None, stats: bool = False, bands=None) -> Dict:
    """cli.py:620-804 without the console output: writes the streaming file, returns the index.  Band 1 only
    (cli.py:698-699): an uncompressed band-sequential (or single-band) file is encoded straight from its memory map
    (no host copy of the band); otherwise its strips / tiles are decoded.  `timings` gets read_s + the stages of
    create_streaming_array.  materialize=True reads the band into host memory first (read_s is then the whole read;
    otherwise the band's pages are read while the encode copies them, inside encode_s).  overviews / resampling /
    max_levels / nodata / stats: as create_streaming_array; nodata="source" takes the GeoTIFF's GDAL_NODATA tag (ValueError
    when the file has none).  `bands` (extension): "all" or 1-based band numbers, band 1 among them (select_bands):
    those bands are stored one after the other (create_streaming_bands_array); without it the file and the path taken
    are what they always were."""
    tm = timings if timings is not None else {}
    t0 = time.perf_counter()
    with geotiff.TiffFile(input_file) as tf:
        transform, epsg, src_nodata, _ = tf.georef()
        if isinstance(nodata, str):
            if nodata != "source":
                raise ValueError(f"nodata must be a number or 'source', got {nodata!r}")
            if src_nodata is None:
                raise ValueError(f"{input_file} has no GDAL_NODATA tag")
            nodata = src_nodata
        crs = f"EPSG:{epsg}" if epsg else None
        if bands is not None:
            nums = select_bands(bands, tf.count)
            planes = [None if materialize else tf.band_view(b - 1) for b in nums]
            planes = [tf.read_rows(bands=[b - 1])[0] if p is None else p for b, p in zip(nums, planes)]
            tm["read_s"] = time.perf_counter() - t0
            transform = transform or geotiff.Affine(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
            index = create_streaming_bands_array(planes, nums, transform, crs, output_file, tile_size, ctx, tm,
                                                 overviews=overviews, resampling=resampling, max_levels=max_levels,
                                                 nodata=nodata, stats=stats, source_count=tf.count)
            del planes
            tm["total_s"] = time.perf_counter() - t0
            return index
        band = None if materialize else tf.band_view(0)
        if band is None:
            band = tf.read_rows(bands=[0])[0]
        tm["read_s"] = time.perf_counter() - t0
        transform = transform or geotiff.Affine(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        index = create_streaming_array(band, transform, crs, output_file, tile_size, ctx, tm, overviews=overviews,
                                       resampling=resampling, max_levels=max_levels, nodata=nodata, stats=stats)
        del band
    tm["total_s"] = time.perf_counter() - t0
    return index


# ----------------------------------------------------------------------------- read / select
class Source:
    """Local file or HTTP(S) URL with byte-range reads (cli.py:898-919, 1001-1011)."""

    def __init__(self, path_or_url: Union[str, Path]):
        self.src = str(path_or_url)
        self.is_url = self.src.startswith(("http://", "https://"))

    def read(self, start: int, length: int) -> bytes:
        if length <= 0:
            return b""
        if self.is_url:
            import requests
            r = requests.get(self.src, headers={"Range": f"bytes={start}-{start + length - 1}"})
            if r.status_code != 206:
                raise ValueError(f"Server doesn't support range requests: {r.status_code}")
            return r.content
        with open(self.src, "rb") as fh:
            fh.seek(start)
            return fh.read(length)

    def read_ranges(self, ranges: Sequence[Tuple[int, int]]) -> List[bytes]:
        if not self.is_url:
            out = []
            with open(self.src, "rb") as fh:
                for s, n in ranges:
                    fh.seek(s)
                    out.append(fh.read(n))
            return out
        return [self.read(s, n) for s, n in ranges]


def read_index(src: Union[str, Path, Source]) -> Tuple[int, Dict]:
    """Index size and JSON index (cli.py:898-919)."""
    s = src if isinstance(src, Source) else Source(src)
    n = struct.unpack(">I", s.read(0, 4))[0]
    return n, json.loads(s.read(4, n).decode("utf-8"))


def select_frame(index: Dict, tile_id: Optional[int] = None, last: bool = False, center: bool = False,
                 bbox: Optional[Sequence[float]] = None) -> Dict:
    """cli.py:926-990: precedence tile_id > last > center > bbox; bbox = first strict intersection."""
    frames = index["frames"]
    if tile_id is not None:
        for f in frames:
            if f["frame_id"] == tile_id:
                return f
        raise KeyError(f"Tile ID {tile_id} not found")
    if last:
        return max(frames, key=lambda f: f["frame_id"])
    if center:
        bbs = [f["bbox"] for f in frames]
        cx = (min(b[0] for b in bbs) + max(b[2] for b in bbs)) / 2
        cy = (min(b[1] for b in bbs) + max(b[3] for b in bbs)) / 2
        best, dmin = None, float("inf")
        for f in frames:
            fx = (f["bbox"][0] + f["bbox"][2]) / 2
            fy = (f["bbox"][1] + f["bbox"][3]) / 2
            d = ((fx - cx) ** 2 + (fy - cy) ** 2) ** 0.5
            if d < dmin:
                dmin, best = d, f
        return best
    if bbox is not None:
        hit = first_intersecting(index, bbox)
        if hit is None:
            raise LookupError(f"No tiles intersect with bbox {bbox}")
        return hit
    raise ValueError("Must specify --tile-id, --bbox, --center, or --last")


_GRID_CACHE: List[Tuple[tuple, Optional[tuple]]] = []  # (fingerprint, grid) of recently queried indexes


def _grid_key(index: Dict) -> tuple:
    """What the derived grid depends on, besides the frames' bboxes (read live at query time): the index object,
    its frame count and the tile geometry.  No reference to the index is kept (a dropped index is not pinned in
    memory); an index whose geometry or frame list length changes in place gets a new grid."""
    t = index.get("transform")
    return (id(index), id(index["frames"]), len(index["frames"]), index.get("tile_size"), index.get("width"),
            index.get("height"), tuple(t) if t else None)


def _grid_of(index: Dict) -> Optional[tuple]:
    """The row-major tile grid of an index as create-streaming writes it (tile size, columns, rows, the transform's
    scale/offset terms), or None when the index is not that grid.  Derived once per index geometry (a bbox query
    is latency-bound: the per-query dict walks cost more than the tests themselves).  The frames' bboxes are not
    cached: first_intersecting reads them from the index on every query."""
    frames = index["frames"]
    key = _grid_key(index)
    for k, g in _GRID_CACHE:
        if k == key:
            return g
    T, W, H, t = index.get("tile_size"), index.get("width"), index.get("height"), index.get("transform")
    g = None
    if T and W and H and t and len(t) >= 6 and t[1] == 0 and t[3] == 0 and t[0] != 0 and t[4] != 0:
        tc, tr = -(-int(W) // int(T)), -(-int(H) // int(T))
        if len(frames) == tc * tr and all(fr["frame_id"] == k for k, fr in enumerate(frames)):
            g = (int(T), tc, tr, float(t[0]), float(t[2]), float(t[4]), float(t[5]))
    _GRID_CACHE.insert(0, (key, g))
    del _GRID_CACHE[8:]
    return g


def first_intersecting(index: Dict, bbox: Sequence[float]) -> Optional[Dict]:
    """intersecting(index, bbox)[0] (cli.py:976-987) without the linear scan when the index is the
    row-major tile grid create-streaming writes: only tiles within one tile of the bbox's pixel footprint
    are tested, in index order, with the same strict inequalities on the stored bboxes."""
    g = _grid_of(index)
    if g is None:
        hits = intersecting(index, bbox)
        return hits[0] if hits else None
    T, tc, tr, a, c, e, f = g
    frames = index["frames"]
    x0, y0, x1, y1 = bbox
    ca, cb = (x0 - c) / a, (x1 - c) / a
    if cb < ca:
        ca, cb = cb, ca
    ra, rb = (y0 - f) / e, (y1 - f) / e
    if rb < ra:
        ra, rb = rb, ra
    floor = math.floor
    ct0, ct1 = max(0, floor(ca / T) - 1), min(tc - 1, floor(cb / T) + 1)
    rt0, rt1 = max(0, floor(ra / T) - 1), min(tr - 1, floor(rb / T) + 1)
    for r in range(rt0, rt1 + 1):
        k = r * tc
        for cc in range(ct0, ct1 + 1):
            fr = frames[k + cc]
            b = fr["bbox"]
            if x0 < b[2] and x1 > b[0] and y0 < b[3] and y1 > b[1]:
                return fr
    return None


def intersecting(index: Dict, bbox: Sequence[float]) -> List[Dict]:
    """cli.py:976-979 strict-inequality intersection, index order."""
    x0, y0, x1, y1 = bbox
    return [f for f in index["frames"]
            if x0 < f["bbox"][2] and x1 > f["bbox"][0] and y0 < f["bbox"][3] and y1 > f["bbox"][1]]


# ----------------------------------------------------------------------------- decode
class TileDecoder:
    """Batched GPU decode of streaming tiles: one frs_decode_frames call for any number of tiles."""

    def __init__(self, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()

    def decode_streams(self, streams: Sequence[bytes]) -> List[Tuple[np.ndarray, Dict]]:
        metas = [container.parse_metadata(s) for s in streams]
        mds = [container.read_raster_tags(m) for m in metas]
        for m, md in zip(metas, mds):
            if md is None:
                raise ValueError("No metadata found in FLAC file or sidecar file")
            if m.bps not in (16, 32):
                raise ValueError("Only int16/int32 data type is supported")
        out: List[Tuple[np.ndarray, Dict]] = [None] * len(streams)
        # group by (channels, bps, blocksize) so each group is one GPU call
        groups: Dict[Tuple[int, int, int], List[int]] = {}
        for i, m in enumerate(metas):
            groups.setdefault((m.channels, m.bps, m.blocksize), []).append(i)
        for (ch, bps, bs), idx in groups.items():
            blobs = [np.frombuffer(streams[i], dtype=np.uint8)[metas[i].audio_offset:] for i in idx]
            counts = [int(mds[i]["width"]) * int(mds[i]["height"]) for i in idx]
            # one fused decode + de-normalise per raster dtype (tiles of one file share it)
            by_dt: Dict[str, List[int]] = {}
            for j, i in enumerate(idx):
                by_dt.setdefault(str(mds[i]["dtype"]), []).append(j)
            vals_of: Dict[int, np.ndarray] = {}
            for dts, js in by_dt.items():
                sel = [idx[j] for j in js]
                sb = [blobs[j] for j in js]
                so = np.zeros(len(sb) + 1, dtype=np.int64)
                so[1:] = np.cumsum([len(b) for b in sb])
                cnt = [counts[j] for j in js]
                blob = sb[0] if len(sb) == 1 else np.concatenate(sb)  # one tile (extract): no host copy
                allv = self.ctx.decode_tiles_host(blob, so, cnt, channels=ch, bps=bps,
                                                  data_min=[mds[i]["data_min"] for i in sel],
                                                  data_max=[mds[i]["data_max"] for i in sel], dtype=np.dtype(dts),
                                                  blocksize=bs)
                p0 = 0
                for j, n in zip(js, cnt):
                    vals_of[j] = allv[p0:p0 + n]
                    p0 += n
            for j, i in enumerate(idx):
                md = mds[i]
                vals = vals_of[j]
                H, W, C = int(md["height"]), int(md["width"]), int(md["count"])
                arr = vals.reshape(H, W, C).transpose(2, 0, 1) if C > 1 else vals.reshape(1, H, W)
                out[i] = (np.ascontiguousarray(arr), md)
        return out


def fetch_tiles(src: Union[str, Path, Source], frames: Sequence[Dict], index_size: int) -> List[bytes]:
    s = src if isinstance(src, Source) else Source(src)
    return s.read_ranges([(4 + index_size + f["byte_offset"], f["byte_size"]) for f in frames])


def extract_streaming(flac_url: Union[str, Path], output: Path, bbox: Optional[Sequence[float]] = None,
                      tile_id: Optional[int] = None, center: bool = False, last: bool = False,
                      ctx: Optional[Context] = None, level: int = 0, nodata="index", band: int = 1) -> Dict:
    """cli.py:875-1039: pick one tile, range-read it, decode it and write it as a GeoTIFF.  `level` (extension):
    pick among the tiles of that overview level (tile ids are the level's own frame ids); the GeoTIFF carries the
    level tile's transform.  `nodata` (nodata_in_force): the GeoTIFF's nodata tag is the value in force.  `band`
    (extension): pick among that stored band's tiles (its frame ids are the ones its index entries carry)."""
    src = Source(flac_url)
    n, index = read_index(src)
    f = select_frame(level_index(band_index(index, band), level), tile_id=tile_id, last=last, center=center,
                     bbox=bbox)
    data = fetch_tiles(src, [f], n)[0]
    (arr, md), = TileDecoder(ctx).decode_streams([data])
    if not (isinstance(nodata, str) and nodata == "index" and "nodata" not in index):  # else: the tile's own tag
        md = dict(md, nodata=nodata_in_force(index, nodata))
    write_tiff_from_meta(Path(output), arr, md)
    return f


def bbox_pixel_window(transform: geotiff.Affine, bbox: Sequence[float], width: int, height: int) -> Dict:
    """Smallest whole-pixel window of a north-up raster that covers bbox [xmin, ymin, xmax, ymax], clipped to the
    raster: columns floor((xmin - c) / a) .. ceil((xmax - c) / a), rows floor((ymax - f) / e) .. ceil((ymin - f) / e).
    Pixel coordinates within 1e-6 of an integer are snapped to it first, so a bbox edge on a pixel (or tile) edge
    does not pull in a sliver pixel through float error (-105.1 -> column 400.0000000000057 for a 0.001 grid)."""
    import math

    def snap(v: float) -> float:
        return float(round(v)) if abs(v - round(v)) < 1e-6 else v
    t = transform
    c0 = math.floor(snap((bbox[0] - t.c) / t.a))
    c1 = math.ceil(snap((bbox[2] - t.c) / t.a))
    r0 = math.floor(snap((bbox[3] - t.f) / t.e))
    r1 = math.ceil(snap((bbox[1] - t.f) / t.e))
    c0, r0 = max(0, c0), max(0, r0)
    c1, r1 = min(width, max(c1, c0)), min(height, max(r1, r0))
    return {"col_off": c0, "row_off": r0, "width": c1 - c0, "height": r1 - r0}


def tile_windows(frames: Sequence[Dict], origin: Tuple[int, int] = (0, 0)) -> List[Tuple[int, int, int, int]]:
    """frs_tile_window rows (col_off, row_off, width, height) of index entries, in their order, relative to the
    (col, row) origin of a destination window: tiles up or left of the origin get negative offsets (the placement
    clips them).  Pure host code."""
    c0, r0 = int(origin[0]), int(origin[1])
    return [(int(f["window"]["col_off"]) - c0, int(f["window"]["row_off"]) - r0, int(f["window"]["width"]),
             int(f["window"]["height"])) for f in frames]


def decode_into_window(streams: Sequence[bytes], frames: Sequence[Dict], origin: Tuple[int, int],
                       shape: Tuple[int, int], ctx: Optional[Context] = None, dst=None, plane: int = 0,
                       planes: int = 1):
    """Decode whole tile streams (one per index entry of `frames`) straight into the (height, width) = shape window
    whose upper-left pixel is the raster's (col, row) = origin: one batched decode + placement on the device
    (frs_decode_tiles_window_device), tiles clipped to the window.  Each tile's frame bytes are uploaded to their
    place in the device blob (the body is never concatenated on the host).  Window pixels no tile covers are zero.
    Returns (DeviceBuffer holding the (1, height, width) raster, its dtype).
    Several bands: the destination is band-planar (planes, height, width) and one call fills plane `plane` of it.
    Without `dst` the buffer is allocated for `planes` planes; with `dst` (the buffer an earlier call returned) the
    tiles go into that buffer, which must hold plane `plane` of this dtype."""
    ctx = ctx or default_context()
    h, w = int(shape[0]), int(shape[1])
    plane, planes = int(plane), int(planes)
    if plane < 0 or (dst is None and plane >= planes):
        raise ValueError("plane must be one of the destination's planes")
    metas = [container.parse_metadata(s) for s in streams]
    mds = [container.read_raster_tags(m) for m in metas]
    wins = tile_windows(frames, origin)
    if not streams or len(wins) != len(streams):
        raise ValueError("one tile stream per index entry")
    for m, md, win in zip(metas, mds, wins):
        if md is None:
            raise ValueError("No metadata found in FLAC file or sidecar file")
        if m.bps not in (16, 32):
            raise ValueError("Only int16/int32 data type is supported")
        if m.channels != 1 or (int(md["width"]), int(md["height"])) != (win[2], win[3]):
            raise ValueError("a streaming tile is one band of its index window's size")
    dtype = np.dtype(mds[0]["dtype"])
    if any(np.dtype(md["dtype"]) != dtype for md in mds):
        raise ValueError("the tiles of one raster share a dtype")
    # one decode call per (bps, blocksize); a file written by create-streaming has one group
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, m in enumerate(metas):
        groups.setdefault((m.bps, m.blocksize), []).append(i)
    order = [i for idx in groups.values() for i in idx]
    sizes = [len(streams[i]) - metas[i].audio_offset for i in order]
    off = np.zeros(len(order) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    pbytes = h * w * dtype.itemsize  # one plane
    if dst is not None and dst.nbytes < (plane + 1) * pbytes:
        raise ValueError("the destination buffer does not hold that plane")
    blob = ctx.alloc(int(off[-1]) + 16)
    own = dst is None
    try:
        if own:
            dst = ctx.alloc(planes * pbytes)
        for k, i in enumerate(order):
            blob.upload(np.frombuffer(streams[i], dtype=np.uint8)[metas[i].audio_offset:], int(off[k]))
        # tiles that do not overlap cover the window exactly when their clipped areas add up to it: only then is the
        # zero fill (np.zeros in the host mosaic this replaces) skipped
        covered = sum(max(0, min(w, c + tw) - max(0, c)) * max(0, min(h, r + th) - max(0, r)) for c, r, tw, th in wins)
        if covered != h * w:
            dst.upload(np.zeros((h, w), dtype=dtype), plane * pbytes)
        k0 = 0
        for (bps, bs), idx in groups.items():
            k1 = k0 + len(idx)
            ctx.decode_tiles_window_device(blob, off[k0:k1 + 1], [wins[i] for i in idx], bps,
                                           [mds[i]["data_min"] for i in idx], [mds[i]["data_max"] for i in idx],
                                           dtype, dst, (1, h, w), blocksize=bs, dst_ptr=dst.ptr + plane * pbytes)
            k0 = k1
    except BaseException:
        if own and dst is not None:
            dst.close()
        raise
    finally:
        blob.close()
    return dst, dtype


def _decode_bands_into_window(src, index_size: int, band_frames: Sequence[Sequence[Dict]], origin: Tuple[int, int],
                              shape: Tuple[int, int], ctx: Optional[Context] = None):
    """decode_into_window for several bands: band_frames[k] holds the index entries of the tiles of plane k.  Only those
    tiles are fetched; each band's are decoded straight into its plane of one band-planar device buffer.  Returns
    (DeviceBuffer holding the (len(band_frames), height, width) raster, its dtype)."""
    dst, dtype = None, None
    try:
        for k, frames in enumerate(band_frames):
            datas = fetch_tiles(src, frames, index_size)
            dst, dt = decode_into_window(datas, frames, origin, shape, ctx, dst=dst, plane=k, planes=len(band_frames))
            if dtype is not None and dt != dtype:
                raise ValueError("the bands of one file share a dtype")
            dtype = dt
    except BaseException:
        if dst is not None:
            dst.close()
        raise
    return dst, dtype


def _download_raster(dst, dtype, h: int, w: int, nb: int = 1) -> np.ndarray:
    out = np.empty((nb, h, w), dtype=dtype)
    try:
        dst.download(out=out)
    finally:
        dst.close()
    return out


def extract_bbox_mosaic(flac_url: Union[str, Path], bbox: Sequence[float], ctx: Optional[Context] = None,
                        crop: bool = True, level: int = 0, bands=None):
    """Extension: decode every tile intersecting bbox in one GPU batch straight into the raster window
    they cover, or (crop=True) into the whole-pixel window of the bbox itself (bbox_pixel_window): the tiles are
    placed and clipped on the device (decode_into_window), the host only receives the final window.  Returns
    (array (1, h, w), window dict, transform list); with `level` > 0 the tiles, the window and the transform are that
    overview level's.  `bands` (stored band numbers, or "all"): those bands, (len(bands), h, w); only their tiles
    are fetched."""
    src = Source(flac_url)
    n, index = read_index(src)
    sel = _bands_to_read(index, bands)
    band_hits = [intersecting(level_index(band_index(index, b), level), bbox) for b in sel]
    index = level_index(band_index(index, sel[0]), level)
    hits = band_hits[0]
    if not hits:
        raise LookupError(f"No tiles intersect with bbox {bbox}")
    c0 = min(f["window"]["col_off"] for f in hits)
    r0 = min(f["window"]["row_off"] for f in hits)
    c1 = max(f["window"]["col_off"] + f["window"]["width"] for f in hits)
    r1 = max(f["window"]["row_off"] + f["window"]["height"] for f in hits)
    t = geotiff.Affine(*index["transform"][:6])
    win = {"col_off": c0, "row_off": r0, "width": c1 - c0, "height": r1 - r0}
    if crop and t.b == 0 and t.d == 0:
        cw = bbox_pixel_window(t, bbox, int(index["width"]), int(index["height"]))
        # (the tiles intersecting the bbox cover its pixel window)
        a0, b0 = max(cw["col_off"], c0), max(cw["row_off"], r0)
        a1 = min(cw["col_off"] + cw["width"], c1)
        b1 = min(cw["row_off"] + cw["height"], r1)
        win = {"col_off": a0, "row_off": b0, "width": max(a1 - a0, 0), "height": max(b1 - b0, 0)}
    if win["width"] == 0 or win["height"] == 0:  # an empty pixel window: nothing to decode
        md = container.read_raster_tags(container.parse_metadata(fetch_tiles(src, hits[:1], n)[0]))
        out = np.zeros((len(sel), win["height"], win["width"]), dtype=np.dtype(md["dtype"]))
    else:
        dst, dtype = _decode_bands_into_window(src, n, band_hits, (win["col_off"], win["row_off"]),
                                               (win["height"], win["width"]), ctx)
        out = _download_raster(dst, dtype, win["height"], win["width"], len(sel))
    wt = geotiff.window_transform(t, win["col_off"], win["row_off"])
    return out, win, list(wt)


RESAMPLING_READ = ("nearest", "bilinear", "average")


def pick_level_for_scale(index: Dict, scale: float) -> int:
    """The coarsest level k the file holds with 2**k <= scale (`scale`: level-0 pixels per output pixel), so that the
    resample that follows still reduces, never enlarges, what it reads; 0 when scale < 1 or the file holds level 0
    only.  Pure."""
    best = 0
    for k in overview_levels(index):
        if k > best and float(2 ** k) <= scale:
            best = k
    return best


def window_request(index: Dict, bbox: Sequence[float], out_w: int, out_h: int, level: Optional[int] = None,
                   margin: int = 0) -> Dict:
    """What read_window needs to return bbox = [xmin, ymin, xmax, ymax] as out_w x out_h pixels, from the index alone
    (pure).  The transform must be north-up (b = d = 0, a > 0, e < 0), else ValueError.
      scale       max(bbox width in level-0 pixels / out_w, bbox height in level-0 pixels / out_h)
      level       pick_level_for_scale(index, scale), or `level` when given
      window      the level's whole pixels to decode: columns floor(x) - 1 .. ceil(x + width) + 1 and rows floor(y) - 1
                  .. ceil(y + height) + 1 of the bbox's fractional pixel rectangle (x, y, width, height) in that level,
                  clipped to the level's raster.  The one-pixel margin serves bilinear's second tap and absorbs the last
                  hi(j) landing an ulp past the rectangle.  Width and height are 0 when nothing is left.  With
                  `margin` = m the rectangle is first widened by m output pixels (m * width / out_w, m * height / out_h)
                  on every side, for a kernel that looks at an output's neighbours (the hillshade); level, rect and
                  transform are the unwidened box's.
      rect        (x0, y0, width, height): the rectangle relative to the window's origin, as frs_window_map takes it
      frames      the level's index entries whose `window` intersects the window, in index order
      transform   of the result: [(xmax - xmin) / out_w, 0, xmin, 0, -(ymax - ymin) / out_h, ymax]"""
    out_w, out_h = int(out_w), int(out_h)
    if out_w < 1 or out_h < 1:
        raise ValueError("the output size must be at least 1 x 1")
    xmin, ymin, xmax, ymax = (float(v) for v in bbox)
    if not (xmax > xmin and ymax > ymin):
        raise ValueError("bbox must be xmin,ymin,xmax,ymax with xmax > xmin and ymax > ymin")
    a0, b0, _, d0, e0, _ = (float(v) for v in list(index["transform"])[:6])
    if b0 != 0 or d0 != 0:
        raise ValueError("a windowed read needs a north-up transform (rotation terms b and d must be 0)")
    if not (a0 > 0 and e0 < 0):
        raise ValueError("a windowed read needs a north-up transform (a > 0, e < 0)")
    scale = max(((xmax - xmin) / a0) / out_w, ((ymin - ymax) / e0) / out_h)
    k = pick_level_for_scale(index, scale) if level is None else int(level)
    li = level_index(index, k)
    a, _, c, _, e, f = (float(v) for v in list(li["transform"])[:6])
    W, H = int(li["width"]), int(li["height"])
    x, y = (xmin - c) / a, (ymax - f) / e
    width, height = (xmax - xmin) / a, (ymin - ymax) / e
    margin = int(margin)
    if margin < 0:
        raise ValueError("margin must be >= 0")
    if margin:
        mx, my = margin * (width / out_w), margin * (height / out_h)
        c0, c1 = max(math.floor(x - mx) - 1, 0), min(math.ceil(x + width + mx) + 1, W)
        r0, r1 = max(math.floor(y - my) - 1, 0), min(math.ceil(y + height + my) + 1, H)
    else:
        c0, c1 = max(math.floor(x) - 1, 0), min(math.ceil(x + width) + 1, W)
        r0, r1 = max(math.floor(y) - 1, 0), min(math.ceil(y + height) + 1, H)
    if c1 <= c0 or r1 <= r0:
        c1, r1 = c0, r0
    frames = []
    if c1 > c0:
        for fr in li["frames"]:
            w = fr["window"]
            if (w["col_off"] < c1 and w["col_off"] + w["width"] > c0 and w["row_off"] < r1
                    and w["row_off"] + w["height"] > r0):
                frames.append(fr)
    return {"level": k, "scale": scale, "out_w": out_w, "out_h": out_h,
            "window": {"col_off": c0, "row_off": r0, "width": c1 - c0, "height": r1 - r0},
            "rect": (x - c0, y - r0, width, height), "frames": frames,
            "transform": [(xmax - xmin) / out_w, 0.0, xmin, 0.0, -(ymax - ymin) / out_h, ymax]}


def _index_dtype(src: "Source", index: Dict, index_size: int) -> np.dtype:
    """The raster dtype, which the index does not carry: from the tags of the file's smallest tile."""
    frames = [fr for k in overview_levels(index) for fr in level_index(index, k)["frames"]]
    if not frames:
        raise ValueError("the streaming index lists no tiles")
    data = fetch_tiles(src, [min(frames, key=lambda fr: fr["byte_size"])], index_size)[0]
    md = container.read_raster_tags(container.parse_metadata(data))
    if md is None:
        raise ValueError("No metadata found in FLAC file or sidecar file")
    return np.dtype(md["dtype"])


def nodata_in_force(index: Dict, nodata="index") -> Optional[float]:
    """The nodata value a read uses: the index's own ("index", the default), none (None or "none"), or a number that
    overrides the index."""
    if nodata is None or (isinstance(nodata, str) and nodata == "none"):
        return None
    if isinstance(nodata, str):
        if nodata != "index":
            raise ValueError(f"nodata must be a number, None, 'none' or 'index', got {nodata!r}")
        return index_nodata(index)
    return float(nodata)


def _fill_in_dtype(fill: float, dtype: np.dtype):
    """`fill` as the resample kernels convert it: integers round half to even, clamp, cast"""
    if dtype.kind == "f":
        return fill
    ii = np.iinfo(dtype)
    return int(min(max(np.rint(float(fill)), ii.min), ii.max))


def read_window(flac_url: Union[str, Path], bbox: Sequence[float], out_w: int, out_h: int,
                resampling: str = "average", level: Optional[int] = None, fill=None, ctx: Optional[Context] = None,
                nodata="index", bands=None):
    """Extension: bbox = [xmin, ymin, xmax, ymax] of band 1 as exactly out_w x out_h pixels.  window_request picks the
    overview level and the tiles; they are range-read (fetch_tiles), decoded and placed into the level's pixel window
    on the device (decode_into_window), resampled there onto the requested grid (frs_resample_window_device, the
    definition in include/flac_raster_amd.h) and only the out_h x out_w result is downloaded.  Pixels outside the
    raster get `fill`; a bbox that misses the raster gives an all-`fill` array without a GPU call.  `level` forces
    the overview level.  `nodata`: "index" (the default) takes the index's "nodata" key, a number overrides it, None
    turns masking off; with a value in force the masked kernel runs (frs_resample_window_nodata_device): nodata pixels
    stay out of every output, and an output with no valid weight gets `fill`.  `fill` defaults to the nodata value in
    force, else to 0; it must be finite, or NaN for a float raster read with a nodata value.  A file without the key
    reads exactly as before.  Returns (array (1, out_h, out_w), transform list).
    `bands` (a sequence of stored band numbers, or "all"): those bands in that order, (len(bands), out_h, out_w).  Only
    their tiles are fetched; they are decoded into one band-planar device window and resampled in one call."""
    if resampling not in RESAMPLING_READ:
        raise ValueError(f"resampling must be one of {', '.join(RESAMPLING_READ)}; got {resampling!r}")
    if fill is not None and math.isinf(float(fill)):
        raise ValueError("fill must be finite")
    src = Source(flac_url)
    n, index = read_index(src)
    nd = nodata_in_force(index, nodata)
    if fill is None:
        fill = 0 if nd is None else nd
    fill = float(fill)
    if not (math.isfinite(fill) or (nd is not None and math.isnan(fill))):
        raise ValueError("fill must be finite (or NaN for a float raster read with a nodata value)")
    sel = _bands_to_read(index, bands)
    nb = len(sel)
    reqs = [window_request(band_index(index, b), bbox, out_w, out_h, level) for b in sel]
    req = reqs[0]
    out_w, out_h = req["out_w"], req["out_h"]
    if not req["frames"]:
        dtype = _index_dtype(src, index, n)
        if nd is not None:
            nodata_for_dtype(nd, dtype)
        if math.isnan(fill) and dtype.kind != "f":
            raise ValueError("a NaN fill needs a float raster")
        out = np.empty((nb, out_h, out_w), dtype=dtype)
        out[...] = _fill_in_dtype(fill, dtype)  # the kernel's rule
        return out, req["transform"]
    ctx = ctx or default_context()
    win = req["window"]
    wdev, dtype = _decode_bands_into_window(src, n, [r["frames"] for r in reqs], (win["col_off"], win["row_off"]),
                                            (win["height"], win["width"]), ctx)
    try:
        dst = ctx.alloc(nb * out_h * out_w * dtype.itemsize)
    except BaseException:
        wdev.close()
        raise
    try:
        if nd is not None:
            nodata_for_dtype(nd, dtype)
        # every plane in one call
        ctx.resample_window_device(wdev.ptr, ctx.make_raster_desc(win["height"], win["width"], dtype, nbands=nb),
                                   dst.ptr, ctx.make_raster_desc(out_h, out_w, dtype, nbands=nb), req["rect"],
                                   resampling, fill, nodata=nd)
    except BaseException:
        dst.close()
        raise
    finally:
        wdev.close()
    return _download_raster(dst, dtype, out_h, out_w, nb), req["transform"]


STATS_FROM = ("auto", "file", "window")
RENDER_WINDOW_BINS = 256  # bins of the histogram stats_from="window" takes at most


def _file_statistics_for(index: Dict, nd: Optional[float]) -> Dict:
    """The index's "statistics" for a render under the nodata value `nd` in force; LookupError when the index has
    none, ValueError when they were taken under another nodata value."""
    st = index_statistics(index)
    if st is None:
        raise LookupError('the file has no "statistics" in its index (create-streaming --stats writes them); '
                          'use stats_from="window" or a range:lo,hi stretch')
    own = index_nodata(index)
    same = (nd is None and own is None) or (nd is not None and own is not None
                                            and (nd == own or (math.isnan(nd) and math.isnan(own))))
    if not same:
        raise ValueError(f"the file's statistics were taken with nodata {own}, the render uses {nd}; "
                         'use stats_from="window"')
    return st


def render_window(flac_url: Union[str, Path], bbox: Sequence[float], out_w: int, out_h: int,
                  stretch: str = "percentile:2,98", stats_from: str = "auto", colormap="gray", gamma: float = 1.0,
                  transfer: str = "linear", lut_size: Optional[int] = None, resampling: str = "average",
                  level: Optional[int] = None, nodata="index", channels: int = 4, nodata_rgba=(0, 0, 0, 0),
                  ctx: Optional[Context] = None, hillshade: Optional[Sequence[float]] = None, z_factor: float = 1.0,
                  shade_strength: float = 1.0, shade_only: bool = False, band: int = 1, bands=None):
    """Extension: bbox = [xmin, ymin, xmax, ymax] of band 1 as a stretched 8-bit image of exactly out_w x out_h pixels.
    `band` renders another stored band by the same path: the stretch and the file statistics are that band's
    (band_index).  `bands` = (r, g, b) renders a colour composite of three stored bands instead
    (frs_render_composite_window_device): their tiles alone are fetched and decoded into one band-planar device window,
    and one kernel resamples the three planes, stretches each over its own limits -- each band's stored statistics
    under stats_from "file" / "auto", each plane of the decoded window under "window"; range:lo,hi applies to all
    three -- and writes R, G, B, A.  A pixel where any of the three bands has no data takes nodata_rgba.  The colormap
    must stay "gray": gamma and transfer shape the three (equal) curves.  hillshade and channels other than 4 are
    rejected with `bands`.
    With hillshade = (azimuth, altitude) in degrees the image is shaded by frs_render_shaded_window_device: Horn's
    gradient on the output grid, the output pixel's ground size (xmax - xmin) / out_w by (ymax - ymin) / out_h, heights
    multiplied by z_factor, the colours scaled by render.shade_table(shade_strength).  The decoded window then reaches
    one output pixel beyond the box (window_request's margin), so that neighbouring map tiles shade identically along
    their seam.  A geographic CRS (degrees against metres) needs a z_factor from the caller; nothing is guessed.
    shade_only renders the shade alone: a one-entry white table over a fixed range, no statistics pass (stretch,
    colormap and stats_from are not looked at).
    It is read_window up to the decoded device window (window_request, fetch_tiles, decode_into_window); then
    frs_render_window_device (the definition in include/flac_raster_amd.h) resamples the window onto the requested
    grid, maps every value to a colour and writes interleaved uint8 pixels, and only those out_h * out_w * channels
    bytes are downloaded.  A pixel without data (outside the raster, masked by the nodata value in force, NaN) takes
    `nodata_rgba`; a bbox that misses the raster gives an image of nothing else without a GPU call.
      stretch      render.stretch_limits: "minmax", "percentile:p,q", "stddev:k" or "range:lo,hi" give (lo, hi)
      stats_from   where the stretch's statistics come from.  "file": the index's "statistics" (create-streaming
                   --stats): LookupError when the index has none, ValueError when the nodata value in force differs from
                   the index's.  "window": frs_band_stats_device and frs_band_histogram_device (256 bins at most) on
                   the decoded device window before it is resampled; nothing but the records is downloaded.  "auto":
                   "file" when it applies, else "window".  A range:lo,hi stretch needs no statistics and runs neither
                   pass.  "window" makes neighbouring map tiles stretch differently -- each sees its own values --
                   which is why "file" is preferred: one stretch for the whole raster.
      colormap, gamma, transfer, lut_size   render.build_lut; lut_size defaults to 256, or to 4096 when gamma != 1 or
                   transfer != "linear"
      channels     1 = R, 2 = R, A, 4 = R, G, B, A
    `resampling`, `level` and `nodata` are read_window's.  Returns (uint8 array (out_h, out_w, channels), transform
    list)."""
    from . import render as rn
    from ._native import pack_rgba
    if resampling not in RESAMPLING_READ:
        raise ValueError(f"resampling must be one of {', '.join(RESAMPLING_READ)}; got {resampling!r}")
    if stats_from not in STATS_FROM:
        raise ValueError(f"stats_from must be one of {', '.join(STATS_FROM)}; got {stats_from!r}")
    channels = int(channels)
    if channels not in (1, 2, 4):
        raise ValueError(f"channels must be 1, 2 or 4; got {channels}")
    if bands is not None:
        bands = [int(b) for b in bands]
        if len(bands) != 3:
            raise ValueError(f"a composite takes three bands (r, g, b); got {bands}")
        if int(band) != 1:
            raise ValueError("give band or bands, not both")
        if hillshade is not None:
            raise ValueError("a composite cannot be hillshaded")
        if channels != 4:
            raise ValueError("a composite is written with 4 channels (R, G, B, A)")
        if not (isinstance(colormap, str) and colormap == "gray"):
            raise ValueError('a composite keeps the "gray" colormap: gamma and transfer shape its curves')
    shade = None
    if hillshade is None:
        if shade_only or z_factor != 1.0 or shade_strength != 1.0:
            raise ValueError("z_factor, shade_strength and shade_only need hillshade")
    else:
        xmin, ymin, xmax, ymax = (float(v) for v in bbox)
        azimuth, altitude = hillshade
        if int(out_w) < 1 or int(out_h) < 1:
            raise ValueError("the output size must be at least 1 x 1")
        shade = (rn.light_vector(azimuth, altitude),
                 *rn.shade_scales((xmax - xmin) / int(out_w), (ymax - ymin) / int(out_h), z_factor),
                 rn.shade_table(shade_strength))
    if shade_only:
        stretch, colormap, gamma, transfer, lut_size = "range:0,1", [(0, 255, 255, 255), (1, 255, 255, 255)], 1.0, \
            "linear", 1
    kind, _ = rn.parse_stretch(stretch)
    lut = rn.build_lut(colormap, rn.default_lut_size(gamma, transfer) if lut_size is None else lut_size, gamma,
                       transfer)
    packed = pack_rgba(nodata_rgba)
    src = Source(flac_url)
    n, index = read_index(src)
    nd = nodata_in_force(index, nodata)
    if bands is not None:
        return _render_composite(src, n, index, bands, bbox, out_w, out_h, stretch, kind, stats_from, lut, packed,
                                 resampling, level, nd, ctx)
    index = band_index(index, band)
    file_stats = None
    if kind != "range" and stats_from != "window":
        try:
            file_stats = _file_statistics_for(index, nd)
        except (LookupError, ValueError):
            if stats_from == "file":
                raise
    req = window_request(index, bbox, out_w, out_h, level) if shade is None else \
        window_request(index, bbox, out_w, out_h, level, margin=1)
    out_w, out_h = req["out_w"], req["out_h"]
    if not req["frames"]:
        out = np.empty((out_h, out_w, channels), dtype=np.uint8)
        rgba = [packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF, packed >> 24]
        out[...] = {1: rgba[:1], 2: [rgba[0], rgba[3]], 4: rgba}[channels]
        return out, req["transform"]
    ctx = ctx or default_context()
    win = req["window"]
    datas = fetch_tiles(src, req["frames"], n)
    wdev, dtype = decode_into_window(datas, req["frames"], (win["col_off"], win["row_off"]),
                                     (win["height"], win["width"]), ctx)
    dst = None
    try:
        if nd is not None:
            nd = nodata_for_dtype(nd, dtype)
        sd = ctx.make_raster_desc(win["height"], win["width"], dtype)
        if kind == "range":
            stats = None
        elif file_stats is not None:
            stats = file_stats
        else:
            from .stats import _device_statistics
            stats = _device_statistics(ctx, wdev.ptr, sd, nd, RENDER_WINDOW_BINS)[0]
        lo, hi = rn.stretch_limits(stats, stretch)
        dst = ctx.alloc(out_h * out_w * channels)
        if shade is None:
            ctx.render_window_device(wdev.ptr, sd, dst.ptr, out_h, out_w, req["rect"], resampling, lo, hi, lut,
                                     nodata_rgba=packed, channels=channels, nodata=nd)
        else:
            ctx.render_shaded_window_device(wdev.ptr, sd, dst.ptr, out_h, out_w, req["rect"], resampling, lo, hi,
                                            lut, shade[0], shade[1], shade[2], shade[3], nodata_rgba=packed,
                                            channels=channels, nodata=nd)
        out = np.empty((out_h, out_w, channels), dtype=np.uint8)
        dst.download(out=out)
    finally:
        wdev.close()
        if dst is not None:
            dst.close()
    return out, req["transform"]


def _render_composite(src: "Source", n: int, index: Dict, bands: Sequence[int], bbox, out_w: int, out_h: int,
                      stretch: str, kind: str, stats_from: str, lut, packed: int, resampling: str,
                      level: Optional[int], nd: Optional[float], ctx: Optional[Context]):
    """render_window(bands=(r, g, b)) behind its argument checks: (uint8 (out_h, out_w, 4), transform list)."""
    from . import render as rn
    bis = [band_index(index, b) for b in bands]
    file_stats: List[Optional[Dict]] = [None, None, None]
    if kind != "range" and stats_from != "window":
        for k, bi in enumerate(bis):
            try:
                file_stats[k] = _file_statistics_for(bi, nd)
            except (LookupError, ValueError):
                if stats_from == "file":
                    raise
    reqs = [window_request(bi, bbox, out_w, out_h, level) for bi in bis]
    req = reqs[0]
    out_w, out_h = req["out_w"], req["out_h"]
    if not req["frames"]:
        out = np.empty((out_h, out_w, 4), dtype=np.uint8)
        out[...] = [packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF, packed >> 24]
        return out, req["transform"]
    ctx = ctx or default_context()
    win = req["window"]
    wdev, dtype = _decode_bands_into_window(src, n, [r["frames"] for r in reqs], (win["col_off"], win["row_off"]),
                                            (win["height"], win["width"]), ctx)
    dst = None
    try:
        if nd is not None:
            nd = nodata_for_dtype(nd, dtype)
        plane = win["height"] * win["width"] * dtype.itemsize
        sd1 = ctx.make_raster_desc(win["height"], win["width"], dtype)
        lo3, hi3 = [], []
        for k in range(3):
            if kind == "range":
                stats = None
            elif file_stats[k] is not None:
                stats = file_stats[k]
            else:
                from .stats import _device_statistics
                stats = _device_statistics(ctx, wdev.ptr + k * plane, sd1, nd, RENDER_WINDOW_BINS)[0]
            lo, hi = rn.stretch_limits(stats, stretch)
            lo3.append(lo)
            hi3.append(hi)
        dst = ctx.alloc(out_h * out_w * 4)
        ctx.render_composite_window_device(wdev.ptr, ctx.make_raster_desc(win["height"], win["width"], dtype, nbands=3),
                                           dst.ptr, out_h, out_w, req["rect"], resampling, lo3, hi3, lut,
                                           nodata_rgba=packed, nodata=nd)
        out = np.empty((out_h, out_w, 4), dtype=np.uint8)
        dst.download(out=out)
    finally:
        wdev.close()
        if dst is not None:
            dst.close()
    return out, req["transform"]


def reconstruct_device(flac_url: Union[str, Path], ctx: Optional[Context] = None, level: int = 0, bands=None):
    """Every tile of a streaming file (of overview level `level`) in one batched decode, placed into the level's full
    raster in device memory.  Returns (DeviceBuffer, dtype, level_index(index, level)).  `bands` (stored band numbers,
    or "all"): the buffer is band-planar (len(bands), H, W), one batched decode per band, and the index returned is the
    first named band's."""
    src = Source(flac_url)
    n, index = read_index(src)
    sel = _bands_to_read(index, bands)
    levels = [level_index(band_index(index, b), level) for b in sel]
    index = levels[0]
    if not all(li["frames"] for li in levels):
        raise ValueError("the streaming index lists no tiles")
    dst, dtype = _decode_bands_into_window(src, n, [li["frames"] for li in levels], (0, 0),
                                           (int(index["height"]), int(index["width"])), ctx)
    return dst, dtype, index


def reconstruct(flac_url: Union[str, Path], ctx: Optional[Context] = None, level: int = 0, bands=None):
    """The whole raster of a streaming file, or of one overview level: (array (1, H, W), transform list); with `bands`
    (stored band numbers, or "all") the array is (len(bands), H, W)."""
    dst, dtype, index = reconstruct_device(flac_url, ctx, level, bands)
    nb = dst.nbytes // (int(index["height"]) * int(index["width"]) * np.dtype(dtype).itemsize)
    return _download_raster(dst, dtype, int(index["height"]), int(index["width"]), nb), list(index["transform"])


def extract_all(flac_url: Union[str, Path], output: Path, ctx: Optional[Context] = None, level: int = 0,
                nodata="index", bands=None) -> Dict:
    """extract-streaming --all: write the reconstruction (of overview level `level`) as a GeoTIFF with the index's CRS
    and the level's transform, and the nodata value in force (nodata_in_force) as its nodata tag.  Returns
    level_index(index, level).  `bands` (stored band numbers, or "all"): a GeoTIFF of those bands."""
    arr, tr = reconstruct(flac_url, ctx, level, bands)
    _, index = read_index(flac_url)
    nd = nodata_in_force(index, nodata)
    index = level_index(index, level)
    crs = index.get("crs")
    epsg = int(crs.split(":")[1]) if crs and str(crs).upper().startswith("EPSG:") else None
    geotiff.write(Path(output), arr, transform=geotiff.Affine(*tr[:6]), epsg=epsg, nodata=nd)
    return index


def verify_streaming(flac_path: Union[str, Path], band: np.ndarray, ctx: Optional[Context] = None,
                     band_number: int = 1) -> Dict:
    """create-streaming --verify: read the written file back (what is checked is what is on disk), decode it into a
    device raster through the window call, upload the source band and compare the two on the device
    (frs_compare_device).  Returns the un-wrapped differences as compare's ``exact`` key: n_different,
    max_difference, mean_difference, first_difference.

    A file with overviews has every level checked the same way: the pyramid is recomputed on the device from the
    uploaded band with the index's ``resampling`` (frs_downsample2_device, level k from level k - 1) and each decoded
    level is compared with it.  The result then also holds ``levels_checked`` (level 0 included) and ``levels``, one
    dict per level (``level`` + the four keys above); the four top-level keys describe the first level that differs,
    or level 0 when none does.  Where the index says ``nodata_aware`` the pyramid is recomputed with the masked step
    and the index's nodata value.  `band_number`: the stored band that `band` is the source of (its tiles, levels and
    overview settings are the ones checked)."""
    from .compare import _exact
    ctx = ctx or default_context()
    band = np.asarray(band)
    sel = None if int(band_number) == 1 else [int(band_number)]
    dst, dtype, index = reconstruct_device(flac_path, ctx, bands=sel)
    bufs = [dst]
    try:
        H, W = int(index["height"]), int(index["width"])
        if band.shape != (H, W) or band.dtype != dtype:
            raise ValueError(f"source band {band.shape} {band.dtype} does not match the file's {(H, W)} {dtype}")
        srcbuf = ctx.alloc(band.nbytes)
        bufs.append(srcbuf)
        srcbuf.upload(band)
        d = ctx.make_compare_desc(H, W, dtype)
        res = _exact(ctx.compare_device(srcbuf.ptr, dst.ptr, d), W)
        ov = index.get("overviews")
        if not ov:
            return res
        per_level = [dict(level=0, **res)]
        nd = index_nodata(index) if ov.get("nodata_aware") else None
        if ov.get("nodata_aware") and nd is None:
            raise ValueError("the index says nodata_aware but carries no nodata value")
        cur, cur_desc = srcbuf, ctx.make_raster_desc(H, W, dtype)
        for lv in sorted(ov.get("levels", []), key=lambda x: int(x["level"])):
            k, h, w = int(lv["level"]), (cur_desc.height + 1) // 2, (cur_desc.width + 1) // 2
            if k != len(per_level) or (int(lv["height"]), int(lv["width"])) != (h, w):
                raise ValueError(f"overview level {k} is not the 2x reduction of the level before it")
            nxt = ctx.alloc(h * w * dtype.itemsize)
            bufs.append(nxt)
            cur_desc = ctx.downsample2_device(cur.ptr, cur_desc, nxt.ptr, mode=ov["resampling"], nodata=nd)
            if cur is not srcbuf:
                cur.close()
            cur = nxt
            got, gdt, _ = reconstruct_device(flac_path, ctx, k, bands=sel)
            bufs.append(got)
            if gdt != dtype:
                raise ValueError(f"overview level {k} is {gdt}, the file's level 0 is {dtype}")
            ex = _exact(ctx.compare_device(cur.ptr, got.ptr, ctx.make_compare_desc(h, w, dtype)), w)
            got.close()
            per_level.append(dict(level=k, **ex))
        bad = [x for x in per_level if x["n_different"] != 0]
        res = {key: (bad[0] if bad else per_level[0])[key] for key in res}
        res.update(levels_checked=len(per_level), levels=per_level)
        return res
    finally:
        for b in bufs:
            b.close()
