"""Shared inputs of the tiny-frame tests (tests/test_tiny_frames_host.py, tests/test_gpu_tiny_frames.py): rasters whose
tiles are whole FLAC streams of one frame of 1..576 samples, or of one 4096-sample frame and such a tail.

rows(n) is an [8, n] raster of eight signal kinds.  Encoded with tile_h = 1 and tile_w = n every row is a tile of its
own: a stream of one n-sample frame ("single").  The [8, 4096 + n] raster at tile_w = 4096 + n gives a full frame and a
tail with frame number 1 ("tail").  The multi-band forms stack kinds as bands, so a tile is one stream of two or three
interleaved channels.  Every array is made once, read-only, and the oracle's streams of it are cached here.
"""
import functools

import numpy as np

from oracle import oracle as O

LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 128, 192, 255, 256, 257,
           576)
TABLE_LENGTHS = (512, 1024, 1152, 2048, 2304)   # further lengths with a block-size code of their own
FULL = 4096
RATE = 44100
KINDS = ("ramp", "resonance", "switching", "constant", "two_level", "noise", "mult8", "two_tones")
PAIRS = ("correlated", "anti", "independent", "constant")
FORMS = ("single", "tail")
LEVELS = (0, 3, 5, 6, 8)
# seed of the two-band rows' noise.  With seed 2 the correlated pair at n = 3 has a side signal of two wasted bits, and
# libFLAC's estimate then makes that VERBATIM frame left-side; seed 3 keeps every frame of n <= 4 independent, which
# tests/test_tiny_frames_host.py demands.  wasted_side_pair() is that other case, kept as an input of its own.
PAIR_SEED = 3


def width(form, n):
    return n if form == "single" else FULL + n


def _kinds(n, rng):
    """[8, n] int64 in int16's range: the eight kinds, KINDS' order"""
    t = np.arange(n, dtype=np.float64)
    var = np.where((np.arange(n) // 8) % 2 == 0, 4.0, 600.0)
    x = np.stack([
        5.0 * t - 12000.0,                                                    # ramp
        9000.0 * np.sin(2.5 * t + 0.3) + rng.integers(-3, 4, n),              # a resonance at 2.5 rad / sample
        2000.0 + var * rng.standard_normal(n),                                # variance switching every 8 samples
        np.full(n, 1234.0),                                                   # constant
        rng.choice([-500.0, 500.0], n),                                       # two levels
        rng.integers(-32768, 32768, n).astype(np.float64),                    # full-range noise
        8.0 * np.rint(300.0 * np.sin(t / 11.0) + rng.integers(-2, 3, n)),     # multiples of 8
        6000.0 * np.sin(0.3 * t) + 4000.0 * np.sin(1.1 * t + 1.0) + rng.integers(-2, 3, n),  # two tones
    ])
    return np.clip(np.rint(x), -32768, 32767).astype(np.int64)


def _as_dtype(x, dtype):
    """int16-range values in `dtype`, scaled so they stay in range (int32: x 4000, the 24-bit path)"""
    dt = np.dtype(dtype)
    if dt == np.int16:
        out = x.astype(np.int16)
    elif dt == np.uint16:
        out = (x + 32768).astype(np.uint16)
    elif dt == np.uint8:
        out = ((x >> 8) + 128).astype(np.uint8)
    elif dt == np.int32:
        out = (x * 4000).astype(np.int32)
    else:
        raise ValueError(dt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _rows64(n, seed):
    x = _kinds(n, np.random.default_rng([seed, n]))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rows(n, seed=0, dtype=np.int16):
    """[8, n] read-only raster of the eight signal kinds"""
    return _as_dtype(_rows64(n, seed), dtype)


@functools.lru_cache(maxsize=None)
def raster(form, n, dtype=np.int16):
    """the mono raster of single(n) / tail(n): [8, n] or [8, 4096 + n]; tile (1, its width)"""
    return rows(width(form, n), 0, dtype)


@functools.lru_cache(maxsize=None)
def raster2(form, n, dtype=np.int16, seed=PAIR_SEED):
    """[2, 8, W] read-only: row r is the pair PAIRS[r % 4] on the base kind ramp-with-noise (r < 4) or two tones"""
    W = width(form, n)
    x = _rows64(W, 1)
    rng = np.random.default_rng([seed, W])
    out = np.empty((2, 8, W), dtype=np.int64)
    for r in range(8):
        base = (x[0] // 2 + x[2] // 4) if r < 4 else x[7]
        pair = PAIRS[r % 4]
        if pair == "correlated":
            other = base + rng.integers(-2, 3, W)
        elif pair == "anti":
            other = -base + rng.integers(-2, 3, W)
        elif pair == "independent":
            other = x[5] // 2
        else:
            base, other = np.full(W, -700 - r), np.full(W, 900 + r)
        out[0, r], out[1, r] = base, other
    return _as_dtype(np.clip(out, -32768, 32767), dtype)


@functools.lru_cache(maxsize=None)
def raster3(form, n, dtype=np.int16):
    """[3, 8, W] read-only: band b of row r is kind (r + 3 b) % 8"""
    x = _rows64(width(form, n), 3)
    return _as_dtype(np.stack([x[(np.arange(8) + 3 * b) % 8] for b in range(3)]), dtype)


def wasted_side_pair():
    """[2, 8, 3] int16: row 4 is a three-sample pair whose side signal has two wasted bits (see PAIR_SEED)"""
    return raster2("single", 3, np.int16, 2)


def raster_of(bands, form, n, dtype=np.int16):
    return {1: raster, 2: raster2, 3: raster3}[bands](form, n, dtype)


def tile_samples(arr, r):
    """row r of a ([bands,] 8, W) raster as the tile's interleaved samples [W, bands]"""
    a = arr[None] if arr.ndim == 2 else arr
    return np.ascontiguousarray(a[:, r, :].T)


def spatial_raster(bands, form, n):
    """int16 ([bands,] 8, W).  The spatial normalisation truncates x / 32767, so only +-32767 and -32768 give a sample
    other than 0: rows 0..4 are noise below that (all-zero frames), row 5 has a few extremes, row 6 one pixel at
    32767 in its last band, row 7 is drawn from {-32768, 0, 32767}."""
    W = width(form, n)
    rng = np.random.default_rng([4, W, bands])
    a = rng.integers(-3000, 3000, (bands, 8, W)).astype(np.int16)
    a[:, 5][rng.random((bands, W)) < 0.1] = 32767
    a[:, 5][rng.random((bands, W)) < 0.1] = -32768
    a[-1, 6, W // 2] = 32767
    a[:, 7] = rng.choice(np.array([-32768, 0, 32767], dtype=np.int16), (bands, W))
    a.setflags(write=False)
    return a if bands > 1 else a[0]


@functools.lru_cache(maxsize=None)
def reference(bands, form, n, dtype=np.int16, level=5, spatial=False):
    """Per tile of raster_of(bands, form, n, dtype) (spatial: spatial_raster): [(pcm [W, bands] int32, data_min,
    data_max, stream_bps, the oracle's frames at `level`)]"""
    arr = spatial_raster(bands, form, n) if spatial else raster_of(bands, form, n, dtype)
    out = []
    for r in range(8):
        s = tile_samples(arr, r)
        if spatial:
            pcm, mn, mx, bps = O.normalize_spatial(s), None, None, 32
        else:
            pcm, mn, mx, bps = O.normalize(s)
        pcm.setflags(write=False)
        out.append((pcm, mn, mx, bps, O.encode_frames(pcm, bps, RATE, level=level)))
    return out


def header_fields(frame: bytes):
    """(block-size nibble, channel assignment, header length incl. CRC-8) of the frame header at frame[0]"""
    assert frame[0] == 0xFF and frame[1] == 0xF8
    bsc, src = frame[2] >> 4, frame[2] & 15
    lead = frame[4]
    n = 5 + (0 if lead < 0x80 else 1 if lead < 0xE0 else 2 if lead < 0xF0 else 3)
    n += {6: 1, 7: 2}.get(bsc, 0) + {12: 1, 13: 2, 14: 2}.get(src, 0)
    return bsc, frame[3] >> 4, n + 1


# --------------------------------------------------------------------------------------- two-dimensional edge tiles
GRIDS = {"131x67": (67, 131, 65), "513x513": (513, 513, 512)}   # name -> (height, width, tile)


@functools.lru_cache(maxsize=None)
def grid_band(name):
    H, W, _ = GRIDS[name]
    rng = np.random.default_rng([5, H, W])
    y, x = np.mgrid[0:H, 0:W]
    b = (800 + 300 * np.sin(0.05 * x) * np.cos(0.07 * y) + rng.integers(-40, 41, size=(H, W)) - 1000).astype(np.int16)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    """O.encode_tiles of grid_band(name): (arena, tile_off, mins, maxs)"""
    return O.encode_tiles(grid_band(name), GRIDS[name][2])


def grid_windows(name):
    """row-major (col_off, row_off, width, height) of the grid's tiles"""
    H, W, T = GRIDS[name]
    return [(c, r, min(T, W - c), min(T, H - r)) for r in range(0, H, T) for c in range(0, W, T)]


# ------------------------------------------------------------------------------------------------------------ files
FILE_H, FILE_W, FILE_TILE = 129, 193, 64
FILE_SHAPES = [(65, 97), (33, 49)]


@functools.lru_cache(maxsize=None)
def file_band():
    """129 x 193 int16, values chosen as tests/test_gpu_overviews.py chooses them"""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:FILE_H, 0:FILE_W]
    base = 1000 + 300 * np.sin(0.05 * x) * np.cos(0.07 * y) + rng.integers(-40, 41, size=(FILE_H, FILE_W))
    b = np.round(base - 1200).astype(np.int16)
    b.setflags(write=False)
    return b


def round_trips(tile: np.ndarray) -> bool:
    """the oracle's own normalise -> encode -> decode -> de-normalise of one single-band tile returns the tile"""
    flat = np.ascontiguousarray(tile).reshape(-1, 1)
    pcm, mn, mx, bps = O.normalize(flat)
    back = O.decode_frames(O.encode_frames(pcm, bps, RATE), 1, bps, len(flat))
    return np.array_equal(O.denormalize_i16(back, mn, mx, tile.dtype), flat)


@functools.lru_cache(maxsize=None)
def lossless_tiles(form, n, dtype):
    """the rows r of raster(form, n, dtype) whose tile survives the reference's round trip"""
    arr = raster(form, n, dtype)
    return tuple(r for r in range(8) if round_trips(arr[r]))
