"""ctypes binding of libflac_raster_amd.so (C-ABI declared in include/flac_raster_amd.h).

There is deliberately no CPU fallback: if the library is not built, or there is no gfx950 device, every
codec entry point raises :class:`NativeUnavailable`.  The CPU oracle under ``oracle/`` is test
infrastructure and is never imported here.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libflac_raster_amd.so"

FRS_OK = 0
STATUS = {-1: "FRS_E_ARG", -2: "FRS_E_HIP", -3: "FRS_E_NOSPACE", -4: "FRS_E_CORRUPT",
          -5: "FRS_E_UNSUPPORTED", -6: "FRS_E_NODEV"}

DTYPE_CODES = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3,
               np.dtype(np.int32): 4, np.dtype(np.uint32): 5, np.dtype(np.float32): 6,
               np.dtype(np.float64): 7}
_DT_CACHE = {}  # dtype argument -> (itemsize, DTYPE_CODES code): the bbox-query path skips np.dtype per call

# names every build must export (tests check them against include/flac_raster_amd.h)
EXPORTS = (
    "frs_abi_version", "frs_device_count", "frs_ctx_create", "frs_ctx_destroy", "frs_last_error",
    "frs_encode_arena_bound", "frs_encode_tiles_device", "frs_encode_tiles",
    "frs_decode_frames_device", "frs_decode_frames", "frs_decode_tiles_device", "frs_decode_tiles",
    "frs_decode_tile_device",
    "frs_denormalize_device", "frs_denormalize",
    "frs_dev_malloc", "frs_dev_free", "frs_host_malloc", "frs_host_free", "frs_memcpy_h2d", "frs_memcpy_d2h", "frs_ctx_sync",
    "frs_synth_raster_device", "frs_ctx_stream", "frs_profile_enable", "frs_profile_avg_ms",
    "frs_profile_reset", "frs_comm_unique_id", "frs_comm_init", "frs_comm_destroy", "frs_comm_allgather_i64",
    "frs_compare_device", "frs_compare",
    "frs_place_tiles_device", "frs_decode_tiles_window_device", "frs_decode_tiles_window",
    "frs_downsample2_device", "frs_downsample2",
    "frs_resample_window_device", "frs_resample_window",
    "frs_downsample2_nodata_device", "frs_downsample2_nodata",
    "frs_resample_window_nodata_device", "frs_resample_window_nodata",
    "frs_band_stats_device", "frs_band_stats", "frs_band_histogram_device", "frs_band_histogram",
    "frs_render_window_device", "frs_render_window",
    "frs_render_shaded_window_device", "frs_render_shaded_window",
    "frs_render_composite_window_device", "frs_render_composite_window",
)

# enum frs_resample
RESAMPLE_NEAREST = 0
RESAMPLE_AVERAGE = 1
RESAMPLE_BILINEAR = 2  # frs_resample_window* only
RESAMPLE_CODES = {"nearest": RESAMPLE_NEAREST, "average": RESAMPLE_AVERAGE}
WINDOW_RESAMPLE_CODES = {"nearest": RESAMPLE_NEAREST, "bilinear": RESAMPLE_BILINEAR, "average": RESAMPLE_AVERAGE}

# launch constants of k_compare (csrc/frs_compare.hip: kCmpBlock, kCmpUnroll, kCmpMaxGroups): a work-group step covers
# COMPARE_BLOCK * COMPARE_UNROLL 16-byte vectors of each raster, and a band gets one work-group per step up to
# COMPARE_MAX_GROUPS // nbands, grid-striding beyond that
COMPARE_BLOCK = 256
COMPARE_UNROLL = 4
COMPARE_MAX_GROUPS = 2048


def compare_groups(count: int, nbands: int, itemsize: int) -> int:
    """Work-groups per band of a compare of `count` elements per band (compare_groups in csrc/frs_compare.hip)."""
    chunk = COMPARE_BLOCK * COMPARE_UNROLL * (16 // itemsize)
    return max(1, min(-(-count // chunk), max(1, COMPARE_MAX_GROUPS // nbands)))


# launch constants of k_band_stats / k_band_histogram (csrc/frs_stats.hip: kStBlock, kStUnroll, kStMaxGroups, kHistBlock,
# kHistUnroll, kHistMaxGroups, kHistMaxBins, kHistCopyBins): a work-group step covers BLOCK * UNROLL 16-byte windows, a
# band gets one work-group per step up to MAX_GROUPS // nbands, grid-striding beyond that
STATS_BLOCK = 256
STATS_UNROLL = 4
STATS_MAX_GROUPS = 2048
HIST_BLOCK = 512
HIST_UNROLL = 4
HIST_MAX_GROUPS = 1024
HIST_MAX_BINS = 16384
HIST_COPY_BINS = 512


def stats_items(height: int, width: int, itemsize: int, dense: bool = True) -> int:
    """16-byte windows (work items) of one band (stats_items in csrc/frs_stats.h): a run of n elements can touch
    (n + 2 * ve - 2) // ve windows, ve = 16 // itemsize; a dense band is one run, any other one run per row."""
    ve = 16 // itemsize
    return (height * width + 2 * ve - 2) // ve if dense else height * ((width + 2 * ve - 2) // ve)


def stats_groups(items: int, nbands: int, block: int = STATS_BLOCK, unroll: int = STATS_UNROLL,
                 max_groups: int = STATS_MAX_GROUPS) -> int:
    """Work-groups per band of a statistics pass over `items` windows per band (stats_groups in csrc/frs_stats.hip)."""
    chunk = block * unroll
    return max(1, min(-(-items // chunk), max(1, max_groups // nbands)))


def encode_align_class(base_ptr: int, es: int, row_stride: int, band_stride: int, tile_w: int, nbands: int) -> int:
    """Alignment class of the level-5 fast encoders' row segments (mirrors align_class as fast_analyze in
    csrc/frs_encode.hip uses it): the widest of 16, 8, 4 bytes dividing the address of the first coded band's origin
    (`base_ptr`), the row stride and the tile width in bytes and, with more than one band, the band stride; 0 (the
    element gather) when none does.  Strides and tile width in elements of `es` bytes."""
    strides = [row_stride * es, tile_w * es] + ([band_stride * es] if nbands > 1 else [])
    for a in (16, 8, 4):
        if base_ptr % a == 0 and all(s % a == 0 for s in strides):
            return a
    return 0


class NativeUnavailable(RuntimeError):
    """The HIP library or a gfx950 device is missing (no CPU fallback exists)."""


class FrsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class EncodeDesc(ctypes.Structure):
    """frs_encode_desc"""
    _fields_ = [
        ("height", ctypes.c_int64), ("width", ctypes.c_int64),
        ("row_stride", ctypes.c_int64), ("band_stride", ctypes.c_int64),
        ("dtype", ctypes.c_int32), ("band0", ctypes.c_int32), ("nbands", ctypes.c_int32),
        ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
        ("blocksize", ctypes.c_int32), ("sample_rate", ctypes.c_int32),
        ("bits_per_sample", ctypes.c_int32), ("compression_level", ctypes.c_int32),
        ("norm_mode", ctypes.c_int32),
        ("tile_begin", ctypes.c_int64), ("tile_end", ctypes.c_int64),
    ]


class CompareDesc(ctypes.Structure):
    """frs_compare_desc"""
    _fields_ = [
        ("height", ctypes.c_int64), ("width", ctypes.c_int64),
        ("nbands", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("a_row_stride", ctypes.c_int64), ("a_band_stride", ctypes.c_int64),
        ("b_row_stride", ctypes.c_int64), ("b_band_stride", ctypes.c_int64),
    ]


class CompareBand(ctypes.Structure):
    """frs_compare_band"""
    _fields_ = [
        ("count", ctypes.c_int64), ("n_diff", ctypes.c_int64), ("first_diff", ctypes.c_int64),
        ("a_min", ctypes.c_double), ("a_max", ctypes.c_double), ("b_min", ctypes.c_double),
        ("b_max", ctypes.c_double), ("np_max_abs", ctypes.c_double), ("np_sum_abs", ctypes.c_double),
        ("np_sum_sq", ctypes.c_double), ("max_abs", ctypes.c_double), ("sum_abs", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class TileWindow(ctypes.Structure):
    """frs_tile_window: a tile's size and its position relative to the destination raster's origin"""
    _fields_ = [
        ("col_off", ctypes.c_int64), ("row_off", ctypes.c_int64),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
    ]


class RasterDesc(ctypes.Structure):
    """frs_raster_desc: a [nbands][height][width] destination raster with element strides"""
    _fields_ = [
        ("height", ctypes.c_int64), ("width", ctypes.c_int64),
        ("row_stride", ctypes.c_int64), ("band_stride", ctypes.c_int64),
        ("dtype", ctypes.c_int32), ("nbands", ctypes.c_int32),
    ]


class WindowMap(ctypes.Structure):
    """frs_window_map: the source rectangle in pixel-edge coordinates of the source buffer, and the fill value"""
    _fields_ = [
        ("x0", ctypes.c_double), ("y0", ctypes.c_double), ("width", ctypes.c_double), ("height", ctypes.c_double),
        ("fill", ctypes.c_double),
    ]


class BandStatsOut(ctypes.Structure):
    """frs_band_stats_out"""
    _fields_ = [
        ("n_valid", ctypes.c_int64), ("n_nodata", ctypes.c_int64), ("n_nan", ctypes.c_int64),
        ("min", ctypes.c_double), ("max", ctypes.c_double), ("sum", ctypes.c_double),
        ("isum_hi", ctypes.c_int64), ("isum_lo", ctypes.c_uint64),
        ("isq_hi", ctypes.c_uint64), ("isq_lo", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        """The fields, with the two 128-bit values joined into Python integers (isum, isq)."""
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["isum"] = (d.pop("isum_hi") << 64) + d.pop("isum_lo")
        d["isq"] = (d.pop("isq_hi") << 64) + d.pop("isq_lo")
        return d


class HistParams(ctypes.Structure):
    """frs_hist_params"""
    _fields_ = [("lo", ctypes.c_double), ("hi", ctypes.c_double), ("nbins", ctypes.c_int32),
                ("centre", ctypes.c_double)]


class BandHistOut(ctypes.Structure):
    """frs_band_hist_out"""
    _fields_ = [("below", ctypes.c_uint64), ("above", ctypes.c_uint64), ("m2", ctypes.c_double)]


class RenderParams(ctypes.Structure):
    """frs_render_params"""
    _fields_ = [("lo", ctypes.c_double), ("hi", ctypes.c_double), ("lut", ctypes.c_void_p), ("n", ctypes.c_int32),
                ("nodata_rgba", ctypes.c_uint32), ("channels", ctypes.c_int32)]


RENDER_MAX_LUT = 4096  # csrc/frs_render.h: kRenderMaxLut


class ShadeParams(ctypes.Structure):
    """frs_shade_params"""
    _fields_ = [("lx", ctypes.c_double), ("ly", ctypes.c_double), ("lz", ctypes.c_double), ("kx", ctypes.c_double),
                ("ky", ctypes.c_double), ("table", ctypes.c_void_p)]


class CompositeParams(ctypes.Structure):
    """frs_composite_params"""
    _fields_ = [("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("lut", ctypes.c_void_p),
                ("n", ctypes.c_int32), ("nodata_rgba", ctypes.c_uint32)]


def pack_rgba(rgba) -> int:
    """nodata_rgba as frs_render_params takes it: R | G << 8 | B << 16 | A << 24, from that integer or from (r, g, b, a)."""
    if isinstance(rgba, (int, np.integer)):
        v = int(rgba)
        if not 0 <= v <= 0xFFFFFFFF:
            raise ValueError("a packed rgba value must fit 32 bits")
        return v
    r, g, b, a = (int(x) for x in rgba)
    if any(not 0 <= x <= 255 for x in (r, g, b, a)):
        raise ValueError("rgba components must be 0..255")
    return r | g << 8 | b << 16 | a << 24


def tile_window_array(windows) -> ctypes.Array:
    """(TileWindow * n) from TileWindow structures or (col_off, row_off, width, height) rows."""
    if isinstance(windows, ctypes.Array) and windows._type_ is TileWindow:
        return windows
    ws = list(windows)
    arr = (TileWindow * max(len(ws), 1))()
    for i, w in enumerate(ws):
        arr[i] = w if isinstance(w, TileWindow) else TileWindow(int(w[0]), int(w[1]), int(w[2]), int(w[3]))
    arr._n = len(ws)
    return arr


_lib = None
_lib_lock = threading.Lock()


def load_library(path: Optional[os.PathLike] = None):
    """Load (once) and prototype the shared library.  Raises NativeUnavailable if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        # FRS_LIB_PATH: an alternative build of the same library (A/B experiments on one GPU box)
        p = Path(path) if path else Path(os.environ.get("FRS_LIB_PATH", str(LIB_PATH)))
        if not p.exists():
            raise NativeUnavailable(
                f"{p} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950)")
        L = ctypes.CDLL(str(p))
        i64, i32, vp, dp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
        ip64 = ctypes.POINTER(ctypes.c_int64)
        ctxp = ctypes.c_void_p
        L.frs_abi_version.restype = i32
        L.frs_abi_version.argtypes = []
        L.frs_device_count.restype = i32
        L.frs_device_count.argtypes = []
        L.frs_ctx_create.restype = i32
        L.frs_ctx_create.argtypes = [i32, ctypes.POINTER(ctxp)]
        L.frs_ctx_destroy.restype = None
        L.frs_ctx_destroy.argtypes = [ctxp]
        L.frs_last_error.restype = ctypes.c_char_p
        L.frs_last_error.argtypes = [ctxp]
        L.frs_encode_arena_bound.restype = i64
        L.frs_encode_arena_bound.argtypes = [ctypes.POINTER(EncodeDesc)]
        enc_args = [ctxp, ctypes.POINTER(EncodeDesc), vp, vp, i64, ip64, dp, dp, ctypes.POINTER(i32)]
        L.frs_encode_tiles_device.restype = i32
        L.frs_encode_tiles_device.argtypes = enc_args
        L.frs_encode_tiles.restype = i32
        L.frs_encode_tiles.argtypes = enc_args
        dec_args = [ctxp, vp, ip64, i32, i32, i32, i32, vp, ip64]
        L.frs_decode_frames_device.restype = i32
        L.frs_decode_frames_device.argtypes = dec_args
        L.frs_decode_frames.restype = i32
        L.frs_decode_frames.argtypes = dec_args
        dect_args = [ctxp, vp, ip64, i32, i32, i32, i32, ip64, dp, dp, i32, vp]
        L.frs_decode_tiles_device.restype = i32
        L.frs_decode_tiles_device.argtypes = dect_args
        L.frs_decode_tiles.restype = i32
        L.frs_decode_tiles.argtypes = dect_args
        L.frs_decode_tile_device.restype = i32
        L.frs_decode_tile_device.argtypes = [ctxp, vp, i64, i64, i64, i32, i32, i32, ctypes.c_double, ctypes.c_double,
                                             i32, vp]
        den_args = [ctxp, vp, i64, i32, ctypes.c_double, ctypes.c_double, i32, vp]
        L.frs_denormalize_device.restype = i32
        L.frs_denormalize_device.argtypes = den_args
        L.frs_denormalize.restype = i32
        L.frs_denormalize.argtypes = den_args
        L.frs_dev_malloc.restype = vp
        L.frs_dev_malloc.argtypes = [ctxp, i64]
        L.frs_dev_free.restype = None
        L.frs_dev_free.argtypes = [ctxp, vp]
        L.frs_host_malloc.restype = vp
        L.frs_host_malloc.argtypes = [ctxp, i64]
        L.frs_host_free.restype = None
        L.frs_host_free.argtypes = [ctxp, vp]
        L.frs_memcpy_h2d.restype = i32
        L.frs_memcpy_h2d.argtypes = [ctxp, vp, vp, i64]
        L.frs_memcpy_d2h.restype = i32
        L.frs_memcpy_d2h.argtypes = [ctxp, vp, vp, i64]
        L.frs_ctx_sync.restype = i32
        L.frs_ctx_sync.argtypes = [ctxp]
        L.frs_synth_raster_device.restype = i32
        L.frs_synth_raster_device.argtypes = [ctxp, vp, i32, i64, i64, i64, i64, ctypes.c_uint64]
        L.frs_ctx_stream.restype = vp
        L.frs_ctx_stream.argtypes = [ctxp]
        L.frs_profile_enable.restype = i32
        L.frs_profile_enable.argtypes = [ctxp, i32]
        L.frs_profile_avg_ms.restype = ctypes.c_double
        L.frs_profile_avg_ms.argtypes = [ctxp, ctypes.c_char_p]
        L.frs_profile_reset.restype = None
        L.frs_profile_reset.argtypes = [ctxp]
        L.frs_comm_unique_id.restype = i32
        L.frs_comm_unique_id.argtypes = [vp]
        L.frs_comm_init.restype = i32
        L.frs_comm_init.argtypes = [ctxp, vp, i32, i32, ctypes.POINTER(ctypes.c_void_p)]
        L.frs_comm_destroy.restype = None
        L.frs_comm_destroy.argtypes = [vp]
        L.frs_comm_allgather_i64.restype = i32
        L.frs_comm_allgather_i64.argtypes = [vp, ip64, i64, ip64]
        cmp_args = [ctxp, ctypes.POINTER(CompareDesc), vp, vp, ctypes.POINTER(CompareBand)]
        L.frs_compare_device.restype = i32
        L.frs_compare_device.argtypes = cmp_args
        L.frs_compare.restype = i32
        L.frs_compare.argtypes = cmp_args
        twp, rdp = ctypes.POINTER(TileWindow), ctypes.POINTER(RasterDesc)
        L.frs_place_tiles_device.restype = i32
        L.frs_place_tiles_device.argtypes = [ctxp, rdp, vp, ip64, twp, i32, vp]
        decw_args = [ctxp, vp, ip64, i32, i32, i32, twp, dp, dp, rdp, vp]
        L.frs_decode_tiles_window_device.restype = i32
        L.frs_decode_tiles_window_device.argtypes = decw_args
        L.frs_decode_tiles_window.restype = i32
        L.frs_decode_tiles_window.argtypes = decw_args
        ds_args = [ctxp, rdp, vp, rdp, vp, i32]
        L.frs_downsample2_device.restype = i32
        L.frs_downsample2_device.argtypes = ds_args
        L.frs_downsample2.restype = i32
        L.frs_downsample2.argtypes = ds_args
        rw_args = [ctxp, rdp, vp, rdp, vp, ctypes.POINTER(WindowMap), i32]
        L.frs_resample_window_device.restype = i32
        L.frs_resample_window_device.argtypes = rw_args
        L.frs_resample_window.restype = i32
        L.frs_resample_window.argtypes = rw_args
        for fn, args in ((L.frs_downsample2_nodata_device, ds_args), (L.frs_downsample2_nodata, ds_args),
                         (L.frs_resample_window_nodata_device, rw_args), (L.frs_resample_window_nodata, rw_args)):
            fn.restype = i32
            fn.argtypes = args + [ctypes.c_double]
        st_args = [ctxp, rdp, vp, dp, ctypes.POINTER(BandStatsOut)]
        hi_args = [ctxp, rdp, vp, dp, ctypes.POINTER(HistParams), ctypes.POINTER(ctypes.c_uint64),
                   ctypes.POINTER(BandHistOut)]
        for fn, args in ((L.frs_band_stats_device, st_args), (L.frs_band_stats, st_args),
                         (L.frs_band_histogram_device, hi_args), (L.frs_band_histogram, hi_args)):
            fn.restype = i32
            fn.argtypes = args
        rn_args = rw_args + [dp, ctypes.POINTER(RenderParams)]
        for fn in (L.frs_render_window_device, L.frs_render_window):
            fn.restype = i32
            fn.argtypes = rn_args
        for fn in (L.frs_render_shaded_window_device, L.frs_render_shaded_window):
            fn.restype = i32
            fn.argtypes = rn_args + [ctypes.POINTER(ShadeParams)]
        for fn in (L.frs_render_composite_window_device, L.frs_render_composite_window):
            fn.restype = i32
            fn.argtypes = rw_args + [dp, ctypes.POINTER(CompositeParams)]
        if L.frs_abi_version() != 1:
            raise NativeUnavailable("ABI version mismatch")
        if path is None:
            _lib = L
        return L


def device_count() -> int:
    return load_library().frs_device_count()


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _is_window_of(raster, desc) -> bool:
    """True when `raster` is a strided numpy view ([bands][rows][cols] or [rows][cols]) whose element strides are the
    descriptor's row_stride / band_stride: a window of a larger raster (cli.py:698-699, rasterio Window reads), passed
    to the C-ABI by its origin pointer without a contiguous copy."""
    if not isinstance(raster, np.ndarray) or raster.flags.c_contiguous or raster.ndim not in (2, 3):
        return False
    es = raster.dtype.itemsize
    st = raster.strides
    if st[-1] != es or any(x <= 0 or x % es for x in st):
        return False
    if st[-2] // es != desc.row_stride or raster.shape[-1] != desc.width or raster.shape[-2] != desc.height:
        return False
    return raster.ndim == 2 or (st[0] // es == desc.band_stride and raster.shape[0] >= desc.band0 + desc.nbands)


def _window_layout(r: np.ndarray):
    """(array, row_stride, band_stride) to hand a (bands, h, w) or (h, w) raster to frs_compare: the array itself with
    its element strides when it is C-contiguous or a window view of a larger raster (unit column stride, positive row
    and band strides that are whole elements, rows not overlapping), else a contiguous copy."""
    es = r.dtype.itemsize
    st = r.strides
    h, w = r.shape[-2], r.shape[-1]
    ok = st[-1] == es and all(x > 0 and x % es == 0 for x in st) and st[-2] // es >= w
    if not ok or r.flags.c_contiguous:
        r = np.ascontiguousarray(r)
        return r, w, h * w
    return r, st[-2] // es, (st[0] // es if r.ndim == 3 else (st[-2] // es) * h)


class DeviceBuffer:
    """A device allocation owned by a Context (freed with it or on close())."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.ptr = ctx.lib.frs_dev_malloc(ctx.handle, self.nbytes)
        if not self.ptr:
            raise FrsError(-2, ctx.last_error() or "device allocation failed")

    def upload(self, host: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(host)
        if offset + a.nbytes > self.nbytes:
            raise ValueError("upload exceeds buffer")
        self.ctx._check(self.ctx.lib.frs_memcpy_h2d(self.ctx.handle, self.ptr + offset, _p(a), a.nbytes))

    def download(self, nbytes: Optional[int] = None, offset: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
        n = self.nbytes - offset if nbytes is None else int(nbytes)
        dst = out if out is not None else np.empty(n, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.frs_memcpy_d2h(self.ctx.handle, _p(dst), self.ptr + offset, n))
        return dst

    def close(self):
        if self.ptr:
            self.ctx.lib.frs_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host memory (frs_host_malloc) the device can address: a decode target the kernels store straight
    into (no device buffer, no D2H copy).  `array` is its uint8 view; freed with close()."""

    def __init__(self, ctx: "Context", nbytes: int):
        # a weak reference: the context caches one HostBuffer (Context._pin), and a strong one would make a cycle that
        # keeps a dropped context's streams and device buffers alive until the cyclic GC runs
        self._ctx = weakref.ref(ctx)
        self.lib = ctx.lib
        self.nbytes = int(nbytes)
        self.ptr = ctx.lib.frs_host_malloc(ctx.handle, self.nbytes)
        if not self.ptr:
            raise FrsError(-2, ctx.last_error())  # FRS_E_HIP
        self.array = np.frombuffer((ctypes.c_uint8 * self.nbytes).from_address(self.ptr), dtype=np.uint8)

    @property
    def ctx(self):
        return self._ctx()

    def close(self):
        if self.ptr:
            self.array = None
            c = self._ctx()
            # a buffer that outlived its context is freed without one (frs_host_free accepts a null context)
            self.lib.frs_host_free(c.handle if c is not None and c.handle else None, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One frs_ctx (one device, one HIP stream).  Not shared between threads."""

    def __init__(self, device: int = 0, lib_path: Optional[os.PathLike] = None):
        self.lib = load_library(lib_path)
        if self.lib.frs_device_count() <= 0:
            raise NativeUnavailable("no gfx950 (MI355X) device visible to HIP")
        h = ctypes.c_void_p()
        rc = self.lib.frs_ctx_create(device, ctypes.byref(h))
        if rc != FRS_OK:
            raise NativeUnavailable(f"frs_ctx_create({device}) failed: {STATUS.get(rc, rc)}")
        self.handle = h
        self.device = device
        self._pin, self._pin_view = None, None  # reusable page-locked buffer, weakref to its last exported view

    def close(self):
        if getattr(self, "handle", None):
            self.release_pinned()
            self.lib.frs_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        m = self.lib.frs_last_error(self.handle)
        return m.decode() if m else ""

    def _check(self, rc: int):
        if rc != FRS_OK:
            raise FrsError(rc, self.last_error())

    # ---- memory
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def host_buffer(self, nbytes: int) -> HostBuffer:
        return HostBuffer(self, nbytes)

    def sync(self):
        self._check(self.lib.frs_ctx_sync(self.handle))

    def pinned(self, nbytes: int) -> np.ndarray:
        """uint8[nbytes] view of a page-locked host buffer (frs_host_malloc): the arena of a large host encode lands in
        it at DMA rate.  The returned array owns the buffer (it is freed when the last view of it dies), so a view
        handed out earlier is never invalidated.  The context keeps one buffer for reuse and hands it out again only
        while no earlier view of it is alive; a request it cannot serve gets a buffer of exactly its size."""
        nbytes = int(nbytes)
        hb = self._pin
        if hb is not None and (hb.nbytes < nbytes or (self._pin_view is not None and self._pin_view() is not None)):
            # too small, or still in use by an earlier result: the context lets go of it (live views keep it)
            self._pin, self._pin_view, hb = None, None, None
        if hb is None:
            hb = HostBuffer(self, nbytes)
            self._pin = hb
        view = (ctypes.c_uint8 * hb.nbytes).from_address(hb.ptr)
        view._owner = hb  # the array's base holds the buffer alive
        self._pin_view = weakref.ref(view)
        return np.frombuffer(view, dtype=np.uint8, count=nbytes)

    def release_pinned(self):
        """Drop the context's reusable page-locked buffer (views still alive keep theirs until they die)."""
        self._pin, self._pin_view = None, None

    # ---- encode
    @staticmethod
    def make_desc(height, width, dtype, *, row_stride=None, band_stride=None, band0=0, nbands=1,
                  tile_h=512, tile_w=512, sample_rate=44100, bits_per_sample=16, blocksize=4096,
                  compression_level=5, tile_begin=0, tile_end=None, norm_mode=0) -> EncodeDesc:
        d = EncodeDesc()
        d.height, d.width = int(height), int(width)
        d.row_stride = int(row_stride if row_stride is not None else width)
        d.band_stride = int(band_stride if band_stride is not None else d.row_stride * height)
        d.dtype = DTYPE_CODES[np.dtype(dtype)]
        d.band0, d.nbands = int(band0), int(nbands)
        d.tile_h, d.tile_w = int(tile_h), int(tile_w)
        d.blocksize, d.sample_rate = int(blocksize), int(sample_rate)
        d.bits_per_sample, d.compression_level = int(bits_per_sample), int(compression_level)
        d.norm_mode = int(norm_mode)
        ntiles = ((d.height + d.tile_h - 1) // d.tile_h) * ((d.width + d.tile_w - 1) // d.tile_w)
        d.tile_begin = int(tile_begin)
        d.tile_end = int(ntiles if tile_end is None else tile_end)
        return d

    def arena_bound(self, desc: EncodeDesc) -> int:
        return int(self.lib.frs_encode_arena_bound(ctypes.byref(desc)))

    def encode_tiles_host(self, raster: np.ndarray, desc: EncodeDesc, pinned: bool = False
                          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """Host-pointer encode.  Returns (arena uint8, tile_off int64[n+1], tile_min, tile_max, stream_bps).
        pinned=True: the arena is a view of the context's page-locked buffer (see pinned())."""
        r = raster if _is_window_of(raster, desc) else np.ascontiguousarray(raster)
        n = desc.tile_end - desc.tile_begin
        off = np.zeros(n + 1, dtype=np.int64)
        mn = np.zeros(max(n, 1), dtype=np.float64)
        mx = np.zeros(max(n, 1), dtype=np.float64)
        bps = ctypes.c_int32()
        cap = self.arena_bound(desc)
        arena = self.pinned(cap) if pinned else np.empty(cap, dtype=np.uint8)
        self._check(self.lib.frs_encode_tiles(
            self.handle, ctypes.byref(desc), _p(r), _p(arena), cap, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            mn.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mx.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            ctypes.byref(bps)))
        return arena[: off[n]], off, mn[:n], mx[:n], bps.value

    def encode_tiles_device(self, raster_ptr: int, desc: EncodeDesc, arena: DeviceBuffer):
        """Device-resident encode (bench path).  Returns (tile_off, tile_min, tile_max, stream_bps)."""
        n = desc.tile_end - desc.tile_begin
        off = np.zeros(n + 1, dtype=np.int64)
        mn = np.zeros(max(n, 1), dtype=np.float64)
        mx = np.zeros(max(n, 1), dtype=np.float64)
        bps = ctypes.c_int32()
        self._check(self.lib.frs_encode_tiles_device(
            self.handle, ctypes.byref(desc), ctypes.c_void_p(raster_ptr), ctypes.c_void_p(arena.ptr), arena.nbytes,
            off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), mn.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            mx.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(bps)))
        return off, mn[:n], mx[:n], bps.value

    # ---- decode
    def decode_frames_host(self, blob: bytes, stream_off: Sequence[int], pcm_counts: Sequence[int], channels: int,
                           bps: int, blocksize: int = 4096) -> np.ndarray:
        """Decode streams (frames only) -> int32 [sum(pcm_counts), channels]."""
        b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        b = np.ascontiguousarray(b)
        soff = np.ascontiguousarray(np.asarray(stream_off, dtype=np.int64))
        poff = np.zeros(len(pcm_counts) + 1, dtype=np.int64)
        poff[1:] = np.cumsum(np.asarray(pcm_counts, dtype=np.int64))
        out = np.empty((int(poff[-1]), channels), dtype=np.int32)
        self._check(self.lib.frs_decode_frames(
            self.handle, _p(b), soff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(pcm_counts), channels, bps,
            blocksize, _p(out), poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def decode_frames_device(self, blob: DeviceBuffer, stream_off: np.ndarray, pcm_counts: Sequence[int],
                             channels: int, bps: int, pcm: DeviceBuffer, blocksize: int = 4096) -> np.ndarray:
        soff = np.ascontiguousarray(np.asarray(stream_off, dtype=np.int64))
        poff = np.zeros(len(pcm_counts) + 1, dtype=np.int64)
        poff[1:] = np.cumsum(np.asarray(pcm_counts, dtype=np.int64))
        self._check(self.lib.frs_decode_frames_device(
            self.handle, ctypes.c_void_p(blob.ptr), soff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            len(pcm_counts), channels, bps, blocksize, ctypes.c_void_p(pcm.ptr),
            poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return poff

    def decode_tiles_host(self, blob, stream_off: Sequence[int], pcm_counts: Sequence[int], channels: int, bps: int,
                          data_min: Sequence[float], data_max: Sequence[float], dtype,
                          blocksize: int = 4096) -> np.ndarray:
        """Decode + de-normalise streams in one pass -> `dtype` [sum(pcm_counts), channels] (converter.py:241-282)."""
        b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        b = np.ascontiguousarray(b)
        soff = np.ascontiguousarray(np.asarray(stream_off, dtype=np.int64))
        poff = np.zeros(len(pcm_counts) + 1, dtype=np.int64)
        poff[1:] = np.cumsum(np.asarray(pcm_counts, dtype=np.int64))
        mn = np.ascontiguousarray(np.asarray(data_min, dtype=np.float64))
        mx = np.ascontiguousarray(np.asarray(data_max, dtype=np.float64))
        if len(mn) != len(pcm_counts) or len(mx) != len(pcm_counts) or len(soff) != len(pcm_counts) + 1:
            raise ValueError("one stream offset pair and one data_min/data_max per stream")
        out = np.empty((int(poff[-1]), channels), dtype=dtype)
        dp = ctypes.POINTER(ctypes.c_double)
        self._check(self.lib.frs_decode_tiles(
            self.handle, _p(b), soff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(pcm_counts), channels, bps,
            blocksize, poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), mn.ctypes.data_as(dp),
            mx.ctypes.data_as(dp), DTYPE_CODES[np.dtype(dtype)], _p(out)))
        return out

    def decode_tiles_device(self, blob: DeviceBuffer, stream_off: np.ndarray, pcm_counts: Sequence[int], channels: int,
                            bps: int, data_min: Sequence[float], data_max: Sequence[float], dtype, out,
                            blocksize: int = 4096, blob_ptr: Optional[int] = None) -> np.ndarray:
        """Device-resident fused decode into `out` (a DeviceBuffer, or a HostBuffer the kernels store straight into);
        returns the sample offsets (pcm_off)."""
        soff = np.ascontiguousarray(np.asarray(stream_off, dtype=np.int64))
        poff = np.zeros(len(pcm_counts) + 1, dtype=np.int64)
        poff[1:] = np.cumsum(np.asarray(pcm_counts, dtype=np.int64))
        mn = np.ascontiguousarray(np.asarray(data_min, dtype=np.float64))
        mx = np.ascontiguousarray(np.asarray(data_max, dtype=np.float64))
        if int(poff[-1]) * channels * np.dtype(dtype).itemsize > out.nbytes:
            raise ValueError("output buffer too small")
        dp = ctypes.POINTER(ctypes.c_double)
        self._check(self.lib.frs_decode_tiles_device(
            self.handle, ctypes.c_void_p(blob.ptr if blob_ptr is None else blob_ptr),
            soff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(pcm_counts), channels, bps, blocksize,
            poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), mn.ctypes.data_as(dp), mx.ctypes.data_as(dp),
            DTYPE_CODES[np.dtype(dtype)], ctypes.c_void_p(out.ptr)))
        return poff

    def decode_tile_device(self, blob, start: int, end: int, count: int, channels: int, bps: int, data_min: float,
                           data_max: float, dtype, out, blocksize: int = 4096) -> None:
        """decode_tiles_device for ONE stream (blob bytes [start, end), `count` samples per channel) -- the latency
        path of a bbox query: argument tables are this context's reused ctypes arrays (no numpy per call)."""
        dt = _DT_CACHE.get(dtype)
        if dt is None:
            dt = _DT_CACHE[dtype] = (np.dtype(dtype).itemsize, DTYPE_CODES[np.dtype(dtype)])
        if count * channels * dt[0] > out.nbytes:
            raise ValueError("output buffer too small")
        rc = self.lib.frs_decode_tile_device(self.handle, blob.ptr, int(start), int(end), int(count), channels, bps,
                                             blocksize, float(data_min), float(data_max), dt[1], out.ptr)
        if rc != FRS_OK:
            raise FrsError(rc, self.last_error())

    def denormalize_host(self, pcm: np.ndarray, data_min: float, data_max: float, dtype, pcm_bps: int = 16) -> np.ndarray:
        p = np.ascontiguousarray(pcm, dtype=np.int32)
        out = np.empty(p.shape, dtype=dtype)
        self._check(self.lib.frs_denormalize(self.handle, _p(p), p.size, int(pcm_bps), float(data_min), float(data_max),
                                             DTYPE_CODES[np.dtype(dtype)], _p(out)))
        return out

    def denormalize_device(self, pcm_ptr: int, n: int, data_min: float, data_max: float, dtype, out_ptr: int,
                           pcm_bps: int = 16):
        self._check(self.lib.frs_denormalize_device(self.handle, ctypes.c_void_p(pcm_ptr), int(n), int(pcm_bps),
                                                    float(data_min), float(data_max), DTYPE_CODES[np.dtype(dtype)],
                                                    ctypes.c_void_p(out_ptr)))

    # ---- compare
    @staticmethod
    def make_compare_desc(height, width, dtype, *, nbands=1, a_row_stride=None, a_band_stride=None,
                          b_row_stride=None, b_band_stride=None) -> CompareDesc:
        d = CompareDesc()
        d.height, d.width, d.nbands = int(height), int(width), int(nbands)
        d.dtype = DTYPE_CODES[np.dtype(dtype)]
        d.a_row_stride = int(width if a_row_stride is None else a_row_stride)
        d.b_row_stride = int(width if b_row_stride is None else b_row_stride)
        d.a_band_stride = int(d.a_row_stride * d.height if a_band_stride is None else a_band_stride)
        d.b_band_stride = int(d.b_row_stride * d.height if b_band_stride is None else b_band_stride)
        return d

    def compare_host(self, a: np.ndarray, b: np.ndarray, as_dicts: bool = True):
        """Difference statistics of two host rasters ((bands, h, w) or (h, w), same shape and dtype): one
        frs_compare_band per band, as dicts (or the CompareBand structures).  A strided window view of a larger
        raster is passed by its origin pointer and strides (as _is_window_of for the encoder); anything else that is
        not C-contiguous is copied first."""
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype != b.dtype or a.ndim not in (2, 3):
            raise ValueError("compare_host needs two (bands, h, w) or (h, w) arrays of one shape and dtype")
        if a.dtype not in DTYPE_CODES:
            raise ValueError(f"unsupported dtype {a.dtype}")
        if a.size == 0:
            raise ValueError("empty raster")
        a, ars, abs_ = _window_layout(a)
        b, brs, bbs = _window_layout(b)
        nb = a.shape[0] if a.ndim == 3 else 1
        d = self.make_compare_desc(a.shape[-2], a.shape[-1], a.dtype, nbands=nb, a_row_stride=ars, a_band_stride=abs_,
                                   b_row_stride=brs, b_band_stride=bbs)
        out = (CompareBand * nb)()
        self._check(self.lib.frs_compare(self.handle, ctypes.byref(d), _p(a), _p(b), out))
        return [x.as_dict() for x in out] if as_dicts else list(out)

    def compare_device(self, a_ptr: int, b_ptr: int, desc: CompareDesc, as_dicts: bool = True):
        """frs_compare_device on two device rasters laid out as `desc` says."""
        out = (CompareBand * max(int(desc.nbands), 1))()
        self._check(self.lib.frs_compare_device(self.handle, ctypes.byref(desc), ctypes.c_void_p(a_ptr),
                                                ctypes.c_void_p(b_ptr), out))
        return [x.as_dict() for x in out] if as_dicts else list(out)

    # ---- placement
    @staticmethod
    def make_raster_desc(height, width, dtype, *, nbands=1, row_stride=None, band_stride=None) -> RasterDesc:
        d = RasterDesc()
        d.height, d.width, d.nbands = int(height), int(width), int(nbands)
        d.dtype = DTYPE_CODES[np.dtype(dtype)]
        d.row_stride = int(width if row_stride is None else row_stride)
        d.band_stride = int(d.row_stride * d.height if band_stride is None else band_stride)
        return d

    def place_tiles_device(self, tiles_ptr: int, pcm_off: Sequence[int], windows, desc: RasterDesc, dst_ptr: int,
                           ntiles: Optional[int] = None) -> None:
        """frs_place_tiles_device: tile t (windows[t].width * height pixels of desc.nbands interleaved elements, from
        element pcm_off[t] * nbands of the device buffer at tiles_ptr) goes to its window of the device raster at
        dst_ptr, clipped to it.  Windows must not overlap inside the destination."""
        win = tile_window_array(windows)
        n = int(getattr(win, "_n", len(win)) if ntiles is None else ntiles)
        poff = np.ascontiguousarray(np.asarray(pcm_off, dtype=np.int64))
        if n > 0 and len(poff) < n:
            raise ValueError("one pcm_off per tile")
        self._check(self.lib.frs_place_tiles_device(
            self.handle, ctypes.byref(desc), ctypes.c_void_p(tiles_ptr),
            poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), win, n, ctypes.c_void_p(dst_ptr)))

    def _window_args(self, stream_off, windows, data_min, data_max):
        win = tile_window_array(windows)
        n = int(getattr(win, "_n", len(win)))
        soff = np.ascontiguousarray(np.asarray(stream_off, dtype=np.int64))
        mn = np.ascontiguousarray(np.asarray(data_min, dtype=np.float64))
        mx = np.ascontiguousarray(np.asarray(data_max, dtype=np.float64))
        if len(soff) != n + 1 or len(mn) != n or len(mx) != n:
            raise ValueError("one stream offset pair and one data_min/data_max per tile window")
        dp = ctypes.POINTER(ctypes.c_double)
        return win, n, soff, soff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), mn, mn.ctypes.data_as(dp), mx, \
            mx.ctypes.data_as(dp)

    def decode_tiles_window_device(self, blob, stream_off, windows, bps: int, data_min, data_max, dtype, dst,
                                   dst_shape, *, row_stride=None, band_stride=None, blocksize: int = 4096,
                                   blob_ptr: Optional[int] = None, dst_ptr: Optional[int] = None) -> RasterDesc:
        """frs_decode_tiles_window_device: stream s of the device blob is tile s; it is decoded, de-normalised to
        `dtype` and placed at windows[s] of the (bands, height, width) = dst_shape raster in the DeviceBuffer `dst`
        (element strides row_stride / band_stride, dense by default).  Returns the raster descriptor used."""
        nb, h, w = (int(x) for x in dst_shape)
        d = self.make_raster_desc(h, w, dtype, nbands=nb, row_stride=row_stride, band_stride=band_stride)
        need = ((nb - 1) * d.band_stride + (h - 1) * d.row_stride + w) * np.dtype(dtype).itemsize
        if dst_ptr is None and need > dst.nbytes:
            raise ValueError("destination buffer too small")
        win, n, soff, soff_p, mn, mn_p, mx, mx_p = self._window_args(stream_off, windows, data_min, data_max)
        self._check(self.lib.frs_decode_tiles_window_device(
            self.handle, ctypes.c_void_p(blob.ptr if blob_ptr is None else blob_ptr), soff_p, n, int(bps),
            int(blocksize), win, mn_p, mx_p, ctypes.byref(d), ctypes.c_void_p(dst.ptr if dst_ptr is None else dst_ptr)))
        return d

    def decode_tiles_window_host(self, blob, stream_off, windows, bps: int, data_min, data_max, dtype,
                                 dst_shape=None, out: Optional[np.ndarray] = None, blocksize: int = 4096) -> np.ndarray:
        """frs_decode_tiles_window: decode the tiles of the host blob into their windows of a (bands, height, width)
        raster.  `out` (C-contiguous, of `dtype`) is filled in place -- elements no tile covers keep their values -- or a
        zero-filled array of dst_shape is made and returned."""
        if out is None:
            out = np.zeros(tuple(int(x) for x in dst_shape), dtype=dtype)
        if out.ndim != 3 or not out.flags.c_contiguous or out.dtype != np.dtype(dtype) or not out.flags.writeable:
            raise ValueError("out must be a writeable C-contiguous (bands, height, width) array of `dtype`")
        if out.size == 0:
            raise ValueError("empty raster")
        b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        b = np.ascontiguousarray(b)
        nb, h, w = out.shape
        d = self.make_raster_desc(h, w, dtype, nbands=nb)
        win, n, soff, soff_p, mn, mn_p, mx, mx_p = self._window_args(stream_off, windows, data_min, data_max)
        self._check(self.lib.frs_decode_tiles_window(self.handle, _p(b), soff_p, n, int(bps), int(blocksize), win, mn_p,
                                                     mx_p, ctypes.byref(d), _p(out)))
        return out

    # ---- pyramid
    @staticmethod
    def _resample_code(mode) -> int:
        if isinstance(mode, str):
            if mode not in RESAMPLE_CODES:
                raise ValueError(f"resampling must be one of {sorted(RESAMPLE_CODES)}, got {mode!r}")
            return RESAMPLE_CODES[mode]
        return int(mode)

    def downsample2_device(self, src_ptr: int, src_desc: RasterDesc, dst_ptr: int, dst_desc: Optional[RasterDesc] = None,
                           mode="average", nodata=None) -> RasterDesc:
        """frs_downsample2_device: one 2x step from the device raster at src_ptr (laid out as src_desc) to the one at
        dst_ptr.  dst_desc defaults to the dense ceil(height/2) x ceil(width/2) raster.  `mode` is "average", "nearest"
        or an enum frs_resample value.  `nodata` (a number): frs_downsample2_nodata_device, the masked step.  Returns
        the destination descriptor."""
        if dst_desc is None:
            dst_desc = RasterDesc()
            dst_desc.height, dst_desc.width = (src_desc.height + 1) // 2, (src_desc.width + 1) // 2
            dst_desc.row_stride, dst_desc.band_stride = dst_desc.width, dst_desc.width * dst_desc.height
            dst_desc.dtype, dst_desc.nbands = src_desc.dtype, src_desc.nbands
        args = (self.handle, ctypes.byref(src_desc), ctypes.c_void_p(src_ptr), ctypes.byref(dst_desc),
                ctypes.c_void_p(dst_ptr), self._resample_code(mode))
        if nodata is None:
            self._check(self.lib.frs_downsample2_device(*args))
        else:
            self._check(self.lib.frs_downsample2_nodata_device(*args, float(nodata)))
        return dst_desc

    def downsample2_host(self, src: np.ndarray, mode="average", nodata=None) -> np.ndarray:
        """frs_downsample2 (frs_downsample2_nodata when `nodata` is a number) on a host raster ((bands, h, w) or
        (h, w)): the reduced raster, same rank and dtype."""
        a = np.ascontiguousarray(src)
        if a.ndim not in (2, 3) or a.dtype not in DTYPE_CODES or a.size == 0:
            raise ValueError("downsample2_host needs a non-empty (bands, h, w) or (h, w) array of a raster dtype")
        nb = a.shape[0] if a.ndim == 3 else 1
        h, w = a.shape[-2], a.shape[-1]
        sd = self.make_raster_desc(h, w, a.dtype, nbands=nb)
        dd = self.make_raster_desc((h + 1) // 2, (w + 1) // 2, a.dtype, nbands=nb)
        out = np.zeros(((nb,) if a.ndim == 3 else ()) + (dd.height, dd.width), dtype=a.dtype)
        args = (self.handle, ctypes.byref(sd), _p(a), ctypes.byref(dd), _p(out), self._resample_code(mode))
        if nodata is None:
            self._check(self.lib.frs_downsample2(*args))
        else:
            self._check(self.lib.frs_downsample2_nodata(*args, float(nodata)))
        return out

    # ---- windowed resample
    @staticmethod
    def _window_resample_code(mode) -> int:
        if isinstance(mode, str):
            if mode not in WINDOW_RESAMPLE_CODES:
                raise ValueError(f"resampling must be one of {list(WINDOW_RESAMPLE_CODES)}, got {mode!r}")
            return WINDOW_RESAMPLE_CODES[mode]
        return int(mode)

    @staticmethod
    def _window_map(rect, fill) -> WindowMap:
        if isinstance(rect, WindowMap):
            return rect
        x0, y0, width, height = (float(v) for v in rect)
        return WindowMap(x0, y0, width, height, float(fill))

    def resample_window_device(self, src_ptr: int, src_desc: RasterDesc, dst_ptr: int, dst_desc: RasterDesc, rect,
                               mode, fill=0, nodata=None) -> None:
        """frs_resample_window_device: the rectangle rect = (x0, y0, width, height), in pixel-edge coordinates of the
        device raster at src_ptr (laid out as src_desc), resampled onto the whole of the device raster at dst_ptr
        (dst_desc).  `mode` is "nearest", "bilinear", "average" or an enum frs_resample value; destination pixels the
        source does not cover get `fill`.  `rect` may be a WindowMap, which then carries its own fill.  `nodata` (a
        number): frs_resample_window_nodata_device, which keeps nodata pixels out of every output and gives `fill` to
        an output without valid weight."""
        m = self._window_map(rect, fill)
        args = (self.handle, ctypes.byref(src_desc), ctypes.c_void_p(src_ptr), ctypes.byref(dst_desc),
                ctypes.c_void_p(dst_ptr), ctypes.byref(m), self._window_resample_code(mode))
        if nodata is None:
            self._check(self.lib.frs_resample_window_device(*args))
        else:
            self._check(self.lib.frs_resample_window_nodata_device(*args, float(nodata)))

    def resample_window(self, a: np.ndarray, rect, out_shape, mode="average", fill=0, nodata=None) -> np.ndarray:
        """frs_resample_window (frs_resample_window_nodata when `nodata` is a number) on a host raster ((bands, H, W)
        or (H, W)): rect = (x0, y0, width, height) of it as an array of out_shape = (h, w) pixels per band, same rank
        and dtype."""
        a = np.ascontiguousarray(a)
        if a.ndim not in (2, 3) or a.dtype not in DTYPE_CODES or a.size == 0:
            raise ValueError("resample_window needs a non-empty (bands, H, W) or (H, W) array of a raster dtype")
        h, w = (int(v) for v in out_shape)
        nb = a.shape[0] if a.ndim == 3 else 1
        sd = self.make_raster_desc(a.shape[-2], a.shape[-1], a.dtype, nbands=nb)
        dd = self.make_raster_desc(h, w, a.dtype, nbands=nb)
        out = np.zeros(((nb,) if a.ndim == 3 else ()) + (max(h, 0), max(w, 0)), dtype=a.dtype)
        m = self._window_map(rect, fill)
        args = (self.handle, ctypes.byref(sd), _p(a), ctypes.byref(dd), _p(out), ctypes.byref(m),
                self._window_resample_code(mode))
        if nodata is None:
            self._check(self.lib.frs_resample_window(*args))
        else:
            self._check(self.lib.frs_resample_window_nodata(*args, float(nodata)))
        return out

    # ---- render
    @staticmethod
    def _render_params(lo, hi, lut, nodata_rgba, channels):
        """(RenderParams, the array its LUT pointer refers to).  `lut` is uint8 (n, 4); its length is the C-ABI's to
        judge, so that a caller sees the library's message."""
        t = np.ascontiguousarray(lut, dtype=np.uint8)
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError("the LUT must be a uint8 array of shape (n, 4)")
        return RenderParams(float(lo), float(hi), t.ctypes.data if t.size else None, int(t.shape[0]),
                            pack_rgba(nodata_rgba), int(channels)), t

    def render_window_device(self, src_ptr: int, src_desc: RasterDesc, dst_ptr: int, out_h: int, out_w: int, rect,
                             mode, lo: float, hi: float, lut, nodata_rgba=0, channels: int = 4, nodata=None,
                             dst_row_stride: Optional[int] = None) -> None:
        """frs_render_window_device: the rectangle rect = (x0, y0, width, height) of the one-band device raster at
        src_ptr (laid out as src_desc), resampled by `mode` onto out_h x out_w pixels and written as interleaved uint8
        [out_h][out_w][channels] at dst_ptr, rows dst_row_stride bytes apart (out_w * channels by default).  A value v
        becomes lut[index] with the bin rule of csrc/frs_render.h over [lo, hi]; `lut` is uint8 (n, 4) R, G, B, A,
        n <= 4096.  A pixel without data (outside the source, masked by `nodata`, or NaN) takes nodata_rgba, a packed
        integer (pack_rgba) or (r, g, b, a).  channels: 1 = R, 2 = R, A, 4 = R, G, B, A."""
        rp, keep = self._render_params(lo, hi, lut, nodata_rgba, channels)
        rs = int(out_w) * int(channels) if dst_row_stride is None else int(dst_row_stride)
        dd = self.make_raster_desc(out_h, out_w, np.uint8, row_stride=rs)
        m = self._window_map(rect, 0.0)
        self._check(self.lib.frs_render_window_device(
            self.handle, ctypes.byref(src_desc), ctypes.c_void_p(src_ptr), ctypes.byref(dd), ctypes.c_void_p(dst_ptr),
            ctypes.byref(m), self._window_resample_code(mode), self._nodata_arg(nodata), ctypes.byref(rp)))
        del keep

    def render_window(self, a: np.ndarray, rect, out_shape, mode, lo: float, hi: float, lut, nodata_rgba=0,
                      channels: int = 4, nodata=None) -> np.ndarray:
        """frs_render_window on a host raster (H, W): uint8 (h, w, channels) of out_shape = (h, w); see
        render_window_device."""
        a = np.ascontiguousarray(a)
        if a.ndim != 2 or a.dtype not in DTYPE_CODES or a.size == 0:
            raise ValueError("render_window needs a non-empty (H, W) array of a raster dtype")
        h, w = (int(v) for v in out_shape)
        rp, keep = self._render_params(lo, hi, lut, nodata_rgba, channels)
        sd = self.make_raster_desc(a.shape[0], a.shape[1], a.dtype)
        dd = self.make_raster_desc(h, w, np.uint8, row_stride=w * int(channels))
        out = np.zeros((max(h, 0), max(w, 0), max(int(channels), 0)), dtype=np.uint8)
        m = self._window_map(rect, 0.0)
        self._check(self.lib.frs_render_window(
            self.handle, ctypes.byref(sd), _p(a), ctypes.byref(dd), _p(out), ctypes.byref(m),
            self._window_resample_code(mode), self._nodata_arg(nodata), ctypes.byref(rp)))
        del keep
        return out

    # ---- hillshaded render
    @staticmethod
    def _shade_params(light, kx, ky, table):
        """(ShadeParams, the array its table pointer refers to).  `light` is (lx, ly, lz), `table` 256 uint8; what the
        five doubles may be is the C-ABI's to judge."""
        t = np.ascontiguousarray(table, dtype=np.uint8)
        if t.shape != (256,):
            raise ValueError("the shade table must be 256 uint8 values")
        lx, ly, lz = (float(v) for v in light)
        return ShadeParams(lx, ly, lz, float(kx), float(ky), t.ctypes.data), t

    def render_shaded_window_device(self, src_ptr: int, src_desc: RasterDesc, dst_ptr: int, out_h: int, out_w: int,
                                    rect, mode, lo: float, hi: float, lut, light, kx: float, ky: float, table,
                                    nodata_rgba=0, channels: int = 4, nodata=None,
                                    dst_row_stride: Optional[int] = None) -> None:
        """frs_render_shaded_window_device: render_window_device with hillshade (the definition in
        include/flac_raster_amd.h).  light = (lx, ly, lz) is the unit vector towards the light (render.light_vector),
        kx = z_factor / (8 cell_x) and ky = z_factor / (8 cell_y) for the ground size of an output pixel, `table` the
        256 uint8 multipliers of the shade levels (render.shade_table)."""
        rp, keep = self._render_params(lo, hi, lut, nodata_rgba, channels)
        sp, keep2 = self._shade_params(light, kx, ky, table)
        rs = int(out_w) * int(channels) if dst_row_stride is None else int(dst_row_stride)
        dd = self.make_raster_desc(out_h, out_w, np.uint8, row_stride=rs)
        m = self._window_map(rect, 0.0)
        self._check(self.lib.frs_render_shaded_window_device(
            self.handle, ctypes.byref(src_desc), ctypes.c_void_p(src_ptr), ctypes.byref(dd), ctypes.c_void_p(dst_ptr),
            ctypes.byref(m), self._window_resample_code(mode), self._nodata_arg(nodata), ctypes.byref(rp),
            ctypes.byref(sp)))
        del keep, keep2

    def render_shaded_window(self, a: np.ndarray, rect, out, mode, lo: float, hi: float, lut, light, kx: float,
                             ky: float, table, nodata_rgba=0, channels: int = 4, nodata=None,
                             dst_row_stride: Optional[int] = None, out_shape=None) -> np.ndarray:
        """frs_render_shaded_window on a host raster (H, W).  `out` is a shape (h, w) -- then a new uint8 (h, w,
        channels) is returned -- or a writable uint8 buffer that holds the destination [h][w * channels] at its start
        with rows dst_row_stride bytes apart (out_shape = (h, w) then): it is returned, padding as it was."""
        a = np.ascontiguousarray(a)
        if a.ndim != 2 or a.dtype not in DTYPE_CODES or a.size == 0:
            raise ValueError("render_shaded_window needs a non-empty (H, W) array of a raster dtype")
        if isinstance(out, np.ndarray):
            h, w = (int(v) for v in out_shape)
            if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("the destination buffer must be a writable contiguous uint8 array")
            rs = w * int(channels) if dst_row_stride is None else int(dst_row_stride)
            if out.size < (h - 1) * rs + w * int(channels):
                raise ValueError("the destination buffer is shorter than the destination")
        else:
            h, w = (int(v) for v in out)
            rs = w * int(channels)
            out = np.zeros((max(h, 0), max(w, 0), max(int(channels), 0)), dtype=np.uint8)
        rp, keep = self._render_params(lo, hi, lut, nodata_rgba, channels)
        sp, keep2 = self._shade_params(light, kx, ky, table)
        sd = self.make_raster_desc(a.shape[0], a.shape[1], a.dtype)
        dd = self.make_raster_desc(h, w, np.uint8, row_stride=rs)
        m = self._window_map(rect, 0.0)
        self._check(self.lib.frs_render_shaded_window(
            self.handle, ctypes.byref(sd), _p(a), ctypes.byref(dd), _p(out), ctypes.byref(m),
            self._window_resample_code(mode), self._nodata_arg(nodata), ctypes.byref(rp), ctypes.byref(sp)))
        del keep, keep2
        return out

    # ---- three-band composite
    @staticmethod
    def _composite_params(lo, hi, lut, nodata_rgba):
        """(CompositeParams, the array its LUT pointer refers to).  lo and hi are three numbers each (R, G, B); `lut` is
        uint8 (n, 4), its length the C-ABI's to judge."""
        t = np.ascontiguousarray(lut, dtype=np.uint8)
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError("the LUT must be a uint8 array of shape (n, 4)")
        lo3, hi3 = [float(v) for v in lo], [float(v) for v in hi]
        if len(lo3) != 3 or len(hi3) != 3:
            raise ValueError("a composite takes three lo and three hi values (R, G, B)")
        d3 = ctypes.c_double * 3
        return CompositeParams(d3(*lo3), d3(*hi3), t.ctypes.data if t.size else None, int(t.shape[0]),
                               pack_rgba(nodata_rgba)), t

    def render_composite_window_device(self, src_ptr: int, src_desc: RasterDesc, dst_ptr: int, out_h: int,
                                       out_w: int, rect, mode, lo, hi, lut, nodata_rgba=0, nodata=None,
                                       dst_row_stride: Optional[int] = None) -> None:
        """frs_render_composite_window_device: the rectangle rect = (x0, y0, width, height) of the three-band
        band-planar device raster at src_ptr (laid out as src_desc, nbands 3), resampled by `mode` onto out_h x out_w
        pixels and written as interleaved uint8 R, G, B, A at dst_ptr, rows dst_row_stride bytes apart (out_w * 4 by
        default).  Plane c gives channel c: its value is quantised over [lo[c], hi[c]] as render_window_device does
        and byte c of that LUT entry is stored; A is 255.  A pixel where any plane has no data takes nodata_rgba."""
        cp, keep = self._composite_params(lo, hi, lut, nodata_rgba)
        rs = int(out_w) * 4 if dst_row_stride is None else int(dst_row_stride)
        dd = self.make_raster_desc(out_h, out_w, np.uint8, row_stride=rs)
        m = self._window_map(rect, 0.0)
        self._check(self.lib.frs_render_composite_window_device(
            self.handle, ctypes.byref(src_desc), ctypes.c_void_p(src_ptr), ctypes.byref(dd), ctypes.c_void_p(dst_ptr),
            ctypes.byref(m), self._window_resample_code(mode), self._nodata_arg(nodata), ctypes.byref(cp)))
        del keep

    def render_composite_window(self, a: np.ndarray, rect, out_shape, mode, lo, hi, lut, nodata_rgba=0,
                                nodata=None) -> np.ndarray:
        """frs_render_composite_window on a host raster (3, H, W): uint8 (h, w, 4) of out_shape = (h, w); see
        render_composite_window_device."""
        a = np.ascontiguousarray(a)
        if a.ndim != 3 or a.dtype not in DTYPE_CODES or a.size == 0:
            raise ValueError("render_composite_window needs a non-empty (3, H, W) array of a raster dtype")
        h, w = (int(v) for v in out_shape)
        cp, keep = self._composite_params(lo, hi, lut, nodata_rgba)
        sd = self.make_raster_desc(a.shape[1], a.shape[2], a.dtype, nbands=a.shape[0])
        dd = self.make_raster_desc(h, w, np.uint8, row_stride=w * 4)
        out = np.zeros((max(h, 0), max(w, 0), 4), dtype=np.uint8)
        m = self._window_map(rect, 0.0)
        self._check(self.lib.frs_render_composite_window(
            self.handle, ctypes.byref(sd), _p(a), ctypes.byref(dd), _p(out), ctypes.byref(m),
            self._window_resample_code(mode), self._nodata_arg(nodata), ctypes.byref(cp)))
        del keep
        return out

    # ---- band statistics and histogram
    @staticmethod
    def _nodata_arg(nodata):
        return None if nodata is None else ctypes.byref(ctypes.c_double(float(nodata)))

    def _stats_host_layout(self, a):
        a = np.asarray(a)
        if a.ndim not in (2, 3) or a.dtype not in DTYPE_CODES or a.size == 0:
            raise ValueError("band statistics need a non-empty (bands, h, w) or (h, w) array of a raster dtype")
        a, rs, bs = _window_layout(a)
        nb = a.shape[0] if a.ndim == 3 else 1
        return a, self.make_raster_desc(a.shape[-2], a.shape[-1], a.dtype, nbands=nb, row_stride=rs, band_stride=bs)

    def band_stats_device(self, ptr: int, desc: RasterDesc, nodata=None, as_dicts: bool = True):
        """frs_band_stats_device on the device raster at `ptr`, laid out as `desc`: one frs_band_stats_out per band, as
        dicts (BandStatsOut.as_dict) or the structures.  `nodata` (a number) masks the pixels that hold it."""
        out = (BandStatsOut * max(int(desc.nbands), 1))()
        self._check(self.lib.frs_band_stats_device(self.handle, ctypes.byref(desc), ctypes.c_void_p(ptr),
                                                   self._nodata_arg(nodata), out))
        return [x.as_dict() for x in out] if as_dicts else list(out)

    def band_stats(self, a: np.ndarray, nodata=None, as_dicts: bool = True):
        """frs_band_stats on a host raster ((bands, h, w) or (h, w)).  A strided window view of a larger raster is
        passed by its origin pointer and strides; anything else that is not C-contiguous is copied first."""
        a, d = self._stats_host_layout(a)
        out = (BandStatsOut * d.nbands)()
        self._check(self.lib.frs_band_stats(self.handle, ctypes.byref(d), _p(a), self._nodata_arg(nodata), out))
        return [x.as_dict() for x in out] if as_dicts else list(out)

    def _hist_call(self, fn, desc, ptr, nodata, lo, hi, nbins, centre):
        nb, n = max(int(desc.nbands), 1), int(nbins)
        counts = np.zeros((nb, max(n, 1)), dtype=np.uint64)
        out = (BandHistOut * nb)()
        hp = HistParams(float(lo), float(hi), n, float(centre))
        self._check(fn(self.handle, ctypes.byref(desc), ptr, self._nodata_arg(nodata), ctypes.byref(hp),
                       counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out))
        return counts, [{"below": int(o.below), "above": int(o.above), "m2": float(o.m2)} for o in out]

    def band_histogram_device(self, ptr: int, desc: RasterDesc, lo: float, hi: float, nbins: int, nodata=None,
                              centre: float = 0.0):
        """frs_band_histogram_device: (counts uint64 [nbands][nbins], [{below, above, m2} per band]) of the device
        raster at `ptr` under the bin rule of csrc/frs_stats.h; m2 is the float dtypes' sum of (x - centre)^2."""
        return self._hist_call(self.lib.frs_band_histogram_device, desc, ctypes.c_void_p(ptr), nodata, lo, hi, nbins,
                               centre)

    def band_histogram(self, a: np.ndarray, lo: float, hi: float, nbins: int, nodata=None, centre: float = 0.0):
        """frs_band_histogram on a host raster ((bands, h, w) or (h, w)); see band_histogram_device and band_stats."""
        a, d = self._stats_host_layout(a)
        return self._hist_call(self.lib.frs_band_histogram, d, _p(a), nodata, lo, hi, nbins, centre)

    # ---- bench helpers
    def synth_raster(self, buf: DeviceBuffer, bands: int, height: int, width: int, row0: int = 0,
                     full_height: Optional[int] = None, seed: int = 1234):
        self._check(self.lib.frs_synth_raster_device(self.handle, ctypes.c_void_p(buf.ptr), bands, height, width, row0,
                                                     full_height if full_height is not None else height, seed))

    def profile(self, on: bool = True):
        self._check(self.lib.frs_profile_enable(self.handle, 1 if on else 0))

    def profile_avg_ms(self, kernel: str) -> float:
        return float(self.lib.frs_profile_avg_ms(self.handle, kernel.encode()))

    def profile_reset(self):
        self.lib.frs_profile_reset(self.handle)


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    """Process-wide context on device 0 (or $FRS_DEVICE / LOCAL_RANK)."""
    global _default_ctx
    if _default_ctx is None:
        dev = int(os.environ.get("FRS_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _default_ctx = Context(dev)
    return _default_ctx
