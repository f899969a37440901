"""A minimal PNG writer for the render command: 8-bit greyscale, greyscale + alpha or RGBA, filter type 0 on every
row, one IDAT chunk.  zlib and struct only; no dependency is added."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOR_TYPES = {1: 0, 2: 4, 4: 6}  # channels -> PNG colour type


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(a: np.ndarray, level: int = 6) -> bytes:
    """The bytes of the PNG of a uint8 (H, W, C) array, C in {1, 2, 4} ((H, W) counts as C = 1)."""
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.dtype != np.uint8 or a.shape[2] not in COLOR_TYPES or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("a PNG is written from a non-empty uint8 (H, W, C) array with C in {1, 2, 4}")
    h, w, c = a.shape
    if h >= 2 ** 31 or w >= 2 ** 31:
        raise ValueError("a PNG's sides must be below 2^31")
    rows = np.zeros((h, 1 + w * c), dtype=np.uint8)  # filter type 0 in front of every row
    rows[:, 1:] = a.reshape(h, w * c)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, COLOR_TYPES[c], 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + \
        _chunk(b"IEND", b"")


def write_png(path, a: np.ndarray) -> None:
    """Write the uint8 (H, W, C) array `a`, C in {1, 2, 4}, as a PNG."""
    data = encode_png(a)
    with open(path, "wb") as f:
        f.write(data)
