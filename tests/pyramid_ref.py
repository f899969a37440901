"""The pyramid step restated in numpy for the tests (csrc/frs_resample.h is the definition), and the pyramid of a
band built with it."""
import numpy as np


def np_downsample2(a: np.ndarray, mode: str) -> np.ndarray:
    """(C, H, W) -> (C, ceil(H/2), ceil(W/2)) by the definition: nearest takes (2r, 2x); the integer average is
    floor((2s + n) / (2n)) of the exact block sum; the float average ((a + b) + (c + d)) * 0.25, (a + b) * 0.5 or a,
    every operation in the dtype."""
    C, H, W = a.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    A = a[:, 0::2, 0::2]
    if mode == "nearest":
        return A.copy()
    hh, ww = H // 2, W // 2  # rows / columns of whole blocks
    B, Cc, D = a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]
    out = np.empty((C, h, w), dtype=a.dtype)
    if a.dtype.kind == "f":
        q, half = a.dtype.type(0.25), a.dtype.type(0.5)
        with np.errstate(all="ignore"):
            out[:, :hh, :ww] = ((A[:, :hh, :ww] + B[:, :hh, :]) + (Cc[:, :, :ww] + D)) * q
            out[:, hh:, :ww] = (A[:, hh:, :ww] + B[:, hh:, :]) * half      # the single last row: pairs along it
            out[:, :hh, ww:] = (A[:, :hh, ww:] + Cc[:, :, ww:]) * half     # the single last column: pairs down it
        out[:, hh:, ww:] = A[:, hh:, ww:]
    else:
        i = np.int64
        out[:, :hh, :ww] = (2 * (A[:, :hh, :ww].astype(i) + B[:, :hh, :] + Cc[:, :, :ww] + D) + 4) // 8
        out[:, hh:, :ww] = (2 * (A[:, hh:, :ww].astype(i) + B[:, hh:, :]) + 2) // 4
        out[:, :hh, ww:] = (2 * (A[:, :hh, ww:].astype(i) + Cc[:, :, ww:]) + 2) // 4
        out[:, hh:, ww:] = A[:, hh:, ww:]
    return out


def np_pyramid(band: np.ndarray, shapes, mode: str):
    """[band, level 1, level 2, ...] of an (H, W) band: level k from level k - 1, one level per entry of `shapes`
    (streaming.overview_shapes), whose sizes the levels must have."""
    out = [np.ascontiguousarray(band)]
    for h, w in shapes:
        out.append(np_downsample2(out[-1][None], mode)[0])
        assert out[-1].shape == (h, w)
    return out
