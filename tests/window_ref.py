"""numpy restatement of the windowed resample (csrc/frs_window_map.h, frs_resample_window*), written from the
definition and not from the C++: fp64 throughout, every numpy operation one IEEE operation, loops over taps, vectorised
over pixels.

The source rectangle (x0, y0, width, height) is in pixel-edge coordinates of the source (pixel i covers [i, i + 1)).
Per axis, N the source and n the destination extent: step = span / n, lo(j) = x0 + j step, hi(j) = x0 + (j + 1) step,
centre(j) = x0 + (j + 0.5) step.
  nearest    i = floor(centre), valid iff 0 <= i < N
  bilinear   valid iff 0 <= floor(centre) < N; u = centre - 0.5, i0 = floor(u), t = u - i0; taps i0, i0 + 1 clamped to
             [0, N - 1], weights 1 - t and t; (a (1 - tx) + b tx) (1 - ty) + (c (1 - tx) + d tx) ty
  average    clo = max(lo, 0), chi = min(hi, N), valid iff chi > clo; taps floor(clo) .. ceil(chi) - 1 with weight
             min(chi, i + 1) - max(clo, i); (sum_j wy_j (sum_i wx_i v_ij)) / ((chi_x - clo_x) (chi_y - clo_y)), sums
             ascending from 0.0
Integers round half to even, clamp, cast; float32 narrows; invalid pixels get fill by the same conversion."""
import numpy as np

MODES = ("nearest", "bilinear", "average")
DTYPES = (np.uint8, np.uint16, np.int16, np.int32, np.uint32, np.float32, np.float64)


def rects(W, H, w, h):
    """The test rectangles for a W x H source and a w x h destination: name -> (x0, y0, width, height)."""
    return {
        "scale_to_fit": (0.0, 0.0, float(W), float(H)),
        "exact_2x": (1.0, 2.0, 2.0 * w, 2.0 * h),
        "1.37x": (0.25, 0.6, 1.37 * w, 1.37 * h),
        "0.4x_upsampling": (3.3, 2.7, 0.4 * w, 0.4 * h),
        "9.3x": (-2.0, -1.5, 9.3 * w, 9.3 * h),
        "over_left_top": (-5.5, -3.25, 20.0, 20.0),
        "over_right_bottom": (W - 10.5, H - 8.25, 20.0, 20.0),
        "over_all_edges": (-3.0, -4.0, W + 7.5, H + 9.25),
        "outside_right": (W + 3.0, 0.0, 10.0, 10.0),
        "outside_up_left": (-20.0, -20.0, 10.0, 10.0),
        "lo_on_pixel_edges": (4.0, 6.0, 0.5 * w, 0.5 * h),
    }


def axis(x0, span, n, N):
    """lo, hi, centre of the n destination pixels of one axis"""
    x0, step = np.float64(x0), np.float64(span) / np.float64(n)
    j = np.arange(n, dtype=np.float64)
    return x0 + j * step, x0 + (j + 1.0) * step, x0 + (j + 0.5) * step


def nearest_axis(x0, span, n, N):
    """(i, valid); i is 0 where not valid"""
    f = np.floor(axis(x0, span, n, N)[2])
    valid = (f >= 0) & (f < N)
    return np.where(valid, f, 0).astype(np.int64), valid


def linear_axis(x0, span, n, N):
    """(i0, i1, t, valid): the clamped taps and the second tap's weight"""
    c = axis(x0, span, n, N)[2]
    f = np.floor(c)
    valid = (f >= 0) & (f < N)
    u = c - 0.5
    f0 = np.floor(u)
    i = np.where(valid, f0, 0).astype(np.int64)
    return np.clip(i, 0, N - 1), np.clip(i + 1, 0, N - 1), u - f0, valid


def area_axis(x0, span, n, N):
    """(clo, chi, i0, i1, valid): taps i0 .. i1 - 1 (0, 0 where not valid)"""
    lo, hi, _ = axis(x0, span, n, N)
    clo, chi = np.maximum(lo, 0.0), np.minimum(hi, np.float64(N))
    valid = chi > clo
    return (clo, chi, np.where(valid, np.floor(clo), 0).astype(np.int64),
            np.where(valid, np.ceil(chi), 0).astype(np.int64), valid)


def area_weight(clo, chi, i):
    i = np.asarray(i, dtype=np.float64)
    return np.minimum(chi, i + 1.0) - np.maximum(clo, i)


def to_dtype(v, dtype):
    """the result rule: integers round half to even, clamp, cast; float32 narrows; float64 as it is"""
    dtype = np.dtype(dtype)
    v = np.asarray(v, dtype=np.float64)
    if dtype.kind == "f":
        with np.errstate(over="ignore", invalid="ignore"):
            return v.astype(dtype)
    ii = np.iinfo(dtype)
    r = np.clip(np.rint(v), float(ii.min), float(ii.max))
    return r.astype(np.int64).astype(dtype)


def resample(src, rect, out_shape, mode, fill=0):
    """src (H, W) or (bands, H, W) -> the rectangle as out_shape = (h, w) pixels per band, same rank and dtype"""
    src = np.asarray(src)
    if src.ndim == 3:
        return np.stack([resample(b, rect, out_shape, mode, fill) for b in src])
    H, W = src.shape
    h, w = out_shape
    x0, y0, width, height = rect
    fillv = to_dtype(fill, src.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "nearest":
            ix, vx = nearest_axis(x0, width, w, W)
            iy, vy = nearest_axis(y0, height, h, H)
            valid = vy[:, None] & vx[None, :]
            return np.where(valid, src[iy[:, None], ix[None, :]], fillv).astype(src.dtype)
        if mode == "bilinear":
            x_0, x_1, tx, vx = linear_axis(x0, width, w, W)
            y_0, y_1, ty, vy = linear_axis(y0, height, h, H)
            valid = vy[:, None] & vx[None, :]
            a = src[y_0[:, None], x_0[None, :]].astype(np.float64)
            b = src[y_0[:, None], x_1[None, :]].astype(np.float64)
            c = src[y_1[:, None], x_0[None, :]].astype(np.float64)
            d = src[y_1[:, None], x_1[None, :]].astype(np.float64)
            tx, ty = tx[None, :], ty[:, None]
            val = (a * (1.0 - tx) + b * tx) * (1.0 - ty) + (c * (1.0 - tx) + d * tx) * ty
            return np.where(valid, to_dtype(val, src.dtype), fillv).astype(src.dtype)
        if mode != "average":
            raise ValueError(mode)
        xlo, xhi, xi0, xi1, vx = area_axis(x0, width, w, W)
        ylo, yhi, yi0, yi1, vy = area_axis(y0, height, h, H)
        valid = vy[:, None] & vx[None, :]
        total = np.zeros((h, w), dtype=np.float64)
        for dj in range(int((yi1 - yi0).max(initial=0))):
            j = yi0 + dj
            on_y = j < yi1
            jc = np.clip(j, 0, H - 1)
            row = np.zeros((h, w), dtype=np.float64)
            for di in range(int((xi1 - xi0).max(initial=0))):
                i = xi0 + di
                on_x = i < xi1
                v = src[jc[:, None], np.clip(i, 0, W - 1)[None, :]].astype(np.float64)
                row = np.where(on_x[None, :], row + area_weight(xlo, xhi, i)[None, :] * v, row)
            total = np.where(on_y[:, None], total + area_weight(ylo, yhi, j)[:, None] * row, total)
        with np.errstate(divide="ignore"):
            val = total / ((xhi - xlo)[None, :] * (yhi - ylo)[:, None])
        return np.where(valid, to_dtype(np.where(valid, val, 0.0), src.dtype), fillv).astype(src.dtype)
