"""numpy restatement of the nodata-aware pyramid step and windowed resample (csrc/frs_nodata.h, frs_downsample2_nodata*,
frs_resample_window_nodata*), written from the definition and not from the C++: every numpy operation is one IEEE
operation, loops over taps, vectorised over pixels.

Predicate: a pixel is nodata iff it equals ndT = dtype(nd), or (floats) both are NaN; -0.0 == 0.0.
Masked 2x average: the m valid pixels of a block in the order a, b, c, d.  m = 0 -> ndT.  Integers:
floor((2s + m) / (2m)) of the exact sum, then the nudge (a result equal to ndT becomes ndT + 1, or ndT - 1 at the dtype's
maximum).  Floats: ((v1 + v2) + (v3 + v4)) * 0.25, ((v1 + v2) + v3) / 3, (v1 + v2) * 0.5, v1, in the dtype.  Nearest
copies (2r, 2x).
Masked windowed resample: indices, weights and validity from tests/window_ref.py.  nearest: a nodata tap gives fill.
bilinear: all four taps valid -> the unmasked expression; else num, den from 0.0 over the valid taps in the order 00, 01,
10, 11 with w00 = (1-tx)(1-ty), w01 = tx(1-ty), w10 = (1-tx)ty, w11 = tx ty; den == 0 -> fill, else num / den.  average:
row = row + wx v, roww = roww + wx over the valid taps of a row, then sum = sum + wy row, wsum = wsum + wy roww; no tap
nodata -> the unmasked value; else wsum == 0 -> fill, else sum / wsum.  Integer results: window_ref.to_dtype and the
nudge."""
import numpy as np

from tests import window_ref as R


def nodata_mask(a, nd):
    a = np.asarray(a)
    ndt = a.dtype.type(nd)
    with np.errstate(invalid="ignore"):
        m = a == ndt
    if a.dtype.kind == "f" and np.isnan(ndt):
        m = m | np.isnan(a)
    return m


def nudge(r, nd, dtype):
    """integer results computed from valid pixels, as int64: ndT -> ndT + 1 (ndT - 1 when ndT is the maximum)"""
    ndt = int(nd)
    other = ndt - 1 if ndt == np.iinfo(dtype).max else ndt + 1
    return np.where(r == ndt, other, r)


def np_downsample2_nodata(a: np.ndarray, mode: str, nd) -> np.ndarray:
    """(C, H, W) -> (C, ceil(H/2), ceil(W/2)); see the module docstring"""
    C, H, W = a.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    if mode == "nearest":
        return a[:, 0::2, 0::2].copy()
    dt = a.dtype
    ndt = dt.type(nd)
    # the four positions of every block, padded to whole blocks; `exists` is False in the padding
    pad = np.zeros((C, 2 * h, 2 * w), dtype=dt)
    pad[:, :H, :W] = a
    exists = np.zeros((C, 2 * h, 2 * w), dtype=bool)
    exists[:, :H, :W] = True
    ok = exists & ~nodata_mask(pad, nd)
    pos = [(0, 0), (0, 1), (1, 0), (1, 1)]  # a, b, c, d
    vals = [pad[:, r::2, c::2] for r, c in pos]
    oks = [ok[:, r::2, c::2] for r, c in pos]
    m = sum(o.astype(np.int64) for o in oks)
    out = np.empty((C, h, w), dtype=dt)
    if dt.kind != "f":
        s = sum(np.where(o, v.astype(np.int64), 0) for v, o in zip(vals, oks))
        mm = np.maximum(m, 1)
        q = (2 * s + mm) // (2 * mm)  # numpy's // on int64 is the floor division
        out[...] = np.where(m == 0, int(ndt), nudge(q, ndt, dt)).astype(dt)
        return out
    # floats: the valid values compacted in order, then the expression of m
    v = np.zeros((4, C, h, w), dtype=dt)
    cnt = np.zeros((C, h, w), dtype=np.int64)
    for val, o in zip(vals, oks):
        for k in range(4):
            sel = o & (cnt == k)
            v[k][sel] = val[sel]
        cnt = cnt + o
    with np.errstate(all="ignore"):
        e4 = ((v[0] + v[1]) + (v[2] + v[3])) * dt.type(0.25)
        e3 = ((v[0] + v[1]) + v[2]) / dt.type(3)
        e2 = (v[0] + v[1]) * dt.type(0.5)
    assert e4.dtype == dt and e3.dtype == dt and e2.dtype == dt
    out[...] = np.select([m == 0, m == 1, m == 2, m == 3], [np.full_like(e4, ndt), v[0], e2, e3], e4)
    return out


def np_pyramid_nodata(band: np.ndarray, shapes, mode: str, nd):
    """[band, level 1, level 2, ...] of an (H, W) band, level k from level k - 1 by the masked step"""
    out = [np.ascontiguousarray(band)]
    for h, w in shapes:
        out.append(np_downsample2_nodata(out[-1][None], mode, nd)[0])
        assert out[-1].shape == (h, w)
    return out


def _finish(val, weight_ok, src_dtype, fillv, nd):
    """to_dtype + nudge where the valid weight is above 0, fill elsewhere"""
    dt = np.dtype(src_dtype)
    r = R.to_dtype(np.where(weight_ok, val, 0.0), dt)
    if dt.kind != "f":
        r = nudge(r.astype(np.int64), dt.type(nd), dt).astype(dt)
    return np.where(weight_ok, r, fillv).astype(dt)


def bilinear_value(a, b, c, d, oa, ob, oc, od, tx, ty):
    """(value, valid weight above 0) of the masked bilinear form; fp64 arrays, broadcast"""
    with np.errstate(all="ignore"):
        full = (a * (1.0 - tx) + b * tx) * (1.0 - ty) + (c * (1.0 - tx) + d * tx) * ty
        w00, w01, w10, w11 = (1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty
        num = np.zeros(np.broadcast(a, tx, ty).shape, dtype=np.float64)
        den = np.zeros_like(num)
        for v, o, wgt in ((a, oa, w00), (b, ob, w01), (c, oc, w10), (d, od, w11)):
            num = np.where(o, num + wgt * v, num)
            den = np.where(o, den + wgt, den)
        allv = oa & ob & oc & od
        part = num / np.where(den == 0, 1.0, den)
    return np.where(allv, full, part), allv | (den != 0)


def area_value(v, ok, wx, wy, divisor):
    """(value, valid weight above 0) of the masked average form for N outputs with a fixed grid of taps: v and ok are
    (N, ny, nx) tap values and validity, wx (N, nx) and wy (N, ny) the weights, divisor (N,) the unmasked form's
    (chi_x - clo_x)(chi_y - clo_y); fp64"""
    n, ny, nx = v.shape
    total, wtotal = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(ny):
            row, roww = np.zeros(n), np.zeros(n)
            for i in range(nx):
                row = np.where(ok[:, j, i], row + wx[:, i] * v[:, j, i], row)
                roww = np.where(ok[:, j, i], roww + wx[:, i], roww)
            total = total + wy[:, j] * row
            wtotal = wtotal + wy[:, j] * roww
        masked = ~ok.reshape(n, -1).all(axis=1)
        part = total / np.where(wtotal == 0, 1.0, wtotal)
        full = total / divisor
    return np.where(masked, part, full), ~masked | (wtotal != 0)


def resample_nodata(src, rect, out_shape, mode, fill, nd):
    """src (H, W) or (bands, H, W) -> the rectangle as out_shape = (h, w) pixels per band, same rank and dtype"""
    src = np.asarray(src)
    if src.ndim == 3:
        return np.stack([resample_nodata(b, rect, out_shape, mode, fill, nd) for b in src])
    H, W = src.shape
    h, w = out_shape
    x0, y0, width, height = rect
    fillv = R.to_dtype(fill, src.dtype)
    bad = nodata_mask(src, nd)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "nearest":
            ix, vx = R.nearest_axis(x0, width, w, W)
            iy, vy = R.nearest_axis(y0, height, h, H)
            valid = vy[:, None] & vx[None, :] & ~bad[iy[:, None], ix[None, :]]
            return np.where(valid, src[iy[:, None], ix[None, :]], fillv).astype(src.dtype)
        if mode == "bilinear":
            x_0, x_1, tx, vx = R.linear_axis(x0, width, w, W)
            y_0, y_1, ty, vy = R.linear_axis(y0, height, h, H)
            inside = vy[:, None] & vx[None, :]
            idx = [(y_0[:, None], x_0[None, :]), (y_0[:, None], x_1[None, :]), (y_1[:, None], x_0[None, :]),
                   (y_1[:, None], x_1[None, :])]
            a, b, c, d = (src[i].astype(np.float64) for i in idx)
            oa, ob, oc, od = (~bad[i] for i in idx)
            val, wok = bilinear_value(a, b, c, d, oa, ob, oc, od, tx[None, :], ty[:, None])
            return _finish(val, inside & wok, src.dtype, fillv, nd)
        if mode != "average":
            raise ValueError(mode)
        xlo, xhi, xi0, xi1, vx = R.area_axis(x0, width, w, W)
        ylo, yhi, yi0, yi1, vy = R.area_axis(y0, height, h, H)
        inside = vy[:, None] & vx[None, :]
        total = np.zeros((h, w), dtype=np.float64)
        wtotal = np.zeros((h, w), dtype=np.float64)
        masked = np.zeros((h, w), dtype=bool)
        for dj in range(int((yi1 - yi0).max(initial=0))):
            j = yi0 + dj
            on_y = j < yi1
            jc = np.clip(j, 0, H - 1)
            row = np.zeros((h, w), dtype=np.float64)
            roww = np.zeros((h, w), dtype=np.float64)
            for di in range(int((xi1 - xi0).max(initial=0))):
                i = xi0 + di
                on = on_x = (i < xi1)[None, :] & on_y[:, None]
                ic = np.clip(i, 0, W - 1)
                v = src[jc[:, None], ic[None, :]].astype(np.float64)
                isbad = bad[jc[:, None], ic[None, :]]
                wx = R.area_weight(xlo, xhi, i)[None, :]
                row = np.where(on & ~isbad, row + wx * v, row)
                roww = np.where(on & ~isbad, roww + wx, roww)
                masked = masked | (on_x & isbad)
            wy = R.area_weight(ylo, yhi, j)[:, None]
            total = np.where(on_y[:, None], total + wy * row, total)
            wtotal = np.where(on_y[:, None], wtotal + wy * roww, wtotal)
        with np.errstate(divide="ignore"):
            full = total / ((xhi - xlo)[None, :] * (yhi - ylo)[:, None])
            part = total / np.where(wtotal == 0, 1.0, wtotal)
        val = np.where(masked, part, full)
        return _finish(val, inside & (~masked | (wtotal != 0)), src.dtype, fillv, nd)
