"""The host side of the 8-bit render of a windowed read (extension: the reference has none).

The GPU kernel (csrc/frs_render.hip) maps a resampled value to a colour by one rule: an index into a look-up table
from the bin rule over [lo, hi], and the table's R, G, B, A bytes.  Everything a user chooses lives in those three
things, and this module makes them: `stretch_limits` gives (lo, hi) from a band's statistics, `build_lut` gives the
table from a colour ramp, a gamma and a transfer function.  Pure: no GPU, no dependency beyond numpy.
"""
from __future__ import annotations

import math
from fractions import Fraction
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .stats import percentile

MAX_LUT = 4096  # _native.RENDER_MAX_LUT
DEFAULT_STRETCH = "percentile:2,98"
TRANSFERS = ("linear", "log")

# Colour ramps: control points (t, r, g, b) with t ascending in [0, 1].  The values are this project's own choice.
COLORMAPS: Dict[str, List[Tuple]] = {
    "gray": [(0, 0, 0, 0), (1, 255, 255, 255)],
    "gray_r": [(0, 255, 255, 255), (1, 0, 0, 0)],
    "heat": [(0, 0, 0, 0), ("0.35", 176, 0, 0), ("0.65", 255, 120, 0), ("0.9", 255, 232, 80), (1, 255, 255, 255)],
    "terrain": [(0, 24, 92, 56), ("0.25", 96, 152, 72), ("0.5", 204, 192, 112), ("0.75", 144, 104, 72),
                ("0.9", 200, 200, 200), (1, 255, 255, 255)],
    "diverging": [(0, 32, 64, 152), ("0.5", 244, 244, 244), (1, 160, 32, 40)],
}


# ------------------------------------------------------------------------------------------------ stretch
def parse_stretch(spec: str) -> Tuple[str, Tuple[float, ...]]:
    """("minmax", ()), ("percentile", (p, q)), ("stddev", (k,)) or ("range", (lo, hi)) from "minmax",
    "percentile:p,q", "stddev:k" or "range:lo,hi"; ValueError for anything else."""
    kind, _, rest = str(spec).partition(":")
    try:
        args = tuple(float(x) for x in rest.split(",")) if rest else ()
    except ValueError:
        raise ValueError(f"--stretch: {spec!r} holds something that is not a number") from None
    if any(not math.isfinite(x) for x in args):
        raise ValueError(f"--stretch: the numbers of {spec!r} must be finite")
    if kind == "minmax" and not rest:
        return kind, ()
    if kind == "percentile" and len(args) == 2:
        if not 0 <= args[0] < args[1] <= 100:
            raise ValueError(f"--stretch percentile:p,q needs 0 <= p < q <= 100, got {spec!r}")
        return kind, args
    if kind == "stddev" and len(args) == 1:
        if not args[0] > 0:
            raise ValueError(f"--stretch stddev:k needs k > 0, got {spec!r}")
        return kind, args
    if kind == "range" and len(args) == 2:
        return kind, args
    raise ValueError(f"--stretch must be minmax, percentile:p,q, stddev:k or range:lo,hi; got {spec!r}")


def stretch_needs_statistics(spec: str) -> bool:
    return parse_stretch(spec)[0] != "range"


def stretch_limits(stats: Optional[Dict], spec: str = DEFAULT_STRETCH) -> Tuple[float, float]:
    """(lo, hi) of the stretch `spec` for a band whose statistics are `stats` (one entry of stats.band_statistics, or
    of an index's "statistics"; not looked at for range:lo,hi).
      minmax            the band's minimum and maximum (of a float band that holds +-inf: its histogram's range, the
                        finite values)
      percentile:p,q    stats.percentile of the band's histogram at p and q (the default is percentile:2,98)
      stddev:k          mean - k std and mean + k std, clipped to [min, max]
      range:lo,hi       the two numbers
    A result with hi <= lo becomes (lo, lo + 1); a band with no valid pixel gives (0, 1).  ValueError when the result is
    not finite (a float band whose mean is)."""
    kind, args = parse_stretch(spec)
    if kind == "range":
        lo, hi = args
    else:
        if stats is None:
            raise ValueError(f"the stretch {spec!r} needs the band's statistics")
        if not stats.get("valid") or stats.get("histogram") is None:
            return 0.0, 1.0
        h = stats["histogram"]
        if kind == "minmax":
            lo, hi = float(stats["min"]), float(stats["max"])
            if not math.isfinite(lo):
                lo = float(h["lo"])
            if not math.isfinite(hi):
                hi = float(h["hi"])
        elif kind == "percentile":
            lo, hi = float(percentile(h, Fraction(args[0]))), float(percentile(h, Fraction(args[1])))
        else:
            m, s = float(stats["mean"]), float(stats["std"])
            lo, hi = max(m - args[0] * s, float(stats["min"])), min(m + args[0] * s, float(stats["max"]))
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"the stretch {spec!r} gives limits that are not finite ({lo}, {hi}); use range:lo,hi")
    if hi <= lo:
        hi = lo + 1.0
    if not (hi > lo and math.isfinite(hi - lo)):
        raise ValueError(f"the stretch {spec!r} gives limits the render cannot use ({lo}, {hi})")
    return lo, hi


# ------------------------------------------------------------------------------------------------ colour ramps
def _frac(t) -> Fraction:
    """A control point's position, exactly: an int, a Fraction, a decimal string, or a float by its shortest decimal."""
    if isinstance(t, (int, Fraction)):
        return Fraction(t)
    return Fraction(t if isinstance(t, str) else repr(float(t)))


def check_colormap(points: Sequence[Sequence]) -> List[Tuple]:
    """Control points as (Fraction t, r, g, b, a), a defaulting to 255: at least two, t strictly ascending in [0, 1],
    components integers 0..255; ValueError otherwise."""
    out = []
    for p in points:
        if len(p) not in (4, 5):
            raise ValueError(f"a control point is t r g b [a], got {tuple(p)!r}")
        try:
            t = _frac(p[0])
        except (ValueError, ZeroDivisionError):
            raise ValueError(f"a control point's t must be a number, got {p[0]!r}") from None
        c = []
        for v in list(p[1:]) + [255] * (5 - len(p)):
            if isinstance(v, str):
                if not v.isdigit():
                    raise ValueError(f"a colour component must be an integer 0..255, got {v!r}")
                v = int(v)
            if v != int(v) or not 0 <= int(v) <= 255:
                raise ValueError(f"a colour component must be an integer 0..255, got {v!r}")
            c.append(int(v))
        if not 0 <= t <= 1:
            raise ValueError(f"a control point's t must lie in [0, 1], got {p[0]!r}")
        if out and t <= out[-1][0]:
            raise ValueError("the control points' t must ascend strictly")
        out.append((t, *c))
    if len(out) < 2:
        raise ValueError("a colour ramp needs at least two control points")
    return out


def load_colormap(path) -> List[Tuple]:
    """The control points of a text file of `t r g b [a]` lines (t in [0, 1] ascending, components 0..255; blank lines
    and what follows a # are skipped), as check_colormap returns them."""
    points = []
    for line in Path(path).read_text().splitlines():
        fields = line.split("#", 1)[0].split()
        if fields:
            points.append(fields)
    return check_colormap(points)


def format_colormap(points: Sequence[Sequence]) -> str:
    """The text load_colormap reads back as the same control points."""
    lines = []
    for t, *c in check_colormap(points):
        lines.append(" ".join([str(t.numerator) if t.denominator == 1 else repr(t.numerator / t.denominator)]
                              + [str(v) for v in c]))
    return "\n".join(lines) + "\n"


def resolve_colormap(colormap) -> List[Tuple]:
    """A name of COLORMAPS, or a list of control points, checked."""
    if isinstance(colormap, str):
        if colormap not in COLORMAPS:
            raise ValueError(f"colormap must be one of {', '.join(COLORMAPS)} or a file; got {colormap!r}")
        return check_colormap(COLORMAPS[colormap])
    return check_colormap(colormap)


def _ramp(points: List[Tuple], u: Fraction) -> List[int]:
    """The ramp at u, per component: linear between the neighbouring control points in exact rational arithmetic, the
    end colours outside them, rounded half up."""
    if u <= points[0][0]:
        return list(points[0][1:])
    if u >= points[-1][0]:
        return list(points[-1][1:])
    k = max(i for i, p in enumerate(points) if p[0] <= u)
    (t0, *c0), (t1, *c1) = points[k], points[k + 1]
    f = (u - t0) / (t1 - t0)
    return [math.floor(a + (b - a) * f + Fraction(1, 2)) for a, b in zip(c0, c1)]


def transfer_value(t: Fraction, gamma: float = 1.0, transfer: str = "linear") -> Fraction:
    """g(t): t ** (1 / gamma), or log1p(99 t) / log(100), as an exact rational (t itself for gamma 1, linear; else the
    double the expression gives, clamped to [0, 1])."""
    if transfer == "log":
        g = math.log1p(99.0 * float(t)) / math.log(100.0)
    elif gamma == 1.0:
        return t
    else:
        g = float(t) ** (1.0 / gamma)
    return Fraction(min(max(g, 0.0), 1.0))


def default_lut_size(gamma: float = 1.0, transfer: str = "linear") -> int:
    """256, or 4096 when a gamma or a logarithmic transfer bends the ramp (256 linear steps would band in the darks)."""
    return 256 if gamma == 1.0 and transfer == "linear" else MAX_LUT


def build_lut(colormap="gray", n: int = 256, gamma: float = 1.0, transfer: str = "linear") -> np.ndarray:
    """The look-up table of the render, uint8 (n, 4) R, G, B, A: entry i is the ramp at g(t_i), t_i = (i + 0.5) / n,
    interpolated in exact rational arithmetic and rounded half up.  g is t ** (1 / gamma) ("linear") or
    log1p(99 t) / log(100) ("log", which ignores gamma).  `colormap` is a name of COLORMAPS or a list of control
    points (t, r, g, b[, a]).  "gray" with gamma 1 and n = 256 is the identity ramp 0..255."""
    n = int(n)
    if not 1 <= n <= MAX_LUT:
        raise ValueError(f"the LUT length must be 1..{MAX_LUT}, got {n}")
    gamma = float(gamma)
    if not (math.isfinite(gamma) and gamma > 0):
        raise ValueError(f"gamma must be a finite number > 0, got {gamma}")
    if transfer not in TRANSFERS:
        raise ValueError(f"transfer must be one of {', '.join(TRANSFERS)}; got {transfer!r}")
    points = resolve_colormap(colormap)
    lut = np.empty((n, 4), dtype=np.uint8)
    for i in range(n):
        lut[i] = _ramp(points, transfer_value(Fraction(2 * i + 1, 2 * n), gamma, transfer))
    return lut


# ------------------------------------------------------------------------------------------------ hillshade
DEFAULT_HILLSHADE = (315.0, 45.0)  # azimuth clockwise from north, altitude; degrees


def light_vector(azimuth_deg: float = 315.0, altitude_deg: float = 45.0) -> Tuple[float, float, float]:
    """(lx, ly, lz), the unit vector towards the light: east, north, up = sin A cos h, cos A cos h, sin h for the
    azimuth A clockwise from north and the altitude h above the horizon, both in degrees.  The azimuth is any finite
    number, the altitude must lie in (0, 90]."""
    a, h = float(azimuth_deg), float(altitude_deg)
    if not math.isfinite(a):
        raise ValueError(f"the azimuth must be finite, got {azimuth_deg}")
    if not 0 < h <= 90:
        raise ValueError(f"the altitude must lie in (0, 90], got {altitude_deg}")
    a, h = math.radians(a), math.radians(h)
    return math.sin(a) * math.cos(h), math.cos(a) * math.cos(h), math.sin(h)


def shade_table(strength: float = 1.0) -> np.ndarray:
    """The 256 multipliers of the shade levels, uint8: m[k] = 255 (1 - strength + strength (k + 1/2) / 256), computed
    in exact rationals and rounded half to even.  strength in [0, 1]: 0 gives all 255 (no shading), 1 the full range."""
    if not (isinstance(strength, (int, float, Fraction)) and 0 <= strength <= 1):
        raise ValueError(f"the shade strength must lie in [0, 1], got {strength!r}")
    s = _frac(strength)
    return np.array([round(255 * (1 - s + s * Fraction(2 * k + 1, 512))) for k in range(256)], dtype=np.uint8)


def parse_hillshade(spec) -> Tuple[float, float]:
    """(azimuth, altitude) from "az,alt" in degrees, the altitude in (0, 90]; ValueError for anything else."""
    parts = str(spec).split(",")
    try:
        az, alt = (float(x) for x in parts)
    except ValueError:
        raise ValueError(f"--hillshade takes AZ,ALT in degrees, got {spec!r}") from None
    if not math.isfinite(az):
        raise ValueError(f"--hillshade: the azimuth must be finite, got {spec!r}")
    if not 0 < alt <= 90:
        raise ValueError(f"--hillshade: the altitude must lie in (0, 90], got {spec!r}")
    return az, alt


def shade_scales(cell_x: float, cell_y: float, z_factor: float = 1.0) -> Tuple[float, float]:
    """(kx, ky) = (z_factor / (8 cell_x), z_factor / (8 cell_y)) for the ground size of an output pixel."""
    cx, cy, z = float(cell_x), float(cell_y), float(z_factor)
    if not (math.isfinite(z) and z > 0):
        raise ValueError(f"the z-factor must be a finite number > 0, got {z_factor}")
    if not (cx > 0 and cy > 0):
        raise ValueError("the cell size must be positive")
    kx, ky = z / (8.0 * cx), z / (8.0 * cy)
    if not (math.isfinite(kx) and math.isfinite(ky)):
        raise ValueError("the z-factor over the cell size is not finite")
    return kx, ky


def max_size_shape(width: float, height: float, max_size: int) -> Tuple[int, int]:
    """(out_w, out_h) that keep the aspect ratio of a width x height box with the longer side max_size: the other is
    rounded (half up) and at least 1."""
    n = int(max_size)
    if n < 1:
        raise ValueError("--max-size must be >= 1")
    if not (width > 0 and height > 0):
        raise ValueError("the box must have a positive width and height")
    if width >= height:
        return n, max(1, math.floor(n * height / width + 0.5))
    return max(1, math.floor(n * width / height + 0.5)), n
