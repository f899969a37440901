"""A corpus of 4096-sample frames for the 32-bit stream encoder (rasters of dtype int32, uint32, float32, float64:
bits_per_sample 24, stream bps 32), each aimed at one coded form ("cell"), in the style of tests/encode_cells.py:
tests/test_wide_cells_host.py holds, with the oracle alone, that the oracle's output on the corpus reaches every cell
and names the frame that does; tests/test_gpu_wide_cells.py compares the GPU byte for byte with the oracle on the same
rasters and runs the oracle's streams through the wave decoder.

numpy only, seeded.  A recipe makes the int32 samples a frame is to have AFTER normalisation.  A float raster goes in
as trunc(x * 8388607) whatever the tile's extremes are, so a float64 x exists for every int32 target (`to_f64` finds
it: target / 8388607, nudged away from zero where the product falls short) and the float64 corpus normalises to the
recipes' own samples; the target INT32_MIN stands for a sample libFLAC receives as INT32_MIN, and is made by +-NaN,
+-inf, 257.0 and -300.0 in turn (x86's cvttsd2si gives INT32_MIN for all of them).  The float32 product has a 24-bit mantissa:
a float32 raster reaches only such samples (every |x| >= 32 carries at least 5 wasted bits), so the float32 corpus is
the float64 one rounded, compared whatever it reaches, before a few recipes stated in float32 itself (`F32_NAMED`).
The integer dtypes scale to +-8388607 by the tile's extremes; they get a 24-bit subset and one tile whose max - min
wraps.  `samples()` returns what a raster really normalises to.

Tiles are four frames (128 x 128, a frame = 32 rows).
"""
import functools

import numpy as np

from tests.encode_cells import alternate, ar, multisine, sine, stepped_noise, steps, walk, fixed_totals  # noqa: F401

FRAME = 4096
TILE = 128
RATE = 44100
SCALE = 8388607.0
MIN32 = -2 ** 31
S = 2 ** 31 - 1           # full scale
A30 = 2 ** 30
_SPECIALS = (np.nan, -np.nan, np.inf, -np.inf, 257.0, -300.0)     # (both signs of NaN)


def _rng(*seed):
    return np.random.default_rng([20261, *seed])


# ------------------------------------------------------------------------------------ targets -> float rasters
def to_f64(target):
    """float64 x with trunc(x * 8388607.0) == target sample for sample (INT32_MIN: the specials in turn)"""
    s = np.asarray(target, dtype=np.int64)
    assert s.min() >= MIN32 and s.max() <= S
    x = s / SCALE
    away = np.where(s < 0, -np.inf, np.inf)
    for _ in range(8):
        bad = np.flatnonzero((np.trunc(x * SCALE) != s) & (s != MIN32))
        if bad.size == 0:
            break
        x[bad] = np.nextafter(x[bad], away[bad])
    assert np.array_equal(np.trunc(x * SCALE)[s != MIN32], s[s != MIN32])
    sp = np.flatnonzero(s == MIN32)
    x[sp] = np.asarray(_SPECIALS)[np.arange(sp.size) % len(_SPECIALS)]
    return x


def to_f32(target):
    """the float32 nearest target / 8388607 (its sample is whatever the float32 product truncates to)"""
    with np.errstate(over="ignore"):
        return to_f64(target).astype(np.float32)


def samples(arr):
    """the int32 samples `arr` normalises to (its own extremes; float data does not depend on them)"""
    from oracle import oracle as O
    pcm, mn, mx, bps = O.normalize(np.ascontiguousarray(arr))
    assert bps == 32
    return pcm


# ------------------------------------------------------------------------------------------------------ recipes
def const(v):
    return lambda n: np.full(n, v, dtype=np.int64)


def noise(amp, seed=0):
    return lambda n: _rng(1, seed).integers(-amp, amp + 1, n)


def shl(base, w, odd_at=0):
    """base << w: exactly `w` wasted bits (sample `odd_at` of the base is made odd)"""
    def make(n):
        x = base(n).astype(np.int64).copy()
        x[odd_at] |= 1
        x = x << w
        assert x.min() > MIN32 and x.max() <= S
        return x
    return make


def put(base, at, values):
    """`base` with the given samples written at `at`, `at + 1`, ..."""
    def make(n):
        x = base(n).astype(np.int64).copy()
        x[at:at + len(values)] = values
        return x
    return make


def offset(base, off):
    return lambda n: base(n) + off


def bigwalk(order, seed):
    """noise summed `order` times at about 2^30: FIXED `order` is the exact predictor and an LPC's 15-bit coefficients
    cannot follow it"""
    return walk(1.0e8, seed, order=order, amp=float(A30))


def ar1_mixed(sign, t, seed=201):
    """x[i] = sign 0.52 x[i - 1] + e[i] at three quarters of full scale, plus white noise of deviation t: the noise
    pulls the order-1 predictor's coefficient towards 0, and t is set (by bisection over the oracle's output) so that
    it lands just inside +-0.5 -- shift 15, and the 15-bit code rounds to 16384, clamped to 16383, or to -16384"""
    def make(n):
        x = ar([sign * 0.52], 0.75 * S, seed)(n)
        return x + np.rint(t * _rng(90, seed).normal(0, 1, n)).astype(np.int64)
    return make


_THUE_MORSE = (1, -1, -1, 1, -1, 1, 1, -1)


def tie(k, events, hmax, seed, base=12345, spacing=9):
    """encode_cells.tie on wide samples: fixed totals k and k + 1 equal, non-zero and the smallest; h up to `hmax`
    (large: the totals pass 2^32), an odd constant added for k >= 1"""
    def make(n):
        rng = _rng(7, seed, k)
        span = spacing * (1 << k) + 8
        slots = rng.choice(np.arange(1, n // span - 1), events, replace=False) * span
        s = np.zeros(n, dtype=np.int64)
        for p in slots:
            h = int(rng.integers(1, hmax + 1)) * int(rng.choice([-1, 1]))
            for j in range(1 << k):
                s[p + spacing * j:p + spacing * j + 2] += h * _THUE_MORSE[j]
        x = s
        for _ in range(k):
            x = np.cumsum(x)
        return x + (base | 1 if k else 0)
    return make


_AR8 = [0.5, -0.4, 0.4, -0.3, 0.3, -0.3, 0.2, -0.2]
_AR4 = [1.1, -0.8, 0.5, -0.3]
_AR12 = [0.9, -0.7, 0.6, -0.6, 0.5, -0.5, 0.4, -0.4, 0.3, -0.3, 0.25, -0.2]
_W = (0, 4, 5, 7, 12)     # wasted bits on both sides of sbps 28


def _matrix():
    """VERBATIM, FIXED and LPC under each wasted-bits count of _W; the FIXED and LPC bases are the same for every w
    (w4_* and w5_* differ in nothing but the shift)"""
    out = []
    for w in _W:
        out += [(f"w{w}_verbatim", shl(noise(2 ** (31 - w) - 1, 40 + w), w)),
                (f"w{w}_walk", shl(walk(300.0, 50, amp=2.0 ** 17), w)),
                (f"w{w}_ar2", shl(ar([1.2, -0.6], 2.0 ** 18, 51), w))]
    return out


MONO = [
    # the types at their plainest
    ("noise_full", noise(S)), ("zeros", const(0)), ("const_w0", const(1234567)), ("const_w4", const(37 << 4)),
    ("const_w5", const(3 << 5)), ("const_w7", const(-5 << 7)), ("const_w12", const(77 << 12)),
    ("const_w28", const(3 << 28)), ("quiet", noise(40, 1)),
] + _matrix() + [
    ("w16_ar2", shl(ar([1.2, -0.6], 2.0 ** 14, 52), 16)), ("w9_noise", shl(noise(2 ** 12, 53), 9)),
    # fixed predictors on wide samples: orders 0..4, ties, totals past 2^32
    ("fixed0_big", noise(2 ** 26, 2)), ("walk_o1", bigwalk(1, 61)), ("walk_o2", bigwalk(2, 62)),
    ("walk_o3", bigwalk(3, 63)), ("walk_o4", bigwalk(4, 64)),
    ("tie_0_1", tie(0, 100, 2 ** 29, 1)), ("tie_1_2", tie(1, 60, 2 ** 16, 0)), ("tie_2_3", tie(2, 40, 2 ** 22, 0)),
    ("tie_3_4", tie(3, 20, 2 ** 18, 0)),
    # INT32_MIN samples and the limit_residual validity
    ("min_order1", put(offset(walk(300.0, 65, amp=2.0 ** 17), -A30), 2000, [-A30, -A30, MIN32, -A30, -A30])),
    ("only_order0", put(noise(1000, 3), 1000, [S, -S])),
    ("lpc_dropped", put(offset(sine(16, 1000.0), -5000), 3000, [MIN32])),
    ("lpc_dropped_verbatim", put(sine(900.5, float(A30)), 1001, [MIN32])),
    ("min_in_verbatim", put(put(put(noise(S, 4), 7, [MIN32]), 2048, [MIN32, MIN32, MIN32]), 4094, [MIN32, MIN32])),
    ("min_in_sine", put(sine(8, float(A30)), 1234, [MIN32])),
    ("min_under_w4", put(shl(noise(2 ** 20, 5), 4), 99, [MIN32])),
    ("min_under_w7", put(shl(noise(2 ** 20, 6), 7), 99, [MIN32, MIN32])),
    # LPC orders 1..8 (9..12 at level 8), shifts, coefficients at the ends of their code on full-scale samples
    ("ar1_0.12", ar([0.12], float(A30), 101)), ("ar1_0.5", ar([0.5], float(S), 1)), ("ar1_0.9", ar([0.9], float(S), 2)),
    ("ar2", ar([1.2, -0.6], float(S), 3)), ("ar3", ar([0.9, -0.5, 0.3], float(S), 4)), ("ar4", ar(_AR4, float(S), 5)),
    ("ar5", ar([0.8, -0.6, 0.5, -0.4, 0.3], float(A30), 6)),
    ("ar6", ar([0.7, -0.5, 0.4, -0.4, 0.3, -0.25], float(A30), 7)),
    ("ar7", ar([0.6, -0.5, 0.4, -0.4, 0.3, -0.3, 0.25], float(S), 8)), ("ar8", ar(_AR8, float(A30), 9)),
    ("ar9", ar(_AR12[:9], float(A30), 79)), ("ar10", ar(_AR12[:10], float(A30), 80)),
    ("ar11", ar(_AR12[:11], float(A30), 81)), ("ar12", ar(_AR12, float(A30), 10)),
    ("coef_top", ar1_mixed(1, 94947400.0)), ("coef_bottom", ar1_mixed(-1, 64042800.0)),
    ("multisine_12", multisine([150, 233, 347, 461, 590, 777], 1.5e8, 3.0e4, 1)),
    ("multisine_hi", multisine([150, 233, 347, 461], 4.0e8, 2.0e4, 2)),
    ("sine_3_full", sine(3, float(S))), ("alt_sine_3_full", alternate(sine(3, float(S)))),
    ("sine_45", sine(45, float(A30))), ("sine_200.5", sine(200.5, float(A30))),
    ("sine_900.5", sine(900.5, float(A30))), ("sine_1500.25", sine(1500.25, float(A30))),
    # residual coding: partition orders under FIXED and LPC, Rice parameters 0..30, both methods in one frame
    ("step_2048", stepped_noise(2048, 3.0e4, 64.0, float(A30))),
    ("step_1024", stepped_noise(1024, 2.0e3, 16.0, float(A30))),
    ("step_512", stepped_noise(512, 1.0e3, 4.0, float(A30))), ("step_256", stepped_noise(256, 40.0, 2.0, float(A30))),
    ("step_128", stepped_noise(128, 8.0, 1.6, float(A30))),
    ("step_mixed", stepped_noise(512, 60.0, 16.0, 2.0 ** 29)),
    ("ar2_step_2048", ar([1.2, -0.6], float(A30), 28, steps(2048, 1.0, 64.0))),
    ("ar2_step_1024", ar([1.2, -0.6], float(A30), 13, steps(1024, 1.0, 8.0))),
    ("ar2_step_512", ar([1.2, -0.6], float(A30), 14, steps(512, 1.0, 3.0))),
    ("ar2_step_256", ar([1.2, -0.6], float(A30), 15, steps(256, 1.0, 1.7))),
    ("ar2_step_128", ar([1.2, -0.6], float(S), 16, steps(128, 1.0, 1.3))),
    ("rice_15", noise(2 ** 16, 7)), ("rice_16", noise(2 ** 17, 8)), ("rice_20", noise(2 ** 21, 9)),
    ("rice_30", noise(int(1.1 * A30), 10)), ("rice_29", noise(int(0.55 * A30), 11)),
]


@functools.lru_cache(maxsize=None)
def frames():
    """[(name, target samples)]: the corpus in tile order, padded with constants to whole tiles"""
    out = [(name, rec(FRAME).astype(np.int64)) for name, rec in MONO]
    while len(out) % 4:
        out.append((f"const_pad{len(out) % 4}", np.full(FRAME, 4321 + 2 * len(out), dtype=np.int64)))
    assert len({n for n, _ in out}) == len(out)
    for _, x in out:
        x.setflags(write=False)
    return out


# recipes stated in float32 itself: (name, float32 values of a frame)
def _f32_named():
    n = FRAME
    t = np.arange(n)
    sine_m = (100.0 + 60.0 * np.sin(2 * np.pi * 5 * t / n)).astype(np.float32)      # metres, all in [32, 256)
    nan_in_sine, big_in_sine = sine_m.copy(), sine_m.copy()
    nan_in_sine[777] = np.nan
    neg_nan_in_sine = sine_m.copy()
    neg_nan_in_sine[3210] = -np.nan                                                  # (the sign bit set)
    inf_in_sine = sine_m.copy()
    inf_in_sine[5], inf_in_sine[4000] = np.inf, -np.inf
    ramp = (32 + (t * 224) // n).astype(np.float32)                                   # whole metres 32 .. 255
    big_in_sine[2001] = 300.0
    k32 = (32 * np.clip(np.rint(_rng(11).normal(0, 0.8, n)), -7, 7)).astype(np.float32)
    whole = np.rint(sine_m)
    return [("f32_const_32", np.full(n, 32.0, np.float32)), ("f32_const_33", np.full(n, 33.0, np.float32)),
            ("f32_const_96", np.full(n, 96.0, np.float32)), ("f32_const_16", np.full(n, 16.0, np.float32)),
            ("f32_zeros", np.zeros(n, np.float32)), ("f32_nan_in_sine", nan_in_sine),
            ("f32_big_in_sine", big_in_sine), ("f32_32k_noise", k32), ("f32_whole_metres", whole.astype(np.float32)),
            ("f32_sine_metres", sine_m), ("f32_unit_noise", _rng(12).uniform(-1, 1, n).astype(np.float32)),
            ("f32_const_neg_200", np.full(n, -200.0, np.float32)), ("f32_neg_nan_in_sine", neg_nan_in_sine),
            ("f32_inf_in_sine", inf_in_sine), ("f32_const_64", np.full(n, 64.0, np.float32)), ("f32_ramp_metres", ramp)]


F32_NAMED = [name for name, _ in _f32_named()]

# the 24-bit subset of the integer dtypes: (name, recipe within +-8388607, loud); a loud frame opens a tile and gets
# both extremes
_H24 = 8388607
INT_MONO = [
    ("i_noise_full", noise(_H24, 20), True), ("i_const", const(-1234567), False), ("i_quiet", noise(40, 21), False),
    ("i_sine_45", sine(45, 8.0e6), False),
    ("i_ar2", ar([1.2, -0.6], float(_H24), 22), True), ("i_walk", walk(3.0e3, 23, amp=8.0e6), False),
    ("i_step_512", stepped_noise(512, 30.0, 4.0, 8.0e6), False), ("i_ar8", ar(_AR8, 8.0e6, 24), False),
    ("i_sine_3", sine(3, float(_H24)), True), ("i_walk_o2", walk(40.0, 25, order=2, amp=8.0e6), False),
    ("i_alt_sine_3", alternate(sine(3, 8.0e6)), False), ("i_rice_15", noise(2 ** 16, 26), False),
]


@functools.lru_cache(maxsize=None)
def int_frames():
    loud = [(n, r(FRAME).astype(np.int64)) for n, r, l in INT_MONO if l]
    rest = [(n, r(FRAME).astype(np.int64)) for n, r, l in INT_MONO if not l]
    out = []
    for t, (name, x) in enumerate(loud):
        x = x.copy()
        x[np.argmax(x)], x[np.argmin(x)] = _H24, -_H24
        out += [(name, x)] + rest[3 * t:3 * t + 3]
    assert len(out) == len(INT_MONO)
    return out


def _rows(frames_raw, tile=TILE):
    return np.concatenate(frames_raw).reshape(-1, tile)


@functools.lru_cache(maxsize=None)
def mono_band(dtype="float64"):
    """The corpus as one band of 128 x 128 tiles stacked in one column.  float64: the recipes' samples; float32: the
    named float32 frames, then the corpus rounded to float32; int32 / uint32: the 24-bit subset at the top / bottom
    of the dtype's range, one constant tile (all samples 0) and one tile of random values whose max - min wraps."""
    if dtype == "float64":
        band = _rows([to_f64(x) for _, x in frames()])
    elif dtype == "float32":
        assert len(F32_NAMED) % 4 == 0
        band = _rows([v for _, v in _f32_named()] + [to_f32(x) for _, x in frames()])
    else:
        info = np.iinfo(dtype)
        base = info.max - 2 * _H24 if dtype == "int32" else 0
        fr = [(x + _H24 + base).astype(dtype) for _, x in int_frames()]
        fr += [np.full(FRAME, info.max - 5, dtype=dtype)] * 4
        rng = _rng(30, info.bits, int(info.min < 0))
        if dtype == "int32":
            over = rng.integers(-2 ** 30, 2 ** 30 + 6, 4 * FRAME)
            over[:2] = [-2 ** 30, 2 ** 30 + 5]
        else:
            over = rng.integers(0, 2 ** 32, 4 * FRAME)
            over[:2] = [0, 2 ** 32 - 1]
        fr.append(over.astype(dtype))
        band = _rows(fr)
    band.setflags(write=False)
    return band


def mono_names(dtype="float64"):
    if dtype == "float64":
        return [n for n, _ in frames()]
    if dtype == "float32":
        return F32_NAMED + [n for n, _ in frames()]
    return [n for n, _ in int_frames()] + [f"i_const_tile/{k}" for k in range(4)] + [f"i_wrap/{k}" for k in range(4)]


# ------------------------------------------------------------------------------------------------ two channels
def _pair_specials():
    """(name, left, right) in target samples: one pair per two-channel cell"""
    n = FRAME
    smooth = sine(16, 3.0e8)(n)
    small = noise(2 ** 12, 31)(n)
    e = np.rint(_rng(5, 1).normal(0, 2.0 ** 14, n)).astype(np.int64)
    full = noise(S // 2 * 2, 35)(n) // 2 * 2 + 1                                 # odd, over the whole range
    s25 = sine(16, 2.0 ** 24)(n)
    e25 = noise(2 ** 9, 36)(n)
    x0 = 2 * noise(2 ** 20, 34)(n)
    return [
        ("independent", sine(45, float(A30))(n), ar(_AR4, float(A30), 5)(n)),     # unrelated channels: code 1
        ("left_side", smooth, smooth + small),                                     # right = left + noise: code 8
        ("right_side", smooth + small, smooth),                                    # code 9
        ("mid_side", 2 * (smooth + e), 2 * (smooth - e)),                          # code 10, the side 4 e: w = 2
        ("side_lpc", smooth + ar([1.2, -0.6], 2.0 ** 20, 39)(n), smooth),             # the side under a predictor
        ("equal", ar([1.2, -0.6], float(A30), 14)(n), ar([1.2, -0.6], float(A30), 14)(n)),   # side 0 at 33 bits: FIXED 0
        # left over the whole range and odd, right = 1 - left: mid 0, side 2 left - 1 odd and beyond 32 bits --
        # VERBATIM at 33 bits
        ("side_33_verbatim", full, 1 - full),
        # side = 32 (2 e + 1): w = 5, sbps 28, limit_residual; side = 64 e: w = 6, sbps 27, the plain estimator
        ("side_w5", 32 * (s25 + e25 + 1), 32 * (s25 - e25)),
        ("side_w6", 32 * (s25 + e25), 32 * (s25 - e25)),
        ("side_w5_const", 32 * (s25 + 3), 32 * s25),                                # side 96 = 3 << 5: sbps 28, FIXED 1
        ("side_w6_const", 32 * (s25 + 6), 32 * s25),                                # side 192 = 3 << 6: sbps 27, CONSTANT
        ("side_min", put(const(-A30), 100, [MIN32])(n), put(const(A30), 100, [S])(n)),   # side -2^32 + 1 in a constant
        # right = 0, so side = left sample for sample; left is FIXED 0, no warm-up sample whose width differs:
        # independent and right-side cost the same, independent is kept
        ("fixed0_tie", x0, np.zeros(n, dtype=np.int64)),
        ("negated", smooth, -smooth),                                               # mid 0 or -1
        ("min_pair", put(noise(1000, 37), 50, [MIN32])(n), put(noise(1000, 38), 50, [MIN32])(n)),
    ]


_PAIRED = ("noise_full", "zeros", "const_w5", "w4_ar2", "w5_ar2", "w7_walk", "w12_verbatim", "walk_o3", "tie_1_2",
           "min_order1", "only_order0", "lpc_dropped", "min_in_verbatim", "ar8", "alt_sine_3_full", "step_mixed",
           "ar2_step_256", "rice_30", "w16_ar2", "sine_3_full")


@functools.lru_cache(maxsize=None)
def stereo_frames():
    """[(name, left, right)]: the special pairs, then some corpus frames beside one another"""
    by = dict(frames())
    return _pair_specials() + [(f"{a}|{b}", by[a], by[b]) for a, b in zip(_PAIRED, _PAIRED[1:] + _PAIRED[:1])]


def stereo_names():
    return [f"{n}/{ch}" for n, _, _ in stereo_frames() for ch in "LR"]


@functools.lru_cache(maxsize=None)
def stereo_raster():
    """float64 [2, frames * 32, 128]: one stream, frame f = the pair f"""
    sf = stereo_frames()
    arr = np.stack([_rows([to_f64(l) for _, l, _ in sf]), _rows([to_f64(r) for _, _, r in sf])])
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def multi_raster(bands=3):
    """float64 [bands, frames * 32, 128]: the corpus dealt over the channels, band b's frame f = frame f * bands + b"""
    fr = frames()
    nf = -(-len(fr) // bands)
    arr = np.stack([_rows([to_f64(fr[(f * bands + b) % len(fr)][1]) for f in range(nf)]) for b in range(bands)])
    arr.setflags(write=False)
    return arr


def multi_names(bands=3):
    fr = frames()
    nf = -(-len(fr) // bands)
    return [fr[(f * bands + b) % len(fr)][0] for f in range(nf) for b in range(bands)]


# ------------------------------------------------------------------------------------------- partial last frames
PTILE = 96          # 96 x 96 = two frames and a 1024-sample tail
TAIL = PTILE * PTILE - 2 * FRAME
TAILS = [
    ("const_w5", const(3 << 5)), ("const_w4", const(37 << 4)), ("zeros", const(0)),
    ("w5_ar2", shl(ar([1.2, -0.6], 2.0 ** 18, 51), 5)), ("w4_ar2", shl(ar([1.2, -0.6], 2.0 ** 18, 51), 4)),
    ("w7_walk", shl(walk(300.0, 50, amp=2.0 ** 17), 7)), ("w12_verbatim", shl(noise(2 ** 19 - 1, 41), 12)),
    ("noise_full", noise(S, 42)), ("walk_o3", bigwalk(3, 66)), ("sine_45", sine(45, float(A30))),
    ("step_128", stepped_noise(128, 2.0e3, 8.0, float(A30))), ("step_64", stepped_noise(64, 60.0, 3.0, float(A30))),
    ("min_in_sine", put(sine(8, float(A30)), 500, [MIN32])), ("rice_30", noise(int(1.1 * A30), 43)),
    ("alt_sine_3_full", alternate(sine(3, float(S)))),
]


@functools.lru_cache(maxsize=None)
def partial_frames():
    """[(name, samples)]: per 96 x 96 tile two corpus frames and a 1024-sample tail"""
    fr = frames()
    out = []
    for t, (name, rec) in enumerate(TAILS):
        out += [fr[(5 * t) % len(fr)], fr[(5 * t + 2) % len(fr)], (f"tail_{name}", rec(TAIL).astype(np.int64))]
    return out


@functools.lru_cache(maxsize=None)
def partial_band():
    band = np.concatenate([to_f64(x) for _, x in partial_frames()]).reshape(-1, PTILE)
    band.setflags(write=False)
    return band


# tiles of one row, a whole frame and a last frame of `tail` samples: 3 (VERBATIM whatever it holds) and 11
TINY = [("noise_full", noise(S, 44)), ("const_w5", const(3 << 5)), ("zeros", const(0)),
        ("w5_ar2", shl(ar([1.2, -0.6], 2.0 ** 18, 51), 5)), ("walk_o2", bigwalk(2, 67)),
        ("min_tail", lambda n: put(noise(1000, 45), n - 2, [MIN32])(n)), ("w7_walk", shl(walk(300.0, 50, amp=2.0 ** 17), 7)),
        ("const_w0", const(1234567))]


@functools.lru_cache(maxsize=None)
def tiny_band(tail):
    """float64 [8, 4096 + tail], tiles (1, 4096 + tail): row r is the recipe TINY[r] over a frame and a tail"""
    band = np.stack([to_f64(rec(FRAME + tail).astype(np.int64)) for _, rec in TINY])
    band.setflags(write=False)
    return band


def tiny_names():
    return [f"{n}{part}" for n, _ in TINY for part in ("", "/tail")]


# -------------------------------------------------------------------------------------- the oracle's references
@functools.lru_cache(maxsize=None)
def tiles_reference(kind="mono", dtype="float64", level=5):
    """(arena bytes, tile offsets, mins, maxs) of mono_band(dtype) ("mono"), partial_band() ("partial") or
    tiny_band(tail) ("tiny3", "tiny11")"""
    from oracle import oracle as O
    if kind == "mono":
        band, th, tw = mono_band(dtype), TILE, TILE
    elif kind == "partial":
        band, th, tw = partial_band(), PTILE, PTILE
    else:
        band = tiny_band(int(kind[4:]))
        th, tw = 1, band.shape[1]
    out, off, mins, maxs = b"", [0], [], []
    for r0 in range(0, band.shape[0], th):
        pcm, mn, mx, bps = O.normalize(np.ascontiguousarray(band[r0:r0 + th]).reshape(-1))
        assert bps == 32
        out += O.encode_frames(pcm, bps, RATE, level=level)
        off.append(len(out))
        mins.append(mn)
        maxs.append(mx)
    return out, off, mins, maxs


@functools.lru_cache(maxsize=None)
def stream_reference(bands, level=5):
    """(frames, pcm [N, bands], min, max) of stereo_raster() (bands 2) or multi_raster(bands)"""
    from oracle import oracle as O
    arr = stereo_raster() if bands == 2 else multi_raster(bands)
    pcm, mn, mx, bps = O.normalize(arr.transpose(1, 2, 0).reshape(-1, bands))
    assert bps == 32
    pcm.setflags(write=False)
    return O.encode_frames(pcm, bps, RATE, level=level), pcm, mn, mx


def census_of_tiles(ref, samples_per_tile, names):
    """the census of a tiles_reference, every subframe named after its corpus frame"""
    from oracle import oracle as O
    data, off = ref[0], ref[1]
    out = []
    for t in range(len(off) - 1):
        out += O.subframe_census(data[off[t]:off[t + 1]], 1, 32, samples_per_tile)
    assert len(out) == len(names), (len(out), len(names))
    for c, name in zip(out, names):
        c["name"] = name
    return out


def census_of_stream(frames_bytes, bands, nsamples, names):
    from oracle import oracle as O
    out = O.subframe_census(frames_bytes, bands, 32, nsamples)
    assert len(out) == len(names), (len(out), len(names))
    for c, name in zip(out, names):
        c["name"] = name
    return out


# -------------------------------------------------------------------------------------------------------- cells
def is_side(c):
    return (c["assignment"], c["channel"]) in ((8, 1), (9, 0), (10, 1))


def sbps_of(c):
    return 32 - c["wasted"] + (1 if is_side(c) else 0)


def wclass(w):
    """the wasted-bits counts the corpus is to reach on either side of sbps 28: 0 and 4; 5, 7 and 9 or more"""
    return w if w in (0, 4, 5, 7) else "9+" if w >= 9 else None


def cells_of(census):
    """{cell: name of the first subframe that reaches it}; a cell is a tuple, e.g. ("type", "FIXED 3"),
    ("kind at", "lpc", 5) (wasted-bits class), ("estimator", "plain", "constant"), ("porder", "lpc", 4),
    ("rice", 30), ("method", 0), ("rice mixed",), ("shift", 12), ("precision", 15), ("coef", "most positive"),
    ("assignment", 10), ("side", "verbatim"), ("side sbps", 27), ("tail", 1024, "fixed")"""
    got = {}
    for c in census:
        kind, name = c["kind"], c["name"]
        label = kind.upper() + (f" {c['order']}" if kind in ("fixed", "lpc") else "")
        sbps = sbps_of(c)
        reach = [("type", label), ("estimator", "plain" if sbps < 28 else "limit_residual", kind)]
        if wclass(c["wasted"]) is not None:
            reach.append(("kind at", kind, wclass(c["wasted"])))
        if kind in ("fixed", "lpc"):
            reach += [("porder", kind, c["porder"]), ("method", c["method"])]
            ks = [k for k in c["params"] if not isinstance(k, tuple)]
            reach += [("rice", k) for k in ks]
            reach += [("rice mixed",)] * (bool(ks) and min(ks) < 15 <= max(ks))
            reach += [("escape",)] * any(isinstance(k, tuple) for k in c["params"])
        if kind == "lpc":
            reach += [("shift", c["shift"]), ("precision", c["precision"])]
            lim = 1 << (c["precision"] - 1)
            reach += [("coef", "most positive")] * (max(c["coefs"]) == lim - 1)
            reach += [("coef", "most negative")] * (min(c["coefs"]) == -lim)
        if c["assignment"] >= 1 and c["blocksize"]:
            reach.append(("assignment", c["assignment"]))
        if is_side(c):
            reach += [("side", kind), ("side sbps", sbps)]
        if c["blocksize"] < FRAME:
            bs = c["blocksize"]
            reach.append(("tail", bs if bs > 16 else "5..16" if bs > 4 else "<=4", kind))
        for r in reach:
            got.setdefault(r, name)
    return got


def limit_residual_validity(x):
    """which of the orders 0..4 FLAC__fixed_compute_best_predictor_limit_residual keeps for the samples x: every
    k-th difference (from sample k on) at most INT32_MAX in magnitude"""
    d = np.asarray(x, dtype=np.int64)
    out = []
    for k in range(5):
        out.append(bool(np.abs(d).max() <= S))
        d = np.diff(d)
    return out


def lpc_sums(c, x):
    """the largest |sum q[j] x[i - 1 - j]| of the LPC subframe c over its (wasted-bits shifted) samples x"""
    x = np.asarray(x, dtype=np.int64) >> c["wasted"]
    o = c["order"]
    acc = np.zeros(len(x) - o, dtype=object)
    for j, q in enumerate(c["coefs"]):
        acc = acc + int(q) * x[o - 1 - j:len(x) - 1 - j].astype(object)
    return max(abs(int(v)) for v in acc)
