"""A corpus of 4096-sample frames, each aimed at one coded form ("cell") of a FLAC subframe, for the encoder tests:
tests/test_encode_cells_host.py holds, with the oracle alone, that the oracle's output on the corpus reaches every
cell and names the frame that does; tests/test_gpu_encode_cells.py compares every encode path of the GPU byte for byte
with the oracle on the same frames, and runs the oracle's streams through every decoder.

numpy only, seeded.  A recipe makes the 16-bit samples a frame is to have AFTER normalisation (`pcm`, within
+-32767).  The uint16 raster that normalises to them is found through the table of the normalisation itself: a tile
that holds 0 and 65534 maps a to about a - 32767, but the fp64 expression (converter.py:56-86) truncates 27 % of the
values to one less or more, and 319 values of the 65535 are never produced.  `to_u16` looks each sample up in the
table (the next producible value for the 319) and returns the samples the raster really normalises to: the
wasted-bits, tie and special two-channel frames need those to be the recipe's own, and `EXACT` / `_exact` hold it.

Tiles are four frames (128 x 128, a frame = 32 rows); frame 0 of every tile is a loud recipe with both extremes
forced into it (the anchors), so frames 1..3 may be anything.  The int16 and uint8 rasters are the uint16 one halved
and recentred / divided by 257: their normalisation gives other samples, which are compared whatever they reach.
"""
import functools

import numpy as np

FRAME = 4096
TILE = 128          # four frames
LO, HI = -32767, 32767
RATE = 44100


def _rng(*seed):
    return np.random.default_rng([20260, *seed])


# ----------------------------------------------------------------------------------- the normalisation's own table
@functools.lru_cache(maxsize=None)
def u16_table():
    """pcm of raw value a = 0..65534 in a tile whose extremes are 0 and 65534 (monotone, checked)"""
    from oracle import oracle as O
    pcm, mn, mx, bps = O.normalize(np.arange(65535, dtype=np.uint16))
    assert (mn, mx, bps) == (0.0, 65534.0, 16) and (np.diff(pcm) >= 0).all() and pcm[0] == LO and pcm[-1] == HI
    pcm.setflags(write=False)
    return pcm


def to_u16(pcm):
    """-> (raw uint16 samples, the pcm they normalise to)"""
    tab = u16_table()
    p = np.asarray(pcm, dtype=np.int64)
    assert p.min() >= LO and p.max() <= HI
    a = np.searchsorted(tab, p, side="left")
    return a.astype(np.uint16), tab[a].astype(np.int64)


# ------------------------------------------------------------------------------------------------------ recipes
def const(v):
    return lambda n: np.full(n, v, dtype=np.int64)


def noise(amp, seed=0):
    return lambda n: _rng(1, seed, amp).integers(-amp, amp + 1, n)


def sine(periods, amp=30000.0, phase=0.3):
    """a pure sine of `periods` per 4096 samples"""
    return lambda n: np.rint(amp * np.sin(2 * np.pi * periods * np.arange(n) / FRAME + phase)).astype(np.int64)


def ar(coefs, amp, seed=0, drive=None):
    """an autoregressive signal x[i] = sum c[j] x[i-1-j] + e[i], scaled to peak `amp`; drive(n) scales e over time"""
    def make(n):
        rng = _rng(2, seed, len(coefs))
        e = rng.normal(0, 1, n + 256)
        if drive is not None:
            e[256:] *= drive(n)
        x = np.zeros(n + 256)
        c = np.asarray(coefs, dtype=np.float64)
        o = len(c)
        for i in range(o, n + 256):
            x[i] = e[i] + np.dot(c, x[i - o:i][::-1])
        x = x[256:]
        return np.rint(x * (amp / np.abs(x).max())).astype(np.int64)
    return make


def steps(every, lo_amp=2.0, ratio=4.0):
    """the envelope of stepped noise: the amplitude multiplies by `ratio` every `every` samples"""
    return lambda n: lo_amp * ratio ** (np.arange(n) // every).astype(np.float64)


def stepped_noise(every, lo_amp=2.0, ratio=4.0, top=30000.0, seed=0):
    """white noise whose amplitude steps every `every` samples (FIXED 0, the partition order follows the step)"""
    def make(n):
        env = np.minimum(steps(every, lo_amp, ratio)(n), top)
        return np.rint(_rng(3, seed, every).uniform(-1, 1, n) * env).astype(np.int64)
    return make


def walk(step_amp, seed=0, order=1, drive=None, amp=30000.0):
    """noise summed `order` times (FIXED `order`), recentred; drive(n) scales the noise over time"""
    def make(n):
        e = _rng(4, seed, order).uniform(-1, 1, n) * step_amp
        if drive is not None:
            e = e * drive(n)
        x = e
        for _ in range(order):
            x = np.cumsum(x)
            x = x - np.linspace(x[0], x[-1], n)      # (no drift: the walk stays in range)
        x = x - (x.max() + x.min()) / 2
        if np.abs(x).max() > amp:
            x = x * (amp / np.abs(x).max())
        return np.rint(x).astype(np.int64)
    return make


def burst(base, at, length=16, level=HI):
    """`base` with an alternating full-scale burst: a few very large residuals in a smooth frame"""
    def make(n):
        x = base(n).copy()
        x[at:at + length:2], x[at + 1:at + length:2] = level, -level
        return x
    return make


def wasted(base, w, offset=0):
    """base << w (+ offset): `w` wasted bits when offset is 0"""
    def make(n):
        x = (base(n) << w) + offset
        assert x.min() >= LO and x.max() <= HI
        return x
    return make


def multisine(periods, amp, noise_sd=0.0, seed=0):
    """a sum of sines, optionally with a little noise: LPC with large coefficients (low shifts)"""
    def make(n):
        t = np.arange(n)
        x = sum(amp * np.sin(2 * np.pi * p * t / FRAME + i) for i, p in enumerate(periods))
        if noise_sd:
            x = x + _rng(9, seed).normal(0, noise_sd, n)
        return np.rint(x).astype(np.int64)
    return make


def alternate(base):
    """base * (-1)^i: the predictor's coefficients change sign (the most negative code)"""
    return lambda n: base(n) * np.where(np.arange(n) % 2, -1, 1)


def random_burst(base, at, length, seed=0):
    """`base` with `length` samples of +-full scale in random order: very large residuals in a smooth frame"""
    def make(n):
        x = base(n).copy()
        x[at:at + length] = np.where(_rng(8, seed).integers(0, 2, length) > 0, HI, LO)
        return x
    return make


_THUE_MORSE = (1, -1, -1, 1, -1, 1, 1, -1)


def tie(k, events, hmax, seed, spacing=9):
    """Fixed totals k and k + 1 equal, non-zero and the smallest: isolated pairs (h, h) in a zero signal have
    sum |s| = sum |diff s| = 2 |h| each, and the signal is that, summed k times; a pair is repeated with the signs
    + - - + ... (2^k of them, `spacing` apart) so that the k-fold sum returns to zero after each group.  For k >= 1 a
    constant is added (it changes total 0 alone) such that every sample survives the normalisation unchanged."""
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
        if k:
            mid = -int(x.max() + x.min()) // 2
            for off in range(mid | 1, mid + 4000, 2):     # (odd: no wasted bits)
                if np.array_equal(to_u16(x + off)[1], x + off):
                    return x + off
            raise AssertionError("no offset keeps the frame exact")
        return x
    return make


def fixed_totals(x):
    """libFLAC FLAC__fixed_compute_best_predictor's five totals: sum |k-th difference| over samples 4..n-1"""
    x = np.asarray(x, dtype=np.int64)
    out, d = [], x
    for k in range(5):
        out.append(int(np.abs(d[4 - k:]).sum()))
        d = np.diff(d)
    return out


# ------------------------------------------------------------------------------------------------- the corpus
_AR8 = [0.5, -0.4, 0.4, -0.3, 0.3, -0.3, 0.2, -0.2]
_AR4 = [1.1, -0.8, 0.5, -0.3]

# (name, recipe, loud): a loud recipe reaches about full scale and may open a tile (the two extremes are forced into
# it: its largest sample becomes 32767, its smallest -32767)
MONO = [
    # the types at their plainest
    ("noise_full", noise(HI), True), ("const_0", const(0), False), ("const_1235", const(1235), False),
    ("noise_40", noise(40), False),
    # pure sines: FIXED 2 / 3 / 4 with partition orders 0, 4 and 5; LPC at shift 9
    ("sine_3", sine(3, HI), True), ("sine_8", sine(8), False), ("sine_16", sine(16), False),
    ("sine_30", sine(30), False), ("sine_45", sine(45, HI), True), ("sine_70", sine(70), False),
    ("sine_110", sine(110), False), ("sine_200.5", sine(200.5), False), ("sine_1", sine(1, HI), True),
    ("sine_900.5", sine(900.5), False), ("sine_1500.25", sine(1500.25), False),
    # sums of sines: LPC order 8 with coefficients above 4 (shifts 7 and 8)
    ("multisine_hi", multisine([150, 233, 347, 461], 7000.0), False),
    ("multisine_hi_noise", multisine([150, 233, 347, 461], 7000.0, 3.0), False),
    ("multisine_lo", multisine([20, 33, 47, 61], 7000.0, 2.0), False),
    # an alternating sine: coefficients -2 and -1 at shift 10, the first at the most negative 12-bit code
    ("alt_sine_3", alternate(sine(3)), False), ("alt_sine_8", alternate(sine(8, 20000.0)), False),
    # stepped noise: FIXED 0 at partition orders 1..4, Rice parameters 0..14
    ("step_2048", stepped_noise(2048, 20.0, 64.0), False), ("step_2048_wide", stepped_noise(2048, 2.0, 4096.0), True),
    ("step_1024", stepped_noise(1024, 2.0, 16.0), False), ("step_512", stepped_noise(512, 1.0, 4.0), False),
    ("step_256", stepped_noise(256, 0.6, 2.0), True), ("step_128", stepped_noise(128, 0.6, 1.4), True),
    ("noise_12000", noise(12000), False),
    # walks: FIXED 1 and 2
    ("walk1", walk(60.0), False), ("walk1_quiet", walk(3.0, 1), False), ("walk2", walk(0.8, 2, order=2), False),
    # autoregressive signals: LPC orders 1..8, shifts 10..14
    ("ar1_0.12_a", ar([0.12], 20000.0, 101), False), ("ar1_0.12_b", ar([0.12], 20000.0, 102), False),
    ("ar1_0.12_c", ar([0.12], 20000.0, 103), False), ("ar1_0.2", ar([0.2], 20000.0, 11), False),
    ("ar1_0.35", ar([0.35], 20000.0, 111), False), ("ar1_0.5", ar([0.5], HI, 1), True),
    ("ar1_0.9", ar([0.9], HI, 2), True), ("ar2", ar([1.2, -0.6], HI, 3), True),
    ("ar3", ar([0.9, -0.5, 0.3], HI, 4), True), ("ar4", ar(_AR4, HI, 5), True),
    ("ar5", ar([0.8, -0.6, 0.5, -0.4, 0.3], 20000.0, 6), False),
    ("ar6", ar([0.7, -0.5, 0.4, -0.4, 0.3, -0.25], 20000.0, 7), False),
    ("ar7", ar([0.6, -0.5, 0.4, -0.4, 0.3, -0.3, 0.25], HI, 8), True), ("ar8", ar(_AR8, 20000.0, 9), False),
    # the driving noise steps: partition orders 1..5 under LPC 2 and under FIXED 1 / LPC 1 at the most positive code
    ("ar2_step_2048", ar([1.2, -0.6], 30000.0, 12, steps(2048, 1.0, 64.0)), False),
    ("ar2_step_1024", ar([1.2, -0.6], 30000.0, 13, steps(1024, 1.0, 8.0)), False),
    ("ar2_step_512", ar([1.2, -0.6], 30000.0, 14, steps(512, 1.0, 3.0)), False),
    ("ar2_step_256", ar([1.2, -0.6], 30000.0, 15, steps(256, 1.0, 1.7)), False),
    ("ar2_step_128", ar([1.2, -0.6], HI, 16, steps(128, 1.0, 1.3)), True),
    ("walk1_step_2048", walk(1.0, 3, drive=steps(2048, 1.0, 64.0)), False),
    ("walk1_step_1024", walk(1.0, 4, drive=steps(1024, 1.0, 8.0)), False),
    ("walk1_step_512", walk(1.0, 5, drive=steps(512, 1.0, 3.0)), False),
    # Rice parameter 14 in a smooth frame: full-scale samples in random order inside one 128-sample partition
    ("sine_8_burst", random_burst(sine(8), 1024, 128), True),
    ("sine_16_burst", random_burst(sine(16, 8000.0), 2048, 64, 1), True),
    ("walk1_burst", random_burst(walk(20.0, 6, amp=8000.0), 3072, 128, 2), True),
    ("sine_16_spike", burst(sine(16, 8000.0), 2222, 2), True),
    # wasted bits 1, 2, 3, 5, 6, 8, 10 and 12 under FIXED, LPC, CONSTANT and VERBATIM
    ("w1_sine_16", wasted(sine(16, 15000.0), 1), False), ("w2_sine_16", wasted(sine(16, 7000.0), 2), False),
    ("w3_ar2", wasted(ar([1.2, -0.6], 3000.0, 20), 3), False), ("w5_ar4", wasted(ar(_AR4, 900.0, 21), 5), False),
    ("w8_sine_45", wasted(sine(45, 120.0), 8), False), ("w12_walk", wasted(walk(0.4, 22, amp=7.0), 12), False),
    ("w8_ar2", wasted(ar([1.2, -0.6], 100.0, 23), 8), False), ("w4_const", const(37 << 4), False),
    ("w1_ar8", wasted(ar(_AR8, 15000.0, 24), 1), False), ("w1_const", const(-2222), False),
    ("w10_const", const(-3 << 10), False), ("w6_noise", wasted(noise(400, 25), 6), False),
    # fixed totals k and k + 1 tied at the minimum
    ("tie_0_1", tie(0, 100, 3001, 1), False), ("tie_1_2", tie(1, 60, 301, 0), False),
    ("tie_2_3", tie(2, 40, 21, 0), False), ("tie_3_4", tie(3, 20, 3, 0), False),
]
EXACT = [name for name, _, _ in MONO if name.startswith(("w", "tie_")) and not name.startswith("walk")]


def _anchored(x):
    x = x.copy()
    x[np.argmax(x)], x[np.argmin(x)] = HI, LO
    return x


@functools.lru_cache(maxsize=None)
def frames():
    """[(name, pcm)]: the corpus in tile order, four frames per tile, a loud frame with the anchors first in each"""
    made = [(name, rec(FRAME), loud) for name, rec, loud in MONO]
    ntiles = -(-len(made) // 4)
    loud = [m for m in made if m[2]]
    assert len(loud) >= ntiles, (len(loud), ntiles)
    rest = [m for m in made if not m[2]] + loud[ntiles:]
    out = []
    for t in range(ntiles):
        out.append((loud[t][0], _anchored(loud[t][1])))
        out += [(name, x) for name, x, _ in rest[3 * t:3 * t + 3]]
    while len(out) % 4:
        out.append((f"const_pad{len(out) % 4}", np.full(FRAME, 4321 + 2 * len(out), dtype=np.int64)))
    for _, x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mono_band(dtype="uint16", tile=TILE):
    """The corpus as one band of `tile` x `tile` tiles stacked in one column, in the named dtype.  uint16 normalises to
    the recipes' samples; int16 (halved and recentred: a range the dtype's own arithmetic does not wrap) and uint8
    (divided by 257) to coarser ones."""
    band = _column([x for _, x in frames()], dtype).reshape(-1, tile)
    band.setflags(write=False)
    return band


# ------------------------------------------------------------------------------------------------ two channels
def _named(name):
    return dict(frames())[name]


def _exact(*xs):
    """the samples, held to survive the normalisation unchanged (nearly all of the 319 lost values are odd)"""
    for x in xs:
        assert np.array_equal(to_u16(x)[1], x)
    return xs


def _pair_specials():
    """(name, left, right) in pcm: one pair per two-channel cell"""
    n = FRAME
    smooth = sine(16, 12000.0)(n)
    small = noise(40, 31)(n)
    e = _rng(5, 1).normal(0, 20, n).round().astype(np.int64)
    u, v = noise(4095, 32)(n), noise(4095, 33)(n)
    x0 = 2 * noise(150, 34)(n)
    return [
        ("independent", sine(45)(n), ar(_AR4, 20000.0, 5)(n)),              # unrelated channels: code 1
        ("left_side", smooth, smooth + small),                                # right = left + noise: code 8
        ("right_side", smooth + small, smooth),                               # code 9
        # code 10; the channels are even, so the side 4 e comes through exactly: two wasted bits
        ("mid_side",) + _exact(2 * (smooth + e), 2 * (smooth - e)),
        ("equal", _named("ar2_step_512"), _named("ar2_step_512")),            # side 0: CONSTANT
        # side = 8 s under a predictor, 3 wasted bits against the left's 1: code 9
        ("side_wasted_3",) + _exact(8 * (smooth // 8) + 2, np.full(n, 2, dtype=np.int64)),
        # left = 2 m over the whole range (VERBATIM at 15 bits), right = -left: mid 0, and the side 4 m is VERBATIM
        # at 15 bits under 2 wasted bits
        ("verbatim_side",) + _exact(2 * noise(16383, 35)(n), -2 * noise(16383, 35)(n)),
        ("noise_pair_wasted",) + _exact(8 * u + 2, 8 * v + 2),               # mid 1 wasted bit, side 3, both FIXED 0
        # right = 0, so side = left sample for sample; left is FIXED 0, which has no warm-up sample whose width
        # differs: independent (left + CONSTANT) and right-side (side + CONSTANT) cost the same
        ("fixed0_tie",) + _exact(x0, np.zeros(n, dtype=np.int64)),
        ("wasted_both",) + _exact(_named("w8_ar2"), _named("w8_sine_45")),    # mid and side keep wasted bits
        ("negated", smooth, -smooth),                                          # mid 0 or -1
    ]


@functools.lru_cache(maxsize=None)
def stereo_frames():
    """[(name, left pcm, right pcm)]: the special pairs, then every corpus frame beside its successor"""
    fr = frames()
    out = _pair_specials() + [(f"{a[0]}|{b[0]}", a[1], b[1]) for a, b in zip(fr, fr[1:] + fr[:1])]
    return out


def _column(frames_pcm, dtype):
    raw = np.concatenate([to_u16(x)[0] for x in frames_pcm])
    if dtype == "int16":
        raw = ((raw >> 1).astype(np.int32) - 16383).astype(np.int16)
    elif dtype == "uint8":
        raw = (raw // 257).astype(np.uint8)
    return raw.reshape(-1, TILE)


@functools.lru_cache(maxsize=None)
def stereo_raster(dtype="uint16"):
    """[2, frames * 32, 128]: one stream, frame f = the pair f (the corpus' anchors put 0 and 65534 into both bands)"""
    sf = stereo_frames()
    arr = np.stack([_column([l for _, l, _ in sf], dtype), _column([r for _, _, r in sf], dtype)])
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def multi_raster(bands, dtype="uint16"):
    """[bands, frames * 32, 128]: the corpus dealt over the channels, band b's frame f = corpus frame f * bands + b"""
    fr = frames()
    nf = -(-len(fr) // bands)
    arr = np.stack([_column([fr[(f * bands + b) % len(fr)][1] for f in range(nf)], dtype) for b in range(bands)])
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def shifted_raster(bands, dtype="uint16"):
    """[bands, frames * 32, 128]: every band holds the whole corpus, band b starting a b-th of the way in (as many
    frames as the corpus: enough for the decoders' batched route)"""
    fr = frames()
    n = len(fr)
    arr = np.stack([_column([fr[(f + b * n // bands) % n][1] for f in range(n)], dtype) for b in range(bands)])
    arr.setflags(write=False)
    return arr


def multi_names(bands):
    fr = frames()
    nf = -(-len(fr) // bands)
    return [fr[(f * bands + b) % len(fr)][0] for f in range(nf) for b in range(bands)]


# ------------------------------------------------------------------------------------------- partial last frames
PTILE = 96          # 96 x 96 = two frames and a 1024-sample tail
TAIL = PTILE * PTILE - 2 * FRAME
TAILS = [
    ("w2_sine_16", wasted(sine(16, 7000.0), 2)), ("w3_ar2", wasted(ar([1.2, -0.6], 3000.0, 20), 3)),
    ("w8_ar2", wasted(ar([1.2, -0.6], 100.0, 23), 8)), ("w12_walk", wasted(walk(0.4, 22, amp=7.0), 12)),
    ("w4_const", const(37 << 4)), ("w1_ar8", wasted(ar(_AR8, 15000.0, 24), 1)),
    ("sine_8", sine(8)), ("sine_16", sine(16)), ("sine_30", sine(30)), ("sine_70", sine(70)), ("sine_110", sine(110)),
    ("step_512", stepped_noise(512, 2.0, 64.0)), ("step_256", stepped_noise(256, 2.0, 8.0)),
    ("step_128", stepped_noise(128, 1.0, 3.0)), ("step_64", stepped_noise(64, 0.6, 1.9)),
    ("ar2_step_256", ar([1.2, -0.6], 30000.0, 13, steps(256, 1.0, 8.0))), ("alt_sine_3", alternate(sine(3))),
    ("noise_full", noise(HI)),
]


@functools.lru_cache(maxsize=None)
def partial_frames():
    """[(name, pcm)]: per 96 x 96 tile an anchored loud corpus frame, a quiet corpus frame and a 1024-sample tail"""
    fr = frames()
    out = []
    for t, (name, rec) in enumerate(TAILS):
        out += [fr[4 * (t % (len(fr) // 4))], fr[(4 * t + 1 + t % 3) % len(fr)], (f"tail_{name}", rec(TAIL))]
    return out


@functools.lru_cache(maxsize=None)
def partial_band(dtype="uint16"):
    band = _column([x for _, x in partial_frames()], dtype).reshape(-1, PTILE)
    band.setflags(write=False)
    return band


# -------------------------------------------------------------------------------------- the oracle's references
@functools.lru_cache(maxsize=None)
def tiles_reference(kind="mono", dtype="uint16", tile=TILE, level=5):
    """(arena bytes, tile offsets, mins, maxs) of the mono ("mono") or partial-tile ("partial") band at `tile`"""
    from oracle import oracle as O
    band = mono_band(dtype, tile) if kind == "mono" else partial_band(dtype)
    if level == 5:
        arena, off, mn, mx = O.encode_tiles(band, tile, RATE)
        return arena.tobytes(), [int(o) for o in off], list(mn), list(mx)
    out, off, mins, maxs = b"", [0], [], []
    for r0 in range(0, band.shape[0], tile):
        pcm, mn, mx, bps = O.normalize(np.ascontiguousarray(band[r0:r0 + tile]).reshape(-1))
        out += O.encode_frames(pcm, bps, RATE, level=level)
        off.append(len(out))
        mins.append(mn)
        maxs.append(mx)
    return out, off, mins, maxs


@functools.lru_cache(maxsize=None)
def stream_reference(bands, dtype="uint16", level=5):
    """(frames, pcm [N, bands], min, max) of the two-channel corpus (bands 2), the corpus dealt over `bands`, or
    (bands < 0) shifted_raster(-bands)"""
    from oracle import oracle as O
    arr = stereo_raster(dtype) if bands == 2 else shifted_raster(-bands, dtype) if bands < 0 else \
        multi_raster(bands, dtype)
    bands = abs(bands)
    pcm, mn, mx, bps = O.normalize(arr.transpose(1, 2, 0).reshape(-1, bands))
    assert bps == 16
    pcm.setflags(write=False)
    return O.encode_frames(pcm, bps, RATE, level=level), pcm, mn, mx


def census_of_tiles(ref, samples_per_tile, names):
    """the census of a tiles_reference, every subframe named after its corpus frame"""
    from oracle import oracle as O
    data, off = ref[0], ref[1]
    out = []
    for t in range(len(off) - 1):
        out += O.subframe_census(data[off[t]:off[t + 1]], 1, 16, samples_per_tile)
    assert len(out) == len(names)
    for c, name in zip(out, names):
        c["name"] = name
    return out


def census_of_stream(frames_bytes, bands, nsamples, names):
    from oracle import oracle as O
    out = O.subframe_census(frames_bytes, bands, 16, nsamples)
    assert len(out) == len(names), (len(out), len(names))
    for c, name in zip(out, names):
        c["name"] = name
    return out


# -------------------------------------------------------------------------------------------------------- cells
def is_side(c):
    return (c["assignment"], c["channel"]) in ((8, 1), (9, 0), (10, 1))


def cells_of(census):
    """{cell: name of the first subframe that reaches it}; a cell is a tuple, e.g. ("type", "FIXED 3"),
    ("porder", "lpc", 4), ("rice", 7), ("rice 14 smooth",), ("wasted", 8), ("wasted type", "lpc"), ("shift", 9),
    ("coef", "most positive"), ("assignment", 10), ("side", "verbatim"), ("side wasted",)"""
    got = {}
    for c in census:
        kind, name = c["kind"], c["name"]
        label = kind.upper() + (f" {c['order']}" if kind in ("fixed", "lpc") else "")
        reach = [("type", label)]
        if kind in ("fixed", "lpc"):
            reach.append(("porder", kind, c["porder"]))
            ks = [k for k in c["params"] if not isinstance(k, tuple)]
            reach += [("rice", k) for k in ks]
            # parameter 14 beside a partition of parameter 10 or less, under a predictor: large residuals in a frame
            # that is smooth elsewhere, not noise that verges on VERBATIM
            if ks and max(ks) == 14 and min(ks) <= 10 and label != "FIXED 0":
                reach.append(("rice 14 smooth",))
            reach += [("escape",)] * any(isinstance(k, tuple) for k in c["params"])
        if c["wasted"]:
            reach += [("wasted", c["wasted"]), ("wasted type", kind)]
        if kind == "lpc":
            reach.append(("shift", c["shift"]))
            lim = 1 << (c["precision"] - 1)
            reach += [("coef", "most positive")] * (max(c["coefs"]) == lim - 1)
            reach += [("coef", "most negative")] * (min(c["coefs"]) == -lim)
        if c["assignment"] >= 1 and c["blocksize"]:
            reach.append(("assignment", c["assignment"]))
        if is_side(c):
            reach.append(("side", kind))
            if c["wasted"]:
                reach.append(("side wasted",))
        for r in reach:
            got.setdefault(r, name)
    return got


REQUIRED_MONO = (
    [("type", t) for t in ["CONSTANT", "VERBATIM"] + [f"FIXED {k}" for k in range(5)] + [f"LPC {k}" for k in range(1, 9)]]
    + [("porder", kind, p) for kind in ("fixed", "lpc") for p in range(6)]
    + [("rice", k) for k in range(15)] + [("rice 14 smooth",)]
    + [("wasted type", k) for k in ("fixed", "lpc", "constant")]
    + [("shift", s) for s in range(9, 15)])
REQUIRED_STEREO = ([("assignment", a) for a in (1, 8, 9, 10)] + [("side", "constant"), ("side", "verbatim"), ("side wasted",)])
OPTIONAL = [("shift", 8), ("shift", 7), ("coef", "most positive"), ("coef", "most negative"), ("shift", 15)]


def wasted_counts_ok(cells):
    """wasted bits: 1, at least two different counts in 2..7, at least one of 8 or more"""
    w = {c[1] for c in cells if c[0] == "wasted"}
    return 1 in w and len(w & set(range(2, 8))) >= 2 and any(v >= 8 for v in w)
