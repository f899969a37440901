"""The hand-built streams of tests/test_flac_builder.py (CPU: the oracle agrees with the known samples) and
tests/test_gpu_decode_layouts.py (GPU: every decoder returns the known samples).  Every stream is valid FLAC
(RFC 9639) with >= 65 frames, so the forced lane decoder and the multi-channel lane path (frames >= 64) take it, and
different layouts sit in neighbouring frames: lanes of one wave diverge, and a frame one decoder declines sits between
frames it accepts.  Every frame stays below the decoders' frame-size bound (5 bytes per sample + 4096: no Rice
parameter far too small for its residuals).  STREAMS maps a name to (builder, decoder kinds it is run on)."""
import functools

import numpy as np

from tests import flac_builder as B
from tests.flac_builder import Sub

NF = 66
ALL, MULTI, WAVE = ("pipe", "pipe_chain", "lane", "wave"), ("lane", "wave"), ("wave",)
ESC = ("esc", None)


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _smooth(n, seed, amp=12000.0, noise=30.0):
    rng = _rng(1, seed)
    t = np.arange(n) + int(rng.integers(0, 1000))
    x = amp * np.sin(t / 23.0) + 0.3 * amp * np.sin(t / 3.7 + 1.0) + rng.normal(0, noise, n)
    return np.rint(x).astype(np.int64)


def _loud(n, seed, bits=16):
    """Uniform over the whole `bits`-bit range, both extremes present."""
    x = _rng(2, seed).integers(-(1 << (bits - 1)), 1 << (bits - 1), n)
    if n >= 2:
        x[n // 3], x[n // 2] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return x.astype(np.int64)


def _lpc(o, prec, seed, **kw):
    """LPC of order o with coefficients over the full `prec`-bit range (none zero, the first and last at the
    extremes, so every tap matters) and the shift that brings sum |q| to [2, 4): residuals stay below 2^(sbps + 2)."""
    lim = 1 << (prec - 1)
    q = _rng(3, seed).integers(-lim, lim, o)
    q[q == 0] = 1
    q[0], q[-1] = -lim, lim - 1
    shift = max(0, int(np.abs(q).sum()).bit_length() - 2)
    return Sub("lpc", order=o, precision=prec, shift=shift, coefs=[int(v) for v in q], **kw)


def _plain(f, n):
    return _smooth(n, f), [Sub("fixed", order=2, porder=2)]


def _cycle(name, bs, makers, nf=NF, bps=16, **hdr):
    """Frame f from makers[f % len(makers)](f, bs) -> (samples, subs[, header arguments])."""
    return B.stream_from_frames([makers[f % len(makers)](f, bs) for f in range(nf)], bps, bs, name, **hdr)


# ------------------------------------------------------------------------------------------------ mono, 16-bit
def lpc_order():
    """Orders 8, 9, 12, 32 at the precision where prec + sbps + ceil(log2 o) is 31 ("32-bit safe", unchecked) and 32
    (checked), partition orders 0..3 (order 32 at partition order 3: an empty first partition)."""
    mk = []
    for o, precs in ((8, (12, 13)), (9, (11, 12)), (12, (11, 12)), (32, (10, 11))):
        for prec in precs:
            assert prec + 16 + (o - 1).bit_length() == (31 if prec == precs[0] else 32)
            mk.append(lambda f, n, o=o, prec=prec: (_loud(n, f), [_lpc(o, prec, f, porder=f // 12 % 4)]))
        mk.append(_plain)
    return _cycle("lpc_order", 256, mk, nf=72)


def lpc12_wasted2():
    """Order 12 on samples with 2 wasted bits (sbps 14): precision 13 (sum 31) and 14 (sum 32)."""
    mk = [lambda f, n, prec=prec: (_loud(n, f, 14) << 2, [_lpc(12, prec, f, wasted=2, porder=f % 3)])
          for prec in (13, 14)]
    mk.append(lambda f, n: (_smooth(n, f, 3000) << 2, [Sub("fixed", order=2, porder=2, wasted=2)]))
    mk.append(_plain)
    return _cycle("lpc12_wasted2", 256, mk)


def _esc_at(p, count=8):
    return [ESC if i == p else None for i in range(count)]


def escape_first():
    """An escape in partition 0 (a decoder that declines it does so before it wrote anything)."""
    return _cycle("escape_first", 256, [
        lambda f, n: (_loud(n, f), [_lpc(8, 12, f, porder=3, params=_esc_at(0))]),
        _plain,
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=2, porder=3, params=_esc_at(0))]),
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=4, porder=0, params=ESC)]),
        _plain])


def escape_mid():
    """An escape in partition 5 of 8 (declined after outputs of the frame were written)."""
    return _cycle("escape_mid", 256, [
        lambda f, n: (_loud(n, f), [_lpc(8, 12, f, porder=3, params=_esc_at(5))]),
        _plain,
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=3, porder=3, params=_esc_at(5))]),
        _plain,
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=1, porder=3, params=_esc_at(7))])])


def escape_misc():
    """Escapes of width 0 (a flat stretch under FIXED 1), of a width wider than needed, on FIXED order 0, and in
    every partition of a frame."""
    def flat(f, n):
        x = _smooth(n, f)
        x[64:192] = x[64]
        par = [None, None, None, ("esc", 0), None, ("esc", 0), None, None]
        return x, [Sub("fixed", order=1, porder=3, params=par)]
    return _cycle("escape_misc", 256, [
        flat,
        _plain,
        lambda f, n: (_smooth(n, f, 900), [Sub("fixed", order=0, porder=2, params=[ESC, None, ESC, None])]),
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=2, porder=1, params=[None, ("esc", 20)])]),
        _plain,
        lambda f, n: (_loud(n, f), [Sub("fixed", order=0, porder=4, params=ESC)])])


def rice2():
    """Rice method 1 (5-bit parameters) on a 16-bit stream: parameters 0, 3, 14, 15, 16 and 30."""
    def flat(f, n):
        return 100 + _rng(4, f).integers(-1, 2, n), [Sub("fixed", order=1, method=1, porder=1, params=0)]
    mk = [flat, _plain]
    mk.append(lambda f, n: (_smooth(n, f, 2000), [Sub("fixed", order=2, method=1, porder=2, params=3)]))
    for k in (14, 15, 16, 30):
        mk.append(lambda f, n, k=k: (_loud(n, f), [Sub("fixed", order=1, method=1, porder=2, params=k)]))
    mk.append(lambda f, n: (_loud(n, f), [_lpc(4, 10, f, method=1, porder=1, params=[15, 16])]))
    mk.append(lambda f, n: (_smooth(n, f), [Sub("fixed", order=2, method=1, porder=2)]))
    return _cycle("rice2", 256, mk)


def rice_long():
    """Rice method 0, parameter 14, under FIXED 4: an alternating full-scale burst gives codes of 64 zeros and more
    (> 64 bits), a single spike codes between 32 and 64 bits; their place moves from frame to frame."""
    longest = []

    def spiky(f, n):
        x = _smooth(n, f, 2000)
        a = 8 + (f * 37) % (n - 40)
        x[a:a + 6] = [32767, -32768, 32767, -32768, 32767, -32768]
        x[a + 20] = 30000
        u = np.abs(B.residuals(x, B.FIXED_COEFS[4], 0)) * 2
        longest.append(sorted(set(((u >> 14) + 15).tolist())))
        return x, [Sub("fixed", order=4, porder=f // 3 % 3, params=14)]
    s = _cycle("rice_long", 256, [spiky, _plain, lambda f, n: (_loud(n, f), [_lpc(6, 12, f, params=14)])])
    assert all(any(32 < b <= 64 for b in l) and any(b > 64 for b in l) for l in longest)
    return s


def porder_fixed4():
    """Partition orders 0..6 under FIXED 4 at block size 256 (6: partition size 4 = the order, an empty first
    partition)."""
    return _cycle("porder_fixed4", 256, [
        lambda f, n, po=po: (_smooth(n, f) if f % 2 else _loud(n, f), [Sub("fixed", order=4, porder=po)])
        for po in range(7)], nf=70)


def porder_lpc8():
    """Partition orders 0..5 under LPC 8 at block size 256 (5: partition size 8 = the order)."""
    return _cycle("porder_lpc8", 256, [
        lambda f, n, po=po: (_loud(n, f), [_lpc(8, 12, f, porder=po)]) for po in range(6)])


def porder_high():
    """Partition orders 7 and 8 = log2(256) (FIXED 1 at 8: partitions of one sample, the first one empty)."""
    return _cycle("porder_high", 256, [
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=1, porder=8)]),
        _plain,
        lambda f, n: (_loud(n, f), [Sub("fixed", order=2, porder=7)]),
        lambda f, n: (_smooth(n, f), [Sub("fixed", order=0, porder=8)]),
        lambda f, n: (_loud(n, f), [_lpc(2, 9, f, porder=7)])])


def wasted():
    """Wasted bits 1, 7 and 15 (sbps 15, 9 and 1) on CONSTANT, VERBATIM, FIXED and LPC."""
    mk = []
    for w in (1, 7, 15):
        mk += [lambda f, n, w=w: (np.full(n, -(f % 2) << w if w == 15 else (37 - 3 * f) << w),
                                  [Sub("constant", wasted=w)]),
               lambda f, n, w=w: (_loud(n, f, 16 - w) << w, [Sub("verbatim", wasted=w)]),
               lambda f, n, w=w: (_loud(n, f, 16 - w) << w, [Sub("fixed", order=2, porder=2, wasted=w)]),
               lambda f, n, w=w: (_loud(n, f, 16 - w) << w, [_lpc(4, 10, f, porder=1, wasted=w)]),
               _plain]
    return _cycle("wasted", 256, mk, nf=75)


def lpc_params():
    """Shift 0 and 15, precision 1 and 15, coefficients at the negative and positive extremes."""
    ext = [-16384, 16383] * 6
    return _cycle("lpc_params", 256, [
        lambda f, n: (_rng(5, f).integers(-8, 9, n), [Sub("lpc", order=2, precision=15, shift=0, coefs=ext[:2])]),
        lambda f, n: (_loud(n, f), [Sub("lpc", order=8, precision=15, shift=15, coefs=[-16384] * 8, porder=2)]),
        _plain,
        lambda f, n: (_loud(n, f), [Sub("lpc", order=8, precision=15, shift=15, coefs=[16383] * 8, porder=1)]),
        lambda f, n: (_loud(n, f), [Sub("lpc", order=3, precision=1, shift=0, coefs=[-1, -1, -1], porder=3)]),
        lambda f, n: (_loud(n, f), [Sub("lpc", order=5, precision=1, shift=15, coefs=[-1, 0, -1, 0, -1])]),
        lambda f, n: (_loud(n, f), [Sub("lpc", order=12, precision=15, shift=15, coefs=ext, porder=2)])], nf=70)


def _maxpo(bs, order, cap):
    po = 0
    while po < cap and bs % (2 << po) == 0 and (bs >> (po + 1)) >= order:
        po += 1
    return po


def blocksize(bs, tail, codes, nf=NF):
    """Streams of `bs`-sample frames, the block-size code cycling through `codes` (table codes, 6 / 7: the explicit
    8- / 16-bit forms), and a last frame of `tail` samples."""
    def sig(f, n):
        return _smooth(n, f) if f % 2 else _loud(n, f)
    mk = [lambda f, n: (sig(f, n), [Sub("fixed", order=2, porder=_maxpo(n, 2, 2))]),
          lambda f, n: (sig(f, n), [_lpc(8, 12, f, porder=_maxpo(n, 8, 3))]),
          lambda f, n: (sig(f, n), [Sub("verbatim")]),
          lambda f, n: (np.full(n, 1000 - 77 * f), [Sub("constant")]),
          lambda f, n: (sig(f, n), [Sub("fixed", order=4, porder=_maxpo(n, 4, 9))]),
          lambda f, n: (sig(f, n), [_lpc(12, 12, f, porder=_maxpo(n, 12, 1))]),
          lambda f, n: (sig(f, n), [Sub("fixed", order=1, porder=_maxpo(n, 1, 8))])]
    frames = []
    for f in range(nf):
        x, subs = mk[f % len(mk)](f, bs)
        frames.append((x, subs, {"bs_code": codes[f % len(codes)]}))
    if tail:
        sub = _lpc(8, 12, nf) if tail > 8 else Sub("fixed", order=4) if tail > 4 else Sub("fixed", order=0)
        frames.append((sig(nf, tail), [sub], {"bs_code": 6 if tail <= 256 else 7}))
    return B.stream_from_frames(frames, 16, bs, f"bs{bs}")


def headers():
    """Sample-rate codes 0, 12, 13, 14 (with their extra header bytes) and 9; sample-size code 0 (from the stream)
    on every other frame."""
    rates = ((0, None), (12, 44), (13, 44100), (14, 4410), (9, None))
    subs = (lambda f: Sub("fixed", order=2, porder=2), lambda f: _lpc(4, 10, f), lambda f: Sub("verbatim"))
    frames = []
    for f in range(NF):
        sr, extra = rates[f % 5]
        frames.append((_smooth(256, f), [subs[f % 3](f)], {"sr_code": sr, "sr_extra": extra, "ss_code": 4 * (f % 2)}))
    return B.stream_from_frames(frames, 16, 256, "headers")


def frame_numbers():
    """2100 frames of 16 samples, CONSTANT / VERBATIM only: frame numbers cross the 1 -> 2 (128) and 2 -> 3 (2048)
    byte boundaries of their UTF-8 coding."""
    return _cycle("frame_numbers", 16, [lambda f, n: (np.full(n, f - 1000), [Sub("constant")]),
                                        lambda f, n: (_loud(n, f), [Sub("verbatim")]),
                                        lambda f, n: (_smooth(n, f), [Sub("verbatim")])], nf=2100)


# ------------------------------------------------------------------------------------------ two channels, 16-bit
def stereo(chass):
    """Assignment 1 (independent), 8 (left/side), 9 (side/right) or 10 (mid/side): the side subframe (channel 1 of
    assignment 1) as full-range VERBATIM (17 bits for a side), CONSTANT, with wasted bits, with an escape partition,
    with LPC order 12, and with odd values only (the parity bit mid/side drops from mid)."""
    sb = 17 if chass >= 8 else 16
    kinds = [
        lambda f, n: (_loud(n, f, sb) * 63 // 64, Sub("verbatim")),
        lambda f, n: (_smooth(n, f, 8000), Sub("fixed", order=2, porder=2)),
        lambda f, n: (np.full(n, 54321 if sb == 17 else 12345), Sub("constant")),
        lambda f, n: ((_loud(n, f, sb - 3) * 63 // 64) << 3, Sub("fixed", order=1, porder=1, wasted=3)),
        lambda f, n: (_smooth(n, f, 20000), Sub("fixed", order=2, porder=2, params=[None, ESC, None, None])),
        lambda f, n: (_loud(n, f, sb) * 63 // 64, _lpc(12, 11, f, porder=1)),
        lambda f, n: (_smooth(n, f, 9000) | 1, Sub("fixed", order=2, porder=2)),
    ]
    frames = []
    for f in range(NF + 4):
        S, ssub = kinds[f % len(kinds)](f, 256)
        M = (S >> 1) + _smooth(256, 1000 + f, 100)
        msub = Sub("fixed", order=2, porder=1)
        if chass == 1:
            L, R, subs = M, S, [msub, ssub]
        elif chass == 9:
            R, subs = M - S, [ssub, msub]
            L = R + S
        else:
            L, subs = M, [msub, ssub]
            R = L - S
        frames.append((np.stack([L, R], axis=1), subs))
    return B.stream_from_frames(frames, 16, 256, f"stereo_chass{chass}", chass=chass)


# ---------------------------------------------------------------------------------------- three channels, 16-bit
def three_channels():
    """Frames where exactly one channel's subframe is LPC order 12 or has an escape partition, in each channel
    position, between frames of FIXED subframes only."""
    frames = []
    for f in range(NF + 4):
        k = f % 7
        subs = [Sub("fixed", order=2, porder=2) for _ in range(3)]
        cols = [_smooth(256, 10 * f + c) for c in range(3)]
        if k < 3:
            subs[k], cols[k] = _lpc(12, 11, f, porder=2), _loud(256, f)
        elif k < 6:
            subs[k - 3] = Sub("fixed", order=2, porder=3, params=_esc_at(f % 8))
        frames.append((np.stack(cols, axis=1), subs))
    return B.stream_from_frames(frames, 16, 256, "three_channels")


# --------------------------------------------------------------------------------------------- 32-bit (control)
def _smooth32(n, seed, amp):
    rng = _rng(6, seed)
    t = np.arange(n) + int(rng.integers(0, 1000))
    return np.rint(amp * np.sin(t / 50.0) + rng.normal(0, 1000, n)).astype(np.int64)


def mono32_lpc12():
    """32-bit mono, samples near full scale: LPC order 12 (a second-difference predictor with small taps 8..11),
    Rice method 1."""
    q = [8192, -4096, 0, 0, 0, 0, 0, 0, 3, -3, 2, -2]
    return _cycle("mono32_lpc12", 256, [
        lambda f, n: (_smooth32(n, f, 0.9 * 2 ** 31),
                      [Sub("lpc", order=12, precision=15, shift=12, coefs=q, method=1, porder=f % 3)]),
        lambda f, n: (_smooth32(n, f, 0.9 * 2 ** 31), [Sub("fixed", order=2, method=1, porder=2)])], bps=32)


def stereo32_side():
    """32-bit stereo with a 33-bit side: an escape partition under mid/side and left/side, VERBATIM under
    side/right, LPC order 12 under mid/side."""
    q = [8192, -4096, 0, 0, 0, 0, 0, 0, 3, -3, 2, -2]
    esc = Sub("fixed", order=2, method=1, porder=2, params=[None, ESC, None, None])
    kinds = [(10, esc), (8, esc), (9, Sub("verbatim")), (10, Sub("fixed", order=2, method=1, porder=2)),
             (10, Sub("lpc", order=12, precision=15, shift=12, coefs=q, method=1, porder=1))]
    frames = []
    for f in range(NF):
        chass, ssub = kinds[f % len(kinds)]
        S = _smooth32(256, f, 0.9 * 2 ** 32) | (f % 2)
        assert S.max() >= 2 ** 31  # a side beyond 32 bits
        L = (S >> 1) + _smooth(256, f, 100)
        msub = Sub("fixed", order=2, method=1, porder=1)
        frames.append((np.stack([L, L - S], axis=1), [ssub, msub] if chass == 9 else [msub, ssub], {"chass": chass}))
    return B.stream_from_frames(frames, 32, 256, "stereo32_side")


STREAMS = {
    "lpc_order": (lpc_order, ALL), "lpc12_wasted2": (lpc12_wasted2, ALL),
    "escape_first": (escape_first, ALL), "escape_mid": (escape_mid, ALL), "escape_misc": (escape_misc, ALL),
    "rice2": (rice2, ALL), "rice_long": (rice_long, ALL),
    "porder_fixed4": (porder_fixed4, ALL), "porder_lpc8": (porder_lpc8, ALL), "porder_high": (porder_high, ALL),
    "wasted": (wasted, ALL), "lpc_params": (lpc_params, ALL),
    "bs16": (lambda: blocksize(16, 1, (6, 7)), ALL), "bs17": (lambda: blocksize(17, 0, (6, 7)), ALL),
    "bs63": (lambda: blocksize(63, 7, (6, 7)), ALL), "bs192": (lambda: blocksize(192, 0, (1, 6, 7)), ALL),
    "bs1000": (lambda: blocksize(1000, 9, (7,)), ALL), "bs4096": (lambda: blocksize(4096, 3001, (12, 7), 65), ALL),
    "headers": (headers, ALL), "frame_numbers": (frame_numbers, ALL),
    "stereo_chass1": (lambda: stereo(1), MULTI), "stereo_chass8": (lambda: stereo(8), MULTI),
    "stereo_chass9": (lambda: stereo(9), MULTI), "stereo_chass10": (lambda: stereo(10), MULTI),
    "three_channels": (three_channels, MULTI),
    "mono32_lpc12": (mono32_lpc12, WAVE), "stereo32_side": (stereo32_side, WAVE),
}


@functools.lru_cache(maxsize=None)
def get(name) -> B.Stream:
    """The stream (built once per process; callers must not change it)."""
    s = STREAMS[name][0]()
    s.pcm.setflags(write=False)
    return s
