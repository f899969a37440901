"""The (dtype, data_min, data_max) cases and the cover streams of the de-normalisation tests
(tests/test_denormalize_host.py on the CPU, tests/test_gpu_denormalize_values.py on the GPU), and the reference both
compare with: numpy's own evaluation of converter.py:88-110 after the PCM_16 round trip.

A cover stream holds every one of the 65 536 16-bit PCM values, so one decode of it with a case's (min, max) shows the
de-normalised value of every PCM value on the path that decoded it.
"""
import functools

import numpy as np

from tests import flac_builder as B
from tests.flac_builder import Sub
from tests.flac_layouts import _lpc

ALL_P16 = np.arange(-32768, 32768, dtype=np.int32)
ALL_P16.setflags(write=False)
LIMITS = {"uint8": (0, 255), "int16": (-32768, 32767), "uint16": (0, 65535), "int32": (-2 ** 31, 2 ** 31 - 1),
          "uint32": (0, 2 ** 32 - 1)}
DTYPES = ("uint8", "int16", "uint16", "int32", "uint32", "float32", "float64")
NARROW = ("uint8", "int16", "uint16")
EDGE_R = (0, 1, 2, 3, 5, 254, 255, 4095, 4096, 4097, 32767, 32768, 32769, 65534, 65535)
WIDE_R = (2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1)


def minima(lo, hi, R):
    """the dtype's lowest value, the highest minimum that R allows, the middle of the two, and one scattered value"""
    top = hi - R
    return sorted({lo, top, lo + (top - lo) // 2, min(top, lo + 577)})


def _cases():
    out = []
    for dt in NARROW:
        lo, hi = LIMITS[dt]
        out += [(dt, mn, mn + R) for R in EDGE_R if R <= hi - lo for mn in minima(lo, hi, R)]
    out += [("int32", -2 ** 31, 2 ** 31 - 1), ("int32", -7, 2 ** 24), ("uint32", 0, 2 ** 32 - 1)]
    # R on either side of fp32's last exact integer, at the dtype's lowest value, at a small minimum and at the highest
    # minimum the range allows.  Such an upper-edge case is in the list only because its minimum leaves room: the
    # largest de-normalised value lies R / 65536 = 256 below the maximum, more than fp32's rounding at 2^31 or 2^32
    # (at most 128 + 1).  A narrow range there, such as uint32 (2^32 - 1 - 70000, 2^32 - 1), rounds up to 2^32, and
    # float -> integer out of range is undefined in the reference: no such case is listed
    # (tests/test_denormalize_host.py asserts that every listed case stays inside its dtype at every PCM value).
    for dt, small in (("int32", -7), ("uint32", 577)):
        lo, hi = LIMITS[dt]
        out += [(dt, mn, mn + R) for R in WIDE_R for mn in (lo, small, hi - R)]
    # a minimum that fp32 rounds (2^24 + 1 -> 2^24): float32(max - min) = 3, where float32(max) - float32(min) is 4
    out += [(dt, 2 ** 24 + 1, 2 ** 24 + 4) for dt in ("int32", "uint32")]
    out += [("float32", -3.5, 1000.25), ("float64", 0.0, 1.0)]      # floats: the range is ignored
    return out


CASES = tuple(_cases())                                             # (dtype name, data_min, data_max)
assert len({c for c in CASES if c[0] in NARROW}) == len([c for c in CASES if c[0] in NARROW]) == 128


def cases_of(dtype):
    return [c for c in CASES if c[0] == np.dtype(dtype).name]


def numpy_rounded(p16, dmin, dmax):
    """np.round(((v + 1) / 2) * (max - min) + min) as float32, before the cast to an integer dtype"""
    v = (np.asarray(p16).astype(np.float64) / 32768.0).astype(np.float32)
    d = (v + 1.0) / 2.0 * (float(dmax) - float(dmin)) + float(dmin)    # Python floats beside a float32 array
    assert d.dtype == np.float32
    return np.round(d)


def numpy_denormalize(p16, dmin, dmax, dtype):
    """The reference's value for 16-bit samples p16 (of a 32-bit stream: pcm >> 16).  Integer dtypes: the rounded
    values must lie inside the dtype (asserted, never skipped: the cast is undefined outside it)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (np.asarray(p16).astype(np.float64) / 32768.0).astype(np.float32).astype(dtype)
    r = numpy_rounded(p16, dmin, dmax)
    lo, hi = LIMITS[dtype.name]
    assert float(r.min()) >= lo and float(r.max()) <= hi, (dtype.name, dmin, dmax, float(r.min()), float(r.max()))
    return r.astype(dtype)


@functools.lru_cache(maxsize=None)
def table(case):
    """numpy's value of every PCM value of a case: table(case)[p16 + 32768] (computed once, read-only)"""
    t = numpy_denormalize(ALL_P16, case[1], case[2], case[0])
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------------------------------ cover streams
SEED = 20261020
TAIL = (-32768, 32767, 0, -1, 1)


def _cover_frames():
    """16 frames of 4096: frame f holds -32768 + 4096 f .. + 4095, as VERBATIM shuffled, FIXED 2 ascending, LPC 8
    shuffled, FIXED 0 descending in turn"""
    rng = np.random.default_rng(SEED)
    frames = []
    for f in range(16):
        x = np.arange(4096, dtype=np.int64) - 32768 + 4096 * f
        k = f % 4
        if k == 0:
            frames.append((rng.permutation(x), [Sub("verbatim")]))
        elif k == 1:
            frames.append((x, [Sub("fixed", order=2, porder=3)]))
        elif k == 2:
            frames.append((rng.permutation(x), [_lpc(8, 12, f)]))
        else:
            frames.append((x[::-1].copy(), [Sub("fixed", order=0)]))
    return frames


def _mono_frames(odd):
    frames = _cover_frames()
    frames += [(np.full(4096, v, dtype=np.int64), [Sub("constant")]) for v in (-32768, 0, 32767)]
    frames.append((np.arange(4096, dtype=np.int64) * 12 - 24576, [Sub("fixed", order=1, porder=2, wasted=2)]))
    if odd:
        frames.append((np.array(TAIL, dtype=np.int64), [Sub("verbatim")]))
    return frames


def mono_frame_starts(odd):
    """byte offsets of the mono cover stream's frames"""
    sizes = [len(B.frame([x], subs, f, 16)) for f, (x, subs) in enumerate(_mono_frames(odd))]
    return [0] + np.cumsum(sizes)[:-1].tolist()


@functools.lru_cache(maxsize=None)
def mono_cover(odd):
    """Mono 16-bit, block 4096: the 16 cover frames, CONSTANT -32768 / 0 / 32767, a FIXED 1 frame with 2 wasted bits;
    odd: a 5-sample last frame, 81 925 samples in all, so that the output bases of consecutive copies of the stream
    run through every residue mod 8 (and no frame but the first of every eighth copy takes the 8-sample stores)."""
    s = B.stream_from_frames(_mono_frames(odd), 16, 4096, "cover_odd" if odd else "cover_aligned")
    s.pcm.setflags(write=False)
    assert len(s.pcm) == (81925 if odd else 81920) and np.unique(s.pcm[:65536]).size == 65536
    return s


SUBS_MC = (Sub("verbatim"), Sub("fixed", order=2, porder=3), Sub("fixed", order=1, porder=2), Sub("fixed", order=0))


@functools.lru_cache(maxsize=None)
def multi_cover(channels, chass):
    """`channels` channels of 16 bits, block 256, 256 frames: channel c is the cover rolled by 8191 c samples."""
    base = mono_cover(False).pcm[:65536, 0]
    pcm = np.stack([np.roll(base, 8191 * c) for c in range(channels)], axis=1)
    s = B.stream(pcm, 16, 256, lambda f, blk: [SUBS_MC[(f + c) % 4] for c in range(channels)],
                 f"cover_{channels}ch_chass{chass}", chass=chass)
    s.pcm.setflags(write=False)
    assert s.nframes == 256 and all(np.unique(s.pcm[:, c]).size == 65536 for c in range(channels))
    return s


MULTI_LAYOUTS = ((2, 1), (2, 10), (3, 2), (4, 3))                    # (channels, channel assignment)


@functools.lru_cache(maxsize=None)
def mono32_cover():
    """Mono 32-bit, block 256: (h << 16) | low with h the cover and low 16 random bits (0x0000 and 0xFFFF beside
    negative h among them); ramp frames FIXED 1 with Rice method 1, shuffled frames VERBATIM.  The WAV round trip keeps
    pcm >> 16 = h."""
    h = mono_cover(False).pcm[:65536, 0]
    low = np.random.default_rng(SEED + 1).integers(0, 65536, 65536)
    neg = np.flatnonzero(h < 0)
    low[neg[:4]] = (0x0000, 0xFFFF, 0x0000, 0xFFFF)
    low[neg[-4:]] = (0xFFFF, 0x0000, 0xFFFF, 0x0000)
    pcm = h * 65536 + low
    assert np.array_equal(pcm >> 16, h) and pcm.min() >= -2 ** 31 and pcm.max() < 2 ** 31

    def layout(f, blk):
        ramp = (f // 16) % 4 in (1, 3)                               # the cover frame of this block
        return [Sub("fixed", order=1, method=1, porder=2) if ramp else Sub("verbatim")]
    s = B.stream(pcm, 32, 256, layout, "cover_mono32")
    s.pcm.setflags(write=False)
    return s


def false_syncs(data: bytes, starts) -> list:
    """Positions outside `starts` where 0xFF 0xF8 / 0xF9 begins bytes that read as a frame header with a correct
    CRC-8 (header length from the block-size, sample-rate and number codes alone: no reserved-code checks, so this
    finds at least what a decoder's candidate search finds)."""
    data = data + bytes(16)
    a = np.frombuffer(data, dtype=np.uint8)
    hits = np.flatnonzero((a[:-1] == 0xFF) & ((a[1:] & 0xFE) == 0xF8))
    out = []
    for p in hits.tolist():
        if p in starts:
            continue
        v = data[p + 4]
        n = 5 + (0 if v < 0x80 else 1 if v < 0xE0 else 2 if v < 0xF0 else 3 if v < 0xF8 else 4 if v < 0xFC else
                 5 if v < 0xFE else 6)
        n += {6: 1, 7: 2}.get(data[p + 2] >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(data[p + 2] & 15, 0)
        if B.crc8(data[p:p + n]) == data[p + n]:
            out.append(p)
    return out
