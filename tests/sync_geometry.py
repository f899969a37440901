"""Blobs with frames at prescribed positions, for the stages that locate frames (csrc/frs_decode.hip: the selection
k_sync_select<4> / <16> and k_sync_count + k_sync_scan + k_sync_scatter, the span checks k_span_crc_wave / _lane /
k_span_pcrc, the chain k_chain_lds).  Built on tests/flac_builder.py; the truth is the samples that went in.
tests/test_sync_geometry_host.py checks the blobs on the CPU (the candidate model, the coverage of every position
class, the oracle's decode, the route of every GPU case); tests/test_gpu_sync_geometry.py decodes them on the GPU.

Positions are in "aligned space": q = p + lead, p the offset from the range's first byte, lead the low four bits of
the device address of that byte (the kernels load from the 16-byte boundary below it).  A selection form has lanes of
16 bytes, steps of 1 KB, waves of W and blocks of Bk bytes (FORMS).  A blob is

    [front guard >= 16 B] [stream 0 .. stream n-1] [back guard >= 32 B]

and a decode passes stream_off[0] = the guard's length, chosen mod 16 against the buffer's address to get `lead`.
A blob is built for one lead: stream 0 absorbs it (it ends at the same q for every lead) and the last stream sets
nbytes + lead, so everything between is built once per form (_body).

Placement is to the byte: a spacer stream of VERBATIM frames (2 bytes per 16-bit sample), a short last frame and the
header forms of tests/test_gpu_decode_layouts.py[headers-*] for the parity (sample-rate code 9 / 12 / 13: +0 / +1 /
+2 bytes, block-size code 7 for the table code: +2) precedes each probe stream.  Probe frames have the longest
header their stream allows (block-size code 7, sample-rate code 13: 10 bytes, 11 at frame numbers >= 128), so a header
really crosses the boundary it is placed at.  VERBATIM samples hold no sync pattern (_clean), so the candidates of a
blob are its frames and the false syncs planted on purpose, nothing else (the host test asserts it).
"""
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import flac_builder as B
from tests.flac_builder import Sub

BS = 1024                                   # block size of the mono blobs
BS8 = 4096                                  # of the 8-channel blob
FORMS = {"small": (4096, 16384), "onepass": (16384, 65536), "twopass": (16384, 65536)}  # form -> (W, Bk)
OFFSETS = tuple(range(-16, 2))              # d: a frame start at boundary + d (-1: the FF / F8 pair is split)
MIB = 1 << 20
Q0 = 512                                    # stream 0 ends at this q under every lead
MIN_SPACER = 13
VERB, CONST = Sub("verbatim"), Sub("constant")
FIXED = Sub("fixed", order=2, porder=2)
LONG = {"bs_code": 7, "sr_code": 13, "sr_extra": 44100}  # the longest header form
# header forms by the bytes they add to a full frame's 6-byte header (table block size, sample-rate code 9)
EXTRA = [{}, {"sr_code": 12, "sr_extra": 44}, {"sr_code": 13, "sr_extra": 44100},
         {"bs_code": 7, "sr_code": 12, "sr_extra": 44}, {"bs_code": 7, "sr_code": 13, "sr_extra": 44100}]


def _rng(*seed):
    return np.random.default_rng([77] + [int(s) for s in seed])


def _clean(x: np.ndarray) -> np.ndarray:
    """16-bit samples whose big-endian bytes hold no FF F8 / FF F9 pair, within a sample or across two: no low byte
    is FF, and a high byte FF (which stays: the selection's 0xFF pre-test sees plenty) is not followed by F8 / F9."""
    x = np.asarray(x, dtype=np.int64)
    x = np.where(x & 0xFF == 0xFF, x - 1, x)
    return np.where((x >> 8 & 0xFF == 0xFF) & (x & 0xFE == 0xF8), x - 8, x)


def _verb(n, *seed, channels=1):
    return _clean(_rng(1, *seed).integers(-32768, 32768, size=(n, channels)))


def _smooth(n, *seed, channels=1):
    rng = _rng(2, *seed)
    t = np.arange(n)[:, None] + rng.integers(0, 1000, size=(1, channels))
    return np.rint(3000 * np.sin(t / 19.0) + rng.normal(0, 4, (n, channels))).astype(np.int64)


def _const(n, v, channels=1):
    return np.full((n, channels), v, dtype=np.int64)


def header_len(frame_no: int, kw: dict, n: int, bs: int) -> int:
    code = kw.get("bs_code")
    if code is None:
        code = B.BS_TABLE.get(n, 6 if n <= 256 else 7)
    return 4 + len(B.utf8_number(frame_no)) + {6: 1, 7: 2}.get(code, 0) + {12: 1, 13: 2, 14: 2}.get(
        kw.get("sr_code", 9), 0) + 1


@dataclass
class Str:
    """One stream: its bytes, the samples that went in ([n, channels] int16), the offset and header length of every
    frame, and the index of the frame a placement aims at."""
    data: bytes
    pcm: np.ndarray
    starts: Tuple[int, ...]
    hlens: Tuple[int, ...]
    target: int = 0
    false_syncs: Tuple[int, ...] = ()   # offsets of planted headers inside frame data
    probe: bool = False


def make_stream(frames, bs: int, target: int = 0, probe: bool = False, false_syncs=()) -> Str:
    """frames: (samples [n, C], subs per channel, header arguments) per frame, every frame but the last `bs` long."""
    out, starts, hlens, blocks = bytearray(), [], [], []
    for f, (x, subs, kw) in enumerate(frames):
        x = np.asarray(x, dtype=np.int64)
        assert len(x) == bs or (f == len(frames) - 1 and 0 < len(x) < bs)
        fr = B.frame([x[:, c] for c in range(x.shape[1])], subs, f, 16, **kw)
        hl = header_len(f, kw, len(x), bs)
        assert B.crc8(fr[:hl - 1]) == fr[hl - 1]
        assert len(fr) < bs * x.shape[1] * 5 + 4096
        starts.append(len(out))
        hlens.append(hl)
        out += fr
        blocks.append(x)
    pcm = np.concatenate(blocks)
    assert pcm.min() >= -32768 and pcm.max() <= 32767
    return Str(bytes(out), pcm.astype(np.int16), tuple(starts), tuple(hlens), target, tuple(false_syncs), probe)


# ------------------------------------------------------------------------------------------------ mono pieces
def _short_frame(nbytes: int, *seed):
    """A short VERBATIM frame of exactly nbytes (13 .. 2058): block-size code 7, sample-rate code 9 / 12."""
    sx = (nbytes - 11) % 2
    n = (nbytes - 11 - sx) // 2
    assert 1 <= n < BS
    return _verb(n, 4, *seed), [VERB], {"bs_code": 7, **EXTRA[sx]}


def first_stream(nbytes: int, *seed) -> Str:
    """Stream 0 of a blob: a CONSTANT frame with the table-code header (11 bytes) and a short frame, nbytes in all."""
    return make_stream([(_const(BS, -4321), [CONST], {}), _short_frame(nbytes - 11, *seed)], BS)


def spacer(nbytes: int, *seed) -> Str:
    """A mono stream of exactly `nbytes` bytes: full VERBATIM frames, whose header forms add 0..4 bytes each, and a
    short last frame (block-size code 7, sample-rate code 9 / 12: 11 or 12 bytes + 2 per sample)."""
    full = 6 + 1 + 2 * BS + 2
    assert nbytes >= MIN_SPACER
    for k in range(min(nbytes // full, 126), -1, -1):
        for e in range(4 * k + 1):
            r = nbytes - k * full - e
            if MIN_SPACER <= r <= 12 + 2 * (BS - 1):
                frames = []
                for f in range(k):
                    frames.append((_verb(BS, 3, f, *seed), [VERB], EXTRA[min(4, e)]))
                    e -= min(4, e)
                frames.append(_short_frame(r, *seed))
                s = make_stream(frames, BS)
                assert len(s.data) == nbytes
                return s
    raise AssertionError("no spacer of %d bytes" % nbytes)


@functools.lru_cache(maxsize=None)
def filler() -> Str:
    """Eight full VERBATIM frames: repeated as further streams to size a blob."""
    return make_stream([(_verb(BS, 5, f), [VERB], {}) for f in range(8)], BS)


@functools.lru_cache(maxsize=None)
def tiny(i: int) -> Str:
    """A one-frame stream of 16 samples (42 bytes)."""
    return make_stream([(_verb(16, 6, i), [VERB], {"bs_code": 6})], BS)


def probe(kind: int, *seed) -> Str:
    """A probe stream: VERBATIM, FIXED and CONSTANT frames, all with the longest header; `target` is the frame that is
    placed.  Kind 2 places frame 129, whose number takes two bytes (an 11-byte header)."""
    v = int(_rng(7, *seed).integers(-30000, 30000))
    if kind == 0:
        fr, t = [(_verb(BS, 8, *seed), [VERB], LONG), (_const(37, v), [CONST], LONG)], 0
    elif kind == 1:
        fr, t = [(_const(BS, v), [CONST], LONG), (_smooth(BS, 8, *seed), [FIXED], LONG),
                 (_verb(100, 9, *seed), [VERB], LONG)], 1
    elif kind == 2:
        fr = [(_const(BS, v + f), [CONST], LONG) for f in range(129)]
        fr += [(_verb(BS, 8, *seed), [VERB], LONG), (_smooth(200, 9, *seed), [FIXED], LONG)]
        t = 129
    else:
        fr, t = [(_verb(BS, 8, *seed), [VERB], LONG), (_const(BS, v), [CONST], LONG),
                 (_smooth(BS, 9, *seed), [FIXED], LONG), (_verb(61, 10, *seed), [VERB], LONG)], 1
    return make_stream(fr, BS, target=t, probe=True)


# ------------------------------------------------------------------------------------------------ the layout
class Layout:
    """Streams appended at an aligned-space cursor."""

    def __init__(self, q: int, form: str, make_spacer=spacer, make_filler=filler):
        self.q, self.form, self.streams = q, form, []
        self.spacer, self.filler = make_spacer, make_filler

    def add(self, s: Str):
        self.streams.append(s)
        self.q += len(s.data)

    def pad_to(self, q: int):
        fill = self.filler()
        while q - self.q >= len(fill.data) + MIN_SPACER + 64:
            self.add(fill)
        if q != self.q:
            self.add(self.spacer(q - self.q, self.q))

    def boundary(self, cls: str, qmin: int) -> int:
        """The first multiple of 1 KB at or above qmin that is a block boundary ("block"), a wave boundary inside a
        block ("wave") or a step boundary inside a wave ("step")."""
        W, Bk = FORMS[self.form]
        unit = {"block": Bk, "wave": W, "step": 1024}[cls]
        m = -(-qmin // unit) * unit
        while (cls == "wave" and m % Bk == 0) or (cls == "step" and m % W == 0):
            m += unit
        return m

    def place(self, s: Str, cls: str, d: int):
        """s.target's first byte at d past the next boundary of the class that leaves room for a spacer."""
        toff = s.starts[s.target]
        m = self.boundary(cls, self.q + MIN_SPACER + 64 + toff - d)
        self.pad_to(m + d - toff)
        self.add(s)


@functools.lru_cache(maxsize=None)
def _body(form: str) -> Tuple[Str, ...]:
    """The lead-independent streams of a form's blob, from q = Q0: a probe at every offset of OFFSETS around a block,
    a wave and a step boundary (G-block, G-wave, G-step; all 16 lane offsets with them: G-lane; stream ends on a block
    boundary and one byte to either side: G-bound), a run of 16-sample streams (G-bound: dense boundaries, a block of
    far more than 32 candidates), a block of exactly 33 candidates (G-cap; 31 and 32 come with the filler)."""
    lay = Layout(Q0, form)
    k = 0
    for d in OFFSETS:
        for cls in ("block", "wave", "step"):
            # the two-byte frame number at the offsets where the most of a header crosses, on every class
            # (a block's probes at -1, 0, +1 begin their stream: its boundary is the stream boundary of G-bound)
            kind = 0 if cls == "block" and d >= -1 else 2 if d in (-1, -10) else k % 2 if form == "small" else \
                (0, 1, 3)[k % 3]
            lay.place(probe(kind, k), cls, d)
            k += 1
    lay.pad_to(lay.boundary("step", lay.q + 200) + 5)
    for i in range(2000 if form == "twopass" else 400):
        lay.add(tiny(i % 4))
    # 33 frame starts in one 64 KB block (two CONSTANT frames and 31 VERBATIM ones behind a frame that begins before
    # the block), one of them 5 bytes before a wave boundary: a block the placement pass reads again holds a header in
    # a wave's last 16 bytes
    fr = [(_verb(BS, 11, 0), [VERB], LONG), (_const(BS, 123), [CONST], LONG), (_const(BS, -7), [CONST], LONG)]
    fr += [(_verb(BS, 11, f), [VERB], LONG) for f in range(1, 32)]
    over = make_stream(fr, BS, target=10, probe=True)
    m = lay.boundary("block", lay.q + 400)
    lay.pad_to(m + 16384 - 5 - over.starts[10])
    assert lay.q < m < lay.q + over.starts[1]
    lay.add(over)
    size = {"small": 0, "onepass": 4 * MIB, "twopass": 16 * MIB}[form]
    if size:
        lay.pad_to(size + 3000)
    return tuple(lay.streams)


def end_q(form: str, lead: int, qmin: int) -> int:
    """nbytes + lead of a form's blob: lead 0 ends on a block boundary (no partial block), lead 1 or 5 one byte past
    one (the last block holds the final CRC byte only), the others elsewhere."""
    Bk = FORMS[form][1]
    m = -(-(qmin + 3000) // Bk) * Bk
    return m if lead == 0 else m + 1 if lead in (1, 5) else m + 16 * lead + (5 * lead + 3) % 16


# ------------------------------------------------------------------------------------------------ the guards
def short_header(b2: int, b3: int, want_crc: Optional[int] = None) -> bytes:
    """FF F8|F9, the code bytes, a one-byte frame number, CRC-8: the shortest complete header of a stream with table
    codes; want_crc: the frame number (and the blocking bit) that give this CRC-8."""
    for b1 in (0xF8, 0xF9):
        for fn in range(128):
            h = bytes([0xFF, b1, b2, b3, fn])
            if want_crc is None or B.crc8(h) == want_crc:
                return h + bytes([B.crc8(h)])
    raise AssertionError("no header with that CRC-8")


def code_header(first: bytes) -> bytes:
    """A complete header of the code bytes of the frame that starts `first` (frame number 0 where it has no other
    bytes to fill in)."""
    b2 = first[2]
    if b2 >> 4 not in (6, 7) and b2 & 15 < 12:
        return short_header(b2, first[3])
    num = 5 + max(0, 7 - (first[4] ^ 0xFF).bit_length())  # the byte after the coded number
    ext = {6: 1, 7: 2}.get(b2 >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(b2 & 15, 0)
    h = bytes([0xFF, 0xF8, b2, first[3], 0]) + first[num:num + ext]
    return h + bytes([B.crc8(h)])


def front_tail(lead: int, first: bytes) -> Tuple[bytes, List[int]]:
    """The front guard's last 32 bytes and the offsets (p < 0) of the complete headers in them.  The kernels load
    from p = -lead: where lead >= 6 leaves room a CRC-8-correct header of the stream's own code bytes lies there (lead
    6: one whose CRC-8 is 0xFF), and for lead >= 1 the guard's last byte is 0xFF."""
    t = bytearray(b"\x11" * 32)
    h = code_header(first)
    if lead == 6:
        at, h = -6, short_header(first[2], first[3], 0xFF)
    elif lead > len(h):
        at = -lead
    else:
        assert lead < 6
        at = -30  # (not in any load)
    t[32 + at:32 + at + len(h)] = h
    if lead >= 1:
        t[-1] = 0xFF
    assert bytes(t[32 + at:32 + at + len(h)]) == h
    return bytes(t), [at]


def back_guard(first: bytes, split: bool = False) -> bytes:
    """>= 32 bytes that begin with a complete header of the stream's code bytes, as the next tile's frame does in an
    arena; split: the header's 0xFF is the range's last byte (the last frame's CRC-16 low byte) and the guard
    completes it from F8."""
    h = code_header(first)
    return (h[1:] if split else h) + bytes(range(0x20, 0x20 + 40))


# ------------------------------------------------------------------------------------------------ the blob
@dataclass
class Blob:
    name: str
    form: str
    lead: int
    channels: int
    blocksize: int
    streams: Tuple[Str, ...]
    front: bytes                      # the front guard's last 32 bytes
    back: bytes
    guard_headers: Tuple[int, ...]    # p of the complete headers in the guards (outside [0, nbytes))
    end_split: bool = False
    cache: Dict = field(default_factory=dict)

    @property
    def body(self) -> bytes:
        if "body" not in self.cache:
            self.cache["body"] = b"".join(s.data for s in self.streams)
        return self.cache["body"]

    @property
    def nbytes(self) -> int:
        return self.rel_off[-1]

    @property
    def rel_off(self) -> List[int]:
        if "off" not in self.cache:
            self.cache["off"] = [0] + np.cumsum([len(s.data) for s in self.streams]).tolist()
        return self.cache["off"]

    @property
    def counts(self) -> List[int]:
        return [len(s.pcm) for s in self.streams]

    @property
    def pcm(self) -> np.ndarray:
        """[sum(counts), channels] int16 (read-only)"""
        if "pcm" not in self.cache:
            p = np.concatenate([s.pcm for s in self.streams])
            p.setflags(write=False)
            self.cache["pcm"] = p
        return self.cache["pcm"]

    @property
    def nframes(self) -> int:
        return sum(len(s.starts) for s in self.streams)

    def frames(self):
        """(p, header length, is a probe stream's frame) of every true frame"""
        for off, s in zip(self.rel_off, self.streams):
            for a, hl in zip(s.starts, s.hlens):
                yield off + a, hl, s.probe

    def false_syncs(self) -> List[int]:
        return [off + a for off, s in zip(self.rel_off, self.streams) for a in s.false_syncs]

    def assemble(self, guard_len: int) -> Tuple[bytes, List[int]]:
        """The blob with a front guard of guard_len >= 32 bytes, and stream_off (stream_off[0] = guard_len)."""
        assert guard_len >= 32
        front = b"\x5a" * (guard_len - 32) + self.front
        return front + self.body + self.back, [guard_len + o for o in self.rel_off]


def _finish(name, form, lead, streams, channels=1, blocksize=BS, split=False) -> Blob:
    first = streams[0].data
    front, at = front_tail(lead, first)
    b = Blob(name, form, lead, channels, blocksize, tuple(streams), front, back_guard(first, split), (), split)
    b.guard_headers = tuple(at) + ((b.nbytes - 1,) if split else (b.nbytes,))
    return b


@functools.lru_cache(maxsize=4)
def main_blob(form: str, lead: int) -> Blob:
    """The blob of a selection form that holds every position class applying to it."""
    body = _body(form)
    lay = Layout(lead, form)
    lay.add(first_stream(Q0 - lead, 12, lead))
    for s in body:
        lay.add(s)
    lay.pad_to(end_q(form, lead, lay.q))
    return _finish(form, form, lead, lay.streams)


def threshold_blob(total: int, lead: int) -> Blob:
    """Pure filler with nbytes + lead == total."""
    lay = Layout(lead, "small" if total <= 4 * MIB else "onepass" if total <= 16 * MIB else "twopass")
    lay.pad_to(total)
    return _finish("thr%d" % total, lay.form, lead, lay.streams)


def _free_sample_frame(n: int, hdr: dict, frame_no: int, *seed):
    """n VERBATIM samples whose frame (number frame_no) has a CRC-16 with the low byte 0xFF: the last sample is found
    by search."""
    x = _verb(n, 13, *seed)
    for v in range(-32768, 32768):
        c = _clean(np.array([v]))[0]
        if c != v:
            continue
        x[-1, 0] = v
        fr = B.frame([x[:, 0]], [VERB], frame_no, 16, **hdr)
        if fr[-1] == 0xFF:
            return x
    raise AssertionError("no sample gives that CRC-16")


EDGE_MODES = ("mod", "bk", "bk1")


@functools.lru_cache(maxsize=None)
def edge_blob(lead: int, mode: str = "mod") -> Blob:
    """G-start and G-end on the small form: a few streams, the first frame at p = 0 behind a guard that ends in a
    complete header, the back guard a header at p = nbytes (even leads) or completing one from the range's last byte
    (odd leads).  mode "mod": (nbytes + lead) mod 16 = (5 lead + 3) mod 16, every value over the 16 leads; "bk" /
    "bk1": nbytes + lead a multiple of the 16 KB block / one byte past it."""
    assert mode in EDGE_MODES
    split = bool(lead & 1)
    lay = Layout(lead, "small")
    lay.add(make_stream([(_verb(BS, 14, lead), [VERB], {}), (_smooth(BS, 14, lead), [FIXED], {}),
                         (_const(50, lead - 7), [CONST], {"bs_code": 7})], BS))
    lay.add(probe(1, 15, lead))
    last_hdr = {"bs_code": 7, "sr_code": 9}
    x = _free_sample_frame(24, last_hdr, 1, lead) if split else _verb(24, 13, lead)
    last = make_stream([(_smooth(BS, 16, lead), [FIXED], {}), (x, [VERB], last_hdr)], BS)
    if mode == "mod":
        end = -(-(lay.q + len(last.data) + 100) // 16) * 16 + (5 * lead + 3) % 16
    else:
        end = -(-(lay.q + len(last.data) + 100) // 16384) * 16384 + (mode == "bk1")
    lay.pad_to(end - len(last.data))
    lay.add(last)
    assert lay.q == end and (not split or last.data[-1] == 0xFF)
    return _finish("edge-%s" % mode, "small", lead, lay.streams, split=split)


@functools.lru_cache(maxsize=None)
def plain_blob() -> Blob:
    """Three ordinary streams: what a context decodes after a sequence, to show it is still in order."""
    lay = Layout(0, "small")
    for s in range(3):
        lay.add(make_stream([(_smooth(BS, 17, s, f), [FIXED], {}) for f in range(4)] +
                            [(_verb(300, 17, s), [VERB], {"bs_code": 7})], BS))
    return _finish("plain", "small", 0, lay.streams)


# ------------------------------------------------------------------------------------------------ 8 channels
def _frame8(n: int, *seed, verbatim: int = 8, hdr=None) -> Str:
    """A one-frame 8-channel stream: `verbatim` VERBATIM channels, the others CONSTANT."""
    x = _verb(n, 18, *seed, channels=8)
    x[:, verbatim:] = np.arange(8 - verbatim) * 100 - 300
    return make_stream([(x, [VERB] * verbatim + [CONST] * (8 - verbatim), hdr or {})], BS8)


@functools.lru_cache(maxsize=None)
def big8() -> Str:
    """One 8-channel VERBATIM frame of 4096 samples: 65552 bytes, longer than a 64 KB block."""
    return _frame8(BS8, 0)


@functools.lru_cache(maxsize=None)
def short8() -> Str:
    return _frame8(124, 1, hdr={"bs_code": 7, "sr_code": 13, "sr_extra": 44100})


def _short8(nbytes: int, *seed):
    """A short 8-channel frame of exactly nbytes (>= 33): one VERBATIM channel, seven CONSTANT ones -- 7 or 8 header
    bytes (block-size code 6 / 7) + 0 / 1 (sample-rate code 9 / 12) + 24 + 2 per sample."""
    for code, base in ((6, 31), (7, 32)):
        sx = (nbytes - base) % 2
        n = (nbytes - base - sx) // 2
        if 1 <= n <= (256 if code == 6 else BS8 - 1):
            x = _verb(n, 18, *seed, channels=8)
            x[:, 1:] = np.arange(7) * 100 - 300
            return x, [VERB] + [CONST] * 7, {"bs_code": code, **EXTRA[sx]}
    raise AssertionError("no 8-channel frame of %d bytes" % nbytes)


def spacer8(nbytes: int, *seed) -> Str:
    s = make_stream([_short8(nbytes, *seed)], BS8)
    assert len(s.data) == nbytes, (len(s.data), nbytes)
    return s


def first8(nbytes: int, *seed) -> Str:
    """Stream 0 of the 8-channel blob: a CONSTANT frame with the table-code header (32 bytes) and a short frame."""
    x = np.tile(np.arange(8) * 11 - 40, (BS8, 1))
    s = make_stream([(x, [CONST] * 8, {}), _short8(nbytes - 32, *seed)], BS8)
    assert len(s.data) == nbytes
    return s


@functools.lru_cache(maxsize=None)
def filler8() -> Str:
    return _frame8(400, 3)


@functools.lru_cache(maxsize=None)
def _body8() -> Tuple[Str, ...]:
    """G-cap: 64 KB blocks of exactly 31, 32 and 33 candidates (short one-frame streams from the block's first byte,
    then a 65552-byte frame that leaves the block), and a block of none (that frame from 12 bytes before a block: the
    whole next block lies inside it and its span crosses the block)."""
    lay = Layout(Q0, "twopass", spacer8, filler8)
    Bk = 65536
    assert Bk < len(big8().data) < Bk + 40 and 32 * len(short8().data) < Bk
    for c in (31, 32, 33):
        lay.pad_to(lay.boundary("block", lay.q + 200))
        for _ in range(c - 1):
            lay.add(short8())
        lay.add(big8())
    for at in (-12, -1):
        lay.pad_to(lay.boundary("block", lay.q + 200) + at)
        lay.add(big8())
    while lay.q < 16 * MIB + 3000:
        lay.add(big8())
    return tuple(lay.streams)


@functools.lru_cache(maxsize=2)
def cap8_blob(lead: int) -> Blob:
    lay = Layout(lead, "twopass", spacer8, filler8)
    lay.add(first8(Q0 - lead, 4, lead))
    for s in _body8():
        lay.add(s)
    lay.pad_to(end_q("twopass", lead, lay.q))
    return _finish("cap8", "twopass", lead, lay.streams, channels=8, blocksize=BS8)


# ------------------------------------------------------------------------------------------------ false syncs
def _spell(x: np.ndarray, at: int, hdr: bytes):
    """hdr written over the big-endian bytes of the mono samples x from sample `at`."""
    raw = bytearray(x[:, 0].astype(">i2").tobytes())
    raw[2 * at:2 * at + len(hdr)] = hdr
    x[:, 0] = np.frombuffer(bytes(raw), dtype=">i2")


def false_stream(two: bool, nframes: int, fidx: int, bs: int = BS, *seed) -> Str:
    """`nframes` frames of `bs` samples with table-code headers; frame fidx is VERBATIM and spells complete,
    CRC-8-correct headers of the stream's own code bytes in its samples (tests/test_gpu_decode_routes.py:
    _spelled_header).  One at a (F-a): nothing verifies from or to it.  two (F-b): a second one at b > a, and the
    sample in front of it is crc16(frame[a:b - 2]): the false candidate at a has the verified span [a, b), while no
    span from the frame's start ends at a or b, and none from b ends anywhere."""
    ia, ib = (1, 10) if bs < 64 else (40, 300)
    frames, hdr = [], {"bs_code": 6} if bs <= 256 and bs not in B.BS_TABLE else {}
    for f in range(nframes):
        if f == fidx:
            frames.append(None)
        elif bs < 64:
            frames.append((_const(bs, f % 1000 - 500), [CONST], hdr) if f % 3 else (_verb(bs, 19, f), [VERB], hdr))
        else:
            frames.append((_smooth(bs, 19, f, *seed), [FIXED], hdr) if f % 2 else
                          (_verb(bs, 19, f, *seed), [VERB], hdr))
    x = _verb(bs, 20, fidx, *seed)
    head = B.frame([x[:, 0]], [VERB], fidx, 16, **hdr)[:16]
    hl = header_len(fidx, hdr, bs, bs)
    spelled = code_header(head)
    _spell(x, ia, spelled)
    if two:
        _spell(x, ib, spelled)
        x[ib - 1, 0] = int(np.array(B.crc16(x[ia:ib - 1, 0].astype(">i2").tobytes()), dtype=np.uint16).astype(np.int16))
    frames[fidx] = (x, [VERB], hdr)
    s = make_stream(frames, bs, target=fidx)
    base = s.starts[fidx] + hl + 1  # (the VERBATIM subframe's header is one byte: the samples are byte-aligned)
    s.false_syncs = (base + 2 * ia,) + ((base + 2 * ib,) if two else ())
    for a in s.false_syncs:
        assert s.data[a:a + len(spelled)] == spelled
    return s


def _false_blob(name: str, lead: int, streams, bs: int = BS, form: str = "small") -> Blob:
    lay = Layout(lead, form)
    for s in streams:
        lay.add(s)
    return _finish(name, form, lead, lay.streams, blocksize=bs)


@functools.lru_cache(maxsize=None)
def false_blob(name: str, lead: int = 0) -> Blob:
    """fa: F-a in a stream of a multi-stream blob; fb-multi: F-b in a mid-stream frame of a multi-stream blob (the
    64-thread k_chain_lds); fb-one: in a one-stream blob (the 1024-thread form); fb-long: in a one-stream blob of more
    than 4096 candidates at block size 16 (the chain's global walk); false-big: F-a and F-b in a blob above 16 MiB.
    The streams do not depend on the lead (no position is aimed at); the guards do."""
    plain = plain_blob().streams
    if name == "fa":
        return _false_blob(name, lead, [plain[0], false_stream(False, 5, 2, BS, 1), plain[1]])
    if name == "fb-multi":
        return _false_blob(name, lead, [plain[0], false_stream(True, 5, 2, BS, 2), plain[1], plain[2]])
    if name == "fb-one":
        return _false_blob(name, lead, [false_stream(True, 6, 3, BS, 3)])
    if name == "fb-long":
        return _false_blob(name, lead, [_fb_long()], bs=16)
    assert name == "false-big"
    lay = Layout(lead, "twopass")
    for s in (plain[0], false_stream(False, 5, 2, BS, 1), plain[1], false_stream(True, 5, 2, BS, 2)):
        lay.add(s)
    lay.pad_to(16 * MIB + 5000)
    return _finish(name, "twopass", lead, lay.streams)


@functools.lru_cache(maxsize=None)
def _fb_long() -> Str:
    return false_stream(True, 4200, 2100, 16)


FALSE_BLOBS = ("fa", "fb-multi", "fb-one", "fb-long", "false-big")


# ------------------------------------------------------------------------------------------------ lookup, classes
THRESHOLDS = {"thr-4m": 4 * MIB, "thr-4m1": 4 * MIB + 1, "thr-16m": 16 * MIB, "thr-16m1": 16 * MIB + 1}


@functools.lru_cache(maxsize=3)
def get(name: str, lead: int = 0) -> Blob:
    """The blob `name` built for `lead` (callers must not change it)."""
    if name in FORMS:
        return main_blob(name, lead)
    if name == "cap8":
        return cap8_blob(lead)
    if name.startswith("edge-"):
        return edge_blob(lead, name[5:])
    if name in THRESHOLDS:
        return threshold_blob(THRESHOLDS[name], lead)
    if name == "plain":
        return plain_blob()
    return false_blob(name, lead)


def block_counts(blob: Blob, candidates) -> np.ndarray:
    """Candidates per 64 KB block of aligned space."""
    n = -(-(blob.nbytes + blob.lead) // 65536)
    return np.bincount((np.asarray(sorted(candidates), dtype=np.int64) + blob.lead) // 65536, minlength=n)


def classes_hit(blob: Blob) -> set:
    """The position classes a blob holds, from its frame starts, its stream offsets and its lead."""
    W, Bk = FORMS[blob.form]
    lead, nb = blob.lead, blob.nbytes
    hit = set()
    body = blob.body
    for p, hl, is_probe in blob.frames():
        q = p + lead
        hit.add(("lane", q % 16))
        if not is_probe or hl < 10:
            continue
        for d in OFFSETS:
            m = q - d
            if m > 0 and m % 1024 == 0:
                hit.add(("block" if m % Bk == 0 else "wave" if m % W == 0 else "step", d))
    ends = np.asarray(blob.rel_off[1:-1], dtype=np.int64) + lead
    for d in (-1, 0, 1):
        if np.any((ends - d) % Bk == 0):  # (the block of the form: 64 KB on the two large ones)
            hit.add(("bound", d))
    if len(ends) and np.bincount(ends // 1024).max() >= 3:
        hit.add(("bound", "three in a step"))
    starts = [p for p, _, _ in blob.frames()] + blob.false_syncs()
    counts = block_counts(blob, starts)
    if counts.max() > 8 * 32:
        hit.add(("bound", "dense"))
    for c in (0, 31, 32, 33):
        if c in counts[:-1]:
            hit.add(("cap", c))
    for p, _, _ in blob.frames():
        if counts[(p + lead) // 65536] > 32 and (p + lead) % 16384 >= 16384 - 16:
            hit.add(("cap", "a wave's last 16 bytes in a block read again"))
    # G-start: the first frame at p = 0 behind the guard's header and 0xFF
    guarded = (lead == 0 or blob.front[-1] == 0xFF) and (lead < 6 or -lead <= blob.guard_headers[0])
    if body[:2] == b"\xff\xf8" and guarded:
        hit.add(("start", lead))
    # G-end
    hit.add(("end", "split" if blob.end_split else "header"))
    hit.add(("end mod 16", (nb + lead) % 16))
    if (nb + lead) % Bk == 0:
        hit.add(("end", "block"))
    if (nb + lead) % Bk == 1:
        hit.add(("end", "block + 1"))
    return hit


POSITIONS = {(cls, d) for cls in ("block", "wave", "step") for d in OFFSETS} | {("lane", j) for j in range(16)}
BOUNDS = {("bound", -1), ("bound", 0), ("bound", 1), ("bound", "three in a step"), ("bound", "dense")}


# ------------------------------------------------------------------------------------------------ the GPU cases
ONE_PASS_SMALL, ONE_PASS, TWO_PASS = 0, 1, 2   # SelForm
PCRC, SPAN_LANE, SPAN_WAVE = 0, 1, 2           # SpanForm
PIPE, LANE, MULTI_LANE, WAVE = 0, 1, 2, 3      # FrameDec
# the DECODERS switches of tests/test_gpu_decode.py, and the default route
KINDS = {"default": {}, "pipe": {"FRS_DECODE_LANE": "0"}, "pipe_chain": {"FRS_DECODE_LANE": "0", "FRS_PIPE_OPT": "0"},
         "lane": {"FRS_DECODE_LANE": "1"}, "wave": {"FRS_FORCE_GENERIC": "1"}}
# (span check, frame decoder, optimistic) of a forced kind on a mono stream
KIND_ROUTE = {"pipe": (SPAN_WAVE, PIPE, 1), "pipe_chain": (SPAN_WAVE, PIPE, 0), "lane": (SPAN_LANE, LANE, 0),
              "wave": (SPAN_LANE, WAVE, 0)}
SMALL_LEADS = (0, 1, 2, 3, 4, 8, 13, 15)
BIG_LEADS = (0, 5, 15)
FALSE_LEADS = (0, 11)


@dataclass(frozen=True)
class Case:
    """One GPU decode: the blob, its lead, the decoder switches, FRS_SPAN_READ (0: unset), and the route it is meant
    to take (selection form, span check, frame decoder, optimistic)."""
    blob: str
    lead: int
    kind: str
    span_read: int
    route: Tuple[int, int, int, int]

    @property
    def id(self) -> str:
        span = "-span%d" % self.span_read if self.span_read else ""
        return "%s-lead%d-%s%s" % (self.blob, self.lead, self.kind, span)

    @property
    def env(self) -> Dict[str, str]:
        e = dict(KINDS[self.kind])
        if self.span_read:
            e["FRS_SPAN_READ"] = str(self.span_read)
        return e


def _cases():
    out = {}
    out["small"] = [Case("small", l, k, 0, (ONE_PASS_SMALL,) + KIND_ROUTE[k]) for k in KIND_ROUTE for l in SMALL_LEADS]
    out["edge"] = [Case("edge-" + m, l, k, 0, (ONE_PASS_SMALL,) + KIND_ROUTE[k]) for k in ("pipe", "lane")
                   for m, leads in (("mod", range(16)), ("bk", (0, 9)), ("bk1", (0, 9))) for l in leads]
    out["onepass"] = [Case("onepass", l, k, 0, (ONE_PASS,) + (KIND_ROUTE["pipe"] if k == "default" else KIND_ROUTE[k]))
                      for k in ("default", "lane") for l in BIG_LEADS]
    out["twopass"] = [Case("twopass", l, "lane", s, (TWO_PASS, SPAN_LANE if s == 1 else PCRC, LANE, 0))
                      for s in (1, 2) for l in BIG_LEADS]
    out["cap8"] = [Case("cap8", l, "default", 0, (TWO_PASS, PCRC, MULTI_LANE, 0)) for l in BIG_LEADS]
    thr = {"thr-4m": (ONE_PASS_SMALL,) + KIND_ROUTE["pipe"], "thr-4m1": (ONE_PASS,) + KIND_ROUTE["pipe"],
           "thr-16m": (ONE_PASS, SPAN_LANE, LANE, 0), "thr-16m1": (TWO_PASS, SPAN_LANE, LANE, 0)}
    out["threshold"] = [Case(n, l, "default", 0, r) for n, r in thr.items() for l in (0, 15)]
    out["false"] = [Case(n, l, k, 0, (ONE_PASS_SMALL,) + KIND_ROUTE[k]) for n in FALSE_BLOBS[:4] for k in KIND_ROUTE
                    for l in FALSE_LEADS]
    out["false-big"] = [Case("false-big", l, "lane", s, (TWO_PASS, SPAN_LANE if s == 1 else PCRC, LANE, 0))
                        for s in (1, 2) for l in FALSE_LEADS]
    return out


CASES = _cases()
