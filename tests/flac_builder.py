"""A forced-choice FLAC frame writer for tests, written from RFC 9639 (sections 9.1 frame header, 9.2 subframes,
9.2.7 coded residual, 9.3 frame footer).  Pure Python + numpy; it imports nothing from the oracle or the product.

The caller passes the samples of every channel and, per subframe, the layout to force (`Sub`): the writer makes no
choice of its own except a Rice parameter where the caller leaves one open.  Residuals are computed in int64 with
numpy, the bits packed with numpy, CRC-8 and CRC-16 appended.  The truth of every test built on this file is the
samples that went in, not another decoder's output.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Union

import numpy as np

FIXED_COEFS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
BS_TABLE = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
            16384: 14, 32768: 15}
SS_TABLE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def _crc_table(poly: int, width: int):
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def utf8_number(v: int) -> bytes:
    """The frame / sample number coding of RFC 9639 9.1.5 (UTF-8's scheme extended to 36 bits)."""
    if v < 0x80:
        return bytes([v])
    for nbytes, lead in ((2, 0xC0), (3, 0xE0), (4, 0xF0), (5, 0xF8), (6, 0xFC), (7, 0xFE)):
        if v < 1 << (5 * nbytes + 1 if nbytes < 7 else 36):
            cont = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(nbytes - 2, -1, -1)]
            return bytes([lead | (v >> (6 * (nbytes - 1)))] + cont)
    raise ValueError("number too large")


class BitWriter:
    """MSB-first fields; a field of value 0 may have any width (a unary run), any other at most 64 bits."""

    def __init__(self):
        self._chunks = []
        self._v: List[int] = []
        self._w: List[int] = []

    def put(self, v: int, n: int):
        assert n >= 0 and (n <= 64 or v == 0)
        self._v.append(int(v) & ((1 << min(n, 64)) - 1))
        self._w.append(n)

    def _flush(self):
        if self._v:
            self._chunks.append((np.array(self._v, dtype=np.uint64), np.array(self._w, dtype=np.int64)))
            self._v, self._w = [], []

    def put_array(self, vals: np.ndarray, widths: np.ndarray):
        self._flush()
        self._chunks.append((np.asarray(vals, dtype=np.uint64), np.asarray(widths, dtype=np.int64)))

    def to_bytes(self) -> bytes:
        """Zero-padded to a byte boundary."""
        self._flush()
        if not self._chunks:
            return b""
        vals = np.concatenate([c[0] for c in self._chunks])
        widths = np.concatenate([c[1] for c in self._chunks])
        ends = np.cumsum(widths)
        bits = np.zeros((int(ends[-1]) + 7) // 8 * 8, dtype=np.uint8)
        nz = vals != 0
        top = int(widths[nz].max()) if nz.any() else 0
        for j in range(top):
            m = nz & (widths > j) & (((vals >> np.uint64(j)) & np.uint64(1)) != 0)
            bits[ends[m] - 1 - j] = 1
        return np.packbits(bits).tobytes()


@dataclass
class Sub:
    """One subframe's forced layout.  kind: "constant" | "verbatim" | "fixed" | "lpc".  params: one entry per
    partition (2**porder of them): a Rice parameter, ("esc", width) for an escape partition with that raw width
    (None: the narrowest that holds the residuals), or None for the cheapest Rice parameter of the method.  A single
    entry (or None) is used for every partition."""
    kind: str
    order: int = 0
    precision: int = 0
    shift: int = 0
    coefs: Sequence[int] = ()
    wasted: int = 0
    method: int = 0
    porder: int = 0
    params: Union[None, int, tuple, Sequence] = None

    @property
    def type_code(self) -> int:
        return {"constant": 0, "verbatim": 1, "fixed": 8 + self.order, "lpc": 31 + self.order}[self.kind]


def residuals(x: np.ndarray, coefs: Sequence[int], shift: int) -> np.ndarray:
    """x[i] - (sum_j coefs[j] * x[i-1-j] >> shift) for i >= len(coefs), in int64 (arithmetic shift: RFC 9639 9.2.6)."""
    x = np.asarray(x, dtype=np.int64)
    o, n = len(coefs), len(x)
    pred = np.zeros(n - o, dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += int(c) * x[o - 1 - j:n - 1 - j]
    return x[o:] - (pred >> shift)


def _signed_width(r: np.ndarray) -> int:
    if r.size == 0 or not r.any():
        return 0
    lo, hi = int(r.min()), int(r.max())
    w = 1
    while not (-(1 << (w - 1)) <= lo and hi < (1 << (w - 1))):
        w += 1
    return w


def _write_residual(bw: BitWriter, res: np.ndarray, bs: int, order: int, sub: Sub):
    assert sub.method in (0, 1)
    pb = 4 if sub.method == 0 else 5
    esc = (1 << pb) - 1
    po = sub.porder
    assert bs % (1 << po) == 0 and (bs >> po) >= order, "partition order does not fit block size / predictor order"
    assert res.size == 0 or (int(res.min()) > -(1 << 31) and int(res.max()) < (1 << 31)), "residual beyond 32 bits"
    bw.put(sub.method, 2)
    bw.put(po, 4)
    params = sub.params
    if params is None or isinstance(params, (int, tuple)):
        params = [params] * (1 << po)
    assert len(params) == 1 << po
    at, written = 0, []
    for p, par in enumerate(params):
        ns = (bs >> po) - (order if p == 0 else 0)
        r = res[at:at + ns]
        at += ns
        if isinstance(par, tuple):
            assert par[0] == "esc"
            nb = _signed_width(r) if par[1] is None else par[1]
            assert 0 <= nb <= 31 and _signed_width(r) <= nb, "escape width too narrow"
            bw.put(esc, pb)
            bw.put(nb, 5)
            written.append(("esc", nb))
            if nb:
                bw.put_array(r.astype(np.uint64) & np.uint64((1 << nb) - 1), np.full(ns, nb))
            continue
        u = ((r << 1) ^ (r >> 63)).astype(np.uint64)  # zigzag fold
        if par is None:
            cost = [int((u >> np.uint64(k)).sum()) + (k + 1) * ns for k in range(esc)]
            par = int(np.argmin(cost))
        assert 0 <= par < esc
        bw.put(par, pb)
        written.append(par)
        k = np.uint64(par)
        vals = np.zeros(2 * ns, dtype=np.uint64)
        widths = np.empty(2 * ns, dtype=np.int64)
        widths[0::2] = (u >> k).astype(np.int64)                               # unary zeros
        vals[1::2] = (np.uint64(1) << k) | (u & ((np.uint64(1) << k) - np.uint64(1)))  # stop bit + low bits
        widths[1::2] = par + 1
        bw.put_array(vals, widths)
    assert at == res.size
    return written


def _write_subframe(bw: BitWriter, x: np.ndarray, sbps: int, sub: Sub):
    """-> the partitions' parameters as written (a Rice parameter or ("esc", width) each; [] without a residual)"""
    x = np.asarray(x, dtype=np.int64)
    bs = len(x)
    w = sub.wasted
    bw.put(0, 1)
    bw.put(sub.type_code, 6)
    if w:
        assert not (x & ((1 << w) - 1)).any(), "samples do not have the wasted bits"
        bw.put(1, 1)
        bw.put(0, w - 1)
        bw.put(1, 1)
        x = x >> w
        sbps -= w
    else:
        bw.put(0, 1)
    assert sbps >= 1
    assert x.size == 0 or (int(x.min()) >= -(1 << (sbps - 1)) and int(x.max()) < (1 << (sbps - 1))), "sample range"
    raw = lambda v: bw.put_array(np.asarray(v).astype(np.uint64) & np.uint64((1 << sbps) - 1), np.full(len(v), sbps))
    if sub.kind == "constant":
        assert (x == x[0]).all()
        raw(x[:1])
    elif sub.kind == "verbatim":
        raw(x)
    elif sub.kind == "fixed":
        o = sub.order
        assert 0 <= o <= 4 and o <= bs
        raw(x[:o])
        return _write_residual(bw, residuals(x, FIXED_COEFS[o], 0), bs, o, sub)
    elif sub.kind == "lpc":
        o, prec = sub.order, sub.precision
        assert 1 <= o <= 32 and o <= bs and len(sub.coefs) == o and 1 <= prec <= 15 and 0 <= sub.shift <= 31
        assert all(-(1 << (prec - 1)) <= c < (1 << (prec - 1)) for c in sub.coefs), "coefficient beyond precision"
        raw(x[:o])
        bw.put(prec - 1, 4)
        bw.put(sub.shift, 5)
        for c in sub.coefs:
            bw.put(c & ((1 << prec) - 1), prec)
        return _write_residual(bw, residuals(x, sub.coefs, sub.shift), bs, o, sub)
    else:
        raise ValueError(sub.kind)
    return []


def frame(channels: Sequence[np.ndarray], subs: Sequence[Sub], frame_no: int, bps: int, *, chass: Optional[int] = None,
          bs_code: Optional[int] = None, sr_code: int = 9, sr_extra: Optional[int] = None,
          ss_code: Optional[int] = None, written: Optional[list] = None) -> bytes:
    """One frame.  channels: the samples per channel (for chass 8..10: left and right; the writer forms side, of
    bps + 1 bits, and mid).  bs_code: a table code, 6 / 7 for the explicit 8- / 16-bit forms, None = the table code
    where one exists, else the narrowest explicit form.  sr_code 12..14 carry sr_extra (kHz in 8 bits, Hz in 16,
    Hz / 10 in 16).  ss_code: None = the code of bps, 0 = "from the stream".  written: a list that receives, per subframe,
    (the assignment code, the Sub, its partitions' parameters as written)."""
    ch = [np.asarray(c, dtype=np.int64) for c in channels]
    bs = len(ch[0])
    assert all(len(c) == bs for c in ch) and 1 <= bs <= 65536 and len(subs) == len(ch)
    if chass is None:
        chass = len(ch) - 1
    assert (chass < 8 and chass == len(ch) - 1) or (8 <= chass <= 10 and len(ch) == 2)
    if bs_code is None:
        bs_code = BS_TABLE.get(bs, 6 if bs <= 256 else 7)
    if bs_code == 6:
        assert bs <= 256
    elif bs_code != 7:
        assert BS_TABLE.get(bs) == bs_code, "block size is not this table code's"
    if ss_code is None:
        ss_code = SS_TABLE[bps]
    assert ss_code == 0 or SS_TABLE[bps] == ss_code
    hdr = bytearray([0xFF, 0xF8, (bs_code << 4) | sr_code, (chass << 4) | (ss_code << 1)])
    hdr += utf8_number(frame_no)
    if bs_code == 6:
        hdr += bytes([bs - 1])
    elif bs_code == 7:
        hdr += (bs - 1).to_bytes(2, "big")
    if sr_code == 12:
        hdr += bytes([sr_extra])
    elif sr_code in (13, 14):
        hdr += int(sr_extra).to_bytes(2, "big")
    else:
        assert sr_code < 12
    hdr += bytes([crc8(hdr)])
    widths = [bps] * len(ch)
    if chass >= 8:
        left, right = ch
        side = left - right
        if chass == 8:
            ch, widths = [left, side], [bps, bps + 1]
        elif chass == 9:
            ch, widths = [side, right], [bps + 1, bps]
        else:
            ch, widths = [(left + right) >> 1, side], [bps, bps + 1]
    bw = BitWriter()
    for x, sbps, sub in zip(ch, widths, subs):
        params = _write_subframe(bw, x, sbps, sub)
        if written is not None:
            written.append((chass, sub, params))
    body = bytes(hdr) + bw.to_bytes()
    return body + crc16(body).to_bytes(2, "big")


@dataclass
class Stream:
    """Frames of one stream with the samples that went in (pcm: [N, channels] int64) and, per subframe in frame-major
    order, the forced (type code, partition order; -1 for CONSTANT / VERBATIM).  layout: per subframe in the same order,
    (assignment code, the Sub it was written from, its partitions' parameters as written: where the Sub left a Rice
    parameter or an escape width open, the writer's choice)."""
    data: bytes
    pcm: np.ndarray
    bps: int
    blocksize: int
    forced: np.ndarray
    name: str = ""
    layout: list = field(default_factory=list)

    @property
    def channels(self) -> int:
        return self.pcm.shape[1]

    @property
    def nframes(self) -> int:
        return len(self.forced) // self.channels


def stream_from_frames(frames, bps: int, blocksize: int, name: str = "", **hdr) -> Stream:
    """frames: (samples [n] or [n, C], list of Sub per channel[, dict of frame() header arguments]) per frame, numbered
    from 0; every frame but the last has `blocksize` samples.  hdr: header arguments for every frame."""
    out, forced, blocks, layout = bytearray(), [], [], []
    for f, fr in enumerate(frames):
        blk = np.asarray(fr[0], dtype=np.int64)
        if blk.ndim == 1:
            blk = blk[:, None]
        subs, kw = fr[1], (fr[2] if len(fr) > 2 else {})
        assert len(blk) == blocksize or (f == len(frames) - 1 and 0 < len(blk) < blocksize)
        out += frame([blk[:, c] for c in range(blk.shape[1])], subs, f, bps, written=layout, **{**hdr, **kw})
        forced += [(s.type_code, s.porder if s.kind in ("fixed", "lpc") else -1) for s in subs]
        blocks.append(blk)
    return Stream(bytes(out), np.concatenate(blocks), bps, blocksize,
                  np.array(forced, dtype=np.int64).reshape(-1, 2), name, layout)


def stream(pcm: np.ndarray, bps: int, blocksize: int, layout, name: str = "", **hdr) -> Stream:
    """Cut pcm ([N] or [N, C]) into frames of `blocksize` (a shorter last one) and write each with
    layout(frame_index, frame_samples[n, C]) -> list of Sub per channel, or (list of Sub, dict of frame() header
    arguments)."""
    pcm = np.asarray(pcm, dtype=np.int64)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    frames = []
    for f, a in enumerate(range(0, len(pcm), blocksize)):
        blk = pcm[a:a + blocksize]
        lay = layout(f, blk)
        frames.append((blk,) + (lay if isinstance(lay, tuple) else (lay,)))
    return stream_from_frames(frames, bps, blocksize, name, **hdr)


def wrapping_lpc_frames(nframes: int, bs: int = 64) -> bytes:
    """Mono 16-bit frames whose LPC prediction sum needs more than 32 bits: order 8, 15-bit coefficients of 16383,
    shift 14, every sample 32767 -> sum q.x = 8 * 16383 * 32767 > 2^31.  libFLAC decodes them with its 64-bit
    restore (prec + bps + log2(order) > 32); a decoder summing mod 2^32 must notice."""
    sub = Sub("lpc", order=8, precision=15, shift=14, coefs=[16383] * 8, params=14)
    return stream(np.full(nframes * bs, 32767), 16, bs, lambda f, blk: [sub], bs_code=7).data
