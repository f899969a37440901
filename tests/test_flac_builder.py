"""The hand-built streams of tests/flac_layouts.py against the oracle's decoder (CPU).

For every stream the GPU tests decode: the oracle decodes it to the samples that went in, and reports the forced
subframe type and partition order.  This keeps a GPU failure attributable to the kernel: the writer
(tests/flac_builder.py, from RFC 9639) and the oracle's decoder are two independent restatements of the format, and
the known samples are the truth.  The oracle's escape-partition and Rice-method-1 paths are pinned by no fixture of
the reference (its encoder emits neither); their agreement with the writer and the known samples here is the check.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flac_builder as B
from tests import flac_layouts as L


def test_crc_check_values():
    """CRC-8 (poly 0x07) and CRC-16 (poly 0x8005), both zero-initialised: the catalogued check values."""
    assert B.crc8(b"123456789") == 0xF4
    assert B.crc16(b"123456789") == 0xFEE8


def test_utf8_number_boundaries():
    assert B.utf8_number(0) == b"\x00" and B.utf8_number(127) == b"\x7f"
    assert B.utf8_number(128) == b"\xc2\x80" and B.utf8_number(2047) == b"\xdf\xbf"
    assert B.utf8_number(2048) == b"\xe0\xa0\x80" and B.utf8_number(65535) == b"\xef\xbf\xbf"
    assert B.utf8_number(65536) == b"\xf0\x90\x80\x80"
    assert B.utf8_number((1 << 36) - 1) == b"\xfe" + b"\xbf" * 6


def test_bitwriter_fields():
    bw = B.BitWriter()
    bw.put(0b101, 3)
    bw.put(0, 70)                                 # a unary run wider than a word
    bw.put_array(np.array([1, 0x1FFFFFFFF]), np.array([1, 33]))
    bw.put(-1, 2)                                 # masked to its width
    bits = "101" + "0" * 70 + "1" + "1" * 33 + "11"
    bits += "0" * (-len(bits) % 8)
    assert bw.to_bytes() == int(bits, 2).to_bytes(len(bits) // 8, "big")


def test_golden_frame_header_and_footer(golden):
    """The writer's header fields and both CRCs against a frame libFLAC wrote (sample_rgb.flac: 3 channels, 16-bit,
    4096-sample frames after an 86-byte stream header): rebuilding the header bytes and the footer from the frame's
    own fields gives the file's bytes."""
    data = (golden / "sample_rgb.flac").read_bytes()[86:]
    assert data[:2] == b"\xff\xf8"
    hdr = bytes([0xFF, 0xF8, (B.BS_TABLE[4096] << 4) | (data[2] & 15), (2 << 4) | (B.SS_TABLE[16] << 1)])
    hdr += B.utf8_number(0)
    assert data[:6] == hdr + bytes([B.crc8(hdr)])
    end = data.find(hdr[:4] + B.utf8_number(1))   # the second frame
    assert end > 0 and B.crc16(data[:end - 2]) == int.from_bytes(data[end - 2:end], "big")


@pytest.mark.parametrize("name", list(L.STREAMS))
def test_oracle_decodes_known_samples(name):
    s = L.get(name)
    n = len(s.pcm)
    assert s.nframes >= 65 and s.nframes == -(-n // s.blocksize)
    got = O.decode_frames(s.data, s.channels, s.bps, n)
    assert np.array_equal(got, s.pcm.astype(np.int32))
    assert np.array_equal(O.subframe_types(s.data, s.channels, s.bps, n, s.blocksize), s.forced)


@pytest.mark.parametrize("name", list(L.STREAMS))
def test_census_reports_the_forced_layout(name):
    """O.subframe_census against what the writer was told to write, field by field, for every subframe: type, order,
    wasted bits, LPC precision, shift and coefficients, residual method, partition order, every partition's Rice
    parameter or escape width, the frame's assignment code, frame and channel numbers and the block size."""
    s = L.get(name)
    n = len(s.pcm)
    cen = O.subframe_census(s.data, s.channels, s.bps, n)
    assert len(cen) == len(s.layout) == len(s.forced)
    bad = []
    for i, (c, (chass, sub, params)) in enumerate(zip(cen, s.layout)):
        f = i // s.channels
        resid = sub.kind in ("fixed", "lpc")
        lpc = sub.kind == "lpc"
        want = dict(frame=f, channel=i % s.channels, assignment=chass, blocksize=min(s.blocksize, n - f * s.blocksize),
                    type=sub.type_code, kind=sub.kind, order=sub.order if resid else 0, wasted=sub.wasted,
                    precision=sub.precision if lpc else 0, shift=sub.shift if lpc else 0,
                    coefs=tuple(int(q) for q in sub.coefs) if lpc else (), method=sub.method if resid else -1,
                    porder=sub.porder if resid else -1, params=list(params))
        if c != want:
            bad.append((i, {k: (c[k], want[k]) for k in want if c[k] != want[k]}))
    assert not bad, bad[:5]


def test_census_pin_covers_the_rare_forms():
    """The streams the pin above runs on do hold what the encoder never emits: escape partitions (width 0 too), 5-bit
    parameters up to 30, LPC orders above 8, partition orders 6, 7 and 8, shifts 0 and 15, both coefficient extremes,
    wasted bits on every subframe kind and all four two-channel assignment codes."""
    subs = [(chass, sub, params) for name in L.STREAMS for chass, sub, params in L.get(name).layout]
    escapes = {p[1] for _, _, params in subs for p in params if isinstance(p, tuple)}
    assert 0 in escapes and len(escapes) > 3
    assert {14, 15, 16, 30} <= {p for _, s, params in subs if s.method == 1 for p in params if not isinstance(p, tuple)}
    assert {9, 12, 32} <= {s.order for _, s, _ in subs if s.kind == "lpc"}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} <= {s.porder for _, s, _ in subs if s.kind in ("fixed", "lpc")}
    assert {0, 15} <= {s.shift for _, s, _ in subs if s.kind == "lpc"}
    assert {-16384, 16383} <= {q for _, s, _ in subs if s.kind == "lpc" for q in s.coefs}
    assert {"constant", "verbatim", "fixed", "lpc"} == {s.kind for _, s, _ in subs if s.wasted}
    assert {1, 8, 9, 10} <= {chass for chass, _, _ in subs}


def _golden_streams(golden):
    """(name, channels, bps, frames) of sample_rgb.flac (one 16-bit stream after an 86-byte header) and of the 32-bit
    tile streams of sample_dem.flac that begin with a bare 86-byte header (every stream but the first, whose header
    carries the tags)."""
    yield "sample_rgb", 3, 16, (golden / "sample_rgb.flac").read_bytes()[86:]
    dem = (golden / "sample_dem.flac").read_bytes()
    starts = [i for i in range(1, len(dem)) if dem[i:i + 4] == b"fLaC"] + [len(dem)]
    assert len(starts) == 4
    for k in range(3):
        yield f"sample_dem[{k + 1}]", 1, 32, dem[starts[k] + 86:starts[k + 1]]


def test_census_agrees_with_the_older_walkers_on_the_golden_files(golden):
    """On libFLAC's own output: type and partition order equal subframe_types', the assignment frame_assignments', and
    the fields hang together (a partition per 2^order, FIXED without LPC fields, 4-bit parameters below 15)."""
    for name, channels, bps, data in _golden_streams(golden):
        _census_agrees(name, channels, bps, data)


def _census_agrees(name, channels, bps, data):
    cap = 1 << 22
    n = len(O.decode_frames(data, channels, bps, cap))
    cen = O.subframe_census(data, channels, bps, n)
    types = O.subframe_types(data, channels, bps, n)
    ca = O.frame_assignments(data, channels, bps, n)
    assert len(cen) == len(types) > 0
    assert [(c["type"], c["porder"]) for c in cen] == [tuple(t) for t in types.tolist()]
    assert [c["assignment"] for c in cen] == [int(ca[c["frame"]]) for c in cen]
    assert [c["channel"] for c in cen] == [i % channels for i in range(len(cen))]
    for c in cen:
        resid = c["kind"] in ("fixed", "lpc")
        assert len(c["params"]) == (1 << c["porder"] if resid else 0)
        assert (c["method"] in (0, 1)) == resid
        if c["kind"] == "lpc":
            assert len(c["coefs"]) == c["order"] == c["type"] - 31 and 1 <= c["precision"] <= 15
        else:
            assert c["coefs"] == () and c["precision"] == 0 and c["shift"] == 0
        if c["method"] == 0:
            assert all(isinstance(p, tuple) or p < 15 for p in c["params"])


def test_wrapping_lpc_frames_need_64_bits():
    fr = B.wrapping_lpc_frames(3, 64)
    assert np.all(O.decode_frames(fr, 1, 16, 192) == 32767)
    assert np.array_equal(O.subframe_types(fr, 1, 16, 192, 64), [[39, 0]] * 3)
    assert 8 * 16383 * 32767 > 2 ** 31
