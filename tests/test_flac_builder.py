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


def test_wrapping_lpc_frames_need_64_bits():
    fr = B.wrapping_lpc_frames(3, 64)
    assert np.all(O.decode_frames(fr, 1, 16, 192) == 32767)
    assert np.array_equal(O.subframe_types(fr, 1, 16, 192, 64), [[39, 0]] * 3)
    assert 8 * 16383 * 32767 > 2 ** 31
