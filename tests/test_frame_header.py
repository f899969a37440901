"""csrc/frs_frame_header.h built by the host compiler alone: every block size, sample rate, sample size, channel
assignment and frame number form against headers assembled here from tests/flac_builder.py and RFC 9639's tables."""
import itertools
import struct
import subprocess
from pathlib import Path

import pytest

from tests.flac_builder import BS_TABLE, SS_TABLE, crc8, utf8_number

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_frame_header.h"

# RFC 9639 9.1.2: the sample rates with a code of their own
RATE_TABLE = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
              96000: 11}

BLOCK_SIZES = [4096, 192, 100, 1000]            # table, table, 8-bit explicit, 16-bit explicit
SAMPLE_RATES = [44100, 192000, 37000, 44110, 44101]  # table, table, kHz, Hz / 10, Hz
SAMPLE_SIZES = [16, 32]
CHANNEL_CODES = [0, 2, 8, 10]
FRAME_NUMBERS = [0, 127, 128, 2047, 2048, 65535, 65536]

PROG = f'''#include "{HEADER}"
#include <stdio.h>
int main() {{
    uint8_t t[256], h[16];
    frs::crc8_table(t);
    int bs, sr, bps, ch;
    unsigned fn;
    while (scanf("%d %d %d %d %u", &bs, &sr, &bps, &ch, &fn) == 5) {{
        const int hb = frs::frame_header(h, bs, sr, bps, ch, fn, t);
        for (int i = 0; i < hb; i++) printf("%02x", h[i]);
        printf(" %u\\n", frs::frame_header_bytes(fn, 0));
    }}
    return 0;
}}'''


def expected_header(bs: int, sr: int, bps: int, ch: int, fn: int) -> bytes:
    """RFC 9639 9.1 with a fixed block size: sync 0xFFF8, codes, coded number, the announced extras, CRC-8."""
    bs_extra = b""
    if bs in BS_TABLE:
        bs_code = BS_TABLE[bs]
    elif bs <= 256:
        bs_code, bs_extra = 6, bytes([bs - 1])
    else:
        bs_code, bs_extra = 7, (bs - 1).to_bytes(2, "big")
    sr_extra = b""
    if sr in RATE_TABLE:
        sr_code = RATE_TABLE[sr]
    elif sr % 1000 == 0 and sr // 1000 <= 255:
        sr_code, sr_extra = 12, bytes([sr // 1000])
    elif sr % 10 == 0 and sr // 10 <= 65535:  # libFLAC prefers tens of Hz to Hz where both hold the rate
        sr_code, sr_extra = 14, (sr // 10).to_bytes(2, "big")
    else:
        sr_code, sr_extra = 13, sr.to_bytes(2, "big")
    h = bytes([0xFF, 0xF8, bs_code << 4 | sr_code, ch << 4 | SS_TABLE[bps] << 1]) + utf8_number(fn) + bs_extra + sr_extra
    return h + bytes([crc8(h)])


@pytest.fixture(scope="module")
def headers(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_header")
    (d / "t.cpp").write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(d / "t"), str(d / "t.cpp")], check=True)
    grid = list(itertools.product(BLOCK_SIZES, SAMPLE_RATES, SAMPLE_SIZES, CHANNEL_CODES, FRAME_NUMBERS))
    text = "".join("%d %d %d %d %d\n" % g for g in grid)
    out = subprocess.run([str(d / "t")], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(grid) + 1 and out[-1] == ""
    return {g: line.split() for g, line in zip(grid, out)}


def test_header_does_not_need_hip():
    text = HEADER.read_text()
    assert "#include <hip" not in text and '#include "frs_' not in text


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("sr", SAMPLE_RATES)
def test_frame_header_bytes(headers, bs, sr):
    for bps, ch, fn in itertools.product(SAMPLE_SIZES, CHANNEL_CODES, FRAME_NUMBERS):
        got = bytes.fromhex(headers[(bs, sr, bps, ch, fn)][0])
        assert got == expected_header(bs, sr, bps, ch, fn), (bs, sr, bps, ch, fn, got.hex())


def test_expected_forms_are_distinct():
    """The grid reaches every form: each explicit block size and sample rate form adds its own bytes."""
    base = len(expected_header(4096, 44100, 16, 0, 0))
    assert [len(expected_header(b, 44100, 16, 0, 0)) - base for b in BLOCK_SIZES] == [0, 0, 1, 2]
    assert [len(expected_header(4096, s, 16, 0, 0)) - base for s in SAMPLE_RATES] == [0, 0, 1, 2, 2]
    assert [len(expected_header(4096, 44100, 16, 0, f)) - base for f in FRAME_NUMBERS] == [0, 0, 1, 1, 2, 2, 3]
    assert expected_header(4096, 44110, 16, 0, 0)[2] & 15 == 14 and expected_header(4096, 44101, 16, 0, 0)[2] & 15 == 13


def test_frame_header_bytes_is_the_length_of_a_4096_table_rate_header(headers):
    """k_encode_v4's length-only helper agrees with the writer (block size 4096, a rate with a code: srx 0)."""
    for sr, fn in itertools.product([44100, 192000], FRAME_NUMBERS):
        hexs, nbytes = headers[(4096, sr, 16, 0, fn)]
        assert int(nbytes) == len(hexs) // 2


# ------------------------------------------------------------------------------------------------ the readers
# parse_header (memory form) and header_ok_regs (register form) of the same header: each case is 16 bytes, the bound
# (`end` of the stream for the memory form, `avail` bytes of the blob for the register form: the same number here),
# the stream's channel count and its sample size.  The program answers with seven int32 per case.
READ_PROG = f'''#include "{HEADER}"
#include <stdio.h>
#include <string.h>
int main() {{
    uint8_t t[256], rec[19];
    frs::crc8_table(t);
    while (fread(rec, 1, sizeof(rec), stdin) == sizeof(rec)) {{
        uint8_t buf[16];
        uint32_t w[4];
        const int bound = rec[16], channels = rec[17], bps = rec[18];
        memset(buf, 0xEE, sizeof(buf));
        memcpy(buf, rec, bound);  // the memory form sees nothing at or past its bound
        memcpy(w, rec, 16);       // little-endian dwords, as the selection holds them
        const frs::FrameHdr h = frs::parse_header(buf, 0, bound, channels, bps, t);
        const int32_t out[7] = {{h.ok, h.ok ? h.frame_no : 0, h.ok ? h.bs : 0, h.ok ? h.hdr_len : 0, h.ok ? h.chass : 0,
                                h.ok ? h.bps : 0, (int32_t)frs::header_ok_regs(w, bound, channels)}};
        fwrite(out, sizeof(out), 1, stdout);
    }}
    return 0;
}}'''

RT_FRAME_NUMBERS = FRAME_NUMBERS + [0x1FFFFF, 0x200000, 0x3FFFFFF, 0x4000000]  # the 5- and 6-byte numbers
LEAD_BYTES = [0x7F, 0x80, 0xBF, 0xC0, 0xDF, 0xE0, 0xEF, 0xF0, 0xF7, 0xF8, 0xFB, 0xFC, 0xFD, 0xFE, 0xFF]
CHANNELS = [1, 2, 8]
SAMPLE_SIZE_BITS = {0: None, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}  # RFC 9639 9.1.4 (3 is reserved)


def rfc_reader(buf: bytes, bound: int, channels: int, stream_bps: int):
    """A frame header at buf[0], written from RFC 9639 9.1 and from nothing in csrc: None, or (frame number, block
    size, header bytes, channel assignment, sample size).  Bytes at or past `bound` do not exist.  The two
    restrictions both readers document are taken over: the coded number has at most 6 bytes (a 0xFE lead byte is
    rejected: frame numbers stay below 2^31), and the header's channel count has to be the stream's."""
    b = buf[:bound]
    try:
        if b[0] != 0xFF or b[1] & 0xFE != 0xF8:  # 15-bit sync code; either blocking strategy
            return None
        bsc, src, chass, ssc = b[2] >> 4, b[2] & 15, b[3] >> 4, b[3] >> 1 & 7
        if bsc == 0 or src == 15 or chass > 10 or ssc == 3 or b[3] & 1:  # reserved / forbidden codes, reserved bit
            return None
        lead = b[4]
        ones = 8 - (lead ^ 0xFF).bit_length()  # leading one bits
        if ones == 1 or ones > 6:  # a continuation byte; 7 bytes (0xFE) and 0xFF
            return None
        ncont = max(ones - 1, 0)
        v = lead & (0x7F >> ones)
        q = 5
        for _ in range(ncont):
            if b[q] & 0xC0 != 0x80:
                return None
            v, q = v << 6 | b[q] & 0x3F, q + 1
        if bsc == 1:
            bs = 192
        elif bsc <= 5:
            bs = 144 << bsc
        elif bsc == 6:
            bs, q = b[q] + 1, q + 1
        elif bsc == 7:
            bs, q = (b[q] << 8 | b[q + 1]) + 1, q + 2
        else:
            bs = 1 << bsc
        q += {12: 1, 13: 2, 14: 2}.get(src, 0)
        if _crc8(b[:q]) != b[q]:
            return None
    except IndexError:
        return None
    if (chass + 1 if chass < 8 else 2) != channels:
        return None
    return v, bs, q + 1, chass, SAMPLE_SIZE_BITS[ssc] or stream_bps


def _crc8_step(c: int) -> int:
    """One byte of CRC-8, polynomial x^8 + x^2 + x + 1, bit by bit (RFC 9639 9.1.8)."""
    for _ in range(8):
        c = (c << 1 ^ 0x07) & 0xFF if c & 0x80 else c << 1
    return c


_CRC8_STEP = [_crc8_step(c) for c in range(256)]


def _crc8(data: bytes) -> int:
    c = 0  # initial value 0
    for byte in data:
        c = _CRC8_STEP[c ^ byte]
    return c


def _ncont(lead: int) -> int:
    """Continuation bytes that a lead byte announces in the cases below (0xFE, 0xFF and 0x80..0xBF: none)."""
    for first, n in ((0xFE, 0), (0xFC, 5), (0xF8, 4), (0xF0, 3), (0xE0, 2), (0xC0, 1)):
        if lead >= first:
            return n
    return 0


_CRC8_OF = {}


def _case(b2, b3, num: bytes, bound=16, channels=1, crc_xor=0) -> bytes:
    """A 19-byte record: sync (the blocking-strategy bit alternates), codes, the coded number as given, the
    extension bytes the codes announce, the CRC-8 (xor crc_xor), filler up to 16; bound, channels, sample size."""
    h = bytes([0xFF, 0xF8 | (b2 ^ b3) & 1, b2, b3]) + num
    h += bytes([0x12, 0x34][:{6: 1, 7: 2}.get(b2 >> 4, 0)]) + bytes([0x56, 0x78][:{12: 1, 13: 2, 14: 2}.get(b2 & 15, 0)])
    c = _CRC8_OF.get(h)
    if c is None:
        c = _CRC8_OF[h] = _crc8(h)
    h = (h + bytes([c ^ crc_xor]) + b"\xa5" * 16)[:16]
    return h + bytes([bound, channels, 16])


def _reader_cases():
    cases = []
    # every (byte 2, byte 3) pair with a valid remainder, for each channel count
    for b2, b3, ch in itertools.product(range(256), range(256), CHANNELS):
        cases.append(_case(b2, b3, b"\x05", channels=ch))
    # the same pairs with a two-byte number, the bound at and around the header's end
    for b2, b3, bound in itertools.product(range(256), range(256), (6, 7, 8, 9, 10, 11)):
        cases.append(_case(b2, b3, b"\xc2\x85", bound=bound, channels=(b3 >> 4) + 1 if b3 >> 4 < 8 else 2))
    # every lead-byte class boundary x extension forms x channel codes x channel counts x every bound: a valid
    # remainder, one broken continuation byte at each position, a wrong CRC-8
    for lead, bsc, src, b3, ch in itertools.product(LEAD_BYTES, (1, 6, 7), (9, 12, 13), (0x08, 0x18, 0x78), CHANNELS):
        b2 = bsc << 4 | src
        ncont = _ncont(lead)
        good = bytes([lead]) + b"\x91" * ncont
        forms = [(good, 0), (good, 0x01)]
        for i, bad in itertools.product(range(5), (0x11, 0x7F, 0xC1, 0xFF)):
            num = bytearray(bytes([lead]) + b"\x91" * 5)  # (positions past ncont: bytes no reader may look at)
            num[1 + i] = bad
            forms.append((bytes(num[:1 + max(ncont, i + 1)]) if i >= ncont else bytes(num[:1 + ncont]), 0))
        for (num, cx), bound in itertools.product(forms, range(17)):
            cases.append(_case(b2, b3, num, bound=bound, channels=ch, crc_xor=cx))
    return cases


def _build(tmp_path_factory, name, text):
    d = tmp_path_factory.mktemp(name)
    (d / "t.cpp").write_text(text)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(d / "t"), str(d / "t.cpp")], check=True)
    return str(d / "t")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    exe = _build(tmp_path_factory, "frame_header_read", READ_PROG)

    def run(records):
        out = subprocess.run([exe], input=b"".join(records), capture_output=True, check=True).stdout
        assert len(out) == 28 * len(records)
        return list(struct.iter_unpack("<7i", out))
    return run


def test_readers_round_trip_the_writer(headers, reader, tmp_path_factory):
    """(a) every header the writer produces parses back to the values written, in both forms."""
    exe = _build(tmp_path_factory, "frame_header_rt", PROG)
    grid = list(itertools.product(BLOCK_SIZES, SAMPLE_RATES, SAMPLE_SIZES, CHANNEL_CODES, RT_FRAME_NUMBERS))
    text = "".join("%d %d %d %d %d\n" % g for g in grid)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(lines) == len(grid) + 1
    recs = []
    for (bs, sr, bps, ch, fn), line in zip(grid, lines):
        h = bytes.fromhex(line.split()[0])
        assert h == expected_header(bs, sr, bps, ch, fn) and len(h) <= 16
        recs.append((h + b"\x00" * 16)[:16] + bytes([len(h), ch + 1 if ch < 8 else 2, 20]))
    for (bs, sr, bps, ch, fn), rec, got in zip(grid, recs, reader(recs)):
        assert got == (1, fn, bs, rec[16], ch, bps, 1), (bs, sr, bps, ch, fn, got)
    assert [len(utf8_number(f)) for f in RT_FRAME_NUMBERS[-4:]] == [4, 5, 5, 6]


def test_readers_accept_what_rfc_9639_accepts(reader):
    """(b) both forms against rfc_reader: the same headers accepted, the same fields read."""
    cases = _reader_cases()
    assert len(cases) == 3 * 65536 + 6 * 65536 + 15 * 3 * 3 * 3 * 3 * 22 * 17 == 1044234
    accepted = 0
    for rec, got in zip(cases, reader(cases)):
        ref = rfc_reader(rec[:16], rec[16], rec[17], rec[18])
        want = (1,) + ref + (1,) if ref else (0, 0, 0, 0, 0, 0, 0)
        if got != want:
            raise AssertionError((rec.hex(), got, want))
        accepted += ref is not None
    assert 50000 < accepted < len(cases) - 50000  # the cases sit on both sides of the test
