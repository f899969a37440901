"""csrc/frs_frame_header.h built by the host compiler alone: every block size, sample rate, sample size, channel
assignment and frame number form against headers assembled here from tests/flac_builder.py and RFC 9639's tables."""
import itertools
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
