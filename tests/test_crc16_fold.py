"""csrc/frs_crc16_fold.h built by the host compiler alone (with UBSan and ASan where it links them): the table-free
CRC-16 against a bitwise CRC-16 written here (polynomial 0x8005, init 0, MSB first), on byte strings, word strings and
the column decomposition of k_encode_v4 (64 ranges of C words over the zero-padded frame buffer, each taken as a
column of N rows, recombined with x^(8 m) factors of either sign)."""
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_crc16_fold.h"

# One request per line: a command, its integer arguments, the message in hex.
#   B          crc16_words over the whole words, crc16_tail over the 0..3 bytes left
#   W          crc16_words (the message is whole words), also at stride 3
#   C n c      the kernel's decomposition with N = n rows: column L = words [L c, L c + c) of the buffer (the message,
#              zero-padded to 64 c words; word w at row w mod c of column w / c), CRC of each by crc16_column<n, 8>
#              (which may read up to 7 zero rows past c), shifted by x^(8 (len - 4 c L - 4 n)) and XORed
#   X e        crc16_xpow(e) and crc16_xpow(-e)
PROG = f'''#include "{HEADER}"
#include <stdio.h>
#include <string.h>
#include <vector>
static std::vector<uint8_t> unhex(const char *s) {{
    std::vector<uint8_t> v;
    unsigned b;
    for (; s[0] && s[1] && sscanf(s, "%2x", &b) == 1; s += 2) v.push_back((uint8_t)b);
    return v;
}}
static std::vector<uint32_t> be_words(const std::vector<uint8_t> &m, size_t nwords) {{
    std::vector<uint32_t> w(nwords, 0u);
    for (size_t i = 0; i < m.size() && i / 4 < nwords; i++) w[i / 4] |= (uint32_t)m[i] << (24 - 8 * (i % 4));
    return w;
}}
template <int N>
static uint32_t columns(const std::vector<uint8_t> &m, int c) {{
    // the kernel's layout: word w at row w mod c, column w / c of a 64-column matrix (+ the zero rows that a group of
    // 8 may read past c)
    const std::vector<uint32_t> lin = be_words(m, 64 * (size_t)c);
    std::vector<uint32_t> buf(64 * ((size_t)c + 8), 0u);
    for (size_t w = 0; w < lin.size(); w++) buf[(w % c) * 64 + w / c] = lin[w];
    uint32_t crc = 0;
    for (int L = 0; L < 64; L++) {{
        const uint32_t v = frs::crc16_column<N, 8>(buf.data() + L, 64, c);
        const long mbytes = (long)m.size() - 4L * c * L - 4L * N;
        // (a column past the message holds zeros only: its CRC is 0 whatever the factor)
        crc ^= frs::crc16_mulmod(v, frs::crc16_xpow(8 * mbytes));
    }}
    return crc;
}}
int main() {{
    static char line[1 << 16], hex[1 << 16];
    while (fgets(line, sizeof line, stdin)) {{
        char cmd;
        long a = 0, b = 0;
        hex[0] = 0;
        if (sscanf(line, "%c %ld %ld %s", &cmd, &a, &b, hex) < 3) return 2;
        const std::vector<uint8_t> m = unhex(hex);
        if (cmd == 'B') {{
            const std::vector<uint32_t> w = be_words(m, m.size() / 4 + 1);
            const uint32_t c = frs::crc16_words(w.data(), 1, (long)(m.size() / 4));
            printf("%u\\n", frs::crc16_tail(c, w[m.size() / 4], (int)(m.size() & 3)));
        }} else if (cmd == 'W') {{
            const std::vector<uint32_t> w = be_words(m, m.size() / 4);
            std::vector<uint32_t> w3(3 * w.size() + 1, 0xA5A5A5A5u);
            for (size_t i = 0; i < w.size(); i++) w3[3 * i] = w[i];
            printf("%u %u\\n", frs::crc16_words(w.data(), 1, (long)w.size()),
                   frs::crc16_words(w3.data(), 3, (long)w.size()));
        }} else if (cmd == 'C') {{
            uint32_t r;
            if (a == 34) r = columns<34>(m, (int)b);
            else if (a == 35) r = columns<35>(m, (int)b);
            else if (a == 45) r = columns<45>(m, (int)b);
            else return 3;
            printf("%u\\n", r);
        }} else if (cmd == 'X') {{
            printf("%u %u\\n", frs::crc16_xpow(a), frs::crc16_xpow(-a));
        }} else {{
            return 4;
        }}
    }}
    return 0;
}}'''


def crc16_bitwise(data: bytes) -> int:
    c = 0
    for byte in data:
        c ^= byte << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


_TABLE = [crc16_bitwise(bytes([i])) for i in range(256)]


def crc16_bytewise(data: bytes) -> int:
    """the bitwise CRC a byte at a time (the long messages of the column test)"""
    c = 0
    for byte in data:
        c = ((c << 8) & 0xFFFF) ^ _TABLE[(c >> 8) ^ byte]
    return c


def mulmod(a: int, b: int) -> int:
    r = 0
    for i in range(15, -1, -1):
        r <<= 1
        if r & 0x10000:
            r ^= 0x18005
        if (b >> i) & 1:
            r ^= a
    return r


def _flags():
    """-fsanitize=undefined,address where the host compiler links them"""
    probe = subprocess.run(["g++", "-fsanitize=undefined,address", "-x", "c++", "-", "-o", "/dev/null"],
                           input="int main() { return 0; }", capture_output=True, text=True)
    return ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"] if probe.returncode == 0 else []


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("crc16_fold")
    (d / "t.cpp").write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *_flags(), "-o", str(d / "t"), str(d / "t.cpp")],
                   check=True)

    def f(requests):
        text = "".join("%s %d %d %s\n" % (c, a, b, m.hex() or "-") for c, a, b, m in requests)
        p = subprocess.run([str(d / "t")], input=text, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        out = p.stdout.split("\n")
        assert len(out) == len(requests) + 1 and out[-1] == ""
        return [[int(v) for v in line.split()] for line in out[:-1]]
    return f


def test_header_does_not_need_hip():
    text = HEADER.read_text()
    assert "#include <hip" not in text and '#include "frs_' not in text and "asm" not in text


def test_bitwise_reference_check_value():
    assert crc16_bitwise(b"123456789") == 0xFEE8


def test_every_length_to_200_bytes(run):
    rng = random.Random(1)
    msgs = [bytes(rng.randrange(256) for _ in range(n)) for n in range(201)]
    msgs += [bytes(n) for n in range(1, 201, 7)] + [b"\xff" * n for n in range(1, 201)] + [b"123456789"]
    got = run([("B", 0, 0, m) for m in msgs])
    for m, g in zip(msgs, got):
        assert g == [crc16_bitwise(m)], (len(m), m.hex())
    assert got[-1] == [0xFEE8]


def test_word_counts_1_to_48(run):
    rng = random.Random(2)
    msgs = []
    for n in range(1, 49):
        msgs += [bytes(rng.randrange(256) for _ in range(4 * n)) for _ in range(4)]
        msgs += [bytes(4 * n), b"\xff" * (4 * n)]
    for n in (60, 61, 75, 76, 200):  # more than one 15-word block after the first pass
        msgs.append(bytes(rng.randrange(256) for _ in range(4 * n)))
    for bit in range(35 * 32):       # one set bit at every position of a 35-word message
        m = bytearray(35 * 4)
        m[bit >> 3] = 0x80 >> (bit & 7)
        msgs.append(bytes(m))
    got = run([("W", 0, 0, m) for m in msgs])
    for m, g in zip(msgs, got):
        want = crc16_bitwise(m)
        assert g == [want, want], (len(m), m.hex())


def _column_cases():
    """(n, c, message): every c from 1 to n, every length mod 4, a last data column that holds one word, a partial
    column, a full column (with and without tail bytes behind it), and a message that ends in an early column"""
    rng = random.Random(3)
    cases = []
    for n in (34, 35, 45):
        for c in (range(1, n + 1) if n < 45 else (1, 2, 44, 45)):
            full = 64 * c                       # words of the buffer
            words = sorted({full - 1,           # every column full, the last short by the footer's room
                            full - c,           # the last data column is column 62, full
                            full - c + 1,       # column 63 holds a single word
                            max(1, full - c // 2 - 1), max(1, full // 3)})
            for nw in words:
                for tail in range(4):
                    body = 4 * nw + tail
                    if body + 2 > 4 * full:     # the frame's footer has room in the buffer
                        continue
                    cases.append((n, c, bytes(rng.randrange(256) for _ in range(body))))
            cases.append((n, c, b"\xff" * (4 * (full - 1) + 1)))
    return cases


def test_column_decomposition(run):
    cases = _column_cases()
    assert {(n, c) for n, c, _ in cases} >= {(n, c) for n in (34, 35) for c in range(1, n + 1)}
    assert {len(m) & 3 for _, _, m in cases} == {0, 1, 2, 3}
    got = run([("C", n, c, m) for n, c, m in cases])
    for (n, c, m), g in zip(cases, got):
        assert g == [crc16_bytewise(m)], (n, c, len(m))


def test_powers_of_x_and_their_inverses(run):
    """crc16_xpow(e) is x^e mod P by the bitwise CRC (x^e is the CRC of a one followed by e - 16 zeros), and
    crc16_xpow(-e) is its inverse: the encoder's column factors x^(512 (j - 3)) include three negative powers"""
    es = list(range(0, 64)) + [512 * j for j in range(1, 140)] + [8 * 35 * 4 * s for s in range(1, 36)] + [32767, 65534]
    got = run([("X", e, 0, b"") for e in es])
    for e, (p, q) in zip(es, got):
        assert mulmod(p, q) == 1, e
        if e >= 16 and (e - 16) % 8 == 0:
            assert p == crc16_bitwise(b"\x01" + bytes((e - 16) // 8)), e
    assert got[0] == [1, 1] and got[1] == [2, 0xC002] and got[16][0] == 0x8005
