"""csrc/frs_normalize.h built by the host compiler alone, and the oracle's normalisation against numpy itself.

The header is the one definition of the tile normalisation's scalar arithmetic; the six sites of frs_encode.hip call
it.  Flags: `g++ -std=c++17 -O2 -ffp-contract=off -mfma -pthread` -- no contraction, as csrc/Makefile builds the
kernels, and the hardware fused multiply-add for the two __builtin_fma of the reciprocal form (without -mfma the
compiler calls libm's fma, which is as exact and far slower; that is what a CPU without the instruction gets).  The
mode and division checks run a second build of the same text with -fsanitize=undefined,address where the compiler
links them.

Exhaustive reciprocal check, 16 threads on an 8-CPU host: 2.0 s wall for the 2.1e9 pairs (measured; one thread of the
same build: 14.5 s -- it evaluates the quotient both ways and three 16-bit values per pair).
"""
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_normalize.h"
THREADS = 16                                  # fixed: not sized by the machine
PAIRS = 65535 * 65538 // 2                    # every 1 <= den <= 65535, 0 <= d <= den
LUT, FASTDIV, SLOW, ZERO = 0, 1, 2, 3         # kNorm*

# recip T    every (d, den) on T threads (den = t + 1, t + 1 + T, ...): pairs visited, pairs whose reciprocal quotient
#            differs from (2.0 * d) / den in any bit, pairs whose 16-bit values differ (exact division, reciprocal,
#            reciprocal with the plain cast)
# modes      stdin lines "imin imax bits signed norm_mode scale_bits" -> norm_mode_of
# udiv       udiv_inv(n, d, 1.0 / d) against n / d for d = 1..70000 at n = k d - 1, k d, k d + 1
#            (k = 1, 2, 4095, 4096, (2^32 - 1) / d; n kept where it fits 32 bits) and n = 2^32 - 1: checked, wrong
PROG = f'''#include "{HEADER}"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
struct Part {{ unsigned long long n = 0, badq = 0, badv = 0; char pad[64]; }};
static void recip_part(int t, int T, Part *out) {{
    Part p;
    for (int den_i = 1 + t; den_i <= 65535; den_i += T) {{
        const double den = (double)den_i, rinv = 1.0 / den;
        for (int d = 0; d <= den_i; d++) {{
            const double a = 2.0 * (double)d;
            const double q1 = frs::norm_quot_recip(a, den, rinv), q = (2.0 * (double)d) / den;
            p.badq += memcmp(&q1, &q, sizeof q) != 0;
            const int32_t v = frs::norm16_div((double)d, den);
            p.badv += v != frs::norm16_recip(a, den, rinv) || v != frs::norm16_recip_inrange(a, den, rinv);
            p.n++;
        }}
    }}
    *out = p;
}}
int main(int argc, char **argv) {{
    if (argc >= 3 && !strcmp(argv[1], "recip")) {{
        const int T = atoi(argv[2]);
        if (T < 1 || T > 16) return 2;
        std::vector<Part> parts(T);
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++) th.emplace_back(recip_part, t, T, &parts[t]);
        Part s;
        for (int t = 0; t < T; t++) {{
            th[t].join();
            s.n += parts[t].n, s.badq += parts[t].badq, s.badv += parts[t].badv;
        }}
        printf("%llu %llu %llu\\n", s.n, s.badq, s.badv);
    }} else if (argc >= 2 && !strcmp(argv[1], "modes")) {{
        long long lo, hi;
        int bits, sg, nm, sb;
        while (scanf("%lld %lld %d %d %d %d", &lo, &hi, &bits, &sg, &nm, &sb) == 6)
            printf("%d\\n", frs::norm_mode_of(lo, hi, bits, sg != 0, nm, sb));
    }} else if (argc >= 2 && !strcmp(argv[1], "udiv")) {{
        unsigned long long checked = 0, wrong = 0;
        for (uint64_t d = 1; d <= 70000; d++) {{
            const double inv = 1.0 / (double)d;
            const uint64_t ks[5] = {{1, 2, 4095, 4096, 0xFFFFFFFFull / d}};
            for (int i = 0; i <= 5; i++)
                for (int e = -1; e <= 1; e++) {{
                    if (i == 5 && e != 0) continue;
                    const uint64_t n = i == 5 ? 0xFFFFFFFFull : ks[i] * d + (uint64_t)(int64_t)e;
                    if (n > 0xFFFFFFFFull) continue;
                    checked++;
                    wrong += frs::udiv_inv((uint32_t)n, (uint32_t)d, inv) != (uint32_t)(n / d);
                }}
        }}
        printf("%llu %llu\\n", checked, wrong);
    }} else {{
        return 3;
    }}
    return 0;
}}'''


def _links(flags):
    return subprocess.run(["g++", *flags, "-x", "c++", "-", "-o", "/dev/null"], input="int main() { return 0; }",
                          capture_output=True, text=True).returncode == 0


def _has_fma():
    try:
        return " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        return False


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    """(fast build, checked build)"""
    d = tmp_path_factory.mktemp("normalize_host")
    (d / "t.cpp").write_text(PROG)
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-pthread"]
    subprocess.run([*base, "-O2", *(["-mfma"] if _has_fma() else []), "-o", str(d / "fast"), str(d / "t.cpp")],
                   check=True)
    san = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    subprocess.run([*base, "-O1", *(san if _links(san) else []), "-o", str(d / "checked"), str(d / "t.cpp")],
                   check=True)
    return d / "fast", d / "checked"


def _run(prog, *args, text=""):
    p = subprocess.run([str(prog), *args], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return [[int(v) for v in line.split()] for line in p.stdout.splitlines()]


def test_header_does_not_need_hip():
    text = HEADER.read_text()
    assert "#include <hip" not in text and '#include "frs_' not in text and "asm" not in text


def test_reciprocal_quotient_is_the_division_for_every_pair(progs):
    """q1 = fma(fma(-q0, den, a), rinv, q0) == (2.0 * d) / den bit for bit, and the 16-bit values of the division,
    the reciprocal and the reciprocal with the plain cast are equal, for every 0 <= d <= den <= 65535, den >= 1."""
    (n, badq, badv), = _run(progs[0], "recip", str(THREADS))
    assert n == PAIRS == 2147516415
    assert (badq, badv) == (0, 0)


INTS = {"u8": (8, 0, 0, 255), "u16": (16, 0, 0, 65535), "i16": (16, 1, -32768, 32767)}
CUTS = (0, 1, 4094, 4095, 4096, 32767, 32768, 65534, 65535)


def _mode_cases():
    """(name, imin, imax, bits, signed, expected at 16-bit scale)"""
    out = []
    for name, (bits, sg, lo, hi) in INTS.items():
        for R in CUTS:
            for mn in sorted({lo, 0, hi - R}):
                if mn < lo or mn + R > hi:
                    continue
                wraps = sg and R >= 32768            # x - min can leave int16
                want = ZERO if R == 0 else SLOW if wraps else LUT if R <= 4095 else FASTDIV
                out.append((name, mn, mn + R, bits, sg, want))
    return out


def test_mode_choice_at_the_cutoffs(progs):
    cases = _mode_cases()
    seen = {(c[0], c[2] - c[1]) for c in cases}
    assert seen >= {("u16", R) for R in CUTS} | {("i16", R) for R in CUTS} | {("u8", R) for R in (0, 1)}
    assert {c[1] for c in cases if c[0] == "i16"} >= {-32768, 0, 32767 - 4096, 32767 - 32767}
    lines16 = "".join("%d %d %d %d 0 16\n" % c[1:5] for c in cases)
    lines24 = "".join("%d %d %d %d 0 24\n" % c[1:5] for c in cases)
    spatial = "".join("%d %d %d %d 1 16\n" % c[1:5] for c in cases)
    got16 = _run(progs[1], "modes", text=lines16)
    assert len(got16) == len(cases)
    for c, (g,) in zip(cases, got16):
        assert g == c[5], c
    assert _run(progs[1], "modes", text=lines24) == [[SLOW]] * len(cases)    # 32-bit scale: always the division
    assert _run(progs[1], "modes", text=spatial) == [[SLOW]] * len(cases)    # the other map has no modes
    # 32-bit dtypes on a 16-bit scale: the same cut-offs, nothing wraps below 2^31
    wide = [(0, 4095, 32, 1, LUT), (-5, 4091, 32, 1, FASTDIV), (-2 ** 31, -2 ** 31 + 65535, 32, 1, FASTDIV),
            (0, 65536, 32, 0, SLOW), (-2 ** 31, 2 ** 31 - 1, 32, 1, SLOW), (0, 2 ** 32 - 1, 32, 0, SLOW),
            (-1, 2 ** 31 - 1, 32, 1, SLOW), (7, 7, 32, 0, ZERO)]
    got = _run(progs[1], "modes", text="".join("%d %d %d %d 0 16\n" % w[:4] for w in wide))
    assert got == [[w[4]] for w in wide]


def test_udiv_inv_at_the_multiples_of_every_divisor(progs):
    d = np.arange(1, 70001, dtype=np.int64)
    top = 2 ** 32 - 1
    want = d.size                                             # n = 2^32 - 1
    for k in (np.full_like(d, 1), np.full_like(d, 2), np.full_like(d, 4095), np.full_like(d, 4096), top // d):
        for e in (-1, 0, 1):
            want += int(np.count_nonzero(k * d + e <= top))
    (checked, wrong), = _run(progs[1], "udiv")
    # 16 values of n per divisor; k d + 1 leaves 32 bits only where d divides 2^32 - 1 = 3 * 5 * 17 * 257 * 65537:
    # 17 divisors up to 70000
    assert checked == want == 16 * 70000 - 17
    assert wrong == 0


def _numpy_normalize(a):
    """converter.py:56-86 as numpy evaluates it (tests/test_oracle_golden.py::test_normalize_matches_numpy's
    expression): same-kind wrapping differences, float data as-is, 8388607 and int32 for the 24-bit dtypes."""
    wide = a.dtype.itemsize > 2
    with warnings.catch_warnings(), np.errstate(over="ignore", invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)       # scalar-overflow and invalid-cast warnings
        if a.dtype.kind == "f":
            norm = a
        elif np.max(a) > np.min(a):
            norm = 2.0 * (a - np.min(a)) / (np.max(a) - np.min(a)) - 1.0
        else:
            norm = np.zeros_like(a, dtype=np.float32)
        if wide:
            return (norm * 8388607).astype(np.int32)
        return (norm * 32767).astype(np.int16).astype(np.int32)


def _numpy_cases():
    rng = np.random.default_rng(1)
    odd = [np.nan, np.inf, -np.inf, 300.0, -300.0, 255.99, -255.99, -256.0, 256.0, 0.0, -0.0, 1.0, -1.0, 1e-30]
    full16 = rng.integers(-32768, 32768, 70000).astype(np.int16)
    full16[:2] = [-32768, 32767]
    full32 = rng.integers(-2 ** 31, 2 ** 31, 70000).astype(np.int32)
    full32[:2] = [-2 ** 31, 2 ** 31 - 1]
    over31 = rng.integers(-2 ** 30, 2 ** 30 + 6, 70000).astype(np.int32)
    over31[:2] = [-2 ** 30, 2 ** 30 + 5]                      # range 2^31 + 5: wraps negative
    fullu32 = rng.integers(0, 2 ** 32, 70000).astype(np.uint32)
    fullu32[:2] = [0, 2 ** 32 - 1]
    return {
        "i16_full": full16,
        "i16_R32767": np.arange(-5, 32763, dtype=np.int16),   # max - min = 32767: the last range that cannot wrap
        "i16_R32768": np.arange(-5, 32764, dtype=np.int16),   # 32768: wraps to -32768
        "i16_R32768_top": np.arange(-1, 32768).astype(np.int16),
        "i32_full": full32,
        "i32_over_2^31": over31,
        "u32_full": fullu32,
        "u32_small": rng.integers(5, 100000, 70000).astype(np.uint32),
        "i32_ramp_70000": np.arange(-7, 69994, dtype=np.int32),
        "const_u8": np.full(300, 17, np.uint8),
        "const_i16": np.full(300, -9, np.int16),
        "const_i32": np.full(300, 123456, np.int32),
        "f32": np.concatenate([rng.normal(0, 1, 5000), rng.uniform(-255, 255, 5000), odd]).astype(np.float32),
        "f64": np.concatenate([rng.normal(0, 1, 5000), rng.uniform(-255, 255, 5000), odd]).astype(np.float64),
    }


@pytest.mark.parametrize("name", list(_numpy_cases()))
def test_oracle_normalize_matches_numpy_on_wrapping_and_wide_inputs(name):
    """O.normalize against numpy's own expression where the suite had only tied the GPU to the oracle: wrapping
    int16, int32 and uint32 (24-bit scale, int32 cast), constants, and floats with NaN, +-inf and |x| >= 256."""
    a = _numpy_cases()[name]
    pcm, mn, mx, bps = O.normalize(a)
    assert bps == (32 if a.dtype.itemsize > 2 else 16)
    ref = _numpy_normalize(a)
    bad = np.flatnonzero(pcm != ref)
    assert bad.size == 0, (name, bad[:5], a[bad[:5]], pcm[bad[:5]], ref[bad[:5]])
    if a.dtype.kind != "f":                                   # the reference never computes a float min / max
        assert (mn, mx) == (float(a.min()), float(a.max()))


@pytest.mark.parametrize("R", [1, 2, 3, 4094, 4095, 4096, 4097, 32767, 32768, 40000, 65534, 65535])
def test_oracle_normalize_matches_numpy_on_complete_ramps(R):
    for a in (np.arange(0, R + 1, dtype=np.uint16), (np.arange(0, R + 1) + 65535 - R).astype(np.uint16),
              (np.arange(0, R + 1) - 32768).astype(np.int16)):
        assert np.unique(a).size == min(R + 1, 65536)
        assert np.array_equal(O.normalize(a)[0], _numpy_normalize(a)), (R, a.dtype)
