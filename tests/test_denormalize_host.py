"""csrc/frs_denormalize.h built by the host compiler alone, against numpy's own evaluation of converter.py:88-110.

The header is the one definition of the de-normalisation's scalar arithmetic; the six sites of frs_decode.hip call it.
Flags: `g++ -std=c++17 -O2 -ffp-contract=off -pthread` -- no contraction, as csrc/Makefile builds the kernels.  A
second build of the same text with -fsanitize=undefined,address (where the compiler links it) runs the numpy tie and
a thinned exhaustive pass.  Nothing is loaded into Python: both are stand-alone programs.

Exhaustive pass (every range R of uint8 / int16 / uint16 at four minima, all 65 536 PCM values: 34 426 847 232
evaluations of both forms), 16 threads on an 8-CPU host: 16 s wall (measured).

Sensitivity, over the 128 uint8 / int16 / uint16 cases of tests/denorm_cases.py x 65 536 PCM values (measured by
test_wrong_variants_show_inside_the_case_list, which asserts only that each is > 0):
  one fused multiply-add instead of the product and the sum:  uint8 0, int16 433, uint16 233 values differ
  round half away from zero instead of half to even:          uint8 9, int16 76 181, uint16 76 814 values differ
(uint8: the product (h + 32768) * (R * 2^-16) has at most 16 + 8 significant bits, so it is exact in fp32 and a
contraction cannot show.)  Exact .5 ties among the 128 cases: 305 489.
"""
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests import denorm_cases as D

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_denormalize.h"
THREADS = 16                                  # fixed: not sized by the machine
CODES = {"uint8": 0, "int16": 1, "uint16": 2, "int32": 3, "uint32": 4, "float32": 5, "float64": 6}
EXHAUSTIVE = (256 + 65536 + 65536) * 4 * 65536

# exh T STEP   every range R = 0, STEP, 2 STEP, .. of uint8, int16 and uint16 on T threads, at the minima lowest,
#              highest - R, their middle and a scattered one, all 65 536 PCM values, wasted-bit shift 0: evaluations,
#              those where the two-operation form differs from the four-operation one (in any bit of the fp32 value or
#              in the rounded integer), those whose rounded value is outside the dtype
# table        stdin lines "form dtype min max shift" -> the 65 536 values of the case as raw elements of the dtype on
#              stdout, PCM values in ascending order.  shift 16: the samples are (p16 << 16) | 16 scrambled low bits.
#              form 4: the four operations and the int64 cast; 2: the two-operation form and the int32 cast;
#              F: WRONG on purpose, one fused multiply-add; H: WRONG on purpose, round half away from zero
PROG = f'''#include "{HEADER}"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
struct Part {{ unsigned long long n = 0, diff = 0, outside = 0; char pad[64]; }};
static const long long kLo[3] = {{0, -32768, 0}}, kHi[3] = {{255, 32767, 65535}};
static void exh_part(int t, int T, int step, Part *out) {{
    Part p;
    for (int ty = 0; ty < 3; ty++) {{
        const long long lo = kLo[ty], hi = kHi[ty];
        const float flo = (float)lo, fhi = (float)hi;
        for (long long R = (long long)t * step; R <= hi - lo; R += (long long)T * step) {{
            const long long top = hi - R;
            const long long mins[4] = {{lo, top, lo + (top - lo) / 2, lo + (R * 40503) % (top - lo + 1)}};
            for (int m = 0; m < 4; m++) {{
                const frs::DnPair dp = frs::dn_pair((double)mins[m], (double)(mins[m] + R));
                const float rng16 = frs::dn_rng16(dp.rng);
                unsigned diff = 0, odd = 0;
                for (int h = -32768; h < 32768; h++) {{
                    const float a4 = frs::dn_value4(frs::dn_unit(frs::dn_pcm16(h, 0)), dp.rng, dp.mn);
                    const float a2 = frs::dn_value2(h, 0, rng16, dp.mn);
                    uint32_t b4, b2;
                    memcpy(&b4, &a4, 4);
                    memcpy(&b2, &a2, 4);
                    diff += b4 != b2;
                    odd += !(a4 >= flo && a4 <= fhi);  // inside [lo, hi] (integers): so is the rounded value
                }}
                p.n += 65536;
                p.diff += diff;
                if (diff || odd)  // rare: look at the rounded values themselves
                    for (int h = -32768; h < 32768; h++) {{
                        const float a4 = frs::dn_value4(frs::dn_unit(h), dp.rng, dp.mn);
                        const float r4 = rintf(a4), r2 = rintf(frs::dn_value2(h, 0, rng16, dp.mn));
                        p.outside += !(r4 >= flo && r4 <= fhi) || !(r2 >= flo && r2 <= fhi);
                    }}
            }}
        }}
    }}
    *out = p;
}}
template <typename O> static void put(O v) {{ fwrite(&v, sizeof v, 1, stdout); }}
int main(int argc, char **argv) {{
    if (argc >= 4 && !strcmp(argv[1], "exh")) {{
        const int T = atoi(argv[2]), step = atoi(argv[3]);
        if (T < 1 || T > 16 || step < 1) return 2;
        std::vector<Part> parts(T);
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++) th.emplace_back(exh_part, t, T, step, &parts[t]);
        Part s;
        for (int t = 0; t < T; t++) {{
            th[t].join();
            s.n += parts[t].n, s.diff += parts[t].diff, s.outside += parts[t].outside;
        }}
        printf("%llu %llu %llu\\n", s.n, s.diff, s.outside);
    }} else if (argc >= 2 && !strcmp(argv[1], "table")) {{
        char form;
        int dt, shift;
        double dmin, dmax;
        while (scanf(" %c %d %lf %lf %d", &form, &dt, &dmin, &dmax, &shift) == 5) {{
            const frs::DnPair dp = frs::dn_pair(dmin, dmax);
            for (int h = -32768; h < 32768; h++) {{
                const int32_t pcm = shift ? (int32_t)(((uint32_t)h << 16) | (((uint32_t)h * 40503u) & 0xFFFFu)) : h;
                const int32_t p16 = frs::dn_pcm16(pcm, shift);
                const float v = frs::dn_unit(p16);
                if (dt == 5) {{ put<float>(v); continue; }}
                if (dt == 6) {{ put<double>((double)v); continue; }}
                int64_t r;
                if (form == '4') r = frs::dn_round64(frs::dn_value4(v, dp.rng, dp.mn));
                else if (form == '2') r = frs::dn_round32(frs::dn_value2(p16, 0, frs::dn_rng16(dp.rng), dp.mn));
                else if (form == 'F') r = (int64_t)rintf(fmaf((float)(p16 + 32768), frs::dn_rng16(dp.rng), dp.mn));
                else if (form == 'H') r = (int64_t)roundf(frs::dn_value4(v, dp.rng, dp.mn));
                else return 4;
                switch (dt) {{
                case 0: put<uint8_t>((uint8_t)r); break;
                case 1: put<int16_t>((int16_t)r); break;
                case 2: put<uint16_t>((uint16_t)r); break;
                case 3: put<int32_t>((int32_t)r); break;
                default: put<uint32_t>((uint32_t)r); break;
                }}
            }}
        }}
    }} else {{
        return 3;
    }}
    return 0;
}}'''


def _links(flags):
    return subprocess.run(["g++", *flags, "-x", "c++", "-", "-o", "/dev/null"], input="int main() { return 0; }",
                          capture_output=True, text=True).returncode == 0


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    """(fast build, checked build)"""
    d = tmp_path_factory.mktemp("denormalize_host")
    (d / "t.cpp").write_text(PROG)
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-pthread"]
    subprocess.run([*base, "-O2", "-o", str(d / "fast"), str(d / "t.cpp")], check=True)
    san = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    subprocess.run([*base, "-O1", *(san if _links(san) else []), "-o", str(d / "checked"), str(d / "t.cpp")],
                   check=True)
    return d / "fast", d / "checked"


def _exh(prog, step):
    p = subprocess.run([str(prog), "exh", str(THREADS), str(step)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return tuple(int(v) for v in p.stdout.split())


def _tables(prog, form, cases, shift=0):
    """the program's 65 536 values of every case, as arrays of the case's dtype"""
    text = "".join(f"{form} {CODES[dt]} {float(mn)!r} {float(mx)!r} {shift}\n" for dt, mn, mx in cases)
    p = subprocess.run([str(prog), "table"], input=text.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out, at = [], 0
    for dt, _, _ in cases:
        n = 65536 * np.dtype(dt).itemsize
        out.append(np.frombuffer(p.stdout[at:at + n], dtype=dt))
        at += n
    assert at == len(p.stdout)
    return out


def _first_difference(case, got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (case, int(D.ALL_P16[bad[0]]), got[bad[0]], want[bad[0]], bad.size)


def test_header_does_not_need_hip():
    text = HEADER.read_text()
    assert "#include <hip" not in text and '#include "frs_' not in text and "asm" not in text


def test_case_list():
    """128 distinct narrow cases with every edge range, the wide ones, one per float dtype; every case stays inside
    its dtype at every PCM value (numpy_denormalize asserts it while D.table evaluates: no case is skipped)."""
    narrow = [c for c in D.CASES if c[0] in D.NARROW]
    assert len(set(narrow)) == len(narrow) == 128 and len(set(D.CASES)) == len(D.CASES)
    for dt in ("int16", "uint16"):
        assert {c[2] - c[1] for c in D.cases_of(dt)} == set(D.EDGE_R)
    assert {c[2] - c[1] for c in D.cases_of("uint8")} == {R for R in D.EDGE_R if R <= 255}
    assert ("int32", -2 ** 31, 2 ** 31 - 1) in D.CASES and ("int32", -7, 2 ** 24) in D.CASES
    assert ("uint32", 0, 2 ** 32 - 1) in D.CASES
    for dt in ("int32", "uint32"):
        assert {c[2] - c[1] for c in D.cases_of(dt)} >= set(D.WIDE_R)
    assert len(D.cases_of("float32")) == len(D.cases_of("float64")) == 1
    # the difference is taken in double before the fp32 cast: a case where casting first gives another range
    assert any(np.float32(c[2]) - np.float32(c[1]) != np.float32(c[2] - c[1]) for c in D.cases_of("int32"))
    assert any(np.float32(c[2]) - np.float32(c[1]) != np.float32(c[2] - c[1]) for c in D.cases_of("uint32"))
    ties = 0
    for c in D.CASES:
        assert D.table(c).shape == (65536,) and D.table(c).dtype == np.dtype(c[0])
        if c[0] in D.NARROW:
            v = (D.ALL_P16.astype(np.float64) / 32768.0).astype(np.float32)
            d = (v + 1.0) / 2.0 * float(c[2] - c[1]) + float(c[1])
            ties += int(np.count_nonzero(np.abs(d - np.trunc(d)) == 0.5))
    print("exact .5 ties among the 128 cases:", ties)
    assert ties > 100000                                      # round-half-even is exercised, not just near-ties


def test_rewrite_is_the_four_operations_for_every_range(progs):
    """(h + 32768) * (rng * 2^-16) + min == ((h / 32768 + 1) / 2) * rng + min bit for bit, and no rounded value leaves
    its dtype: every R of uint8 / int16 / uint16, four minima, every PCM value."""
    t0 = time.perf_counter()
    n, diff, outside = _exh(progs[0], 1)
    print(f"evaluated {n}, rewrite differs {diff}, outside the dtype {outside}; "
          f"{time.perf_counter() - t0:.1f} s on {THREADS} threads")
    assert n == EXHAUSTIVE == 34426847232
    assert (diff, outside) == (0, 0)


def test_thinned_pass_under_the_sanitizers(progs):
    step = 257
    n, diff, outside = _exh(progs[1], step)
    assert n == sum(len(range(0, span + 1, step)) for span in (255, 65535, 65535)) * 4 * 65536
    assert (diff, outside) == (0, 0)


@pytest.mark.parametrize("build", ["fast", "checked"])
def test_header_matches_numpy_on_every_case(progs, build):
    """The four-operation form with the int64 cast on all 153 cases, at shift 0 and on 32-bit samples (shift 16); the
    two-operation form with the int32 cast on the 128 narrow ones: every PCM value equals numpy's."""
    prog = progs[build == "checked"]
    narrow = [c for c in D.CASES if c[0] in D.NARROW]
    for form, cases, shift in (("4", list(D.CASES), 0), ("4", list(D.CASES), 16), ("2", narrow, 0), ("2", narrow, 16)):
        for c, got in zip(cases, _tables(prog, form, cases, shift)):
            assert _first_difference(c, got, D.table(c)) is None, (form, shift, _first_difference(c, got, D.table(c)))


def test_oracle_matches_numpy_on_every_case():
    """oracle.denormalize_i16 on every case and PCM value, as 16-bit samples and as the high halves of 32-bit ones
    (tests/test_oracle_golden.py::test_denormalize_matches_numpy samples 3 x 20 000 of these)."""
    low = (D.ALL_P16.astype(np.int64) * 40503) & 0xFFFF
    low[:4] = (0, 0xFFFF, 0, 0xFFFF)
    wide = (D.ALL_P16.astype(np.int64) * 65536 + low).astype(np.int32)
    assert np.array_equal(wide >> 16, D.ALL_P16)
    for c in D.CASES:
        for pcm, bps in ((D.ALL_P16, 16), (wide, 32)):
            got = O.denormalize_i16(pcm, float(c[1]), float(c[2]), np.dtype(c[0]), pcm_bps=bps)
            assert _first_difference(c, got, D.table(c)) is None, (bps, _first_difference(c, got, D.table(c)))


def test_wrong_variants_show_inside_the_case_list(progs):
    """Two deliberately wrong forms, written in the test program only: each must differ from numpy somewhere in the
    case list, for every dtype where it can (the counts are in the module docstring).  This is what lets the GPU
    tests, which run the same cases, catch a site that contracts its multiply-add or rounds half away."""
    narrow = [c for c in D.CASES if c[0] in D.NARROW]
    count = {}
    for form in "FH":
        for c, got in zip(narrow, _tables(progs[0], form, narrow)):
            count[form, c[0]] = count.get((form, c[0]), 0) + int(np.count_nonzero(got != D.table(c)))
    print("values that differ:", count)
    assert count["F", "int16"] > 0 and count["F", "uint16"] > 0
    assert count["F", "uint8"] == 0                            # exact product: nothing to contract
    assert all(count["H", dt] > 0 for dt in D.NARROW)


def test_cover_streams_hold_every_pcm_value_and_no_false_sync():
    """The GPU tests' streams (tests/denorm_cases.py), on the CPU: the oracle decodes each to the samples that went
    in, every channel holds all 65 536 values, and the mono streams hold no byte run that reads as a frame header
    outside their frame starts, in one copy or across the seam of two (so the optimistic decode has no reason to
    decline them)."""
    for odd in (True, False):
        s = D.mono_cover(odd)
        assert np.unique(s.pcm[:65536]).size == 65536 and len(s.pcm) == (81925 if odd else 81920)
        starts = D.mono_frame_starts(odd)
        assert all(s.data[p:p + 2] == b"\xff\xf8" for p in starts) and len(starts) == s.nframes
        twice = set(starts) | {p + len(s.data) for p in starts}
        assert D.false_syncs(s.data * 2, twice) == []
    streams = [D.mono_cover(True), D.mono_cover(False), D.mono32_cover()] + [D.multi_cover(*l) for l in D.MULTI_LAYOUTS]
    for s in streams:
        ref = O.decode_frames(s.data, s.channels, s.bps, len(s.pcm))
        assert np.array_equal(ref.reshape(-1, s.channels), s.pcm), s.name
        h = s.pcm >> (s.bps - 16)
        assert all(np.unique(h[:, c]).size == 65536 for c in range(s.channels)), s.name
    low = D.mono32_cover().pcm[:, 0] & 0xFFFF
    neg = D.mono32_cover().pcm[:, 0] < 0
    assert (low[neg] == 0).any() and (low[neg] == 0xFFFF).any()
