"""The fixed-predictor totals on packed int16 pairs (csrc/frs_fixed_totals.h), built by the host compiler.

`fixed_totals_pairs` gives one lane's sums of |e_k(i)|, k = 0..4, over its 64 samples (tk; lane 0 from sample 4) and the
terms at k <= i < 4 (hk).  The program below compares both, exactly, with a plain restatement of the sums of fixed.c
FLAC__fixed_compute_best_predictor on 8 samples of history and the lane's 64, for lane 0 (history of zeros, as the
kernel gives it) and for any other lane: full-scale alternations in both phases and in runs of two, all-equal
samples, one full-scale spike at each of the 64 positions and at each of the 8 history positions, 100,000 random lanes
over the int16 range and 100,000 over +-127.  The same program is also built and run once with the address and
undefined-behaviour sanitizers.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_fixed_totals.h"

_PROGRAM = r"""
#include "frs_fixed_totals.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static long n_cases = 0, n_bad = 0;

// s[0..7]: history, s[8..71]: the lane's samples
static void reference(const int *s, bool l0, uint32_t *tk, uint32_t *hk) {
    for (int k = 0; k < 5; k++) tk[k] = hk[k] = 0;
    for (int i = 8; i < 72; i++) {
        const long e0 = s[i], e1 = e0 - s[i - 1], e2 = e1 - (s[i - 1] - s[i - 2]);
        const long e3 = e2 - (s[i - 1] - 2 * s[i - 2] + s[i - 3]);
        const long e4 = e3 - (s[i - 1] - 3 * s[i - 2] + 3 * s[i - 3] - s[i - 4]);
        const long e[5] = {e0, e1, e2, e3, e4};
        const int j = i - 8;
        for (int k = 0; k < 5; k++) {
            if (j >= 4 || !l0) tk[k] += (uint32_t)labs(e[k]);
            if (j < 4 && j >= k) hk[k] += (uint32_t)labs(e[k]);
        }
    }
}

static void run(const int *s72, bool l0) {
    int s[72];
    for (int i = 0; i < 72; i++) s[i] = (l0 && i < 8) ? 0 : s72[i];
    uint32_t E[36];
    for (int m = 0; m < 36; m++) E[m] = ((uint32_t)s[2 * m] & 0xFFFFu) | ((uint32_t)s[2 * m + 1] << 16);
    uint32_t tk[5], hk[5], rt[5], rh[5];
    frs::fixed_totals_pairs(E, l0, tk, hk);
    reference(s, l0, rt, rh);
    bool bad = false;
    for (int k = 0; k < 5; k++) bad |= tk[k] != rt[k] || hk[k] != rh[k];
    if (bad && n_bad < 5) {
        printf("mismatch l0=%d:", (int)l0);
        for (int k = 0; k < 5; k++) printf(" t%d %u/%u h%d %u/%u", k, tk[k], rt[k], k, hk[k], rh[k]);
        printf("\n");
    }
    n_bad += bad;
    n_cases++;
}
static void both(const int *s) {
    run(s, false);
    run(s, true);
}

int main() {
    const int lo = -32768, hi = 32767;
    int s[72];
    // full-scale alternation, both phases, single samples and runs of two
    for (int run_len = 1; run_len <= 2; run_len++)
        for (int phase = 0; phase < 2 * run_len; phase++) {
            for (int i = 0; i < 72; i++) s[i] = (((i + phase) / run_len) & 1) ? hi : lo;
            both(s);
        }
    // all-equal samples
    const int levels[] = {lo, -1, 0, 1, 127, hi};
    for (int v : levels) {
        for (int i = 0; i < 72; i++) s[i] = v;
        both(s);
    }
    // one full-scale spike at each of the 8 history positions and the 64 lane positions, on three floors
    const int floors[] = {0, lo, hi};
    for (int f : floors)
        for (int at = 0; at < 72; at++)
            for (int v : {lo, hi}) {
                if (v == f) continue;
                for (int i = 0; i < 72; i++) s[i] = f;
                s[at] = v;
                both(s);
            }
    // random lanes over the int16 range and over +-127 (the 8-bit types)
    std::mt19937 g(20240607);
    for (int range = 0; range < 2; range++) {
        std::uniform_int_distribution<int> d(range ? -127 : lo, range ? 127 : hi);
        for (int t = 0; t < 100000; t++) {
            for (int i = 0; i < 72; i++) s[i] = d(g);
            both(s);
        }
    }
    printf("%ld %ld\n", n_cases, n_bad);
    return n_bad != 0;
}
"""

N_CASES = 2 * (6 + 6 + (144 + 72 + 72) + 200000)  # alternations, levels, spikes, random; lane 0 and another lane


def _build_and_run(tmp_path, name, flags):
    (tmp_path / "t.cpp").write_text(_PROGRAM)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(HEADER.parent), "-o", str(exe),
                    str(tmp_path / "t.cpp")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    n, bad = (int(v) for v in p.stdout.split()[-2:])
    assert n == N_CASES and bad == 0


def test_fixed_totals_pairs_match_the_plain_sums(tmp_path):
    _build_and_run(tmp_path, "t", ["-O2"])


def test_fixed_totals_pairs_under_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: no report, same counts"""
    _build_and_run(tmp_path, "t_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
