"""The arithmetic of the band statistics and histogram, csrc/frs_stats.h, built with the host compiler into a small
program of its own and compared with the restatement tests/stats_ref.py: the bin rule on every dtype at its edges, the
128-bit carries, and both lane functions run lane by lane over small rasters.  Then the Python rules of
flac_raster_amd/stats.py (histogram_range, percentile, mean / std from exact sums, the index key) and every argument
error of the `stats` command and of `create-streaming --stats`.  No GPU."""
import json
import math
import struct
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import stats as S
from flac_raster_amd import streaming
from flac_raster_amd.cli import app
from tests import stats_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_stats.h"
GOLDEN = ROOT / "tests" / "golden"

DTYPES = ["uint8", "uint16", "int16", "int32", "uint32", "float32", "float64"]

# stats_host bin DTYPE LO HI NBINS IN OUT      IN raw values of DTYPE -> OUT int32 hist_bin of (double)v  (LO, HI: the
#                                              doubles' bit patterns in hex)
# stats_host u128 IN OUT                       IN uint64 values, added with add_u128 -> OUT hi, lo
# stats_host fold DTYPE H W ROWSTRIDE OFFSET GX MASKED ND LO HI NBINS CENTRE IN OUT
#     IN raw elements of DTYPE; the band starts OFFSET elements into a 64-byte aligned copy of them.  Every lane of
#     every work-group of a (GX, 1) grid with BLOCK = 4, UNROLL = 2 runs stats_fold for both passes; OUT gets int64
#     n_valid, n_nodata, n_nan, bits(min), bits(max), isum_hi, isum_lo, isq_hi, isq_lo, bits(fsum), below, above,
#     bits(m2), pixels handed to the accumulator, then NBINS counts
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "%s"

using namespace frs;

static int64_t bits(double v) { int64_t b; memcpy(&b, &v, 8); return b; }
static double from_hex(const char *s) { const uint64_t b = strtoull(s, nullptr, 16); double v; memcpy(&v, &b, 8); return v; }

static std::vector<char> read_all(const char *path) {
    std::vector<char> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    v.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (v.size() && fread(v.data(), 1, v.size(), f) != v.size()) exit(3);
    fclose(f);
    return v;
}
template <typename T> static int write_all(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f) return 4;
    fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return 0;
}

template <typename T> static int bin_mode(char **a) {
    const HistRange r = hist_range(from_hex(a[3]), from_hex(a[4]), atoi(a[5]));
    const std::vector<char> raw = read_all(a[6]);
    const size_t n = raw.size() / sizeof(T);
    std::vector<int32_t> o(n);
    for (size_t i = 0; i < n; i++) {
        T v;
        memcpy(&v, raw.data() + i * sizeof(T), sizeof(T));
        o[i] = hist_bin(r, (double)v);
    }
    return write_all(a[7], o);
}

struct HostSink {
    int64_t *bins;
    void add(int32_t b, uint32_t n) { bins[b] += n; }
};

template <typename T, bool MASKED> static int fold_masked(char **a) {
    constexpr int BLOCK = 4, UNROLL = 2;
    constexpr bool F = NdFloat<T>::value;
    StatsParams P;
    P.height = atoll(a[3]), P.width = atoll(a[4]), P.row_stride = atoll(a[5]);
    P.dense = P.row_stride == P.width;
    const int64_t offset = atoll(a[6]);
    const int gx = atoi(a[7]);
    const T nd = nd_cast<T>(from_hex(a[9]));
    const HistRange r = hist_range(from_hex(a[10]), from_hex(a[11]), atoi(a[12]));
    const double centre = from_hex(a[13]);
    const std::vector<char> raw = read_all(a[14]);
    char *mem = (char *)aligned_alloc(64, (raw.size() + 127) / 64 * 64);
    memcpy(mem, raw.data(), raw.size());
    const T *band0 = reinterpret_cast<const T *>(mem) + offset;

    int64_t nv = 0, nn = 0, nnan = 0, below = 0, above = 0, seen = 0;
    double mn = __builtin_inf(), mx = -__builtin_inf(), fsum = 0.0, m2 = 0.0;
    __int128 isum = 0;
    uint64_t qh = 0, ql = 0;
    std::vector<int64_t> counts((size_t)r.nbins, 0);
    for (int g = 0; g < gx; g++)
        for (int tid = 0; tid < BLOCK; tid++) {
            StatsAcc<T, MASKED> s;
            s.nd = nd;
            stats_fold<BLOCK, UNROLL>(s, band0, P, g, gx, tid);
            nv += s.n_valid, nn += s.n_nodata, nnan += s.n_nan;
            seen += (int64_t)s.n_valid + s.n_nodata + s.n_nan;
            if (s.n_valid) {
                mn = (double)s.mn < mn ? (double)s.mn : mn;
                mx = (double)s.mx > mx ? (double)s.mx : mx;
            }
            if constexpr (F) fsum = fsum + s.sum;
            else {
                isum += s.sum;
                add_u128(qh, ql, s.sq_hi, s.sq_lo);
            }
            HistAcc<T, MASKED, HostSink> h;
            h.r = r, h.centre = centre, h.nd = nd, h.sink.bins = counts.data();
            stats_fold<BLOCK, UNROLL>(h, band0, P, g, gx, tid);
            below += h.below, above += h.above;
            m2 = m2 + h.m2;
        }
    std::vector<int64_t> o = {nv, nn, nnan, bits(mn), bits(mx), (int64_t)(isum >> 64), (int64_t)(uint64_t)isum,
                              (int64_t)qh, (int64_t)ql, bits(fsum), below, above, bits(m2), seen};
    o.insert(o.end(), counts.begin(), counts.end());
    free(mem);
    return write_all(a[15], o);
}
template <typename T> static int fold_mode(char **a) {
    return atoi(a[8]) ? fold_masked<T, true>(a) : fold_masked<T, false>(a);
}

#define DISPATCH(fn, dt, a)                                  \
    do {                                                     \
        if (!strcmp(dt, "uint8")) return fn<uint8_t>(a);     \
        if (!strcmp(dt, "uint16")) return fn<uint16_t>(a);   \
        if (!strcmp(dt, "int16")) return fn<int16_t>(a);     \
        if (!strcmp(dt, "int32")) return fn<int32_t>(a);     \
        if (!strcmp(dt, "uint32")) return fn<uint32_t>(a);   \
        if (!strcmp(dt, "float32")) return fn<float>(a);     \
        if (!strcmp(dt, "float64")) return fn<double>(a);    \
        return 1;                                            \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 1;
    if (!strcmp(argv[1], "bin") && argc == 8) DISPATCH(bin_mode, argv[2], argv);
    if (!strcmp(argv[1], "fold") && argc == 16) DISPATCH(fold_mode, argv[2], argv);
    if (!strcmp(argv[1], "u128") && argc == 4) {
        const std::vector<char> raw = read_all(argv[2]);
        uint64_t hi = 0, lo = 0;
        for (size_t i = 0; i + 8 <= raw.size(); i += 8) {
            uint64_t x;
            memcpy(&x, raw.data() + i, 8);
            add_u128(hi, lo, x);
        }
        return write_all(argv[3], std::vector<uint64_t>{hi, lo});
    }
    return 1;
}
'''


def hexbits(v: float) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("stats_host")
    src = d / "stats_host.cpp"
    src.write_text(PROGRAM % HEADER)
    exe = d / "stats_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), str(src)], check=True)
    count = [0]

    def run(*args, inp: np.ndarray, out_dtype):
        count[0] += 1
        fi, fo = d / f"in{count[0]}.bin", d / f"out{count[0]}.bin"
        fi.write_bytes(np.ascontiguousarray(inp).tobytes())
        subprocess.run([str(exe), *[str(a) for a in args], str(fi), str(fo)], check=True)
        return np.frombuffer(fo.read_bytes(), dtype=out_dtype)

    return run


# ---- the bin rule
def edge_values(dtype, lo, hi):
    dt = np.dtype(dtype)
    vals = [lo, hi, np.nextafter(lo, np.inf), np.nextafter(lo, -np.inf), np.nextafter(hi, -np.inf),
            np.nextafter(hi, np.inf), (lo + hi) / 2, lo + (hi - lo) / 3]
    if dt.kind == "f":
        vals += [np.inf, -np.inf, 0.0, -0.0]
        a = np.array(vals, dtype=np.float64).astype(dt)
    else:
        ii = np.iinfo(dt)
        vals += [ii.min, ii.max, ii.min + 1, ii.max - 1, 0, 1]
        a = np.clip(np.floor(np.array(vals, dtype=np.float64)), ii.min, ii.max).astype(dt)
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbins", [1, 2, 7, 256, 16384])
def test_bin_rule_at_the_edges(prog, dtype, nbins):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        ranges = [(-3.5, 10.25), (0.0, 1.0), (-1e30, 1e30)]
    else:
        ii = np.iinfo(dt)
        ranges = [(float(ii.min), float(ii.max)), (float(ii.min) + 3, float(ii.min) + 40), (10.0, 200.0)]
    for lo, hi in ranges:
        vals = edge_values(dtype, lo, hi)
        got = prog("bin", dtype, hexbits(lo), hexbits(hi), nbins, inp=vals, out_dtype=np.int32)
        want = [R.bin_index(float(v), lo, hi, nbins) for v in vals.astype(np.float64)]
        assert got.tolist() == want, (lo, hi)


def test_bin_rule_clamps_a_product_that_rounds_up_to_nbins(prog):
    # x == hi always lands on nbins; so do some x just below hi, whose product (x - lo) * scale rounds up to it
    rng = np.random.default_rng(11)
    found = 0
    for _ in range(2000):
        lo, hi, nbins = float(rng.uniform(-5, 5)), float(rng.uniform(6, 50)), int(rng.integers(1, 16385))
        x = np.nextafter(hi, 0)
        scale = np.float64(nbins) / (np.float64(hi) - np.float64(lo))
        if np.floor((x - lo) * scale) < nbins:
            continue
        found += 1
        xs = np.array([hi, x, np.nextafter(x, 0)], dtype=np.float64)
        got = prog("bin", "float64", hexbits(lo), hexbits(hi), nbins, inp=xs, out_dtype=np.int32)
        assert got[0] == got[1] == nbins - 1
        assert got.tolist() == [R.bin_index(v, lo, hi, nbins) for v in xs]
        if found == 10:
            break
    assert found  # the case exists: without the clamp the index would be out of range


@pytest.mark.parametrize("dtype", DTYPES[:5])
def test_per_value_bins_at_both_ends_of_the_dtype(prog, dtype):
    ii = np.iinfo(dtype)
    for m, M in [(ii.min, ii.min + 255), (ii.max - 255, ii.max), (ii.max - 16383, ii.max) if ii.max > 16384 else (0, 255)]:
        lo, hi, nbins = S.histogram_range(dtype, m, M, 16384)
        assert (lo, hi, nbins) == (float(m), float(M + 1), M - m + 1)
        vals = np.array([m, m + 1, (m + M) // 2, M - 1, M], dtype=dtype)
        got = prog("bin", dtype, hexbits(lo), hexbits(hi), nbins, inp=vals, out_dtype=np.int32)
        assert got.tolist() == [int(v) - m for v in vals]


# ---- 128-bit carries
def test_add_u128_carries(prog):
    for vals in ([2 ** 62] * 8, [2 ** 64 - 1] * 5, [(2 ** 32 - 1) ** 2] * 9, [0, 1, 2 ** 64 - 1, 1]):
        hi, lo = prog("u128", inp=np.array(vals, dtype=np.uint64), out_dtype=np.uint64)
        assert (int(hi) << 64) + int(lo) == sum(vals)


# ---- the lane functions, lane by lane
def run_fold(prog, big, offset, h, w, row_stride, gx, nodata, lo, hi, nbins, centre=0.0):
    out = prog("fold", str(big.dtype), h, w, row_stride, offset, gx, 0 if nodata is None else 1,
               hexbits(0.0 if nodata is None else nodata), hexbits(lo), hexbits(hi), nbins, hexbits(centre),
               inp=big, out_dtype=np.int64)
    f = lambda i: struct.unpack("<d", struct.pack("<q", int(out[i])))[0]  # noqa: E731
    return {"n_valid": int(out[0]), "n_nodata": int(out[1]), "n_nan": int(out[2]), "min": f(3), "max": f(4),
            "isum": (int(out[5]) << 64) + (int(out[6]) & (2 ** 64 - 1)),
            "isq": ((int(out[7]) & (2 ** 64 - 1)) << 64) + (int(out[8]) & (2 ** 64 - 1)),
            "fsum": f(9), "below": int(out[10]), "above": int(out[11]), "m2": f(12), "seen": int(out[13]),
            "counts": out[14:]}


def check_fold(got, band, nodata, lo, hi, nbins, centre=0.0):
    want = R.band_stats(band, nodata)
    hist = R.histogram(band, lo, hi, nbins, nodata, centre)
    assert got["seen"] == band.size  # every pixel once: nothing outside [height][width], nothing twice
    assert (got["n_valid"], got["n_nodata"], got["n_nan"]) == (want["n_valid"], want["n_nodata"], want["n_nan"])
    if want["n_valid"]:
        assert got["min"] == want["min"] and got["max"] == want["max"]
    if band.dtype.kind in "iu":
        assert got["isum"] == want["isum"] and got["isq"] == want["isq"]
    elif np.isfinite(band[R.classes(band, nodata)[0]]).all():
        n = want["n_valid"]
        assert abs(got["fsum"] - want["fsum"]) <= R.gamma(n - 1) * want["abs_sum"]
        t = hist["m2_terms"]
        assert abs(got["m2"] - math.fsum(t)) <= (R.gamma(n - 1) + R.U) * math.fsum(t)
    assert got["counts"].tolist() == hist["counts"].tolist()
    assert (got["below"], got["above"]) == (hist["below"], hist["above"])


def make_band(rng, dtype, h, w):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal((h, w)) * 100).astype(dt)
    ii = np.iinfo(dt)
    span = min(int(ii.max) - int(ii.min), 1000)
    return (rng.integers(0, span + 1, (h, w)) + max(int(ii.min), -500)).astype(dt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_functions_over_small_rasters(prog, dtype):
    rng = np.random.default_rng(DTYPES.index(dtype))
    dt = np.dtype(dtype)
    for h, w, pad, offset, gx in [(1, 1, 0, 0, 1), (5, 7, 0, 1, 2), (3, 33, 5, 3, 1), (6, 40, 0, 0, 3),
                                  (9, 9, 7, 2, 2), (2, 300, 1, 5, 2)]:
        rs = w + pad
        big = make_band(rng, dtype, 1, offset + h * rs + 16).ravel()
        # the surround: below the minimum, above the maximum, and the nodata value
        band = big[offset:offset + h * rs].reshape(h, rs)[:, :w]
        nodata = float(band.flat[0])
        lo, hi = float(np.percentile(band, 10)), float(np.percentile(band, 90)) + 1.0
        keep = band.copy()
        big[:] = nodata
        big[::3] = dt.type(np.iinfo(dt).min if dt.kind in "iu" else -1e30)
        big[1::3] = dt.type(np.iinfo(dt).max if dt.kind in "iu" else 1e30)
        big[offset:offset + h * rs].reshape(h, rs)[:, :w] = keep
        for nd in (None, nodata):
            for nbins in (1, 5, 64):
                got = run_fold(prog, big, offset, h, w, rs, gx, nd, lo, hi, nbins, centre=float(band.mean()))
                check_fold(got, keep, nd, lo, hi, nbins, centre=float(band.mean()))


def test_lane_function_32_bit_carries(prog):
    a = np.full((1, 8), -2 ** 31, dtype=np.int32)  # the squares add up to 2^65
    got = run_fold(prog, a.ravel(), 0, 1, 8, 8, 1, None, -2.0 ** 31, -2.0 ** 31 + 1, 1)
    assert got["isq"] == 8 * 2 ** 62 and got["isum"] == -8 * 2 ** 31 and got["counts"].tolist() == [8]
    b = np.full((3, 11), 2 ** 32 - 1, dtype=np.uint32)
    got = run_fold(prog, b.ravel(), 0, 3, 11, 11, 2, None, 0.0, 2.0 ** 32, 16)
    assert got["isq"] == 33 * (2 ** 32 - 1) ** 2 and got["isum"] == 33 * (2 ** 32 - 1)
    assert got["counts"].tolist() == [0] * 15 + [33]


def test_lane_function_float_classes(prog):
    a = np.array([[np.nan, 1.5, np.inf, -np.inf, 0.0, -0.0, 7.0, np.nan, 2.0]], dtype=np.float32)
    for nd in (None, float("nan"), float("-inf"), 0.0):
        got = run_fold(prog, a.ravel(), 0, 1, 9, 9, 1, nd, 0.0, 8.0, 8)
        check_fold(got, a, nd, 0.0, 8.0, 8)


# ---- the Python rules
def test_histogram_range():
    assert S.histogram_range(np.uint16, 10, 265, 256) == (10.0, 266.0, 256)         # range + 1 == bins: per value
    assert S.histogram_range(np.uint16, 10, 266, 256) == (10.0, 266.0, 256)         # one more: binned over [min, max]
    assert S.histogram_range(np.int16, -5, 250, 256) == (-5.0, 251.0, 256)          # range + 1 == bins: per value
    assert S.histogram_range(np.int16, -5, 251, 256) == (-5.0, 251.0, 256)          # one more: binned over [min, max]
    assert S.histogram_range(np.int16, 7, 7, 256) == (7.0, 8.0, 1)
    assert S.histogram_range(np.float32, 2.5, 2.5, 16) == (2.5, 3.5, 16)
    assert S.histogram_range(np.float64, -1.0, 3.0, 100) == (-1.0, 3.0, 100)
    for bad in (0, 16385, -1):
        with pytest.raises(ValueError):
            S.histogram_range(np.uint8, 0, 1, bad)


def per_value_hist(v):
    m, M = int(v.min()), int(v.max())
    lo, hi, nbins = S.histogram_range(v.dtype, m, M, 16384)
    h = R.histogram(v, lo, hi, nbins)
    return {"lo": m, "hi": M + 1, "counts": h["counts"].tolist(), "per_value": True}


def test_percentile_is_the_sorted_value():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 100, 1001):
        v = rng.integers(-300, 5000, n).astype(np.int16)
        h = per_value_hist(v)
        for q in (0, 2, 50, 98, 100):
            assert S.percentile(h, q) == R.percentile_sorted(v.tolist(), q)


def test_percentile_matches_numpy_inverted_cdf():
    rng = np.random.default_rng(6)
    for q, n in [(2, 77), (50, 33), (98, 101), (25, 10), (75, 7), (37, 53)]:
        assert (q * n) % 100 != 0
        v = rng.integers(0, 1000, n).astype(np.uint16)
        assert S.percentile(per_value_hist(v), q) == int(np.percentile(v, q, method="inverted_cdf"))


def test_binned_percentile_is_within_half_a_bin():
    rng = np.random.default_rng(7)
    v = (rng.standard_normal(5000) * 50 + 10).astype(np.float32)
    lo, hi, nbins = S.histogram_range(v.dtype, float(v.min()), float(v.max()), 64)
    h = R.histogram(v, lo, hi, nbins)
    hist = {"lo": lo, "hi": hi, "counts": h["counts"].tolist(), "per_value": False}
    bound = (hi - lo) / nbins / 2 + np.spacing(hi)
    for q in (0, 2, 50, 98, 100):
        exact = float(R.percentile_sorted(v.astype(np.float64).tolist(), q))
        assert abs(S.percentile(hist, q) - exact) <= bound
    assert S.percentile({"lo": 0, "hi": 1, "counts": [0, 0], "per_value": False}, 50) is None


def test_mean_std_from_hand_made_128_bit_sums():
    cases = [[-2 ** 31] * 8 + [2 ** 31 - 1], [2 ** 32 - 1] * 1000 + [0], [1, 2, 3, 4], [5], [-7, -7, -7],
             list(range(-1000, 2000, 7))]
    for vals in cases:
        n, isum, isq = len(vals), sum(vals), sum(v * v for v in vals)
        mean, std = S.mean_std_from_sums(n, isum, isq)
        fm, var = R.mean_std(vals)
        assert mean == float(fm)  # float(Fraction) rounds once, to nearest
        assert R.is_nearest_sqrt(std, var)
    # a sum of squares beyond 2^64 really is needed
    assert sum(v * v for v in cases[0]) > 2 ** 64


def test_index_key_round_trip_with_non_finite_numbers():
    band = {"valid": 3, "nodata_count": 1, "nan": 2, "min": -math.inf, "max": math.inf, "mean": math.nan,
            "std": math.nan, "histogram": {"lo": 0.0, "hi": 1.0, "counts": [1, 0], "below": 1, "above": 1,
                                           "per_value": False}}
    idx = S.statistics_to_index(band)
    text = json.dumps({"statistics": idx}, allow_nan=False)  # plain JSON: no NaN / Infinity tokens
    back = streaming.index_statistics(json.loads(text))
    assert back["min"] == -math.inf and back["max"] == math.inf and math.isnan(back["mean"]) and math.isnan(back["std"])
    assert back["histogram"] == band["histogram"] and back["valid"] == 3
    assert idx["min"] == streaming._nodata_to_index(-math.inf) and idx["mean"] == streaming._nodata_to_index(math.nan)
    empty = dict(band, valid=0, min=None, max=None, mean=None, std=None, histogram=None)
    assert streaming.index_statistics({"statistics": S.statistics_to_index(empty)}) == empty
    assert streaming.index_statistics({"frames": []}) is None


# ---- the commands
def hand_made_streaming(path: Path, with_stats: bool):
    index = {"crs": "EPSG:4326", "transform": [1.0, 0.0, 0.0, 0.0, -1.0, 0.0], "width": 4, "height": 4, "tile_size": 4,
             "frames": []}
    if with_stats:
        index["statistics"] = S.statistics_to_index(
            {"valid": 16, "nodata_count": 0, "nan": 0, "min": 3, "max": 12, "mean": 7.5, "std": 2.25,
             "histogram": {"lo": 3, "hi": 13, "counts": [1] * 10, "below": 0, "above": 0, "per_value": True}})
    path.write_bytes(streaming.streaming_head(index))


def test_info_prints_the_stored_statistics(tmp_path):
    runner = CliRunner()
    hand_made_streaming(tmp_path / "with.flac", True)
    hand_made_streaming(tmp_path / "without.flac", False)
    r = runner.invoke(app, ["info", str(tmp_path / "with.flac")])
    assert r.exit_code == 0 and "Statistics (level 0)" in r.output
    assert "Minimum: 3" in r.output and "Maximum: 12" in r.output and "Mean: 7.5" in r.output
    r = runner.invoke(app, ["info", str(tmp_path / "without.flac")])
    assert r.exit_code == 0 and "Streaming format: Yes" in r.output and "Statistics" not in r.output


def test_stats_argument_errors(tmp_path):
    runner = CliRunner()
    tif = str(GOLDEN / "sample_dem.tif")
    hand_made_streaming(tmp_path / "s.flac", False)
    cases = [
        (["stats", str(tmp_path / "missing.tif")], "does not exist"),
        (["stats", tif, "--level", "1"], "--level applies to streaming FLAC files"),
        (["stats", tif, "--bins", "0"], "--bins must be 1..16384"),
        (["stats", tif, "--bins", "16385"], "--bins must be 1..16384"),
        (["stats", tif, "--nodata", "abc"], "--nodata must be a number or 'none'"),
        (["stats", tif, "--nodata", "0.5"], "is not an integer inside the range of int16"),
        (["stats", tif, "--nodata", "40000"], "is not an integer inside the range of int16"),
        (["stats", tif, "--percentiles", "2,x"], "--percentiles"),
        (["stats", tif, "--percentiles", "101"], "--percentiles"),
        (["stats", str(tmp_path / "s.flac"), "--level", "3"], "level 3"),
    ]
    (tmp_path / "x.png").write_bytes(b"")
    cases.append((["stats", str(tmp_path / "x.png")], "Unsupported file format"))
    for argv, text in cases:
        r = runner.invoke(app, argv)
        assert r.exit_code == 1, argv
        assert "Error" in r.output and text in r.output, (argv, r.output)


def test_create_streaming_stats_rejects_several_gpus(tmp_path):
    runner = CliRunner()
    tif = str(GOLDEN / "sample_dem.tif")
    for extra in (["--gpus", "2"], ["--distributed"]):
        r = runner.invoke(app, ["create-streaming", tif, "-o", str(tmp_path / "o.flac"), "--stats"] + extra)
        assert r.exit_code == 1
        assert "--stats runs on one GPU: it cannot be combined with --gpus > 1 or --distributed" in r.output
    assert not (tmp_path / "o.flac").exists()


def test_nodata_the_dtype_cannot_hold_is_a_value_error():
    # (the stats command turns it into "Error: ..." / exit status 1; the conversion itself needs no GPU)
    with pytest.raises(ValueError):
        streaming.nodata_for_dtype(-1.0, np.uint8)
    with pytest.raises(ValueError):
        streaming.nodata_for_dtype(0.5, np.int16)
