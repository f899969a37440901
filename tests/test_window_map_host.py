"""The arithmetic of the windowed resample, csrc/frs_window_map.h, built with the host compiler into a small program
of its own and compared bit for bit with the numpy restatement tests/window_ref.py: per-axis indices, weights and
validity of every mode, the bilinear expression, and the rounding and clamp at every dtype's range ends.  No GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import window_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_window_map.h"

# window_map_host axis X0 SPAN n N OUT WEIGHTS   (X0, SPAN: the doubles' bit patterns in hex)
#     OUT gets 11 8-byte fields per destination pixel: nearest i, valid; bilinear i0, i1, t, valid; average clo, chi,
#     i0, i1, valid (doubles as their bits); WEIGHTS the average's tap weights, pixel after pixel
# window_map_host conv DTYPE IN OUT       IN doubles -> OUT win_result<DTYPE>
# window_map_host bilin IN OUT            IN rows of a b c d tx ty -> OUT doubles
# window_map_host norm IN OUT             IN rows of sum xclo xchi yclo ychi -> OUT win_area_value
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "%s"

static int64_t bits(double v) { int64_t b; memcpy(&b, &v, 8); return b; }
static double from_hex(const char *s) { const uint64_t b = strtoull(s, nullptr, 16); double v; memcpy(&v, &b, 8); return v; }

static std::vector<double> read_doubles(const char *path) {
    std::vector<double> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    v.resize((size_t)ftell(f) / 8);
    fseek(f, 0, SEEK_SET);
    if (fread(v.data(), 8, v.size(), f) != v.size()) exit(3);
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
template <typename T> static int conv(const char *in, const char *out) {
    const std::vector<double> v = read_doubles(in);
    std::vector<T> o(v.size());
    for (size_t i = 0; i < v.size(); i++) o[i] = frs::win_result<T>(v[i]);
    return write_all(out, o);
}

int main(int argc, char **argv) {
    if (argc < 2) return 1;
    if (!strcmp(argv[1], "axis") && argc == 8) {
        const int64_t n = atoll(argv[4]), N = atoll(argv[5]);
        const frs::WinAxis a = frs::win_axis(from_hex(argv[2]), from_hex(argv[3]), n, N);
        std::vector<int64_t> o;
        std::vector<double> wts;
        for (int64_t j = 0; j < n; j++) {
            const frs::WinNearest q = frs::win_nearest(a, j);
            const frs::WinLinear l = frs::win_linear(a, j);
            const frs::WinArea r = frs::win_area(a, j);
            const int64_t rec[11] = {q.i, q.valid, l.i0, l.i1, bits(l.t), l.valid, bits(r.clo), bits(r.chi), r.i0, r.i1,
                                     r.valid};
            o.insert(o.end(), rec, rec + 11);
            for (int64_t i = r.i0; i < r.i1; i++) wts.push_back(frs::win_area_weight(r, i));
        }
        if (int rc = write_all(argv[6], o)) return rc;
        return write_all(argv[7], wts);
    }
    if (!strcmp(argv[1], "conv") && argc == 5) {
        const char *dt = argv[2];
        if (!strcmp(dt, "uint8")) return conv<uint8_t>(argv[3], argv[4]);
        if (!strcmp(dt, "uint16")) return conv<uint16_t>(argv[3], argv[4]);
        if (!strcmp(dt, "int16")) return conv<int16_t>(argv[3], argv[4]);
        if (!strcmp(dt, "int32")) return conv<int32_t>(argv[3], argv[4]);
        if (!strcmp(dt, "uint32")) return conv<uint32_t>(argv[3], argv[4]);
        if (!strcmp(dt, "float32")) return conv<float>(argv[3], argv[4]);
        if (!strcmp(dt, "float64")) return conv<double>(argv[3], argv[4]);
        return 1;
    }
    if (!strcmp(argv[1], "bilin") && argc == 4) {
        const std::vector<double> v = read_doubles(argv[2]);
        std::vector<double> o(v.size() / 6);
        for (size_t i = 0; i < o.size(); i++) {
            const double *p = v.data() + 6 * i;
            o[i] = frs::win_bilinear_value(p[0], p[1], p[2], p[3], p[4], p[5]);
        }
        return write_all(argv[3], o);
    }
    if (!strcmp(argv[1], "norm") && argc == 4) {
        const std::vector<double> v = read_doubles(argv[2]);
        std::vector<double> o(v.size() / 5);
        for (size_t i = 0; i < o.size(); i++) {
            const double *p = v.data() + 5 * i;
            frs::WinArea x, y;
            x.clo = p[1], x.chi = p[2], y.clo = p[3], y.chi = p[4];
            o[i] = frs::win_area_value(p[0], x, y);
        }
        return write_all(argv[3], o);
    }
    return 1;
}
'''


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_map_host")
    src = d / "window_map_host.cpp"
    src.write_text(PROGRAM % HEADER)
    exe = d / "window_map_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe), str(src)],
                   check=True)

    def run(*args, inp=None, out_dtype=np.float64):
        fin, fout = d / "in.bin", d / "out.bin"
        if inp is not None:
            np.ascontiguousarray(inp, dtype=np.float64).tofile(fin)
        subprocess.run([str(exe), *[str(a) for a in args], *([str(fin)] if inp is not None else []), str(fout)],
                       check=True)
        return np.fromfile(fout, dtype=out_dtype)
    run.dir = d
    run.exe = exe
    return run


def hexbits(v):
    return format(int(np.float64(v).view(np.uint64)), "x")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# (name, x0, span, n, N): the rectangles of the issue on one axis, N = 37 and 53 as in the GPU test
def axis_cases():
    out = []
    for N in (37, 53):
        for n in (1, 5, 7, 8, 9, 33, 40, 300):
            out += [("scale_to_fit", 0.0, float(N), n, N), ("exact_2x", 1.0, 2.0 * n, n, N),
                    ("1.37x", 0.25, 1.37 * n, n, N), ("0.4x_upsampling", 3.3, 0.4 * n, n, N),
                    ("9.3x", -2.0, 9.3 * n, n, N), ("over_low_edge", -5.5, 20.0, n, N),
                    ("over_high_edge", N - 10.5, 20.0, n, N), ("over_both_edges", -3.0, N + 7.5, n, N),
                    ("outside_high", N + 3.0, 10.0, n, N), ("outside_low", -20.0, 10.0, n, N),
                    ("lo_on_pixel_edges", 4.0, 0.5 * n, n, N)]
        out.append(("identity", 0.0, float(N), N, N))
    return out


@pytest.mark.parametrize("case", axis_cases(), ids=lambda c: f"{c[0]}-n{c[3]}-N{c[4]}")
def test_axis_indices_weights_and_validity(prog, case):
    _, x0, span, n, N = case
    wfile = prog.dir / "weights.bin"
    subprocess.run([str(prog.exe), "axis", hexbits(x0), hexbits(span), str(n), str(N), str(prog.dir / "axis.bin"),
                    str(wfile)], check=True)
    got = np.fromfile(prog.dir / "axis.bin", dtype=np.int64).reshape(n, 11)
    ni, nv = R.nearest_axis(x0, span, n, N)
    l0, l1, lt, lv = R.linear_axis(x0, span, n, N)
    clo, chi, a0, a1, av = R.area_axis(x0, span, n, N)
    want = np.stack([ni, nv.astype(np.int64), l0, l1, bits(lt), lv.astype(np.int64), bits(clo), bits(chi), a0, a1,
                     av.astype(np.int64)], axis=1)
    assert np.array_equal(got, want)
    ww = [R.area_weight(clo[j], chi[j], np.arange(a0[j], a1[j])) for j in range(n)]
    ww = np.concatenate(ww) if ww else np.zeros(0)
    assert np.array_equal(bits(np.fromfile(wfile, dtype=np.float64)), bits(ww))
    # what the definition promises: taps inside the source, positive weights that add up to the clipped interval
    assert np.all((a0[av] >= 0) & (a1[av] <= N) & (a1[av] > a0[av]))
    assert np.all(ww > 0)
    assert np.all((l0 >= 0) & (l1 <= N - 1)) and np.all((ni >= 0) & (ni < N))


def test_identity_axis_is_one_tap_of_weight_one(prog):
    for N in (37, 53):
        clo, chi, a0, a1, av = R.area_axis(0.0, float(N), N, N)
        assert av.all() and np.array_equal(a0, np.arange(N)) and np.array_equal(a1, np.arange(N) + 1)
        assert np.array_equal(chi - clo, np.ones(N))
        i0, i1, t, lv = R.linear_axis(0.0, float(N), N, N)
        assert lv.all() and np.array_equal(i0, np.arange(N)) and np.array_equal(t, np.zeros(N))
        ni, nv = R.nearest_axis(0.0, float(N), N, N)
        assert nv.all() and np.array_equal(ni, np.arange(N))


def range_end_values(dtype):
    """the doubles around both range ends and around 0, with their halves, and far outside"""
    ends = [0.0]
    if np.dtype(dtype).kind == "f":
        fi = np.finfo(dtype)
        ends += [float(fi.max), float(fi.min), float(fi.tiny), 1e300, -1e300, 1e-320]
    else:
        ii = np.iinfo(dtype)
        ends += [float(ii.min), float(ii.max)]
    vals = []
    for e in ends:
        for d in (-2.0, -1.5, -1.0, -0.5000000001, -0.5, -0.4999999999, -0.25, 0.0, 0.25, 0.4999999999, 0.5,
                  0.5000000001, 1.0, 1.5, 2.0, 2.5, 3.5):
            vals.append(e + d)
        with np.errstate(over="ignore"):  # past float64's largest value: inf
            vals += [np.nextafter(e, np.inf), np.nextafter(e, -np.inf)]
    vals += [1e19, -1e19, 2.0 ** 63, -2.0 ** 63, 1e300, -1e300, -0.0]
    if np.dtype(dtype).kind == "f":
        vals += [np.nan, np.inf, -np.inf]
    return np.array(vals, dtype=np.float64)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_rounding_and_clamp_at_the_range_ends(prog, dtype):
    v = range_end_values(dtype)
    got = prog("conv", np.dtype(dtype).name, inp=v, out_dtype=dtype)
    want = R.to_dtype(v, dtype)
    assert got.tobytes() == want.tobytes()
    if np.dtype(dtype).kind != "f":  # and against exact Python arithmetic: half to even, then the clamp
        ii = np.iinfo(dtype)
        assert [int(g) for g in got] == [min(max(round(float(x)), ii.min), ii.max) for x in v]


def test_random_values_round_half_to_even(prog):
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(-70000, 70000, 20000) + 0.5, rng.uniform(-70000, 70000, 20000)])
    for dtype in (np.uint8, np.int16, np.uint16, np.int32):
        ii = np.iinfo(dtype)
        got = prog("conv", np.dtype(dtype).name, inp=v, out_dtype=dtype)
        assert [int(g) for g in got] == [min(max(round(float(x)), ii.min), ii.max) for x in v]


def test_bilinear_expression_and_area_divisor(prog):
    rng = np.random.default_rng(6)
    rows = np.concatenate([rng.uniform(-1e6, 1e6, (5000, 4)), rng.uniform(0, 1, (5000, 2))], axis=1)
    rows[:50, 4] = 0.0
    rows[50:100, 5] = 0.0
    rows[100, 1] = np.inf
    rows[101, 2] = np.nan
    a, b, c, d, tx, ty = rows.T
    with np.errstate(invalid="ignore"):
        want = (a * (1.0 - tx) + b * tx) * (1.0 - ty) + (c * (1.0 - tx) + d * tx) * ty
    assert np.array_equal(bits(prog("bilin", inp=rows)), bits(want))
    q = np.concatenate([rng.uniform(-1e9, 1e9, (5000, 1)), np.sort(rng.uniform(0, 50, (5000, 2)), axis=1),
                        np.sort(rng.uniform(0, 50, (5000, 2)), axis=1)], axis=1)
    s, xlo, xhi, ylo, yhi = q.T
    assert np.array_equal(bits(prog("norm", inp=q)), bits(s / ((xhi - xlo) * (yhi - ylo))))
