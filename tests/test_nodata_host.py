"""Host side of nodata through the streaming path: the arithmetic of csrc/frs_nodata.h built with the host compiler into
a small program of its own (the masked 2x average against exact Python integers and numpy's expressions, the nudge, the
masked bilinear and average accumulations against tests/nodata_ref.py), streaming.nodata_for_dtype, the tile tag, the
index key through level_index, and the CLI's rejections.  No GPU."""
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, container, geotiff, streaming
from flac_raster_amd.cli import app
from tests import nodata_ref as N

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "flac_raster_amd" / "csrc"
HEADER = CSRC / "frs_nodata.h"
runner = CliRunner()

INT_DTYPES = [np.uint8, np.uint16, np.int16, np.int32, np.uint32]
FLOAT_DTYPES = [np.float32, np.float64]

# nodata_host avg DTYPE N ND IN OUT      IN: blocks of N elements (a, b[, c, d]); OUT: one masked average per block
# nodata_host res DTYPE ND FILL IN OUT   IN: (value, valid) pairs of doubles; OUT: nd_win_result per pair
# nodata_host bil IN OUT                 IN: records a b c d oa ob oc od tx ty (doubles); OUT: (value, valid) per record
# nodata_host area NY NX IN OUT          IN: records of wy[NY] wx[NX] v[NY*NX] ok[NY*NX] clo_x chi_x clo_y chi_y;
#                                        OUT: (value, valid) per record
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "%s"

template <typename T> static std::vector<T> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
    fclose(f);
    return v;
}
template <typename T> static int dump(const char *path, const std::vector<T> &o) {
    FILE *f = fopen(path, "wb");
    if (!f) return 4;
    fwrite(o.data(), sizeof(T), o.size(), f);
    fclose(f);
    return 0;
}

template <typename T> static int avg(int n, double ndd, const char *in, const char *out) {
    if (!frs::nd_representable<T>(ndd)) return 5;
    const T nd = frs::nd_cast<T>(ndd);
    const std::vector<T> v = slurp<T>(in);
    std::vector<T> o(v.size() / (size_t)n);
    for (size_t i = 0; i < o.size(); i++) {
        const T *p = v.data() + i * (size_t)n;
        o[i] = frs::nd_avg(p[0], p[n >= 2 ? 1 : 0], p[n == 4 ? 2 : 0], p[n == 4 ? 3 : 0], n, nd);
    }
    return dump(out, o);
}

template <typename T> static int res(double ndd, double fill, const char *in, const char *out) {
    if (!frs::nd_representable<T>(ndd) || !frs::nd_fill_ok<T>(fill)) return 5;
    const std::vector<double> v = slurp<double>(in);
    std::vector<T> o(v.size() / 2);
    for (size_t i = 0; i < o.size(); i++) {
        frs::NdValue r;
        r.v = v[2 * i], r.valid = v[2 * i + 1] != 0.0;
        o[i] = frs::nd_win_result<T>(r, frs::win_result<T>(fill), frs::nd_cast<T>(ndd));
    }
    return dump(out, o);
}

#define BY_DTYPE(call)                                  \
    if (!strcmp(dt, "uint8")) return call(uint8_t);     \
    if (!strcmp(dt, "uint16")) return call(uint16_t);   \
    if (!strcmp(dt, "int16")) return call(int16_t);     \
    if (!strcmp(dt, "int32")) return call(int32_t);     \
    if (!strcmp(dt, "uint32")) return call(uint32_t);   \
    if (!strcmp(dt, "float32")) return call(float);     \
    if (!strcmp(dt, "float64")) return call(double);

int main(int argc, char **argv) {
    if (argc < 2) return 1;
    if (!strcmp(argv[1], "avg") && argc == 7) {
        const char *dt = argv[2];
        const int n = atoi(argv[3]);
        if (n != 1 && n != 2 && n != 4) return 1;
#define AVG(T) avg<T>(n, strtod(argv[4], nullptr), argv[5], argv[6])
        BY_DTYPE(AVG)
        return 1;
    }
    if (!strcmp(argv[1], "res") && argc == 7) {
        const char *dt = argv[2];
#define RES(T) res<T>(strtod(argv[3], nullptr), strtod(argv[4], nullptr), argv[5], argv[6])
        BY_DTYPE(RES)
        return 1;
    }
    if (!strcmp(argv[1], "bil") && argc == 4) {
        const std::vector<double> v = slurp<double>(argv[2]);
        std::vector<double> o(v.size() / 10 * 2);
        for (size_t i = 0; i < v.size() / 10; i++) {
            const double *p = v.data() + 10 * i;
            const frs::NdValue r = frs::nd_bilinear(p[0], p[1], p[2], p[3], p[4] != 0.0, p[5] != 0.0, p[6] != 0.0,
                                                    p[7] != 0.0, p[8], p[9]);
            o[2 * i] = r.v, o[2 * i + 1] = r.valid ? 1.0 : 0.0;
        }
        return dump(argv[3], o);
    }
    if (!strcmp(argv[1], "area") && argc == 6) {
        const int ny = atoi(argv[2]), nx = atoi(argv[3]);
        const size_t rec = (size_t)(ny + nx + 2 * ny * nx + 4);
        const std::vector<double> v = slurp<double>(argv[4]);
        std::vector<double> o(v.size() / rec * 2);
        for (size_t i = 0; i < v.size() / rec; i++) {
            const double *wy = v.data() + rec * i, *wx = wy + ny, *val = wx + nx, *ok = val + ny * nx, *lim = ok + ny * nx;
            frs::NdArea acc;
            for (int j = 0; j < ny; j++) {
                for (int k = 0; k < nx; k++) acc.tap(wx[k], val[j * nx + k], ok[j * nx + k] != 0.0);
                acc.end_row(wy[j]);
            }
            frs::WinArea rx, ry;
            rx.clo = lim[0], rx.chi = lim[1], ry.clo = lim[2], ry.chi = lim[3];
            rx.i0 = ry.i0 = 0, rx.i1 = nx, ry.i1 = ny, rx.valid = ry.valid = true;
            const frs::NdValue r = acc.value(rx, ry);
            o[2 * i] = r.v, o[2 * i + 1] = r.valid ? 1.0 : 0.0;
        }
        return dump(argv[5], o);
    }
    return 1;
}
'''


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """run(args..., input array) -> the program's output bytes"""
    d = tmp_path_factory.mktemp("nodata_host")
    src = d / "nodata_host.cpp"
    src.write_text(PROGRAM % HEADER)
    exe = d / "nodata_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe), str(src)],
                   check=True)

    def run(args, data: np.ndarray, out_dtype, ok=True):
        fin, fout = d / "in.bin", d / "out.bin"
        np.ascontiguousarray(data).tofile(fin)
        p = subprocess.run([str(exe), *[str(a) for a in args], str(fin), str(fout)])
        if not ok:
            return p.returncode
        assert p.returncode == 0, (args, p.returncode)
        return np.fromfile(fout, dtype=out_dtype)
    return run


def _avg(prog, blocks, nd):
    blocks = np.ascontiguousarray(blocks)
    out = prog(["avg", blocks.dtype.name, blocks.shape[1], repr(float(nd))], blocks, blocks.dtype)
    assert out.shape == (blocks.shape[0],)
    return out


def edge_values(dtype):
    """min, min+1, -1, 0, 1, max-1, max: those the dtype holds, once each"""
    ii = np.iinfo(dtype)
    return sorted({v for v in (ii.min, ii.min + 1, -1, 0, 1, ii.max - 1, ii.max) if ii.min <= v <= ii.max})


def exact_masked_average(block, nd, dtype):
    """the definition in Python integers"""
    ii = np.iinfo(dtype)
    valid = [int(v) for v in block if int(v) != nd]
    m = len(valid)
    if m == 0:
        return nd
    q = (2 * sum(valid) + m) // (2 * m)
    if q == nd:
        q = nd - 1 if nd == ii.max else nd + 1
    return q


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", [1, 2, 4])
def test_integer_masked_average_every_validity_pattern_of_edge_values(prog, dtype, n):
    """every block of edge values with nodata at the dtype's min, 0 and max: since nodata is one of the values drawn,
    all 2^n - 1 validity patterns with a valid pixel (15, 3, 1) and the all-nodata block occur, with every value"""
    ii = np.iinfo(dtype)
    blocks = np.array(list(itertools.product(edge_values(dtype), repeat=n)), dtype=dtype)
    for nd in sorted({ii.min, 0, ii.max}):
        patterns = {tuple(int(v) != nd for v in row) for row in blocks}
        assert len(patterns) == 2 ** n
        got = _avg(prog, blocks, nd)
        assert [int(v) for v in got] == [exact_masked_average(row, nd, dtype) for row in blocks], nd


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_integer_masked_average_random_blocks(prog, dtype):
    rng = np.random.default_rng(61)
    ii = np.iinfo(dtype)
    for n in (4, 2):
        for nd in (ii.min, 0, ii.max, 5):
            blocks = rng.integers(ii.min, ii.max, size=(20000, n), dtype=dtype, endpoint=True)
            small = rng.integers(max(ii.min, -3) if nd in (0, 5) else ii.min, 9, size=(20000, n), endpoint=True)
            blocks[10000:] = small[10000:].astype(dtype)  # blocks near 0 and 5, whose means land on them
            blocks[rng.random(blocks.shape) < 0.3] = nd
            got = _avg(prog, blocks, nd)
            assert [int(v) for v in got] == [exact_masked_average(row, nd, dtype) for row in blocks], (n, nd)


def test_the_nudge_at_both_ends_and_inside(prog):
    i16, u8 = np.int16, np.uint8
    assert _avg(prog, np.array([[4, 6, 4, 6]], i16), 5)[0] == 6             # the mean lands on nodata: + 1
    assert _avg(prog, np.array([[4, 6, 5, 5]], i16), 5)[0] == 6             # two valid
    assert _avg(prog, np.array([[-1, 1, 0, 0]], i16), 0)[0] == 1
    assert _avg(prog, np.array([[4, 4, 4, 5]], i16), 5)[0] == 4             # no hit: untouched
    assert _avg(prog, np.array([[5, 5, 5, 5]], i16), 5)[0] == 5             # m = 0: nodata itself
    # at the ends of the range a mean of valid pixels cannot reach nodata; the windowed result, which clamps, can
    for dtype in INT_DTYPES:
        ii = np.iinfo(dtype)
        pairs = np.array([[float(ii.max), 1.0], [float(ii.max) + 10.0, 1.0], [float(ii.min), 1.0], [float(ii.min) - 10.0, 1.0],
                          [7.0, 1.0], [7.0, 0.0], [float(ii.max), 0.0]])
        hi = prog(["res", np.dtype(dtype).name, repr(float(ii.max)), "9"], pairs, dtype)
        assert [int(v) for v in hi] == [ii.max - 1, ii.max - 1, ii.min, ii.min, 7, 9, 9]
        lo = prog(["res", np.dtype(dtype).name, repr(float(ii.min)), "9"], pairs, dtype)
        assert [int(v) for v in lo] == [ii.max, ii.max, ii.min + 1, ii.min + 1, 7, 9, 9]
        mid = prog(["res", np.dtype(dtype).name, "7", repr(float(ii.min))], pairs, dtype)
        assert [int(v) for v in mid] == [ii.max, ii.max, ii.min, ii.min, 8, ii.min, ii.min]
    # floats are not nudged, and NaN may fill them
    pairs = np.array([[5.0, 1.0], [5.0, 0.0]])
    assert prog(["res", "float32", "5", "nan"], pairs, np.float32).tolist()[0] == 5.0
    assert np.isnan(prog(["res", "float64", "5", "nan"], pairs, np.float64)[1])
    assert prog(["res", "int16", "5", "nan"], pairs, i16, ok=False) == 5     # NaN cannot fill integers
    assert prog(["res", "float32", "5", "inf"], pairs, np.float32, ok=False) == 5
    assert prog(["avg", "uint8", 4, "256"], np.zeros((1, 4), u8), u8, ok=False) == 5
    assert prog(["avg", "uint8", 4, "0.5"], np.zeros((1, 4), u8), u8, ok=False) == 5
    assert prog(["avg", "int16", 4, "nan"], np.zeros((1, 4), i16), i16, ok=False) == 5


def _same_floats(a, b):
    """equal bit for bit (the sign of zero included) where neither is NaN, NaN in the same places"""
    assert a.dtype == b.dtype
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    assert np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def _float_blocks(dtype, n):
    fi = np.finfo(dtype)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, fi.max, -fi.max, fi.smallest_subnormal, 1.0 + fi.eps, 3.0]
    rng = np.random.default_rng(62)
    rnd = (rng.standard_normal((20000, n)) * 10.0 ** rng.integers(-6, 7, size=(20000, n))).astype(dtype)
    rnd[rng.random(rnd.shape) < 0.3] = 3.0
    return np.concatenate([np.array(list(itertools.product(special, repeat=n)), dtype=dtype), rnd])


@pytest.mark.parametrize("dtype", FLOAT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_float_masked_forms_equal_numpy(prog, dtype):
    """every block of special values and 20000 random ones per nodata value (3.0 is sprinkled over the random blocks),
    against the restatement and, for m = n, against the unmasked expressions"""
    dt = np.dtype(dtype)
    with np.errstate(all="ignore"):
        for n in (4, 2, 1):
            b = _float_blocks(dtype, n)
            for nd in (3.0, 0.0, float("nan"), float("inf"), float("-inf"), float(np.finfo(dtype).max)):
                got = _avg(prog, b, nd)
                # (C, H, W) with one block per column pair: n = 4 -> 2 x 2, n = 2 -> 1 x 2, n = 1 -> 1 x 1
                ras = b.reshape(-1, 2, 2).transpose(1, 0, 2).reshape(1, 2, -1) if n == 4 else b.reshape(1, 1, -1)
                if n == 1:  # single pixels: blocks of one column each need an odd width of 1 per block
                    want = np.where(N.nodata_mask(b[:, 0], nd), dt.type(nd), b[:, 0])
                else:
                    want = N.np_downsample2_nodata(ras, "average", nd)[0, 0]
                _same_floats(got, want.astype(dt))
                full = ~N.nodata_mask(b, nd).any(axis=1)
                plain = ((b[:, 0] + b[:, 1]) + (b[:, 2] + b[:, 3])) * dt.type(0.25) if n == 4 else \
                    (b[:, 0] + b[:, 1]) * dt.type(0.5) if n == 2 else b[:, 0]
                _same_floats(got[full], plain[full])
    # -0.0 is nodata 0.0 and the other way round; an all-nodata block gives (T)nd, +0.0 for nodata 0.0
    z = _avg(prog, np.array([[-0.0, 0.0, 2.0, 4.0], [-0.0, -0.0, 0.0, 0.0]], dt), 0.0)
    assert z[0] == 3.0 and z[1] == 0.0 and not np.signbit(z[1])
    z = _avg(prog, np.array([[-0.0, 0.0, 2.0, 4.0]], dt), -0.0)
    assert z[0] == 3.0
    assert _avg(prog, np.array([[1.0, 2.0, 4.0, np.nan]], dt), float("nan"))[0] == dt.type(7.0) / dt.type(3.0)


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_all_valid_integer_blocks_equal_the_unmasked_average(prog, dtype):
    """m = n: floor((2s + n) / (2n)), the unmasked rule, wherever that does not land on nodata"""
    rng = np.random.default_rng(63)
    ii = np.iinfo(dtype)
    for n in (4, 2, 1):
        blocks = rng.integers(ii.min, ii.max, size=(20000, n), dtype=dtype, endpoint=True)
        nd = 5
        blocks[blocks == nd] = 6
        got = _avg(prog, blocks, nd).astype(object)
        s = blocks.astype(object).sum(axis=1)
        plain = (2 * s + n) // (2 * n)
        assert np.array_equal(got, np.where(plain == nd, nd + 1, plain))


def test_masked_bilinear_accumulation(prog):
    rng = np.random.default_rng(64)
    n = 40000
    taps = rng.standard_normal((n, 4)) * 10.0 ** rng.integers(-3, 4, size=(n, 4))
    ok = rng.random((n, 4)) < 0.6
    ok[:2000] = True                                   # the all-valid fast form
    t = rng.random((n, 2))
    t[2000:4000] = rng.integers(0, 2, size=(2000, 2))  # weights of exactly 0 and 1 ...
    ok[2000:3000] = False
    ok[2000:3000, 0] = True                            # ... with one valid tap, often of weight 0: den = 0
    taps[4000:4100, 1] = np.inf
    rec = np.concatenate([taps, ok.astype(np.float64), t], axis=1)
    got = prog(["bil"], rec, np.float64).reshape(n, 2)
    val, wok = N.bilinear_value(taps[:, 0], taps[:, 1], taps[:, 2], taps[:, 3], ok[:, 0], ok[:, 1], ok[:, 2], ok[:, 3],
                                t[:, 0], t[:, 1])
    assert np.array_equal(got[:, 1] != 0, wok)
    assert wok[:2000].all() and (~wok[2000:3000]).sum() > 100 and wok[2000:3000].sum() > 100
    _same_floats(got[wok, 0], val[wok])
    with np.errstate(all="ignore"):
        a, b, c, d = taps[:2000].T
        tx, ty = t[:2000].T
        _same_floats(got[:2000, 0], (a * (1.0 - tx) + b * tx) * (1.0 - ty) + (c * (1.0 - tx) + d * tx) * ty)


def test_masked_average_accumulation(prog):
    rng = np.random.default_rng(65)
    n, ny, nx = 20000, 3, 4
    wy, wx = rng.random((n, ny)) + 1e-3, rng.random((n, nx)) + 1e-3
    v = rng.standard_normal((n, ny, nx)) * 10.0 ** rng.integers(-3, 4, size=(n, ny, nx))
    ok = rng.random((n, ny, nx)) < 0.7
    ok[:3000] = True     # no tap nodata: the unmasked form
    ok[3000:4000] = False  # all taps nodata: no valid weight
    lim = np.stack([np.zeros(n), wx.sum(axis=1), np.zeros(n), wy.sum(axis=1)], axis=1)  # chi - clo = the weights' sum
    rec = np.concatenate([wy, wx, v.reshape(n, -1), ok.reshape(n, -1).astype(np.float64), lim], axis=1)
    got = prog(["area", ny, nx], rec, np.float64).reshape(n, 2)
    val, wok = N.area_value(v, ok, wx, wy, (lim[:, 1] - lim[:, 0]) * (lim[:, 3] - lim[:, 2]))
    assert np.array_equal(got[:, 1] != 0, wok) and wok[:3000].all() and not wok[3000:4000].any()
    _same_floats(got[wok, 0], val[wok])


def test_header_includes_nothing_from_hip():
    text = HEADER.read_text()
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', text) == ["stdint.h", "frs_resample.h", "frs_window_map.h"]
    assert "#include <hip" not in text and "__HIP" not in text and "asm" not in text


# ------------------------------------------------------------------------------------------------ host python
def test_nodata_for_dtype():
    f = streaming.nodata_for_dtype
    assert f(-9999, np.int16) == -9999 and isinstance(f(-9999.0, np.int16), int)
    assert f(0, np.uint8) == 0 and f(255.0, np.uint8) == 255 and f(-32768, np.int16) == -32768
    assert f(2 ** 32 - 1, np.uint32) == 2 ** 32 - 1 and f(-2 ** 31, np.int32) == -2 ** 31
    assert f(-9999, np.float32) == -9999.0 and isinstance(f(-9999, np.float32), float)
    assert f(0.1, np.float32) == float(np.float32(0.1)) and f(0.1, np.float64) == 0.1
    assert np.isnan(f(float("nan"), np.float32)) and f(float("-inf"), np.float64) == float("-inf")
    assert f(1e300, np.float32) == float("inf")
    for bad, dt in ((256, np.uint8), (-1, np.uint8), (0.5, np.int16), (32768, np.int16), (-32769, np.int16),
                    (2 ** 32, np.uint32), (float("nan"), np.int32), (float("inf"), np.uint16), (-1e300, np.int32)):
        with pytest.raises(ValueError):
            f(bad, dt)


def test_tile_header_builder_emits_the_tag():
    tt = geotiff.Affine(0.001, 0.0, -106.0, 0.0, -0.001, 41.0)
    for nd, text in ((None, "None"), (-9999, "-9999.0"), (0, "0.0"), (float("nan"), "nan"), (2.5, "2.5")):
        hb = streaming.TileHeaderBuilder("EPSG:4326", np.int16 if nd != 2.5 else np.float32, 16, nodata=nd)
        hdr = hb.header(tt, 64, 48, 1.0, 9.0, 1234)
        meta = container.parse_metadata(hdr + b"\xff" * 16)
        assert meta.tag("GEOSPATIAL_NODATA") == text
        # byte-identical to the direct path with the same value
        tags = streaming.tile_tags("EPSG:4326", tt, 64, 48, np.int16 if nd != 2.5 else np.float32, 1.0, 9.0, nodata=nd)
        assert dict(tags)["GEOSPATIAL_NODATA"] == text
        back = container.read_raster_tags(meta)["nodata"]
        assert back is None if nd is None else (np.isnan(back) if nd != nd else back == float(nd))
    plain = streaming.TileHeaderBuilder("EPSG:4326", np.int16, 16).header(tt, 64, 48, 1.0, 9.0, 1234)
    assert plain == streaming.TileHeaderBuilder("EPSG:4326", np.int16, 16, nodata=None).header(tt, 64, 48, 1.0, 9.0, 1234)


def test_level_index_passes_the_key_through_and_reads_pick_it_up():
    tr = [0.001, 0.0, -106.0, 0.0, -0.001, 41.0]
    fr = {"frame_id": 0, "bbox": [0, 0, 1, 1], "window": {"col_off": 0, "row_off": 0, "width": 1, "height": 1},
          "byte_offset": 0, "byte_size": 0}
    levels = [{"level": k, "factor": 2 ** k, "width": w, "height": h, "transform": streaming.level_transform(tr, k),
               "frames": [fr]} for k, (h, w) in enumerate(streaming.overview_shapes(250, 300, 64), start=1)]
    index = {"crs": "EPSG:4326", "transform": tr, "width": 300, "height": 250, "tile_size": 64, "frames": [fr],
             "nodata": -9999, "overviews": {"resampling": "average", "levels": levels, "nodata_aware": True}}
    for k in streaming.overview_levels(index):
        assert streaming.level_index(index, k)["nodata"] == -9999
    plain = {k: v for k, v in index.items() if k != "nodata"}
    assert "nodata" not in streaming.level_index(plain, 2)
    assert list(streaming.level_index(plain, 2)) == ["crs", "transform", "width", "height", "tile_size", "frames"]
    assert streaming.index_nodata(index) == -9999.0 and streaming.index_nodata(plain) is None
    assert np.isnan(streaming.index_nodata(dict(index, nodata="nan")))
    assert streaming.index_nodata(dict(index, nodata="-inf")) == float("-inf")
    f = streaming.nodata_in_force
    assert f(index) == -9999.0 and f(index, None) is None and f(index, "none") is None and f(index, 7) == 7.0
    assert f(plain) is None and f(plain, -1) == -1.0
    with pytest.raises(ValueError):
        f(index, "source")
    # NaN goes into the index as a JSON string, and comes back
    js = container.index_json(dict(plain, nodata=streaming._nodata_to_index(float("nan"))))
    assert b'"nodata":"nan"' in js
    assert streaming._nodata_to_index(-9999) == -9999 and streaming._nodata_to_index(2.5) == 2.5


def test_new_entry_points_are_declared_and_bound():
    import ctypes
    names = {"frs_downsample2_nodata_device", "frs_downsample2_nodata", "frs_resample_window_nodata_device",
             "frs_resample_window_nodata"}
    assert names <= set(_native.EXPORTS)
    L = _native.load_library()
    rdp, vp, i32 = ctypes.POINTER(_native.RasterDesc), ctypes.c_void_p, ctypes.c_int32
    for name in ("frs_downsample2_nodata_device", "frs_downsample2_nodata"):
        assert getattr(L, name).argtypes == [vp, rdp, vp, rdp, vp, i32, ctypes.c_double]
    for name in ("frs_resample_window_nodata_device", "frs_resample_window_nodata"):
        assert getattr(L, name).argtypes == [vp, rdp, vp, rdp, vp, ctypes.POINTER(_native.WindowMap), i32,
                                             ctypes.c_double]


def test_geotiff_nodata_tag_round_trip(tmp_path):
    a = np.arange(12, dtype=np.float32).reshape(1, 3, 4)
    for nd in (-9999, 2.5, float("nan"), float("-inf"), None):
        p = tmp_path / "t.tif"
        geotiff.write(p, a, nodata=nd)
        back = geotiff.read(p).nodata
        assert back is None if nd is None else (np.isnan(back) if nd != nd else back == float(nd))


# ------------------------------------------------------------------------------------------------ CLI rejections
def test_create_streaming_nodata_rejections(tmp_path):
    missing = str(tmp_path / "missing.tif")
    for extra in (["--gpus", "2"], ["--distributed"]):
        r = runner.invoke(app, ["create-streaming", missing, "--nodata", "-9999"] + extra)
        assert r.exit_code == 1 and "--nodata runs on one GPU" in r.output and "does not exist" not in r.output
    r = runner.invoke(app, ["create-streaming", missing, "--nodata", "blue"])
    assert r.exit_code == 1 and "--nodata must be a number or 'source'" in r.output and "does not exist" not in r.output
    r = runner.invoke(app, ["create-streaming", missing, "--nodata", "none"])
    assert r.exit_code == 1 and "--nodata must be a number or 'source'" in r.output
    # alone, the option reaches the input check
    for v in ("-9999", "source", "nan", "0.5"):
        r = runner.invoke(app, ["create-streaming", missing, "--nodata", v])
        assert r.exit_code == 1 and "does not exist" in r.output, v


def test_extract_streaming_nodata_rejections(tmp_path):
    f, out = str(tmp_path / "missing.flac"), str(tmp_path / "o.tif")
    for v in ("blue", "source"):
        r = runner.invoke(app, ["extract-streaming", f, "--all", "-o", out, "--nodata", v])
        assert r.exit_code == 1 and "--nodata must be a number or 'none'" in r.output
    assert not Path(out).exists()
