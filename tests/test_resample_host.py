"""Host side of the overview pyramid: the arithmetic of csrc/frs_resample.h built with the host compiler into a small
program of its own, the pure index functions of streaming.py (overview_shapes, level_transform, level_index,
pick_level), the new ctypes surface against the header, and the CLI's argument rejections.  No GPU."""
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
from typer.testing import CliRunner

from flac_raster_amd import _native, streaming
from flac_raster_amd.cli import app

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_resample.h"
runner = CliRunner()

INT_DTYPES = [np.uint8, np.uint16, np.int16, np.int32, np.uint32]
FLOAT_DTYPES = [np.float32, np.float64]

# resample_host DTYPE N IN OUT: IN holds blocks of N elements (a, b[, c, d]); OUT gets one average per block
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "%s"

template <typename T> static int run(int n, const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) return 3;
    fclose(f);
    const size_t blocks = v.size() / (size_t)n;
    std::vector<T> o(blocks);
    for (size_t i = 0; i < blocks; i++) {
        const T *p = v.data() + i * (size_t)n;
        o[i] = n == 4 ? frs::resample_avg4(p[0], p[1], p[2], p[3]) : n == 2 ? frs::resample_avg2(p[0], p[1]) : p[0];
    }
    f = fopen(out, "wb");
    if (!f) return 4;
    fwrite(o.data(), sizeof(T), o.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 5) return 1;
    const int n = atoi(argv[2]);
    if (n != 1 && n != 2 && n != 4) return 1;
    const char *dt = argv[1];
    if (!strcmp(dt, "uint8")) return run<uint8_t>(n, argv[3], argv[4]);
    if (!strcmp(dt, "uint16")) return run<uint16_t>(n, argv[3], argv[4]);
    if (!strcmp(dt, "int16")) return run<int16_t>(n, argv[3], argv[4]);
    if (!strcmp(dt, "int32")) return run<int32_t>(n, argv[3], argv[4]);
    if (!strcmp(dt, "uint32")) return run<uint32_t>(n, argv[3], argv[4]);
    if (!strcmp(dt, "float32")) return run<float>(n, argv[3], argv[4]);
    if (!strcmp(dt, "float64")) return run<double>(n, argv[3], argv[4]);
    return 1;
}
'''


@pytest.fixture(scope="module")
def resample(tmp_path_factory):
    """blocks (N x n array of a dtype) -> the program's N averages"""
    d = tmp_path_factory.mktemp("resample_host")
    src = d / "resample_host.cpp"
    src.write_text(PROGRAM % HEADER)
    exe = d / "resample_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe), str(src)],
                   check=True)

    def run(blocks: np.ndarray) -> np.ndarray:
        blocks = np.ascontiguousarray(blocks)
        fin, fout = d / "in.bin", d / "out.bin"
        blocks.tofile(fin)
        subprocess.run([str(exe), blocks.dtype.name, str(blocks.shape[1]), str(fin), str(fout)], check=True)
        out = np.fromfile(fout, dtype=blocks.dtype)
        assert out.shape == (blocks.shape[0],)
        return out
    return run


def edge_values(dtype):
    """min, min+1, -2, -1, 0, 1, 2, max-1, max: those the dtype holds, once each"""
    ii = np.iinfo(dtype)
    vals = [ii.min, ii.min + 1, -2, -1, 0, 1, 2, ii.max - 1, ii.max]
    return sorted({v for v in vals if ii.min <= v <= ii.max})


def exact_average(blocks: np.ndarray) -> list:
    """floor((2s + n) / (2n)) in Python integers"""
    n = blocks.shape[1]
    return [(2 * s + n) // (2 * n) for s in (sum(int(v) for v in row) for row in blocks)]


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", [1, 2, 4])
def test_integer_average_every_block_of_edge_values(resample, dtype, n):
    blocks = np.array(list(itertools.product(edge_values(dtype), repeat=n)), dtype=dtype)
    assert len(blocks) == len(edge_values(dtype)) ** n
    got = resample(blocks)
    assert [int(v) for v in got] == exact_average(blocks)


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_integer_average_random_blocks(resample, dtype):
    rng = np.random.default_rng(11)
    ii = np.iinfo(dtype)
    for n in (4, 2):
        blocks = rng.integers(ii.min, ii.max, size=(100000, n), dtype=dtype, endpoint=True)
        got = resample(blocks).astype(object)
        s = blocks.astype(object).sum(axis=1)
        assert np.array_equal(got, (2 * s + n) // (2 * n))


def test_integer_average_examples_of_the_definition(resample):
    i16, i32, u32 = np.int16, np.int32, np.uint32
    assert resample(np.array([[-1, -1, -1, -2]], i16))[0] == -1
    assert resample(np.array([[-1, -2]], i16))[0] == -1
    assert resample(np.array([[-3, -2]], i16))[0] == -2
    assert resample(np.array([[1, 2]], i16))[0] == 2           # half towards +infinity
    assert resample(np.array([[1, 1, 1, 2]], i16))[0] == 1      # 1.25
    assert resample(np.array([[1, 1, 2, 2]], i16))[0] == 2      # 1.5
    lo, hi = np.iinfo(i32).min, np.iinfo(np.uint32).max
    assert resample(np.array([[lo] * 4], i32))[0] == lo
    assert resample(np.array([[hi] * 4], u32))[0] == hi
    assert resample(np.array([[hi, hi - 1]], u32))[0] == hi


def _float_blocks(dtype, n):
    fi = np.finfo(dtype)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, fi.max, -fi.max, fi.tiny, fi.smallest_subnormal, 1.0 + fi.eps,
               3.0, 1e-3]
    rng = np.random.default_rng(5)
    # a third random blocks of mixed magnitude, so that the order of the additions shows
    rnd = (rng.standard_normal((20000, n)) * 10.0 ** rng.integers(-6, 7, size=(20000, n))).astype(dtype)
    prod = np.array(list(itertools.product(special, repeat=n)), dtype=dtype)
    return np.concatenate([prod, rnd])


def _same_floats(a, b):
    """equal bit for bit (the sign of zero included) where neither is NaN, NaN in the same places"""
    assert a.dtype == b.dtype
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    assert np.array_equal(a.view(u)[~na], b.view(u)[~nb])


@pytest.mark.parametrize("dtype", FLOAT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_float_forms_equal_the_expression_in_numpy(resample, dtype):
    with np.errstate(all="ignore"):
        b4 = _float_blocks(dtype, 4)
        a, b, c, d = (b4[:, i] for i in range(4))
        want4 = ((a + b) + (c + d)) * dtype(0.25)
        assert want4.dtype == dtype
        _same_floats(resample(b4), want4)
        b2 = _float_blocks(dtype, 2)
        _same_floats(resample(b2), (b2[:, 0] + b2[:, 1]) * dtype(0.5))
        b1 = _float_blocks(dtype, 1)
        got1 = resample(b1)
        u = np.uint32 if dtype == np.float32 else np.uint64
        assert np.array_equal(got1.view(u), b1[:, 0].view(u))  # n = 1 moves the bits, NaN included


def test_header_includes_nothing_from_hip():
    text = HEADER.read_text()
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', text) == ["stdint.h"]


# ------------------------------------------------------------------------------------------------ index functions
def test_overview_shapes():
    f = streaming.overview_shapes
    assert f(1, 1, 64) == []
    assert f(64, 64, 64) == []           # tile-sized: already one tile
    assert f(65, 64, 64) == [(33, 32)]   # tile + 1
    assert f(64, 65, 64) == [(32, 33)]
    assert f(250, 300, 64) == [(125, 150), (63, 75), (32, 38)]
    lv = f(40000, 40000, 512)
    assert len(lv) == 7 and lv[0] == (20000, 20000) and lv[-1] == (313, 313) and lv[-2] == (625, 625)
    assert f(250, 300, 64, max_levels=2) == [(125, 150), (63, 75)]
    assert f(250, 300, 64, max_levels=0) == []
    assert f(250, 300, 64, max_levels=9) == f(250, 300, 64)
    assert f(1, 1000, 64) == [(1, 500), (1, 250), (1, 125), (1, 63)]
    with pytest.raises(ValueError):
        f(0, 5, 64)


def _index_with_levels():
    tr = [0.001, 0.0, -106.0, 0.0, -0.001, 41.0]
    fr = lambda i: {"frame_id": i, "bbox": [0, 0, 1, 1], "window": {"col_off": 0, "row_off": 0, "width": 1, "height": 1},
                    "byte_offset": 0, "byte_size": 0}  # noqa: E731
    levels = [{"level": k, "factor": 2 ** k, "width": w, "height": h, "transform": streaming.level_transform(tr, k),
               "frames": [fr(100 * k)]} for k, (h, w) in enumerate(streaming.overview_shapes(250, 300, 64), start=1)]
    return {"crs": "EPSG:4326", "transform": tr, "width": 300, "height": 250, "tile_size": 64, "frames": [fr(0)],
            "overviews": {"resampling": "average", "levels": levels}}


def test_level_transform_scales_the_pixel_and_keeps_the_origin():
    tr = [0.001, 0.25, -106.0, -0.5, -0.001, 41.0]
    assert streaming.level_transform(tr, 0) == tr
    assert streaming.level_transform(tr, 3) == [0.001 * 8.0, 2.0, -106.0, -4.0, -0.001 * 8.0, 41.0]
    assert streaming.level_transform(tr + [0.0, 0.0, 1.0], 1) == [0.002, 0.5, -106.0, -1.0, -0.002, 41.0]


def test_level_index_and_its_errors():
    index = _index_with_levels()
    assert streaming.level_index(index, 0) is index
    assert streaming.overview_levels(index) == [0, 1, 2, 3]
    li = streaming.level_index(index, 2)
    assert list(li) == ["crs", "transform", "width", "height", "tile_size", "frames"]
    assert (li["height"], li["width"], li["tile_size"], li["crs"]) == (63, 75, 64, "EPSG:4326")
    assert li["transform"] == [0.004, 0.0, -106.0, 0.0, -0.004, 41.0]
    assert li["frames"] is index["overviews"]["levels"][1]["frames"]
    assert streaming.select_frame(li, last=True)["frame_id"] == 200
    with pytest.raises(LookupError, match=r"level 4 .*\[0, 1, 2, 3\]"):
        streaming.level_index(index, 4)
    plain = {k: v for k, v in index.items() if k != "overviews"}
    assert streaming.level_index(plain, 0) is plain and streaming.overview_levels(plain) == [0]
    with pytest.raises(LookupError, match=r"level 1 .*\[0\]"):
        streaming.level_index(plain, 1)


def test_pick_level():
    index = _index_with_levels()  # 250 x 300: levels 150, 75, 38 wide
    pick = streaming.pick_level
    assert pick(index, 300, 250, 300) == 0
    assert pick(index, 300, 250, 299) == 1
    assert pick(index, 300, 250, 150) == 1
    assert pick(index, 300, 250, 149) == 2
    assert pick(index, 300, 250, 80) == 2
    assert pick(index, 300, 250, 38) == 3
    assert pick(index, 300, 250, 37) == 3    # none qualifies: the coarsest
    assert pick(index, 250, 300, 80) == 2    # the longer side, whichever it is
    assert pick(index, 33, 17, 16) == 2      # a window: ceil(33 / 4) = 9 <= 16 < ceil(33 / 2)
    plain = {k: v for k, v in index.items() if k != "overviews"}
    assert pick(plain, 300, 250, 10) == 0
    with pytest.raises(ValueError):
        pick(index, 300, 250, 0)


# ------------------------------------------------------------------------------------------------ ABI surface
def test_resample_enum_and_prototypes_match_the_header(tmp_path):
    """enum frs_resample's values and the two prototypes, from a C program that includes the header."""
    hdr = ROOT / "include" / "flac_raster_amd.h"
    # the prototypes: assigning to a pointer of the expected type compiles without a warning only if they agree
    proto = "int (*)(frs_ctx *, const frs_raster_desc *, const void *, const frs_raster_desc *, void *, int32_t)"
    c = tmp_path / "t.c"
    c.write_text(f'#include "{hdr}"\n' + "".join(
        f"{proto.replace('(*)', f'(*p{i})')} = {name};\n"
        for i, name in enumerate(("frs_downsample2_device", "frs_downsample2"))))
    subprocess.run(["gcc", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(c)], check=True)
    # the enum's values and the descriptor's size, printed by a program that includes the header
    exe = tmp_path / "v"
    (tmp_path / "v.c").write_text(f'#include "{hdr}"\n#include <stdio.h>\nint main(void){{printf("%d %d %zu\\n", '
                                  '(int)FRS_RESAMPLE_NEAREST, (int)FRS_RESAMPLE_AVERAGE, sizeof(frs_raster_desc));'
                                  'return 0;}\n')
    subprocess.run(["gcc", "-o", str(exe), str(tmp_path / "v.c")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    import ctypes
    assert [int(x) for x in out] == [_native.RESAMPLE_NEAREST, _native.RESAMPLE_AVERAGE,
                                     ctypes.sizeof(_native.RasterDesc)]
    assert _native.RESAMPLE_CODES == {"nearest": _native.RESAMPLE_NEAREST, "average": _native.RESAMPLE_AVERAGE}
    assert {"frs_downsample2_device", "frs_downsample2"} <= set(_native.EXPORTS)
    assert streaming.RESAMPLING == ("average", "nearest")


def test_library_exports_the_downsample_entry_points():
    L = _native.load_library()
    import ctypes
    rdp, vp = ctypes.POINTER(_native.RasterDesc), ctypes.c_void_p
    for name in ("frs_downsample2_device", "frs_downsample2"):
        fn = getattr(L, name)
        assert fn.argtypes == [vp, rdp, vp, rdp, vp, ctypes.c_int32] and fn.restype is ctypes.c_int32


# ------------------------------------------------------------------------------------------------ CLI rejections
def test_create_streaming_overviews_rejects_multi_gpu_before_the_input_is_opened(tmp_path):
    missing = str(tmp_path / "missing.tif")
    for extra in (["--gpus", "2"], ["--distributed"]):
        r = runner.invoke(app, ["create-streaming", missing, "--overviews"] + extra)
        assert r.exit_code == 1 and "--overviews runs on one GPU" in r.output and "does not exist" not in r.output
    r = runner.invoke(app, ["create-streaming", missing, "--overviews", "--resampling", "cubic"])
    assert r.exit_code == 1 and "--resampling must be one of" in r.output and "does not exist" not in r.output
    for opts in (["--resampling", "nearest"], ["--overview-levels", "2"]):
        r = runner.invoke(app, ["create-streaming", missing] + opts)
        assert r.exit_code == 1 and "need --overviews" in r.output and "does not exist" not in r.output
    # alone, the options reach the input check
    for opts in (["--overviews"], ["--overviews", "--resampling", "nearest", "--overview-levels", "2"]):
        r = runner.invoke(app, ["create-streaming", missing] + opts)
        assert r.exit_code == 1 and "does not exist" in r.output


def test_extract_streaming_level_options_rejected_before_anything_is_read(tmp_path):
    f, out = str(tmp_path / "missing.flac"), str(tmp_path / "o.tif")
    r = runner.invoke(app, ["extract-streaming", f, "--all", "-o", out, "--level", "1", "--max-size", "80"])
    assert r.exit_code == 1 and "--level and --max-size exclude each other" in r.output
    for sel in (["--tile-id", "0"], ["--center"], ["--last"], ["--bbox", "0,0,1,1"]):
        r = runner.invoke(app, ["extract-streaming", f, "-o", out, "--max-size", "80"] + sel)
        assert r.exit_code == 1 and "--max-size works with --all or --bbox --mosaic only" in r.output, sel
    assert not Path(out).exists()
