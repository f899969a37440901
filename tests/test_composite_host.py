"""Host side of the three-band composite: csrc/frs_composite.h -- the lane function composite_group -- built by the host
compiler into a stand-alone program with its own main and compared bit for bit with tests/composite_ref.py
(tests/render_ref.py applied per plane, plus the any-plane-missing rule).  composite_group is run lane by lane over the
shapes of tests/render_cases.py, into a buffer of exactly the destination's extent pre-filled with a marker byte; the same
program is also built with the address and undefined-behaviour sanitizers when the host compiler accepts them.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import composite_ref as CR
from tests import window_ref as R
from tests.render_cases import LUT_SIZES, PAD, RECTS, SIZES, SRC_H, SRC_W, lut_of, nodata_of

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "flac_raster_amd" / "csrc"
HEADER = CSRC / "frs_composite.h"

# composite_host DTYPE MODE ND SRC_H SRC_W SRS SBS SRC LUT MANIFEST OUT
#     SRC holds 2 * SBS + (SRC_H - 1) * SRS + SRC_W elements (three planes SBS apart), LUT 4096 packed entries, ND is
#     "none" or the nodata value.  Each MANIFEST line "n lo0 lo1 lo2 hi0 hi1 hi2 nodata_rgba x0 y0 width height h w drs
#     lead gx gy" is one composite into a buffer of exactly lead + (h - 1) * drs + w * 4 bytes filled with 0xa5, its
#     origin `lead` bytes in; OUT gets the buffers, one after the other.
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "%s"

using namespace frs;

template <typename T> static std::vector<T> read_all(const char *path) {
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

template <int MODE, typename T, typename Mask>
static int group_mask(char **a, const Mask &mask) {
    const int64_t sh = atoll(a[3]), sw = atoll(a[4]), srs = atoll(a[5]), sbs = atoll(a[6]);
    const std::vector<T> file = read_all<T>(a[7]);
    if ((int64_t)file.size() != 2 * sbs + (sh - 1) * srs + sw) return 5;
    T *src = (T *)malloc(file.size() * sizeof(T));  // exactly the three planes' extent
    memcpy(src, file.data(), file.size() * sizeof(T));
    const std::vector<uint32_t> lut = read_all<uint32_t>(a[8]);
    FILE *m = fopen(a[9], "r"), *out = fopen(a[10], "wb");
    if (!m || !out) return 6;
    int n;
    unsigned rgba;
    char lo[3][64], hi[3][64], x0[64], y0[64], wd[64], ht[64];
    long long h, w, drs, lead, gx, gy;
    while (fscanf(m, "%%d %%63s %%63s %%63s %%63s %%63s %%63s %%u %%63s %%63s %%63s %%63s %%lld %%lld %%lld %%lld %%lld %%lld",
                  &n, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], &rgba, x0, y0, wd, ht, &h, &w, &drs, &lead, &gx,
                  &gy) == 18) {
        WinParams P;
        P.src_h = sh, P.src_w = sw, P.dst_h = h, P.dst_w = w;
        P.src_row_stride = srs, P.src_band_stride = sbs, P.dst_row_stride = drs, P.dst_band_stride = 0;
        P.x0 = strtod(x0, nullptr), P.y0 = strtod(y0, nullptr), P.width = strtod(wd, nullptr);
        P.height = strtod(ht, nullptr), P.fill = 0.0;
        uint32_t *table = (uint32_t *)malloc((size_t)n * 4);  // exactly n entries
        memcpy(table, lut.data(), (size_t)n * 4);
        CompParams R;
        for (int c = 0; c < 3; c++) R.range[c] = hist_range(strtod(lo[c], nullptr), strtod(hi[c], nullptr), n);
        R.lut = table, R.nodata_rgba = rgba;
        const size_t bytes = (size_t)(lead + (h - 1) * drs + w * 4);
        uint8_t *buf = (uint8_t *)malloc(bytes);  // 16-byte aligned: the origin is `lead` bytes past a boundary
        memset(buf, 0xa5, bytes);
        for (long long by = 0; by < gy; by++)
            for (long long bx = 0; bx < gx; bx++)
                for (uint32_t tid = 0; tid < (uint32_t)kRenderBlock; tid++)
                    composite_group<MODE, T>(src, buf + lead, P, R, mask, bx, gx, by, gy, tid);
        fwrite(buf, 1, bytes, out);
        free(buf);
        free(table);
    }
    fclose(m);
    fclose(out);
    free(src);
    return 0;
}

template <int MODE, typename T> static int group_mode(char **a) {
    if (!strcmp(a[2], "none")) return group_mask<MODE, T>(a, NoNodata{});
    return group_mask<MODE, T>(a, Nodata<T>{nd_cast<T>(strtod(a[2], nullptr))});
}

template <typename T> static int run(char **a) {
    if (!strcmp(a[1], "nearest")) return group_mode<kWindowNearest, T>(a);
    if (!strcmp(a[1], "bilinear")) return group_mode<kWindowBilinear, T>(a);
    if (!strcmp(a[1], "average")) return group_mode<kWindowAverage, T>(a);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 12) return 1;
    char **a = argv + 1;
    if (!strcmp(a[0], "uint8")) return run<uint8_t>(a);
    if (!strcmp(a[0], "uint16")) return run<uint16_t>(a);
    if (!strcmp(a[0], "int16")) return run<int16_t>(a);
    if (!strcmp(a[0], "int32")) return run<int32_t>(a);
    if (!strcmp(a[0], "uint32")) return run<uint32_t>(a);
    if (!strcmp(a[0], "float32")) return run<float>(a);
    if (!strcmp(a[0], "float64")) return run<double>(a);
    return 1;
}
'''

FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("composite_host")
    (d / "composite_host.cpp").write_text(PROGRAM % HEADER)
    return d


@pytest.fixture(scope="module")
def program(workdir):
    exe = workdir / "composite_host"
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", str(exe), str(workdir / "composite_host.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def sanitized(workdir):
    """the same program under the address and undefined-behaviour sanitizers, or None when the host compiler does not
    accept them (no such build then: the plain program's comparison stands alone)"""
    probe = workdir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    ok = subprocess.run(["g++"] + SANITIZE + ["-o", str(workdir / "probe"), str(probe)], capture_output=True)
    if ok.returncode != 0 or subprocess.run([str(workdir / "probe")], capture_output=True).returncode != 0:
        return None
    exe = workdir / "composite_host_san"
    subprocess.run(["g++"] + SANITIZE + FLAGS + ["-o", str(exe), str(workdir / "composite_host.cpp")], check=True)
    return exe


def test_header_includes_nothing_from_hip():
    text = (CSRC / "frs_composite.h").read_text()
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', text) == ["stdint.h", "frs_render.h"]


def _grid(h, w):
    """the grid frs_composite.hip launches"""
    cpr = (w * 4 + 15) // 16 + 1
    return max(1, min(cpr // 256, 65535)), min(h, 32768)


def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", CR.DTYPES, ids=lambda d: np.dtype(d).name)
def test_composite_group_lane_by_lane_equals_the_restatement(program, sanitized, workdir, dtype, mode):
    """every plane-mask combination, destination size, rectangle and LUT length, the destination's origin at each of
    the 16 positions within a chunk, with the launch's grid and with a smaller one whose work-groups stride over rows
    and chunks; the whole buffer, marker bytes included"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(61)
    lut = lut_of(4096)
    lut.tofile(workdir / "lut.bin")
    lo3, hi3 = CR.channel_limits(dt)
    srs = SRC_W + PAD
    sbs = (SRC_H - 1) * srs + SRC_W + CR.BAND_PAD
    case = 0
    for masks in CR.PLANE_MASKS:
        for nd in ((None, nodata_of(dt)) if masks == CR.PLANE_MASKS[0] else (nodata_of(dt),)):
            planes = CR.make_planes(rng, dt, masks)
            src = np.full(2 * sbs + (SRC_H - 1) * srs + SRC_W, _sentinel(dt), dtype=dt)
            for c in range(3):
                np.lib.stride_tricks.as_strided(src[c * sbs:], shape=(SRC_H, SRC_W),
                                                strides=(srs * dt.itemsize, dt.itemsize))[...] = planes[c]
            src.tofile(workdir / "src.bin")
            lines, wants = [], []
            for k, (h, w) in enumerate(SIZES):
                rects = R.rects(SRC_W, SRC_H, w, h)
                for rname in RECTS:
                    for n in LUT_SIZES:
                        rgba = 0x80402010 + n
                        lead = CR.LEADS[case % 16]
                        case += 1
                        drs = w * 4 + PAD
                        gx, gy = _grid(h, w) if (k + n) % 2 else (1, min(h, 3))
                        lines.append(" ".join([str(n)] + [float(x).hex() for x in lo3 + hi3] + [str(rgba)]
                                              + [float(x).hex() for x in rects[rname]]
                                              + [str(x) for x in (h, w, drs, lead, gx, gy)]))
                        want = np.full(lead + (h - 1) * drs + w * 4, 0xA5, dtype=np.uint8)
                        view = np.lib.stride_tricks.as_strided(want[lead:], shape=(h, w * 4), strides=(drs, 1))
                        view[...] = CR.composite(planes, rects[rname], (h, w), mode, nd, lo3, hi3, lut[:n],
                                                 rgba).reshape(h, w * 4)
                        wants.append(want)
            (workdir / "manifest.txt").write_text("\n".join(lines) + "\n")
            want = np.concatenate(wants)
            for exe in (program, sanitized):
                if exe is None:
                    continue
                subprocess.run([str(exe), dt.name, mode, "none" if nd is None else float(nd).hex(), str(SRC_H),
                                str(SRC_W), str(srs), str(sbs), str(workdir / "src.bin"), str(workdir / "lut.bin"),
                                str(workdir / "manifest.txt"), str(workdir / "out.bin")], check=True)
                got = np.fromfile(workdir / "out.bin", dtype=np.uint8)
                assert got.shape == want.shape
                if not np.array_equal(got, want):
                    bad = int(np.flatnonzero(got != want)[0])
                    sizes = np.cumsum([len(x) for x in wants])
                    i = int(np.searchsorted(sizes, bad, side="right"))
                    raise AssertionError((masks, nd, lines[i], bad - (int(sizes[i - 1]) if i else 0)))
