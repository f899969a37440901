"""Host side of the hillshaded render: csrc/frs_shade.h -- shade_level and the two lane functions shade_fill and
shade_emit -- built by the host compiler into a stand-alone program with its own main, and compared bit for bit with
the numpy restatement in tests/shade_ref.py.  The lane functions run as a work-group does: every lane's fill, then
every lane's emit, a plain array standing in for LDS, over every work-group of a grid, into a buffer allocated to
exactly the destination's extent.  The same program is also built with the address and undefined-behaviour sanitizers
when the host compiler links them.  No GPU."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import shade_cases as SC
from tests import shade_ref as SR
from tests import window_ref as R
from tests.render_cases import PAD, SRC_H, SRC_W, limits, lut_of, nodata_of

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "flac_raster_amd" / "csrc"
HEADER = CSRC / "frs_shade.h"

# shade_host level IN OUT
#     IN holds records of 14 doubles (z[3][3] north to south, lx, ly, lz, kx, ky); OUT gets one int32 level per record
# shade_host group DTYPE MODE ND SRC_H SRC_W SRS SRC LUT TABLE KX KY MANIFEST OUT
#     as render_host's group (tests/test_render_host.py); TABLE holds the 256 shade multipliers, the light is LIGHT.
#     Each MANIFEST line "C n lo hi nodata_rgba x0 y0 width height h w drs lead gx gy" is one render by a gx x gy grid
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

static int level(char **a) {
    const std::vector<double> in = read_all<double>(a[1]);
    std::vector<int32_t> o(in.size() / 14);
    for (size_t i = 0; i < o.size(); i++) {
        const double *r = in.data() + i * 14;
        double z[3][3];
        for (int j = 0; j < 9; j++) z[j / 3][j %% 3] = r[j];
        ShadeParams S;
        S.lx = r[9], S.ly = r[10], S.lz = r[11], S.kx = r[12], S.ky = r[13], S.table = nullptr;
        o[i] = shade_level(z, S);
    }
    FILE *f = fopen(a[2], "wb");
    if (!f) return 4;
    fwrite(o.data(), 4, o.size(), f);
    fclose(f);
    return 0;
}

template <int MODE, typename T, typename Mask, int C>
static void run_grid(const T *src, uint8_t *dst, const WinParams &P, const RenderParams &R, const ShadeParams &S,
                     const Mask &mask, long long gx, long long gy) {
    double *tile = (double *)malloc(sizeof(double) * ShadeShape<C>::samples);  // exactly the LDS array
    const int64_t ntx = shade_tiles_x<C>(P), nty = shade_tiles_y(P);
    for (long long by = 0; by < gy; by++)
        for (long long bx = 0; bx < gx; bx++)
            for (int64_t ty = by; ty < nty; ty += gy)
                for (int64_t tx = bx; tx < ntx; tx += gx) {
                    const ShadeTile t = shade_tile<C>(dst, P, tx, ty);
                    for (uint32_t tid = 0; tid < (uint32_t)kShadeBlock; tid++)
                        shade_fill<MODE, T, Mask, C>(src, P, mask, t, tile, tid);
                    for (uint32_t tid = 0; tid < (uint32_t)kShadeBlock; tid++)
                        shade_emit<C>(dst, P, R, S, t, tile, tid);
                }
    free(tile);
}

template <int MODE, typename T, typename Mask>
static int group_mask(char **a, const Mask &mask) {
    const int64_t sh = atoll(a[4]), sw = atoll(a[5]), srs = atoll(a[6]);
    const std::vector<T> file = read_all<T>(a[7]);
    if ((int64_t)file.size() != (sh - 1) * srs + sw) return 5;
    T *src = (T *)malloc(file.size() * sizeof(T));  // exactly the source's extent
    memcpy(src, file.data(), file.size() * sizeof(T));
    const std::vector<uint32_t> lut = read_all<uint32_t>(a[8]);
    const std::vector<uint8_t> tab = read_all<uint8_t>(a[9]);
    if (tab.size() != 256) return 7;
    uint8_t *table = (uint8_t *)malloc(256);
    memcpy(table, tab.data(), 256);
    ShadeParams S;
    S.lx = %s, S.ly = %s, S.lz = %s;
    S.kx = strtod(a[10], nullptr), S.ky = strtod(a[11], nullptr), S.table = table;
    FILE *m = fopen(a[12], "r"), *out = fopen(a[13], "wb");
    if (!m || !out) return 6;
    int C, n;
    unsigned rgba;
    char lo[64], hi[64], x0[64], y0[64], wd[64], ht[64];
    long long h, w, drs, lead, gx, gy;
    while (fscanf(m, "%%d %%d %%63s %%63s %%u %%63s %%63s %%63s %%63s %%lld %%lld %%lld %%lld %%lld %%lld", &C, &n, lo, hi,
                  &rgba, x0, y0, wd, ht, &h, &w, &drs, &lead, &gx, &gy) == 15) {
        WinParams P;
        P.src_h = sh, P.src_w = sw, P.dst_h = h, P.dst_w = w;
        P.src_row_stride = srs, P.src_band_stride = 0, P.dst_row_stride = drs, P.dst_band_stride = 0;
        P.x0 = strtod(x0, nullptr), P.y0 = strtod(y0, nullptr), P.width = strtod(wd, nullptr);
        P.height = strtod(ht, nullptr), P.fill = 0.0;
        uint32_t *lutn = (uint32_t *)malloc((size_t)n * 4);  // exactly n entries
        memcpy(lutn, lut.data(), (size_t)n * 4);
        RenderParams R;
        R.range = hist_range(strtod(lo, nullptr), strtod(hi, nullptr), n);
        R.lut = lutn, R.nodata_rgba = rgba, R.channels = C;
        const size_t bytes = (size_t)(lead + (h - 1) * drs + w * C);
        uint8_t *buf = (uint8_t *)malloc(bytes);  // 16-byte aligned: the origin is `lead` bytes past a boundary
        memset(buf, 0xa5, bytes);
        if (C == 1) run_grid<MODE, T, Mask, 1>(src, buf + lead, P, R, S, mask, gx, gy);
        else if (C == 2) run_grid<MODE, T, Mask, 2>(src, buf + lead, P, R, S, mask, gx, gy);
        else run_grid<MODE, T, Mask, 4>(src, buf + lead, P, R, S, mask, gx, gy);
        fwrite(buf, 1, bytes, out);
        free(buf);
        free(lutn);
    }
    fclose(m);
    fclose(out);
    free(table);
    free(src);
    return 0;
}

template <int MODE, typename T> static int group_mode(char **a) {
    if (!strcmp(a[3], "none")) return group_mask<MODE, T>(a, NoNodata{});
    return group_mask<MODE, T>(a, Nodata<T>{nd_cast<T>(strtod(a[3], nullptr))});
}

template <typename T> static int run(int argc, char **a) {
    if (strcmp(a[0], "group") || argc != 14) return 1;
    if (!strcmp(a[2], "nearest")) return group_mode<kWindowNearest, T>(a);
    if (!strcmp(a[2], "bilinear")) return group_mode<kWindowBilinear, T>(a);
    if (!strcmp(a[2], "average")) return group_mode<kWindowAverage, T>(a);
    return 1;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "level")) return level(argv + 1);
    if (argc < 3) return 1;
    const char *dt = argv[2];
    argc -= 1, argv += 1;
    if (!strcmp(dt, "uint8")) return run<uint8_t>(argc, argv);
    if (!strcmp(dt, "uint16")) return run<uint16_t>(argc, argv);
    if (!strcmp(dt, "int16")) return run<int16_t>(argc, argv);
    if (!strcmp(dt, "int32")) return run<int32_t>(argc, argv);
    if (!strcmp(dt, "uint32")) return run<uint32_t>(argc, argv);
    if (!strcmp(dt, "float32")) return run<float>(argc, argv);
    if (!strcmp(dt, "float64")) return run<double>(argc, argv);
    return 1;
}
'''

FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_host")
    (d / "shade_host.cpp").write_text(PROGRAM % ((HEADER,) + tuple(float(v).hex() for v in SC.LIGHT)))
    return d


@pytest.fixture(scope="module")
def program(workdir):
    exe = workdir / "shade_host"
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", str(exe), str(workdir / "shade_host.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def sanitized(workdir):
    """the same program under the address and undefined-behaviour sanitizers, or None where a probe program does not
    link and run under them"""
    probe = workdir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    ok = subprocess.run(["g++"] + SANITIZE + ["-o", str(workdir / "probe"), str(probe)], capture_output=True)
    if ok.returncode != 0 or subprocess.run([str(workdir / "probe")], capture_output=True).returncode != 0:
        return None
    exe = workdir / "shade_host_san"
    subprocess.run(["g++"] + SANITIZE + FLAGS + ["-o", str(exe), str(workdir / "shade_host.cpp")], check=True)
    return exe


def test_header_includes_nothing_from_hip():
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', HEADER.read_text()) == ["stdint.h", "frs_render.h",
                                                                              "frs_window_row.h"]


# ------------------------------------------------------------------------------------------------ shade_level
def _levels(exe, d, z, light, kx, ky):
    z = np.asarray(z, dtype=np.float64).reshape(-1, 9)
    rec = np.empty((len(z), 14), dtype=np.float64)
    rec[:, :9] = z
    rec[:, 9:12] = light
    rec[:, 12], rec[:, 13] = kx, ky
    rec.tofile(d / "l_in.bin")
    subprocess.run([str(exe), "level", str(d / "l_in.bin"), str(d / "l_out.bin")], check=True)
    return np.fromfile(d / "l_out.bin", dtype=np.int32).astype(np.int64)


def _light(az, alt):
    a, h = math.radians(az), math.radians(alt)
    return (math.sin(a) * math.cos(h), math.cos(a) * math.cos(h), math.sin(h))


def _plane(a, b, cell=1.0):
    """z = a E + b N on the 3 x 3 grid (rows north to south)"""
    e = np.array([-1.0, 0.0, 1.0]) * cell
    return a * e[None, :] + b * (-e)[:, None]


def test_shade_level_equals_the_restatement(program, sanitized, workdir):
    light = _light(315, 45)
    zs = [np.zeros((3, 3)), np.full((3, 3), 1234.5)]
    for k in range(8):  # planes facing each of eight directions
        t = math.radians(45 * k)
        zs.append(_plane(math.sin(t), math.cos(t)))
    big = np.zeros((3, 3))
    big[0, 0], big[2, 2], big[0, 2], big[2, 0] = -2147483648.0, 2147483647.0, 2147483647.0, -2147483648.0
    zs.append(big)
    zs.append(big.T)
    for v in (np.inf, -np.inf):
        for pos in ((0, 0), (1, 2), (2, 1)):
            z = _plane(0.3, -0.2)
            z[pos] = v
            zs.append(z)
    z = _plane(0.3, -0.2)
    z[0, 1] = np.nan  # (the lane functions replace it; shade_level itself gives level 0)
    zs.append(z)
    rng = np.random.default_rng(5)
    zs += list(rng.standard_normal((2000, 3, 3)) * 3.0)
    zs += list(rng.integers(-32768, 32767, size=(2000, 3, 3)).astype(np.float64))
    zs = np.array(zs)
    for kx, ky in ((0.125, 0.125), (1.0 / 240.0, 1.0 / 250.0), (1e-5, 2e-5)):
        want = SR.level(zs, light, kx, ky)
        assert want[0] == want[1] == 181  # flat ground: floor(256 sin 45)
        for exe in (program, sanitized):
            if exe is not None:
                assert np.array_equal(_levels(exe, workdir, zs, light, kx, ky), want)
    inf_rows = np.isinf(zs).any(axis=(1, 2))
    assert (SR.level(zs, light, 0.125, 0.125)[inf_rows] == 0).all() and inf_rows.sum() == 6


def test_shade_level_where_the_product_lands_on_and_next_to_an_integer(program, workdir):
    """flat ground under a light whose lz is j / 256 and its two neighbours: s * 256 is j exactly, just below, just
    above; and a sweep of slopes along x through every level"""
    got, want = [], []
    for j in (1, 2, 100, 181, 255, 256):
        c = j / 256.0
        for lz in (np.nextafter(c, 0.0), c, np.nextafter(c, 2.0)):
            l = (0.0, 0.0, float(lz))
            got.append(int(_levels(program, workdir, np.zeros((3, 3)), l, 1.0, 1.0)[0]))
            want.append(int(SR.level(np.zeros((3, 3)), l, 1.0, 1.0)))
    assert got == want
    assert got[:3] == [0, 1, 1] and got[-3:] == [255, 255, 255] and got[9:12] == [180, 181, 181]
    # slopes: gx = 8 a, p = a, s = (lz - a lx) / sqrt(1 + a^2)
    light = _light(315, 45)
    a = np.linspace(-3.0, 1.2, 20001)
    zs = np.array([_plane(v, 0.0) for v in a])
    want = SR.level(zs, light, 0.125, 0.125)
    assert len(np.unique(want)) > 200
    assert np.array_equal(_levels(program, workdir, zs, light, 0.125, 0.125), want)


def test_planes_against_the_closed_form(program, workdir):
    """independent of the restatement: on z = a E + b N the level is within 1 of 256 n.L, n the unit normal
    (-a, -b, 1) / |.|, and the slope that faces the light is the brightest"""
    for az, alt in ((315, 45), (0, 30), (90, 60), (200, 10), (135, 90)):
        L = _light(az, alt)
        for cell in (1.0, 30.0):
            k8 = 1.0 / (8 * cell)
            for a, b in ((0, 0), (0.5, 0), (0, 0.5), (-0.5, 0.25), (1.5, -2.0), (-0.1, -0.1)):
                k = _levels(program, workdir, _plane(a, b, cell), L, k8, k8)[0]
                nl = (-a * L[0] - b * L[1] + L[2]) / math.sqrt(1 + a * a + b * b)
                assert abs(k - min(max(256 * nl, 0), 255)) <= 1, (az, alt, a, b, k, nl)
            if alt < 90:
                # slopes of the steepness whose normal can point at the light, turned through the compass: the one
                # that descends away from the light's azimuth (and so faces it) is the brightest
                tl = math.tan(math.radians(90 - alt))
                turns = list(range(0, 360, 15))
                zs = [_plane(-tl * math.sin(math.radians(t)), -tl * math.cos(math.radians(t)), cell) for t in turns]
                ks = _levels(program, workdir, np.array(zs), L, k8, k8)
                best = turns[int(np.argmax(ks))]
                assert ks.max() == 255 and abs((best - az + 180) % 360 - 180) <= 15, (az, alt, best)


# ------------------------------------------------------------------------------------------------ the lane functions
def _sentinel(dt):
    return np.frombuffer(b"\xa5" * 8, dtype=np.uint8).view(dt)[0]


def _grid(h, w, C):
    """the grid frs_shade.hip launches"""
    return (-(-((w * C + 15) // 16 + 1) // 16), -(-h // 16))


def _run_group(exe, d, dt, mode, masked, cases, tab, grid_of):
    a = SC.source(dt.name, masked)
    srs = SRC_W + PAD
    src = np.full((SRC_H - 1) * srs + SRC_W, _sentinel(dt), dtype=dt)
    np.lib.stride_tricks.as_strided(src, shape=(SRC_H, SRC_W), strides=(srs * dt.itemsize, dt.itemsize))[...] = a
    src.tofile(d / "src.bin")
    lut_of(4096).tofile(d / "lut.bin")
    tab.tofile(d / "table.bin")
    lo, hi = limits(dt)
    kx, ky = SC.scales(dt)
    lines = []
    for i, (C, n, rgba, rect, h, w, drs, lead, _) in enumerate(cases):
        gx, gy = grid_of(i, h, w, C)
        lines.append(" ".join([str(C), str(n), float(lo).hex(), float(hi).hex(), str(rgba)]
                              + [float(x).hex() for x in rect] + [str(x) for x in (h, w, drs, lead, gx, gy)]))
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    subprocess.run([str(exe), "group", dt.name, mode, float(nodata_of(dt)).hex() if masked else "none", str(SRC_H),
                    str(SRC_W), str(srs), str(d / "src.bin"), str(d / "lut.bin"), str(d / "table.bin"),
                    float(kx).hex(), float(ky).hex(), str(d / "manifest.txt"), str(d / "out.bin")], check=True)
    return np.fromfile(d / "out.bin", dtype=np.uint8), lines


def _compare(got, wants, lines, tag):
    want = np.concatenate(wants)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        sizes = np.cumsum([len(x) for x in wants])
        case = int(np.searchsorted(sizes, bad, side="right"))
        raise AssertionError((tag, lines[case], bad - (int(sizes[case - 1]) if case else 0)))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_fill_then_emit_over_every_work_group_equals_the_restatement(program, sanitized, workdir, dtype, mode):
    """every destination size around the tile, rectangle, channel count and LUT length, with and without nodata, by the
    launch's grid and by a smaller one whose work-groups stride over tiles; the whole buffer, sentinels included"""
    dt = np.dtype(dtype)
    for masked in (False, True):
        cases = SC.cases(dt.name, mode, masked)
        for exe in (program, sanitized):
            if exe is not None:
                got, lines = _run_group(exe, workdir, dt, mode, masked, cases, SC.table(),
                                        lambda i, h, w, C: _grid(h, w, C) if i % 2 else (1, 1))
                _compare(got, [c[-1] for c in cases], lines, (dt.name, mode, masked))


def test_strength_zero_equals_the_plain_render(program, workdir):
    dt = np.dtype(np.int16)
    for mode in R.MODES:
        cases = SC.cases(dt.name, mode, True)
        got, lines = _run_group(program, workdir, dt, mode, True, cases, np.full(256, 255, dtype=np.uint8),
                                lambda i, h, w, C: _grid(h, w, C))
        wants = []
        for C, n, rgba, rect, h, w, drs, lead, shaded in cases:
            want = np.full(len(shaded), 0xA5, dtype=np.uint8)
            np.lib.stride_tricks.as_strided(want[lead:], shape=(h, w * C), strides=(drs, 1))[...] = \
                SC.plain(dt.name, mode, True, C, rect, h, w, n, rgba).reshape(h, w * C)
            wants.append(want)
        _compare(got, wants, lines, mode)
