// nodata_groups_host.hip -- run downsample_group (frs_pyramid.hip) and window_group (frs_window.hip) on the HOST, lane
// by lane, under both mask policies, against a direct per-pixel evaluation with the scalar functions of frs_nodata.h
// (Nodata<T>) and of frs_resample.h / frs_window_map.h (NoNodata).  Source and destination live in allocations of
// exactly their extent, so that a build with the address and undefined-behaviour sanitizers reports any read or write
// outside them; every destination element outside [height][width] must keep its sentinel.  No GPU is used.  The cases
// are those of tests/test_gpu_pyramid_nodata.py and test_gpu_window_nodata.py: their shapes, layouts, masks, nodata
// values, rectangles and destination sizes; the unmasked policy walks the same shapes, layouts, rectangles and sizes
// over sources of random values, in every instantiation the library launches.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=all -I flac_raster_amd/csrc -I include -o nodata_groups_host
//         tools/micro/nodata_groups_host.hip && ./nodata_groups_host
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <random>
#include <vector>

#include "frs_pyramid.hip"
#include "frs_window.hip"

// what the two files need of the rest of the library (their jobs are not run here)
namespace frs {
void prof_begin(frs_ctx *, const char *, hipEvent_t *, hipStream_t) {}
void prof_end(frs_ctx *, const char *, hipEvent_t, hipStream_t) {}
void prof_collect(frs_ctx *) {}
int dtype_size(int dt) {
    static const int sz[8] = {0, 1, 2, 2, 4, 4, 4, 8};
    return dt >= 1 && dt <= 7 ? sz[dt] : 0;
}
bool nodata_ok(int, double) { return true; }
}  // namespace frs

using namespace frs;

static long g_cases = 0, g_bad = 0;
static char g_note[200];  // the case being checked, for the message
static std::mt19937_64 g_rng(12345);

template <typename T> static bool same(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0 || (a != a && b != b); }

template <typename T> static T sentinel() {
    T s;
    memset(&s, 0xa5, sizeof(T));
    return s;
}

template <typename T> static T random_value() {
    if constexpr (NdFloat<T>::value) {
        const int k = (int)(g_rng() % 40);
        if (k == 0) return std::numeric_limits<T>::quiet_NaN();
        if (k == 1) return std::numeric_limits<T>::infinity();
        if (k == 2) return -std::numeric_limits<T>::infinity();
        if (k == 3) return (T)-0.0;
        return (T)(((double)(g_rng() % 2000001) - 1000000.0) * pow(10.0, (double)(g_rng() % 7) - 3.0));
    } else {
        const int k = (int)(g_rng() % 6);
        if (k == 0) return std::numeric_limits<T>::min();
        if (k == 1) return std::numeric_limits<T>::max();
        return (T)g_rng();
    }
}

// an exact-size raster: C bands of h x w with row padding, band slack and `lead` elements before and after
template <typename T> struct Raster {
    int64_t C, h, w, rs, bs, lead, ext;
    T *buf;
    Raster(int64_t C_, int64_t h_, int64_t w_, int64_t pad, int64_t slack, int64_t lead_)
        : C(C_), h(h_), w(w_), rs(w_ + pad), bs((w_ + pad) * h_ + slack), lead(lead_) {
        ext = lead + (C - 1) * bs + (h - 1) * rs + w + lead;
        buf = (T *)malloc((size_t)ext * sizeof(T));
        for (int64_t i = 0; i < ext; i++) buf[i] = sentinel<T>();
    }
    ~Raster() { free(buf); }
    T *origin() { return buf + lead; }
    T &at(int64_t c, int64_t r, int64_t x) { return buf[lead + c * bs + r * rs + x]; }
    bool inside(int64_t i) const {  // is element i of buf a pixel?
        i -= lead;
        if (i < 0) return false;
        const int64_t c = i / bs, o = i % bs;
        return c < C && o / rs < h && o % rs < w;
    }
};

// mask k of the tests: 0 none, 1 all, 2 checkerboard, 3 ~30 % random, 4 one valid per block, 5 last column and row,
// 6 a collar of 3 pixels
template <typename T> static void fill_plain(Raster<T> &s) {
    for (int64_t c = 0; c < s.C; c++)
        for (int64_t r = 0; r < s.h; r++)
            for (int64_t x = 0; x < s.w; x++) s.at(c, r, x) = random_value<T>();
}

template <typename T> static void fill_source(Raster<T> &s, T nd, int mask) {
    for (int64_t c = 0; c < s.C; c++)
        for (int64_t r = 0; r < s.h; r++)
            for (int64_t x = 0; x < s.w; x++) {
                T v = random_value<T>();
                while (nd_is(v, nd)) v = random_value<T>();
                bool m = false;
                if (mask == 1) m = true;
                if (mask == 2) m = (r + x) % 2 == 0;
                if (mask == 3) m = g_rng() % 10 < 3;
                if (mask == 4) m = (int64_t)(g_rng() % 4) != (r % 2) * 2 + x % 2;
                if (mask == 5) m = r == s.h - 1 || x == s.w - 1;
                if (mask == 6) m = r < 3 || x < 3 || r >= s.h - 3 || x >= s.w - 3;
                s.at(c, r, x) = m ? (NdFloat<T>::value && nd == 0 && g_rng() % 2 ? (T)-0.0 : nd) : v;
            }
}

template <typename T, typename F> static void check(Raster<T> &d, F want, const char *what) {
    g_cases++;
    for (int64_t i = 0; i < d.ext; i++) {
        T w = sentinel<T>();
        if (d.inside(i)) {
            const int64_t j = i - d.lead, c = j / d.bs, o = j % d.bs;
            w = want(c, o / d.rs, o % d.rs);
        }
        if (!same(d.buf[i], w)) {
            if (g_bad++ < 10)
                fprintf(stderr, "%s: element %lld differs, got %g want %g (%s)\n", what, (long long)i, (double)d.buf[i],
                        (double)w, g_note);
            return;
        }
    }
}

// every lane of a gx x gy grid over the C bands
template <int ES, int MODE, int DT, typename Mask>
static void run_pyramid(Raster<typename PyrElem<ES, DT>::T> &s, Raster<typename PyrElem<ES, DT>::T> &d,
                        const PyrParams &P, const Mask &mask) {
    const int64_t gx = 1 + (int64_t)(g_rng() % 2), gy = 1 + (int64_t)(g_rng() % 3);
    for (int64_t c = 0; c < s.C; c++)
        for (int64_t bx = 0; bx < gx; bx++)
            for (int64_t by = 0; by < gy; by++)
                for (uint32_t tid = 0; tid < (uint32_t)kPyrBlock; tid++)
                    downsample_group<ES, MODE, DT>(s.origin() + c * s.bs, d.origin() + c * d.bs, P, mask, bx, gx, by,
                                                   gy, tid);
}

// MASKED: the average under Nodata<T>, every nodata value and mask; otherwise (ES, MODE, DT) under NoNodata
template <int ES, int MODE, int DT, bool MASKED> static long pyramid_cases() {
    using T = typename PyrElem<ES, DT>::T;
    const long before = g_cases;
    const int64_t shapes[][2] = {{1, 1}, {2, 2}, {3, 5}, {5, 3}, {33, 67}, {64, 130}, {4, 131}, {3, 9000 / ES}};
    std::vector<double> nds = {0.0};
    if constexpr (MASKED) {
        nds.push_back(5.0);
        if constexpr (NdFloat<T>::value) {
            nds.insert(nds.end(), {(double)std::numeric_limits<T>::lowest(), (double)std::numeric_limits<T>::max(), NAN,
                                   -INFINITY});
        } else {
            nds.insert(nds.end(), {(double)std::numeric_limits<T>::min(), (double)std::numeric_limits<T>::max()});
        }
    }
    for (double ndd : nds)
        for (auto &sh : shapes)
            for (int64_t C : {1, 3})
                for (int layout = 0; layout < 2; layout++)
                    for (int mask = 0; mask < (MASKED ? 6 : 1); mask++) {
                        const int64_t H = sh[0], W = sh[1], h = (H + 1) / 2, w = (W + 1) / 2;
                        const int64_t pad = layout ? 3 : 0, slack = layout ? 5 : 0, lead = layout ? 1 : 0;
                        Raster<T> s(C, H, W, pad, slack, lead), d(C, h, w, pad, slack, lead);
                        PyrParams P;
                        P.src_h = H, P.src_w = W, P.dst_h = h, P.dst_w = w;
                        P.src_row_stride = s.rs, P.src_band_stride = s.bs, P.dst_row_stride = d.rs, P.dst_band_stride = d.bs;
                        snprintf(g_note, sizeof g_note, "ES %d mode %d dtype %d masked %d nodata %g, %lld x %lld x %lld, layout %d, mask %d",
                                 ES, MODE, DT, (int)MASKED, ndd, (long long)C, (long long)H, (long long)W, layout, mask);
                        if constexpr (MASKED) {
                            const T nd = nd_cast<T>(ndd);
                            fill_source(s, nd, mask);
                            run_pyramid<ES, MODE, DT>(s, d, P, Nodata<T>{nd});
                            check(d, [&](int64_t c, int64_t r, int64_t x) {
                                const bool right = 2 * x + 1 < W, below = 2 * r + 1 < H;
                                T v[4];
                                int m = 0;
                                for (int k = 0; k < 4; k++) {
                                    if ((k & 1 && !right) || (k & 2 && !below)) continue;
                                    const T p = s.at(c, 2 * r + (k >> 1), 2 * x + (k & 1));
                                    if (!nd_is(p, nd)) v[m++] = p;
                                }
                                return nd_mean(v, m, nd);
                            }, "pyramid, masked");
                        } else {
                            fill_plain(s);
                            run_pyramid<ES, MODE, DT>(s, d, P, NoNodata{});
                            check(d, [&](int64_t c, int64_t r, int64_t x) {
                                const bool right = 2 * x + 1 < W, below = 2 * r + 1 < H;
                                const T a = s.at(c, 2 * r, 2 * x);
                                if constexpr (MODE == kResampleNearest) return a;
                                else {
                                    if (right && below)
                                        return resample_avg4(a, s.at(c, 2 * r, 2 * x + 1), s.at(c, 2 * r + 1, 2 * x),
                                                             s.at(c, 2 * r + 1, 2 * x + 1));
                                    if (right) return resample_avg2(a, s.at(c, 2 * r, 2 * x + 1));
                                    if (below) return resample_avg2(a, s.at(c, 2 * r + 1, 2 * x));
                                    return a;
                                }
                            }, "pyramid, unmasked");
                        }
                    }
    return g_cases - before;
}

// one output by the definition; nd is read under Nodata<T> only
template <int MODE, typename T, bool MASKED>
static T window_direct(Raster<T> &s, int64_t c, const WinParams &P, T nd, int64_t r, int64_t x) {
    const WinAxis ax = win_axis(P.x0, P.width, P.dst_w, P.src_w), ay = win_axis(P.y0, P.height, P.dst_h, P.src_h);
    const T fill = win_result<T>(P.fill);
    if constexpr (MODE == kWindowNearest) {
        const WinNearest nx = win_nearest(ax, x), ny = win_nearest(ay, r);
        if (!(nx.valid && ny.valid)) return fill;
        const T v = s.at(c, ny.i, nx.i);
        return MASKED && nd_is(v, nd) ? fill : v;
    } else if constexpr (MODE == kWindowBilinear) {
        const WinLinear lx = win_linear(ax, x), ly = win_linear(ay, r);
        if (!(lx.valid && ly.valid)) return fill;
        const T a = s.at(c, ly.i0, lx.i0), b = s.at(c, ly.i0, lx.i1), cc = s.at(c, ly.i1, lx.i0), d = s.at(c, ly.i1, lx.i1);
        if constexpr (!MASKED)
            return win_result<T>(win_bilinear_value((double)a, (double)b, (double)cc, (double)d, lx.t, ly.t));
        else
            return nd_win_result<T>(nd_bilinear((double)a, (double)b, (double)cc, (double)d, !nd_is(a, nd), !nd_is(b, nd),
                                                !nd_is(cc, nd), !nd_is(d, nd), lx.t, ly.t), fill, nd);
    } else {
        const WinArea rx = win_area(ax, x), ry = win_area(ay, r);
        if (!(rx.valid && ry.valid)) return fill;
        if constexpr (!MASKED) {
            double sum = 0.0;
            for (int64_t j = ry.i0; j < ry.i1; j++) {
                double row = 0.0;
                for (int64_t i = rx.i0; i < rx.i1; i++) row = row + win_area_weight(rx, i) * (double)s.at(c, j, i);
                sum = sum + win_area_weight(ry, j) * row;
            }
            return win_result<T>(win_area_value(sum, rx, ry));
        } else {
            NdArea acc;
            for (int64_t j = ry.i0; j < ry.i1; j++) {
                for (int64_t i = rx.i0; i < rx.i1; i++) {
                    const T v = s.at(c, j, i);
                    acc.tap(win_area_weight(rx, i), (double)v, !nd_is(v, nd));
                }
                acc.end_row(win_area_weight(ry, j));
            }
            return nd_win_result<T>(acc.value(rx, ry), fill, nd);
        }
    }
}

template <int MODE, typename T, typename Mask>
static void run_window(Raster<T> &s, Raster<T> &d, const WinParams &P, const Mask &mask) {
    const int64_t gx = 1 + (int64_t)(g_rng() % 2), gy = 1 + (int64_t)(g_rng() % 3);
    for (int64_t c = 0; c < d.C; c++)
        for (int64_t bx = 0; bx < gx; bx++)
            for (int64_t by = 0; by < gy; by++)
                for (uint32_t tid = 0; tid < (uint32_t)kWinBlock; tid++)
                    window_group<MODE, T>(s.origin() + c * s.bs, d.origin() + c * d.bs, P, mask, bx, gx, by, gy, tid);
}

template <int MODE, typename T, bool MASKED> static long window_cases() {
    const long before = g_cases;
    const int64_t H = 37, W = 53;
    const int64_t widths[] = {1, 7, 8, 9, 33, 130, 300}, heights[] = {1, 3, 5, 17, 40};
    std::vector<double> nds = {0.0};
    std::vector<int> masks = {0};
    if constexpr (MASKED) {
        if constexpr (NdFloat<T>::value) nds.insert(nds.end(), {NAN, -INFINITY, (double)std::numeric_limits<T>::max()});
        else nds.insert(nds.end(), {(double)std::numeric_limits<T>::min(), (double)std::numeric_limits<T>::max()});
        masks = {0, 1, 3, 6};
    }
    for (double ndd : nds)
        for (int mask : masks) {
            const T nd = nd_cast<T>(ndd);
            Raster<T> s(3, H, W, 3, 5, 1);
            if constexpr (MASKED) fill_source(s, nd, mask);
            else fill_plain(s);
            for (int64_t w : widths)
                for (int64_t h : heights) {
                    const double rects[][4] = {{0.0, 0.0, (double)W, (double)H}, {1.0, 2.0, 2.0 * w, 2.0 * h},
                                               {0.25, 0.6, 1.37 * w, 1.37 * h}, {3.3, 2.7, 0.4 * w, 0.4 * h},
                                               {-2.0, -1.5, 9.3 * w, 9.3 * h}, {-5.5, -3.25, 20.0, 20.0},
                                               {W - 10.5, H - 8.25, 20.0, 20.0}, {-3.0, -4.0, W + 7.5, H + 9.25},
                                               {W + 3.0, 0.0, 10.0, 10.0}, {-20.0, -20.0, 10.0, 10.0},
                                               {4.0, 6.0, 0.5 * w, 0.5 * h}};
                    for (auto &rc : rects)
                        for (int64_t C : {1, 3}) {
                            Raster<T> d(C, h, w, 3, 5, 1);
                            WinParams P;
                            P.src_h = H, P.src_w = W, P.dst_h = h, P.dst_w = w;
                            P.src_row_stride = s.rs, P.src_band_stride = s.bs, P.dst_row_stride = d.rs, P.dst_band_stride = d.bs;
                            P.x0 = rc[0], P.y0 = rc[1], P.width = rc[2], P.height = rc[3];
                            // (a NaN fill is for float rasters with a nodata value only)
                            P.fill = MASKED && NdFloat<T>::value && g_rng() % 3 == 0 ? NAN : g_rng() % 2 ? 200.5 : ndd == ndd && fabs(ndd) < 1e30 ? ndd : 7.0;
                            snprintf(g_note, sizeof g_note, "mode %d, %zu-byte elements, masked %d, nodata %g, mask %d, %lld x %lld, fill %g",
                                     MODE, sizeof(T), (int)MASKED, ndd, mask, (long long)h, (long long)w, P.fill);
                            if constexpr (MASKED) run_window<MODE, T>(s, d, P, Nodata<T>{nd});
                            else run_window<MODE, T>(s, d, P, NoNodata{});
                            check(d, [&](int64_t c, int64_t r, int64_t x) { return window_direct<MODE, T, MASKED>(s, c, P, nd, r, x); },
                                  MASKED ? "window, masked" : "window, unmasked");
                        }
                }
        }
    return g_cases - before;
}

static long g_masked = 0, g_plain = 0;
static bool g_all_plain = true;  // every unmasked instantiation ran at least one case

static void count(const char *what, int mode, const char *type, long masked, long plain, bool has_masked) {
    printf("%-8s mode %d %-8s masked %6ld%s unmasked %6ld\n", what, mode, type, masked, has_masked ? " " : "*", plain);
    g_masked += masked, g_plain += plain;
    if (plain == 0) g_all_plain = false;
}

template <int ES, int DT> static void pyramid_dtype(const char *type) {
    count("pyramid", kResampleAverage, type, pyramid_cases<ES, kResampleAverage, DT, true>(),
          pyramid_cases<ES, kResampleAverage, DT, false>(), true);
}

template <typename T> static void window_dtype(const char *type) {
    count("window", kWindowNearest, type, window_cases<kWindowNearest, T, true>(), window_cases<kWindowNearest, T, false>(), true);
    count("window", kWindowBilinear, type, window_cases<kWindowBilinear, T, true>(), window_cases<kWindowBilinear, T, false>(), true);
    count("window", kWindowAverage, type, window_cases<kWindowAverage, T, true>(), window_cases<kWindowAverage, T, false>(), true);
}

int main() {
    // nearest is instantiated per element size and has no masked form (*)
    count("pyramid", kResampleNearest, "1-byte", 0, pyramid_cases<1, kResampleNearest, 0, false>(), false);
    count("pyramid", kResampleNearest, "2-byte", 0, pyramid_cases<2, kResampleNearest, 0, false>(), false);
    count("pyramid", kResampleNearest, "4-byte", 0, pyramid_cases<4, kResampleNearest, 0, false>(), false);
    count("pyramid", kResampleNearest, "8-byte", 0, pyramid_cases<8, kResampleNearest, 0, false>(), false);
    pyramid_dtype<1, FRS_DT_U8>("uint8");
    pyramid_dtype<2, FRS_DT_U16>("uint16");
    pyramid_dtype<2, FRS_DT_I16>("int16");
    pyramid_dtype<4, FRS_DT_I32>("int32");
    pyramid_dtype<4, FRS_DT_U32>("uint32");
    pyramid_dtype<4, FRS_DT_F32>("float32");
    pyramid_dtype<8, FRS_DT_F64>("float64");
    window_dtype<uint8_t>("uint8");
    window_dtype<uint16_t>("uint16");
    window_dtype<int16_t>("int16");
    window_dtype<int32_t>("int32");
    window_dtype<uint32_t>("uint32");
    window_dtype<float>("float32");
    window_dtype<double>("float64");
    printf("masked cases %ld, unmasked cases %ld, differing %ld\n", g_masked, g_plain, g_bad);
    if (!g_all_plain) fprintf(stderr, "an unmasked instantiation ran no case\n");
    return g_bad || !g_all_plain ? 1 : 0;
}
