"""The corpus of tests/wide_cells.py reaches every coded form of a 32-bit stream it is meant to reach (CPU, the oracle
alone), at level 5 and at level 8.

The GPU tests compare bytes with the oracle on these rasters; this file holds that the oracle's own output on them does
contain each form ("cell"), names the frame that reaches it, and that every stream decodes to the normalised samples.
The cell list is this file's own table: (cell, the recipe meant for it).  A cell that is not reached fails and names
that recipe; the recipe is then to be changed, never the list.  Run with -s for the tables.

libFLAC 1.4.3 picks the fixed-predictor estimator per subframe from subframe_bps = 32 - wasted (+ 1 for a side): below
28 the plain one (every estimate from its own total; CONSTANT when total 1 is zero and the samples are equal), from 28
on ..._limit_residual (every estimate from total 0: a non-zero constant block is FIXED 1, never CONSTANT; an order with
a difference beyond INT32_MAX is out).  ("estimator", "limit_residual", "constant") is therefore a cell that must NOT
be reached.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import wide_cells as W

KINDS = ("verbatim", "fixed", "lpc")


def _mono_census(dtype="float64", level=5):
    return W.census_of_tiles(W.tiles_reference("mono", dtype, level), 4 * W.FRAME, W.mono_names(dtype))


def _stereo_census(level=5):
    fr, pcm, mn, mx = W.stream_reference(2, level)
    return W.census_of_stream(fr, 2, len(pcm), W.stereo_names())


def _show(title, cells, wanted):
    print(f"\n{title}")
    for r, meant in wanted:
        print(f"  {' '.join(str(v) for v in r):40s} {cells.get(r, '-- not reached')}   (meant: {meant})")


def _require(title, census, wanted):
    """every cell of `wanted` is reached, and by the recipe meant for it (a two-channel pair by either channel)"""
    cells = W.cells_of(census)
    _show(title, cells, wanted)
    missing = []
    for r, meant in wanted:
        own = [c for c in census if c["name"] == meant or c["name"].startswith(meant + "/")]
        if not any(r in W.cells_of([c]) for c in own):
            missing.append(f"{' '.join(str(v) for v in r)} (recipe {meant}{'' if own else ': not in the corpus'}; "
                           f"reached by {cells.get(r, 'none')})")
    assert not missing, f"{title}: cells not reached by their recipes: " + "; ".join(missing)
    return cells


def _wname(w):
    return 12 if w == "9+" else w


# the float64 mono corpus at level 5: (cell, recipe meant for it)
MONO_5 = (
    # both estimators: wasted bits 0 and 4 (sbps >= 28), 5, 7 and 9 or more (sbps < 28), each under the three kinds
    [(("kind at", k, w), f"w{_wname(w)}_{'walk' if k == 'fixed' else 'ar2' if k == 'lpc' else k}")
     for w in (0, 4, 5, 7, "9+") for k in KINDS]
    + [(("kind at", "constant", w), f"const_w{_wname(w)}") for w in (5, 7, "9+")]
    + [(("estimator", "limit_residual", k), f"w4_{r}") for k, r in zip(KINDS, ("verbatim", "walk", "ar2"))]
    + [(("estimator", "plain", k), f"w5_{r}") for k, r in zip(KINDS, ("verbatim", "walk", "ar2"))]
    + [(("estimator", "plain", "constant"), "const_w5")]
    + [(("type", "CONSTANT"), "const_w5"), (("type", "VERBATIM"), "noise_full")]
    # fixed predictors on wide samples, LPC orders 1..8
    + [(("type", f"FIXED {k}"), "fixed0_big" if k == 0 else f"walk_o{k}") for k in range(5)]
    + [(("type", f"LPC {k}"), "ar1_0.5" if k == 1 else f"ar{k}") for k in range(1, 9)]
    + [(("precision", 15), "ar2"), (("coef", "most positive"), "coef_top"), (("coef", "most negative"), "coef_bottom")]
    + [(("shift", s), r) for s, r in ((9, "multisine_12"), (10, "multisine_hi"), (11, "sine_200.5"),
                                      (12, "sine_900.5"), (13, "ar2"), (14, "ar1_0.5"), (15, "ar1_0.12"))]
    # residual coding
    + [(("porder", "fixed", p), r) for p, r in enumerate(("quiet", "step_2048", "step_1024", "step_512", "step_256",
                                                          "step_128"))]
    + [(("porder", "lpc", p), r) for p, r in enumerate(("ar2", "ar2_step_2048", "ar2_step_1024", "ar2_step_512",
                                                        "ar2_step_256", "ar2_step_128"))]
    + [(("method", 0), "quiet"), (("method", 1), "rice_15"), (("rice", 15), "rice_15"), (("rice", 16), "rice_16"),
       (("rice", 20), "rice_20"), (("rice", 25), "fixed0_big"), (("rice", 29), "rice_29"), (("rice", 30), "rice_30"),
       (("rice mixed",), "step_mixed")]
    + [(("rice", 0), "const_w0"), (("rice", 5), "quiet")])
MONO_8 = [(("type", f"LPC {k}"), f"ar{k}") for k in range(9, 13)] + [(("porder", "fixed", 6), "tie_0_1")]
STEREO_5 = ([(("assignment", a), r) for a, r in ((1, "independent"), (8, "left_side"), (9, "right_side"),
                                                 (10, "mid_side"))]
            + [(("side", "verbatim"), "side_33_verbatim"), (("side sbps", 33), "side_33_verbatim"),
               (("side sbps", 28), "side_w5"), (("side sbps", 27), "side_w6"), (("side", "constant"), "side_w6_const"),
               (("side", "fixed"), "side_w5"), (("side", "lpc"), "side_lpc")])
TAILS_5 = ([(("tail", 1024, k), f"tail_{r}") for k, r in (("constant", "const_w5"), ("fixed", "w7_walk"),
                                                         ("lpc", "w5_ar2"), ("verbatim", "noise_full"))]
           + [(("tail", "5..16", k), f"{r}/tail") for k, r in (("constant", "const_w5"), ("fixed", "w7_walk"),
                                                              ("verbatim", "noise_full"))]
           + [(("tail", "<=4", "verbatim"), "noise_full/tail")])


def test_corpus_is_small_and_normalises_to_its_recipes():
    fr = W.frames()
    assert len(fr) % 4 == 0 and len(fr) <= 120 and len(W.stereo_frames()) <= 60 and len(W.partial_frames()) <= 60
    got = W.samples(W.mono_band("float64")).reshape(-1, W.FRAME)
    for f, (name, x) in enumerate(fr):
        assert np.array_equal(got[f], x), name                   # (INT32_MIN targets: NaN, +-inf, 257.0, -300.0)
    assert sum(int((x == W.MIN32).sum()) for _, x in fr) >= 10   # every special value is used
    sf = W.stereo_frames()
    got = W.samples(W.stereo_raster())
    for f, (name, l, r) in enumerate(sf):
        assert np.array_equal(got[0].reshape(-1, W.FRAME)[f], l) and np.array_equal(got[1].reshape(-1, W.FRAME)[f], r), name
    print(f"\n{len(fr)} mono frames, {len(sf)} pairs, {len(W.partial_frames())} frames in 96 x 96 tiles")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_extremes_are_numpy_s(dtype):
    """data_min / data_max are np.min / np.max of the tile: NaN for both as soon as the tile holds one, of either
    sign; +-inf otherwise stay.  The corpus has tiles of each kind."""
    band = W.mono_band(dtype)
    data, off, mins, maxs = W.tiles_reference("mono", dtype)
    kinds = set()
    for t in range(len(off) - 1):
        tile = band[t * W.TILE:(t + 1) * W.TILE]
        with np.errstate(invalid="ignore"):
            want = (float(np.min(tile)), float(np.max(tile)))
        got = (mins[t], maxs[t])
        assert all(g == w or (np.isnan(g) and np.isnan(w)) for g, w in zip(got, want)), (dtype, t, got, want)
        nan = tile[np.isnan(tile)]
        kinds |= {("nan", bool(np.signbit(nan).all()), bool((~np.signbit(nan)).all()))} if nan.size else \
            {("inf",)} if np.isinf(tile).any() else {("finite",)}
    assert {("finite",), ("nan", False, True)} <= kinds, kinds         # (a tile whose only NaN has the sign clear)
    if dtype == "float32":
        assert ("nan", True, False) in kinds, kinds                     # (... and one whose only NaN has it set)


def test_float64_reaches_every_cell_at_level_5():
    cells = _require("float64 mono, level 5", _mono_census(), MONO_5)
    assert ("estimator", "limit_residual", "constant") not in cells   # the quirk: never CONSTANT at sbps >= 28
    assert ("escape",) not in cells


def test_level_8_adds_the_long_predictors():
    cells = _require("float64 mono, level 8", _mono_census(level=8), MONO_8)
    missing = [c for c, _ in MONO_5 if c not in cells and c[0] in ("kind at", "estimator")]
    assert not missing, missing
    assert ("estimator", "limit_residual", "constant") not in cells


def test_level_0_keeps_the_estimators_apart():
    cells = W.cells_of(_mono_census(level=0))
    assert not any(c[0] == "type" and c[1].startswith("LPC") for c in cells)
    for k in ("verbatim", "fixed"):
        assert ("estimator", "plain", k) in cells and ("estimator", "limit_residual", k) in cells, k
    assert ("estimator", "plain", "constant") in cells and ("estimator", "limit_residual", "constant") not in cells


def test_constants_and_the_w4_w5_neighbours():
    cen = {c["name"]: c for c in _mono_census()}
    want = {"zeros": ("fixed", 0, 0), "const_w0": ("fixed", 1, 0), "const_w4": ("fixed", 1, 4),
            "const_w5": ("constant", 0, 5), "const_w7": ("constant", 0, 7), "const_w12": ("constant", 0, 12),
            "const_w28": ("constant", 0, 28)}
    for name, form in want.items():
        c = cen[name]
        assert (c["kind"], c["order"], c["wasted"]) == form, (name, c)
        assert c["kind"] == "constant" or set(c["params"]) == {0}, (name, c)     # (zero residuals)
    # the same shape at w = 4 (sbps 28, limit_residual) and at w = 5 (sbps 27, plain)
    fr = dict(W.frames())
    for base in ("walk", "ar2", "verbatim"):
        a, b = cen[f"w4_{base}"], cen[f"w5_{base}"]
        assert (a["wasted"], b["wasted"]) == (4, 5) and a["kind"] == b["kind"], (a, b)
        if base != "verbatim":
            assert np.array_equal(fr[f"w4_{base}"] >> 4, fr[f"w5_{base}"] >> 5)
            assert (a["order"], a["porder"], a["params"], a["coefs"]) == (b["order"], b["porder"], b["params"], b["coefs"])


def _limit_totals(x):
    """FLAC__fixed_compute_best_predictor_limit_residual's five totals: sum |k-th difference| over samples k..n-1"""
    d = np.asarray(x, dtype=np.int64)
    out = []
    for _ in range(5):
        out.append(int(np.abs(d).astype(object).sum()))
        d = np.diff(d)
    return out


def test_fixed_total_ties_and_totals_past_32_bits():
    """In each tie frame two of the five totals are equal, non-zero and the smallest, in the limit_residual form (these
    frames have no wasted bits) as in the plain one, and the frame is coded FIXED of the lower order."""
    cen = {c["name"]: c for c in _mono_census()}
    frames = dict(W.frames())
    for k in range(4):
        name = f"tie_{k}_{k + 1}"
        for T in (W.fixed_totals(frames[name]), _limit_totals(frames[name])):
            assert T[k] == T[k + 1] == min(T) > 0 and sorted(T)[2] > T[k], (name, T)
        assert (cen[name]["kind"], cen[name]["order"], cen[name]["wasted"]) == ("fixed", k, 0), (name, cen[name])
    assert _limit_totals(frames["tie_0_1"])[0] >= 2 ** 32
    for name in ("fixed0_big", "walk_o1", "walk_o4", "rice_30"):
        assert cen[name]["kind"] == "fixed" and max(_limit_totals(frames[name])) >= 2 ** 32, name
    assert _limit_totals(frames["rice_30"])[0] >= 2 ** 41      # the chosen order's own total


def test_int32_min_samples_and_the_validity_of_orders():
    frames = dict(W.frames())
    for level in (5, 8):
        cen = {c["name"]: c for c in _mono_census(level=level)}
        # order 0 is out (|INT32_MIN| > INT32_MAX), 1 stays, 2..4 are out: FIXED 1
        assert W.limit_residual_validity(frames["min_order1"]) == [False, True, False, False, False]
        assert (cen["min_order1"]["kind"], cen["min_order1"]["order"]) == ("fixed", 1), cen["min_order1"]
        # a +- full-scale pair: only order 0 survives
        assert W.limit_residual_validity(frames["only_order0"]) == [True, False, False, False, False]
        assert (cen["only_order0"]["kind"], cen["only_order0"]["order"]) == ("fixed", 0), cen["only_order0"]
        # an LPC candidate whose residual does not fit in int32 is dropped: FIXED 1 (order 1 alone is valid) ...
        assert (frames["lpc_dropped"] == W.MIN32).sum() == 1
        assert W.limit_residual_validity(frames["lpc_dropped"]) == [False, True, False, False, False]
        assert (cen["lpc_dropped"]["kind"], cen["lpc_dropped"]["order"]) == ("fixed", 1), cen["lpc_dropped"]
        # ... or VERBATIM (no order valid) where the same sine without the sample is an LPC subframe of 19 bits
        assert W.limit_residual_validity(frames["lpc_dropped_verbatim"]) == [False] * 5
        assert cen["lpc_dropped_verbatim"]["kind"] == "verbatim" and cen["sine_900.5"]["kind"] == "lpc"
        assert max(cen["sine_900.5"]["params"]) <= 20
        assert np.array_equal(np.flatnonzero(frames["lpc_dropped_verbatim"] != frames["sine_900.5"]), [1001])
        # INT32_MIN inside VERBATIM subframes, and under wasted bits (where it is an ordinary sample)
        for name in ("min_in_verbatim", "min_in_sine"):
            assert cen[name]["kind"] == "verbatim" and (frames[name] == W.MIN32).any(), name
        for name, w in (("min_under_w4", 4), ("min_under_w7", 7)):
            assert (cen[name]["kind"], cen[name]["wasted"]) == ("fixed", w) and (frames[name] == W.MIN32).any(), name


def test_lpc_products_need_the_64_bit_accumulator():
    """Coefficients at either end of the 15-bit code on samples near full scale: |sum q x| of 2^44 and more"""
    cen = {c["name"]: c for c in _mono_census()}
    frames = dict(W.frames())
    for name, q in (("coef_top", 16383), ("coef_bottom", -16384)):
        c = cen[name]
        assert (c["kind"], c["order"], c["precision"], c["shift"], c["coefs"]) == ("lpc", 1, 15, 15, (q,)), (name, c)
        assert W.lpc_sums(c, frames[name]) >= 2 ** 44, name
    for name in ("ar8", "ar4", "alt_sine_3_full"):
        assert cen[name]["kind"] == "lpc" and W.lpc_sums(cen[name], frames[name]) >= 2 ** 40, name


def test_float32_cells():
    """The forms a float32 DEM takes: every |x| >= 32 carries 5 wasted bits, so the plain estimator decides."""
    x = W._rng(50).uniform(32, 256, 4096).astype(np.float32) * W._rng(51).choice([-1, 1], 4096).astype(np.float32)
    assert not (W.samples(x) & 31).any()
    cen = {c["name"]: c for c in _mono_census("float32")}
    want = {"f32_const_32": ("constant", 0, 5), "f32_const_33": ("constant", 0, 5), "f32_const_96": ("constant", 0, 7),
            "f32_const_16": ("fixed", 1, 4), "f32_zeros": ("fixed", 0, 0), "f32_const_neg_200": ("constant", 0, 8)}
    for name, form in want.items():
        assert (cen[name]["kind"], cen[name]["order"], cen[name]["wasted"]) == form, (name, cen[name])
    for name in ("f32_nan_in_sine", "f32_big_in_sine", "f32_32k_noise", "f32_whole_metres", "f32_sine_metres"):
        assert cen[name]["wasted"] >= 5 and W.sbps_of(cen[name]) < 28, (name, cen[name])
    assert cen["f32_32k_noise"]["method"] == 1 and 23 in cen["f32_32k_noise"]["params"], cen["f32_32k_noise"]
    band = W.samples(W.mono_band("float32")).reshape(-1, W.FRAME)
    names = W.mono_names("float32")
    assert (band[names.index("f32_nan_in_sine")] == W.MIN32).sum() == 1
    assert (band[names.index("f32_big_in_sine")] == W.MIN32).sum() == 1
    cells = _require("float32 mono", list(cen.values()),
                     [(("estimator", "plain", k), r) for k, r in zip(KINDS, ("w5_verbatim", "f32_whole_metres", "f32_inf_in_sine"))]
                     + [(("estimator", "limit_residual", k), r) for k, r in zip(KINDS, ("noise_full", "f32_const_16", "ar2"))]
                     + [(("estimator", "plain", "constant"), "f32_const_32")])
    assert ("estimator", "limit_residual", "constant") not in cells


@pytest.mark.parametrize("dtype", ["int32", "uint32"])
def test_integer_dtypes_report_what_they_reach(dtype):
    """+-8388607 in a 32-bit stream: no wasted bits but in whole constant frames.  Held: FIXED and LPC, both Rice
    methods, and the tile whose max - min does not fit the dtype."""
    cen = _mono_census(dtype)
    cells = W.cells_of(cen)
    _show(f"{dtype} mono", cells, [(c, "") for c in sorted(cells, key=str) if c[0] in ("type", "method", "porder")])
    assert {c[1].split()[0] for c in cells if c[0] == "type"} >= {"FIXED", "LPC"}
    assert ("method", 0) in cells and ("method", 1) in cells
    band = W.mono_band(dtype)
    last = band[-W.TILE:].astype(np.int64)
    assert int(last.max() - last.min()) > (2 ** 31 if dtype == "int32" else 2 ** 32 - 2)
    pcm = W.samples(band[:W.TILE])
    assert pcm.min() == -8388607 and pcm.max() == 8388607
    assert not W.samples(band[-2 * W.TILE:-W.TILE]).any()        # the constant tile: all zero, FIXED 0
    assert all(c["kind"] == "fixed" and c["order"] == 0 for c in cen if c["name"].startswith("i_const_tile"))


def test_two_band_cells():
    for level in (5, 8):
        cen = _stereo_census(level)
        _require(f"two bands, level {level}", cen, STEREO_5)
        by = {c["name"]: c for c in cen}
        c = by["side_33_verbatim/R"]
        assert (c["kind"], c["wasted"], c["assignment"]) == ("verbatim", 0, 10), c
        assert (by["side_w5/R"]["wasted"], by["side_w6/R"]["wasted"]) == (5, 6)
        assert (by["side_w5_const/R"]["kind"], by["side_w5_const/R"]["order"], by["side_w5_const/R"]["wasted"]) == \
            ("fixed", 1, 5), by["side_w5_const/R"]                 # sbps 28: the quirk side
        assert (by["side_w6_const/R"]["kind"], by["side_w6_const/R"]["wasted"]) == ("constant", 6)   # sbps 27
        assert by["side_w5_const/R"]["assignment"] == by["side_w6_const/R"]["assignment"] == 8
        assert (by["equal/R"]["kind"], by["equal/R"]["order"], by["equal/R"]["assignment"]) == ("fixed", 0, 8)
    sf = W.stereo_frames()
    side = dict((n, l - r) for n, l, r in sf)["side_33_verbatim"]
    assert side.min() < W.MIN32 and side.max() > W.S and (side & 1).all()


def test_two_band_tie_between_the_two_best_assignments():
    """fixed0_tie: right = 0, so the side is the left channel sample for sample, and the left is a FIXED 0 subframe --
    no warm-up sample, so its estimate does not depend on the subframe's width.  Independent and right-side then cost
    the same, left-side and mid-side more: libFLAC keeps independent, a later assignment winning only when strictly
    smaller."""
    cen = {c["name"]: c for c in _stereo_census()}
    left, right = cen["fixed0_tie/L"], cen["fixed0_tie/R"]
    assert left["assignment"] == 1 and (left["kind"], left["order"]) == ("fixed", 0), left
    assert (right["kind"], right["order"], set(right["params"])) == ("fixed", 0, {0}), right
    l, r = dict((n, (a, b)) for n, a, b in W.stereo_frames())["fixed0_tie"]
    assert not r.any() and left["wasted"] == 1


def test_three_bands_reach_the_mono_cells():
    fr, pcm, mn, mx = W.stream_reference(3)
    cells = W.cells_of(W.census_of_stream(fr, 3, len(pcm), W.multi_names(3)))
    missing = [c for c, _ in MONO_5 if c not in cells]
    assert not missing, missing


def test_tails_reach_their_cells():
    cen = [c for c in W.census_of_tiles(W.tiles_reference("partial"), W.PTILE ** 2, [n for n, _ in W.partial_frames()])
           if c["name"].startswith("tail_")]
    assert len(cen) == len(W.TAILS) and all(c["blocksize"] == W.TAIL for c in cen)
    for tail in (3, 11):
        tiny = W.census_of_tiles(W.tiles_reference(f"tiny{tail}"), W.FRAME + tail, W.tiny_names())
        assert all(c["blocksize"] == tail for c in tiny[1::2])
        cen += tiny[1::2]
    cells = _require("tails", cen, TAILS_5)
    by = {(c["name"], c["blocksize"]): c for c in cen}
    assert by[("tail_const_w4", 1024)]["kind"] == "fixed" and by[("tail_zeros", 1024)]["kind"] == "fixed"
    assert all(c["kind"] == "verbatim" for c in cen if c["blocksize"] == 3)
    assert {c[2] for c in cells if c[:2] == ("porder", "fixed")} >= {0, 3, 4}


@pytest.mark.parametrize("level", [0, 5, 8])
def test_every_stream_decodes_to_the_normalised_samples(level):
    for dtype in ("float64", "float32") + (("int32", "uint32") if level == 5 else ()):
        band = W.mono_band(dtype)
        data, off, mn, mx = W.tiles_reference("mono", dtype, level)
        for t in range(len(off) - 1):
            want = W.samples(band[t * W.TILE:(t + 1) * W.TILE]).reshape(-1)
            got = O.decode_frames(data[off[t]:off[t + 1]], 1, 32, 4 * W.FRAME).reshape(-1)
            assert np.array_equal(got, want), (dtype, level, t)
    if level == 5:
        for kind, band in (("partial", W.partial_band()), ("tiny3", W.tiny_band(3)), ("tiny11", W.tiny_band(11))):
            data, off, mn, mx = W.tiles_reference(kind)
            th = W.PTILE if kind == "partial" else 1
            for t in range(len(off) - 1):
                want = W.samples(band[t * th:(t + 1) * th]).reshape(-1)
                assert np.array_equal(O.decode_frames(data[off[t]:off[t + 1]], 1, 32, want.size).reshape(-1), want)
    for bands in (2, 3) if level != 0 else (2,):
        fr, pcm, mn, mx = W.stream_reference(bands, level if bands == 2 else 5)
        assert np.array_equal(O.decode_frames(fr, bands, 32, len(pcm)), pcm), (bands, level)
    if level == 5:
        fr, pcm, mn, mx = W.stream_reference(2, 4)      # loose mid/side
        assert np.array_equal(O.decode_frames(fr, 2, 32, len(pcm)), pcm)
