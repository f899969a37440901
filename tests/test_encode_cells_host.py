"""The corpus of tests/encode_cells.py reaches every coded subframe form it is meant to reach (CPU, the oracle alone).

The GPU tests compare bytes with the oracle on these frames; this file holds that the oracle's own output on them does
contain each form ("cell"), and names the frame that reaches it -- so a cell that silently dropped out of the corpus
(another seed, another normalisation) fails here, without a GPU.  The census walker itself is pinned in
tests/test_flac_builder.py.  Run with -s for the tables.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import encode_cells as C


def _mono_census(dtype):
    return C.census_of_tiles(C.tiles_reference("mono", dtype), 4 * C.FRAME, [n for n, _ in C.frames()])


def _show(title, cells, wanted):
    print(f"\n{title}")
    for r in wanted:
        print(f"  {' '.join(str(v) for v in r):28s} {cells.get(r, '-- not reached')}")


def test_corpus_is_small_and_in_range():
    fr = C.frames()
    assert len(fr) % 4 == 0 and len(fr) <= 150 and len(C.stereo_frames()) <= 150 and len(C.partial_frames()) <= 150
    assert len({n for n, _ in fr}) == len(fr)
    for t in range(0, len(fr), 4):      # the anchors: every tile normalises by 0 .. 65534
        assert fr[t][1].min() == C.LO and fr[t][1].max() == C.HI, fr[t][0]
    print(f"\n{len(fr)} mono frames, {len(C.stereo_frames())} pairs, {len(C.partial_frames())} frames in 96 x 96 tiles")


def test_exact_frames_survive_the_normalisation():
    """The wasted-bits and tie frames depend on every sample: O.normalize of the uint16 band returns the recipe's."""
    band = C.mono_band("uint16")
    got = np.concatenate([O.normalize(np.ascontiguousarray(band[r:r + C.TILE]))[0].reshape(-1)
                          for r in range(0, band.shape[0], C.TILE)])
    fr = C.frames()
    for f, (name, x) in enumerate(fr):
        same = np.array_equal(got[f * C.FRAME:(f + 1) * C.FRAME], x)
        assert same or name not in C.EXACT, name
        assert np.abs(got[f * C.FRAME:(f + 1) * C.FRAME] - x).max() <= 1, name
    assert len(C.EXACT) >= 16


def test_uint16_reaches_every_required_cell():
    cells = C.cells_of(_mono_census("uint16"))
    _show("uint16 mono, required", cells, C.REQUIRED_MONO + sorted(c for c in cells if c[0] == "wasted"))
    _show("uint16 mono, optional", cells, C.OPTIONAL)
    missing = [r for r in C.REQUIRED_MONO if r not in cells]
    assert not missing, missing
    assert C.wasted_counts_ok(cells), sorted(c for c in cells if c[0] == "wasted")
    assert ("escape",) not in cells     # (level 5 writes none; the decoders' escapes are tests/flac_layouts.py's)


@pytest.mark.parametrize("dtype", ["int16", "uint8"])
def test_other_dtypes_report_what_they_reach(dtype):
    """Their normalisation gives other samples; they are compared on the GPU whatever they reach.  Held here: each
    still reaches all four subframe kinds, wasted bits and three partition orders."""
    cells = C.cells_of(_mono_census(dtype))
    _show(f"{dtype} mono", cells, C.REQUIRED_MONO + C.OPTIONAL)
    kinds = {c[1].split()[0] for c in cells if c[0] == "type"}
    assert kinds == {"CONSTANT", "VERBATIM", "FIXED", "LPC"}
    assert any(c[0] == "wasted" for c in cells) and len({c[2] for c in cells if c[0] == "porder"}) >= 3


def test_fixed_total_ties():
    """In each tie frame two of libFLAC's five fixed totals are equal, non-zero and the smallest, and the oracle codes
    the frame as a FIXED subframe of the lower of the two orders: the first minimum decides the bytes."""
    cen = {c["name"]: c for c in _mono_census("uint16")}
    frames = dict(C.frames())
    for k in range(4):
        name = f"tie_{k}_{k + 1}"
        T = C.fixed_totals(frames[name])
        assert T[k] == T[k + 1] == min(T) > 0 and sorted(T)[2] > T[k], (name, T)
        assert (cen[name]["kind"], cen[name]["order"]) == ("fixed", k), (name, cen[name])


def test_two_channel_cells():
    fr, pcm, mn, mx = C.stream_reference(2)
    assert (mn, mx) == (0.0, 65534.0)
    sf = C.stereo_frames()
    cen = C.census_of_stream(fr, 2, len(pcm), [f"{n}/{ch}" for n, _, _ in sf for ch in "LR"])
    cells = C.cells_of(cen)
    _show("two bands", cells, C.REQUIRED_STEREO + C.REQUIRED_MONO)
    missing = [r for r in C.REQUIRED_STEREO if r not in cells]
    assert not missing, missing
    by = {c["name"]: c for c in cen}
    assert by["equal/R"]["kind"] == "constant" and by["equal/R"]["assignment"] == 8
    assert (by["verbatim_side/R"]["kind"], by["verbatim_side/R"]["wasted"], by["verbatim_side/R"]["assignment"]) == \
        ("verbatim", 2, 10)
    assert by["mid_side/R"]["wasted"] == 2 and by["side_wasted_3/L"]["wasted"] == 3


def _fixed0_estimate(x, w, sbps, params, porder):
    """libFLAC's estimate of a FIXED 0 subframe with these Rice parameters (set_partitioned_rice_'s count): header,
    no warm-up, 6 residual header bits, per partition 4 + (1 + k) n + (sum |r| >> (k - 1)) - n / 2"""
    r = np.abs(np.asarray(x, dtype=np.int64) >> w)
    n = len(r) >> porder
    bits = 8 + w + 0 * sbps + 6
    for p, k in enumerate(params):
        s = int(r[p * n:(p + 1) * n].sum())
        bits += 4 + (1 + k) * n + ((s >> (k - 1)) if k else (s << 1)) - (n >> 1)
    return bits


def test_two_channel_tie_between_the_two_best_assignments():
    """fixed0_tie: right = 0, so the side is the left channel sample for sample, and the left is a FIXED 0 subframe --
    no warm-up sample, so its estimate does not depend on the subframe's width.  Independent (left + a 24-bit CONSTANT)
    and right-side (side + the same CONSTANT) then cost exactly the same, left-side and mid-side twice as much: libFLAC
    keeps independent, a later assignment winning only when strictly smaller.  Held here: the emitted pair is code 1
    with FIXED 0 and CONSTANT, the side's samples are the left's, and the FIXED 0 estimate evaluated for the left (15
    bits a sample under 1 wasted bit) and for the side (16 bits) is one number."""
    fr, pcm, mn, mx = C.stream_reference(2)
    sf = C.stereo_frames()
    f = [n for n, _, _ in sf].index("fixed0_tie")
    cen = O.subframe_census(fr, 2, 16, len(pcm))
    left, right = cen[2 * f], cen[2 * f + 1]
    assert left["assignment"] == 1 and (left["kind"], left["order"]) == ("fixed", 0) and right["kind"] == "constant"
    L, R = pcm[f * C.FRAME:(f + 1) * C.FRAME, 0].astype(np.int64), pcm[f * C.FRAME:(f + 1) * C.FRAME, 1]
    assert not R.any() and np.array_equal(L - R, L) and left["wasted"] == 1
    est = [_fixed0_estimate(x, 1, sbps, left["params"], left["porder"]) for x, sbps in ((L, 15), (L - R, 16))]
    assert est[0] == est[1] and est[0] + 24 < 2 * est[0]


@pytest.mark.parametrize("bands", [3, 8])
def test_dealt_over_channels_every_mono_cell_is_still_reached(bands):
    fr, pcm, mn, mx = C.stream_reference(bands)
    assert (mn, mx) == (0.0, 65534.0)
    cells = C.cells_of(C.census_of_stream(fr, bands, len(pcm), C.multi_names(bands)))
    missing = [r for r in C.REQUIRED_MONO if r not in cells]
    assert not missing and C.wasted_counts_ok(cells), missing


def test_partial_tails_reach_their_cells():
    """The 1024-sample last frames of the 96 x 96 tiles: wasted bits under FIXED, LPC and CONSTANT, FIXED 3 and 4,
    partition orders 1..4 under FIXED 0, VERBATIM."""
    names = [n for n, _ in C.partial_frames()]
    cen = [c for c in C.census_of_tiles(C.tiles_reference("partial", "uint16", C.PTILE), C.PTILE ** 2, names)
           if c["name"].startswith("tail_")]
    assert len(cen) == len(C.TAILS) and all(c["blocksize"] == C.TAIL for c in cen)
    cells = C.cells_of(cen)
    want = ([("type", t) for t in ("CONSTANT", "VERBATIM", "FIXED 0", "FIXED 3", "FIXED 4")]
            + [("porder", "fixed", p) for p in range(5)] + [("wasted type", k) for k in ("fixed", "lpc", "constant")]
            + [("wasted", w) for w in (1, 2, 3, 4, 8, 12)])
    _show("partial tails", cells, want)
    missing = [r for r in want if r not in cells]
    assert not missing, missing


def test_level_8_census_is_printed():
    """Informative: what compression level 8 adds on the same frames (orders up to 12, partition order 6, shifts)."""
    names = [n for n, _ in C.frames()]
    five = C.cells_of(_mono_census("uint16"))
    eight = C.cells_of(C.census_of_tiles(C.tiles_reference("mono", "uint16", C.TILE, 8), 4 * C.FRAME, names))
    added = sorted((c for c in eight if c not in five), key=str)
    print("\nlevel 8 adds:", ", ".join(f"{' '.join(str(v) for v in c)} ({eight[c]})" for c in added))
    assert eight
