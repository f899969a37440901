"""The preconditions of tests/test_gpu_tiny_frames.py, checked with the oracle alone: the inputs of tests/tiny_frames.py
really produce the frames the GPU tests are about (VERBATIM at n <= 4, CONSTANT from 5, FIXED with partitions and LPC in
frames of at most 64 samples, level 8 parting from level 5, every block-size code form, every channel assignment), so
those tests cannot lose their subject unnoticed."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import pipeline as P
from tests import tiny_frames as TF
from tests.pyramid_ref import np_pyramid

DTYPES = (np.int16, np.uint16, np.uint8)
CONSTANT_ROW = TF.KINDS.index("constant")


def _types(frames, channels, bps, n):
    """subframe (type, partition order) rows of a one-frame stream"""
    sf = O.subframe_types(frames, channels, bps, n)
    assert len(sf) == channels
    return sf


@pytest.mark.parametrize("bands,dtype", [(1, np.int16), (1, np.uint16), (1, np.uint8), (1, np.int32), (2, np.int16),
                                         (3, np.int16)])
def test_every_oracle_stream_decodes_to_the_normalised_samples(bands, dtype):
    for form in TF.FORMS:
        for n in TF.LENGTHS:
            for lv in (TF.LEVELS if (bands, np.dtype(dtype)) == (1, np.dtype(np.int16)) else (5,)):
                for r, (pcm, mn, mx, bps, fr) in enumerate(TF.reference(bands, form, n, dtype, lv)):
                    assert np.array_equal(O.decode_frames(fr, bands, bps, len(pcm)), pcm), (form, n, lv, r)
    for n in TF.LENGTHS:  # loose mid/side
        for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(2, "tail", n, np.int16, 1)):
            assert np.array_equal(O.decode_frames(fr, 2, bps, len(pcm)), pcm), (n, r)


@pytest.mark.parametrize("bands", [1, 2, 3])
def test_spatial_streams_decode_and_most_frames_are_all_zero(bands):
    zero = total = 0
    for form in TF.FORMS:
        for n in TF.LENGTHS:
            for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(bands, form, n, np.int16, 5, True)):
                assert bps == 32 and set(np.unique(pcm)) <= {-1, 0, 1}
                assert np.array_equal(O.decode_frames(fr, bands, 32, len(pcm)), pcm), (form, n, r)
                if form == "single":
                    total += 1
                    zero += not pcm.any()
                    t = _types(fr, bands, 32, n)[:, 0]
                    if not pcm.any():
                        # the zero-frame route: VERBATIM zeros up to 4 samples; above, FIXED order 0 (an all-zero
                        # block of a 32-bit stream is not CONSTANT: fixed_best_limit_residual in oracle/flac_oracle.c)
                        assert (t == (1 if n <= 4 else 8)).all(), (n, r, t)
    assert zero * 2 > total
    assert zero < total


def test_up_to_four_samples_every_subframe_is_verbatim():
    for dtype in DTYPES + (np.int32,):
        for n in (1, 2, 3, 4):
            for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(1, "single", n, dtype)):
                assert (_types(fr, 1, bps, n)[:, 0] == 1).all(), (dtype, n, r)
            # the tail of a two-frame stream
            for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(1, "tail", n, dtype)):
                sf = O.subframe_types(fr, 1, bps, TF.FULL + n)
                assert len(sf) == 2 and sf[1, 0] == 1, (dtype, n, r)
    for bands in (2, 3):
        for n in (1, 2, 3, 4):
            for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(bands, "single", n)):
                assert (_types(fr, bands, bps, n)[:, 0] == 1).all(), (bands, n, r)
    # the constant row, by itself: all-zero samples, VERBATIM all the same
    for n in (1, 2, 3, 4):
        pcm, _, _, bps, fr = TF.reference(1, "single", n)[CONSTANT_ROW]
        assert not pcm.any() and _types(fr, 1, bps, n)[0, 0] == 1
        assert len(fr) == 4 + 1 + 1 + 1 + 1 + 2 * n + 2   # codes, frame number, block size, CRC-8, subframe header


def test_constant_from_five_samples():
    for n in TF.LENGTHS:
        if n >= 5:
            pcm, _, _, bps, fr = TF.reference(1, "single", n)[CONSTANT_ROW]
            assert _types(fr, 1, bps, n)[0, 0] == 0, n
    assert any(0 in _types(fr, 3, bps, 5)[:, 0] for _, _, _, bps, fr in TF.reference(3, "single", 5))


def test_short_frames_reach_fixed_with_partitions_and_lpc():
    fixed_po, lpc_orders = set(), set()
    for n in TF.LENGTHS:
        if n <= 64:
            for _, _, _, bps, fr in TF.reference(1, "single", n):
                t, po = _types(fr, 1, bps, n)[0]
                if 8 <= t <= 12 and po >= 1:
                    fixed_po.add((n, int(po)))
                if t >= 32:
                    lpc_orders.add((n, int(t) - 31))
    assert fixed_po, "no FIXED subframe with partition order >= 1 at n <= 64"
    assert lpc_orders, "no LPC subframe at n <= 64"
    # partition order ctz(n): the most a block of 16 / 32 / 64 samples allows at a predictor order below n >> order
    assert any(po >= 3 for _, po in fixed_po), fixed_po


def test_level_8_equals_level_5_up_to_32_samples_and_parts_from_it_by_96():
    differs = []
    for n in TF.LENGTHS:
        if n > 96:
            break
        a = [t[4] for t in TF.reference(1, "single", n, np.int16, 5)]
        b = [t[4] for t in TF.reference(1, "single", n, np.int16, 8)]
        if n <= 32:
            assert a == b, n
        elif a != b:
            differs.append(n)
    assert differs


def test_block_size_codes_of_first_frames_and_tails():
    seen = {"single": set(), "tail": set()}
    hdr_len = {}
    for form in TF.FORMS:
        for n in TF.LENGTHS:
            for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(1, form, n)):
                bsc, ca, hl = TF.header_fields(fr)
                if form == "tail":
                    assert bsc == 12
                    # the tail starts where the stream of the first 4096 samples alone ends
                    first = O.encode_frames(pcm[:TF.FULL], bps, TF.RATE)
                    assert fr.startswith(first) and fr[len(first) + 4] == 1   # (frame number 1)
                    bsc, ca, hl = TF.header_fields(fr[len(first):])
                seen[form].add(bsc)
                hdr_len[form, n] = hl
    for form in TF.FORMS:
        assert seen[form] == {6, 7, 1, 8, 2}, (form, seen[form])
        assert hdr_len[form, 192] == hdr_len[form, 256] == 6 and hdr_len[form, 255] == 7 and hdr_len[form, 257] == 8


def test_two_channel_inputs_reach_every_assignment():
    seen = set()
    for form in TF.FORMS:
        for n in TF.LENGTHS:
            for r, (pcm, _, _, bps, fr) in enumerate(TF.reference(2, form, n)):
                ca = O.frame_assignments(fr, 2, bps, len(pcm))
                assert len(ca) == (1 if form == "single" else 2)
                if n <= 4:
                    assert ca[-1] == 1, (form, n, r)
                    assert TF.header_fields(fr)[1] == (1 if form == "single" else ca[0])
                seen |= set(int(c) for c in ca)
    assert seen == {1, 8, 9, 10}, seen


@pytest.mark.parametrize("dtype", DTYPES)
def test_which_tiles_survive_the_references_round_trip(dtype):
    """Recorded, not demanded: the reference's normalise / de-normalise round trip is not lossless everywhere.  The
    GPU tests compare with the source on the tiles listed here and with the oracle everywhere; this keeps the list
    from running empty."""
    kept = total = 0
    for form in TF.FORMS:
        for n in TF.LENGTHS:
            ok = TF.lossless_tiles(form, n, dtype)
            kept += len(ok)
            total += 8
            assert CONSTANT_ROW in ok, (form, n)
    assert kept * 2 > total, (kept, total)


def test_grid_tiles_are_the_edge_tiles_meant():
    assert [(w, h) for _, _, w, h in TF.grid_windows("131x67")] == [(65, 65), (65, 65), (1, 65), (65, 2), (65, 2), (1, 2)]
    assert [(w, h) for _, _, w, h in TF.grid_windows("513x513")] == [(512, 512), (1, 512), (512, 1), (1, 1)]
    for name in TF.GRIDS:
        H, W, T = TF.GRIDS[name]
        band = TF.grid_band(name)
        arena, off, mins, maxs = TF.grid_reference(name)
        raw = P.create_streaming(band, [1.0, 0.0, 0.0, 0.0, -1.0, 0.0], "EPSG:4326", T)
        for t, (c, r, w, h) in enumerate(TF.grid_windows(name)):
            fr = arena[off[t]:off[t + 1]].tobytes()
            assert fr in raw
            tile = np.ascontiguousarray(band[r:r + h, c:c + w]).reshape(-1, 1)
            pcm, mn, mx, bps = O.normalize(tile)
            assert (mn, mx) == (mins[t], maxs[t])
            assert np.array_equal(O.decode_frames(fr, 1, bps, w * h), pcm)
            assert TF.round_trips(band[r:r + h, c:c + w]), (name, t)
    # the 1 x 512 tile: one 512-sample frame with a table block-size code; the 1 x 1 tile: a 12-byte stream
    arena, off, _, _ = TF.grid_reference("513x513")
    assert TF.header_fields(arena[off[1]:off[2]].tobytes())[0] == 9 and TF.header_fields(arena[off[2]:].tobytes())[0] == 9
    assert off[4] - off[3] == 12


def test_file_band_survives_the_round_trip_on_every_level():
    from flac_raster_amd import streaming
    assert streaming.overview_shapes(TF.FILE_H, TF.FILE_W, TF.FILE_TILE) == TF.FILE_SHAPES
    sizes = set()
    for mode in ("average", "nearest"):
        for k, lvl in enumerate(np_pyramid(TF.file_band(), TF.FILE_SHAPES, mode)):
            for c, r, w, h in streaming.tile_grid(lvl.shape[0], lvl.shape[1], TF.FILE_TILE):
                assert TF.round_trips(lvl[r:r + h, c:c + w]), (mode, k, c, r)
                sizes.add((k, w, h))
    assert {(0, 1, 64), (0, 64, 1), (0, 1, 1), (1, 64, 1), (1, 33, 1), (1, 33, 64)} <= sizes


def test_wasted_bits_make_a_three_sample_frame_left_side():
    """Not one of the inputs above (they are independent at n <= 4): all VERBATIM, yet left-side, because the side
    signal's two wasted bits make its 17-bit samples cheaper than the right channel's 16-bit ones."""
    s = TF.tile_samples(TF.wasted_side_pair(), 4)
    pcm, _, _, bps = O.normalize(s)
    fr = O.encode_frames(pcm, bps, TF.RATE)
    assert list(O.frame_assignments(fr, 2, bps, 3)) == [8]
    assert (O.subframe_types(fr, 2, bps, 3)[:, 0] == 1).all()
    assert np.array_equal(O.decode_frames(fr, 2, bps, 3), pcm)


def test_table_lengths_take_their_codes():
    want = {512: 9, 1024: 10, 1152: 3, 2048: 11, 2304: 4}
    for n in TF.TABLE_LENGTHS:
        for bands in (1, 2, 3):
            for pcm, _, _, bps, fr in TF.reference(bands, "single", n):
                assert TF.header_fields(fr)[0] == want[n] and TF.header_fields(fr)[2] == 6
                assert np.array_equal(O.decode_frames(fr, bands, bps, n), pcm)
            for pcm, _, _, bps, fr in TF.reference(bands, "tail", n):
                # the tail's header is the stream's last: sync code, the code nibble, frame number 1, no extra bytes
                want_b2 = (want[n] << 4) | 9
                assert any(fr[p] == 0xFF and fr[p + 1] == 0xF8 and fr[p + 2] == want_b2 and fr[p + 4] == 1
                           for p in range(len(fr) - 6)), (n, bands)
                assert np.array_equal(O.decode_frames(fr, bands, bps, TF.FULL + n), pcm)
