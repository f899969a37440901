"""What tests/test_gpu_encode_layouts.py relies on, checked on the CPU: the layout table of tests/encode_layouts.py
reaches every alignment class for every content and dtype (and, for several bands, once through the band stride alone),
the parents' padding is made of sentinels outside the data, the oracle's streams of the contents decode back to the
oracle's PCM, and the mono content has a tile of every normalisation mode in both of its columns."""
import numpy as np
import pytest

from flac_raster_amd import _native
from oracle import oracle as O
from tests import encode_layouts as EL

NAMES = list(EL.CONTENTS)


def _classes_wanted(c):
    # 4-byte elements: every address and stride is a multiple of 4, so the gather class does not exist for them
    return {16, 8, 4} if np.dtype(c.dtype).itemsize == 4 else {16, 8, 4, 0}


def test_align_class_mirror():
    f = _native.encode_align_class
    assert f(256, 2, 10984, 0, 1024, 1) == 16
    assert f(256, 2, 10980, 0, 1024, 1) == 8          # the dense Sentinel-2 row: 21960 bytes
    assert f(256, 2, 10982, 0, 1024, 1) == 4
    assert f(256, 2, 10981, 0, 1024, 1) == 0
    assert f(264, 1, 64, 0, 64, 1) == 8 and f(260, 1, 64, 0, 64, 1) == 4 and f(257, 1, 64, 0, 64, 1) == 0
    assert f(256, 1, 64, 5, 64, 1) == 16              # one band: its base is all the band stride decides
    assert f(256, 1, 64, 64 * 256 + 5, 64, 3) == 0    # three uint8 bands 5 bytes off: the other bands' bases
    assert f(256, 1, 64, 64 * 256 + 8, 64, 3) == 8 and f(256, 1, 64, 64 * 256 + 4, 64, 2) == 4
    assert f(256, 2, 64, 0, 8, 1) == 16 and f(256, 2, 64, 0, 4, 1) == 8 and f(256, 1, 64, 0, 4, 1) == 4


@pytest.mark.parametrize("name", NAMES)
def test_layouts_reach_every_class(name):
    """with the parent 256-byte aligned (the device allocator's alignment; the GPU test asserts on the real pointer)"""
    c = EL.content(name)
    got = {}
    for lay in EL.layouts(c):
        got.setdefault(EL.align_class(c, EL.place(c, lay), 256), []).append(lay.name)
    assert set(got) == _classes_wanted(c), got
    assert got[16] == ["aligned"], got
    if EL.bands_of(c) > 1:
        # the band stride alone lowers the class, to each of the lower classes
        only_band = {EL.align_class(c, EL.place(c, lay), 256) for lay in EL.layouts(c)
                     if lay.lead == 0 and lay.row_res == 0 and lay.band_res != 0}
        assert only_band == _classes_wanted(c) - {16}, only_band


@pytest.mark.parametrize("name", NAMES)
def test_views_and_sentinels(name):
    c = EL.content(name)
    lo, hi = EL.sentinels(c.dtype)
    es = np.dtype(c.dtype).itemsize
    for lay in EL.layouts(c):
        p = EL.place(c, lay)
        assert np.array_equal(p.view, c.data) and np.array_equal(np.ascontiguousarray(p.view), c.data), lay
        assert p.view.strides[-2] == p.row_stride * es >= c.data.shape[-1] * es, lay
        assert (p.row_stride * es) % 16 == lay.row_res, lay
        if EL.bands_of(c) > 1:
            assert p.view.strides[0] == p.band_stride * es and (p.band_stride * es) % 16 == lay.band_res, lay
            assert p.band_stride >= p.row_stride * c.data.shape[-2], lay
        assert p.view.__array_interface__["data"][0] - p.parent.__array_interface__["data"][0] == lay.lead, lay
        inside = EL.view_mask(c, p)
        assert int(inside.sum()) == c.data.size, lay
        outside = p.parent[~inside]
        assert outside.size >= 16 // es and np.isin(outside, [lo, hi]).all(), lay      # (at least the tail)
        at = np.flatnonzero(~inside)
        assert np.array_equal(outside, np.where(at % 2 == 0, lo, hi)), lay
        if lay.lead:
            assert not inside[: lay.lead // es].any(), lay
    if c.inside:
        assert lo < c.data.min() and c.data.max() < hi, (c.data.min(), c.data.max())
    else:
        r0, c0, h, w = EL.tile_boxes(c)[0]       # raw uint8: its all-zero tile still lies strictly inside
        first = c.data[..., r0:r0 + h, c0:c0 + w]
        assert lo < first.min() and first.max() < hi


@pytest.mark.parametrize("name", NAMES)
def test_oracle_streams_decode_to_oracle_pcm(name):
    c = EL.content(name)
    ref = EL.reference(name)
    B = EL.bands_of(c)
    pcm = EL.reference_pcm(name)
    assert len(pcm) == len(ref.off) - 1 == len(EL.tile_boxes(c))
    for t, want in enumerate(pcm):
        got = O.decode_frames(ref.data[ref.off[t]:ref.off[t + 1]], B, ref.bps, len(want))
        assert np.array_equal(got, want.reshape(-1, B)), (name, t)
    assert EL.reference(name) is ref               # computed once


def _mode(tile):
    """frs_normalize.h norm_mode_of for 16-bit streams: the range R = max - min decides, and whether it wraps in the
    dtype (R beyond the dtype's largest value)"""
    mn, mx = int(tile.min()), int(tile.max())
    R = mx - mn
    nowrap = R <= int(np.iinfo(tile.dtype).max)
    if R == 0:
        return EL.ZERO
    if nowrap and R + 1 <= 4096:
        return EL.LUT
    if nowrap and R <= 65535:
        return EL.FASTDIV
    return EL.SLOW


@pytest.mark.parametrize("dtype", list(EL.MONO_MODES))
def test_mono_tiles_have_every_mode_in_both_columns(dtype):
    c = EL.mono(dtype)
    boxes = EL.tile_boxes(c)
    assert sorted({w for _, _, _, w in boxes}) == [80, 128]
    assert all(h * w >= EL.FRAME for _, _, h, w in boxes) and (128 * 80) % EL.FRAME == 2048
    want = {EL.LUT, EL.ZERO} if dtype == "uint8" else {EL.LUT, EL.FASTDIV, EL.ZERO}
    if dtype == "int16":
        want |= {EL.SLOW}
    flat = [m for row in EL.MONO_MODES[dtype] for m in row]
    for width in (128, 80):
        seen = set()
        for (r0, c0, h, w), planned in zip(boxes, flat):
            if w == width:
                got = _mode(c.data[r0:r0 + h, c0:c0 + w])
                assert got == planned, (dtype, r0, c0, EL.MODE_NAMES[got], EL.MODE_NAMES[planned])
                seen.add(got)
        assert seen == want, (dtype, width, seen)


def test_other_contents_are_what_they_claim():
    s2 = EL.s2row()
    assert s2.data.shape[1] * 2 == 21960 and 21960 % 16 == 8      # dense rows: class 8
    boxes = EL.tile_boxes(s2)
    assert len(boxes) == 11 and boxes[-1][3] == 740
    assert all(_mode(s2.data[r:r + h, x:x + w]) == EL.LUT for r, x, h, w in boxes)
    for name in NAMES:
        c = EL.content(name)
        if c.kind == "raw":                        # the first tile's frames are all-zero, the second's are not
            zero, mixed = EL.reference_pcm(name)
            assert not zero.any() and mixed.any(), name
            if EL.bands_of(c) == 3:
                assert not mixed[:, 1].any() and mixed[:, 0].any() and mixed[:, 2].any(), name
        if c.kind == "stereo":                     # more than one channel assignment occurs
            ref = EL.reference(name)
            ca = O.frame_assignments(ref.data, 2, 16, c.data[0].size)
            assert len(set(ca.tolist())) >= 3, (name, ca.tolist())
