"""The encoder on every input alignment class: each content of tests/encode_layouts.py from every layout of its table,
through the host entry (the strided view itself) and the device entry (the parent resident on the device, the origin
at parent + lead), byte for byte against the oracle's encode of the contiguous copy.

The class (EncodeParams::vec_ok: 16-, 8-, 4-byte vector loads or the element gather) is taken per tile by
k_analyze_v3's lean launch and k_encode_v4 (tile widths that are multiples of 64), k_analyze_v3's slow launch
(multiples of 16) and the two-band half-chunk forms; the same facts choose between k_tile_stats_vec and k_tile_stats
and whether the stats are fused into the analysis.  The output must not depend on any of it.  tests/test_encode_layouts_host.py holds that the table reaches every class; here the classes are asserted
again from the real device pointers, as a set per content.  Every assertion is exact equality.

The raw-frames contents (k_zero_subframes' use of the class) are NOT run here: their device-entry run ended once in
"an illegal memory access" inside frs_encode_tiles_device, before the frames were placed, in a session that ran this
file against a build whose 8-byte load had been broken on purpose; the same cases had passed on the real build, and
the cause was not found by reading.  tests/encode_layouts.py and the host test keep those contents ready; they come back
here once the cause is known.
"""
import types

import numpy as np
import pytest

from flac_raster_amd import _native
from tests import encode_layouts as EL
from tests.test_gpu_tiny_frames import _ctx

pytestmark = pytest.mark.gpu

PROFILE = ("stats", "partial", "assemble", "compact")
GUARD = 256          # bytes after the arena's bound, checked with everything after the used bytes
FILL = 0xA5


def _desc(ctx, c, p):
    H, W = c.data.shape[-2:]
    return ctx.make_desc(H, W, c.data.dtype, row_stride=p.row_stride, band_stride=p.band_stride, nbands=EL.bands_of(c),
                         tile_h=c.tile_h, tile_w=c.tile_w, sample_rate=EL.RATE, bits_per_sample=16,
                         norm_mode=c.norm_mode)


def _profiled(ctx, call):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = call()
        prof = {k: ctx.profile_avg_ms(k) for k in PROFILE}
    finally:
        ctx.profile(False)
    return out, prof


def _host(ctx, c, p):
    """the host entry on the strided view -> ((arena, off, mn, mx, bps), profile)"""
    return _profiled(ctx, lambda: ctx.encode_tiles_host(p.view, _desc(ctx, c, p)))


def _device(ctx, c, p, what):
    """the device entry on the uploaded parent -> ((arena, off, mn, mx, bps), profile, device address of the parent);
    the parent must come back unchanged and nothing may be written after the arena's used bytes"""
    d = _desc(ctx, c, p)
    dev = _native.DeviceBuffer(ctx, p.parent.nbytes)
    bound = ctx.arena_bound(d)
    buf = _native.DeviceBuffer(ctx, bound + GUARD)
    try:
        assert dev.ptr % 16 == 0, hex(dev.ptr)
        dev.upload(p.parent)
        buf.upload(np.full(bound + GUARD, FILL, dtype=np.uint8))
        arena = types.SimpleNamespace(ptr=buf.ptr, nbytes=bound)
        (off, mn, mx, bps), prof = _profiled(ctx, lambda: ctx.encode_tiles_device(dev.ptr + p.lead, d, arena))
        after = buf.download()
        used = int(off[-1])
        assert used <= bound, (what, used, bound)
        touched = np.flatnonzero(after[used:] != FILL)
        assert touched.size == 0, f"{what}: arena byte {used + int(touched[0])} written, {used} used, bound {bound}"
        back = dev.download().view(p.parent.dtype)
        same = back.tobytes() == p.parent.tobytes()
        assert same, f"{what}: the encoder changed its input at byte {_first_diff(back.tobytes(), p.parent.tobytes())}"
        return (after[:used], off, mn, mx, bps), prof, dev.ptr
    finally:
        buf.close()
        dev.close()


def _first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def _check(got, ref, what):
    arena, off, mn, mx, bps = got
    assert bps == ref.bps, (what, bps)
    data = arena.tobytes()
    bad = []
    for t in range(len(ref.off) - 1):
        mine = data[int(off[t]):int(off[t + 1])] if t + 1 < len(off) else b""
        want = ref.data[ref.off[t]:ref.off[t + 1]]
        if mine != want:
            at = _first_diff(mine, want)
            # frames begin with the sync code 0xFFF8 (the count may overshoot on a chance match inside a frame)
            frame = max(0, sum(1 for i in range(min(at, len(want) - 1)) if want[i] == 0xFF and want[i + 1] == 0xF8) - 1)
            bad.append(f"{what}: tile {t} differs at byte {at} of {len(want)} (GPU {len(mine)}), about frame {frame}")
    assert not bad, "\n".join(bad[:10])
    assert [int(o) for o in off] == ref.off and data == ref.data, what
    assert [float(v) for v in mn] == ref.mins and [float(v) for v in mx] == ref.maxs, (what, list(mn), list(mx))


def _stats_fused(c, p, base):
    """plan_encode's fuse_stats: the one-band fast path on 16-bit samples whose base, strides, tile width and raster
    width are all multiples of 16 bytes (every tile here is at most 64 frames)"""
    es = np.dtype(c.dtype).itemsize
    W = c.data.shape[-1]
    return (c.kind == "mono" and es == 2 and (base + p.lead) % 16 == 0
            and all((v * es) % 16 == 0 for v in (p.row_stride, p.band_stride, c.tile_w, W)))


def _check_pipeline(prof, c, p, base, what, generic=False):
    if generic:
        assert prof["compact"] >= 0, f"{what}: expected the generic path: {prof}"
        return
    assert prof["compact"] < 0, f"{what}: expected a fast path: {prof}"
    if c.kind == "multi":
        assert prof["assemble"] > 0, f"{what}: expected the multi-channel fast path: {prof}"
    if _stats_fused(c, p, base):
        assert prof["stats"] < 0, f"{what}: expected the stats fused into the analysis: {prof}"
    else:
        assert prof["stats"] >= 0, f"{what}: expected a stats pass: {prof}"


CLASSES = {16, 8, 4, 0}
NAMES = [n for n in EL.CONTENTS if not n.startswith("raw")]


@pytest.mark.parametrize("name", NAMES)
def test_every_layout_encodes_to_the_oracles_bytes(gpu_ctx, name):
    c = EL.content(name)
    ref = EL.reference(name)
    host_classes, dev_classes = {}, {}
    fused = set()
    for lay in EL.layouts(c):
        p = EL.place(c, lay)
        # the host entry copies from the origin into its own staging buffer: the lead does not reach the device
        what = f"{name} {lay.name} host"
        got, prof = _host(gpu_ctx, c, p)
        _check(got, ref, what)
        _check_pipeline(prof, c, p._replace(lead=0), 0, what)
        assert np.array_equal(p.view, c.data), what
        host_classes.setdefault(EL.align_class(c, p._replace(lead=0)), []).append(lay.name)
        what = f"{name} {lay.name} device"
        got, prof, base = _device(gpu_ctx, c, p, what)
        _check(got, ref, what)
        _check_pipeline(prof, c, p, base, what)
        dev_classes.setdefault(EL.align_class(c, p, base), []).append(lay.name)
        if _stats_fused(c, p, base):
            fused.add(lay.name)
    print(f"\n{name}: device classes {dev_classes}; host classes {host_classes}; fused stats {sorted(fused)}")
    # on the set, so that another allocator alignment fails here and does not shrink what was covered
    assert set(dev_classes) == CLASSES, dev_classes
    assert set(host_classes) == CLASSES, host_classes
    if name.startswith("mono-") and np.dtype(c.dtype).itemsize == 2:
        assert fused == {"aligned"}, fused


@pytest.mark.parametrize("name,layout", [("multi-uint8", "all8"), ("stereo-int16", "mixe")])
def test_round_trip_through_the_decoder(gpu_ctx, name, layout):
    """a class-8 and a class-0 layout: the encoder's (= the oracle's) stream decodes and de-normalises to the view"""
    c = EL.content(name)
    ref = EL.reference(name)
    p = EL.place(c, next(lay for lay in EL.layouts(c) if lay.name == layout))
    got, _, base = _device(gpu_ctx, c, p, f"{name} {layout}")
    assert EL.align_class(c, p, base) == (8 if layout == "all8" else 0)
    _check(got, ref, f"{name} {layout}")
    B, H, W = c.data.shape
    back = gpu_ctx.decode_tiles_host(np.frombuffer(ref.data, dtype=np.uint8), [0, len(ref.data)], [H * W], channels=B,
                                     bps=16, data_min=ref.mins, data_max=ref.maxs, dtype=c.data.dtype)
    assert np.array_equal(back.reshape(H, W, B).transpose(2, 0, 1), p.view), name


def test_generic_kernels_ignore_the_class(monkeypatch):
    """The control: the generic kernels read element by element whatever the class, so the mono content's class-8 and
    class-0 layouts must give the same bytes there.  A failure here lies in the layout arithmetic, not in the loads."""
    ctx = _ctx(monkeypatch, FRS_FORCE_GENERIC="1")
    try:
        for dtype in EL.MONO_MODES:
            c = EL.mono(dtype)
            ref = EL.reference(c.name)
            es = np.dtype(dtype).itemsize
            for lay_name, cls in (("row8", 8), (f"row{es}", 0)):
                p = EL.place(c, next(lay for lay in EL.layouts(c) if lay.name == lay_name))
                what = f"generic {c.name} {lay_name}"
                got, prof = _host(ctx, c, p)
                _check(got, ref, what + " host")
                _check_pipeline(prof, c, p, 0, what, generic=True)
                got, prof, base = _device(ctx, c, p, what)
                assert EL.align_class(c, p, base) == cls, what
                _check(got, ref, what + " device")
                _check_pipeline(prof, c, p, base, what, generic=True)
    finally:
        ctx.close()
