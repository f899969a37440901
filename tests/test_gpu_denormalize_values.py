"""The de-normalisation on the GPU at every PCM value, on every decode path, against numpy itself.

csrc/frs_denormalize.h holds the arithmetic once (tests/test_denormalize_host.py ties it to numpy on the CPU); this
module pins that each device site computes it, for every output dtype, both store alignments and each stream's own
(range, min) pair.  Streams come from tests/denorm_cases.py: a cover stream holds all 65 536 PCM values, and a blob is
that stream's bytes once per case of a dtype, each copy with its own data_min / data_max.  Every comparison is exact,
with numpy's expression (D.table) and not the oracle; a failure names the first differing (case, stream, sample index,
pcm, got, want).

Which site a test reaches:
  mono, pipe         the optimistic decode's per-group stores (dn1) and its 8-sample stores (dfast) on the aligned
                     variant; the per-sample stores (dn_store) on the odd one and for wide / float dtypes
  mono, pipe_chain   the same kernel after the span check and the chain
  mono, lane         the staged 1- / 2-byte stores (dn_bits_t), kOutAny's dn_store for wide / float dtypes
  mono, wave         dn_store from the int32 scratch
  multi, lane        k_interleave_dn: packed 8-byte stores (4 x 16 bits), packed 4-byte stores (2 channels), dn_store
                     per sample (3 channels, uint8, wide and float dtypes)
  32-bit, wave       dn_store with shift 16
  unfused            k_denormalize
Reverting a site to a contracted multiply-add or to round-half-away fails here: over these very cases the first
changes 433 (int16) / 233 (uint16) values and the second 9 / 76 181 / 76 814 (uint8 / int16 / uint16), as
tests/test_denormalize_host.py measures, and every test below decodes every PCM value with every case.
"""
import numpy as np
import pytest

from tests import denorm_cases as D
from tests.test_gpu_decode import DECODERS

pytestmark = pytest.mark.gpu

NAMES = ("decode_span", "decode_frames", "decode_fallback", "lane_fallback_frames")
SWITCHES = ("FRS_FORCE_GENERIC", "FRS_DECODE_LANE", "FRS_PIPE_OPT", "FRS_SPAN_READ")


@pytest.fixture(scope="module")
def decoders():
    """kind -> a context created under that kind's switches (they are read when a context is created)"""
    from flac_raster_amd import _native
    out = {}
    for kind, env in DECODERS.items():
        with pytest.MonkeyPatch.context() as mp:
            for k in SWITCHES:
                mp.delenv(k, raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            out[kind] = _native.Context(0)
    yield out
    for ctx in out.values():
        ctx.close()


def _profiled(ctx, call):
    """(call's result, the set of profile names that ran)"""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = call()
        ran = {n for n in NAMES if ctx.profile_avg_ms(n) >= 0}
    finally:
        ctx.profile(False)
    return out, ran


def _decode_cases(ctx, stream, cases, dtype):
    """the stream's bytes once per case, decoded and de-normalised in one call -> ([case, sample * channel], ran)"""
    blob = np.frombuffer(stream.data * len(cases), dtype=np.uint8)
    off = (np.arange(len(cases) + 1) * len(stream.data)).tolist()
    vals, ran = _profiled(ctx, lambda: ctx.decode_tiles_host(
        blob, off, [len(stream.pcm)] * len(cases), channels=stream.channels, bps=stream.bps,
        data_min=[float(c[1]) for c in cases], data_max=[float(c[2]) for c in cases], dtype=np.dtype(dtype),
        blocksize=stream.blocksize))
    assert vals.dtype == np.dtype(dtype) and vals.shape == (len(cases) * len(stream.pcm), stream.channels)
    return vals.reshape(len(cases), -1), ran


def _assert_cases(label, got, cases, pcm, shift=0):
    """got[s] == numpy's value of every sample of `pcm` (flattened, interleaved) under case s"""
    flat = np.asarray(pcm).reshape(-1)
    idx = (flat >> shift) + 32768
    for s, c in enumerate(cases):
        want = D.table(c)[idx]
        bad = np.flatnonzero(got[s] != want)
        assert bad.size == 0, (label, c, "stream", s, "sample", int(bad[0]), "pcm", int(flat[bad[0]]), "got",
                               got[s][bad[0]], "want", want[bad[0]], "differing", bad.size)


def _assert_route(kind, ran):
    if kind == "pipe":       # the optimistic decode alone: its early per-group stores are what was compared
        assert "decode_frames" in ran and not ran & {"decode_span", "decode_fallback", "lane_fallback_frames"}, ran
    elif kind == "pipe_chain":
        assert {"decode_span", "decode_frames"} <= ran and not ran & {"decode_fallback", "lane_fallback_frames"}, ran
    elif kind == "lane":
        assert {"decode_span", "decode_frames", "lane_fallback_frames"} <= ran and "decode_fallback" not in ran, ran
    else:
        assert {"decode_span", "decode_frames"} <= ran and not ran & {"decode_fallback", "lane_fallback_frames"}, ran


@pytest.mark.parametrize("variant", ["odd", "aligned"])
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("kind", list(DECODERS))
def test_mono_every_pcm_value(decoders, kind, dtype, variant):
    """Mono 16-bit cover stream, one copy per case of the dtype.  odd: 81 925 samples per copy, so the copies' output
    bases run through every residue mod 8 and a frame's last block is 5 samples; aligned: every frame takes the
    8-sample stores where the decoder has them."""
    stream = D.mono_cover(variant == "odd")
    cases = D.cases_of(dtype)
    got, ran = _decode_cases(decoders[kind], stream, cases, dtype)
    _assert_route(kind, ran)
    _assert_cases((kind, dtype, variant), got, cases, stream.pcm)


@pytest.mark.parametrize("layout", D.MULTI_LAYOUTS, ids=lambda l: f"{l[0]}ch_chass{l[1]}")
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("kind", ["lane", "wave"])
def test_multichannel_every_pcm_value(decoders, kind, dtype, layout):
    """2 (independent and mid/side), 3 and 4 channels of 256 frames, every channel holding every PCM value."""
    stream = D.multi_cover(*layout)
    cases = D.cases_of(dtype)
    got, ran = _decode_cases(decoders[kind], stream, cases, dtype)
    _assert_route(kind, ran)
    _assert_cases((kind, dtype, layout), got, cases, stream.pcm)


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_32_bit_stream_every_high_half(decoders, dtype):
    """32-bit samples keep their high half (pcm >> 16) through the WAV round trip, whatever the low half holds."""
    stream = D.mono32_cover()
    cases = D.cases_of(dtype)
    got, ran = _decode_cases(decoders["wave"], stream, cases, dtype)
    _assert_route("wave", ran)
    _assert_cases(("wave32", dtype), got, cases, stream.pcm, shift=16)


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_unfused_every_pcm_value(gpu_ctx, dtype):
    """frs_denormalize on all 65 536 values, and on the 32-bit cover samples with pcm_bps=32."""
    wide = D.mono32_cover().pcm[:, 0]
    for c in D.cases_of(dtype):
        got = gpu_ctx.denormalize_host(D.ALL_P16, float(c[1]), float(c[2]), np.dtype(dtype))
        _assert_cases(("unfused", dtype), got[None, :], [c], D.ALL_P16)
        got = gpu_ctx.denormalize_host(wide.astype(np.int32), float(c[1]), float(c[2]), np.dtype(dtype), pcm_bps=32)
        _assert_cases(("unfused32", dtype), got[None, :], [c], wide, shift=16)


@pytest.mark.parametrize("kind", list(DECODERS))
def test_cover_streams_decode_to_their_samples(decoders, kind):
    """Frames only: the cover streams themselves, against the samples that went into them."""
    ctx = decoders[kind]
    streams = [D.mono_cover(True), D.mono_cover(False)]
    if kind in ("lane", "wave"):
        streams += [D.multi_cover(*l) for l in D.MULTI_LAYOUTS]
    if kind == "wave":
        streams.append(D.mono32_cover())
    for s in streams:
        blob = np.frombuffer(s.data * 3, dtype=np.uint8)                     # three copies: more than one stream
        off = (np.arange(4) * len(s.data)).tolist()
        pcm, ran = _profiled(ctx, lambda: ctx.decode_frames_host(blob, off, [len(s.pcm)] * 3, channels=s.channels,
                                                                 bps=s.bps, blocksize=s.blocksize))
        if s.channels == 1 and s.bps == 16:
            _assert_route(kind, ran)
        assert np.array_equal(pcm.reshape(3, -1), np.tile(s.pcm.reshape(-1), (3, 1))), (kind, s.name)
