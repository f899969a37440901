"""Which stages a decode runs (plan_decode_route, csrc/frs_decode_plan.h), read from the profile, at the thresholds
between the frame decoders and on the optimistic decode's decline; every decode is compared with the oracle.

A profile name is present (profile_avg_ms >= 0) when its stage ran: "decode_span" the span check and the chain,
"decode_frames" the frame decoder, "decode_fallback" the frame decoder after a declined optimistic decode, and
"lane_fallback_frames" whenever a lane decoder ran.  Streams come from tests/flac_builder.py; where the frame count
matters the block size is 64.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flac_builder as B

pytestmark = pytest.mark.gpu

NAMES = ("decode", "decode_span", "decode_frames", "decode_fallback", "lane_fallback_frames")
FIXED2 = B.Sub("fixed", order=2, params=None)
SWITCHES = ("FRS_FORCE_GENERIC", "FRS_DECODE_LANE", "FRS_PIPE_OPT", "FRS_SPAN_READ")


def _ctx(monkeypatch, **env):
    from flac_raster_amd import _native
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _native.Context(0)


def _decode(ctx, blob: bytes, stream_off, counts, channels, blocksize):
    """(samples, the set of profile names that ran)"""
    ctx.profile(True)
    ctx.profile_reset()
    pcm = ctx.decode_frames_host(np.frombuffer(blob, dtype=np.uint8), stream_off, counts, channels=channels, bps=16,
                                 blocksize=blocksize)
    ran = {n for n in NAMES if ctx.profile_avg_ms(n) >= 0}
    ctx.profile(False)
    return pcm.reshape(-1, channels), ran


def _oracle(blob: bytes, stream_off, counts, channels):
    return np.concatenate([O.decode_frames(blob[a:b], channels, 16, n)
                           for a, b, n in zip(stream_off[:-1], stream_off[1:], counts)])


def _smooth(n, channels=1, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] + 977 * np.arange(channels)[None, :]
    return (6000 * np.sin(t * 0.013) + 900 * np.sin(t * 0.21) + rng.integers(-6, 7, size=t.shape)).astype(np.int64)


def _spelled_header(bs_code_byte: int, code_byte: int) -> np.ndarray:
    """4096 random 16-bit samples whose first three, as a VERBATIM subframe's big-endian bytes, are a complete frame
    header: FF F8, the stream's code bytes, frame number 0 and its CRC-8."""
    hdr = bytes([0xFF, 0xF8, bs_code_byte, code_byte, 0x00])
    hdr += bytes([B.crc8(hdr)])
    x = np.random.default_rng(11).integers(-30000, 30000, size=4096).astype(np.int64)
    x[:3] = np.frombuffer(hdr, dtype=">i2")
    return x


@pytest.fixture(scope="module")
def mono_two_streams():
    """Two streams of three 4096-sample frames: (plain, with a spelled header in stream 1's middle frame)."""
    pcm = _smooth(2 * 3 * 4096).reshape(2, 3 * 4096)
    plain = [B.stream(p, 16, 4096, lambda f, blk: [FIXED2]).data for p in pcm]
    first = plain[0][:4]
    assert first[:2] == b"\xff\xf8"
    trap_pcm = pcm[1].copy()
    trap_pcm[4096:8192] = _spelled_header(first[2], first[3])
    trap = B.stream(trap_pcm, 16, 4096, lambda f, blk: [B.Sub("verbatim") if f == 1 else FIXED2]).data
    # the subframe header is one byte, so the samples are byte-aligned: the header's bytes are in the stream
    hdr = trap_pcm[4096:4099].astype(">i2").tobytes()
    assert trap.count(hdr) == 2 and trap.startswith(hdr)  # (frame 0 has the same header)

    def pack(streams):
        off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).tolist()
        return b"".join(streams), off, [3 * 4096] * 2
    return pack(plain), pack([plain[0], trap])


@pytest.fixture(scope="module")
def short_frames():
    """channels -> (the frames of one stream at block size 64, their end offsets): 4096 mono, 64 of three channels."""
    out = {}
    for channels, nframes in ((1, 4096), (3, 64)):
        pcm = _smooth(nframes * 64, channels)
        frames = [B.frame([pcm[64 * f:64 * f + 64, c] for c in range(channels)], [FIXED2] * channels, f, 16)
                  for f in range(nframes)]
        out[channels] = (b"".join(frames), np.cumsum([len(f) for f in frames]).tolist())
    return out


def test_default_route_is_the_optimistic_decode(mono_two_streams, monkeypatch):
    (blob, off, counts), _ = mono_two_streams
    want = _oracle(blob, off, counts, 1)
    ctx = _ctx(monkeypatch)
    try:
        pcm, ran = _decode(ctx, blob, off, counts, 1, 4096)
    finally:
        ctx.close()
    assert np.array_equal(pcm, want)
    assert "decode_frames" in ran and not ran & {"decode_span", "decode_fallback", "lane_fallback_frames"}, ran
    ctx = _ctx(monkeypatch, FRS_PIPE_OPT="0")
    try:
        pcm, ran = _decode(ctx, blob, off, counts, 1, 4096)
    finally:
        ctx.close()
    assert np.array_equal(pcm, want)
    assert {"decode_span", "decode_frames"} <= ran and "decode_fallback" not in ran, ran


def test_optimistic_decode_declines_on_a_false_sync(mono_two_streams, monkeypatch):
    """A complete, CRC-8-correct frame header inside a frame's data is a candidate too many: the optimistic decode
    declines, and the span check, the chain and the decoder run after it."""
    _, (blob, off, counts) = mono_two_streams
    want = _oracle(blob, off, counts, 1)
    ctx = _ctx(monkeypatch)
    try:
        pcm, ran = _decode(ctx, blob, off, counts, 1, 4096)
    finally:
        ctx.close()
    assert np.array_equal(pcm, want)
    assert {"decode_frames", "decode_span", "decode_fallback"} <= ran, ran


@pytest.mark.parametrize("channels,nframes,lane", [(1, 4095, False), (1, 4096, True), (3, 63, False), (3, 64, True)])
def test_lane_decoder_thresholds(short_frames, monkeypatch, channels, nframes, lane):
    """Mono: the lane-per-frame decoder from 4096 frames; three channels: the lane walk + k_interleave_dn from 64
    frames (below: the pipelined / the wave decoder)."""
    frames, ends = short_frames[channels]
    blob, off, counts = frames[:ends[nframes - 1]], [0, ends[nframes - 1]], [nframes * 64]
    want = _oracle(blob, off, counts, channels)
    assert len(want) == nframes * 64
    ctx = _ctx(monkeypatch)
    try:
        pcm, ran = _decode(ctx, blob, off, counts, channels, 64)
    finally:
        ctx.close()
    assert np.array_equal(pcm, want)
    assert ("lane_fallback_frames" in ran) == lane, ran
    assert ("decode_span" in ran) == (lane or channels == 3), ran  # (mono below the threshold: optimistic)


def test_generic_route(mono_two_streams, monkeypatch):
    (blob, off, counts), _ = mono_two_streams
    ctx = _ctx(monkeypatch, FRS_FORCE_GENERIC="1")
    try:
        pcm, ran = _decode(ctx, blob, off, counts, 1, 4096)
    finally:
        ctx.close()
    assert np.array_equal(pcm, _oracle(blob, off, counts, 1))
    assert {"decode_span", "decode_frames"} <= ran and not ran & {"lane_fallback_frames", "decode_fallback"}, ran
