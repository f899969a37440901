"""GPU decoders on hand-built FLAC layouts (tests/flac_layouts.py, written by tests/flac_builder.py).

Most of the decoder code is dispatch: k_decode_frames_pipe (and its chained form), k_decode_frames_lane (mono and
multi-channel) and the wave decoder each take some subframe layouts and decline the rest to the next one.  The
level-5 encoder emits almost none of the layouts those conditions look at (LPC order > 8, escape partitions, 5-bit
Rice parameters, partition orders above 6, precision / bps / order sums on either side of the 32-bit-safe limit,
wasted bits on every subframe type, block sizes other than 4096, headers with extra bytes, multi-byte frame
numbers, one declined subframe among accepted ones), so they are written by hand here.  Every stream is valid FLAC;
the truth is the samples that went in (tests/test_flac_builder.py checks the oracle against the same streams on the
CPU).  All comparisons are exact.

Each stream is checked two ways: decode_frames_host must return the known samples, and decode_tiles_host into
int16, uint16 and uint8 must equal the oracle's de-normalisation of the known samples (the fused stores of accepted
frames and the rewrite of declined ones).  The de-normalisation range is fixed per output type (its full range, so
that distinct samples stay distinct wherever the type allows), not taken from the data.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flac_layouts as L
from tests.test_gpu_decode import _decoder_ctx

pytestmark = pytest.mark.gpu

RANGES = ((np.int16, -32768.0, 32767.0), (np.uint16, 0.0, 65535.0), (np.uint8, 0.0, 255.0))
CASES = [(name, kind) for name, (_, kinds) in L.STREAMS.items() for kind in kinds]


def _first_diff(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return f"{bad.size} samples differ, first at {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}"


@pytest.mark.parametrize("name,kind", CASES, ids=[f"{n}-{k}" for n, k in CASES])
def test_layout_decodes_to_known_samples(name, kind, monkeypatch):
    s = L.get(name)
    n, ch = len(s.pcm), s.channels
    want = s.pcm.astype(np.int32)
    blob = np.frombuffer(s.data, dtype=np.uint8)
    dctx = _decoder_ctx(kind, monkeypatch)
    try:
        got = dctx.decode_frames_host(blob, [0, blob.size], [n], channels=ch, bps=s.bps, blocksize=s.blocksize)
        got = got.reshape(n, ch)
        assert np.array_equal(got, want), (_first_diff(got, want), "frames",
                                           np.unique(np.flatnonzero((got != want).any(1)) // s.blocksize).tolist())
        for dtype, mn, mx in RANGES:
            vals = dctx.decode_tiles_host(blob, [0, blob.size], [n], channels=ch, bps=s.bps, data_min=[mn],
                                          data_max=[mx], dtype=dtype, blocksize=s.blocksize)
            ref = O.denormalize_i16(want, mn, mx, dtype, pcm_bps=s.bps)
            assert np.array_equal(vals.reshape(-1), ref.reshape(-1)), (np.dtype(dtype).name, _first_diff(vals, ref))
    finally:
        dctx.close()
