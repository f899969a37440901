"""Frame location on the GPU at every work boundary: the blobs of tests/sync_geometry.py (frames at prescribed
positions of the selection's lanes, steps, waves and blocks, under a prescribed `lead`; false syncs whose spans do and
do not verify) through the selection, the span check and the chain of csrc/frs_decode.hip, on every route
tests/test_sync_geometry_host.py pins.  Each blob is uploaded once, behind a front guard whose length sets the low four
bits of the range's address, and decoded with decode_frames_device and a nonzero stream_off[0].  The truth is the
samples that went in: every comparison is exact, no FrsError is raised, and the context decodes a plain stream after."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sync_geometry as G

pytestmark = pytest.mark.gpu

SWITCHES = ("FRS_FORCE_GENERIC", "FRS_DECODE_LANE", "FRS_PIPE_OPT", "FRS_SPAN_READ")
DMIN, DMAX = -500.0, 1500.0


class Device:
    """Uploaded blobs, (name, lead) -> (blob, buffer, stream_off), and one output buffer, on the session's context
    (plain device memory: the contexts of the cases read and write it)."""

    def __init__(self, ctx):
        self.ctx, self.held, self.out, self.poison = ctx, {}, None, np.zeros(0, dtype=np.uint8)

    def blob(self, name: str, lead: int):
        key = (name, lead)
        if key not in self.held:
            blob = G.get(name, lead)
            buf = self.ctx.alloc(blob.nbytes + 48 + len(blob.back) + 64)
            guard = 32 + (lead - buf.ptr) % 16
            data, off = blob.assemble(guard)
            assert (buf.ptr + off[0]) % 16 == lead and off[0] >= 16 and len(data) - off[-1] >= 32
            buf.upload(np.frombuffer(data, dtype=np.uint8))
            blob.cache.pop("body", None)  # (the joined bytes of a 16 MiB blob are not kept beside the upload)
            self.held[key] = (blob, buf, np.asarray(off, dtype=np.int64))
        return self.held[key]

    def output(self, nbytes: int):
        """A buffer of at least nbytes whose first nbytes hold no earlier result."""
        if self.out is None or self.out.nbytes < nbytes + 64:
            if self.out is not None:
                self.out.close()
            self.out = self.ctx.alloc(nbytes + 64)
        if len(self.poison) < nbytes:
            self.poison = np.full(nbytes, 0x5A, dtype=np.uint8)
        self.out.upload(self.poison[:nbytes])
        return self.out

    def close(self):
        for _, buf, _ in self.held.values():
            buf.close()
        if self.out is not None:
            self.out.close()


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


@pytest.fixture
def make_ctx(monkeypatch):
    """Contexts under a case's switches (read when the context is made; FRS_SPAN_READ per call), closed after."""
    made = []

    def make(env):
        from flac_raster_amd import _native
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        made.append(_native.Context(0))
        return made[-1]
    yield make
    for c in made:
        c.close()


def decode_frames(ctx, dev, name, lead):
    """decode_frames_device of an uploaded blob against the samples that went in."""
    blob, buf, off = dev.blob(name, lead)
    n, ch = blob.pcm.shape
    out = dev.output(4 * n * ch)
    ctx.decode_frames_device(buf, off, blob.counts, ch, 16, out, blocksize=blob.blocksize)
    got = out.download(4 * n * ch).view(np.int32).reshape(n, ch)
    bad = np.flatnonzero((got != blob.pcm).any(axis=1))
    assert bad.size == 0, "%s lead %d: %d samples differ, the first at %d" % (name, lead, bad.size, bad[0])


_DENORM = {}


def decode_tiles(ctx, dev, name, lead):
    """decode_tiles_device into int16 against the oracle's de-normalisation of the samples that went in."""
    blob, buf, off = dev.blob(name, lead)
    n, ch = blob.pcm.shape
    if (name, lead) not in _DENORM:
        _DENORM[name, lead] = O.denormalize_i16(blob.pcm.astype(np.int32), DMIN, DMAX, np.int16)
    out = dev.output(2 * n * ch)
    ns = len(blob.counts)
    ctx.decode_tiles_device(buf, off, blob.counts, ch, 16, [DMIN] * ns, [DMAX] * ns, np.int16, out,
                            blocksize=blob.blocksize)
    got = out.download(2 * n * ch).view(np.int16).reshape(n, ch)
    assert np.array_equal(got, _DENORM[name, lead].reshape(n, ch)), (name, lead)


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", G.CASES["small"], ids=_ids(G.CASES["small"]))
def test_small_form_positions(dev, make_ctx, case):
    """k_sync_select<4> (4 KB waves, 16 KB blocks): G-lane, G-step, G-wave, G-block, G-bound under eight leads on every
    decoder kind; leads 1, 2, 3 on pipe_chain are k_span_crc_wave's unaligned dword staging."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_tiles(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["edge"], ids=_ids(G.CASES["edge"]))
def test_range_start_and_end(dev, make_ctx, case):
    """G-start and G-end under all 16 leads: a complete header in the bytes the first load reads in front of the
    range, one at the range's end, one the range's last byte begins; the range ending on, and one byte past, a block."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_tiles(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["onepass"], ids=_ids(G.CASES["onepass"]))
def test_one_pass_form_positions(dev, make_ctx, case):
    """k_sync_select<16> (16 KB waves, 64 KB blocks) on a range just above 4 MiB."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["twopass"], ids=_ids(G.CASES["twopass"]))
def test_two_pass_form_positions(dev, make_ctx, case):
    """k_sync_count + k_sync_scan + k_sync_scatter on a range just above 16 MiB, with the reading span check
    (FRS_SPAN_READ=1) and the prefix-CRC one (=2: k_bound_mark, sbib, k_span_pcrc)."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["cap8"], ids=_ids(G.CASES["cap8"]))
def test_two_pass_block_capacity(dev, make_ctx, case):
    """G-cap on the default route of 8 channels (MultiLane + Pcrc): blocks of exactly 31, 32 and 33 candidates (the
    kept positions, the last kept one, the re-read) and a block inside one frame."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)


def test_two_pass_between_small_forms(dev, make_ctx):
    """One context: a small-form decode, a two-pass one, a small-form one again (the epoch-tagged status words and
    the re-armed ticket across forms), then a plain stream."""
    ctx = make_ctx({"FRS_DECODE_LANE": "1", "FRS_SPAN_READ": "2"})
    decode_frames(ctx, dev, "small", 3)
    decode_frames(ctx, dev, "twopass", 5)
    decode_frames(ctx, dev, "edge-bk1", 9)
    decode_frames(ctx, dev, "small", 3)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["threshold"], ids=_ids(G.CASES["threshold"]))
def test_form_thresholds(dev, make_ctx, case):
    """nbytes + lead of exactly 4 MiB, 4 MiB + 1, 16 MiB and 16 MiB + 1: the last range of a form and the first of the
    next."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["false"], ids=_ids(G.CASES["false"]))
def test_false_syncs(dev, make_ctx, case):
    """F-a (nothing verifies at the spelled header) and F-b (the false candidate's span verifies: k_chain_lds counts
    one verified candidate more than frames and falls back to the exact walk -- its 64-thread form, its 1024-thread
    form, and the global walk of more than 4096 candidates).  The optimistic decode declines and the full path runs."""
    ctx = make_ctx(case.env)
    if case.kind == "pipe":
        ctx.profile(True)
        ctx.profile_reset()
    decode_frames(ctx, dev, case.blob, case.lead)
    if case.kind == "pipe":
        assert ctx.profile_avg_ms("decode_fallback") >= 0 and ctx.profile_avg_ms("decode_span") >= 0
        ctx.profile(False)
    decode_frames(ctx, dev, "plain", 0)


@pytest.mark.parametrize("case", G.CASES["false-big"], ids=_ids(G.CASES["false-big"]))
def test_false_syncs_in_a_large_range(dev, make_ctx, case):
    """F-a and F-b in a range above 16 MiB, by the reading span check and by the prefix CRCs."""
    ctx = make_ctx(case.env)
    decode_frames(ctx, dev, case.blob, case.lead)
    decode_frames(ctx, dev, "plain", 0)
