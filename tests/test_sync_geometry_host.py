"""The blobs of tests/sync_geometry.py on the CPU: what tests/test_gpu_sync_geometry.py decodes is what it is meant to
be.  An independent model of the selection (every FF F8|F9 whose header the RFC reader of tests/test_frame_header.py
accepts, bounded by the range end) finds exactly the true frames and the planted false syncs; every position class is
present for every selection form it applies to; the oracle decodes every stream to the samples that went in; every GPU
case takes the route it is meant to (csrc/frs_decode_plan.h); and the CRC-16 relations of the false syncs hold."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flac_builder as B
from tests import sync_geometry as G
from tests.test_decode_plan import plan  # noqa: F401  (the compiled plan_decode_route harness, a fixture)
from tests.test_frame_header import rfc_reader

ALL_CASES = [c for group in G.CASES.values() for c in group]
BLOBS = sorted({(c.blob, c.lead) for c in ALL_CASES} | {("plain", 0)})


def model_candidates(blob: G.Blob):
    """p of every sync code in [0, nbytes) with a header RFC 9639 accepts for this stream, bounded by the range end."""
    body, nb = blob.body, blob.nbytes
    a = np.frombuffer(body, dtype=np.uint8)
    pairs = np.flatnonzero((a[:-1] == 0xFF) & ((a[1:] & 0xFE) == 0xF8))
    return [int(p) for p in pairs if rfc_reader(body[p:p + 16], min(16, nb - int(p)), blob.channels, 16)]


@pytest.mark.parametrize("name,lead", BLOBS, ids=["%s-lead%d" % b for b in BLOBS])
def test_candidates_are_the_frames_and_the_planted_false_syncs(name, lead):
    blob = G.get(name, lead)
    true = [p for p, _, _ in blob.frames()]
    assert true[0] == 0 and true == sorted(true)
    planted = blob.false_syncs()
    assert len(planted) == {"fa": 1, "false-big": 3}.get(name, 2 if name.startswith("fb-") else 0)
    assert model_candidates(blob) == sorted(true + planted)  # no accidental ones
    assert [int(c) for c in blob.counts] == [len(s.pcm) for s in blob.streams]
    assert blob.nframes == sum(-(-n // blob.blocksize) for n in blob.counts)
    # the guards: complete headers that lie outside [0, nbytes), behind >= 16 and before >= 32 bytes
    whole, off = blob.assemble(32 + lead)
    assert off[0] == 32 + lead and off[-1] - off[0] == blob.nbytes and len(whole) - off[-1] >= 32
    assert whole[off[0]:off[-1]] == blob.body
    for g in blob.guard_headers:
        assert g < 0 or g + 2 > blob.nbytes
        assert rfc_reader(whole[off[0] + g:off[0] + g + 16], 16, blob.channels, 16) is not None, g
    if lead >= 6:
        assert -lead <= blob.guard_headers[0] < 0  # inside the first 16-byte load
    if lead >= 1:
        assert whole[off[0] - 1] == 0xFF


@pytest.mark.parametrize("form", list(G.FORMS))
def test_every_position_class_is_present(form):
    """The coverage of the builder: nothing of the issue's list may be missing, for any lead a GPU case runs."""
    leads = G.SMALL_LEADS if form == "small" else G.BIG_LEADS
    ends = set()
    for lead in leads:
        hit = G.classes_hit(G.get(form, lead))
        assert not G.POSITIONS - hit, (lead, sorted(G.POSITIONS - hit))
        assert not G.BOUNDS - hit, (lead, G.BOUNDS - hit)
        assert ("start", lead) in hit
        if form == "twopass":
            assert {("cap", 31), ("cap", 32), ("cap", 33)} <= hit
            assert ("cap", "a wave's last 16 bytes in a block read again") in hit
        ends |= {h for h in hit if h[0] == "end"}
    assert {("end", "block"), ("end", "block + 1"), ("end", "header")} <= ends


def test_g_cap_blocks_of_the_eight_channel_blob():
    for lead in G.BIG_LEADS:
        blob = G.get("cap8", lead)
        hit = G.classes_hit(blob)
        assert {("cap", 0), ("cap", 31), ("cap", 32), ("cap", 33), ("start", lead)} <= hit
        assert blob.nbytes + lead > 16 * G.MIB and blob.nframes >= 64
        # the block without a candidate lies inside one frame of ~65.5 KB
        counts = G.block_counts(blob, [p for p, _, _ in blob.frames()])
        assert 0 in counts[1:-1]


def test_g_start_and_g_end_under_every_lead():
    mods, ends = set(), set()
    for lead in range(16):
        blob = G.get("edge-mod", lead)
        hit = G.classes_hit(blob)
        assert ("start", lead) in hit
        assert ("end mod 16", (5 * lead + 3) % 16) in hit
        mods |= {h[1] for h in hit if h[0] == "end mod 16"}
        ends |= {h for h in hit if h[0] == "end"}
        if blob.end_split:  # the range's last byte is the 0xFF of a header the back guard completes
            assert blob.body[-1] == 0xFF and blob.back[0] == 0xF8
    assert mods == set(range(16)) and ends == {("end", "header"), ("end", "split")}
    for lead in (0, 9):
        assert ("end", "block") in G.classes_hit(G.get("edge-bk", lead))
        assert ("end", "block + 1") in G.classes_hit(G.get("edge-bk1", lead))
        assert (G.get("edge-bk", lead).nbytes + lead) % 16384 == 0
        assert (G.get("edge-bk1", lead).nbytes + lead) % 16384 == 1


def test_blob_sizes_and_thresholds():
    for lead in G.SMALL_LEADS:
        assert 200 << 10 < G.get("small", lead).nbytes + lead < 1 << 20
    for lead in G.BIG_LEADS:
        assert 4 * G.MIB < G.get("onepass", lead).nbytes + lead < 4 * G.MIB + (256 << 10)
        assert 16 * G.MIB < G.get("twopass", lead).nbytes + lead < 16 * G.MIB + (256 << 10)
    for name, total in G.THRESHOLDS.items():
        for lead in (0, 15):
            assert G.get(name, lead).nbytes + lead == total


@pytest.mark.parametrize("name,lead", BLOBS, ids=["%s-lead%d" % b for b in BLOBS])
def test_oracle_decodes_known_samples(name, lead):
    """Every distinct stream of the blob (filler repeats one stream; the 8-channel blob one 65.5 KB frame)."""
    blob = G.get(name, lead)
    seen = set()
    for s in blob.streams:
        if id(s) in seen:
            continue
        seen.add(id(s))
        got = O.decode_frames(s.data, blob.channels, 16, len(s.pcm))
        assert np.array_equal(got.reshape(-1, blob.channels), s.pcm.astype(np.int32))


def test_routes_of_the_gpu_cases(plan):  # noqa: F811
    lines, want = [], []
    for c in ALL_CASES:
        blob = G.get(c.blob, c.lead)
        e = c.env
        # (decode_job reads FRS_SPAN_READ above 4 MiB only)
        span = int(e.get("FRS_SPAN_READ", 0)) if blob.nbytes > 4 * G.MIB else 0
        args = (blob.channels, 16, blob.blocksize, blob.nframes, len(blob.streams), blob.nbytes, c.lead,
                int(e.get("FRS_FORCE_GENERIC", 0)), int(e.get("FRS_DECODE_LANE", -1)), int(e.get("FRS_PIPE_OPT", 1)),
                span, 0)
        lines.append("r " + " ".join(str(v) for v in args))
        want.append(c.route)
    for c, got, route in zip(ALL_CASES, plan(lines), want):
        assert got[:4] == route, (c.id, got[:4], route)
    # every selection form, span check and frame decoder is among them
    assert [{r[i] for r in want} for i in range(3)] == [{0, 1, 2}, {0, 1, 2}, {0, 1, 2, 3}]


def _be16(v: int) -> bytes:
    return v.to_bytes(2, "big")


@pytest.mark.parametrize("lead", G.FALSE_LEADS)
@pytest.mark.parametrize("name", G.FALSE_BLOBS)
def test_false_sync_crc_relations(name, lead):
    """F-a: no span ends at or starts from the spelled header.  F-b: the false candidate at a has the verified span
    [a, b); the frame's start links to neither a nor b but to the next frame; nothing verifies from b or from a to the
    next frame: the only consistent chain is the true one, and it has one verified candidate more than frames."""
    blob = G.get(name, lead)
    body = blob.body
    true = [p for p, _, _ in blob.frames()] + [blob.nbytes]
    for off, s in zip(blob.rel_off, blob.streams):
        if not s.false_syncs:
            continue
        fs = [off + a for a in s.false_syncs]
        start = max(p for p in true if p < fs[0])
        nxt = min(p for p in true if p > fs[-1])
        assert B.crc16(body[start:nxt - 2]) == int.from_bytes(body[nxt - 2:nxt], "big")
        for a in fs:
            assert start < a < nxt
            assert _be16(B.crc16(body[start:a - 2])) != body[a - 2:a]
            assert _be16(B.crc16(body[a:nxt - 2])) != body[nxt - 2:nxt]
        if len(fs) == 2:
            a, b = fs
            assert _be16(B.crc16(body[a:b - 2])) == body[b - 2:b]
    if name == "fb-long":
        assert len(blob.streams) == 1 and blob.nframes > 4096 and blob.blocksize == 16
    if name == "fb-one":
        assert len(blob.streams) == 1
    if name == "fb-multi":
        s = blob.streams[1]
        assert len(blob.streams) > 1 and s.false_syncs and 0 < s.target < len(s.starts) - 1
