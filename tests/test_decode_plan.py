"""csrc/frs_decode_plan.h built by the host compiler alone: the decode route against a transcription of the conditions
decode_job used to evaluate inline, and the two scratch carves (regions in order, disjoint, aligned, inside the
allocation)."""
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flac_raster_amd" / "csrc" / "frs_decode_plan.h"

PROG = f'''#include "{HEADER}"
#include <stdio.h>
int main() {{
    char kind;
    while (scanf(" %c", &kind) == 1) {{
        if (kind == 'r') {{
            int ch, bps, bs, ns, lead, fg, dl, po, sm, fused;
            long long frames, bytes;
            if (scanf("%d %d %d %lld %d %lld %d %d %d %d %d %d", &ch, &bps, &bs, &frames, &ns, &bytes, &lead, &fg, &dl,
                      &po, &sm, &fused) != 12) return 1;
            const frs::DecodeRoute r = frs::plan_decode_route(ch, bps, bs, frames, ns, bytes, lead, fg, dl, po, sm, fused);
            printf("%d %d %d %d %d %d %d %lld %lld %lld %lld %lld %lld\\n", (int)r.sel, (int)r.span, (int)r.dec,
                   (int)r.pipe_opt, (int)r.planar16, (int)r.tabs_by_arg, (int)r.fused, (long long)r.nblocks,
                   (long long)r.nfull, (long long)r.sel_bytes, (long long)r.cand_cap, (long long)r.max_frame,
                   (long long)r.planar_words);
        }} else if (kind == 's') {{
            long long nb;
            if (scanf("%lld", &nb) != 1) return 1;
            const frs::SelLayout l = frs::sel_layout(nb);
            printf("%zu %zu %zu %zu\\n", l.bcount, l.bbase, l.bpos, l.total);
        }} else {{
            long long nb, cap;
            int ns;
            if (scanf("%lld %d %lld", &nb, &ns, &cap) != 3) return 1;
            const frs::PcrcLayout l = frs::pcrc_layout(nb, ns, cap);
            printf("%zu %zu %zu %zu %zu %zu %zu\\n", l.bp, l.bfirst, l.bcrc, l.bipc, l.sbib, l.pcrc, l.total);
        }}
    }}
    printf("%d %d %d %d %d %d %d %d %d %d\\n", frs::kCntCand, frs::kCntValid, frs::kCntBroken, frs::kCntFallback,
           frs::kCntTicket, frs::kCntDecline, frs::kCntOptValid, frs::kCntRearm, frs::kCntHostWords, frs::kSelBlkCap);
    return 0;
}}'''

ONE_PASS_SMALL, ONE_PASS, TWO_PASS = 0, 1, 2   # SelForm
PCRC, SPAN_LANE, SPAN_WAVE = 0, 1, 2           # SpanForm
PIPE, LANE, MULTI_LANE, WAVE = 0, 1, 2, 3      # FrameDec
SEL_BLK_CAP = 32


def old_route(ch, bps, bs, frames, ns, nbytes, lead, fg, dl, po, sm, fused):
    """decode_job's conditions before the plan existed, in the order and the words it had them (k_span_crc, the
    fourth span check it could never reach, is the `assert` below)."""
    max_frame = bs * ch * 5 + 4096
    pipe = ch == 1 and bps <= 16 and bs <= 4096 and not fg
    lane = pipe and frames >= 4096
    if dl >= 0:
        lane = pipe and dl == 1
    mcl = 2 <= ch <= 8 and bps <= 16 and bs <= 4096 and not fg and frames >= 64 and dl != 0
    planar_words = frames * ch * bs if mcl else 0
    cand_cap = min(2 * frames + nbytes // 1024 + 4096, 0x7FFFFFF0)
    lead_bytes = nbytes + lead
    small_bytes = 4 * 1024 * (256 // 64)
    sel_small = (lead_bytes + small_bytes - 1) // small_bytes <= 256
    sel_bytes = small_bytes if sel_small else 64 * 1024
    nblocks = (lead_bytes + sel_bytes - 1) // sel_bytes
    tabs_by_arg = ns == 1 and nblocks <= 256
    span_mode = sm if nblocks > 256 else 0  # (the environment was read for the two-pass selection only)
    pcrc_span = (span_mode != 1 and (span_mode == 2 or mcl) and nblocks > 256 and (lane or not pipe)
                 and max_frame < 4096 * 256)
    sel = (ONE_PASS_SMALL if sel_small else ONE_PASS) if nblocks <= 256 else TWO_PASS
    nfull = min(nblocks, lead_bytes // (64 * 1024)) if sel == TWO_PASS else 0
    pipe_opt = pipe and not lane and max_frame < 4096 * 256 and po
    if pcrc_span:
        span = PCRC
    elif lane or not pipe:
        span = SPAN_LANE
    else:
        assert max_frame < 4096 * 256  # else: k_span_crc
        span = SPAN_WAVE
    dec = LANE if lane else MULTI_LANE if mcl else PIPE if pipe else WAVE
    planar16 = mcl and ch >= 3
    return (sel, span, dec, int(bool(pipe_opt)), int(planar16), int(tabs_by_arg), int(fused), nblocks, nfull, sel_bytes,
            cand_cap, max_frame, planar_words)


def _grid():
    small, big = 16 * 1024, 64 * 1024
    # blob bytes on either side of the small / one-pass and the one-pass / two-pass block counts
    sizes = [1, 256 * small - 15, 256 * small - 14, 256 * small, 256 * small + 1, 256 * big - 15, 256 * big - 14,
             256 * big, 256 * big + 1, 1000 * big + 5]
    shapes = [(ch, bps, bs) for ch in (1, 2, 3, 8, 9) for bps in (16, 17) for bs in (4096, 4097)]
    # max_frame on either side of 4096 * 256 for shapes that are never Pipe: 9 channels x 5 x bs + 4096
    shapes += [(9, 16, 23210), (9, 16, 23211), (2, 32, 104447), (2, 32, 104448)]
    for (ch, bps, bs), frames, nbytes, lead in itertools.product(shapes, (1, 63, 64, 4095, 4096), sizes, (0, 15)):
        for ns, fg, dl, po, sm in itertools.product((1, 2), (0, 1), (-1, 0, 1), (0, 1), (0, 1, 2)):
            yield (ch, bps, bs, frames, ns, nbytes, lead, fg, dl, po, sm, (ns + dl + sm) & 1)  # (fused: passed on)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_plan")
    (d / "t.cpp").write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(d / "t"), str(d / "t.cpp")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "t")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        rows = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
        assert len(rows) == len(lines) + 1
        return rows
    return run


def test_header_does_not_need_hip():
    text = HEADER.read_text()
    assert "#include <hip" not in text and '#include "' not in text


def test_route_is_the_old_conditions(plan):
    grid = list(_grid())
    assert len(grid) == 24 * 5 * 10 * 2 * 72
    rows = plan(["r " + " ".join(str(v) for v in g) for g in grid])
    seen = set()
    for g, got in zip(grid, rows):
        assert got == old_route(*g), (g, got, old_route(*g))
        seen.add(got[:3])
        # no Pipe route is outside the x^(8m) tables: the span check that case had could never run
        assert got[2] != PIPE or got[11] < 4096 * 256, g
    # every form of each stage is reached, and both sides of the table range by shapes that are not Pipe
    assert {s[0] for s in seen} == {ONE_PASS_SMALL, ONE_PASS, TWO_PASS}
    assert {s[1] for s in seen} == {PCRC, SPAN_LANE, SPAN_WAVE}
    assert {s[2] for s in seen} == {PIPE, LANE, MULTI_LANE, WAVE}
    assert {r[11] >= 4096 * 256 for r in rows[:-1]} == {False, True}


def test_counter_names(plan):
    """The counters word: the selection's 64-bit ticket at byte 16, eight words to the host, the re-armed one after."""
    assert plan([])[-1] == (0, 1, 2, 3, 4, 6, 7, 8, 8, SEL_BLK_CAP)


def _check_regions(offsets, sizes, elems, total):
    for i, (off, size, elem) in enumerate(zip(offsets, sizes, elems)):
        assert off % elem == 0, (i, off, elem)
        end = off + size
        assert end <= (offsets[i + 1] if i + 1 < len(offsets) else total), (i, offsets, sizes, total)


@pytest.mark.parametrize("nb", [257, 258, 4097])
def test_layouts(plan, nb):
    bcount, bbase, bpos, total = plan(["s %d" % nb])[0]
    assert bcount == 0
    _check_regions([bcount, bbase, bpos], [4 * nb, 8 * (nb + 1), 8 * SEL_BLK_CAP * nb], [4, 8, 8], total)
    for ns, cap in itertools.product((1, 2, 6241), (4097, 4098)):
        *offs, total = plan(["p %d %d %d" % (nb, ns, cap)])[0]
        assert offs[0] == 0
        _check_regions(offs, [4 * (nb + 1), 4 * nb, 2 * nb, 2 * SEL_BLK_CAP * nb, 2 * (ns + 1), 2 * cap],
                       [4, 4, 2, 2, 2, 2], total)
