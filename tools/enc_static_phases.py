#!/usr/bin/env python3
"""Static per-phase instruction table of k_encode_v4's mono 16-bit instance from a line-table build.

usage: tools/enc_static_phases.py [SOURCE.hip [LISTING.s]]

Compiles SOURCE (default flac_raster_amd/csrc/frs_encode.hip) for gfx950 with -DFRS_PROBE_I16 -gline-tables-only -S
(unless LISTING is given) and assigns every instruction of k_encode_v4<3, false, false, false, 8> to the source line
of its innermost inlined function (.loc; lines of the HIP headers count with the code before them), and the line to
a phase by the marker comments and function heads named in PHASES.  Counts are static (instructions in the ISA,
every path once: the slow normalisers, the gather loads and the repack path count like the hot path), as VALU / SALU
/ LDS / VMEM, with the v_readlane and v_writelane among the VALU listed apart.  Helpers shared by several phases
(the DPP reductions, the dot2 residual chains, the bit-buffer layout) have rows of their own.
"""
import re
import subprocess
import sys
import tempfile
from collections import Counter, defaultdict
from pathlib import Path

KERNEL = "_ZN3frs11k_encode_v4ILi3ELb0ELb0ELb0ELi8E"

# (marker text that begins a range of frs_encode.hip, phase of the lines from there to the next marker)
PHASES = [
    ("__device__ inline uint32_t gf_mulmod(", "CRC"),
    ("__device__ inline uint32_t wg_crc16(", "other"),
    ("__device__ inline int32_t norm_fast(", "load and normalise"),
    ("__global__ void __launch_bounds__(256) k_build_lut(", "other"),
    ("template <int DT, int N> struct ChunkN {", "load and normalise"),
    ("__global__ void __launch_bounds__(256) k_zero_subframes(", "other"),
    ("template <int CTRL> __device__ inline uint32_t dpp_mov(", "cross-lane helpers (DPP sums, scans)"),
    ("typedef short v2s16", "residual helpers (dot2 chains)"),
    ("constexpr uint64_t kFlagAgg", "other"),
    ("struct FbMap {", "bit-buffer helpers (layout, code writer)"),
    ("__device__ inline void lut_gather_pairs(", "load and normalise"),
    ("__device__ inline uint32_t zigzag(", "packing"),
    ("__device__ __forceinline__ void resolve_and_store(", "resolve/look-back"),
    ("        // ---- store [prefix, prefix + fbytes)", "store"),
    ("    // leave the bit buffer zeroed for this wave's next frame", "store (re-zeroing)"),
    ("struct LanePairs {", "lane samples (residuals, warm-up, history)"),
    ("__device__ __forceinline__ void rice_candidates(", "Rice search"),
    ("constexpr int kPrivRows", "assembly"),
    ("constexpr int kCrcRows", "CRC"),
    ("__device__ __forceinline__ void encode_frame_v4(", "frame set-up and copy path"),
    ("    // ---- this lane's 64 samples of the coded signal", "load and normalise"),
    ("    // ---- candidates: the fixed order guess from the totals", "candidates and choice (totals, LPC sums)"),
    ("    // ---- field positions", "header and fields"),
    ("    // ---- the previous frame of this wave", "packing"),
    ("    // ---- assembly into the v3 frame layout", "assembly"),
    ("    // ---- header, subframe header, warm-up, coefficients", "header and fields"),
    ("template <int DT, bool SUB> constexpr int enc_nw()", "ticket loop"),
    ("// ---------------------------------------------------------------- multi-channel streams", "other"),
]
BY_FILE = {"frs_crc16_fold.h": "CRC", "frs_frame_header.h": "header and fields", "frs_store_select.h": "store",
           "frs_fixed_totals.h": "totals"}


def line_phases(src_text):
    lines = src_text.splitlines()
    marks = []
    for text, phase in PHASES:
        hits = [i + 1 for i, l in enumerate(lines) if l.startswith(text)]
        assert hits, text
        marks.append((hits[0], phase))
    marks.sort()
    return marks


def phase_of(marks, line):
    ph = "other"
    for start, p in marks:
        if line < start:
            break
        ph = p
    return ph


def main():
    src = Path(sys.argv[1] if len(sys.argv) > 1 else "flac_raster_amd/csrc/frs_encode.hip")
    if len(sys.argv) > 2:
        asm = Path(sys.argv[2]).read_text()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = Path(td) / "k.s"
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-fno-fast-math", "-DFRS_PROBE_I16", "--cuda-device-only",
                            "-gline-tables-only", "-S", "-I", str(Path("flac_raster_amd/csrc").resolve()), "-o", str(out),
                            str(src)], check=True, stderr=subprocess.DEVNULL)
            asm = out.read_text()
    marks = line_phases(src.read_text())
    files = {}
    for m in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', asm, re.M):
        files[int(m.group(1))] = Path(m.group(2)).name
    m = re.search(r"^(" + KERNEL + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert m, "kernel not in the listing"
    tab = defaultdict(Counter)
    phase = "other"
    for line in m.group(2).splitlines():
        s = line.strip()
        loc = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if loc:
            f = files.get(int(loc.group(1)), "?")
            if f == src.name:
                phase = phase_of(marks, int(loc.group(2)))
            elif f in BY_FILE:
                phase = BY_FILE[f]
            # (a line of the HIP headers -- atomicOr, min, __umul24 -- stays with the phase that called it)
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        kind = ("VALU" if op.startswith("v_") else "LDS" if op.startswith("ds_") else
                "VMEM" if op.startswith(("global_", "flat_", "buffer_", "scratch_")) else
                "SALU" if op.startswith("s_") else "other")
        tab[phase][kind] += 1
        if op.startswith(("v_readlane", "v_writelane")):
            tab[phase]["lane"] += 1
    cols = ("VALU", "SALU", "LDS", "VMEM", "lane")
    print("| phase | VALU | SALU (with waits, branches) | LDS | VMEM | of the VALU: v_readlane + v_writelane |")
    print("|---|---:|---:|---:|---:|---:|")
    tot = Counter()
    for ph in sorted(tab, key=lambda p: -tab[p]["VALU"]):
        print(f"| {ph} | " + " | ".join(str(tab[ph][c]) for c in cols) + " |")
        tot.update(tab[ph])
    print("| **total** | " + " | ".join(str(tot[c]) for c in cols) + " |")


if __name__ == "__main__":
    main()
