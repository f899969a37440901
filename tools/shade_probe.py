#!/usr/bin/env python3
"""Shade probe: device time of frs_render_shaded_window_device beside the plain frs_render_window_device on the same
source, rectangle and mode, in one process, the two alternating.

The source and the box are tools/render_probe.py's: a 16384 x 16384 int16 band (512 MB) resident in device memory --
the synthetic DEM (frs_synth_raster_device) with a 1024-row nodata band at the top and the bottom -- rendered to
8192 x 8192 pixels: the three modes, without and with the nodata value, C = 1 and C = 4, a 256-entry colour table.
Kernel times come from HIP events on the context stream (frs_profile_avg_ms("render_shaded" / "render")) after warm-up.
Prints, and writes to profiles/shade_probe.json.

usage: shade_probe.py [--src N] [--dst N] [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

NODATA = -9999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, default=16384)
    ap.add_argument("--dst", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shade_probe.json"))
    args = ap.parse_args()
    from flac_raster_amd import _native, render
    S, D = args.src, args.dst
    ctx = _native.Context(0)
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    band = min(1024, S // 16)
    light = render.light_vector(*render.DEFAULT_HILLSHADE)
    kx, ky = render.shade_scales(float(S) / D, float(S) / D, 1.0)  # a source pixel is one ground unit
    table = render.shade_table(1.0)
    out = {"library_sha256_16": sha, "source": [S, S], "dtype": "int16", "source_bytes": S * S * 2,
           "destination": [D, D], "rect": [0.0, 0.0, float(S), float(S)], "reps": args.reps, "warmup": args.warmup,
           "nodata": NODATA, "nodata_rows_top_and_bottom": band, "lut_entries": 256, "light": list(light),
           "kx": kx, "ky": ky, "cases": []}
    src = ctx.alloc(S * S * 2)
    dst_shaded = ctx.alloc(D * D * 4)
    dst_plain = ctx.alloc(D * D * 4)
    try:
        ctx.synth_raster(src, 1, S, S, seed=1234)
        rows = np.full((band, S), NODATA, dtype=np.int16)
        src.upload(rows, offset=0)
        src.upload(rows, offset=(S - band) * S * 2)
        sd = ctx.make_raster_desc(S, S, np.int16)
        st = ctx.band_stats_device(src.ptr, sd, nodata=NODATA)[0]
        lo, hi = float(st["min"]), float(st["max"])
        out["stretch"] = [lo, hi]
        rect = (0.0, 0.0, float(S), float(S))
        lut = render.build_lut("terrain", 256)
        for mode in ("nearest", "bilinear", "average"):
            for nd in (None, NODATA):
                for C in (1, 4):
                    def both():
                        ctx.render_shaded_window_device(src.ptr, sd, dst_shaded.ptr, D, D, rect, mode, lo, hi, lut,
                                                        light, kx, ky, table, channels=C, nodata=nd)
                        ctx.render_window_device(src.ptr, sd, dst_plain.ptr, D, D, rect, mode, lo, hi, lut,
                                                 channels=C, nodata=nd)
                    ctx.profile(False)
                    for _ in range(args.warmup):
                        both()
                    ctx.profile(True)
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        both()
                    wall_ms = (time.perf_counter() - t0) * 1e3 / args.reps
                    s_ms, p_ms = ctx.profile_avg_ms("render_shaded"), ctx.profile_avg_ms("render")
                    row = {"mode": mode, "nodata": nd, "channels": C, "shaded_ms": round(s_ms, 4),
                           "plain_ms": round(p_ms, 4), "shaded_over_plain": round(s_ms / p_ms, 3),
                           "store_bytes": D * D * C, "shaded_pixels_per_s": D * D / (s_ms * 1e-3),
                           "pair_wall_ms": round(wall_ms, 4)}
                    print(json.dumps(row), flush=True)
                    out["cases"].append(row)
    finally:
        for b in (src, dst_shaded, dst_plain):
            b.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
