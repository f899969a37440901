#!/usr/bin/env python3
"""Render probe: device time of frs_render_window_device beside frs_resample_window_device on the same source,
rectangle and mode, in one process, the two alternating.

A 16384 x 16384 int16 band (512 MB) resident in device memory -- the synthetic DEM (frs_synth_raster_device) with a
1024-row nodata band at the top and the bottom -- is rendered to 8192 x 8192 pixels: the three modes, C = 1 and C = 4,
LUT lengths 256 and 4096, without and with the nodata value.  A table of 256 entries is timed in both placements: in LDS
(the library's choice) and gathered from global memory (FRS_RENDER_LUT=global), the placement a longer table always
has.  Kernel times come from HIP events on the context stream (frs_profile_avg_ms("render" / "resample")) after
warm-up.  Each row carries the bytes each kernel stores: the render C bytes per pixel, the resample 2.  Prints, and
writes to profiles/render_probe.json.

usage: render_probe.py [--src N] [--dst N] [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import os
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "render_probe.json"))
    args = ap.parse_args()
    from flac_raster_amd import _native, render
    S, D = args.src, args.dst
    ctx = _native.Context(0)
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    band = min(1024, S // 16)
    out = {"library_sha256_16": sha, "source": [S, S], "dtype": "int16", "source_bytes": S * S * 2,
           "destination": [D, D], "rect": [0.0, 0.0, float(S), float(S)], "reps": args.reps, "warmup": args.warmup,
           "nodata": NODATA, "nodata_rows_top_and_bottom": band, "cases": []}
    src = ctx.alloc(S * S * 2)
    dst_render = ctx.alloc(D * D * 4)
    dst_resample = ctx.alloc(D * D * 2)
    try:
        ctx.synth_raster(src, 1, S, S, seed=1234)
        rows = np.full((band, S), NODATA, dtype=np.int16)
        src.upload(rows, offset=0)
        src.upload(rows, offset=(S - band) * S * 2)
        sd = ctx.make_raster_desc(S, S, np.int16)
        dd = ctx.make_raster_desc(D, D, np.int16)
        st = ctx.band_stats_device(src.ptr, sd, nodata=NODATA)[0]
        lo, hi = float(st["min"]), float(st["max"])
        out["stretch"] = [lo, hi]
        rect = (0.0, 0.0, float(S), float(S))
        for mode in ("nearest", "bilinear", "average"):
            for nd in (None, NODATA):
                for C in (1, 4):
                    for n, where in ((256, "lds"), (256, "global"), (4096, "global")):
                        lut = render.build_lut("terrain", n)
                        if n == 256 and where == "global":
                            os.environ["FRS_RENDER_LUT"] = "global"
                        else:
                            os.environ.pop("FRS_RENDER_LUT", None)

                        def both():
                            ctx.render_window_device(src.ptr, sd, dst_render.ptr, D, D, rect, mode, lo, hi, lut,
                                                     channels=C, nodata=nd)
                            ctx.resample_window_device(src.ptr, sd, dst_resample.ptr, dd, rect, mode, 0, nodata=nd)
                        ctx.profile(False)
                        for _ in range(args.warmup):
                            both()
                        ctx.profile(True)
                        ctx.profile_reset()
                        t0 = time.perf_counter()
                        for _ in range(args.reps):
                            both()
                        wall_ms = (time.perf_counter() - t0) * 1e3 / args.reps
                        r_ms, s_ms = ctx.profile_avg_ms("render"), ctx.profile_avg_ms("resample")
                        row = {"mode": mode, "nodata": nd, "channels": C, "lut_entries": n, "lut_in": where,
                               "render_ms": round(r_ms, 4), "resample_ms": round(s_ms, 4),
                               "render_over_resample": round(r_ms / s_ms, 3),
                               "render_store_bytes": D * D * C, "resample_store_bytes": D * D * 2,
                               "render_store_bytes_per_s": D * D * C / (r_ms * 1e-3),
                               "resample_store_bytes_per_s": D * D * 2 / (s_ms * 1e-3),
                               "pair_wall_ms": round(wall_ms, 4)}
                        print(json.dumps(row), flush=True)
                        out["cases"].append(row)
        os.environ.pop("FRS_RENDER_LUT", None)
    finally:
        for b in (src, dst_render, dst_resample):
            b.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
