#!/usr/bin/env python3
"""Composite probe: device time of frs_render_composite_window_device beside three C = 1 frs_render_window_device
calls on the same three planes, rectangle and mode, in one process, the two alternating; then the wall time and the
file size of a multi-band create-streaming beside one single-band run per band.

The source is three 16384 x 16384 int16 planes (1.5 GB) resident in device memory -- the synthetic multispectral DEM
(frs_synth_raster_device) with a 1024-row nodata band at the top and the bottom -- rendered to 8192 x 8192 pixels: the
three modes, without and with the nodata value, a 256-entry table (LDS) and a 4096-entry one (global gather).  Kernel
times come from HIP events on the context stream (frs_profile_avg_ms("render_composite" / "render")), read after every
repetition so that the spread across the alternation shows: min / median / max per side.  The file part encodes
three 8192 x 8192 planes (tile 1024, overviews and statistics) once as one file and once as three.  Prints, and writes
to profiles/composite_probe.json.

usage: composite_probe.py [--src N] [--dst N] [--reps N] [--warmup N] [--file-src N] [--out PATH]"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

NODATA = -9999


def _three(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}


def render_part(ctx, args, out):
    from flac_raster_amd import render
    S, D = args.src, args.dst
    band = min(1024, S // 16)
    out.update({"source": [3, S, S], "dtype": "int16", "source_bytes": 3 * S * S * 2, "destination": [D, D],
                "rect": [0.0, 0.0, float(S), float(S)], "reps": args.reps, "warmup": args.warmup, "nodata": NODATA,
                "nodata_rows_top_and_bottom": band, "cases": []})
    plane = S * S * 2
    src = ctx.alloc(3 * plane)
    dst_c = ctx.alloc(D * D * 4)
    dst_1 = ctx.alloc(D * D)
    try:
        ctx.synth_raster(src, 3, S, S, seed=1234)
        rows = np.full((band, S), NODATA, dtype=np.int16)
        for c in range(3):
            src.upload(rows, offset=c * plane)
            src.upload(rows, offset=c * plane + (S - band) * S * 2)
        sd3 = ctx.make_raster_desc(S, S, np.int16, nbands=3)
        sd1 = ctx.make_raster_desc(S, S, np.int16)
        st = ctx.band_stats_device(src.ptr, sd3, nodata=NODATA)
        lo3, hi3 = [float(s["min"]) for s in st], [float(s["max"]) for s in st]
        out["stretch"] = [lo3, hi3]
        rect = (0.0, 0.0, float(S), float(S))
        for n in (256, 4096):
            lut = render.build_lut("gray", n, 2.2 if n > 256 else 1.0)
            for mode in ("nearest", "bilinear", "average"):
                for nd in (None, NODATA):
                    def composite():
                        ctx.render_composite_window_device(src.ptr, sd3, dst_c.ptr, D, D, rect, mode, lo3, hi3, lut,
                                                           nodata=nd)

                    def three():
                        for c in range(3):
                            ctx.render_window_device(src.ptr + c * plane, sd1, dst_1.ptr, D, D, rect, mode, lo3[c],
                                                     hi3[c], lut, channels=1, nodata=nd)
                    ctx.profile(False)
                    for _ in range(args.warmup):
                        composite()
                        three()
                    ctx.profile(True)
                    comp, sep = [], []
                    for _ in range(args.reps):  # alternated: drift hits both sides alike
                        ctx.profile_reset()
                        composite()
                        comp.append(ctx.profile_avg_ms("render_composite"))
                        ctx.profile_reset()
                        three()
                        sep.append(3.0 * ctx.profile_avg_ms("render"))
                    ctx.profile(False)
                    c_ms, s_ms = statistics.median(comp), statistics.median(sep)
                    row = {"lut_entries": n, "mode": mode, "nodata": nd, "composite_ms": _three(comp),
                           "three_renders_ms": _three(sep), "composite_over_three": round(c_ms / s_ms, 3),
                           "store_bytes": D * D * 4, "composite_pixels_per_s": D * D / (c_ms * 1e-3)}
                    print(json.dumps(row), flush=True)
                    out["cases"].append(row)
    finally:
        for b in (src, dst_c, dst_1):
            b.close()


def file_part(ctx, args, out):
    from flac_raster_amd import geotiff, streaming
    S = args.file_src
    buf = ctx.alloc(3 * S * S * 2)
    try:
        ctx.synth_raster(buf, 3, S, S, seed=4321)
        planes = np.empty((3, S, S), dtype=np.int16)
        buf.download(out=planes)
    finally:
        buf.close()
    tr = geotiff.Affine(1.0, 0.0, 0.0, 0.0, -1.0, float(S))
    kw = dict(tile_size=1024, ctx=ctx, overviews=True, stats=True)
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        runs = []
        for rep in range(3):  # the first repetition warms up; multi and singles alternate
            t0 = time.perf_counter()
            streaming.create_streaming_bands_array(planes, [1, 2, 3], tr, "EPSG:32613", d / "multi.flac", **kw)
            t1 = time.perf_counter()
            for b in range(3):
                streaming.create_streaming_array(planes[b], tr, "EPSG:32613", d / f"band{b + 1}.flac", **kw)
            t2 = time.perf_counter()
            runs.append((t1 - t0, t2 - t1))
        sizes = [(d / f"band{b}.flac").stat().st_size for b in (1, 2, 3)]
        multi = (d / "multi.flac").stat().st_size
    res = {"planes": [3, S, S], "tile_size": 1024, "overviews": True, "stats": True,
           "multi_band_wall_s": [round(a, 4) for a, _ in runs[1:]],
           "three_single_band_wall_s": [round(b, 4) for _, b in runs[1:]],
           "multi_band_file_bytes": multi, "single_band_file_bytes": sizes,
           "growth_per_added_band_bytes": round((multi - sizes[0]) / 2.0, 1)}
    print(json.dumps(res), flush=True)
    out["create_streaming"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, default=16384)
    ap.add_argument("--dst", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--file-src", type=int, default=8192)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "composite_probe.json"))
    args = ap.parse_args()
    from flac_raster_amd import _native
    ctx = _native.Context(0)
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    out = {"library_sha256_16": sha}
    render_part(ctx, args, out)
    if args.file_src > 0:
        file_part(ctx, args, out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
