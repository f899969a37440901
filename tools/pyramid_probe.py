#!/usr/bin/env python3
"""Pyramid-kernel probe: device time of every level of frs_downsample2_device on the benchmark sizes, and the host wall
time of create_streaming_array with and without overviews.

Kernel part.  A device band filled with the synthetic DEM (frs_synth_raster_device) is reduced level by level, level
k from level k - 1, down to the level that fits one 512-px tile; each level's launch is timed with HIP events on the
context stream (frs_profile_avg_ms("pyramid")) over --reps calls after --warmup warm-ups.  Cases: one int16 band at C3
size (16384 x 16384) and at C4 size (40000 x 40000), and C3's bytes read as uint8 (16384 x 32768) and as float32
(16384 x 8192); every case in both resampling modes.  Prints, and writes to profiles/pyramid_probe.json: milliseconds
per level and, for levels of at least 64 MiB moved, (bytes read + bytes written) per second as a fraction of the
6.29 TB/s achievable HBM rate (smaller levels are launch-bound: their times are reported, not their rates).

End-to-end part (--e2e): streaming.create_streaming_array of a C3 int16 band (device-synthesised, downloaded once)
into a file under /tmp, without and with overviews, alternated --rounds times in this process after one warm-up of
each; medians of the wall time and of the stage timings.

Nodata part (--nodata, instead of the two above): the C4 level-0 step (40000 x 40000 int16, average) by k_downsample2
and by k_downsample2_nodata on the same nodata-free band (nodata -9999, which the band does not hold), alternated
--rounds times in this call, and the masked kernel on the band with about 30 % of its pixels set to -9999.  Written to
profiles/pyramid_nodata_probe.json with the ratio of the medians (the bar: masked on nodata-free input <= 1.15 x
unmasked).

usage: pyramid_probe.py [--cases c3,c4,c3_u8,c3_f32] [--reps N] [--warmup N] [--e2e] [--rounds N] [--nodata]
                        [--out PATH]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]

HBM_ACHIEVABLE = 6.29e12  # bytes/s, measured achievable rate of the MI355X
RATE_FLOOR = 64 << 20     # levels moving fewer bytes are launch-bound: no rate

CASES = {  # name: (dtype, height, width)
    "c3": (np.int16, 16384, 16384),
    "c4": (np.int16, 40000, 40000),
    "c3_u8": (np.uint8, 16384, 32768),
    "c3_f32": (np.float32, 16384, 8192),
}
TILE = 512


def kernel_cases(args, out):
    from flac_raster_amd import _native, streaming
    ctx = _native.Context(0)
    for name in args.cases.split(","):
        dtype, H, W = CASES[name]
        es = np.dtype(dtype).itemsize
        shapes = [(H, W)] + streaming.overview_shapes(H, W, TILE)
        bufs = [ctx.alloc(h * w * es) for h, w in shapes]
        # the synthetic DEM is int16: the other dtypes read the same bytes
        ctx.synth_raster(bufs[0], 1, H, W * es // 2, seed=1234)
        for mode in ("average", "nearest"):
            for k in range(1, len(shapes)):
                (sh, sw), (dh, dw) = shapes[k - 1], shapes[k]
                sd = ctx.make_raster_desc(sh, sw, dtype)
                ctx.profile(False)
                for _ in range(args.warmup):
                    ctx.downsample2_device(bufs[k - 1].ptr, sd, bufs[k].ptr, mode=mode)
                ctx.profile(True)
                ctx.profile_reset()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    ctx.downsample2_device(bufs[k - 1].ptr, sd, bufs[k].ptr, mode=mode)
                wall_ms = (time.perf_counter() - t0) * 1e3 / args.reps
                ms = ctx.profile_avg_ms("pyramid")
                # nearest reads every other element of every other row; the lines it touches are the even rows' lines
                read = sh * sw * es if mode == "average" else ((sh + 1) // 2) * sw * es
                moved = read + dh * dw * es
                row = {"case": name, "dtype": np.dtype(dtype).name, "mode": mode, "level": k, "source": [sh, sw],
                       "destination": [dh, dw], "bytes_read_plus_written": moved, "kernel_ms": round(ms, 4),
                       "call_wall_ms": round(wall_ms, 4)}
                if moved >= RATE_FLOOR:
                    rate = moved / (ms * 1e-3)
                    row.update(bytes_per_s=rate, fraction_of_achievable=round(rate / HBM_ACHIEVABLE, 4))
                print(json.dumps(row), flush=True)
                out["cases"].append(row)
        for b in bufs:
            b.close()
    ctx.close()


def _timed_step(ctx, args, call):
    ctx.profile(False)
    for _ in range(args.warmup):
        call()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(args.reps):
        call()
    return ctx.profile_avg_ms("pyramid")


def nodata_cases(args, out):
    from flac_raster_amd import _native
    ND = -9999
    ctx = _native.Context(0)
    dtype, H, W = CASES["c4"]
    src, holes, dst = ctx.alloc(H * W * 2), ctx.alloc(H * W * 2), ctx.alloc((H // 2) * (W // 2) * 2)
    ctx.synth_raster(src, 1, H, W, seed=1234)
    # the same band with ~30 % of its pixels nodata: one random mask of `rows` rows, applied slab by slab
    rows = 4000
    mask = np.random.default_rng(7).random((rows, W)) < 0.3
    slab = np.empty((rows, W), np.int16)
    for r0 in range(0, H, rows):
        src.download(slab.nbytes, r0 * W * 2, out=slab.reshape(-1).view(np.uint8))
        assert not (slab == ND).any()
        slab[mask] = ND
        holes.upload(slab, r0 * W * 2)
    del slab, mask
    sd = ctx.make_raster_desc(H, W, dtype)
    moved = H * W * 2 + (H // 2) * (W // 2) * 2
    runs = {"unmasked": [], "masked_nodata_free": [], "masked_30_percent_nodata": []}
    for rnd in range(args.rounds):
        runs["unmasked"].append(_timed_step(ctx, args, lambda: ctx.downsample2_device(src.ptr, sd, dst.ptr)))
        runs["masked_nodata_free"].append(
            _timed_step(ctx, args, lambda: ctx.downsample2_device(src.ptr, sd, dst.ptr, nodata=ND)))
        runs["masked_30_percent_nodata"].append(
            _timed_step(ctx, args, lambda: ctx.downsample2_device(holes.ptr, sd, dst.ptr, nodata=ND)))
        print(json.dumps({"round": rnd, **{k: round(v[-1], 4) for k, v in runs.items()}}), flush=True)
    for b in (src, holes, dst):
        b.close()
    ctx.close()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    out["nodata"] = {"case": "c4 level-0 step, 40000 x 40000 int16, average", "nodata": ND,
                     "bytes_read_plus_written": moved, "kernel_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                     "kernel_ms_median": {k: round(v, 4) for k, v in med.items()},
                     "fraction_of_achievable": {k: round(moved / (v * 1e-3) / HBM_ACHIEVABLE, 4) for k, v in med.items()},
                     "masked_nodata_free_over_unmasked": round(med["masked_nodata_free"] / med["unmasked"], 4),
                     "masked_30_percent_over_unmasked": round(med["masked_30_percent_nodata"] / med["unmasked"], 4),
                     "bar": 1.15}
    print(json.dumps(out["nodata"]), flush=True)


def end_to_end(args, out):
    from flac_raster_amd import _native, geotiff, streaming
    ctx = _native.Context(0)
    _, H, W = CASES["c3"]
    d = ctx.alloc(H * W * 2)
    ctx.synth_raster(d, 1, H, W, seed=1234)
    band = np.empty((H, W), np.int16)
    d.download(band.nbytes, 0, out=band.reshape(-1).view(np.uint8))
    d.close()
    t = geotiff.Affine(0.001, 0.0, -106.0, 0.0, -0.001, 41.0)
    path = Path("/tmp/pyramid_probe_streaming.flac")
    runs = []
    for rnd in range(-1, args.rounds):  # round -1 warms both paths up
        for ov in (False, True):
            tm = {}
            t0 = time.perf_counter()
            index = streaming.create_streaming_array(band, t, "EPSG:4326", path, TILE, ctx, tm, overviews=ov)
            wall = time.perf_counter() - t0
            r = {"round": rnd, "overviews": ov, "wall_s": round(wall, 4), "file_bytes": path.stat().st_size,
                 "levels": len(streaming.overview_levels(index)) - 1}
            r.update({k: round(v, 4) for k, v in tm.items()})
            print(json.dumps(r), flush=True)
            if rnd >= 0:
                runs.append(r)
    path.unlink()
    ctx.close()
    e = {"band": f"{H} x {W} int16, tile {TILE}", "runs": runs}
    for ov, label in ((False, "plain"), (True, "overviews")):
        sel = [r for r in runs if r["overviews"] == ov]
        for key in ("wall_s", "encode_s", "pyramid_s", "index_s", "write_s"):
            vals = [r[key] for r in sel if key in r]
            if vals:
                e[f"{key}_{label}_median"] = round(float(np.median(vals)), 4)
        e[f"file_bytes_{label}"] = sel[0]["file_bytes"]
    out["end_to_end"] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c4,c3_u8,c3_f32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e", action="store_true", help="also time create_streaming_array with and without overviews")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodata", action="store_true",
                    help="time the masked step beside the unmasked one instead (profiles/pyramid_nodata_probe.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("pyramid_nodata_probe.json" if args.nodata else "pyramid_probe.json"))
    sys.path.insert(0, str(ROOT))
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    out = {"library_sha256_16": sha, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "reps": args.reps,
           "warmup": args.warmup, "tile": TILE, "cases": []}
    if args.nodata:
        nodata_cases(args, out)
    elif args.cases:
        kernel_cases(args, out)
    if args.e2e and not args.nodata:
        end_to_end(args, out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
