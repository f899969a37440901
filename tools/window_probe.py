#!/usr/bin/env python3
"""Window-resample probe: device time of frs_resample_window_device next to the pyramid step that moves the same
bytes, and the wall time of streaming.read_window next to the mosaic read it replaces.

Kernel part.  A C3-size int16 band (16384 x 16384, the synthetic DEM of frs_synth_raster_device) is resampled
  * as a whole onto 8192 x 8192 (an exact 2x reduction), in all three modes,
  * from a fractional rectangle of it (a quarter of the raster, off the pixel grid) onto 256 x 256, in all three modes,
each timed with HIP events on the context stream (frs_profile_avg_ms("resample")) over --reps calls after --warmup
warm-ups.  In the same process k_downsample2's average on 16384^2 -> 8192^2 is timed the same way ("pyramid"): it is
the yardstick for equal bytes, and the ratio resample / pyramid is reported per mode.

End-to-end part (--e2e): a C3-size file with overviews is written under /tmp, then a 256 x 256 view of a quarter of the
raster is read with read_window and, for the same bbox, with extract_bbox_mosaic(level=pick_level(...)) -- the level a
caller limited to 256 pixels would have picked by hand; medians of --rounds wall times after one warm-up of each, and
the bytes each downloads from the device.

Nodata part (--nodata, instead of the two above): 16384^2 -> 8192^2 in each mode by k_resample_window and by
k_resample_window_nodata on the same nodata-free band (nodata -9999, which the band does not hold), alternated three
times in this call, and the masked kernel on the band with about 30 % of its pixels set to -9999; medians and ratios,
written to profiles/window_nodata_probe.json.

Writes profiles/window_probe.json, stamped with the library hash.

usage: window_probe.py [--reps N] [--warmup N] [--e2e] [--rounds N] [--no-kernel] [--nodata] [--out PATH]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]

HBM_ACHIEVABLE = 6.29e12  # bytes/s, measured achievable rate of the MI355X
H = W = 16384
TILE = 512
MODES = ("nearest", "bilinear", "average")


def _timed(ctx, entry, reps, warmup, call):
    ctx.profile(False)
    for _ in range(warmup):
        call()
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall_ms = (time.perf_counter() - t0) * 1e3 / reps
    return ctx.profile_avg_ms(entry), wall_ms


def kernel_cases(args, out):
    from flac_raster_amd import _native
    ctx = _native.Context(0)
    src = ctx.alloc(H * W * 2)
    half = ctx.alloc((H // 2) * (W // 2) * 2)
    small = ctx.alloc(256 * 256 * 2)
    ctx.synth_raster(src, 1, H, W, seed=1234)
    sd = ctx.make_raster_desc(H, W, np.int16)
    hd = ctx.make_raster_desc(H // 2, W // 2, np.int16)
    md = ctx.make_raster_desc(256, 256, np.int16)
    ms, wall = _timed(ctx, "pyramid", args.reps, args.warmup,
                      lambda: ctx.downsample2_device(src.ptr, sd, half.ptr, hd, "average"))
    moved = H * W * 2 + (H // 2) * (W // 2) * 2
    yard = {"case": "downsample2_average_16384_to_8192", "kernel_ms": round(ms, 4), "call_wall_ms": round(wall, 4),
            "bytes_read_plus_written": moved, "fraction_of_achievable": round(moved / (ms * 1e-3) / HBM_ACHIEVABLE, 4)}
    print(json.dumps(yard), flush=True)
    out["cases"].append(yard)
    frac = (4096.37, 2048.61, 8192.5, 8191.25)  # a quarter of the raster, off the pixel grid: 32x per axis
    for mode in MODES:
        ms2, wall = _timed(ctx, "resample", args.reps, args.warmup,
                           lambda: ctx.resample_window_device(src.ptr, sd, half.ptr, hd, (0.0, 0.0, float(W), float(H)),
                                                              mode))
        # nearest touches every other row's lines only; bilinear at an exact 2x reads all four pixels of each block
        read = H * W * 2 if mode != "nearest" else (H // 2) * W * 2
        mv = read + (H // 2) * (W // 2) * 2
        row = {"case": "resample_16384_to_8192", "mode": mode, "kernel_ms": round(ms2, 4),
               "call_wall_ms": round(wall, 4), "bytes_read_plus_written": mv,
               "fraction_of_achievable": round(mv / (ms2 * 1e-3) / HBM_ACHIEVABLE, 4),
               "ratio_to_downsample2_average": round(ms2 / ms, 3)}
        print(json.dumps(row), flush=True)
        out["cases"].append(row)
    for mode in MODES:
        ms3, wall = _timed(ctx, "resample", args.reps, args.warmup,
                           lambda: ctx.resample_window_device(src.ptr, sd, small.ptr, md, frac, mode))
        row = {"case": "resample_fractional_quarter_to_256", "mode": mode, "rect": list(frac),
               "kernel_ms": round(ms3, 4), "call_wall_ms": round(wall, 4)}
        print(json.dumps(row), flush=True)
        out["cases"].append(row)
    for b in (src, half, small):
        b.close()
    ctx.close()


def nodata_cases(args, out):
    from flac_raster_amd import _native
    ND = -9999
    ctx = _native.Context(0)
    src, holes, half = ctx.alloc(H * W * 2), ctx.alloc(H * W * 2), ctx.alloc((H // 2) * (W // 2) * 2)
    ctx.synth_raster(src, 1, H, W, seed=1234)
    rows = 2048  # one random mask of `rows` rows, applied slab by slab
    mask = np.random.default_rng(7).random((rows, W)) < 0.3
    slab = np.empty((rows, W), np.int16)
    for r0 in range(0, H, rows):
        src.download(slab.nbytes, r0 * W * 2, out=slab.reshape(-1).view(np.uint8))
        assert not (slab == ND).any()
        slab[mask] = ND
        holes.upload(slab, r0 * W * 2)
    del slab, mask
    sd = ctx.make_raster_desc(H, W, np.int16)
    hd = ctx.make_raster_desc(H // 2, W // 2, np.int16)
    rect = (0.0, 0.0, float(W), float(H))
    out["nodata"] = {"case": "16384 x 16384 int16 -> 8192 x 8192", "nodata": ND, "modes": {}}
    for mode in MODES:
        runs = {"unmasked": [], "masked_nodata_free": [], "masked_30_percent_nodata": []}
        for _ in range(3):
            for key, buf, nd in (("unmasked", src, None), ("masked_nodata_free", src, ND),
                                 ("masked_30_percent_nodata", holes, ND)):
                ms, _w = _timed(ctx, "resample", args.reps, args.warmup,
                                lambda: ctx.resample_window_device(buf.ptr, sd, half.ptr, hd, rect, mode, ND, nodata=nd))
                runs[key].append(ms)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        row = {"kernel_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
               "kernel_ms_median": {k: round(v, 4) for k, v in med.items()},
               "masked_nodata_free_over_unmasked": round(med["masked_nodata_free"] / med["unmasked"], 4),
               "masked_30_percent_over_unmasked": round(med["masked_30_percent_nodata"] / med["unmasked"], 4)}
        print(json.dumps({"mode": mode, **row}), flush=True)
        out["nodata"]["modes"][mode] = row
    for b in (src, holes, half):
        b.close()
    ctx.close()


def end_to_end(args, out):
    from flac_raster_amd import _native, geotiff, streaming
    ctx = _native.Context(0)
    d = ctx.alloc(H * W * 2)
    ctx.synth_raster(d, 1, H, W, seed=1234)
    band = np.empty((H, W), np.int16)
    d.download(band.nbytes, 0, out=band.reshape(-1).view(np.uint8))
    d.close()
    t = geotiff.Affine(0.001, 0.0, -106.0, 0.0, -0.001, 41.0)
    path = Path("/tmp/window_probe_streaming.flac")
    index = streaming.create_streaming_array(band, t, "EPSG:4326", path, TILE, ctx, overviews=True)
    del band
    # a quarter of the raster, off the pixel grid
    c0, r0 = 4096.37, 2048.61
    bbox = [t.c + c0 * t.a, t.f + (r0 + H / 2) * t.e, t.c + (c0 + W / 2) * t.a, t.f + r0 * t.e]
    req = streaming.window_request(index, bbox, 256, 256)
    lvl = streaming.pick_level(index, W // 2, H // 2, 256)
    runs = {"read_window": [], "mosaic": []}
    shapes = {}
    for rnd in range(-1, args.rounds):  # round -1 warms both paths up
        t0 = time.perf_counter()
        arr, _ = streaming.read_window(path, bbox, 256, 256, "average", ctx=ctx)
        t1 = time.perf_counter()
        mos, _, _ = streaming.extract_bbox_mosaic(path, bbox, ctx, level=lvl)
        t2 = time.perf_counter()
        shapes = {"read_window": list(arr.shape), "mosaic": list(mos.shape)}
        if rnd >= 0:
            runs["read_window"].append(t1 - t0)
            runs["mosaic"].append(t2 - t1)
    path.unlink()
    ctx.close()
    e = {"band": f"{H} x {W} int16, tile {TILE}, levels {streaming.overview_levels(index)}", "bbox": bbox,
         "read_window": {"level": req["level"], "tiles": len(req["frames"]),
                         "tile_bytes_fetched": sum(f["byte_size"] for f in req["frames"]),
                         "decoded_window": [req["window"]["height"], req["window"]["width"]], "shape": shapes["read_window"],
                         "bytes_downloaded": int(np.prod(shapes["read_window"])) * 2,
                         "wall_ms_median": round(float(np.median(runs["read_window"])) * 1e3, 3),
                         "wall_ms": [round(v * 1e3, 3) for v in runs["read_window"]]},
         "mosaic": {"level": lvl, "shape": shapes["mosaic"], "bytes_downloaded": int(np.prod(shapes["mosaic"])) * 2,
                    "wall_ms_median": round(float(np.median(runs["mosaic"])) * 1e3, 3),
                    "wall_ms": [round(v * 1e3, 3) for v in runs["mosaic"]]}}
    print(json.dumps(e), flush=True)
    out["end_to_end"] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-kernel", action="store_true", help="skip the kernel part")
    ap.add_argument("--e2e", action="store_true", help="also time read_window against the mosaic read")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nodata", action="store_true",
                    help="time the masked kernel beside the unmasked one instead (profiles/window_nodata_probe.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("window_nodata_probe.json" if args.nodata else "window_probe.json"))
    sys.path.insert(0, str(ROOT))
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    out = {"library_sha256_16": sha, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "reps": args.reps,
           "warmup": args.warmup, "tile": TILE, "cases": []}
    if args.nodata:
        nodata_cases(args, out)
    elif not args.no_kernel:
        kernel_cases(args, out)
    if args.e2e and not args.nodata:
        end_to_end(args, out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
