#!/usr/bin/env python3
"""Compare-kernel probe: device time of frs_compare_device on the benchmark sizes.

Two device rasters are filled with the synthetic DEM (frs_synth_raster_device): with the same seed for the equal
case, with different seeds for the unequal one.  The kernel is timed with HIP events on the context stream
(frs_profile_avg_ms("compare")) after warm-up.  Cases: C3 (16384 x 16384 x 4 int16), C4 (40000 x 40000 x 4 int16),
and the C3 buffers' bytes read as uint8 (16384 x 32768 x 4) and as float32 (16384 x 8192 x 4), so every case of a
size moves the same bytes.  Prints, and writes to profiles/compare_probe.json: milliseconds, bytes read per
millisecond as a fraction of the 6.29 TB/s achievable HBM read rate, and the wall time of the reference's numpy
expressions (compare.py:55-64) on a 4 x 8192 x 8192 int16 slice on this host.

usage: compare_probe.py [--cases c3,c4,u8,f32] [--reps N] [--warmup N] [--no-numpy] [--out PATH]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_ACHIEVABLE = 6.29e12  # bytes/s, measured achievable read rate of the MI355X

CASES = {  # name: (bands, height, width as synthesised int16, dtype compared, width in that dtype)
    "c3": (4, 16384, 16384, np.int16, 16384),
    "c4": (4, 40000, 40000, np.int16, 40000),
    "u8": (4, 16384, 16384, np.uint8, 32768),
    "f32": (4, 16384, 16384, np.float32, 8192),
}


def numpy_reference_seconds(ctx) -> float:
    """Wall time of the reference's whole-raster expressions on a 4 x 8192 x 8192 int16 pair (this host's CPU)."""
    B, H, W = 4, 8192, 8192
    bufs = []
    for seed in (1234, 4321):
        d = ctx.alloc(B * H * W * 2)
        ctx.synth_raster(d, B, H, W, seed=seed)
        h = np.empty((B, H, W), np.int16)
        d.download(h.nbytes, 0, out=h.reshape(-1).view(np.uint8))
        d.close()
        bufs.append(h)
    a, b = bufs
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        res = [np.array_equal(a, b), float(np.max(np.abs(a - b))), float(np.mean(np.abs(a - b))),
               float(np.sqrt(np.mean((a - b) ** 2))), float(np.min(a)), float(np.max(a)), float(np.min(b)),
               float(np.max(b))]
    dt = time.perf_counter() - t0
    print(f"numpy reference on 4x8192x8192 int16: {dt:.2f} s  {res}", flush=True)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c4,u8,f32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "compare_probe.json"))
    args = ap.parse_args()
    from flac_raster_amd import _native
    ctx = _native.Context(0)
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    out = {"library_sha256_16": sha, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "reps": args.reps, "cases": []}
    for name in args.cases.split(","):
        B, H, W16, dtype, W = CASES[name]
        nbytes = B * H * W16 * 2
        a, b, c = ctx.alloc(nbytes), ctx.alloc(nbytes), ctx.alloc(nbytes)
        ctx.synth_raster(a, B, H, W16, seed=1234)
        ctx.synth_raster(b, B, H, W16, seed=1234)
        ctx.synth_raster(c, B, H, W16, seed=4321)
        desc = ctx.make_compare_desc(H, W, dtype, nbands=B)
        for label, other in (("equal", b), ("unequal", c)):
            ctx.profile(False)
            for _ in range(args.warmup):
                bands = ctx.compare_device(a.ptr, other.ptr, desc)
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                ctx.compare_device(a.ptr, other.ptr, desc)
            wall_ms = (time.perf_counter() - t0) * 1e3 / args.reps
            ms = ctx.profile_avg_ms("compare")
            rate = 2 * nbytes / (ms * 1e-3)
            row = {"case": name, "pair": label, "dtype": np.dtype(dtype).name, "shape": [B, H, W],
                   "bytes_read": 2 * nbytes, "kernel_ms": round(ms, 4), "call_wall_ms": round(wall_ms, 4),
                   "bytes_per_s": rate, "fraction_of_achievable": round(rate / HBM_ACHIEVABLE, 4),
                   "n_diff": int(sum(x["n_diff"] for x in bands)),
                   "groups_per_band": _native.compare_groups(H * W, B, np.dtype(dtype).itemsize)}
            print(json.dumps(row), flush=True)
            out["cases"].append(row)
        for x in (a, b, c):
            x.close()
    if not args.no_numpy:
        out["numpy_reference_4x8192x8192_int16_s"] = round(numpy_reference_seconds(ctx), 3)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
