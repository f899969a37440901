#!/usr/bin/env python3
"""Statistics probe: device time of frs_band_stats_device and frs_band_histogram_device on one 40000 x 40000 int16 band
(3.2 GB) that is resident in device memory.

Three inputs: the synthetic DEM band (frs_synth_raster_device), a constant band (every lane of every wave adds to the
same LDS counter: the worst case for the histogram), and the DEM band with a 2000-pixel nodata collar.  Each is timed
without and with a nodata value: the first pass, the second pass at 256 bins over the band's [min, max] and at 16384
bins over [-8192, 8192] (scale 1: a bin per value).  Kernel times come from HIP events on the context stream
(frs_profile_avg_ms("band_stats" / "band_hist"; the latter includes the slab reduction) after warm-up.  Both passes read
the band once, so each time is set against the once-read rate this project measured itself (tools/micro/reread.hip:
3.2 GB in 0.537 ms).  Prints, and writes to profiles/stats_probe.json.

usage: stats_probe.py [--size N] [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ONCE_READ = 3.2e9 / 0.537e-3  # bytes/s: tools/micro/reread.hip, 3.2 GB read once in 0.537 ms
NODATA = -9999
COLLAR = 2000


def fill_rows(buf, width, row0, row1, value):
    """rows [row0, row1) of the int16 band in `buf` := value"""
    step = 1024
    chunk = np.full((step, width), value, dtype=np.int16)
    for r in range(row0, row1, step):
        n = min(step, row1 - r)
        buf.upload(chunk[:n], offset=r * width * 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stats_probe.json"))
    args = ap.parse_args()
    from flac_raster_amd import _native
    N = args.size
    nbytes = N * N * 2
    collar = min(COLLAR, N // 8)
    ctx = _native.Context(0)
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    desc = ctx.make_raster_desc(N, N, np.int16)
    items = _native.stats_items(N, N, 2)
    out = {"library_sha256_16": sha, "once_read_bytes_per_s": ONCE_READ, "shape": [1, N, N], "dtype": "int16",
           "bytes_read": nbytes, "reps": args.reps, "nodata": NODATA, "collar_pixels": collar,
           "groups_per_band": {"band_stats": _native.stats_groups(items, 1),
                               "band_hist": _native.stats_groups(items, 1, _native.HIST_BLOCK, _native.HIST_UNROLL,
                                                                 _native.HIST_MAX_GROUPS)},
           "cases": []}
    buf = ctx.alloc(nbytes)
    try:
        for name in ("synth", "constant", "collar"):
            if name == "constant":
                fill_rows(buf, N, 0, N, 1000)
            else:
                ctx.synth_raster(buf, 1, N, N, seed=1234)
            if name == "collar":
                fill_rows(buf, N, 0, collar, NODATA)
                fill_rows(buf, N, N - collar, N, NODATA)
                side = np.full(collar, NODATA, dtype=np.int16)
                for r in range(collar, N - collar):
                    buf.upload(side, offset=(r * N) * 2)
                    buf.upload(side, offset=(r * N + N - collar) * 2)
            for nd in (None, NODATA):
                st = ctx.band_stats_device(buf.ptr, desc, nodata=nd)[0]
                lo, hi = float(st["min"]), float(st["max"])
                if hi == lo:
                    hi = lo + 1.0
                passes = [("band_stats", None), ("band_hist", (lo, hi, 256)), ("band_hist", (-8192.0, 8192.0, 16384))]
                for kernel, hp in passes:
                    def call():
                        if hp is None:
                            return ctx.band_stats_device(buf.ptr, desc, nodata=nd)
                        return ctx.band_histogram_device(buf.ptr, desc, hp[0], hp[1], hp[2], nodata=nd)
                    ctx.profile(False)
                    for _ in range(args.warmup):
                        res = call()
                    ctx.profile(True)
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        call()
                    wall_ms = (time.perf_counter() - t0) * 1e3 / args.reps
                    ms = ctx.profile_avg_ms(kernel)
                    rate = nbytes / (ms * 1e-3)
                    row = {"input": name, "nodata": nd, "pass": kernel, "nbins": None if hp is None else hp[2],
                           "range": None if hp is None else [hp[0], hp[1]], "kernel_ms": round(ms, 4),
                           "call_wall_ms": round(wall_ms, 4), "bytes_per_s": rate,
                           "fraction_of_once_read": round(rate / ONCE_READ, 4), "n_valid": int(st["n_valid"]),
                           "n_nodata": int(st["n_nodata"])}
                    if hp is not None:
                        counts, ho = res
                        row["counted"] = int(counts.sum()) + ho[0]["below"] + ho[0]["above"]
                        row["bins_in_use"] = int((counts > 0).sum())
                    print(json.dumps(row), flush=True)
                    out["cases"].append(row)
    finally:
        buf.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
