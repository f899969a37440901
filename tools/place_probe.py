#!/usr/bin/env python3
"""Placement-kernel probe: device time of frs_place_tiles_device on the benchmark sizes, and the host wall time of the
two paths built on it against another build of the package.

Kernel part.  A device buffer filled with the synthetic DEM (frs_synth_raster_device) is read as tiles and placed into
a second device raster; the kernel is timed with HIP events on the context stream (frs_profile_avg_ms("place")) after
warm-up.  Cases: one int16 band at C3 size (16384 x 16384, tile 512) and at C4 size (40000 x 40000, tile 512: the
64-px edge column and row are in it), each with the destination's origin at the raster's (0, 0) and at (3, 3) (a crop:
every destination row starts off a 16-byte boundary and the tiles overhang it), and four int16 channels at 16384 x
16384, as one tile (what `convert` decodes) and as 512-px tiles.  Prints, and writes to profiles/place_probe.json:
milliseconds and (bytes read + bytes written) per second as a fraction of the 6.29 TB/s achievable HBM rate.

End-to-end part (--e2e OTHER_TREE): streaming.extract_bbox_mosaic over the full extent of an 8192 x 8192 int16, tile
512 streaming file, and RasterFLACConverter.decode_bytes of a 4 x 4096 x 4096 int16 stream, both files written under
/tmp by this tree; each path then runs in a child process on this tree and on OTHER_TREE (a checkout of another commit
with its library built), alternating, --rounds times.  A child times each call with time.perf_counter after one
warm-up call.

usage: place_probe.py [--cases c3,c3_crop,c4,c4_crop,c3x4,c3x4_tiles] [--reps N] [--warmup N] [--e2e OTHER_TREE]
                      [--rounds N] [--out PATH]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]

HBM_ACHIEVABLE = 6.29e12  # bytes/s, measured achievable rate of the MI355X

CASES = {  # name: (channels, height, width, tile or None for one tile, destination origin)
    "c3": (1, 16384, 16384, 512, (0, 0)),
    "c3_crop": (1, 16384, 16384, 512, (3, 3)),
    "c4": (1, 40000, 40000, 512, (0, 0)),
    "c4_crop": (1, 40000, 40000, 512, (3, 3)),
    "c3x4": (4, 16384, 16384, None, (0, 0)),
    "c3x4_tiles": (4, 16384, 16384, 512, (0, 0)),
}


def kernel_cases(args, out):
    from flac_raster_amd import _native, streaming
    ctx = _native.Context(0)
    for name in args.cases.split(","):
        C, H, W, tile, (oc, orow) = CASES[name]
        grid = streaming.tile_grid(H, W, tile) if tile else [(0, 0, W, H)]
        wins = _native.tile_window_array([(c - oc, r - orow, w, h) for c, r, w, h in grid])
        poff = np.zeros(len(grid), dtype=np.int64)
        poff[1:] = np.cumsum([w * h for _, _, w, h in grid])[:-1]
        dh, dw = H - 2 * orow, W - 2 * oc  # a crop: the window (o, o) .. (W - o, H - o)
        src, dst = ctx.alloc(C * H * W * 2), ctx.alloc(C * dh * dw * 2)
        ctx.synth_raster(src, C, H, W, seed=1234)
        desc = ctx.make_raster_desc(dh, dw, np.int16, nbands=C)
        ctx.profile(False)
        for _ in range(args.warmup):
            ctx.place_tiles_device(src.ptr, poff, wins, desc, dst.ptr)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.place_tiles_device(src.ptr, poff, wins, desc, dst.ptr)
        wall_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        ms = ctx.profile_avg_ms("place")
        moved = 2 * C * dh * dw * 2  # every destination element is read once from the tiles and written once
        rate = moved / (ms * 1e-3)
        row = {"case": name, "channels": C, "raster": [H, W], "tile": tile, "ntiles": len(grid),
               "destination": [dh, dw], "origin": [oc, orow], "bytes_read_plus_written": moved,
               "kernel_ms": round(ms, 4), "call_wall_ms": round(wall_ms, 4), "bytes_per_s": rate,
               "fraction_of_achievable": round(rate / HBM_ACHIEVABLE, 4)}
        print(json.dumps(row), flush=True)
        out["cases"].append(row)
        src.close()
        dst.close()
    ctx.close()


MOSAIC_FILE = Path("/tmp/place_probe_8192_streaming.flac")
CONVERT_FILE = Path("/tmp/place_probe_4x4096.flac")


def write_e2e_inputs():
    from flac_raster_amd import _native, geotiff, streaming
    from flac_raster_amd.converter import RasterFLACConverter, raster_metadata
    ctx = _native.Context(0)

    def synth(B, H, W):
        d = ctx.alloc(B * H * W * 2)
        ctx.synth_raster(d, B, H, W, seed=1234)
        h = np.empty((B, H, W), np.int16)
        d.download(h.nbytes, 0, out=h.reshape(-1).view(np.uint8))
        d.close()
        return h
    t = geotiff.Affine(0.001, 0.0, -106.0, 0.0, -0.001, 41.0)
    streaming.create_streaming_array(synth(1, 8192, 8192)[0], t, "EPSG:4326", MOSAIC_FILE, 512, ctx)
    data = synth(4, 4096, 4096)
    conv = RasterFLACConverter(ctx)
    frames, dmin, dmax, sbps, sr = conv.encode_array(data)
    md = raster_metadata(geotiff.GeoRaster(data, t, epsg=4326), dmin, dmax)
    conv.write_flac(CONVERT_FILE, frames, md, 4, sbps, sr)
    ctx.close()
    print(f"wrote {MOSAIC_FILE} ({MOSAIC_FILE.stat().st_size} bytes), {CONVERT_FILE} "
          f"({CONVERT_FILE.stat().st_size} bytes)", flush=True)


def child(tree: str):
    """Runs in a fresh process on the package of `tree`: one warm-up and one timed call of each path."""
    sys.path.insert(0, tree)
    import zlib
    from flac_raster_amd import streaming
    from flac_raster_amd.converter import RasterFLACConverter
    bbox = [-106.0, 41.0 - 8.192, -106.0 + 8.192, 41.0]
    res = {}
    for _ in range(2):
        t0 = time.perf_counter()
        arr, win, _ = streaming.extract_bbox_mosaic(MOSAIC_FILE, bbox)
        res["mosaic_s"] = time.perf_counter() - t0
    res["mosaic_shape"] = list(arr.shape)
    res["mosaic_crc32"] = zlib.crc32(arr)
    del arr
    buf = CONVERT_FILE.read_bytes()
    conv = RasterFLACConverter()
    for _ in range(2):
        t0 = time.perf_counter()
        out, _ = conv.decode_bytes(buf)
        res["decode_bytes_s"] = time.perf_counter() - t0
    res["decode_shape"] = list(out.shape)
    res["decode_crc32"] = zlib.crc32(out)
    print("CHILD " + json.dumps(res), flush=True)


def end_to_end(args, out):
    write_e2e_inputs()
    runs = []
    for rnd in range(args.rounds):
        for label, tree in (("this", str(ROOT)), ("other", str(Path(args.e2e).resolve()))):
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", tree], capture_output=True,
                               text=True, timeout=600)
            line = [x for x in p.stdout.splitlines() if x.startswith("CHILD ")]
            if p.returncode != 0 or not line:
                raise RuntimeError(f"child on {tree} failed ({p.returncode}): {p.stderr[-2000:]}")
            r = json.loads(line[-1][6:])
            r.update(build=label, round=rnd)
            print(json.dumps(r), flush=True)
            runs.append(r)
    out["end_to_end"] = {"mosaic_file": "8192 x 8192 int16, tile 512, full extent",
                         "decode_bytes_stream": "4 x 4096 x 4096 int16", "runs": runs}
    for key in ("mosaic_s", "decode_bytes_s"):
        for label in ("this", "other"):
            out["end_to_end"][f"{key}_{label}_median"] = round(float(np.median([r[key] for r in runs
                                                                                  if r["build"] == label])), 4)
    same = all(r[k] == runs[0][k] for r in runs for k in ("mosaic_crc32", "decode_crc32", "mosaic_shape"))
    out["end_to_end"]["results_identical_across_builds"] = same
    MOSAIC_FILE.unlink()
    CONVERT_FILE.unlink()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c3_crop,c4,c4_crop,c3x4,c3x4_tiles")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e", default=None, help="another checkout (library built) to alternate the end-to-end runs with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "place_probe.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    sys.path.insert(0, str(ROOT))
    lib = ROOT / "flac_raster_amd" / "libflac_raster_amd.so"
    sha = subprocess.run(["sha256sum", str(lib)], capture_output=True, text=True).stdout.split()[0][:16]
    out = {"library_sha256_16": sha, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "reps": args.reps,
           "warmup": args.warmup, "cases": []}
    if args.cases:
        kernel_cases(args, out)
    if args.e2e:
        end_to_end(args, out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
