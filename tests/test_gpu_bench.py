"""bench.py's N > 1 line rehearsed on one GPU (the tile loop cli.py:690-763 sharded by tile rows).

The driver runs `bench.py --gpus N` on an 8-GPU node; this box has one GPU, so two ranks share it over the host
exchange (FRS_COMM_BACKEND=tcp).  The line must carry n_gpus, the all-gather figures reported apart from the
encode, and the same compressed bytes as the single-rank run of the same raster (the shards are the same tiles).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
SIZE = ["--height", "4096", "--width", "4096", "--steps", "3", "--warmup", "1"]
ARGS = [*SIZE, "--full", "--no-extras", "--no-cpu", "--queries", "50"]


def _bench(gpus: int, args=ARGS) -> dict:
    env = dict(os.environ, FRS_COMM_BACKEND="tcp", FRS_COMM_TIMEOUT="60")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", str(ROOT / "bench.py"), "--gpus", str(gpus), *args], env=env,
                       capture_output=True, text=True, timeout=240, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_two_ranks_reports_allgather_and_same_bytes():
    one = _bench(1)
    two = _bench(2)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert "allgather_us" not in one
    ag = two["allgather_us"]
    for k in ("in_step", "isolated"):
        assert set(ag[k]) == {"mean", "max", "p50"} and ag[k]["mean"] > 0 and ag[k]["max"] >= ag[k]["p50"]
    assert ag["steps"] == 3
    assert two["config"]["compressed_bytes_total"] == one["config"]["compressed_bytes_total"] > 0
    assert two["config"]["tiles"] == one["config"]["tiles"] == 64
    assert two["bbox_extract"]["queries"] == one["bbox_extract"]["queries"] == 50
    assert two["bbox_extract"]["lossless"] and one["bbox_extract"]["lossless"]


@pytest.mark.gpu
def test_plain_run_times_only_the_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """Without --full the line carries the headline figures and none of the other legs; --dump-outputs writes the
    last step's return values (float64 / float32 arrays, 64 tiles), identical from run to run."""
    lines = [_bench(1, [*SIZE, "--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for r in lines:
        assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["unit"] == "Mpixels/s" and r["dtype"] == "int16"
        # value is the raster's pixels over the step time (ms_per_step is rounded to 1 us of a step of ~0.1 ms or more)
        assert r["value"] == pytest.approx(4096 * 4096 / (r["ms_per_step"] * 1e-3) / 1e6, rel=0.01)
        assert not {"bbox_extract", "cpu_baseline", "end_to_end", "batched_decode", "allgather_us"} & set(r)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["frames_sample.npy", "tile_bytesum.npy", "tile_max.npy", "tile_min.npy", "tile_off.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n].dtype in (np.float32, np.float64)
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n)), n
    off = a["tile_off.npy"]
    assert off.shape == (65,) and off[0] == 0 and np.all(np.diff(off) > 0)
    assert off[-1] == lines[0]["config"]["compressed_bytes_total"]
    assert a["tile_bytesum.npy"].shape == a["tile_min.npy"].shape == a["tile_max.npy"].shape == (64,)
    assert np.all(a["tile_min.npy"] <= a["tile_max.npy"])
    # 16 seeded tiles, whole or their first 512 KiB; every FLAC frame starts with the sync code 0xFFF8
    assert 0 < a["frames_sample.npy"].size <= 16 * (512 << 10)
    assert list(a["frames_sample.npy"][:2]) == [0xFF, 0xF8]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 << 20
