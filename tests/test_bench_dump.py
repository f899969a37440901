"""bench.py --dump-outputs: the files written for a step's outputs, checked on the host against a stand-in arena."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


class Arena:
    """What dump_outputs uses of a DeviceBuffer: download(nbytes, offset) -> uint8 array."""

    def __init__(self, data):
        self.data = data

    def download(self, nbytes, offset=0):
        assert 0 <= offset and offset + nbytes <= len(self.data)
        return self.data[offset:offset + nbytes].copy()


@pytest.mark.parametrize("chunk", [1, 1000, 1 << 20])  # a tile per group, several tiles per group, one group
def test_dump_outputs_files(tmp_path, chunk):
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 700, size=37)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = rng.integers(0, 256, size=int(off[-1]) + 50, dtype=np.uint8)  # (the arena is larger than its frames)
    tmin, tmax = rng.normal(size=37), rng.normal(size=37) + 10
    bench.dump_outputs(tmp_path, Arena(data), off, tmin, tmax, 0, sample_tiles=5, sample_bytes=300, chunk=chunk)
    got = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert sorted(got) == ["frames_sample", "tile_bytesum", "tile_max", "tile_min", "tile_off"]
    assert all(a.dtype == (np.float32 if k == "frames_sample" else np.float64) for k, a in got.items())
    assert np.array_equal(got["tile_off"], off) and np.array_equal(got["tile_min"], tmin)
    assert np.array_equal(got["tile_max"], tmax)
    want = [int(data[off[i]:off[i + 1]].sum(dtype=np.int64)) for i in range(37)]
    assert np.array_equal(got["tile_bytesum"], want)
    picks = np.sort(np.random.default_rng(20240607).choice(37, size=5, replace=False))
    sample = np.concatenate([data[off[t]:off[t] + min(sizes[t], 300)] for t in picks])
    assert np.array_equal(got["frames_sample"], sample)


def test_dump_outputs_other_rank_and_no_tiles(tmp_path):
    bench.dump_outputs(tmp_path, Arena(np.zeros(1, np.uint8)), np.zeros(1, np.int64), np.zeros(0), np.zeros(0), 2)
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"{n}_rank2.npy" for n in (
        "frames_sample", "tile_bytesum", "tile_max", "tile_min", "tile_off")]
    assert np.load(tmp_path / "frames_sample_rank2.npy").size == 0
