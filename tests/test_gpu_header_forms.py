"""Sample rates without a code of their own (RFC 9639 9.1.2: kHz in 8 bits, Hz in 16, Hz / 10 in 16) through every
encode path: the frame headers then carry one or two more bytes after the frame number, which moves every later bit
of the frame.  Each tile's frames are compared byte for byte with the oracle's at the same rate."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILE = 64
RATES = [37000, 44110, 44101]  # kHz form (code 12), Hz / 10 form (14), Hz form (13)
# (bands, dtype, bits_per_sample, fast path expected)
PATHS = {
    "mono_fast": (1, np.int16, 16, True),
    "mc3_fast": (3, np.int16, 16, True),
    "stereo_fast": (2, np.int16, 16, True),
    "i32_generic": (1, np.int32, 24, False),
}
# 128 x 128: four tiles of one 4096-sample frame; 96 x 64: the second tile is a 2048-sample partial frame, coded by the
# generic kernels inside the fast paths
SHAPES = [(128, 128), (96, 64)]


def _raster(bands, H, W, dtype):
    rng = np.random.default_rng(bands * 1000 + H)
    t = np.arange(bands * H * W).reshape(bands, H, W)
    a = 1500 + 700 * np.sin(t / 23.0) + 90 * np.sin(t / 3.1) + rng.integers(0, 25, t.shape)
    a[1:] += 0.5 * a[:1]  # correlated bands: side / mid signals worth coding
    return (a * (4000 if np.dtype(dtype).itemsize == 4 else 1)).astype(dtype)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("path", list(PATHS))
def test_extended_sample_rate_headers_match_oracle(gpu_ctx, path, rate, shape):
    bands, dtype, bits, fast = PATHS[path]
    H, W = shape
    arr = _raster(bands, H, W, dtype)
    d = gpu_ctx.make_desc(H, W, dtype, nbands=bands, tile_h=TILE, tile_w=TILE, sample_rate=rate, bits_per_sample=bits)
    gpu_ctx.profile(True)
    gpu_ctx.profile_reset()
    arena, off, mn, mx, bps = gpu_ctx.encode_tiles_host(arr if bands > 1 else arr[0], d)
    compact_ms = gpu_ctx.profile_avg_ms("compact")
    gpu_ctx.profile(False)
    assert (compact_ms < 0) == fast, f"{path}: took the {'generic' if fast else 'fast'} kernels"
    data = arena.tobytes()
    ti = 0
    for r0 in range(0, H, TILE):
        for c0 in range(0, W, TILE):
            tile = arr[:, r0:r0 + TILE, c0:c0 + TILE]
            pcm, omn, omx, obps = O.normalize(np.ascontiguousarray(tile.transpose(1, 2, 0)).reshape(-1, bands))
            ref = O.encode_frames(pcm, obps, rate)
            assert bps == obps and mn[ti] == omn and mx[ti] == omx, (path, rate, ti)
            got = data[int(off[ti]):int(off[ti + 1])]
            assert got[:16] == ref[:16], f"{path} rate {rate} tile {ti}: header {got[:16].hex()} != {ref[:16].hex()}"
            assert got == ref, (path, rate, ti)
            ti += 1
    assert ti + 1 == len(off) and int(off[-1]) == len(data)
