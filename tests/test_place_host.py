"""Host side of the tile placement (frs_place_tiles_device / frs_decode_tiles_window*): the window table built from
index entries, the ctypes layouts against the header, and the CLI's argument rejections.  No GPU."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

from typer.testing import CliRunner

from flac_raster_amd import streaming
from flac_raster_amd._native import RasterDesc, TileWindow, tile_window_array
from flac_raster_amd.cli import app

ROOT = Path(__file__).resolve().parents[1]
runner = CliRunner()


def _frame(fid, col, row, w, h):
    return {"frame_id": fid, "bbox": [0, 0, 1, 1], "window": {"col_off": col, "row_off": row, "width": w, "height": h},
            "byte_offset": 0, "byte_size": 0}


# a 2 x 2 grid of a 300 x 250 raster at tile 200, row-major as create-streaming writes it
FRAMES = [_frame(0, 0, 0, 200, 200), _frame(1, 200, 0, 100, 200), _frame(2, 0, 200, 200, 50),
          _frame(3, 200, 200, 100, 50)]


def test_tile_windows_origin_zero_reproduces_index_windows():
    assert streaming.tile_windows(FRAMES) == [(0, 0, 200, 200), (200, 0, 100, 200), (0, 200, 200, 50),
                                              (200, 200, 100, 50)]
    assert streaming.tile_windows([]) == []


def test_tile_windows_relative_to_an_origin():
    # origin (col 210, row 30): tiles left of / above it get negative offsets, sizes never change
    assert streaming.tile_windows(FRAMES, origin=(210, 30)) == [(-210, -30, 200, 200), (-10, -30, 100, 200),
                                                                (-210, 170, 200, 50), (-10, 170, 100, 50)]


def test_tile_windows_keeps_the_given_order():
    order = [FRAMES[3], FRAMES[0], FRAMES[2]]
    assert streaming.tile_windows(order, origin=(1, 2)) == [(199, 198, 100, 50), (-1, -2, 200, 200),
                                                            (-1, 198, 200, 50)]


def test_tile_window_array_from_rows():
    arr = tile_window_array([(-3, 7, 64, 512), (1 << 40, -(1 << 40), 1, 1)])
    assert (arr[0].col_off, arr[0].row_off, arr[0].width, arr[0].height) == (-3, 7, 64, 512)
    assert (arr[1].col_off, arr[1].row_off) == (1 << 40, -(1 << 40))
    assert tile_window_array(arr) is arr


def test_window_and_raster_desc_layouts_match_header():
    """ctypes TileWindow / RasterDesc against frs_tile_window / frs_raster_desc (sizes and offsets from a C program)."""
    src = ROOT / "include" / "flac_raster_amd.h"
    prog = f'''#include "{src}"
#include <stdio.h>
#include <stddef.h>
int main(void){{printf("%zu %zu %zu %zu %zu\\n", sizeof(frs_tile_window), offsetof(frs_tile_window, col_off),
offsetof(frs_tile_window, row_off), offsetof(frs_tile_window, width), offsetof(frs_tile_window, height));
printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(frs_raster_desc), offsetof(frs_raster_desc, height),
offsetof(frs_raster_desc, width), offsetof(frs_raster_desc, row_stride), offsetof(frs_raster_desc, band_stride),
offsetof(frs_raster_desc, dtype), offsetof(frs_raster_desc, nbands));return 0;}}'''
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(prog)
        subprocess.run(["gcc", "-o", str(Path(d) / "t"), str(c)], check=True)
        out = subprocess.run([str(Path(d) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    T, R = TileWindow, RasterDesc
    assert [int(x) for x in out[0].split()] == [ctypes.sizeof(T), T.col_off.offset, T.row_off.offset, T.width.offset,
                                                T.height.offset]
    assert [int(x) for x in out[1].split()] == [ctypes.sizeof(R), R.height.offset, R.width.offset, R.row_stride.offset,
                                                R.band_stride.offset, R.dtype.offset, R.nbands.offset]


def test_extract_streaming_all_rejects_a_tile_selection(tmp_path):
    # checked before anything is read: the file does not exist
    f, out = str(tmp_path / "missing.flac"), str(tmp_path / "o.tif")
    for sel in (["--bbox", "0,0,1,1"], ["--tile-id", "0"], ["--center"], ["--last"]):
        r = runner.invoke(app, ["extract-streaming", f, "--all", "-o", out] + sel)
        assert r.exit_code == 1 and "--all cannot be combined" in r.output, sel


def test_create_streaming_verify_rejects_multi_gpu_before_the_input_is_opened(tmp_path):
    missing = str(tmp_path / "missing.tif")
    r = runner.invoke(app, ["create-streaming", missing, "--verify", "--gpus", "2"])
    assert r.exit_code == 1 and "--verify runs on one GPU" in r.output and "does not exist" not in r.output
    r = runner.invoke(app, ["create-streaming", missing, "--verify", "--distributed"])
    assert r.exit_code == 1 and "--verify runs on one GPU" in r.output and "does not exist" not in r.output
    # without --verify the same command reaches the input check
    r = runner.invoke(app, ["create-streaming", missing, "--gpus", "2"])
    assert r.exit_code == 1 and "does not exist" in r.output
