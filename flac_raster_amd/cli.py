"""flac-raster command line (reference cli.py:15-93, 620-804, 875-1039): convert, create-streaming,
extract-streaming -- same command names, options and defaults; every sample goes through the GPU codec."""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Optional

import typer

app = typer.Typer(name="flac-raster", add_completion=False,
                  help="Convert between TIFF raster and FLAC audio formats while preserving geospatial metadata "
                       "(MI355X codec)")
log = logging.getLogger("flac_raster")


@app.command()
def convert(
    input_file: Path = typer.Argument(..., help="Input file (TIFF or FLAC)"),
    output_file: Optional[Path] = typer.Option(None, "--output", "-o", help="Output file path"),
    compression_level: int = typer.Option(5, "--compression", "-c", min=0, max=8,
                                          help="FLAC compression level (0-8); the GPU encoder implements 0-5 "
                                               "(not 1/4 on two bands) and rejects the others"),
    force: bool = typer.Option(False, "--force", "-f", help="Overwrite existing output file"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose logging"),
    spatial_tiling: bool = typer.Option(False, "--spatial", "-s", help="Enable spatial tiling for HTTP range streaming"),
    tile_size: int = typer.Option(512, "--tile-size", help="Size of spatial tiles (default: 512x512)"),
    verify: bool = typer.Option(False, "--verify", help="Extension: decode the written FLAC and compare it with the "
                                                        "source raster on the GPU (plain TIFF to FLAC only); exit "
                                                        "status 3 when it differs"),
):
    """Convert between TIFF and FLAC formats"""
    from .converter import RasterFLACConverter
    if verbose:
        logging.getLogger("flac_raster").setLevel(logging.DEBUG)
    # --verify is checked before anything else is looked at or done
    if verify and (spatial_tiling or input_file.suffix.lower() not in (".tif", ".tiff")):
        typer.echo("Error: --verify applies to plain TIFF to FLAC conversion", err=True)
        raise typer.Exit(1)
    if not input_file.exists():
        typer.echo(f"Error: Input file does not exist: {input_file}", err=True)
        raise typer.Exit(1)
    suf = input_file.suffix.lower()
    if suf in (".tif", ".tiff"):
        kind, out_suf = "tiff_to_flac", ".flac"
    elif suf == ".flac":
        kind, out_suf = "flac_to_tiff", ".tif"
    else:
        typer.echo(f"Error: Unsupported file format: {suf}", err=True)
        raise typer.Exit(1)
    output_file = output_file or input_file.with_suffix(out_suf)
    if output_file.exists() and not force:
        typer.echo(f"Error: Output file already exists: {output_file}", err=True)
        raise typer.Exit(1)
    differs = False
    try:
        conv = RasterFLACConverter()
        if kind == "tiff_to_flac":
            res = conv.tiff_to_flac(input_file, output_file, compression_level, spatial_tiling, tile_size)
            if spatial_tiling and res:
                typer.echo(f"Spatial index created with {len(res.frames)} tiles")
        else:
            conv.flac_to_tiff(input_file, output_file)
        typer.echo(f"SUCCESS: {output_file}")
        if verify:
            from . import geotiff
            from .compare import compare_arrays
            back, _ = conv.decode_bytes(output_file.read_bytes())
            ex = compare_arrays(geotiff.read(input_file).data, back, ctx=conv.ctx, show_bands=False)["exact"]
            differs = ex["n_different"] != 0
            if differs:
                typer.echo(f"VERIFY: differs (n_different={ex['n_different']}, "
                           f"max_difference={ex['max_difference']})")
            else:
                typer.echo("VERIFY: lossless")
    except Exception as e:  # reference: any error -> exit 1 (cli.py:90-93)
        log.exception("Conversion failed")
        typer.echo(f"Error during conversion: {e}", err=True)
        raise typer.Exit(1)
    if differs:
        raise typer.Exit(3)


@app.command("create-streaming")
def create_streaming(
    input_file: Path = typer.Argument(..., help="Input TIFF file to convert"),
    output_file: Optional[Path] = typer.Option(None, "--output", "-o", help="Output streaming FLAC file"),
    tile_size: int = typer.Option(1024, "--tile-size", help="Size of streaming tiles (default: 1024x1024)"),
    force: bool = typer.Option(False, "--force", "-f", help="Overwrite existing output file"),
    gpus: int = typer.Option(1, "--gpus", help="Extension: shard the tiles over N local GPUs (one process each)"),
    distributed: bool = typer.Option(False, "--distributed",
                                     help="Extension: run as one rank of a launcher (RANK/WORLD_SIZE/LOCAL_RANK/"
                                          "MASTER_ADDR/MASTER_PORT in the environment)"),
    verify: bool = typer.Option(False, "--verify", help="Extension: read the written file back, decode it into one "
                                                        "raster on the GPU and compare it with band 1 of the source "
                                                        "there, or every stored band with --bands (single GPU only); "
                                                        "exit status 3 when it differs"),
    overviews: bool = typer.Option(False, "--overviews", help="Extension: append reduced-resolution levels (each a 2x "
                                                              "reduction of the one before, made on the GPU) until "
                                                              "one fits in a single tile (single GPU only)"),
    resampling: str = typer.Option("average", "--resampling", help="Overview resampling: average or nearest"),
    overview_levels: Optional[int] = typer.Option(None, "--overview-levels", min=0,
                                                  help="Write at most N overview levels"),
    nodata: Optional[str] = typer.Option(None, "--nodata", help="Extension: the value of pixels without data, a number "
                                                                "or 'source' (the GeoTIFF's own nodata tag): written "
                                                                "to the index and the tiles, and kept out of the "
                                                                "overview averages (single GPU only)"),
    stats: bool = typer.Option(False, "--stats", help="Extension: compute the band's statistics and a histogram of at "
                                                      "most 256 bins on the GPU and store them in the index (single "
                                                      "GPU only)"),
    bands: Optional[str] = typer.Option(None, "--bands", help="Extension: store these bands, 'all' or 1-based numbers "
                                                              "such as 1,2,3 (band 1 must be among them), each as "
                                                              "mono tiles after the band before it (single GPU "
                                                              "only; default: band 1 alone)"),
):
    """Create Netflix-style streaming FLAC with self-contained tiles"""
    from . import streaming
    sel = None
    if bands is not None:
        if gpus > 1 or distributed:
            typer.echo("Error: --bands runs on one GPU: it cannot be combined with --gpus > 1 or --distributed",
                       err=True)
            raise typer.Exit(1)
        try:
            sel = streaming.parse_bands(bands)
            if sel != "all" and 1 not in sel:
                raise ValueError(f"--bands must name band 1 (the index's top-level keys are band 1's), got {bands!r}")
        except ValueError as e:
            typer.echo(f"Error: {e}", err=True)
            raise typer.Exit(1)
    if stats and (gpus > 1 or distributed):
        typer.echo("Error: --stats runs on one GPU: it cannot be combined with --gpus > 1 or --distributed", err=True)
        raise typer.Exit(1)
    nd = None
    if nodata is not None:
        if gpus > 1 or distributed:
            typer.echo("Error: --nodata runs on one GPU: it cannot be combined with --gpus > 1 or --distributed",
                       err=True)
            raise typer.Exit(1)
        nd = _nodata_option(nodata, "source")
    # --verify and --overviews are checked before anything else is looked at or done
    if verify and (gpus > 1 or distributed):
        typer.echo("Error: --verify runs on one GPU: it cannot be combined with --gpus > 1 or --distributed", err=True)
        raise typer.Exit(1)
    if overviews and (gpus > 1 or distributed):
        typer.echo("Error: --overviews runs on one GPU: it cannot be combined with --gpus > 1 or --distributed",
                   err=True)
        raise typer.Exit(1)
    if resampling not in streaming.RESAMPLING:
        typer.echo(f"Error: --resampling must be one of {', '.join(streaming.RESAMPLING)}, got: {resampling}", err=True)
        raise typer.Exit(1)
    if not overviews and (resampling != "average" or overview_levels is not None):
        typer.echo("Error: --resampling and --overview-levels need --overviews", err=True)
        raise typer.Exit(1)
    if not input_file.exists():
        typer.echo(f"Error: Input file does not exist: {input_file}", err=True)
        raise typer.Exit(1)
    if input_file.suffix.lower() not in (".tif", ".tiff"):
        typer.echo(f"Error: Input must be a TIFF file, got: {input_file.suffix}", err=True)
        raise typer.Exit(1)
    if output_file is None:
        output_file = input_file.with_suffix(".flac").with_name(input_file.stem + "_streaming.flac")
    if output_file.exists() and not force and not distributed:
        typer.echo(f"Error: Output file already exists: {output_file}", err=True)
        raise typer.Exit(1)
    if sel is not None:  # the one rule that needs the source: checked before anything is written
        from . import geotiff
        try:
            with geotiff.TiffFile(input_file) as tf:
                sel = streaming.select_bands(sel, tf.count)
        except ValueError as e:
            typer.echo(f"Error: --bands: {e}", err=True)
            raise typer.Exit(1)
    if gpus > 1 and not distributed:
        from .launch import run_ranks
        argv = ["create-streaming", str(input_file), "--output", str(output_file), "--tile-size", str(tile_size),
                "--force", "--distributed"]
        rc = run_ranks(gpus, argv)
        if rc:
            typer.echo(f"Error creating streaming FLAC: a rank exited with {rc}", err=True)
            raise typer.Exit(1)
        typer.echo(f"SUCCESS: {output_file} ({gpus} GPUs)")
        return
    differs = False
    try:
        if distributed:
            from .distributed import create_streaming_distributed
            index = create_streaming_distributed(input_file, output_file, tile_size)
        else:
            index = streaming.create_streaming(input_file, output_file, tile_size, overviews=overviews,
                                               resampling=resampling, max_levels=overview_levels, nodata=nd,
                                               stats=stats, bands=sel)
        top = max(streaming.overview_levels(index))
        if sel is not None:
            typer.echo(f"BANDS: {','.join(str(b) for b in streaming.bands_of(index))} of "
                       f"{index['bands']['count']}")
        if overviews:
            typer.echo(f"SUCCESS: {output_file} ({len(index['frames'])} tiles, {top} overview levels)")
        else:
            typer.echo(f"SUCCESS: {output_file} ({len(index['frames'])} tiles)")
        if "nodata" in index:
            typer.echo(f"NODATA: {index['nodata']}")
        if "statistics" in index:
            st = index["statistics"]
            typer.echo(f"STATS: valid={st['valid']} nodata={st['nodata_count']} nan={st['nan']} min={st['min']} "
                       f"max={st['max']} mean={st['mean']} std={st['std']}")
        if verify and sel is not None:
            from . import geotiff
            stored = streaming.bands_of(index)
            with geotiff.TiffFile(input_file) as tf:
                for b in stored:  # every stored band, and every level of it, against the source's band
                    ex = streaming.verify_streaming(output_file, tf.read_rows(bands=[b - 1])[0], band_number=b)
                    if ex["n_different"] != 0:
                        differs = True
                        typer.echo(f"VERIFY: differs (band {b}, n_different={ex['n_different']}, "
                                   f"max_difference={ex['max_difference']})")
                        break
            if not differs:
                lv = f", levels 0..{ex['levels_checked'] - 1}" if overviews else ""
                typer.echo(f"VERIFY: lossless (bands {','.join(str(b) for b in stored)}{lv})")
        elif verify:
            from . import geotiff
            ex = streaming.verify_streaming(output_file, geotiff.read(input_file).data[0])
            differs = ex["n_different"] != 0
            if differs:
                typer.echo(f"VERIFY: differs (n_different={ex['n_different']}, "
                           f"max_difference={ex['max_difference']})")
            elif overviews:
                typer.echo(f"VERIFY: lossless (levels 0..{ex['levels_checked'] - 1})")
            else:
                typer.echo("VERIFY: lossless")
    except Exception as e:
        log.exception("Streaming FLAC creation failed")
        typer.echo(f"Error creating streaming FLAC: {e}", err=True)
        raise typer.Exit(1)
    if differs:
        raise typer.Exit(3)


@app.command("extract-streaming")
def extract_streaming(
    flac_url: str = typer.Argument(..., help="Streaming FLAC file (local path or HTTP URL)"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="Bounding box as 'xmin,ymin,xmax,ymax'"),
    tile_id: Optional[int] = typer.Option(None, "--tile-id", help="Extract specific tile by ID"),
    output: Path = typer.Option(..., "--output", "-o", help="Output TIFF file path"),
    center: bool = typer.Option(False, "--center", help="Extract center tile"),
    last: bool = typer.Option(False, "--last", help="Extract last tile"),
    mosaic: bool = typer.Option(False, "--mosaic", help="Extension: mosaic every tile intersecting --bbox"),
    all_tiles: bool = typer.Option(False, "--all", help="Extension: decode every tile and write the whole raster"),
    level: Optional[int] = typer.Option(None, "--level", min=0, help="Extension: read overview level K (0: full "
                                                                     "resolution) of a file written with --overviews"),
    max_size: Optional[int] = typer.Option(None, "--max-size", min=1,
                                           help="Extension: with --all or --bbox --mosaic, read the finest level at "
                                                "which the result is at most N pixels on its longer side"),
    out_size: Optional[str] = typer.Option(None, "--out-size",
                                           help="Extension: with --bbox, return the box as exactly WxH pixels, "
                                                "resampled on the GPU from the overview level that fits"),
    resampling: Optional[str] = typer.Option(None, "--resampling",
                                             help="With --out-size: nearest, bilinear or average (default)"),
    fill: Optional[float] = typer.Option(None, "--fill", help="With --out-size: value of pixels outside the raster "
                                                              "(default: the nodata value in force, else 0)"),
    nodata: Optional[str] = typer.Option(None, "--nodata", help="Extension: override the file's nodata value with a "
                                                                "number, or 'none' to read without one (default: the "
                                                                "value in the file's index)"),
    bands: Optional[str] = typer.Option(None, "--bands", help="Extension: the stored bands to read, 'all' or numbers "
                                                              "such as 3,1: a multi-band GeoTIFF with --all, --bbox "
                                                              "--mosaic or --out-size; exactly one band with "
                                                              "--tile-id, --center, --last or a plain --bbox "
                                                              "(default: band 1)"),
):
    """Extract tiles from Netflix-style streaming FLAC files"""
    from . import streaming
    nd = "index" if nodata is None else _nodata_option(nodata, "none")
    # --bands: every rule is checked before anything is read
    sel = None
    if bands is not None:
        try:
            sel = streaming.parse_bands(bands)
        except ValueError as e:
            typer.echo(f"Error: {e}", err=True)
            raise typer.Exit(1)
        many = all_tiles or (mosaic and bbox is not None) or out_size is not None
        if not many and (sel == "all" or len(sel) != 1):
            typer.echo("Error: --tile-id, --center, --last and a plain --bbox read one tile: --bands must name exactly "
                       "one band there", err=True)
            raise typer.Exit(1)
    # --out-size: every rule is checked before anything is read
    size = None
    if out_size is None and (resampling is not None or fill is not None):
        typer.echo("Error: --resampling and --fill work with --out-size only", err=True)
        raise typer.Exit(1)
    if out_size is not None:
        if bbox is None:
            typer.echo("Error: --out-size needs --bbox", err=True)
            raise typer.Exit(1)
        if mosaic or all_tiles or tile_id is not None or center or last or max_size is not None:
            typer.echo("Error: --out-size cannot be combined with --mosaic, --all, --tile-id, --center, --last or "
                       "--max-size", err=True)
            raise typer.Exit(1)
        parts = out_size.lower().split("x")
        if len(parts) != 2 or not all(p.isascii() and p.isdigit() for p in parts) or min(int(p) for p in parts) < 1:
            typer.echo(f"Error: --out-size must be WxH with W and H >= 1, got {out_size!r}", err=True)
            raise typer.Exit(1)
        size = (int(parts[0]), int(parts[1]))
        resampling = "average" if resampling is None else resampling
        if resampling not in streaming.RESAMPLING_READ:
            typer.echo(f"Error: --resampling must be one of {', '.join(streaming.RESAMPLING_READ)}", err=True)
            raise typer.Exit(1)
    # --all takes no tile selection: checked before anything is read
    if all_tiles and (bbox is not None or tile_id is not None or center or last):
        typer.echo("Error: --all cannot be combined with --bbox, --tile-id, --center or --last", err=True)
        raise typer.Exit(1)
    if level is not None and max_size is not None:
        typer.echo("Error: --level and --max-size exclude each other", err=True)
        raise typer.Exit(1)
    if max_size is not None and not (all_tiles or (mosaic and bbox is not None)):
        typer.echo("Error: --max-size works with --all or --bbox --mosaic only", err=True)
        raise typer.Exit(1)
    coords = None
    if bbox:
        try:
            coords = [float(x.strip()) for x in bbox.split(",")]
            if len(coords) != 4:
                raise ValueError("Bbox must have exactly 4 coordinates")
        except (ValueError, IndexError) as e:
            typer.echo(f"Error: Invalid bbox format. Use 'xmin,ymin,xmax,ymax': {e}", err=True)
            raise typer.Exit(1)
    try:
        lvl = level or 0
        if max_size is not None:
            _, index = streaming.read_index(flac_url)
            wpx, hpx = int(index["width"]), int(index["height"])
            if not all_tiles:
                from . import geotiff
                t = geotiff.Affine(*index["transform"][:6])
                if t.b == 0 and t.d == 0:
                    win = streaming.bbox_pixel_window(t, coords, wpx, hpx)
                    wpx, hpx = max(win["width"], 1), max(win["height"], 1)
            lvl = streaming.pick_level(index, wpx, hpx, max_size)
        at = f" (level {lvl})" if level is not None or max_size is not None else ""
        if size is not None:
            from . import geotiff
            _, index = streaming.read_index(flac_url)
            req = streaming.window_request(index, coords, size[0], size[1], level)
            arr, tr = streaming.read_window(flac_url, coords, size[0], size[1], resampling=resampling, level=level,
                                            fill=fill, nodata=nd, bands=sel)
            crs = index.get("crs")
            epsg = int(crs.split(":")[1]) if crs and crs.upper().startswith("EPSG:") else None
            geotiff.write(output, arr, transform=geotiff.Affine(*tr[:6]), epsg=epsg,
                          nodata=streaming.nodata_in_force(index, nd))
            typer.echo(f"SUCCESS: window {size[0]}x{size[1]} (level {req['level']}, {resampling}) -> {output}")
        elif all_tiles:
            index = streaming.extract_all(flac_url, output, level=lvl, nodata=nd, bands=sel)
            typer.echo(f"SUCCESS: Extracted all {len(index['frames'])} tiles to {output}{at}")
        elif mosaic and coords is not None:
            from . import geotiff
            arr, win, tr = streaming.extract_bbox_mosaic(flac_url, coords, level=lvl, bands=sel)
            n, index = streaming.read_index(flac_url)
            crs = index.get("crs")
            epsg = int(crs.split(":")[1]) if crs and crs.upper().startswith("EPSG:") else None
            geotiff.write(output, arr, transform=geotiff.Affine(*tr[:6]), epsg=epsg,
                          nodata=streaming.nodata_in_force(index, nd))
            typer.echo(f"SUCCESS: mosaic {win} -> {output}{at}")
        else:
            f = streaming.extract_streaming(flac_url, output, bbox=coords, tile_id=tile_id, center=center, last=last,
                                            level=lvl, nodata=nd, band=1 if sel is None else sel[0])
            typer.echo(f"SUCCESS: Extracted tile {f['frame_id']} to {output}{at}")
    except (KeyError, LookupError, ValueError) as e:
        typer.echo(f"Error: {e}", err=True)
        raise typer.Exit(1)
    except Exception as e:
        log.exception("Streaming extraction failed")
        typer.echo(f"Error during streaming extraction: {e}", err=True)
        raise typer.Exit(1)


def _nodata_option(text: str, word: str):
    """--nodata: a number, or the one word the command allows"""
    if text.strip().lower() == word:
        return word
    try:
        return float(text)
    except ValueError:
        typer.echo(f"Error: --nodata must be a number or '{word}', got {text!r}", err=True)
        raise typer.Exit(1)


def _bbox(text: str):
    coords = [float(x.strip()) for x in text.split(",")]
    if len(coords) != 4:
        raise ValueError("Bbox must have 4 coordinates")
    return coords


@app.command()
def info(file_path: str = typer.Argument(..., help="FLAC or TIFF file to inspect (local path or HTTP URL)")):
    """Display information about a FLAC or TIFF file"""  # reference cli.py:96-244
    from rich.console import Console
    con = Console()
    is_url = file_path.startswith(("http://", "https://"))
    if not is_url:
        p = Path(file_path)
        if not p.exists():
            con.print(f"[red]Error: File does not exist: {file_path}[/red]")
            raise typer.Exit(1)
        suffix = p.suffix.lower()
    else:
        from urllib.parse import urlparse
        suffix = Path(urlparse(file_path).path).suffix.lower()
    if suffix in (".tif", ".tiff"):
        from . import geotiff
        if is_url:
            con.print("[red]Error: URL-based TIFF inspection not supported yet[/red]")
            raise typer.Exit(1)
        r = geotiff.read(file_path)
        con.print("[cyan]TIFF Information:[/cyan]")
        con.print(f"  Dimensions: {r.width} x {r.height}")
        con.print(f"  Bands: {r.count}")
        con.print(f"  Data type: {r.dtype}")
        con.print(f"  CRS: {r.crs_string}")
        con.print(f"  Bounds: {r.bounds}")
        con.print(f"  File size: {Path(file_path).stat().st_size / 1024 / 1024:.2f} MB")
    elif suffix == ".flac":
        con.print("[cyan]FLAC Information:[/cyan]")
        if is_url:
            try:
                import requests
                from .spatial_encoder import SpatialFLACStreamer
                size = int(requests.head(file_path).headers.get("content-length", 0))
                con.print(f"  Remote file size: {size / 1024 / 1024:.2f} MB")
                st = SpatialFLACStreamer(file_path)
                con.print(f"  Spatial tiles: {len(st.spatial_index.frames)}")
                con.print(f"  Total indexed data: {st.spatial_index.total_bytes:,} bytes")
                con.print("\n[green]Spatial FLAC Metadata:[/green]")
                con.print("  Spatial format: Yes")
                con.print(f"  Total frames/tiles: {len(st.spatial_index.frames)}")
                con.print(f"  CRS: {st.spatial_index.crs}")
                con.print(f"  Transform: {st.spatial_index.transform}")
            except Exception as e:
                con.print(f"  [red]Error reading remote FLAC file: {e}[/red]")
            return
        from . import container
        buf = Path(file_path).read_bytes()
        if buf[:4] != b"fLaC":  # a streaming file starts with its index
            try:
                from . import streaming
                _, index = container.parse_streaming_header(buf)
                levels = streaming.overview_levels(index)
                con.print("  Streaming format: Yes")
                con.print(f"  Dimensions: {index['width']} x {index['height']}")
                con.print(f"  Tile size: {index['tile_size']}")
                con.print(f"  Tiles (level 0): {len(index['frames'])}")
                con.print(f"  Overview levels: {len(levels) - 1}")
                stored = streaming.bands_of(index)
                of = f" of {index['bands']['count']}" if "bands" in index else ""
                con.print(f"  Bands stored: {','.join(str(b) for b in stored)}{of}")
                con.print(f"  CRS: {index.get('crs')}")
                con.print(f"  Nodata: {index['nodata'] if 'nodata' in index else 'None'}")
                if "statistics" in index:
                    from .stats import format_band
                    con.print("  Statistics (level 0):")
                    for b in stored:
                        st = streaming.index_statistics(streaming.band_index(index, b))
                        for line in format_band(b, st)[0 if len(stored) > 1 else 1:]:
                            con.print("  " + line, highlight=False)
                con.print(f"  File size: {len(buf) / 1024 / 1024:.2f} MB")
                return
            except Exception:
                pass  # not a streaming file either: the messages below
        meta = None
        try:
            import numpy as np
            from ._native import default_context
            meta = container.parse_metadata(buf)
            frames = np.frombuffer(buf, dtype=np.uint8)[meta.audio_offset:]
            md0 = container.read_raster_tags(meta)
            n = int(md0["width"]) * int(md0["height"]) if md0 else None
            if n is None:
                raise ValueError("sample count unknown without geospatial tags (STREAMINFO total is 0)")
            pcm = default_context().decode_frames_host(frames, [0, len(frames)], [n], channels=meta.channels,
                                                       bps=meta.bps, blocksize=meta.blocksize)
            con.print(f"  Sample rate: {meta.sample_rate} Hz")
            con.print(f"  Channels: {meta.channels}")
            con.print(f"  Audio shape: {pcm.shape}")
            con.print("  Data type: float64")
            con.print(f"  File size: {len(buf) / 1024 / 1024:.2f} MB")
        except Exception as e:
            con.print(f"  [red]Error reading FLAC file: {e}[/red]")
            con.print(f"  File size: {len(buf) / 1024 / 1024:.2f} MB")
        shown = False
        try:
            m = meta or container.parse_metadata(buf)
            if m.tag("GEOSPATIAL_CRS") is None:
                raise ValueError("No embedded metadata")
            con.print("\n[green]Embedded Geospatial Metadata:[/green]")
            g = lambda k: m.tag(k) if m.tag(k) is not None else "N/A"  # noqa: E731
            con.print(f"  Original dimensions: {g('GEOSPATIAL_WIDTH')} x {g('GEOSPATIAL_HEIGHT')}")
            con.print(f"  Original bands: {g('GEOSPATIAL_COUNT')}")
            con.print(f"  Original dtype: {g('GEOSPATIAL_DTYPE')}")
            con.print(f"  CRS: {g('GEOSPATIAL_CRS')}")
            con.print(f"  Data range: [{g('GEOSPATIAL_DATA_MIN')}, {g('GEOSPATIAL_DATA_MAX')}]")
            tiled = (m.tag("GEOSPATIAL_SPATIAL_TILING") or "false").lower() == "true"
            con.print(f"  Spatial tiling: {'Yes' if tiled else 'No'}")
            bs = m.tag("GEOSPATIAL_BOUNDS")
            if bs:
                b = json.loads(bs)
                if isinstance(b, dict):
                    b = [b["left"], b["bottom"], b["right"], b["top"]]
                con.print(f"  Bounds: ({b[0]:.6f}, {b[1]:.6f}, {b[2]:.6f}, {b[3]:.6f})")
            shown = True
        except Exception:
            side = Path(file_path).with_suffix(".json")
            if side.exists():
                mj = json.loads(side.read_text())
                con.print(f"\n[yellow]Raster Metadata (from {side.name}):[/yellow]")
                con.print(f"  Original dimensions: {mj['width']} x {mj['height']}")
                con.print(f"  Original bands: {mj['count']}")
                con.print(f"  Original dtype: {mj['dtype']}")
                con.print(f"  CRS: {mj.get('crs', 'None')}")
                if mj.get("bounds"):
                    b = mj["bounds"]
                    con.print(f"  Bounds: ({b['left']}, {b['bottom']}, {b['right']}, {b['top']})")
                shown = True
        if not shown:
            con.print("\n[yellow]No embedded or sidecar metadata found[/yellow]")
    else:
        con.print(f"[red]Error: Unsupported file format: {suffix}[/red]")
        raise typer.Exit(1)


@app.command()
def stats(
    file_path: Path = typer.Argument(..., help="TIFF or streaming FLAC file"),
    level: Optional[int] = typer.Option(None, "--level", min=0, help="Overview level K of a streaming file written "
                                                                     "with --overviews (0: full resolution)"),
    nodata: Optional[str] = typer.Option(None, "--nodata", help="Override the file's nodata value with a number, or "
                                                                "'none' to count every pixel (default: the file's "
                                                                "own value)"),
    bins: int = typer.Option(256, "--bins", help="Histogram bins at most (1..16384); an integer band whose value range "
                                                 "fits gets one bin per value"),
    percentiles: str = typer.Option("2,50,98", "--percentiles", help="Percentiles to read off the histogram"),
    as_json: bool = typer.Option(False, "--json", help="Print one JSON document"),
    band: Optional[int] = typer.Option(None, "--band", help="One band (1-based) instead of every band the file holds"),
):
    """Band statistics and histogram, computed on the GPU (extension)"""
    from .stats import MAX_BINS
    if band is not None and band < 1:
        typer.echo(f"Error: --band numbers start at 1, got {band}", err=True)
        raise typer.Exit(1)
    # every argument rule is checked before anything is read
    if not 1 <= bins <= MAX_BINS:
        typer.echo(f"Error: --bins must be 1..{MAX_BINS}, got {bins}", err=True)
        raise typer.Exit(1)
    try:
        from fractions import Fraction
        qs = [p.strip() for p in percentiles.split(",") if p.strip()]
        if not qs or not all(0 <= Fraction(q) <= 100 for q in qs):
            raise ValueError(percentiles)
    except (ValueError, ZeroDivisionError):
        typer.echo(f"Error: --percentiles must be numbers 0..100 separated by commas, got {percentiles!r}", err=True)
        raise typer.Exit(1)
    nd = "file" if nodata is None else _nodata_option(nodata, "none")
    if not file_path.exists():
        typer.echo(f"Error: Input file does not exist: {file_path}", err=True)
        raise typer.Exit(1)
    suffix = file_path.suffix.lower()
    if suffix not in (".tif", ".tiff", ".flac"):
        typer.echo(f"Error: Unsupported file format: {suffix}", err=True)
        raise typer.Exit(1)
    if level is not None and suffix != ".flac":
        typer.echo("Error: --level applies to streaming FLAC files: a TIFF has one level", err=True)
        raise typer.Exit(1)
    try:
        from .stats import format_band, raster_file_statistics, with_percentiles
        res = raster_file_statistics(file_path, level=level or 0, nodata=nd, bins=bins, band=band)
        res["bands"] = [with_percentiles(b, qs) for b in res["bands"]]
        if as_json:
            from .stats import statistics_to_index
            doc = dict(res, nodata=None if res["nodata"] is None else _nodata_word(res["nodata"]),
                       bands=[dict(statistics_to_index(b), percentiles=b["percentiles"]) for b in res["bands"]])
            typer.echo(json.dumps(doc))
        else:
            at = f", level {res['level']}" if suffix == ".flac" else ""
            typer.echo(f"{file_path}: {res['width']} x {res['height']}, {len(res['bands'])} band(s), {res['dtype']}"
                       f"{at}, nodata {res['nodata']}")
            for i, b in zip(res["band_numbers"], res["bands"]):
                for line in format_band(i, b, qs):
                    typer.echo(line)
    except (KeyError, LookupError, ValueError) as e:
        typer.echo(f"Error: {e}", err=True)
        raise typer.Exit(1)
    except Exception as e:
        log.exception("Statistics failed")
        typer.echo(f"Error during statistics: {e}", err=True)
        raise typer.Exit(1)


def _hillshade_value_follows(args, i) -> bool:
    """Is args[i + 1] the AZ,ALT of the --hillshade at args[i]?  It is when it begins like a number."""
    import re
    return i + 1 < len(args) and re.match(r"[-+]?(\d|\.\d|nan|inf)", args[i + 1], re.IGNORECASE) is not None


class _RenderCommand(typer.core.TyperCommand):
    """`--hillshade` may stand alone: the default azimuth and altitude are put behind it before the options are parsed
    (an option of the parser takes a value or none, not either)."""

    def parse_args(self, ctx, args):
        from .render import DEFAULT_HILLSHADE
        out = []
        for i, a in enumerate(args):
            out.append(a)
            if a == "--hillshade" and not _hillshade_value_follows(args, i):
                out.append("%r,%r" % DEFAULT_HILLSHADE)
        return super().parse_args(ctx, out)


@app.command(cls=_RenderCommand)
def render(
    flac_url: str = typer.Argument(..., help="Streaming FLAC file (local path or HTTP URL)"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="Bounding box as 'xmin,ymin,xmax,ymax' (default: "
                                                                   "the raster's bounds)"),
    out_size: Optional[str] = typer.Option(None, "--out-size", help="The image as exactly WxH pixels"),
    max_size: Optional[int] = typer.Option(None, "--max-size", help="The image's longer side as N pixels, the other "
                                                                    "by the box's aspect ratio"),
    output: Path = typer.Option(..., "--output", "-o", help="Output .png, or .tif (georeferenced, 8-bit)"),
    stretch: str = typer.Option("percentile:2,98", "--stretch", help="minmax, percentile:p,q, stddev:k or range:lo,hi"),
    stats_from: str = typer.Option("auto", "--stats-from", help="auto, file (the index's statistics: one stretch for "
                                                                "the whole raster) or window (the decoded window's)"),
    colormap: str = typer.Option("gray", "--colormap", help="gray, gray_r, heat, terrain, diverging, or a text file "
                                                            "of 't r g b [a]' lines"),
    gamma: float = typer.Option(1.0, "--gamma", help="Gamma of the ramp (> 0)"),
    transfer: str = typer.Option("linear", "--transfer", help="linear or log"),
    resampling: str = typer.Option("average", "--resampling", help="nearest, bilinear or average"),
    level: Optional[int] = typer.Option(None, "--level", min=0, help="Read overview level K instead of the one that "
                                                                     "fits"),
    nodata: Optional[str] = typer.Option(None, "--nodata", help="Override the file's nodata value with a number, or "
                                                                "'none' to render without one"),
    channels: int = typer.Option(4, "--channels", help="1 (grey), 2 (grey, alpha) or 4 (R, G, B, A)"),
    force: bool = typer.Option(False, "--force", help="Overwrite the output file"),
    hillshade: Optional[str] = typer.Option(None, "--hillshade", help="Shade the image by the relief: the light's "
                                            "azimuth (clockwise from north) and altitude in degrees as 'AZ,ALT', or "
                                            "alone for 315,45.  Horn's gradient on the output grid, with the output "
                                            "pixel's size in the units of the file's coordinates: a geographic CRS "
                                            "(degrees against metres) needs --z-factor, nothing is guessed"),
    z_factor: Optional[float] = typer.Option(None, "--z-factor", help="Heights are multiplied by F before the slope is "
                                                                      "taken (> 0; needs --hillshade)"),
    shade_strength: Optional[float] = typer.Option(None, "--shade-strength", help="0 (none) .. 1 (full, the default) "
                                                                                  "(needs --hillshade)"),
    shade_only: bool = typer.Option(False, "--shade-only", help="The shade alone, in grey: no stretch, colour ramp or "
                                                                "statistics (needs --hillshade)"),
    band: Optional[int] = typer.Option(None, "--band", help="Render stored band B (1-based) instead of band 1: the "
                                                            "stretch and the file statistics are that band's"),
    bands: Optional[str] = typer.Option(None, "--bands", help="A colour composite of three stored bands as 'R,G,B': "
                                                              "each stretched over its own statistics; --colormap "
                                                              "stays gray (gamma and transfer shape the curves), no "
                                                              "--hillshade, --channels 4"),
):
    """Render a window of a streaming file as a stretched 8-bit colour image on the GPU (extension)"""
    from . import render as rn
    from . import streaming
    # every argument rule is checked before anything is read
    def fail(msg: str):
        typer.echo(f"Error: {msg}", err=True)
        raise typer.Exit(1)

    if (out_size is None) == (max_size is None):
        fail("give exactly one of --out-size WxH and --max-size N")
    size = None
    if out_size is not None:
        parts = out_size.lower().split("x")
        if len(parts) != 2 or not all(p.isascii() and p.isdigit() for p in parts) or min(int(p) for p in parts) < 1:
            fail(f"--out-size must be WxH with W and H >= 1, got {out_size!r}")
        size = (int(parts[0]), int(parts[1]))
    elif max_size < 1:
        fail(f"--max-size must be >= 1, got {max_size}")
    suffix = output.suffix.lower()
    if suffix not in (".png", ".tif", ".tiff"):
        fail(f"the output must be .png or .tif, got {output.name!r}")
    if channels not in (1, 2, 4):
        fail(f"--channels must be 1, 2 or 4, got {channels}")
    if stats_from not in streaming.STATS_FROM:
        fail(f"--stats-from must be one of {', '.join(streaming.STATS_FROM)}")
    if resampling not in streaming.RESAMPLING_READ:
        fail(f"--resampling must be one of {', '.join(streaming.RESAMPLING_READ)}")
    if transfer not in rn.TRANSFERS:
        fail(f"--transfer must be one of {', '.join(rn.TRANSFERS)}")
    if not (gamma > 0 and gamma != float("inf")):
        fail(f"--gamma must be a finite number > 0, got {gamma}")
    try:
        rn.parse_stretch(stretch)
    except ValueError as e:
        fail(str(e))
    band_kw = {}
    if band is not None and bands is not None:
        fail("give --band or --bands, not both")
    if band is not None:
        if band < 1:
            fail(f"--band numbers start at 1, got {band}")
        band_kw["band"] = band
    if bands is not None:
        parts = [p.strip() for p in bands.split(",")]
        if len(parts) != 3 or not all(p.isascii() and p.isdigit() and int(p) >= 1 for p in parts):
            fail(f"--bands takes three band numbers 'R,G,B', got {bands!r}")
        if hillshade is not None:
            fail("--bands cannot be combined with --hillshade")
        if channels != 4:
            fail("--bands writes R, G, B, A: --channels must stay 4")
        if colormap != "gray":
            fail("--bands keeps --colormap gray: --gamma and --transfer shape the three curves")
        band_kw["bands"] = tuple(int(p) for p in parts)
    shade_kw = {}
    if hillshade is None:
        for name, v in (("--z-factor", z_factor), ("--shade-strength", shade_strength),
                        ("--shade-only", shade_only or None)):
            if v is not None:
                fail(f"{name} needs --hillshade")
    else:
        import math
        try:
            shade_kw["hillshade"] = rn.parse_hillshade(hillshade)
        except ValueError as e:
            fail(str(e))
        if z_factor is not None:
            if not (math.isfinite(z_factor) and z_factor > 0):
                fail(f"--z-factor must be a finite number > 0, got {z_factor}")
            shade_kw["z_factor"] = z_factor
        if shade_strength is not None:
            if not 0 <= shade_strength <= 1:
                fail(f"--shade-strength must lie in [0, 1], got {shade_strength}")
            shade_kw["shade_strength"] = shade_strength
        if shade_only:
            if colormap != "gray" or stretch != rn.DEFAULT_STRETCH or stats_from != "auto":
                fail("--shade-only renders the shade alone: it excludes --colormap, --stretch and --stats-from")
            shade_kw["shade_only"] = True
    nd = "index" if nodata is None else _nodata_option(nodata, "none")
    coords = None
    if bbox is not None:
        try:
            coords = _bbox(bbox)
            if not (coords[2] > coords[0] and coords[3] > coords[1]):
                raise ValueError("xmax > xmin and ymax > ymin are needed")
        except (ValueError, IndexError) as e:
            fail(f"Invalid bbox format. Use 'xmin,ymin,xmax,ymax': {e}")
    ramp = colormap
    if colormap not in rn.COLORMAPS:  # a file: the one thing read before the raster, and an argument like the others
        if not Path(colormap).is_file():
            fail(f"--colormap must be one of {', '.join(rn.COLORMAPS)} or a file; got {colormap!r}")
        try:
            ramp = rn.load_colormap(colormap)
        except ValueError as e:
            fail(f"--colormap {colormap}: {e}")
    if output.exists() and not force:
        fail(f"{output} exists; use --force to overwrite it")
    try:
        from . import geotiff
        _, index = streaming.read_index(flac_url)
        if coords is None:
            coords = list(geotiff.bounds_of(geotiff.Affine(*index["transform"][:6]), int(index["width"]),
                                            int(index["height"])))
        if size is None:
            size = rn.max_size_shape(coords[2] - coords[0], coords[3] - coords[1], max_size)
        img, tr = streaming.render_window(flac_url, coords, size[0], size[1], stretch=stretch, stats_from=stats_from,
                                          colormap=ramp, gamma=gamma, transfer=transfer, resampling=resampling,
                                          level=level, nodata=nd, channels=channels, **shade_kw, **band_kw)
        if suffix == ".png":
            from .png import write_png
            write_png(output, img)
        else:
            crs = index.get("crs")
            epsg = int(crs.split(":")[1]) if crs and crs.upper().startswith("EPSG:") else None
            geotiff.write(output, img.transpose(2, 0, 1), transform=geotiff.Affine(*tr[:6]), epsg=epsg,
                          alpha=channels > 1)
        what = f"{stretch}, {resampling}"
        if shade_kw:
            az, alt = shade_kw["hillshade"]
            what = (f"shade only, {resampling}" if shade_only else what) + f", hillshade {az:g},{alt:g}"
            what += f" z-factor {shade_kw.get('z_factor', 1.0):g} strength {shade_kw.get('shade_strength', 1.0):g}"
        if bands is not None:
            what += f", bands {bands}"
        elif band is not None:
            what += f", band {band}"
        typer.echo(f"SUCCESS: rendered {size[0]}x{size[1]}x{channels} ({what}) -> {output}")
    except (KeyError, LookupError, ValueError) as e:
        typer.echo(f"Error: {e}", err=True)
        raise typer.Exit(1)
    except Exception as e:
        log.exception("Render failed")
        typer.echo(f"Error during render: {e}", err=True)
        raise typer.Exit(1)


def _nodata_word(v):
    """A nodata value as JSON holds it (streaming._nodata_to_index)"""
    from .streaming import _nodata_to_index
    return _nodata_to_index(v)


@app.command()
def compare(
    file1: Path = typer.Argument(..., help="First TIFF file"),
    file2: Path = typer.Argument(..., help="Second TIFF file"),
    show_bands: bool = typer.Option(True, "--show-bands/--no-bands", help="Show per-band statistics"),
    export_json: Optional[Path] = typer.Option(None, "--export", "-e", help="Export comparison results to JSON"),
):
    """Compare two TIFF files and display statistics"""  # reference cli.py:247-290
    from rich.console import Console
    con = Console()
    for f in (file1, file2):
        if not f.exists():
            con.print(f"[red]Error: File does not exist: {f}[/red]")
            raise typer.Exit(1)
    for f in (file1, file2):
        if f.suffix.lower() not in (".tif", ".tiff"):
            con.print(f"[red]Error: {f} is not a TIFF file[/red]")
            raise typer.Exit(1)
    try:
        from .compare import compare_tiffs, display_comparison_table
        results = compare_tiffs(file1, file2, show_bands)
        display_comparison_table(results, con)
        if export_json:
            with open(export_json, "w") as fh:
                json.dump(results, fh, indent=2)
            con.print(f"\n[green]SUCCESS: Comparison results exported to: {export_json}[/green]")
    except Exception as e:
        log.exception("Comparison failed")
        con.print(f"[red]Error during comparison: {e}[/red]")
        raise typer.Exit(1)


@app.command()
def query(
    flac_file: str = typer.Argument(..., help="Spatial FLAC file to query (local path or HTTP URL)"),
    bbox: str = typer.Option(..., "--bbox", "-b", help="Bounding box as 'xmin,ymin,xmax,ymax'"),
    output: Optional[Path] = typer.Option(None, "--output", "-o", help="Output file for extracted data"),
    format: str = typer.Option("ranges", "--format", "-f", help="Output format: 'ranges' or 'data'"),
):
    """Query spatial FLAC file by bounding box for HTTP range streaming"""  # reference cli.py:293-406
    from rich.console import Console
    from rich.table import Table
    con = Console()
    is_url = flac_file.startswith(("http://", "https://"))
    if not is_url and not Path(flac_file).exists():
        con.print(f"[red]Error: FLAC file does not exist: {flac_file}[/red]")
        raise typer.Exit(1)
    try:
        coords = _bbox(bbox)
    except (ValueError, IndexError) as e:
        con.print(f"[red]Error: Invalid bbox format. Use 'xmin,ymin,xmax,ymax': {e}[/red]")
        raise typer.Exit(1)
    try:
        from .spatial_encoder import SpatialFLACStreamer
        st = SpatialFLACStreamer(flac_file)
        if format == "ranges":
            ranges = st.get_byte_ranges_for_bbox(tuple(coords))
            con.print(f"[green]Found {len(ranges)} byte ranges for bbox {bbox}[/green]")
            table = Table(title=f"HTTP Byte Ranges for {flac_file.split('/')[-1] if is_url else Path(flac_file).name}")
            for c in ("Range #", "Start Byte", "End Byte", "Size (bytes)", "HTTP Range Header"):
                table.add_column(c)
            total = 0
            for i, (a, b) in enumerate(ranges, 1):
                total += b - a + 1
                table.add_row(str(i), f"{a:,}", f"{b:,}", f"{b - a + 1:,}", f"bytes={a}-{b}")
            con.print(table)
            con.print(f"[bold]Total data to fetch: {total:,} bytes[/bold]")
            if output:
                data = {"bbox": coords, "total_ranges": len(ranges), "total_bytes": total,
                        "ranges": [{"start": a, "end": b, "size": b - a + 1} for a, b in ranges],
                        "http_headers": [f"bytes={a}-{b}" for a, b in ranges]}
                with open(output, "w") as fh:
                    json.dump(data, fh, indent=2)
                con.print(f"[green]Ranges saved to: {output}[/green]")
        elif format == "data":
            con.print(f"[cyan]Streaming data for bbox {bbox}...[/cyan]")
            data = st.stream_bbox_data(tuple(coords))
            con.print(f"[green]Extracted {len(data):,} bytes of FLAC data[/green]")
            if output:
                Path(output).write_bytes(data)
                con.print(f"[green]Data saved to: {output}[/green]")
            else:
                con.print("[yellow]Use --output to save extracted data to file[/yellow]")
        else:
            con.print(f"[red]Error: Unknown format '{format}'. Use 'ranges' or 'data'[/red]")
            raise typer.Exit(1)
    except typer.Exit:
        raise
    except FileNotFoundError as e:
        con.print(f"[red]Error: Spatial index not found. File may not have spatial tiling enabled: {e}[/red]")
        raise typer.Exit(1)
    except Exception as e:
        log.exception("Query failed")
        con.print(f"[red]Error during query: {e}[/red]")
        raise typer.Exit(1)


@app.command("spatial-info")
def spatial_info(flac_file: str = typer.Argument(..., help="Spatial FLAC file to analyze (local path or HTTP URL)")):
    """Show spatial index information for FLAC file"""  # reference cli.py:807-872
    from rich.console import Console
    from rich.table import Table
    con = Console()
    is_url = flac_file.startswith(("http://", "https://"))
    if not is_url and not Path(flac_file).exists():
        con.print(f"[red]Error: FLAC file does not exist: {flac_file}[/red]")
        raise typer.Exit(1)
    try:
        from .spatial_encoder import SpatialFLACStreamer
        idx = SpatialFLACStreamer(flac_file).spatial_index
        con.print(f"[green]Spatial FLAC File: {Path(flac_file).name if not is_url else flac_file}[/green]")
        con.print(f"CRS: {idx.crs}")
        con.print(f"Transform: {idx.transform}")
        con.print(f"Total frames/tiles: {len(idx.frames)}")
        table = Table(title="Spatial Frames")
        for c in ("Frame ID", "Bbox (xmin, ymin, xmax, ymax)", "Window (col, row, width, height)", "Byte Range",
                  "Size"):
            table.add_column(c)
        total = 0
        for f in idx.frames[:10]:
            table.add_row(str(f.frame_id), f"({f.bbox[0]:.6f}, {f.bbox[1]:.6f}, {f.bbox[2]:.6f}, {f.bbox[3]:.6f})",
                          f"({f.window.col_off}, {f.window.row_off}, {f.window.width}, {f.window.height})",
                          f"{f.byte_offset}-{f.byte_offset + f.byte_size - 1}", f"{f.byte_size:,} bytes")
            total += f.byte_size
        con.print(table)
        if len(idx.frames) > 10:
            con.print(f"[yellow]... and {len(idx.frames) - 10} more frames[/yellow]")
        con.print(f"[bold]Total indexed data: {total:,} bytes[/bold]")
    except FileNotFoundError as e:
        con.print(f"[red]Error: Spatial index not found. File may not have spatial tiling enabled: {e}[/red]")
        raise typer.Exit(1)
    except Exception as e:
        log.exception("Spatial info failed")
        con.print(f"[red]Error reading spatial info: {e}[/red]")
        raise typer.Exit(1)


def main():
    app()


if __name__ == "__main__":
    main()
