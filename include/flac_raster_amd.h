/*
 * flac_raster_amd.h -- C-ABI of the MI355X (gfx950) spatial-FLAC codec library
 *                      (libflac_raster_amd.so, built from the HIP sources in flac_raster_amd/csrc).
 *
 * This is the drop-in boundary for the reference's hot path.  In the reference
 * (Youssef-Harby/flac-raster @ 2025-07-25) that seam is Python -> pyFLAC 3.0.0 (cffi) -> libFLAC 1.4.3:
 *
 *   reference call site                                     replaced by
 *   ------------------------------------------------------  ------------------------------------------
 *   converter.py:56-86   _normalize_to_audio (numpy)        frs_encode_tiles*   (fused, on device)
 *   converter.py:185-194 band interleave/reshape            frs_encode_tiles*   (desc.nbands channels)
 *   converter.py:201-216 pyflac.StreamEncoder(...).process   frs_encode_tiles*   (whole tiles, no per-frame
 *                        + finish()  (sonos-pyflac.txt:        write callback; frames land in one arena)
 *                        1968-2014, 2175-2212; libFLAC
 *                        FLAC__stream_encoder_process_interleaved)
 *   cli.py:690-763       create_streaming per-tile loop     frs_encode_tiles*   (all tiles in one call)
 *   converter.py:241-242 pyflac.FileDecoder(path).process()  frs_decode_frames*  (batched frames -> int32)
 *                        (sonos-pyflac.txt:1584-1640, 1809-1854; libFLAC
 *                        FLAC__stream_decoder_process_until_end_of_stream)
 *   converter.py:88-110  _denormalize_from_audio (numpy)    frs_denormalize*
 *
 * Container bytes (STREAMINFO, VORBIS_COMMENT tags, PADDING, streaming index JSON) are built by the
 * Python host (flac_raster_amd/container.py): they are text/metadata, not data-parallel work.
 *
 * Conventions: plain C types only; every buffer is caller-allocated.  Functions ending in _device take
 * device pointers (hipMalloc memory of the context's device) and run on the context's HIP
 * stream; the others take host pointers and copy through the context's staging buffers.  All functions
 * return FRS_OK (0) or a negative frs_status; frs_last_error() gives the message.  A context is bound to
 * one device and must not be used from two host threads at once (one context per GPU / rank).
 */
#ifndef FLAC_RASTER_AMD_H
#define FLAC_RASTER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRS_ABI_VERSION 1

typedef struct frs_ctx frs_ctx;

/* element types (numpy dtype of the raster) */
enum frs_dtype {
    FRS_DT_U8 = 1,
    FRS_DT_U16 = 2,
    FRS_DT_I16 = 3,
    FRS_DT_I32 = 4,
    FRS_DT_U32 = 5,
    FRS_DT_F32 = 6,
    FRS_DT_F64 = 7
};

enum frs_status {
    FRS_OK = 0,
    FRS_E_ARG = -1,         /* bad argument */
    FRS_E_HIP = -2,         /* HIP runtime error */
    FRS_E_NOSPACE = -3,     /* output buffer too small; required size reported where documented */
    FRS_E_CORRUPT = -4,     /* undecodable FLAC data */
    FRS_E_UNSUPPORTED = -5, /* valid but not supported by this build */
    FRS_E_NODEV = -6        /* no gfx950 device */
};

/* Geometry of one encode job.  The raster is [nbands_total][height][width] elements with the given
 * strides (elements).  Tiles are tile_h x tile_w windows in row-major tile order (cli.py:691-692),
 * edge tiles truncated.  Each tile is one FLAC stream whose channels are `nbands` bands starting at
 * band `band0` (create-streaming: nbands = 1, band0 = 0 -- cli.py:699 reads band 1 only; plain convert:
 * one tile covering the raster with nbands = count, converter.py:185-189).  Only the tiles
 * [tile_begin, tile_end) of the row-major tile grid are encoded (multi-GPU sharding).
 * The raster's origin, row_stride and band_stride need element alignment only: a wider common alignment of the band
 * bases, the row stride and the tile width (16, 8 or 4 bytes) only selects faster loads, never other output. */
typedef struct {
    int64_t height, width;      /* raster size in pixels */
    int64_t row_stride;         /* elements between rows */
    int64_t band_stride;        /* elements between bands */
    int32_t dtype;              /* enum frs_dtype */
    int32_t band0, nbands;      /* channels of each stream */
    int32_t tile_h, tile_w;     /* tile size in pixels */
    int32_t blocksize;          /* FLAC block size (4096, converter.py:205) */
    int32_t sample_rate;        /* STREAMINFO / frame header sample rate (converter.py:25-54) */
    int32_t bits_per_sample;    /* 16 or 24 from _calculate_audio_params (converter.py:29-37) */
    int32_t compression_level;  /* 0..8 (cli.py:36-37; create-streaming uses 5, cli.py:733); 6..8 with
                                   subdivide_tukey apodizations, 1 / 4 on two bands with loose mid/side */
    int32_t norm_mode;          /* FRS_NORM_CONVERTER or FRS_NORM_SPATIAL */
    int64_t tile_begin, tile_end;
} frs_encode_desc;

/* sample normalisation of an encode job */
enum frs_norm_mode {
    FRS_NORM_CONVERTER = 0, /* converter.py:56-86: min/max -> int16 (bps 16) or int32 x 8388607 (bps 24) */
    FRS_NORM_SPATIAL = 1    /* spatial_encoder.py:229-248: dtype-fixed float32 scaling, pyflac casts to int32
                               (32-bit stream, samples in {-1, 0, 1}: the lossy raw-frames format) */
};

int frs_abi_version(void);
/* number of usable gfx950 devices (0 when none) */
int frs_device_count(void);
int frs_ctx_create(int device, frs_ctx **out);
void frs_ctx_destroy(frs_ctx *ctx);
const char *frs_last_error(const frs_ctx *ctx);

/* Upper bound of the arena bytes frs_encode_tiles* can need for desc (all frames verbatim). */
int64_t frs_encode_arena_bound(const frs_encode_desc *desc);

/* Encode tiles [tile_begin, tile_end) into FLAC *frames* (no stream header), tile after tile, into
 * `arena` (device memory for _device).  On return (host arrays, one entry per encoded tile):
 *   tile_off[i]..tile_off[i+1]  arena byte range of tile i's frames   (tile_off has ntiles+1 entries)
 *   tile_min[i], tile_max[i]    float(np.min(tile)), float(np.max(tile)) over the tile's channels
 *                               (converter.py:152-153), used for the GEOSPATIAL_DATA_MIN/MAX tags
 *   *stream_bps                 bits per sample written in STREAMINFO (16 or 32, pyflac
 *                               encoder.py: itemsize*8, sonos-pyflac.txt:1986-1992)
 * Frames are bit-identical to libFLAC 1.4.3 level 5 fed through pyflac with blocksize `blocksize`.
 * FRS_E_NOSPACE: arena_cap too small; tile_off[ntiles] holds the bytes required. */
int frs_encode_tiles_device(frs_ctx *ctx, const frs_encode_desc *desc, const void *raster_dev, void *arena_dev,
                            int64_t arena_cap, int64_t *tile_off, double *tile_min, double *tile_max,
                            int32_t *stream_bps);
int frs_encode_tiles(frs_ctx *ctx, const frs_encode_desc *desc, const void *raster_host, uint8_t *arena_host,
                     int64_t arena_cap, int64_t *tile_off, double *tile_min, double *tile_max,
                     int32_t *stream_bps);

/* Decode the FLAC frames of `nstreams` streams.  Stream s occupies blob[stream_off[s], stream_off[s+1])
 * and must start at its first frame (the caller skips the metadata blocks; container.py parses them).
 * channels/bps describe every stream (STREAMINFO); samples are written interleaved as int32 at
 * pcm_out + pcm_off[s] * channels, pcm_off has nstreams+1 entries (per-stream sample counts known
 * from the tile windows).  Frames are located by sync code + CRC-8/CRC-16 and decoded in parallel: one lane per
 * frame for large calls (thousands of frames), two waves per frame (a Rice-decoding and a restoring wave) for a
 * single tile, one wave per frame for 32-bit / wide streams.  Ranges of any size are accepted (64-bit positions);
 * a stream with more sync-code
 * candidates than the capacity (2 x frames + bytes / 1024 + 4096) is rejected with FRS_E_CORRUPT before
 * anything is written past it. */
int frs_decode_frames_device(frs_ctx *ctx, const uint8_t *blob_dev, const int64_t *stream_off, int32_t nstreams,
                             int32_t channels, int32_t bps, int32_t blocksize, int32_t *pcm_dev,
                             const int64_t *pcm_off);
int frs_decode_frames(frs_ctx *ctx, const uint8_t *blob_host, const int64_t *stream_off, int32_t nstreams,
                      int32_t channels, int32_t bps, int32_t blocksize, int32_t *pcm_host, const int64_t *pcm_off);

/* Decode + de-normalise in one pass: replaces converter.py:241-282 as a whole (pyflac FileDecoder ->
 * soundfile PCM_16 WAV -> _denormalize_from_audio, sonos-pyflac.txt:1584-1640, converter.py:88-110) for
 * `nstreams` tiles at once.  Same stream layout as frs_decode_frames; stream s carries its own
 * GEOSPATIAL_DATA_MIN/MAX (data_min[s], data_max[s], converter.py:375-427) and its samples are written
 * interleaved as out_dtype at out + (pcm_off[s] + i) * channels + c -- the int32 PCM never reaches memory for
 * mono 16-bit streams (create-streaming tiles).  out_dev is device memory, or page-locked host memory from
 * frs_host_malloc: the kernels then store the result straight into host memory (no separate D2H copy; a C5 query
 * returns one tile this way).  On FRS_OK the result is complete and visible to the host: a device-memory out_dev
 * after the call has synchronised the context stream; page-locked host memory from frs_host_malloc as soon as the
 * kernels have published it (system-scope fences), possibly before the stream has retired -- a fault of those kernels
 * is then reported by the next call on the context.  Errors as frs_decode_frames. */
int frs_decode_tiles_device(frs_ctx *ctx, const uint8_t *blob_dev, const int64_t *stream_off, int32_t nstreams,
                            int32_t channels, int32_t bps, int32_t blocksize, const int64_t *pcm_off,
                            const double *data_min, const double *data_max, int32_t out_dtype, void *out_dev);
int frs_decode_tiles(frs_ctx *ctx, const uint8_t *blob_host, const int64_t *stream_off, int32_t nstreams,
                     int32_t channels, int32_t bps, int32_t blocksize, const int64_t *pcm_off, const double *data_min,
                     const double *data_max, int32_t out_dtype, void *out_host);
/* frs_decode_tiles_device for ONE tile -- the bbox query of cli.py:984-1023 (extract-streaming decodes the single
 * selected tile): its frames are blob_dev[start, end), `count` samples per channel, scalar arguments only (no
 * per-call tables for the binding to marshal on the latency path).  Errors as frs_decode_tiles_device. */
int frs_decode_tile_device(frs_ctx *ctx, const uint8_t *blob_dev, int64_t start, int64_t end, int64_t count,
                           int32_t channels, int32_t bps, int32_t blocksize, double data_min, double data_max,
                           int32_t out_dtype, void *out_dev);

/* converter.py:88-110 after pyflac+soundfile's WAV round trip (sonos-pyflac.txt:1629, 1827-1852): the
 * decoder's int32 samples go into a PCM_16 WAV (16-bit streams unchanged; 32-bit streams keep x >> 16,
 * libsndfile's int->short conversion) and are read back as float64 = pcm16/32768.  Then
 * out = round_half_even(((float32(v) + 1)/2) * float32(max-min) + float32(min)), all fp32 ops, cast to
 * out_dtype; for a float out_dtype float32(v) is written as-is.  pcm_bps = STREAMINFO bits per sample. */
int frs_denormalize_device(frs_ctx *ctx, const int32_t *pcm_dev, int64_t n, int32_t pcm_bps, double data_min,
                           double data_max, int32_t out_dtype, void *out_dev);
int frs_denormalize(frs_ctx *ctx, const int32_t *pcm_host, int64_t n, int32_t pcm_bps, double data_min,
                    double data_max, int32_t out_dtype, void *out_host);

/* Difference statistics of two rasters in one pass over both: replaces compare.py:55-78 (np.array_equal,
 * np.max(np.abs(a-b)), np.mean(np.abs(a-b)), np.sqrt(np.mean((a-b)**2)), np.min/np.max of each file, overall and
 * per band).  A and B are [nbands][height][width] elements of the same dtype, each with its own row / band stride
 * (elements), so a window of a larger raster can be compared.  out_host has nbands entries:
 *   count                    height*width
 *   n_diff, first_diff       elements with a != b (C: NaN differs from everything, -0.0 == 0.0) and the smallest
 *                            row*width+col among them, or -1
 *   a_min .. b_max           as double; NaN when the band holds a NaN (numpy's min/max propagate it)
 *   np_max_abs, np_sum_abs,  what numpy computes IN THE DTYPE, wraps included: integer a-b wraps (uint8: 5-10 = 251),
 *   np_sum_sq                abs of a signed value wraps (abs(int16(-32768)) = -32768), unsigned abs is the identity,
 *                            an integer square wraps (int16: 300*300 -> 24464); float terms are formed in the dtype
 *                            (the square is a separate rounded product).  np_max_abs is NaN when a difference is NaN.
 *                            mean = np_sum_abs/count and rmse = sqrt(np_sum_sq/count) are numpy's values.
 *   max_abs, sum_abs         the true |a-b| without wrap (int64 for integer dtypes, double for floats)
 * Integer sums are exact (64-bit partials added in 128 bits, converted to double once); float terms are accumulated
 * in double in a fixed order that depends only on shape and dtype, so results reproduce bit for bit.  Dense or
 * 16-byte-aligned-row inputs run on 16-byte loads; any other layout is read element by element (slower, same
 * result).  FRS_E_ARG: height, width or nbands < 1, nbands > 65535, a row stride < width, unknown dtype, a pointer not
 * aligned to the element size, or a shape whose 64-bit partial sums could overflow (more than 2^30 elements per
 * work-group: beyond ~2^41 elements per band).  frs_compare copies (nbands-1)*band_stride + (height-1)*row_stride +
 * width elements of each raster through the context's staging buffers.  Both are synchronous on the context stream. */
typedef struct {
    int64_t height, width;
    int32_t nbands, dtype;      /* dtype: enum frs_dtype */
    int64_t a_row_stride, a_band_stride, b_row_stride, b_band_stride;
} frs_compare_desc;
typedef struct {
    int64_t count, n_diff, first_diff;
    double a_min, a_max, b_min, b_max, np_max_abs, np_sum_abs, np_sum_sq, max_abs, sum_abs;
} frs_compare_band;
int frs_compare_device(frs_ctx *ctx, const frs_compare_desc *desc, const void *a_dev, const void *b_dev,
                       frs_compare_band *out_host);
int frs_compare(frs_ctx *ctx, const frs_compare_desc *desc, const void *a_host, const void *b_host,
                frs_compare_band *out_host);

/* Place decoded tiles at their windows of a raster in device memory: the decoder-side mirror of frs_encode_desc's
 * strided raster view.  Replaces streaming.extract_bbox_mosaic's host loop (np.zeros of the union window, one slice
 * assignment per tile, a second copy for the crop) and converter.py's `.reshape(H, W, C).transpose(2, 0, 1)` +
 * ascontiguousarray after a multi-band decode.
 *   tiles_dev   what frs_decode_tiles_device writes: tile t is width*height pixels in row-major order, each pixel
 *               nbands interleaved elements, starting at element pcm_off[t] * nbands (pcm_off: ntiles entries read)
 *   win[t]      the tile's size and its position relative to the destination's origin; col_off / row_off may be
 *               negative or reach past the destination's width / height
 *   dst         [nbands][height][width] elements of `dtype` with the given strides (elements)
 * Element (r, x) of channel c of tile t goes to
 *   dst_dev + c*band_stride + (row_off[t] + r)*row_stride + (col_off[t] + x).
 * Pixels outside the destination are dropped; a tile wholly outside writes nothing.  Destination elements that no tile
 * covers are not touched, the row padding of row_stride > width included.  The windows of one call MUST NOT overlap
 * inside the destination: this is not checked, and overlapping tiles race for the shared elements.  The kernel moves
 * bytes only (every dtype by its element size; whole 16-byte chunks of a destination row by aligned 16-byte stores).
 * FRS_E_ARG: ntiles < 0, a tile width or height < 1, a destination height or width < 1, row_stride < width, nbands
 * outside 1..8, unknown dtype, a negative pcm_off, a null pointer or one not aligned to the element size; also a
 * band_stride (nbands > 1) smaller than (height-1)*row_stride + width, an extent that overflows 63 bits, and a tile
 * offset beyond +-2^61.  ntiles == 0 is FRS_OK without a launch.  Synchronous on the context stream.
 *
 * frs_decode_tiles_window_device = frs_decode_tiles_device + the placement: stream s is tile s, decoded (channels =
 * dst->nbands, out_dtype = dst->dtype, samples win[s].width * win[s].height, pcm_off their prefix sums) into a
 * staging buffer the context owns and grows, then placed.  Errors as frs_decode_tiles_device and as above; synchronous
 * on return.  frs_decode_tiles_window takes a host blob and a host destination: the destination ((nbands-1)*band_stride
 * + (height-1)*row_stride + width elements) is uploaded first and downloaded after the placement, so elements no tile
 * covers survive the round trip. */
typedef struct {
    int64_t col_off, row_off;   /* position relative to the destination origin */
    int32_t width, height;      /* tile size in pixels */
} frs_tile_window;
typedef struct {
    int64_t height, width;      /* destination size in pixels */
    int64_t row_stride;         /* elements between rows */
    int64_t band_stride;        /* elements between bands */
    int32_t dtype;              /* enum frs_dtype */
    int32_t nbands;             /* 1..8: channels of every tile */
} frs_raster_desc;
int frs_place_tiles_device(frs_ctx *ctx, const frs_raster_desc *dst, const void *tiles_dev, const int64_t *pcm_off,
                           const frs_tile_window *win, int32_t ntiles, void *dst_dev);
int frs_decode_tiles_window_device(frs_ctx *ctx, const uint8_t *blob_dev, const int64_t *stream_off, int32_t nstreams,
                                   int32_t bps, int32_t blocksize, const frs_tile_window *win, const double *data_min,
                                   const double *data_max, const frs_raster_desc *dst, void *dst_dev);
int frs_decode_tiles_window(frs_ctx *ctx, const uint8_t *blob_host, const int64_t *stream_off, int32_t nstreams,
                            int32_t bps, int32_t blocksize, const frs_tile_window *win, const double *data_min,
                            const double *data_max, const frs_raster_desc *dst, void *dst_host);

/* One 2x reduction step of an overview pyramid: an H x W raster to ceil(H/2) x ceil(W/2).  The reference's streaming
 * files hold one resolution; create-streaming --overviews (streaming.py) builds level k from level k-1 with this call
 * and encodes every level with frs_encode_tiles_device.  Both rasters are band-planar [nbands][height][width] elements
 * of the same dtype, each with its own row / band stride (frs_raster_desc, nbands 1..8).  Output pixel (r, x) covers
 * source rows 2r .. min(2r+1, H-1) and columns 2x .. min(2x+1, W-1): n = 4, 2 or 1 source pixels; the edge blocks of odd
 * sizes are partial, never padded.
 *   FRS_RESAMPLE_NEAREST   the source pixel (2r, 2x), every dtype
 *   FRS_RESAMPLE_AVERAGE   integers: floor((2s + n) / (2n)) of the exact 64-bit block sum s, the mean rounded half
 *                          towards +infinity ((s + 2) >> 2 for n = 4: -1,-1,-1,-2 -> -1; -1,-2 -> -1; -3,-2 -> -2).
 *                          Floats: ((a + b) + (c + d)) * 0.25 with a = (2r, 2x), b = (2r, 2x+1), c = (2r+1, 2x),
 *                          d = (2r+1, 2x+1); (a + b) * 0.5 for n = 2; a for n = 1; every operation rounded in the dtype,
 *                          NaN and +-inf as the expression gives them.  The definition is this library's own.
 * Destination elements outside [height][width] are never written, the row padding of row_stride > width included (whole
 * 16-byte chunks of a destination row by aligned 16-byte stores, the rest element by element; nothing is read past a
 * source row's width or the last source row).  FRS_E_ARG: dst height or width not ceil(src / 2), a size < 1,
 * row_stride < width, nbands outside 1..8 or unequal, dtypes unequal or unknown, a band_stride (nbands > 1) smaller than
 * (height-1)*row_stride + width, an extent that overflows 63 bits, an unknown mode, a null pointer or one not aligned
 * to the element size, and source and destination byte ranges (origin to the end of the last row) that overlap.
 * Synchronous on the context stream; profile entry "pyramid".  frs_downsample2 takes host rasters: both are copied
 * through the context's staging buffers (the destination goes up first and comes back whole, so its padding survives). */
/* FRS_RESAMPLE_BILINEAR is frs_resample_window*'s alone: frs_downsample2* reject every mode but 0 and 1 */
enum frs_resample { FRS_RESAMPLE_NEAREST = 0, FRS_RESAMPLE_AVERAGE = 1, FRS_RESAMPLE_BILINEAR = 2 };
int frs_downsample2_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev, const frs_raster_desc *dst,
                           void *dst_dev, int32_t mode);
int frs_downsample2(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host, const frs_raster_desc *dst,
                    void *dst_host, int32_t mode);

/* Resample a rectangle of a raster onto a destination grid of any size: the last stage of a windowed read
 * (streaming.read_window: "this bounding box as exactly w x h pixels"), so that only the w x h result crosses to the
 * host.  The reference has no such read.  Both rasters are band-planar [nbands][height][width] elements of the same
 * dtype (all seven), each with its own row / band stride (frs_raster_desc, nbands 1..8, equal).  The source is H x W,
 * the destination h x w.  The map's rectangle x0, y0, width, height is in pixel-EDGE coordinates of the source (pixel i
 * covers [i, i+1)) and may reach outside it.  Per axis, with N the source and n the destination extent:
 * step = span / n, lo(j) = x0 + j*step, hi(j) = x0 + (j+1)*step, centre(j) = x0 + (j+0.5)*step, each operator one IEEE
 * fp64 operation (csrc/frs_window_map.h holds the arithmetic for host and device).
 *   FRS_RESAMPLE_NEAREST    i = floor(centre); the pixel is valid iff 0 <= i < N on both axes
 *   FRS_RESAMPLE_BILINEAR   valid iff 0 <= floor(centre) < N; u = centre - 0.5, i0 = floor(u), t = u - i0; taps i0 and
 *                           i0 + 1, each clamped to [0, N-1], weights 1 - t and t; the value is
 *                           (a(1-tx) + b tx)(1-ty) + (c(1-tx) + d tx) ty with a, b on the upper row
 *   FRS_RESAMPLE_AVERAGE    clo = max(lo, 0), chi = min(hi, N); valid iff chi > clo on both axes; taps floor(clo) ..
 *                           ceil(chi) - 1 with weight min(chi, i+1) - max(clo, i); the value is (sum over rows ascending
 *                           of wy * (sum over columns ascending of wx * v)) / ((chi_x - clo_x)(chi_y - clo_y)), both sums
 *                           from 0.0.  The tap count is not capped (a 150x reduction reads 150 x 150 taps per pixel).
 * Source values are converted to double (exact).  Integer results round half to EVEN, are clamped to the dtype's range
 * and cast (frs_downsample2's integer average rounds half towards +infinity: a different call with a different
 * definition); float32 narrows the double, float64 keeps it; NaN and +-inf come out as the expression gives them.  A
 * pixel that is not valid gets map->fill, converted by the same rule; a rectangle wholly outside the source is FRS_OK
 * and fills the destination.  With x0 = y0 = 0, width = W = w, height = H = h every mode returns a finite source
 * unchanged.  The definition is this library's own; no parity with GDAL is claimed.
 * Destination elements outside [h][w] are never written, the row padding of row_stride > width included (whole 16-byte
 * chunks of a destination row by aligned 16-byte stores, the rest element by element); nothing is read outside the
 * source's [H][W].  FRS_E_ARG: a size < 1, row_stride < width, nbands outside 1..8 or unequal, dtypes unequal or unknown,
 * a band_stride (nbands > 1) smaller than (height-1)*row_stride + width, an extent that overflows 63 bits, an unknown
 * mode, a null pointer or one not aligned to the element size, source and destination byte ranges (origin to the end
 * of the last row) that overlap, a non-finite map field (fill included), width <= 0 or height <= 0, and a coordinate
 * (x0, y0, width, height, x0 + width, y0 + height) of magnitude >= 2^52.  Synchronous on the context stream; profile
 * entry "resample".  frs_resample_window takes host rasters: both are copied through the context's staging buffers (the
 * destination goes up first and comes back whole, so its padding survives). */
typedef struct { double x0, y0, width, height, fill; } frs_window_map;
int frs_resample_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                               const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map, int32_t mode);
int frs_resample_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host, const frs_raster_desc *dst,
                        void *dst_host, const frs_window_map *map, int32_t mode);

/* The nodata-aware forms of the two calls above: the same descriptors, validation, synchrony and profile entries
 * ("pyramid", "resample"), with a trailing nodata value that marks pixels which hold no data.  They keep a nodata
 * collar or hole from being averaged into its neighbours.  csrc/frs_nodata.h holds the arithmetic for host and device;
 * the definitions are this library's own, no parity with GDAL is claimed.
 * Predicate, with ndT = (T)nodata.  Integer dtypes: nodata must be an integer value inside the dtype's range (FRS_E_ARG
 * otherwise, NaN included); a pixel is nodata iff it equals ndT.  Float dtypes: a pixel is nodata iff it equals ndT or
 * both are NaN; +-inf is allowed; -0.0 matches 0.0.
 * frs_downsample2_nodata*, FRS_RESAMPLE_AVERAGE: the block is frs_downsample2's (n = 4, 2 or 1 pixels); its m <= n valid
 * pixels v1 .. vm are taken in the order a, b, c, d.  m = 0 gives ndT.  Integers: floor((2s + m) / (2m)) of the exact
 * 64-bit sum s of the valid pixels, the mean rounded half towards +infinity.  Floats: ((v1 + v2) + (v3 + v4)) * 0.25 for
 * m = 4, ((v1 + v2) + v3) / 3 for m = 3, (v1 + v2) * 0.5 for m = 2, v1 for m = 1, every operation rounded in the dtype.
 * A block with every pixel valid gives frs_downsample2's result bit for bit, before the nudge: an integer mean (m > 0,
 * m = n included) that equals ndT becomes ndT + 1, or ndT - 1 when ndT is the dtype's maximum, so that no hole appears
 * where data exists; floats are not nudged.  FRS_RESAMPLE_NEAREST is frs_downsample2's: the pixel (2r, 2x) is copied, nodata or not.
 * frs_resample_window_nodata*: indices, weights and axis validity are frs_resample_window's.  An output whose valid
 * weight is zero (outside the source, all taps nodata, or only zero-weight taps valid) gets map->fill.  Nearest: a
 * nodata tap gives fill.  Bilinear: with all four taps valid the value is frs_resample_window's; otherwise, with
 * w00 = (1-tx)(1-ty), w01 = tx(1-ty), w10 = (1-tx)ty, w11 = tx ty and num = den = 0.0, the valid taps are accumulated in
 * the order 00, 01, 10, 11 (num = num + w v, den = den + w) and the value is num / den, or fill when den == 0.  Average:
 * per row over its valid taps, columns ascending, row = row + wx v and roww = roww + wx; then, rows ascending,
 * sum = sum + wy row and wsum = wsum + wy roww; with no tap nodata the value is frs_resample_window's, otherwise
 * sum / wsum, or fill when wsum == 0.  Integer results are rounded as in frs_resample_window and nudged off ndT as
 * above.  map->fill must be finite; for float dtypes it may also be NaN. */
int frs_downsample2_nodata_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                  const frs_raster_desc *dst, void *dst_dev, int32_t mode, double nodata);
int frs_downsample2_nodata(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host, const frs_raster_desc *dst,
                           void *dst_host, int32_t mode, double nodata);
int frs_resample_window_nodata_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                      const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map,
                                      int32_t mode, double nodata);
int frs_resample_window_nodata(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host,
                               const frs_raster_desc *dst, void *dst_host, const frs_window_map *map, int32_t mode,
                               double nodata);

/* Statistics and histogram of the bands of ONE raster, each in one pass over every band: what a caller needs to stretch
 * a window for display, check a nodata collar or sanity-check a conversion (gdalinfo -stats -hist).  The reference has
 * no such call.  The raster is band-planar [nbands][height][width] elements with row / band strides in elements
 * (frs_raster_desc, all seven dtypes, nbands 1..8).  nodata is null, or points at the nodata value (predicate of the
 * nodata-aware calls above).  csrc/frs_stats.h holds the arithmetic for host and device; the definitions are this
 * library's own.
 * Validity: a pixel is nodata by that predicate (only when a value is given); otherwise NaN (float dtypes only);
 * otherwise valid.  +-inf are valid values.  Everything but the three counts is over the valid pixels.
 * frs_band_stats*, out_host[nbands]:
 *   n_valid, n_nodata, n_nan   the three classes (they add up to height*width)
 *   min, max                   as double, exact for every dtype; NaN when n_valid == 0
 *   sum                        integers: the exact sum rounded once; floats: an fp64 sum of (double)v in a fixed order
 *                              that depends on shape, dtype and layout only (bit-reproducible)
 *   isum_hi, isum_lo           integer dtypes: the exact sum as a signed 128-bit value; 0 for floats
 *   isq_hi, isq_lo             integer dtypes: the exact sum of squares as an unsigned 128-bit value; 0 for floats
 * frs_band_histogram*, with scale = (double)nbins / (hi - lo) computed once and x = (double)v of a valid pixel:
 * x < lo counts in `below`, x > hi in `above`, otherwise bin floor((x - lo) * scale), clamped to nbins - 1.  With
 * lo = m, hi = M + 1, nbins = M - m + 1 every integer value m .. M has a bin of its own.  counts_host is
 * [nbands][nbins]; out_host[nbands] holds below, above and, for float dtypes, m2 = the sum of (x - centre)^2 over the
 * valid pixels in the same kind of fixed order (0 for integer dtypes, whose exact sum of squares the first call gives).
 * Nothing outside [height][width] is read (16-byte loads cut at the 16-byte boundaries of each row, or of the band when
 * row_stride == width).  FRS_E_ARG, before anything is launched or written: the descriptor errors of
 * frs_resample_window*, a null pointer or one not aligned to the element size, a nodata value the dtype cannot hold,
 * nbins outside 1..16384, lo, hi, hi - lo or centre not finite, hi <= lo, and a shape in which one work-group would fold
 * more than 2^30 elements (beyond ~2^40 elements).  Synchronous on the context stream; profile entries "band_stats" and
 * "band_hist".  The host variants copy the raster through the context's staging buffer. */
typedef struct {
    int64_t n_valid, n_nodata, n_nan;
    double min, max, sum;
    int64_t isum_hi;
    uint64_t isum_lo;
    uint64_t isq_hi, isq_lo;
} frs_band_stats_out;
typedef struct {
    double lo, hi;
    int32_t nbins;
    double centre;
} frs_hist_params;
typedef struct {
    uint64_t below, above;
    double m2;
} frs_band_hist_out;
int frs_band_stats_device(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_dev, const double *nodata,
                          frs_band_stats_out *out_host);
int frs_band_stats(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_host, const double *nodata,
                   frs_band_stats_out *out_host);
int frs_band_histogram_device(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_dev, const double *nodata,
                              const frs_hist_params *params, uint64_t *counts_host, frs_band_hist_out *out_host);
int frs_band_histogram(frs_ctx *ctx, const frs_raster_desc *desc, const void *raster_host, const double *nodata,
                       const frs_hist_params *params, uint64_t *counts_host, frs_band_hist_out *out_host);

/* Render a rectangle of ONE band as stretched 8-bit colour: frs_resample_window* fused with a quantiser, a colour
 * look-up table and an alpha for "no data", so that a windowed read leaves the device as the w x h x C bytes a viewer
 * shows.  The reference has no such call; csrc/frs_render.h holds the arithmetic for host and device, the definition is
 * this library's own.  The source is one band (nbands == 1) of any of the seven dtypes, laid out as in
 * frs_resample_window*; map, mode and nodata (null, or a pointer at the nodata value) mean what they mean there, but
 * map->fill is ignored.  One output pixel comes from one resampled value v in the source dtype and a flag has_data:
 *   v, has_data   v is exactly what frs_resample_window* (the _nodata form when nodata is given) writes for the pixel:
 *                 same taps, weights, rounding and nudge.  has_data is false exactly where that call writes fill (an
 *                 axis is invalid, masked nearest hit a nodata tap, a masked output has no valid weight) and, for float
 *                 rasters, where v is NaN.  +-inf are data.
 *   quantise      scale = (double)n / (hi - lo), computed once.  x = (double)v < lo gives index 0, x > hi gives n - 1,
 *                 otherwise min((int64)floor((x - lo) * scale), n - 1): frs_band_histogram*'s bin rule, every step one
 *                 IEEE fp64 operation.
 *   colour        rgba = lut[index]; lut holds n entries of 4 bytes R, G, B, A (a host pointer: the call copies it).  A
 *                 pixel without data takes nodata_rgba = R | G << 8 | B << 16 | A << 24.  Gamma, a logarithmic transfer
 *                 and the colour ramp are all in the LUT, which is why n goes up to 4096.
 *   channels      C = 1: R;  C = 2: R, A;  C = 4: R, G, B, A.
 * The destination is pixel-interleaved uint8 [height][width][C]: dst->dtype FRS_DT_U8, dst->width in pixels,
 * dst->row_stride in BYTES (>= width * C), dst->nbands 1.  No byte outside [height][width * C] of any row is written
 * (whole 16-byte chunks of a destination row by aligned 16-byte stores, the rest byte by byte); nothing is read outside
 * the source's [H][W].  FRS_E_ARG, before anything is sized, copied or launched: everything frs_resample_window*
 * rejects of the descriptors, the mode, the rectangle, the nodata value and the pointers (the source's aligned to its
 * element size), and nbands != 1, channels not 1, 2 or 4, n outside 1..4096, a null LUT, lo or hi or hi - lo not finite,
 * hi <= lo, a destination that is not uint8, a byte row stride < width * C, and source and destination byte ranges that
 * overlap.  Synchronous on the context stream; profile entry "render".  frs_render_window takes host rasters: both are
 * copied through the context's staging buffers (the destination goes up first and comes back whole, so its padding
 * survives). */
typedef struct {
    double lo, hi;
    const uint8_t *lut; /* host: n * 4 bytes */
    int32_t n;
    uint32_t nodata_rgba;
    int32_t channels;
} frs_render_params;
int frs_render_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev, const frs_raster_desc *dst,
                             void *dst_dev, const frs_window_map *map, int32_t mode, const double *nodata,
                             const frs_render_params *render);
int frs_render_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host, const frs_raster_desc *dst,
                      void *dst_host, const frs_window_map *map, int32_t mode, const double *nodata,
                      const frs_render_params *render);

/* The render above with hillshade: Horn's 3 x 3 gradient taken on the OUTPUT grid, a Lambertian shade, and the colour
 * scaled by a 256-entry table.  csrc/frs_shade.h holds the arithmetic for host and device; the definition is this
 * library's own (the gradient is Horn's, as in gdaldem hillshade, but no parity with GDAL is claimed).  Every step is
 * one IEEE fp64 operation.  src, dst, map, mode, nodata and render mean what they mean in frs_render_window*.
 *   samples    For an output pixel (x, y), z[dy][dx], dx, dy in {-1, 0, +1}, is the resampled value at output position
 *              (x + dx, y + dy) under the call's own mapping, converted to double.  Positions -1 and width / height are
 *              included: they are plain arithmetic in the position, so the apron comes from the raster, not from
 *              replication (two neighbouring map tiles shade identically along their seam when the source reaches one
 *              output pixel beyond the box).  A sample has no data where frs_render_window* finds none (NaN included;
 *              +-inf are data).  A centre without data gives nodata_rgba; a neighbour without data is replaced by the
 *              centre's value.
 *   gradient   Rows grow southwards; 2z is z + z, every sum left to right as written:
 *              gx = (z[-1][+1] + (z[0][+1] + z[0][+1]) + z[+1][+1]) - (z[-1][-1] + (z[0][-1] + z[0][-1]) + z[+1][-1])
 *              gy = (z[+1][-1] + (z[+1][0] + z[+1][0]) + z[+1][+1]) - (z[-1][-1] + (z[-1][0] + z[-1][0]) + z[-1][+1])
 *              p = gx * kx, q = gy * ky, with kx = z_factor / (8 cell_x), ky = z_factor / (8 cell_y) computed by the
 *              caller from the ground size of an OUTPUT pixel.
 *   shade      (lx, ly, lz) is the unit vector towards the light: sin A cos h, cos A cos h, sin h for the azimuth A
 *              clockwise from north and the altitude h (the trigonometry is the caller's).
 *              num = (lz - p * lx) + q * ly;  den = sqrt((1.0 + p * p) + q * q), correctly rounded;  s = num / den;
 *              k = 0 when s > 0 is false (NaN included), otherwise min((int)floor(s * 256.0), 255).
 *   colour     rgba = lut[index of the centre value], the plain render's colour; m = table[k]; R, G and B each become
 *              (c * m + 127) / 255 in integer arithmetic, A is untouched.  C = 1 stores the shaded R, C = 2 the shaded
 *              R and A, C = 4 R, G, B, A.  With m = 255 the pixel is frs_render_window*'s.
 * FRS_E_ARG, before anything is sized, copied or launched: everything frs_render_window* rejects, a null `shade` or
 * table, and any of the five doubles not finite.  The store contract is frs_render_window*'s.  Synchronous on the
 * context stream; profile entry "render_shaded".  frs_render_shaded_window takes host rasters, staged like
 * frs_render_window's. */
typedef struct {
    double lx, ly, lz, kx, ky;
    const uint8_t *table; /* host: 256 bytes */
} frs_shade_params;
int frs_render_shaded_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                    const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map, int32_t mode,
                                    const double *nodata, const frs_render_params *render,
                                    const frs_shade_params *shade);
int frs_render_shaded_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host,
                             const frs_raster_desc *dst, void *dst_host, const frs_window_map *map, int32_t mode,
                             const double *nodata, const frs_render_params *render, const frs_shade_params *shade);

/* Render a rectangle of THREE bands as one stretched 8-bit colour image: frs_render_window* with a plane per colour
 * channel, in one pass over the output (the tap indices and weights of an output are computed once and applied to the
 * three planes).  csrc/frs_composite.h holds the arithmetic for host and device; the definition is this library's own.
 * The source is band-planar [3][H][W] of any of the seven dtypes (src->nbands == 3, row and band strides in elements,
 * band_stride >= (H - 1) * row_stride + W); map, mode and nodata (null, or a pointer at the one nodata value of all
 * three planes) mean what they mean in frs_render_window*.
 *   v_c, has_data_c   for c in {0, 1, 2}: exactly what frs_render_window* computes for plane c alone: same taps,
 *                     weights, rounding, nudge and NaN rule.
 *   quantise          i_c = the index frs_render_window* gives v_c under lo[c], hi[c] and n.
 *   colour            byte c of the pixel is byte c of lut[i_c]: R from the R bytes of the table, G from its G bytes, B
 *                     from its B bytes (a grey ramp with gamma is three equal curves; the columns may differ).  A = 255.
 *                     A pixel where any of the three planes has no data is nodata_rgba, whole.
 * lut holds n (1 .. 4096) entries of 4 bytes R, G, B, A (a host pointer: the call copies it); nodata_rgba is packed
 * R | G << 8 | B << 16 | A << 24.  The destination is pixel-interleaved uint8 [height][width][4] (R, G, B, A; no other
 * channel count): dst->dtype FRS_DT_U8, dst->width in pixels, dst->row_stride in BYTES (>= width * 4), dst->nbands 1.
 * No byte outside [height][width * 4] of any row is written (whole 16-byte chunks of a destination row by aligned
 * 16-byte stores, the rest byte by byte); nothing is read outside any plane's [H][W].  FRS_E_ARG, before anything is
 * sized, copied or launched: everything frs_render_window* rejects (with C = 4, and each lo[c], hi[c] pair checked like
 * its lo, hi), except that src->nbands must be 3; a band stride smaller than the plane's extent; null parameters; and a
 * destination that overlaps any of the three planes.  Synchronous on the context stream; profile entry
 * "render_composite".  frs_render_composite_window takes host rasters, staged like frs_render_window's. */
typedef struct {
    double lo[3], hi[3];
    const uint8_t *lut; /* host: n * 4 bytes */
    int32_t n;
    uint32_t nodata_rgba;
} frs_composite_params;
int frs_render_composite_window_device(frs_ctx *ctx, const frs_raster_desc *src, const void *src_dev,
                                       const frs_raster_desc *dst, void *dst_dev, const frs_window_map *map,
                                       int32_t mode, const double *nodata, const frs_composite_params *composite);
int frs_render_composite_window(frs_ctx *ctx, const frs_raster_desc *src, const void *src_host,
                                const frs_raster_desc *dst, void *dst_host, const frs_window_map *map, int32_t mode,
                                const double *nodata, const frs_composite_params *composite);

/* Multi-GPU create-streaming (one process per GPU).  The reference's tile loop (cli.py:690-763) is
 * serial; here tiles shard by contiguous tile rows and the only exchange is an RCCL all-gather (xGMI) of per-tile
 * byte sizes, after which every rank writes its own tiles at their file offsets.  librccl.so is loaded at run
 * time; rank 0 calls frs_comm_unique_id and the host ships the FRS_COMM_ID_BYTES bytes to every rank (any
 * bootstrap: flac_raster_amd/distributed.py uses a TCP star), then each rank calls frs_comm_init with its context
 * (one GPU per rank).  frs_comm_allgather_i64: `count` int64 per rank, host in/out, result in rank order;
 * synchronous on the context's stream. */
typedef struct frs_comm frs_comm;
#define FRS_COMM_ID_BYTES 128
int frs_comm_unique_id(uint8_t *id_out);
int frs_comm_init(frs_ctx *ctx, const uint8_t *id, int32_t nranks, int32_t rank, frs_comm **out);
void frs_comm_destroy(frs_comm *comm);
int frs_comm_allgather_i64(frs_comm *comm, const int64_t *send_host, int64_t count, int64_t *recv_host);

/* Device memory helpers so hosts need no other GPU runtime binding (no PyTorch in the codec path). */
void *frs_dev_malloc(frs_ctx *ctx, int64_t bytes);
void frs_dev_free(frs_ctx *ctx, void *ptr);
/* Page-locked host memory: an arena_host given to frs_encode_tiles in such memory takes the frames back at DMA rate
 * (a fresh pageable buffer is page-faulted and pinned page by page during the copy).  create-streaming writes the
 * file straight from it (streaming.create_streaming_array). */
void *frs_host_malloc(frs_ctx *ctx, int64_t bytes);
void frs_host_free(frs_ctx *ctx, void *ptr);
int frs_memcpy_h2d(frs_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes);
int frs_memcpy_d2h(frs_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes);
int frs_ctx_sync(frs_ctx *ctx);

/* Benchmark input: fills a [bands][height][width] int16 raster in device memory with the survey's
 * synthetic multispectral DEM: band b = int16(1000 + 300 sin(X(0.5+0.3b)) cos(0.3Y)
 * + 150 sin(1.2X) sin(1.1Y) + 50 u), X,Y = linspace(0, 20) over the full raster width/height, u a
 * counter-based uniform [0,1) draw of (seed, b, y, x).  Rows [row0, row0+height) of a raster of
 * full_height rows are generated (multi-GPU slabs).  Parity never depends on this generator: tests
 * download what it produced and feed the same bytes to the oracle. */
int frs_synth_raster_device(frs_ctx *ctx, int16_t *dev, int32_t bands, int64_t height, int64_t width,
                            int64_t row0, int64_t full_height, uint64_t seed);

/* Stream of the context (hipStream_t as void*) so callers can order their own work / events with it. */
void *frs_ctx_stream(frs_ctx *ctx);
/* Average device time (ms) of the named kernel over the launches since the last reset, measured with
 * HIP events on the context stream (kernel: "encode" = the frame-encode kernel, "analyze", "stats",
 * "compact", "decode", "compare", "place", "pyramid", "resample", "band_stats", "band_hist", "render",
 * "render_shaded", "render_composite"); returns -1 when not recorded.  frs_profile_enable(ctx, 1) turns recording on. */
int frs_profile_enable(frs_ctx *ctx, int on);
double frs_profile_avg_ms(frs_ctx *ctx, const char *kernel);
void frs_profile_reset(frs_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* FLAC_RASTER_AMD_H */
