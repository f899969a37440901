// frs_place.hip -- place decoded tiles at their windows of a strided, band-planar raster (frs_place_tiles_device,
// frs_decode_tiles_window*): the decoder-side mirror of the encoder's strided raster view.
//
// Host paths replaced: streaming.extract_bbox_mosaic's loop (np.zeros of the union window, one slice assignment per
// tile, a second copy for the crop) and converter.py's `.reshape(H, W, C).transpose(2, 0, 1)` + ascontiguousarray after a
// multi-band decode.  The decoders keep writing what they write today -- tile t as width*height pixels in row-major
// order, C interleaved elements each, from element pcm_off[t] * C -- and this kernel moves those bytes to
//     dst + c*band_stride + (row_off[t] + r)*row_stride + (col_off[t] + x)
// clipped to the destination.  It moves bytes and nothing else, so one instantiation per element size serves every dtype.
//
//   k_place_tiles   grid (ntiles, row blocks), 256 threads.  Work-group (t, b) owns rows [b*R, b*R + R) of tile t, with
//                   R = 16 KiB / (width * C * element size) clamped to 1..height: a 512-px int16 tile is 32 work-groups
//                   of 16 rows, a 64-px edge tile 4 work-groups of 128 rows, so an edge tile costs what its bytes cost.
//                   The tile's table entry is indexed by blockIdx.x alone: it arrives in SGPRs by scalar loads, and the
//                   clipping and the row range are scalar arithmetic.
//
// Store side (it decides the speed: a 2-byte store costs about 12.5x a 16-byte store per byte).  A clipped row of a
// band plane is cut at the 16-byte boundaries of the DESTINATION: chunk k of a row is the 16 bytes at
// align_down(row start, 16) + 16k.  A work-group's items are (row, chunk) pairs, one per lane and step.  A chunk that
// lies wholly inside the row is written with one aligned 16-byte store; the first and last chunk of a row, when the row
// does not start or end on a boundary, are written element by element (the scalar head and tail).  Source and
// destination rows differ in alignment, and the difference changes from row to row when width*es or row_stride*es is
// no multiple of 16 (Sentinel-2: 10980 int16 columns, tile 1024, 740-px edge tiles), so the alignment is worked out
// per item from the destination address, never per tile.
//
// Load side: the 16 source bytes of a chunk start wherever the destination's alignment puts them, so they are read with
// UNALIGNED 16-byte global loads (gfx950 global memory instructions take any byte address; the code object runs with
// unaligned access enabled, the HSA default).  The alternative -- two aligned loads and four v_alignbyte per chunk, with
// the shift kept per lane because it changes per row -- doubles the load instructions to save nothing a bandwidth kernel
// is short of: an unaligned 16-byte load touches at most one 64-byte line more than an aligned one, and the neighbouring
// lane reads that line anyway.  What the compiler makes of it: one global_load_dwordx4 and one
// global_store_dwordx4 per chunk for one channel, C global_load_dwordx4 and C global_store_dwordx4 for C = 2, 3, 4.
//
// More than one channel: a lane's chunk is 16 / es whole pixels; it reads their C * 16 contiguous source bytes,
// de-interleaves them in registers and writes one 16-byte store per band plane.  The chunk grid is plane 0's; a plane
// whose offset c*band_stride*es is a multiple of 16 gets the same aligned stores, any other plane gets the same single
// store instruction at an unaligned address (correct, slower).  C = 2, 3, 4 are specialised; 5..8 share one loop that
// gathers a plane's elements one by one (strided loads that hit the lines the lane has just read) and still writes wide.
//
// Not checked, by contract: the windows of one call must not overlap inside the destination (two tiles would race for
// the same elements).  Destination elements no tile covers -- row padding included -- are never written.
#include <algorithm>

#include "frs_internal.h"

namespace frs {

constexpr int kPlaceBlock = 256;          // threads per work-group
constexpr int kPlaceGroupBytes = 16384;   // tile bytes one work-group moves (4 chunks per lane and plane)
constexpr int kPlaceMaxGridY = 32768;     // row blocks beyond this are strided over

// device copy of one tile's window and source position (32 bytes: two scalar loads)
struct PlaceTile {
    int64_t col_off, row_off;
    int32_t width, height;
    int64_t pcm_off;
};

struct PlaceParams {
    int64_t height, width, row_stride, band_stride;
    int32_t channels;
};

// rows of a tile one work-group owns (the same value on the host, which sizes the grid with it)
__host__ __device__ inline int64_t place_rows_per_group(int64_t w, int64_t h, int es, int channels) {
    int64_t r = kPlaceGroupBytes / (w * es * channels);
    r = r < 1 ? 1 : r;
    return r < h ? r : h;
}

template <int ES> struct PlaceElem;
template <> struct PlaceElem<1> { using T = uint8_t; };
template <> struct PlaceElem<2> { using T = uint16_t; };
template <> struct PlaceElem<4> { using T = uint32_t; };
template <> struct PlaceElem<8> { using T = uint64_t; };

// One lane's share of a work-group: lane tid of the work-group that owns row blocks by, by + gy, ... of tile t.  (Plain
// C++, so that a host program can run it lane by lane against a direct evaluation, under a sanitizer.)
// CT: channels known at compile time (1..4), or 0 for the generic loop over P.channels (up to kMaxChannels)
template <int ES, int CT>
__host__ __device__ inline void place_group(const typename PlaceElem<ES>::T *__restrict__ src,
                                            typename PlaceElem<ES>::T *__restrict__ dst, const PlaceTile &t,
                                            const PlaceParams &P, int64_t by, int64_t gy, uint32_t tid) {
    using T = typename PlaceElem<ES>::T;
    constexpr int VE = 16 / ES;  // elements per 16-byte chunk
    const int C = CT ? CT : P.channels;
    const int64_t w = t.width, h = t.height;
    // the tile's part inside the destination, in tile coordinates
    const int64_t xlo = t.col_off < 0 ? -t.col_off : 0, xhi = std::min<int64_t>(w, P.width - t.col_off);
    const int64_t ylo = t.row_off < 0 ? -t.row_off : 0, yhi = std::min<int64_t>(h, P.height - t.row_off);
    if (xlo >= xhi || ylo >= yhi) return;  // wholly outside
    const int64_t R = place_rows_per_group(w, h, ES, C);
    const int64_t nblk = (h + R - 1) / R;
    const uint32_t n = (uint32_t)(xhi - xlo);      // clipped pixels per row
    const uint32_t cpr = (n + VE - 1) / VE + 1;    // chunks a row can touch (one more when it starts off a boundary)
    for (int64_t rb = by; rb < nblk; rb += gy) {
        const int64_t r0 = std::max(rb * R, ylo), r1 = std::min(rb * R + R, yhi);
        if (r0 >= r1) continue;
        // R > 1 only for rows of <= 8 KiB, and one row has < 2^31 chunks: the item count fits 32 bits
        const uint32_t items = (uint32_t)(r1 - r0) * cpr;
        for (uint32_t it = tid; it < items; it += kPlaceBlock) {
            const uint32_t row = it / cpr, k = it - row * cpr;
            const int64_t r = r0 + row;
            // plane-0 element index of the row's first clipped pixel
            const int64_t de = (t.row_off + r) * P.row_stride + t.col_off + xlo;
            const uint32_t first = (uint32_t)(reinterpret_cast<uintptr_t>(dst + de) & 15) / ES;
            // chunk k holds the row's clipped pixels [p0, p0 + VE)
            const int64_t p0 = (int64_t)k * VE - first;
            const int64_t pa = p0 < 0 ? 0 : p0, pb = std::min<int64_t>(p0 + VE, n);
            if (pa >= pb) continue;
            const T *s = src + (t.pcm_off + r * w + xlo + pa) * C;
            T *d = dst + de + pa;
            if (pb - pa == VE) {  // a whole chunk: d is 16-byte aligned (plane 0)
                if constexpr (CT == 1) {
                    uint4 v;
                    __builtin_memcpy(&v, s, 16);  // unaligned 16-byte load
                    *reinterpret_cast<uint4 *>(d) = v;
                } else if constexpr (CT > 1) {
                    T in[VE * CT];
                    __builtin_memcpy(in, s, 16 * CT);
#pragma unroll
                    for (int c = 0; c < CT; c++) {
                        T o[VE];
#pragma unroll
                        for (int e = 0; e < VE; e++) o[e] = in[e * CT + c];
                        __builtin_memcpy(d + c * P.band_stride, o, 16);
                    }
                } else {
                    for (int c = 0; c < C; c++) {
                        T o[VE];
#pragma unroll
                        for (int e = 0; e < VE; e++) o[e] = s[e * C + c];
                        __builtin_memcpy(d + c * P.band_stride, o, 16);
                    }
                }
            } else {  // head or tail of the row: element by element
                const int m = (int)(pb - pa);
                for (int c = 0; c < C; c++)
                    for (int e = 0; e < m; e++) d[c * P.band_stride + e] = s[e * C + c];
            }
        }
    }
}

template <int ES, int CT>
__global__ void __launch_bounds__(kPlaceBlock) k_place_tiles(const typename PlaceElem<ES>::T *__restrict__ src,
                                                             typename PlaceElem<ES>::T *__restrict__ dst,
                                                             const PlaceTile *__restrict__ tab, PlaceParams P) {
    // the table entry is indexed by blockIdx.x alone: wave-uniform, scalar loads
    place_group<ES, CT>(src, dst, tab[blockIdx.x], P, blockIdx.y, gridDim.y, threadIdx.x);
}

template <int ES>
static void launch_place(hipStream_t st, dim3 grid, const void *src, void *dst, const PlaceTile *tab,
                         const PlaceParams &P) {
    using T = typename PlaceElem<ES>::T;
    const T *s = static_cast<const T *>(src);
    T *d = static_cast<T *>(dst);
    switch (P.channels) {
    case 1: k_place_tiles<ES, 1><<<grid, kPlaceBlock, 0, st>>>(s, d, tab, P); break;
    case 2: k_place_tiles<ES, 2><<<grid, kPlaceBlock, 0, st>>>(s, d, tab, P); break;
    case 3: k_place_tiles<ES, 3><<<grid, kPlaceBlock, 0, st>>>(s, d, tab, P); break;
    case 4: k_place_tiles<ES, 4><<<grid, kPlaceBlock, 0, st>>>(s, d, tab, P); break;
    default: k_place_tiles<ES, 0><<<grid, kPlaceBlock, 0, st>>>(s, d, tab, P); break;
    }
}

// The arguments are already validated (frs_abi.hip: check_place_args).  Synchronous on the context stream.
int place_job(frs_ctx *ctx, const frs_raster_desc *d, const void *tiles_dev, const int64_t *pcm_off,
              const frs_tile_window *win, int32_t ntiles, void *dst_dev) {
    if (ntiles == 0) return FRS_OK;
    const int es = dtype_size(d->dtype);
    const size_t bytes = (size_t)ntiles * sizeof(PlaceTile);
    FRS_HIP(ctx->place_pin.ensure(bytes));
    FRS_HIP(ctx->place_tab.ensure(bytes));
    PlaceTile *ht = ctx->place_pin.at<PlaceTile>(0);
    int64_t max_blk = 1;
    for (int32_t i = 0; i < ntiles; i++) {
        ht[i] = {win[i].col_off, win[i].row_off, win[i].width, win[i].height, pcm_off[i]};
        const int64_t R = place_rows_per_group(win[i].width, win[i].height, es, d->nbands);
        max_blk = std::max(max_blk, (win[i].height + R - 1) / R);
    }
    FRS_HIP(hipMemcpyAsync(ctx->place_tab.ptr, ht, bytes, hipMemcpyHostToDevice, ctx->stream));
    PlaceParams P;
    P.height = d->height, P.width = d->width, P.row_stride = d->row_stride, P.band_stride = d->band_stride;
    P.channels = d->nbands;
    const dim3 grid((unsigned)ntiles, (unsigned)std::min<int64_t>(max_blk, kPlaceMaxGridY));
    const PlaceTile *tab = ctx->place_tab.as<PlaceTile>();
    hipEvent_t ev;
    prof_begin(ctx, "place", &ev);
    switch (es) {
    case 1: launch_place<1>(ctx->stream, grid, tiles_dev, dst_dev, tab, P); break;
    case 2: launch_place<2>(ctx->stream, grid, tiles_dev, dst_dev, tab, P); break;
    case 4: launch_place<4>(ctx->stream, grid, tiles_dev, dst_dev, tab, P); break;
    default: launch_place<8>(ctx->stream, grid, tiles_dev, dst_dev, tab, P); break;
    }
    prof_end(ctx, "place", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FRS_OK;
}

}  // namespace frs
