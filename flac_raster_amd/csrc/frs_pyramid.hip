// frs_pyramid.hip -- one 2x reduction step of the overview pyramid (frs_downsample2*): an H x W band-planar raster to
// ceil(H/2) x ceil(W/2), by the arithmetic of frs_resample.h (nearest, or the 2 x 2 block average) and, with a nodata
// value, of frs_nodata.h (the average of the block's valid pixels).
//
// There is no reference path: the reference's streaming files hold one resolution.  create-streaming --overviews
// (streaming.py) calls this once per level, level k from level k - 1, and encodes each level as a raster of its own.
//
//   k_downsample2          grid (gx, gy, nbands), 256 threads.  Work-group (bx, by, band) owns destination rows by,
//   k_downsample2_nodata   by + gy, ... of the band and, of each, the 16-byte chunks bx * 512 + {0, 256} + lane,
//                          striding gx * 512.  Row and band come from the block index alone: the row pointers, "is
//                          there a second source row" and the row's alignment are scalar.
//
// Both kernels are one lane function, downsample_group, with a mask policy (frs_nodata.h): NoNodata, or Nodata<T> with
// the nodata value, which exists for the average only (nearest copies (2r, 2x) whatever it holds, so with a nodata
// value the job still launches k_downsample2).  The policy changes what a lane computes from the bytes it has loaded,
// never what it loads or stores.
//
// It is a pure bandwidth kernel (reads 4 elements, writes 1), so the rules of frs_place.hip apply.  Store side: a
// destination row is cut at the 16-byte boundaries of the DESTINATION; chunk k of a row is the 16 bytes at
// align_down(row start, 16) + 16k.  A chunk that lies wholly inside the row leaves as one aligned 16-byte store per
// lane; the first and last chunk of a row that starts or ends off a boundary go element by element.  The alignment
// is worked out per row from the destination address (strides need not be multiples of 16 bytes).  Load side: a
// lane's chunk of 16 / ES outputs reads 32 contiguous bytes of each of two source rows, wherever the destination's
// alignment puts them: four UNALIGNED 16-byte global loads (two for nearest, or for the single last row of an odd
// height), all issued before the first is used; with two chunks per lane and step that is up to eight loads in
// flight per lane.  A whole chunk whose last output would need the column past an odd width takes the
// element path as well, so nothing is read past a source row's `width` or past the last row.  No LDS, no atomics, no
// init pass; destination elements outside [height][width] are never written.
//
// Masked: a lane compares the elements of a wide chunk with the nodata value as it unpacks them.  A chunk without a
// hit (the common case) takes the unmasked expressions (an integer mean that lands on the nodata value is still nudged
// off it), one with a hit counts and sums the valid pixels of each output.  The branch is per lane; a wave none of
// whose lanes has a hit never enters the second form.
//
// Average instantiates per dtype (the sum and the rounding differ); nearest moves bytes and is instantiated per
// element size.
#include <algorithm>

#include "frs_internal.h"
#include "frs_nodata.h"
#include "frs_resample.h"

namespace frs {

constexpr int kPyrBlock = 256;         // threads per work-group
constexpr int kPyrUnroll = 2;          // chunks per lane and step (4 loads each)
constexpr int kPyrMaxGridY = 32768;    // destination rows beyond this are strided over

struct PyrParams {
    int64_t src_h, src_w, dst_h, dst_w;
    int64_t src_row_stride, src_band_stride, dst_row_stride, dst_band_stride;
};

// element type of a (dtype, mode) pair: the dtype's own for the average, an unsigned integer of its size for nearest
template <int ES, int DT> struct PyrElem;
template <> struct PyrElem<1, 0> { using T = uint8_t; };
template <> struct PyrElem<2, 0> { using T = uint16_t; };
template <> struct PyrElem<4, 0> { using T = uint32_t; };
template <> struct PyrElem<8, 0> { using T = uint64_t; };
template <> struct PyrElem<1, FRS_DT_U8> { using T = uint8_t; };
template <> struct PyrElem<2, FRS_DT_U16> { using T = uint16_t; };
template <> struct PyrElem<2, FRS_DT_I16> { using T = int16_t; };
template <> struct PyrElem<4, FRS_DT_I32> { using T = int32_t; };
template <> struct PyrElem<4, FRS_DT_U32> { using T = uint32_t; };
template <> struct PyrElem<4, FRS_DT_F32> { using T = float; };
template <> struct PyrElem<8, FRS_DT_F64> { using T = double; };

typedef uint32_t pyr_u32x4 __attribute__((ext_vector_type(4)));

// The 16 loaded bytes as an opaque value: without it the compiler splits a 16-byte load of which only every other
// element is used (nearest) into element-sized loads, 16 global_load_ubyte per uint8 chunk.  No instruction is emitted.
__host__ __device__ inline void pyr_keep_wide(pyr_u32x4 &q) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(q));
#else
    (void)q;
#endif
}

// does any element of the 32 bytes equal nd?  Integers of 1 and 2 bytes: `pat` is nd in every element of a 32-bit
// word; w ^ pat has a zero element exactly where w holds nd, and (x - ones) & ~x & tops is non-zero iff x has a zero
// element (the borrow of a zero element can only reach elements above it, so the test as a whole is exact).
template <typename T> __host__ __device__ inline bool pyr_any_nodata(const pyr_u32x4 (&q)[2], T nd) {
    if constexpr (!NdFloat<T>::value && sizeof(T) <= 2) {
        constexpr uint32_t ones = sizeof(T) == 1 ? 0x01010101u : 0x00010001u, tops = ones << (8 * sizeof(T) - 1);
        const uint32_t pat = (uint32_t)(typename PyrElem<(int)sizeof(T), 0>::T)nd * ones;
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t x = q[i >> 2][i & 3] ^ pat;
            acc |= (x - ones) & ~x;
        }
        return (acc & tops) != 0;
    } else {
        T v[32 / sizeof(T)];
        __builtin_memcpy(v, q, 32);
        bool hit = false;
#pragma unroll
        for (int e = 0; e < (int)(32 / sizeof(T)); e++) hit |= nd_is(v[e], nd);
        return hit;
    }
}

// one output from its block, by the element path: a0 / a1 point at source (2r, 2x) and (2r+1, 2x); `right` / `below`
// say whether the block has a second column / row
template <int MODE, typename T, typename Mask>
__host__ __device__ inline T downsample_one(const T *a0, const T *a1, bool right, bool below, const Mask &mask) {
    if constexpr (MODE == kResampleNearest) return a0[0];
    else if constexpr (Mask::masked) {
        if (right && below) return nd_avg(a0[0], a0[1], a1[0], a1[1], 4, mask.nd);
        if (right) return nd_avg(a0[0], a0[1], a0[0], a0[0], 2, mask.nd);
        if (below) return nd_avg(a0[0], a1[0], a0[0], a0[0], 2, mask.nd);
        // (ndT itself, not the pixel: a float -0.0 or NaN of another payload)
        return nd_is(a0[0], mask.nd) ? mask.nd : a0[0];
    } else {
        if (right && below) return resample_avg4(a0[0], a0[1], a1[0], a1[1]);
        if (right) return resample_avg2(a0[0], a0[1]);
        if (below) return resample_avg2(a0[0], a1[0]);
        return a0[0];
    }
}

// One lane's share of a work-group: lane tid of work-group (bx of gx, by of gy) of one band (src / dst are the band's
// origins).  `mask` is NoNodata, or Nodata<T> for the masked average.  (Plain C++, so that a host program can run it
// lane by lane against a direct evaluation.)
template <int ES, int MODE, int DT, typename Mask>
__host__ __device__ inline void downsample_group(const typename PyrElem<ES, DT>::T *__restrict__ src,
                                                 typename PyrElem<ES, DT>::T *__restrict__ dst, const PyrParams &P,
                                                 const Mask &mask, int64_t bx, int64_t gx, int64_t by, int64_t gy,
                                                 uint32_t tid) {
    using T = typename PyrElem<ES, DT>::T;
    static_assert(!Mask::masked || MODE == kResampleAverage, "nearest has no masked form");
    constexpr int VE = 16 / ES;  // outputs per 16-byte chunk
    const int64_t w = P.dst_w, W = P.src_w;
    for (int64_t r = by; r < P.dst_h; r += gy) {
        const bool below = 2 * r + 1 < P.src_h;
        const T *s0 = src + 2 * r * P.src_row_stride;
        const T *s1 = s0 + (below ? P.src_row_stride : 0);  // (never read when !below)
        T *d = dst + r * P.dst_row_stride;
        const int64_t first = (int64_t)(reinterpret_cast<uintptr_t>(d) & 15) / ES;
        const int64_t cpr = (first + w + VE - 1) / VE;  // chunks the row touches
        for (int64_t k0 = bx * (kPyrBlock * kPyrUnroll); k0 < cpr; k0 += gx * (kPyrBlock * kPyrUnroll)) {
            // chunk k holds the row's outputs [pa, pb)
            int64_t pa[kPyrUnroll], pb[kPyrUnroll];
            bool wide[kPyrUnroll];
            pyr_u32x4 q0[kPyrUnroll][2], q1[kPyrUnroll][2];  // 32 bytes of source row 2r / 2r + 1 per chunk
#pragma unroll
            for (int u = 0; u < kPyrUnroll; u++) {
                const int64_t p0 = (k0 + u * kPyrBlock + tid) * VE - first;
                pa[u] = p0 < 0 ? 0 : p0;
                pb[u] = std::min<int64_t>(p0 + VE, w);
                // a whole chunk (d + pa is 16-byte aligned) whose 2 * VE source columns all exist
                wide[u] = pb[u] - pa[u] == VE && 2 * pb[u] <= W;
                if (wide[u]) {
                    __builtin_memcpy(q0[u], s0 + 2 * pa[u], 32);  // two unaligned 16-byte loads
                    if (MODE == kResampleAverage && below) __builtin_memcpy(q1[u], s1 + 2 * pa[u], 32);
                }
            }
#pragma unroll
            for (int u = 0; u < kPyrUnroll; u++) {
                if (pa[u] >= pb[u]) continue;
                if (wide[u]) {
                    T o[VE], in0[2 * VE], in1[2 * VE];
                    pyr_keep_wide(q0[u][0]), pyr_keep_wide(q0[u][1]);
                    __builtin_memcpy(in0, q0[u], 32);
                    if constexpr (MODE == kResampleNearest) {
#pragma unroll
                        for (int e = 0; e < VE; e++) o[e] = in0[2 * e];
                    } else if constexpr (!Mask::masked) {
                        if (below) {
                            pyr_keep_wide(q1[u][0]), pyr_keep_wide(q1[u][1]);
                            __builtin_memcpy(in1, q1[u], 32);
#pragma unroll
                            for (int e = 0; e < VE; e++)
                                o[e] = resample_avg4(in0[2 * e], in0[2 * e + 1], in1[2 * e], in1[2 * e + 1]);
                        } else {
#pragma unroll
                            for (int e = 0; e < VE; e++) o[e] = resample_avg2(in0[2 * e], in0[2 * e + 1]);
                        }
                    } else {
                        const T nd = mask.nd;
                        bool hit = pyr_any_nodata<T>(q0[u], nd);
                        if (below) {
                            pyr_keep_wide(q1[u][0]), pyr_keep_wide(q1[u][1]);
                            __builtin_memcpy(in1, q1[u], 32);
                            hit |= pyr_any_nodata<T>(q1[u], nd);
                        }
                        if (!hit) {  // the unmasked expressions (and, for integers, the nudge off ndT)
                            if (below) {
#pragma unroll
                                for (int e = 0; e < VE; e++)
                                    o[e] = nd_nudge(
                                        resample_avg4(in0[2 * e], in0[2 * e + 1], in1[2 * e], in1[2 * e + 1]), nd);
                            } else {
#pragma unroll
                                for (int e = 0; e < VE; e++)
                                    o[e] = nd_nudge(resample_avg2(in0[2 * e], in0[2 * e + 1]), nd);
                            }
                        } else if (below) {
#pragma unroll
                            for (int e = 0; e < VE; e++)
                                o[e] = nd_avg(in0[2 * e], in0[2 * e + 1], in1[2 * e], in1[2 * e + 1], 4, nd);
                        } else {
#pragma unroll
                            for (int e = 0; e < VE; e++)
                                o[e] = nd_avg(in0[2 * e], in0[2 * e + 1], in0[2 * e], in0[2 * e], 2, nd);
                        }
                    }
                    uint4 v;
                    __builtin_memcpy(&v, o, 16);
                    *reinterpret_cast<uint4 *>(d + pa[u]) = v;
                } else {  // head or tail of the row, or the chunk with the last column of an odd width
                    for (int64_t x = pa[u]; x < pb[u]; x++)
                        d[x] = downsample_one<MODE>(s0 + 2 * x, s1 + 2 * x, 2 * x + 1 < W, below, mask);
                }
            }
        }
    }
}

// The two kernels differ in their arguments alone.
template <int ES, int MODE, int DT>
__global__ void __launch_bounds__(kPyrBlock) k_downsample2(const typename PyrElem<ES, DT>::T *__restrict__ src,
                                                           typename PyrElem<ES, DT>::T *__restrict__ dst, PyrParams P) {
    const int64_t band = blockIdx.z;
    downsample_group<ES, MODE, DT>(src + band * P.src_band_stride, dst + band * P.dst_band_stride, P, NoNodata{},
                                   blockIdx.x, gridDim.x, blockIdx.y, gridDim.y, threadIdx.x);
}

template <int ES, int DT>
__global__ void __launch_bounds__(kPyrBlock)
    k_downsample2_nodata(const typename PyrElem<ES, DT>::T *__restrict__ src,
                         typename PyrElem<ES, DT>::T *__restrict__ dst, PyrParams P, typename PyrElem<ES, DT>::T nd) {
    using T = typename PyrElem<ES, DT>::T;
    const int64_t band = blockIdx.z;
    downsample_group<ES, kResampleAverage, DT>(src + band * P.src_band_stride, dst + band * P.dst_band_stride, P,
                                               Nodata<T>{nd}, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y,
                                               threadIdx.x);
}

// nodata: null without one
template <int ES, int MODE, int DT>
static void launch_downsample(hipStream_t st, dim3 grid, const void *src, void *dst, const PyrParams &P,
                              const double *nodata) {
    using T = typename PyrElem<ES, DT>::T;
    const T *s = static_cast<const T *>(src);
    T *d = static_cast<T *>(dst);
    if constexpr (MODE == kResampleAverage) {
        if (nodata) {
            k_downsample2_nodata<ES, DT><<<grid, kPyrBlock, 0, st>>>(s, d, P, nd_cast<T>(*nodata));
            return;
        }
    }
    k_downsample2<ES, MODE, DT><<<grid, kPyrBlock, 0, st>>>(s, d, P);
}

// The arguments are already validated (frs_abi.hip: downsample_entry), the nodata value for the dtype as well (null:
// none).  Synchronous on the context stream.
int downsample_job(frs_ctx *ctx, const frs_raster_desc *s, const void *src, const frs_raster_desc *d, void *dst,
                   int32_t mode, const double *nodata) {
    const int es = dtype_size(d->dtype);
    PyrParams P;
    P.src_h = s->height, P.src_w = s->width, P.dst_h = d->height, P.dst_w = d->width;
    P.src_row_stride = s->row_stride, P.src_band_stride = s->band_stride;
    P.dst_row_stride = d->row_stride, P.dst_band_stride = d->band_stride;
    // chunks of the longest row (one more when it starts off a boundary); whole steps only, the rest is strided over
    const int64_t cpr = (d->width + 16 / es - 1) / (16 / es) + 1;
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(cpr / (kPyrBlock * kPyrUnroll), 65535));
    const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(d->height, kPyrMaxGridY), (unsigned)d->nbands);
    hipStream_t st = ctx->stream;
    hipEvent_t ev;
    prof_begin(ctx, "pyramid", &ev);
    if (mode == FRS_RESAMPLE_NEAREST) {
        switch (es) {
        case 1: launch_downsample<1, kResampleNearest, 0>(st, grid, src, dst, P, nodata); break;
        case 2: launch_downsample<2, kResampleNearest, 0>(st, grid, src, dst, P, nodata); break;
        case 4: launch_downsample<4, kResampleNearest, 0>(st, grid, src, dst, P, nodata); break;
        default: launch_downsample<8, kResampleNearest, 0>(st, grid, src, dst, P, nodata); break;
        }
    } else {
        switch (d->dtype) {
        case FRS_DT_U8: launch_downsample<1, kResampleAverage, FRS_DT_U8>(st, grid, src, dst, P, nodata); break;
        case FRS_DT_U16: launch_downsample<2, kResampleAverage, FRS_DT_U16>(st, grid, src, dst, P, nodata); break;
        case FRS_DT_I16: launch_downsample<2, kResampleAverage, FRS_DT_I16>(st, grid, src, dst, P, nodata); break;
        case FRS_DT_I32: launch_downsample<4, kResampleAverage, FRS_DT_I32>(st, grid, src, dst, P, nodata); break;
        case FRS_DT_U32: launch_downsample<4, kResampleAverage, FRS_DT_U32>(st, grid, src, dst, P, nodata); break;
        case FRS_DT_F32: launch_downsample<4, kResampleAverage, FRS_DT_F32>(st, grid, src, dst, P, nodata); break;
        default: launch_downsample<8, kResampleAverage, FRS_DT_F64>(st, grid, src, dst, P, nodata); break;
        }
    }
    prof_end(ctx, "pyramid", ev);
    FRS_HIP(hipGetLastError());
    FRS_HIP(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FRS_OK;
}

}  // namespace frs
