// trt_despeckle_kernels.h — trt_despeckle / trt_despeckle_device (include/trt.h) for gfx950.  The arithmetic is trt_despeckle.h's; this
// file only says which thread takes which pixel and where the taps come from.
//
//   k_despeckle<R, LDS>  one pixel per thread, 16 x 16 blocks (4 waves of 16 x 4).  Every thread reads its own pixel once (colour, albedo,
//                        depth, the variance if there is one: 28 or 32 bytes) and writes 12 to 20.  LDS = true: the block stages the
//                        demodulated luminance of its tile plus an R-pixel apron, (16 + 2R)^2 floats (1296 B at R = 1, 1600 B at R = 2):
//                        each thread stores its own pixel's, and the threads share out the 68 (R = 1) or 144 (R = 2) apron cells.  A cell
//                        whose pixel does not count (outside the image, a miss) holds NaN, so that a tap counts iff it is finite, and the
//                        (2R + 1)^2 - 1 taps read LDS.  LDS = false computes each tap's luminance from global memory (the A/B arm of
//                        TRT_DESPECKLE_LDS=0; same bits).
//                        The tile's rows are 18 or 20 floats apart: the two rows that one 32-lane half of a wave reads fall 2 (R = 1) or
//                        4 (R = 2) banks short of disjoint, so a tap read costs two LDS cycles for that half instead of one.  At 8 or
//                        24 reads per pixel beside 40 to 52 bytes of global traffic that is not what the kernel waits for.
#ifndef TRT_DESPECKLE_KERNELS_H
#define TRT_DESPECKLE_KERNELS_H

#include <hip/hip_runtime.h>

#include "trt_despeckle.h"

namespace trtd {

constexpr int DS_BX = 16, DS_BY = 16;

// The block's tile of luminances in LDS; element (0, 0) is image pixel (ox, oy).  trt_ds_pixel asks for the window of a pixel of the block
// only, and the tile holds a value (NaN outside the image) for every pixel of those windows.
template <int R>
struct DsFetchLds {
    const float* tile;
    int ox, oy;
    __device__ float operator()(int x, int y) const { return tile[(y - oy) * (DS_BX + 2 * R) + (x - ox)]; }
};

// The e-th cell of the apron, e in [0, 2R (16 + 2R) + 32R): the R rows above the tile, the R rows below it, then the R columns to either
// side of its 16 rows.  -> the cell's column and row in the (16 + 2R)^2 tile.
template <int R>
__device__ inline void dsApronCell(int e, int& ax, int& ay)
{
    constexpr int TW = DS_BX + 2 * R;
    if (e < R * TW) {
        ay = e / TW;
        ax = e % TW;
    } else if (e < 2 * R * TW) {
        e -= R * TW;
        ay = DS_BY + R + e / TW;
        ax = e % TW;
    } else {
        e -= 2 * R * TW;
        const int col = e % (2 * R);
        ay = R + e / (2 * R);
        ax = col < R ? col : DS_BX + col;
    }
}

// variance / out_variance (both or neither) and out_scale may be null.  No output may alias an input: a pixel reads its neighbours.
template <int R, bool LDS>
__global__ __launch_bounds__(DS_BX * DS_BY) void k_despeckle(trt_ds_args a, const float* __restrict__ color, const float* __restrict__ variance,
                                                             const float* __restrict__ albedo, const float* __restrict__ depth,
                                                             float* __restrict__ out_color, float* __restrict__ out_variance, float* __restrict__ out_scale)
{
    const int x = (int)(blockIdx.x * DS_BX + threadIdx.x), y = (int)(blockIdx.y * DS_BY + threadIdx.y);
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    float c[3] = {0.0f, 0.0f, 0.0f}, al[3] = {0.0f, 0.0f, 0.0f}, z = TRT_INF, var = 0.0f;
    if (inside) {
        c[0] = color[3 * p];
        c[1] = color[3 * p + 1];
        c[2] = color[3 * p + 2];
        al[0] = albedo[3 * p];
        al[1] = albedo[3 * p + 1];
        al[2] = albedo[3 * p + 2];
        z = depth[p];
        if (variance) var = variance[p];
    }
    const trt_ds_frame frame{color, albedo, depth, a.width, a.height};
    trt_ds_pixel_out o;
    if constexpr (LDS) {
        constexpr int TW = DS_BX + 2 * R, TH = DS_BY + 2 * R, APRON = TW * TH - DS_BX * DS_BY;
        __shared__ float tile[TW * TH];
        const int ox = (int)(blockIdx.x * DS_BX) - R, oy = (int)(blockIdx.y * DS_BY) - R;
        tile[((int)threadIdx.y + R) * TW + (int)threadIdx.x + R] = inside ? trt_ds_luminance(c, al, z) : trt_ds_nan();
        for (int e = (int)(threadIdx.y * DS_BX + threadIdx.x); e < APRON; e += DS_BX * DS_BY) {
            int ax, ay;
            dsApronCell<R>(e, ax, ay);
            tile[ay * TW + ax] = frame(ox + ax, oy + ay);
        }
        __syncthreads();
        if (!inside) return;
        o = trt_ds_pixel<R>(a, DsFetchLds<R>{tile, ox, oy}, x, y, c, al, z, var);
    } else {
        if (!inside) return;
        o = trt_ds_pixel<R>(a, frame, x, y, c, al, z, var);
    }
    out_color[3 * p] = o.color[0];
    out_color[3 * p + 1] = o.color[1];
    out_color[3 * p + 2] = o.color[2];
    if (out_variance) out_variance[p] = o.variance;
    if (out_scale) out_scale[p] = o.scale;
}

}  // namespace trtd

#endif  // TRT_DESPECKLE_KERNELS_H
