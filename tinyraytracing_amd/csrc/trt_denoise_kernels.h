// trt_denoise_kernels.h — the a-trous filter of trt_denoise / trt_denoise_device (include/trt.h) for gfx950.  The arithmetic is
// trt_denoise.h's; this file only decides where the pixels come from.
//
//   k_denoise_prepare   once per call: demodulates the input into cv (c, var), packs the guide gd (n, z) and aux (a, gz)
//   k_denoise_level     one launch per level, cv ping-pong; the last level remodulates into the caller's RGB buffer instead
//
// Blocks are 16 x 16 pixels (4 waves of 16 x 4).  Levels with steps 1 and 2 (aprons of 2 and 4 pixels) stage the block's tile plus
// apron of cv and gd in LDS (12.5 and 18 KiB), so the 25 taps and the 3 x 3 prefilter read LDS; wider steps read each tap's two 16-B
// records from global memory, where neighbouring blocks share them through L2 and the Infinity Cache.
#ifndef TRT_DENOISE_KERNELS_H
#define TRT_DENOISE_KERNELS_H

#include <hip/hip_runtime.h>

#include "trt_denoise.h"

namespace trtd {

constexpr int DN_BX = 16, DN_BY = 16;

__global__ __launch_bounds__(DN_BX * DN_BY) void k_denoise_prepare(int width, int height, const float* __restrict__ color,
                                                                   const float* __restrict__ variance, const float* __restrict__ albedo,
                                                                   const float* __restrict__ normal, const float* __restrict__ depth,
                                                                   trt_dn4* __restrict__ cv, trt_dn4* __restrict__ gd, trt_dn4* __restrict__ aux)
{
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    trt_dn4 a = trt_dn_factor(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]);
    cv[p] = trt_dn_demodulate(color[3 * p], color[3 * p + 1], color[3 * p + 2], variance[p], a);
    gd[p] = trt_dn4{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]};
    a.w = trt_dn_depth_gradient(trt_dn_depth{depth, width}, x, y, width, height);
    aux[p] = a;
}

// A (DN_BX + 2 AP) x (DN_BY + 2 AP) tile of cv and gd in LDS whose element (0, 0) is image pixel (ox, oy).  Only in-image pixels are
// staged; the tap loop never asks for any other.
struct DnFetchLds {
    const trt_dn4* cvt;
    const trt_dn4* gdt;
    int ox, oy, pitch;
    __device__ trt_dn4 cv(int x, int y) const { return cvt[(y - oy) * pitch + (x - ox)]; }
    __device__ trt_dn4 gd(int x, int y) const { return gdt[(y - oy) * pitch + (x - ox)]; }
    __device__ float var(int x, int y) const { return cvt[(y - oy) * pitch + (x - ox)].w; }
};

// LDS_STEP = 1 or 2: the level's step (staged in LDS); 0: any step, taps from global memory.  LAST: write out = c * a (RGB) instead of cv_out.
template <int LDS_STEP, bool LAST>
__global__ __launch_bounds__(DN_BX * DN_BY) void k_denoise_level(trt_dn_args a, const trt_dn4* __restrict__ cv_in, const trt_dn4* __restrict__ gd,
                                                                 const trt_dn4* __restrict__ aux, trt_dn4* __restrict__ cv_out, float* __restrict__ out)
{
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    trt_dn4 r;
    if constexpr (LDS_STEP > 0) {
        constexpr int AP = 2 * LDS_STEP, TW = DN_BX + 2 * AP, TH = DN_BY + 2 * AP;
        __shared__ trt_dn4 s_cv[TW * TH];
        __shared__ trt_dn4 s_gd[TW * TH];
        const int ox = (int)(blockIdx.x * DN_BX) - AP, oy = (int)(blockIdx.y * DN_BY) - AP;
        for (int k = (int)(threadIdx.y * DN_BX + threadIdx.x); k < TW * TH; k += DN_BX * DN_BY) {
            const int tx = k % TW, ty = k / TW, gx = ox + tx, gy = oy + ty;
            if (trt_dn_inside(gx, gy, a.width, a.height)) {
                const size_t q = (size_t)gy * (size_t)a.width + (size_t)gx;
                s_cv[k] = cv_in[q];
                s_gd[k] = gd[q];
            }
        }
        __syncthreads();
        if (x >= a.width || y >= a.height) return;
        r = trt_dn_level(DnFetchLds{s_cv, s_gd, ox, oy, TW}, x, y, aux[p].w, a);
    } else {
        if (x >= a.width || y >= a.height) return;
        r = trt_dn_level(trt_dn_fetch{cv_in, gd, a.width}, x, y, aux[p].w, a);
    }
    if constexpr (LAST) {
        float o[3];
        trt_dn_remodulate(r, aux[p], o);
        out[3 * p] = o[0];
        out[3 * p + 1] = o[1];
        out[3 * p + 2] = o[2];
    } else {
        cv_out[p] = r;
    }
}

}  // namespace trtd

#endif  // TRT_DENOISE_KERNELS_H
