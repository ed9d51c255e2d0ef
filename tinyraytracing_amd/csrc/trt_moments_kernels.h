// trt_moments_kernels.h — trt_reproject_moments / trt_reproject_moments_device (include/trt.h) for gfx950.  The arithmetic is
// trt_moments.h's; this file only says which thread takes which pixel and where the pixels come from.
//
//   k_reproject_moments<MOTION>  stage A: k_reproject's shape — one pixel per thread, 16 x 16 blocks (4 waves of 16 x 4), the history's cv
//                                and mom records as 16-byte vector loads, no LDS.  32 bytes of the current frame in and 52 out per pixel
//                                (12 more in with MOTION), up to four taps of 52 bytes gathered through L2.
//   k_moments_variance<LDS>      stage B: a launch of its own, because a pixel reads its neighbours' out_mom.  A block none of whose pixels
//                                needs the spatial estimate returns after one vote: in steady state that is nearly every block, and the
//                                launch costs a read of 12 bytes per pixel (depth, length, s).  A block that stays stages its tile plus a
//                                3-pixel apron in LDS, (m1, m2, s) as three planes and (n, z) as 16-byte records: 22 x 22 x 28 B = 13.2 KiB;
//                                the 49 taps and the depth gradient then read LDS.  LDS = false reads the taps from global memory (the A/B
//                                arm of TRT_MOMENTS_LDS=0; same bits).
#ifndef TRT_MOMENTS_KERNELS_H
#define TRT_MOMENTS_KERNELS_H

#include <hip/hip_runtime.h>

#include "trt_moments.h"

namespace trtd {

constexpr int MV_BX = 16, MV_BY = 16;

template <bool MOTION>
__global__ __launch_bounds__(MV_BX * MV_BY) void k_reproject_moments(trt_mv_args a, const float* __restrict__ color, const float* __restrict__ albedo,
                                                                     const float* __restrict__ normal, const float* __restrict__ depth,
                                                                     const float* __restrict__ prev_point, trt_mv_fetch hist,
                                                                     float* __restrict__ out_color, float* __restrict__ out_variance,
                                                                     trt_dn4* __restrict__ out_cv, float* __restrict__ out_len, trt_dn4* __restrict__ out_mom)
{
    const int x = (int)(blockIdx.x * MV_BX + threadIdx.x), y = (int)(blockIdx.y * MV_BY + threadIdx.y);
    if (x >= a.rp.width || y >= a.rp.height) return;
    const size_t p = (size_t)y * (size_t)a.rp.width + (size_t)x;
    const float c[3] = {color[3 * p], color[3 * p + 1], color[3 * p + 2]};
    const float al[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
    const float n[3] = {normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]};
    float pp[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (MOTION) {
        pp[0] = prev_point[3 * p];
        pp[1] = prev_point[3 * p + 1];
        pp[2] = prev_point[3 * p + 2];
    }
    const trt_mv_pixel_out o = trt_mv_pixel<MOTION>(a, hist, x, y, c, al, n, depth[p], pp);
    out_color[3 * p] = o.color[0];
    out_color[3 * p + 1] = o.color[1];
    out_color[3 * p + 2] = o.color[2];
    out_variance[p] = o.variance;
    out_cv[p] = o.cv;
    out_len[p] = o.len;
    out_mom[p] = o.mom;
}

constexpr int MV_AP = TRT_MV_RADIUS, MV_TW = MV_BX + 2 * MV_AP, MV_TH = MV_BY + 2 * MV_AP;

// The block's tile in LDS; element (0, 0) is image pixel (ox, oy).  Only in-image pixels are staged, and trt_mv_spatial asks for no other.
struct MvFetchLds {
    const float* m1;
    const float* m2;
    const float* s;
    const trt_dn4* gdt;
    int ox, oy;
    __device__ int at(int x, int y) const { return (y - oy) * MV_TW + (x - ox); }
    __device__ trt_dn4 mom(int x, int y) const
    {
        const int k = at(x, y);
        return trt_dn4{m1[k], m2[k], s[k], 0.0f};
    }
    __device__ trt_dn4 gd(int x, int y) const { return gdt[at(x, y)]; }
    __device__ float operator()(int x, int y) const { return gdt[at(x, y)].w; }
};

// normal, depth, out_len and out_mom are read; out_cv's fourth float and out_variance are written, at this thread's own pixel only.
template <bool LDS>
__global__ __launch_bounds__(MV_BX * MV_BY) void k_moments_variance(trt_mv_args a, const float* __restrict__ albedo, const float* __restrict__ normal,
                                                                    const float* __restrict__ depth, const float* __restrict__ out_len,
                                                                    const trt_dn4* __restrict__ out_mom, float* out_cv, float* __restrict__ out_variance)
{
    const int x = (int)(blockIdx.x * MV_BX + threadIdx.x), y = (int)(blockIdx.y * MV_BY + threadIdx.y);
    const bool inside = x < a.rp.width && y < a.rp.height;
    const size_t p = (size_t)y * (size_t)a.rp.width + (size_t)x;
    bool need = false;
    if (inside) {
        const float z = depth[p];
        need = trt_dn_hit(z) && !trt_mv_temporal(a, z, out_len[p], out_mom[p].z);
    }
    float var;
    if constexpr (LDS) {
        if (!__syncthreads_or(need ? 1 : 0)) return;
        __shared__ float s_m1[MV_TW * MV_TH];
        __shared__ float s_m2[MV_TW * MV_TH];
        __shared__ float s_s[MV_TW * MV_TH];
        __shared__ trt_dn4 s_gd[MV_TW * MV_TH];
        const int ox = (int)(blockIdx.x * MV_BX) - MV_AP, oy = (int)(blockIdx.y * MV_BY) - MV_AP;
        for (int k = (int)(threadIdx.y * MV_BX + threadIdx.x); k < MV_TW * MV_TH; k += MV_BX * MV_BY) {
            const int tx = k % MV_TW, ty = k / MV_TW, gx = ox + tx, gy = oy + ty;
            if (trt_dn_inside(gx, gy, a.rp.width, a.rp.height)) {
                const size_t q = (size_t)gy * (size_t)a.rp.width + (size_t)gx;
                const trt_dn4 m = out_mom[q];
                s_m1[k] = m.x;
                s_m2[k] = m.y;
                s_s[k] = m.z;
                s_gd[k] = trt_dn4{normal[3 * q], normal[3 * q + 1], normal[3 * q + 2], depth[q]};
            }
        }
        __syncthreads();
        if (!need) return;
        var = trt_mv_spatial(a, MvFetchLds{s_m1, s_m2, s_s, s_gd, ox, oy}, x, y);
    } else {
        if (!need) return;
        var = trt_mv_spatial(a, trt_mv_frame{out_mom, normal, depth, a.rp.width}, x, y);
    }
    const float al[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
    out_cv[4 * p + 3] = var;
    out_variance[p] = trt_mv_remodulate_variance(var, al);
}

}  // namespace trtd

#endif  // TRT_MOMENTS_KERNELS_H
