// trt_reproject_kernels.h — trt_reproject / trt_reproject_device (include/trt.h) for gfx950.  The arithmetic is trt_reproject.h's; this
// file only says which thread takes which pixel.
//
//   k_reproject          one launch per call, one pixel per thread, 16 x 16 blocks (4 waves of 16 x 4, as the a-trous kernels)
//   k_reproject_motion   trt_reproject_motion*: the same with the pixel's previous world point streamed in (12 more bytes per pixel)
//
// Per pixel the kernel streams 44 bytes of the current frame in and 36 bytes out, and gathers up to four history taps of 36 bytes (depth,
// then normal, then the 16-B cv record as one vector load, then the length).  Neighbouring pixels land on neighbouring taps, so the
// gather is served by L2 and each history byte leaves HBM about once: no LDS tile could do better, and none is used.
#ifndef TRT_REPROJECT_KERNELS_H
#define TRT_REPROJECT_KERNELS_H

#include <hip/hip_runtime.h>

#include "trt_reproject.h"

namespace trtd {

constexpr int RP_BX = 16, RP_BY = 16;

__global__ __launch_bounds__(RP_BX * RP_BY) void k_reproject(trt_rp_args a, const float* __restrict__ color, const float* __restrict__ variance,
                                                             const float* __restrict__ albedo, const float* __restrict__ normal,
                                                             const float* __restrict__ depth, trt_rp_fetch hist, float* __restrict__ out_color,
                                                             float* __restrict__ out_variance, trt_dn4* __restrict__ out_cv, float* __restrict__ out_len)
{
    const int x = (int)(blockIdx.x * RP_BX + threadIdx.x), y = (int)(blockIdx.y * RP_BY + threadIdx.y);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float c[3] = {color[3 * p], color[3 * p + 1], color[3 * p + 2]};
    const float al[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
    const float n[3] = {normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]};
    const trt_rp_pixel_out o = trt_rp_pixel(a, hist, x, y, c, variance[p], al, n, depth[p]);
    out_color[3 * p] = o.color[0];
    out_color[3 * p + 1] = o.color[1];
    out_color[3 * p + 2] = o.color[2];
    out_variance[p] = o.variance;
    out_cv[p] = o.cv;
    out_len[p] = o.len;
}

// A kernel of its own, not a template of k_reproject: that kernel's code stays what it was.
__global__ __launch_bounds__(RP_BX * RP_BY) void k_reproject_motion(trt_rp_args a, const float* __restrict__ color, const float* __restrict__ variance,
                                                                    const float* __restrict__ albedo, const float* __restrict__ normal,
                                                                    const float* __restrict__ depth, const float* __restrict__ prev_point,
                                                                    trt_rp_fetch hist, float* __restrict__ out_color, float* __restrict__ out_variance,
                                                                    trt_dn4* __restrict__ out_cv, float* __restrict__ out_len)
{
    const int x = (int)(blockIdx.x * RP_BX + threadIdx.x), y = (int)(blockIdx.y * RP_BY + threadIdx.y);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float c[3] = {color[3 * p], color[3 * p + 1], color[3 * p + 2]};
    const float al[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
    const float n[3] = {normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]};
    const float pp[3] = {prev_point[3 * p], prev_point[3 * p + 1], prev_point[3 * p + 2]};
    const trt_rp_pixel_out o = trt_rp_pixel_motion(a, hist, c, variance[p], al, n, depth[p], pp);
    out_color[3 * p] = o.color[0];
    out_color[3 * p + 1] = o.color[1];
    out_color[3 * p + 2] = o.color[2];
    out_variance[p] = o.variance;
    out_cv[p] = o.cv;
    out_len[p] = o.len;
}

}  // namespace trtd

#endif  // TRT_REPROJECT_KERNELS_H
