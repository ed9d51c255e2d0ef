// CPU build of the per-element code of trt_reproject_motion (tinyraytracing_amd/csrc/trt_reproject.h: trt_rp_project_point,
// trt_rp_pixel_motion) and of trt_trace_points (csrc/trt_path.h: hitPoint) for the tests: the kernels' loops, element by element, with
// g++ -ffp-contract=off.  Same bits as the GPU (tests/test_gpu_motion.py).
#include <cstring>

#include "trt_path.h"
#include "trt_reproject.h"

extern "C" {

// Arguments as for trt_reproject_motion; returns 0, or 1 for arguments it refuses with TRT_EINVAL.
int reproject_motion_cpu(const trt_reproject_params* prm, int width, int height, const float* color, const float* variance, const float* albedo,
                         const float* normal, const float* depth, const float* prev_point, const float* prev_cv, const float* prev_len,
                         const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance, float* out_cv, float* out_len)
{
    const bool required = color && variance && albedo && normal && depth && prev_point && out_color && out_variance && out_cv && out_len;
    const int given = (prev_cv ? 1 : 0) + (prev_len ? 1 : 0) + (prev_normal ? 1 : 0) + (prev_depth ? 1 : 0);
    trt_rp_args a{};
    if (trt_rp_check(prm, width, height, required, given, a)) return 1;
    // cv records need not be 16-byte aligned here: they are copied in and out
    struct Fetch {
        const float *cvb, *lenb, *normalb, *depthb;
        trt_dn4 cv(size_t q) const { return trt_dn4{cvb[4 * q], cvb[4 * q + 1], cvb[4 * q + 2], cvb[4 * q + 3]}; }
        float len(size_t q) const { return lenb[q]; }
        float depth(size_t q) const { return depthb[q]; }
        void normal(size_t q, float* n) const { std::memcpy(n, normalb + 3 * q, 3 * sizeof(float)); }
    };
    const Fetch hist{prev_cv, prev_len, prev_normal, prev_depth};
#pragma omp parallel for schedule(static)
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            const trt_rp_pixel_out o =
                trt_rp_pixel_motion(a, hist, color + 3 * p, variance[p], albedo + 3 * p, normal + 3 * p, depth[p], prev_point + 3 * p);
            std::memcpy(out_color + 3 * p, o.color, 3 * sizeof(float));
            out_variance[p] = o.variance;
            out_cv[4 * p] = o.cv.x;
            out_cv[4 * p + 1] = o.cv.y;
            out_cv[4 * p + 2] = o.cv.z;
            out_cv[4 * p + 3] = o.cv.w;
            out_len[p] = o.len;
        }
    return 0;
}

// Steps 3' and 4' for one point: out = (fx, fy, z'); 1 = projected, 0 = no place in the previous image, -1 = parameters refused.
int motion_cpu_project_point(const trt_reproject_params* prm, int width, int height, const float* point3, float* out3)
{
    trt_rp_args a{};
    if (!prm || trt_rp_resolve(*prm, a)) return -1;
    a.width = width;
    a.height = height;
    return trt_rp_project_point(a, point3, out3[0], out3[1], out3[2]) ? 1 : 0;
}

// k_hit_points' arithmetic on given hits: tri[n] (-1 = a miss), uv[n][2] -> point[n][3] on the coordinates tri_v_other[.][3][3].
void motion_cpu_hit_points(const float* tri_v_other, uint32_t n, const int32_t* tri, const float* uv, float* point)
{
    for (uint32_t i = 0; i < n; ++i) {
        trtd::f3 p = trtd::mk3(trtd::u2f(TRT_POINT_MISS_BITS), trtd::u2f(TRT_POINT_MISS_BITS), trtd::u2f(TRT_POINT_MISS_BITS));
        if (tri[i] >= 0) p = trtd::hitPoint(tri_v_other + (size_t)tri[i] * 9, uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
        std::memcpy(point + 3 * (size_t)i, &p, 3 * sizeof(float));
    }
}

}  // extern "C"
