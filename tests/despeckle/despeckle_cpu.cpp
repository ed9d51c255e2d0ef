// CPU build of the per-pixel code of trt_despeckle (tinyraytracing_amd/csrc/trt_despeckle.h: trt_ds_check, trt_ds_pixel over trt_ds_frame)
// for the tests: the kernel's loop, pixel by pixel, with g++ -ffp-contract=off.  Same bits as the GPU (tests/test_gpu_despeckle.py).
#include "trt_despeckle.h"

namespace {

template <int R>
void run(const trt_ds_args& a, const float* color, const float* variance, const float* albedo, const float* depth, float* out_color,
         float* out_variance, float* out_scale)
{
    const trt_ds_frame frame{color, albedo, depth, a.width, a.height};
#pragma omp parallel for schedule(static)
    for (int y = 0; y < a.height; ++y)
        for (int x = 0; x < a.width; ++x) {
            const size_t p = (size_t)y * a.width + x;
            const trt_ds_pixel_out o = trt_ds_pixel<R>(a, frame, x, y, color + 3 * p, albedo + 3 * p, depth[p], variance ? variance[p] : 0.0f);
            out_color[3 * p] = o.color[0];
            out_color[3 * p + 1] = o.color[1];
            out_color[3 * p + 2] = o.color[2];
            if (out_variance) out_variance[p] = o.variance;
            if (out_scale) out_scale[p] = o.scale;
        }
}

}  // namespace

extern "C" {

// Arguments as for trt_despeckle; returns 0, or 1 for arguments it refuses with TRT_EINVAL.
int despeckle_cpu(const trt_despeckle_params* prm, int width, int height, const float* color, const float* variance, const float* albedo,
                  const float* depth, float* out_color, float* out_variance, float* out_scale)
{
    trt_ds_args a{};
    if (trt_ds_check(prm, width, height, color && albedo && depth && out_color, (variance != nullptr) == (out_variance != nullptr), a)) return 1;
    if (a.radius == 1)
        run<1>(a, color, variance, albedo, depth, out_color, out_variance, out_scale);
    else
        run<2>(a, color, variance, albedo, depth, out_color, out_variance, out_scale);
    return 0;
}

// The resolved parameters: out = (radius, sigma); 0, or 1 for parameters that are refused.
int despeckle_cpu_defaults(const trt_despeckle_params* prm, float* out2)
{
    trt_ds_args a{};
    if (trt_ds_check(prm, 1, 1, true, true, a)) return 1;
    out2[0] = (float)a.radius;
    out2[1] = a.sigma;
    return 0;
}

}  // extern "C"
