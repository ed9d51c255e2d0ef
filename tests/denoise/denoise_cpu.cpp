// CPU build of the a-trous filter (tinyraytracing_amd/csrc/trt_denoise.h) for the tests: the buffers and passes of trt_denoise's kernels,
// pixel by pixel, with g++ -ffp-contract=off.  Same bits as the GPU (tests/test_gpu_denoise.py).
#include <cstring>
#include <vector>

#include "trt_denoise.h"

extern "C" {

// params as for trt_denoise (NULL = defaults); returns 0, or 1 for arguments trt_denoise refuses with TRT_EINVAL.
int denoise_cpu(const trt_denoise_params* prm, int width, int height, const float* color, const float* variance, const float* albedo,
                const float* normal, const float* depth, float* out)
{
    if (!color || !variance || !albedo || !normal || !depth || !out || width < 1 || height < 1) return 1;
    if ((unsigned long long)width * (unsigned long long)height > TRT_DENOISE_MAX_PIXELS) return 1;
    trt_denoise_params d{};
    if (prm) d = *prm;
    if (d.iterations < 0 || d.iterations > TRT_DENOISE_MAX_ITERATIONS || d.sigma_normal < 0 || d.sigma_normal > 256 || !(d.sigma_depth >= 0.0f) ||
        !(d.sigma_luminance >= 0.0f) || d.flags != 0)
        return 1;
    trt_dn_args a{};
    a.width = width;
    a.height = height;
    a.sigma_normal = d.sigma_normal ? d.sigma_normal : TRT_DN_SIGMA_NORMAL;
    a.sigma_depth = d.sigma_depth != 0.0f ? d.sigma_depth : TRT_DN_SIGMA_DEPTH;
    a.sigma_luminance = d.sigma_luminance != 0.0f ? d.sigma_luminance : TRT_DN_SIGMA_LUMINANCE;
    const int levels = d.iterations ? d.iterations : TRT_DN_ITERATIONS;
    const size_t n = (size_t)width * (size_t)height;
    std::vector<trt_dn4> cv0(n), cv1(n), gd(n), aux(n);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            trt_dn4 f = trt_dn_factor(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]);
            cv0[p] = trt_dn_demodulate(color[3 * p], color[3 * p + 1], color[3 * p + 2], variance[p], f);
            gd[p] = trt_dn4{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]};
            f.w = trt_dn_depth_gradient(trt_dn_depth{depth, width}, x, y, width, height);
            aux[p] = f;
        }
    trt_dn4* cv[2] = {cv0.data(), cv1.data()};
    for (int k = 0; k < levels; ++k) {
        a.step = 1 << k;
        const trt_dn_fetch f{cv[k & 1], gd.data(), width};
        trt_dn4* nxt = cv[(k + 1) & 1];
        const bool last = k + 1 == levels;
#pragma omp parallel for schedule(static)
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) {
                const size_t p = (size_t)y * width + x;
                const trt_dn4 r = trt_dn_level(f, x, y, aux[p].w, a);
                if (last) trt_dn_remodulate(r, aux[p], out + 3 * p);
                else nxt[p] = r;
            }
    }
    return 0;
}

// The building blocks on their own, for the restatement's unit checks.
float denoise_cpu_expf_neg(float x) { return trt_expf_neg(x); }
float denoise_cpu_radius(int d2) { return trt_dn_radius(d2); }
float denoise_cpu_powi(float b, int e) { return trt_dn_powi(b, e); }

}  // extern "C"
