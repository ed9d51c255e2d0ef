// A stand-alone driver for the host sanitizers (tests/test_despeckle_cpu.py builds it together with despeckle_cpu.cpp under
// -fsanitize=address,undefined and runs it): NaN, infinite and negative colours, zero and negative albedos and NaN depths through the CPU
// build of trt_despeckle's per-pixel code, at 1 x 1, 1 x 40 and 17 x 3, R = 1 and 2, with and without the optional buffers.  Every buffer
// is a heap allocation of exactly the size the contract names, so an index outside the image is an AddressSanitizer report.  Prints
// "ok <cases>" and returns 0 when every case was accepted, the inputs came back unmodified, and every pixel that must pass through (a miss,
// a NaN depth) carries the input's bits and scale 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "trt.h"

extern "C" int despeckle_cpu(const trt_despeckle_params* prm, int width, int height, const float* color, const float* variance, const float* albedo,
                             const float* depth, float* out_color, float* out_variance, float* out_scale);

namespace {

struct Frame {
    int W, H;
    std::vector<float> color, variance, albedo, depth;
    Frame(int w, int h) : W(w), H(h), color(w * h * 3, 0.5f), variance(w * h, 0.01f), albedo(w * h * 3, 0.7f), depth(w * h, 5.0f)
    {
        for (int p = 0; p < w * h; ++p) color[3 * p + 1] = 0.25f + 0.01f * (float)(p % 7);
    }
};

// Runs one call in every combination of radius and optional buffers.  -> the number of failed expectations.
int run(const Frame& f, float sigma)
{
    int bad = 0;
    const int n = f.W * f.H;
    for (int radius : {0, 1, 2})
        for (int opt = 0; opt < 4; ++opt) {
            const bool var = opt & 1, scale = opt & 2;
            const Frame keep = f;
            std::vector<float> out_color(n * 3, -1.0f), out_variance(var ? n : 0, -1.0f), out_scale(scale ? n : 0, -1.0f);
            trt_despeckle_params prm{};
            prm.radius = radius;
            prm.sigma = sigma;
            if (despeckle_cpu(&prm, f.W, f.H, f.color.data(), var ? f.variance.data() : nullptr, f.albedo.data(), f.depth.data(), out_color.data(),
                              var ? out_variance.data() : nullptr, scale ? out_scale.data() : nullptr) != 0) {
                ++bad;
                continue;
            }
            bad += std::memcmp(keep.color.data(), f.color.data(), n * 3 * sizeof(float)) != 0;
            bad += std::memcmp(keep.albedo.data(), f.albedo.data(), n * 3 * sizeof(float)) != 0;
            bad += std::memcmp(keep.depth.data(), f.depth.data(), n * sizeof(float)) != 0;
            bad += std::memcmp(keep.variance.data(), f.variance.data(), n * sizeof(float)) != 0;
            for (int p = 0; p < n; ++p) {
                if (f.depth[p] < TRT_INF) continue;  // false for a miss and for a NaN
                bad += std::memcmp(&out_color[3 * p], &f.color[3 * p], 3 * sizeof(float)) != 0;
                if (var) bad += std::memcmp(&out_variance[p], &f.variance[p], sizeof(float)) != 0;
                if (scale) bad += out_scale[p] != 1.0f;
            }
            if (scale)
                for (int p = 0; p < n; ++p) bad += std::isnan(out_scale[p]);  // 1, 0 or T / l_p with l_p finite and above T: never a NaN
        }
    return bad;
}

}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    int cases = 0, bad = 0;
    const int sizes[3][2] = {{1, 1}, {1, 40}, {17, 3}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1], n = W * H;
        for (float sigma : {0.0f, 3.0f, 0.5f}) {
            bad += run(Frame(W, H), sigma);
            ++cases;
            // hostile colours, each in every pixel, in every other pixel and in one channel of every third
            for (float v : {nan, inf, -inf, -3.0f, 0.0f, 3.0e38f, -3.0e38f, 1.0e-42f})
                for (int mode = 0; mode < 3; ++mode) {
                    Frame f(W, H);
                    for (int p = 0; p < n; p += mode + 1)
                        for (int k = 0; k < (mode == 2 ? 1 : 3); ++k) f.color[3 * p + k] = v;
                    bad += run(f, sigma);
                    ++cases;
                }
            // zero, negative and non-finite albedos (a channel that is not positive demodulates by 1)
            for (float v : {0.0f, -0.5f, nan, inf, -inf, 1.0e-42f, 3.0e38f})
                for (int stride : {1, 2}) {
                    Frame f(W, H);
                    for (int p = 0; p < n; p += stride) f.albedo[3 * p + p % 3] = v;
                    bad += run(f, sigma);
                    ++cases;
                }
            // hostile depths: NaN and the misses pass through, a negative depth is a hit
            for (float z : {nan, inf, -inf, -5.0f, 0.0f, 114514.0f, 114513.99f})
                for (int stride : {1, 2, 3}) {
                    Frame f(W, H);
                    for (int p = 0; p < n; p += stride) f.depth[p] = z;
                    bad += run(f, sigma);
                    ++cases;
                }
            // hostile variances
            for (float v : {nan, inf, -1.0f}) {
                Frame f(W, H);
                for (int p = 0; p < n; p += 2) f.variance[p] = v;
                for (int p = 1; p < n; p += 4) f.color[3 * p] = nan;  // replaced pixels beside them
                bad += run(f, sigma);
                ++cases;
            }
        }
    }
    std::printf("%s %d\n", bad ? "FAILED" : "ok", cases);
    return bad ? 1 : 0;
}
