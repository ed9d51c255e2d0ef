// A stand-alone driver for the host sanitizers (tests/test_reproject_cpu.py builds it together with reproject_cpu.cpp under
// -fsanitize=address,undefined and runs it): hostile depths and cameras through the CPU build of trt_reproject's per-pixel code.  Every
// buffer is a heap allocation of exactly the size the contract names, so an index outside the image is an AddressSanitizer report.
// Prints "ok <cases>" and returns 0 when every case finished and no pixel that must be without history found one.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "trt.h"

extern "C" int reproject_cpu(const trt_reproject_params* prm, int width, int height, const float* color, const float* variance, const float* albedo,
                             const float* normal, const float* depth, const float* prev_cv, const float* prev_len, const float* prev_normal,
                             const float* prev_depth, float* out_color, float* out_variance, float* out_cv, float* out_len);

namespace {

const int W = 19, H = 11;

trt_camera camera(float ex, float ey, float ez)
{
    // looks down -z from (ex, ey, ez): a viewport of 2 x 2 * H / W at distance 1
    const float vh = 2.0f * H / W;
    trt_camera c{};
    const float eye[3] = {ex, ey, ez}, llc[3] = {ex - 1.0f, ey - vh / 2, ez - 1.0f}, hor[3] = {2.0f, 0.0f, 0.0f}, ver[3] = {0.0f, vh, 0.0f};
    std::memcpy(c.eye, eye, sizeof eye);
    std::memcpy(c.lower_left_corner, llc, sizeof llc);
    std::memcpy(c.horizontal, hor, sizeof hor);
    std::memcpy(c.vertical, ver, sizeof ver);
    return c;
}

// `c` with its k-th float (eye, lower_left_corner, horizontal, vertical: 12 in all) replaced by v
trt_camera poke(const trt_camera& c, int k, float v)
{
    float a[12];
    static_assert(sizeof a == sizeof(trt_camera), "trt_camera is 12 floats");
    std::memcpy(a, &c, sizeof a);
    a[k] = v;
    trt_camera r;
    std::memcpy(&r, a, sizeof a);
    return r;
}

struct Frame {
    std::vector<float> color, variance, albedo, normal, depth, cv, len, out_color, out_variance, out_cv, out_len;
    Frame()
        : color(W * H * 3, 0.5f), variance(W * H, 1e-3f), albedo(W * H * 3, 0.7f), normal(W * H * 3, 0.0f), depth(W * H, 5.0f), cv(W * H * 4, 0.25f),
          len(W * H, 3.0f), out_color(W * H * 3), out_variance(W * H), out_cv(W * H * 4), out_len(W * H)
    {
        for (int p = 0; p < W * H; ++p) normal[3 * p + 2] = 1.0f;
    }
};

// Runs one call; `prev_depth` / `prev_normal` are the history's feature buffers.  -> the number of pixels with out_len > 1, or -1.
int run(const trt_reproject_params& prm, Frame& f, const std::vector<float>& prev_normal, const std::vector<float>& prev_depth)
{
    if (reproject_cpu(&prm, W, H, f.color.data(), f.variance.data(), f.albedo.data(), f.normal.data(), f.depth.data(), f.cv.data(), f.len.data(),
                      prev_normal.data(), prev_depth.data(), f.out_color.data(), f.out_variance.data(), f.out_cv.data(), f.out_len.data()) != 0)
        return -1;
    int n = 0;
    for (float l : f.out_len) n += l > 1.0f;
    return n;
}

}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    int cases = 0, bad = 0;
    const Frame clean;
    for (unsigned flags : {0u, (unsigned)TRT_FLAG_FIXED_PIXELS}) {
        trt_reproject_params prm{};
        prm.flags = flags;
        prm.cur = camera(0.1f, 0.0f, 0.0f);
        prm.prev = camera(0.0f, 0.05f, 0.0f);
        {  // the plain case finds history nearly everywhere
            Frame f;
            const int n = run(prm, f, clean.normal, clean.depth);
            bad += n < W * H / 2;
            ++cases;
        }
        // hostile depths of the current frame, each in every pixel: none may find history or index outside
        for (float z : {nan, inf, -inf, -5.0f, 0.0f, 3.0e38f, 1.0e-42f, 114513.99f}) {
            Frame f;
            for (float& d : f.depth) d = z;
            const int n = run(prm, f, clean.normal, clean.depth);
            bad += n != 0;
            ++cases;
        }
        // hostile depths in the history: never used
        for (float z : {nan, inf, -inf, 114514.0f}) {
            Frame f;
            std::vector<float> pd(W * H, z);
            const int n = run(prm, f, clean.normal, pd);
            bad += n != 0;
            ++cases;
        }
        // a degenerate previous camera (zero horizontal): the determinant is 0
        {
            trt_reproject_params q = prm;
            q.prev.horizontal[0] = 0.0f;
            Frame f;
            bad += run(q, f, clean.normal, clean.depth) != 0;
            ++cases;
        }
        // every point behind the previous eye
        {
            trt_reproject_params q = prm;
            q.prev = camera(0.0f, 0.0f, -50.0f);
            Frame f;
            bad += run(q, f, clean.normal, clean.depth) != 0;
            ++cases;
        }
        // cameras that are not numbers, component by component, and far away
        for (int k = 0; k < 12; ++k)
            for (float v : {nan, inf, -inf, 3.0e38f, -3.0e38f}) {
                trt_reproject_params q = prm;
                q.prev = poke(prm.prev, k, v);
                Frame f;
                bad += run(q, f, clean.normal, clean.depth) < 0;
                q = prm;
                q.cur = poke(prm.cur, k, v);
                bad += run(q, f, clean.normal, clean.depth) < 0;
                cases += 2;
            }
        // a 1 x 1 image: the reference's grid divides by W - 1 = 0
        {
            std::vector<float> c3(3, 0.5f), v1(1, 1e-3f), a3(3, 0.7f), n3{0.0f, 0.0f, 1.0f}, z1(1, 5.0f), cv4(4, 0.25f), l1(1, 3.0f), oc(3), ov(1), ocv(4), ol(1);
            bad += reproject_cpu(&prm, 1, 1, c3.data(), v1.data(), a3.data(), n3.data(), z1.data(), cv4.data(), l1.data(), n3.data(), z1.data(), oc.data(),
                                 ov.data(), ocv.data(), ol.data()) != 0;
            ++cases;
        }
    }
    std::printf("%s %d\n", bad ? "FAILED" : "ok", cases);
    return bad ? 1 : 0;
}
