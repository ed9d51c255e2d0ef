// A stand-alone driver for the host sanitizers (tests/test_moments_cpu.py builds it together with moments_cpu.cpp under
// -fsanitize=address,undefined and runs it): hostile depths, cameras, points and mom records through both stages of the CPU build of
// trt_reproject_moments' per-pixel code, at 1 x 1, 5 x 7 and 33 x 17.  Every buffer is a heap allocation of exactly the size the contract
// names, so an index outside the image is an AddressSanitizer report.  Prints "ok <cases>" and returns 0 when every case was accepted and
// no pixel that must be without history found one.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "trt.h"

extern "C" int reproject_moments_cpu(const trt_moments_params* prm, int width, int height, const float* color, const float* albedo, const float* normal,
                                     const float* depth, const float* prev_point, const float* prev_cv, const float* prev_len, const float* prev_normal,
                                     const float* prev_depth, const float* prev_mom, float* out_color, float* out_variance, float* out_cv, float* out_len,
                                     float* out_mom);

namespace {

trt_camera camera(int W, int H, float ex, float ey, float ez)
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
    int W, H;
    std::vector<float> color, albedo, normal, depth, point, cv, len, mom, out_color, out_variance, out_cv, out_len, out_mom;
    Frame(int w, int h)
        : W(w), H(h), color(w * h * 3, 0.5f), albedo(w * h * 3, 0.7f), normal(w * h * 3, 0.0f), depth(w * h, 5.0f), point(w * h * 3, 0.0f),
          cv(w * h * 4, 0.25f), len(w * h, 6.0f), mom(w * h * 4, 0.0f), out_color(w * h * 3), out_variance(w * h), out_cv(w * h * 4), out_len(w * h),
          out_mom(w * h * 4)
    {
        for (int p = 0; p < w * h; ++p) {
            normal[3 * p + 2] = 1.0f;
            point[3 * p + 2] = -5.0f;
            mom[4 * p] = 0.7f;
            mom[4 * p + 1] = 0.55f;
            mom[4 * p + 2] = 0.25f;
        }
    }
};

// Runs one call; `prev_depth` / `prev_normal` are the history's feature buffers.  -> the number of pixels with out_len > 1, or -1.
int run(const trt_moments_params& prm, Frame& f, const std::vector<float>& prev_normal, const std::vector<float>& prev_depth, bool motion)
{
    if (reproject_moments_cpu(&prm, f.W, f.H, f.color.data(), f.albedo.data(), f.normal.data(), f.depth.data(), motion ? f.point.data() : nullptr,
                              f.cv.data(), f.len.data(), prev_normal.data(), prev_depth.data(), f.mom.data(), f.out_color.data(), f.out_variance.data(),
                              f.out_cv.data(), f.out_len.data(), f.out_mom.data()) != 0)
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
    const int sizes[3][2] = {{1, 1}, {5, 7}, {33, 17}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        const Frame clean(W, H);
        for (unsigned flags : {0u, (unsigned)TRT_FLAG_FIXED_PIXELS})
            for (bool motion : {false, true}) {
                trt_moments_params prm{};
                prm.rp.flags = flags;
                prm.rp.cur = camera(W, H, 0.1f, 0.0f, 0.0f);
                prm.rp.prev = camera(W, H, 0.0f, 0.05f, 0.0f);
                {  // the plain case finds history (on the reference's grid a 1 x 1 image divides by W - 1 = 0 and finds none)
                    Frame f(W, H);
                    const int n = run(prm, f, clean.normal, clean.depth, motion);
                    bad += (W > 1 || motion) ? n < W * H / 2 : n < 0;
                    ++cases;
                }
                // a first frame: every pixel through stage B
                {
                    Frame f(W, H);
                    bad += reproject_moments_cpu(&prm, W, H, f.color.data(), f.albedo.data(), f.normal.data(), f.depth.data(), nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, f.out_color.data(), f.out_variance.data(), f.out_cv.data(), f.out_len.data(),
                                                 f.out_mom.data()) != 0;
                    ++cases;
                }
                // hostile depths of the current frame, each in every pixel and in every other pixel: no history where they are, both stages run
                for (float z : {nan, inf, -inf, -5.0f, 0.0f, 3.0e38f, 1.0e-42f, 114513.99f})
                    for (int stride : {1, 2}) {
                        Frame f(W, H);
                        for (int p = 0; p < W * H; p += stride) f.depth[p] = z;
                        const int n = run(prm, f, clean.normal, clean.depth, false);
                        bad += stride == 1 ? n != 0 : n < 0;
                        ++cases;
                    }
                // hostile depths in the history: never used
                for (float z : {nan, inf, -inf, 114514.0f}) {
                    Frame f(W, H);
                    std::vector<float> pd(W * H, z);
                    bad += run(prm, f, clean.normal, pd, motion) != 0;
                    ++cases;
                }
                // hostile points: no history, or at least no fault
                for (float v : {nan, inf, -inf, 3.0e38f, -3.0e38f, 1.0e19f, 0.0f})
                    for (int k = 0; k < 3; ++k) {
                        Frame f(W, H);
                        for (int p = 0; p < W * H; ++p) f.point[3 * p + k] = v;
                        bad += run(prm, f, clean.normal, clean.depth, true) < 0;
                        ++cases;
                    }
                // hostile moments records, each in every pixel and in every third: they flow into the results and index nothing
                for (float v : {nan, inf, -inf, -3.0f, 0.0f, 1.0f, 1.5f, 3.0e38f})
                    for (int k = 0; k < 3; ++k)
                        for (int stride : {1, 3}) {
                            Frame f(W, H);
                            for (int p = 0; p < W * H; p += stride) f.mom[4 * p + k] = v;
                            bad += run(prm, f, clean.normal, clean.depth, motion) < 0;
                            ++cases;
                        }
                // hostile history lengths and colours
                for (float v : {nan, inf, -inf, -3.0f, 0.0f, 3.0e38f}) {
                    Frame f(W, H);
                    for (float& l : f.len) l = v;
                    bad += run(prm, f, clean.normal, clean.depth, motion) < 0;
                    Frame g(W, H);
                    for (float& c : g.color) c = v;
                    bad += run(prm, g, clean.normal, clean.depth, motion) < 0;
                    cases += 2;
                }
                // a degenerate previous camera (zero horizontal): the determinant is 0
                {
                    trt_moments_params q = prm;
                    q.rp.prev.horizontal[0] = 0.0f;
                    Frame f(W, H);
                    bad += run(q, f, clean.normal, clean.depth, motion) != 0;
                    ++cases;
                }
                // cameras that are not numbers, component by component, and far away
                for (int k = 0; k < 12; ++k)
                    for (float v : {nan, inf, -inf, 3.0e38f, -3.0e38f}) {
                        trt_moments_params q = prm;
                        q.rp.prev = poke(prm.rp.prev, k, v);
                        Frame f(W, H);
                        bad += run(q, f, clean.normal, clean.depth, motion) < 0;
                        q = prm;
                        q.rp.cur = poke(prm.rp.cur, k, v);
                        bad += run(q, f, clean.normal, clean.depth, motion) < 0;
                        cases += 2;
                    }
            }
    }
    std::printf("%s %d\n", bad ? "FAILED" : "ok", cases);
    return bad ? 1 : 0;
}
