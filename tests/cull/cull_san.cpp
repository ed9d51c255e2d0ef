// A stand-alone driver for the host sanitizers (tests/test_cull_cpu.py builds it together with cull_cpu.cpp under
// -fsanitize=address,undefined and runs it): the cull bound (trt_cull.h) over a corpus of cameras — in front of, inside, beside and behind
// the boxes, rolled, turned, degenerate (zero and parallel axes) and hostile (NaN, infinities, 3e38, denormals) — and of boxes (the unit pair,
// empty, inverted, infinite, NaN, huge), at sizes from 1 x 1 to 65536 x 2, `fixed` on and off.  Every active bound must be a set of counts
// inside its image, and its sweep must find no culled ray that passes a box or has a zero component.  Prints "ok <cases>" and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "trt.h"

extern "C" int cull_bound(const trt_camera* cam, int W, int H, int fixed, const float* boxes, uint32_t n_nodes, double margin_pixels, int32_t* out, const char** why);
extern "C" int cull_sweep(const trt_camera* cam, int W, int H, int fixed, const float* boxes, uint32_t n_nodes, double margin_pixels, uint64_t seed, int n_interior,
                          uint64_t* counts);

namespace {

struct V { float x, y, z; };
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V mul(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V unit(V a) { const float l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return mul(a, 1.0f / l); }

trt_camera lookAt(V eye, V target, V up, float fovy_deg, int W, int H)
{
    const float vh = 2.0f * std::tan(fovy_deg * 0.008726646f), vw = vh * (float)W / (float)(H > 0 ? H : 1);
    const V w = unit(sub(eye, target)), u = unit(cross(up, w)), v = cross(w, u);
    const V hor = mul(u, vw), ver = mul(v, vh), llc = sub(sub(sub(eye, mul(hor, 0.5f)), mul(ver, 0.5f)), w);
    trt_camera c;
    const V src[4] = {eye, llc, hor, ver};
    float* dst[4] = {c.eye, c.lower_left_corner, c.horizontal, c.vertical};
    for (int k = 0; k < 4; ++k) { dst[k][0] = src[k].x; dst[k][1] = src[k].y; dst[k][2] = src[k].z; }
    return c;
}

}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[][2] = {{1, 1}, {2, 2}, {2, 25}, {64, 2}, {33, 25}, {97, 41}, {65536, 2}, {3, 65536}};
    std::vector<std::vector<float>> boxes = {
        {-1, -1, -1, 0, 1, 1, 0, -1, -1, 1, 1, 1},
        {-1, -1, -1, 1, 1, 1, nan, nan, nan, nan, nan, nan},
        {1, 1, 1, -1, -1, -1, 0, 0, 0, 0, 0, 0},
        {-inf, -1, -1, 0, 1, 1, 0, -1, -1, inf, 1, 1},
        {-3e38f, -3e38f, -3e38f, 3e38f, 3e38f, 3e38f, 0, 0, 0, 1, 1, 1},
        {0, 0, 0, 0, 0, 0, 1e-42f, 1e-42f, 1e-42f, 2e-42f, 2e-42f, 2e-42f},
        {4e4f, 4e4f, 4e4f, 4.0001e4f, 4.0001e4f, 4.0001e4f, 4e4f, 4e4f, 4e4f, 4.0002e4f, 4.0001e4f, 4.0001e4f},
    };
    int cases = 0, bad = 0;
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        std::vector<trt_camera> cams = {
            lookAt({0, 0, -12}, {0, 0, 0}, {0, 1, 0}, 30, W, H), lookAt({0, 0, -12}, {0, 0, 0}, {1, 0, 0}, 30, W, H),
            lookAt({9, 3, -17}, {0, 0, 0}, {0, 1, 0}, 12, W, H), lookAt({9, 3, -17}, {0, 0, 0}, {0, 1, 0}, 70, W, H),
            lookAt({0.25f, 0.1f, -0.5f}, {0.25f, 0.1f, 5}, {0, 1, 0}, 30, W, H), lookAt({5, 0, -1}, {5, 0, 5}, {0, 1, 0}, 30, W, H),
            lookAt({1, 0, -12}, {1, 0, 0}, {0, 1, 0}, 30, W, H), lookAt({0, 0, -12}, {0, 0, -24}, {0, 1, 0}, 30, W, H),
            lookAt({0, 0, -40}, {-9.5f, 6.5f, 0}, {0, 1, 0}, 30, W, H), lookAt({4e4f, 4e4f, 3e4f}, {4e4f, 4e4f, 4e4f}, {0, 1, 0}, 1, W, H),
        };
        {   // degenerate and hostile cameras
            trt_camera c = cams[0];
            for (float v : {0.0f, nan, inf, -inf, 3e38f, 1e-42f}) {
                for (int f = 0; f < 12; ++f) { trt_camera d = c; (&d.eye[0])[f] = v; cams.push_back(d); }
                trt_camera z = c;
                for (int k = 0; k < 3; ++k) { z.horizontal[k] = v; z.vertical[k] = v; }
                cams.push_back(z);
            }
            trt_camera p = c;
            for (int k = 0; k < 3; ++k) p.vertical[k] = p.horizontal[k];  // parallel axes: every system is singular
            cams.push_back(p);
        }
        for (const trt_camera& cam : cams)
            for (const auto& bx : boxes)
                for (int fixed = 0; fixed < 2; ++fixed)
                    for (uint32_t n_nodes : {1u, 0u}) {
                        int32_t out[16];
                        const char* why = nullptr;
                        const int active = cull_bound(&cam, W, H, fixed, bx.data(), n_nodes, 1.0, out, &why);
                        ++cases;
                        if (!why) { ++bad; continue; }
                        if (!active) {
                            for (int k = 0; k < 8; ++k) bad += out[k] != 0;
                            continue;
                        }
                        bad += n_nodes == 0;
                        bad += out[0] < 0 || out[1] < 0 || out[0] > W || out[1] > W || out[2] < 0 || out[3] < 0 || out[2] > H || out[3] > H;
                        bad += out[4] < 0 || out[5] < 0 || out[4] + out[5] > H || out[6] < 0 || out[7] < 0 || out[6] + out[7] > W;
                        if ((int64_t)W * H <= 4096) {
                            uint64_t counts[7];
                            cull_sweep(&cam, W, H, fixed, bx.data(), n_nodes, 1.0, 7, 4, counts);
                            bad += counts[2] != 0 || counts[3] != 0 || counts[4] != 0 || counts[5] != 0;
                        }
                    }
    }
    std::printf("%s %d\n", bad ? "FAILED" : "ok", cases);
    return bad ? 1 : 0;
}
