// onelight_san.cpp — TEST INFRASTRUCTURE.  A stand-alone program around the CPU build of TRT_FLAG_ONE_LIGHT (onelight_cpu.cpp, compiled in), built with
// -fsanitize=address,undefined by tests/test_one_light_cpu.py: `lamps` with 8 lamps at 16 x 9 x 2 spp, then lightPick over hostile light tables — NaN,
// negative, zero and infinite areas and radiances, 2 and 300 lights, the uniforms 0 and 1 - 2^-24, with and without the selection table.  Every index
// returned must lie in [0, L); a sampled light must have a positive weight.  argv[1]: the directory of scenes/back.  Prints "ok ..." and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "trt.h"
#include "trt_host.h"

extern "C" int onelight_render(const trt_scene* s, const trt_params* p, float* out_rgb, uint64_t rays[3], int mutant);
extern "C" int onelight_pick(uint32_t n, const float* area, const float* radiance, int table, uint64_t m, const float* u, uint8_t* sampled, uint32_t* index, float* inv_p,
                             uint32_t* draws, float* cdf_out);

namespace {
int fail(const char* what)
{
    std::printf("FAILED: %s\n", what);
    return 1;
}
uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return fail("usage: onelight_san <scenes/back>");
    const std::string d = argv[1];
    trth_scene* sc = trth_scene_load((d + "/back.xml").c_str(), (d + "/back.obj").c_str(), (d + "/back.mtl").c_str(), d.c_str(), 16, 9);
    if (!sc) return fail(trth_last_error());
    if (trth_scene_add_lamps(sc, 0x5EED0006u, 8) || trth_scene_build(sc, 8, TRTH_BVH_AUTO)) return fail(trth_last_error());
    const trt_scene* flat = trth_scene_flat(sc);
    if (!flat || flat->n_lights != 9) return fail("lamps: 9 lights expected");
    trt_params p{};
    p.width = 16; p.height = 9; p.spp = 2; p.seed = 7;
    p.x1 = 16; p.y1 = 9;
    p.row_block = 1; p.row_mod = 1;
    p.flags = TRT_FLAG_ONE_LIGHT | TRT_FLAG_FIXED_NEE;
    std::vector<float> img(16 * 9 * 3);
    uint64_t rays[3] = {0, 0, 0};
    double sum = 0.0;
    for (int mode = 0; mode < 3; ++mode) {
        if (onelight_render(flat, &p, img.data(), rays, mode)) return fail("onelight_render");
        for (float v : img) {
            if (!std::isfinite(v)) return fail("a pixel is not finite");
            sum += v;
        }
        if (rays[0] != 16u * 9u * 2u) return fail("camera rays");
    }
    p.flags = TRT_FLAG_ONE_LIGHT;
    if (onelight_render(flat, &p, img.data(), rays, 0) == 0) return fail("the flag without TRT_FLAG_FIXED_NEE was accepted");
    trth_scene_free(sc);

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float hostile[] = {nan, -1.0f, 0.0f, -0.0f, inf, -inf, 1.0e-45f, 3.0e38f, 1.0f, 2.5f, 1.0e-30f, 1.0e30f};
    const uint32_t nh = sizeof(hostile) / sizeof(hostile[0]);
    const float us[] = {0.0f, 1.0f - 1.0f / 16777216.0f, 0.5f, 1.0f / 16777216.0f, 0.999f};
    const uint32_t nu = sizeof(us) / sizeof(us[0]);
    uint32_t seed = 12345u;
    uint64_t picks = 0, none = 0;
    for (uint32_t L : {2u, 300u, 0u, 1u})
        for (int round = 0; round < 200; ++round) {
            std::vector<float> area(L + 1), rad(3 * (size_t)L + 3);
            // round 0: everything hostile; later rounds mix hostile and plain entries
            for (uint32_t l = 0; l < L; ++l) {
                area[l] = (round == 0 || lcg(seed) % 3 == 0) ? hostile[lcg(seed) % nh] : 0.25f + (float)(lcg(seed) % 1000);
                for (int k = 0; k < 3; ++k) rad[3 * l + k] = (round == 0 || lcg(seed) % 4 == 0) ? hostile[lcg(seed) % nh] : (float)(lcg(seed) % 50);
            }
            for (int table = 0; table < 2; ++table) {
                uint8_t sampled[nu];
                uint32_t index[nu], draws[nu];
                float inv_p[nu];
                std::vector<float> cdf(L + 1);
                if (onelight_pick(L, area.data(), rad.data(), table, nu, us, sampled, index, inv_p, draws, cdf.data())) return fail("onelight_pick: lightPick and lightPickAt disagree");
                for (uint32_t k = 0; k < nu; ++k) {
                    if (draws[k] != (L >= 2 ? 1u : 0u)) return fail("draws taken");
                    if (L == 0 ? (sampled[k] || index[k] != 0u) : index[k] >= L) return fail("index out of [0, L)");
                    if (!sampled[k]) { none++; continue; }
                    picks++;
                    if (L >= 2 && !(inv_p[k] >= 1.0f)) return fail("inv_p below 1 or NaN for a sampled light");
                }
            }
        }
    std::printf("ok %llu picks, %llu vertices without a light, image sum %.6g\n", (unsigned long long)picks, (unsigned long long)none, sum);
    return 0;
}
