// nearlights_san.cpp — TEST INFRASTRUCTURE.  A stand-alone program around the CPU build of TRT_FLAG_NEAR_LIGHTS (nearlights_cpu.cpp, compiled in), built with
// -fsanitize=address,undefined by tests/test_near_lights_cpu.py: a corridor scene (tests/near_cases.py writes it) at 16 x 9 x 2 spp in all five modes, then
// the tree and the descent over hostile light tables — NaN, negative, zero and infinite areas, radiances and vertices, 0, 1, 2, 3 and 300 lights, the
// uniforms 0 and 1 - 2^-24, points at the lights, far away and at 1e30 — then an update that moves the lamps: the tree rebuilt from the moved tables.
// Every index returned must lie in [0, L); a sampled light must carry an inv_p >= 1.  argv[1]: the directory of the scene, argv[2]: its name.
// Prints "ok ..." and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "trt.h"
#include "trt_host.h"

extern "C" int nearlights_render(const trt_scene* s, const trt_params* p, float* out_rgb, uint64_t rays[3], int mode);
extern "C" int nearlights_scene_tables(const trt_scene* s, float* area, float* radiance, uint32_t* tri_first, uint32_t* tri_count, float* verts);
extern "C" int nearlights_tree(uint32_t n, const float* area, const float* radiance, const uint32_t* tri_first, const uint32_t* tri_count, uint32_t n_ltris, const float* verts,
                               void* nodes, uint32_t info[3]);
extern "C" int nearlights_pick(uint32_t n, const float* area, const float* radiance, const uint32_t* tri_first, const uint32_t* tri_count, uint32_t n_ltris, const float* verts,
                               uint64_t m, const float* P, const float* u, uint8_t* sampled, uint32_t* index, float* inv_p, uint32_t* draws, float* u_used);

namespace {
int fail(const char* what)
{
    std::printf("FAILED: %s\n", what);
    return 1;
}
uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

struct Tables {
    std::vector<float> area, rad, verts;
    std::vector<uint32_t> first, count;
    explicit Tables(uint32_t L) : area(L + 1), rad(3 * (size_t)L + 3), verts(18 * (size_t)L + 9), first(L + 1), count(L + 1) {}
};
// the tree and picks at the points P (m of them, each with u = 0, u = 1 - 2^-24, u = 0.5 at every level, and a stream of its own) -> 0, or what broke
const char* probe(uint32_t L, const Tables& t, uint32_t n_ltris, const std::vector<float>& P, uint64_t& picks, uint64_t& none)
{
    std::vector<float> nodes(16 * (size_t)(L > 2 ? L : 2));
    uint32_t info[3];
    if (nearlights_tree(L, t.area.data(), t.rad.data(), t.first.data(), t.count.data(), n_ltris, t.verts.data(), nodes.data(), info)) return "nearlights_tree";
    const uint32_t M = info[2];
    if (M > L || info[1] != (M >= 2 ? M - 1 : 0)) return "node count is not M - 1";
    const uint64_t m = P.size() / 3;
    std::vector<uint8_t> sampled(m);
    std::vector<uint32_t> index(m), draws(m);
    std::vector<float> inv_p(m), used(16 * m), u(16 * m);
    const float us[] = {0.0f, 1.0f - 1.0f / 16777216.0f, 0.5f};
    for (int k = 0; k < 4; ++k) {
        if (k < 3) u.assign(16 * m, us[k]);
        if (int rc = nearlights_pick(L, t.area.data(), t.rad.data(), t.first.data(), t.count.data(), n_ltris, t.verts.data(), m, P.data(), k < 3 ? u.data() : nullptr,
                                     sampled.data(), index.data(), inv_p.data(), draws.data(), used.data()))
            return rc == 3 ? "lightPickNear and the per-level loop disagree" : "nearlights_pick";
        for (uint64_t i = 0; i < m; ++i) {
            if (L == 0 ? (sampled[i] || index[i] != 0u) : index[i] >= L) return "index out of [0, L)";
            if (draws[i] > 16u || ((L < 2 || M < 2) && draws[i] != 0u)) return "draws taken";
            if (L >= 2 && M == 0 && sampled[i]) return "a light was sampled without a tree light";
            if (!sampled[i]) { none++; continue; }
            picks++;
            if (!(inv_p[i] >= 1.0f) || !std::isfinite(inv_p[i])) return "inv_p below 1 or not finite for a sampled light";
            if (L >= 2 && M == 1 && inv_p[i] != 1.0f) return "inv_p of the only tree light is not 1";
        }
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return fail("usage: nearlights_san <scene directory> <scene name>");
    const std::string d = argv[1], n = argv[2];
    trth_scene* sc = trth_scene_load((d + "/" + n + ".xml").c_str(), (d + "/" + n + ".obj").c_str(), (d + "/" + n + ".mtl").c_str(), d.c_str(), 16, 9);
    if (!sc) return fail(trth_last_error());
    if (trth_scene_build(sc, 2, TRTH_BVH_AUTO)) return fail(trth_last_error());
    const trt_scene* flat = trth_scene_flat(sc);
    if (!flat || flat->n_lights < 2) return fail("a corridor of two or more lamps expected");
    trt_params p{};
    p.width = 16; p.height = 9; p.spp = 2; p.seed = 7;
    p.x1 = 16; p.y1 = 9;
    p.row_block = 1; p.row_mod = 1;
    p.flags = TRT_FLAG_NEAR_LIGHTS | TRT_FLAG_ONE_LIGHT | TRT_FLAG_FIXED_NEE;
    std::vector<float> img(16 * 9 * 3);
    uint64_t rays[3] = {0, 0, 0};
    double sum = 0.0;
    for (int mode = 0; mode < 5; ++mode) {
        if (nearlights_render(flat, &p, img.data(), rays, mode)) return fail("nearlights_render");
        for (float v : img) {
            if (!std::isfinite(v)) return fail("a pixel is not finite");
            sum += v;
        }
        if (rays[0] != 16u * 9u * 2u) return fail("camera rays");
    }
    p.flags = TRT_FLAG_NEAR_LIGHTS | TRT_FLAG_ONE_LIGHT;
    if (nearlights_render(flat, &p, img.data(), rays, 0) == 0) return fail("the flags without TRT_FLAG_FIXED_NEE were accepted");

    uint64_t picks = 0, none = 0;
    // ---- the scene's own tables, then an update that moves the lamps: the tree is rebuilt from the moved vertices
    {
        const uint32_t L = flat->n_lights, nt = flat->n_light_tris;
        Tables t(L);
        t.verts.resize(9 * (size_t)nt + 9);
        if (nearlights_scene_tables(flat, t.area.data(), t.rad.data(), t.first.data(), t.count.data(), t.verts.data())) return fail("nearlights_scene_tables");
        std::vector<float> P;
        for (uint32_t k = 0; k < nt; ++k)
            for (int a = 0; a < 3; ++a) P.push_back(t.verts[9 * (size_t)k + a] + (a == 1 ? -1.0f : 0.25f));  // on the floor under the lamps
        for (int move = 0; move < 2; ++move) {
            if (const char* e = probe(L, t, nt, P, picks, none)) return fail(e);
            for (uint32_t k = 0; k < nt; ++k)
                for (int v = 0; v < 3; ++v) { t.verts[9 * (size_t)k + 3 * v] += 1.5f; t.verts[9 * (size_t)k + 3 * v + 1] += 0.25f; }
        }
    }
    trth_scene_free(sc);

    // ---- hostile tables
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float hostile[] = {nan, -1.0f, 0.0f, -0.0f, inf, -inf, 1.0e-45f, 3.0e38f, 1.0f, 2.5f, 1.0e-30f, 1.0e30f};
    const uint32_t nh = sizeof(hostile) / sizeof(hostile[0]);
    uint32_t seed = 12345u;
    for (uint32_t L : {2u, 3u, 300u, 0u, 1u})
        for (int round = 0; round < 40; ++round) {
            Tables t(L);
            // round 0: everything hostile; later rounds mix hostile and plain entries; the last rounds leave one plain light or none
            for (uint32_t l = 0; l < L; ++l) {
                const bool plain_only = round >= 38 && l == 0 && round == 38;
                t.area[l] = plain_only ? 1.0f : ((round == 0 || round >= 38 || lcg(seed) % 3 == 0) ? hostile[lcg(seed) % nh] : 0.25f + (float)(lcg(seed) % 1000));
                for (int k = 0; k < 3; ++k)
                    t.rad[3 * l + k] = plain_only ? 1.0f : ((round == 0 || lcg(seed) % 4 == 0) ? hostile[lcg(seed) % nh] : (float)(lcg(seed) % 50));
                t.first[l] = 2 * l;
                t.count[l] = (lcg(seed) % 8 == 0) ? 0u : 2u;
                if (plain_only) t.count[l] = 2u;
                for (int k = 0; k < 18; ++k)
                    t.verts[18 * (size_t)l + k] = (!plain_only && (round == 0 || lcg(seed) % 40 == 0)) ? hostile[lcg(seed) % nh] : (float)(lcg(seed) % 2000) * 0.01f - 10.0f;
            }
            if (round >= 38)
                for (uint32_t l = 1; l < L; ++l) t.area[l] = (l & 1u) ? nan : -1.0f;
            std::vector<float> P;
            for (uint32_t l = 0; l < L && l < 8; ++l)
                for (int a = 0; a < 3; ++a) P.push_back(t.verts[18 * (size_t)l + a]);
            for (float x : {0.0f, 5.0f, -1.0e4f, 1.0e30f, -1.0e30f, nan, inf})
                for (int a = 0; a < 3; ++a) P.push_back(a == 1 ? 0.5f * x : x);
            if (const char* e = probe(L, t, 2 * L, P, picks, none)) return fail(e);
        }
    std::printf("ok %llu picks, %llu vertices without a light, image sum %.6g\n", (unsigned long long)picks, (unsigned long long)none, sum);
    return 0;
}
