// shade_cases_host.h — TEST INFRASTRUCTURE.  The CPU side of tools/shade_case_check: the same case file, the same section functions (tools/shade_cases.h),
// the same order of output words, under OpenMP.  A template on the functions under test: hostsim.cpp runs the headers' own, shade_mutants.cpp altered copies.
#pragma once
#include <cstring>
#include <vector>

#include "../../tools/shade_cases.h"

namespace shadecases {

template <class T>
inline std::vector<T> section(const uint8_t* p, size_t n)
{
    std::vector<T> v(n ? n : 1);  // an aligned copy: the caller's buffer need not be
    if (n) std::memcpy(static_cast<void*>(v.data()), p, n * sizeof(T));
    return v;
}

// -> 0, or 2 for a file parse() refuses or a result buffer of the wrong size
template <class F>
inline int runFileHost(const uint8_t* buf, uint64_t size, uint32_t* out, uint64_t n_words)
{
    View v;
    if (parse(buf, size, v) || v.n_words != n_words) return 2;
    const Header& h = v.h;
    const auto mat = section<MaterialDev>(v.mat, h.n_mat);
    const auto tex = section<TextureDev>(v.tex, h.n_tex);
    const auto lights = section<LightDev>(v.lights, h.n_lights);
    const auto ltris = section<LightTriDev>(v.ltris, h.n_ltris);
    const auto tshade = section<TriShade>(v.tshade, h.n_tris);
    const auto tisect = section<TriIsect>(v.tisect, h.n_tris);
    const auto prim = section<PrimCase>(v.prim, h.n_prim);
    const auto cam = section<CamCase>(v.cam, h.n_cam);
    const auto vert = section<VertCase>(v.vert, h.n_vert);
    const auto light = section<LightCase>(v.light, h.n_light);
    const auto next = section<NextCase>(v.next, h.n_next);
    const auto dir = section<DirCase>(v.dir, h.n_dir);
    const auto bounce = section<BounceCase>(v.bounce, h.n_bounce);
    const auto plights = section<LightDev>(v.plights, h.n_plights);
    const auto psel = section<float>(v.psel, h.n_psel);
    const auto pnodes = section<LightNode>(v.pnodes, h.n_pnodes);  // (over-aligned type: the vector's storage is 16-byte aligned)
    const auto sets = section<LightSet>(v.sets, h.n_sets);
    const auto pick = section<PickCase>(v.pick, h.n_pick);
    const auto step = section<StepCase>(v.step, h.n_step);
    const auto near = section<NearCase>(v.near, h.n_near);
    const Pools pl{plights.data(), psel.data(), pnodes.data(), sets.data()};
    std::vector<float> cum(h.n_ltris ? h.n_ltris : 1);
    for (uint32_t i = 0; i < h.n_ltris; ++i) cum[i] = ltris[i].cum_area;
    int32_t rows[BOUNCE_ROWS];
    for (int r = 0; r < BOUNCE_ROWS; ++r) rows[r] = r;
    SceneDev sc{};
    sc.materials = mat.data();
    sc.textures = tex.data();
    sc.tex_bytes = v.texbytes;
    sc.lights = lights.data();
    sc.light_tris = ltris.data();
    sc.tri_shade = tshade.data();
    sc.tri_isect = tisect.data();
    sc.n_tris = h.n_tris;
    sc.n_lights = h.n_lights;
    uint32_t* o = out;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_prim; ++i) runPrim(prim[i], o + (size_t)W_PRIM * i);
    o += (size_t)W_PRIM * h.n_prim;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_cam; ++i) runCam(cam[i], o + (size_t)W_CAM * i);
    o += (size_t)W_CAM * h.n_cam;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_vert; ++i) runVert<F>(sc, vert[i], o + (size_t)W_VERT * i);
    o += (size_t)W_VERT * h.n_vert;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_light; ++i) runLight<F>(sc, cum.data(), light[i], o + (size_t)W_LIGHT * i);
    o += (size_t)W_LIGHT * h.n_light;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_next; ++i) runNext<F>(sc, next[i], o + (size_t)W_NEXT * i);
    o += (size_t)W_NEXT * h.n_next;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_dir; ++i) runDir<F>(dir[i], o + (size_t)W_DIR * i);
    o += (size_t)W_DIR * h.n_dir;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_bounce; ++i) runBounce(sc, rows, bounce[i], o + (size_t)W_BOUNCE * i);
    o += (size_t)W_BOUNCE * h.n_bounce;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_pick; ++i) runPick<F>(pl, pick[i], o + (size_t)W_PICK * i);
    o += (size_t)W_PICK * h.n_pick;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)h.n_step; ++i) runStep<F>(step[i], o + (size_t)W_STEP * i);
    o += (size_t)W_STEP * h.n_step;
#pragma omp parallel for schedule(dynamic, 256)
    for (long long i = 0; i < (long long)h.n_near; ++i) runNear(pl, near[i], o + (size_t)W_NEAR * i);
    return 0;
}

}  // namespace shadecases
