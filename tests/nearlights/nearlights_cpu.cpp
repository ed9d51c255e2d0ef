// nearlights_cpu.cpp — TEST INFRASTRUCTURE.  The CPU build of TRT_FLAG_NEAR_LIGHTS (include/trt.h): hostsim_render's per-path loop (tests/hostsim/hostsim.cpp,
// included for its HostScene) with the loop over the lights replaced by what k_shade's SHADE_NEAR flavour and k_tail do under TileDesc::near_lights —
// lightPickNear (trt_path.h) on the tree buildLightTree (trt_lighttree.h) makes, that light's lightSample, the occlusion test, the contribution times
// inv_p.  Sums in k_tail's order.  Nothing in the product loads it.
#include "../hostsim/hostsim.cpp"
#include "trt_lighttree.h"

// mode 0: the feature.  1: inv_p forced to 1.  2: the tree's pick with inv_p = TRT_FLAG_ONE_LIGHT's cdf_{L-1} / w_l (as if the pick had been by power).
// 3: TRT_FLAG_ONE_LIGHT.  4: every light at every vertex, TRT_FLAG_FIXED_NEE's estimator.  (1 and 2 are biased: the sensitivity checks of tests/test_near_lights_cpu.py.)
namespace {
enum { NEAR = 0, MUTANT_NO_WEIGHT = 1, MUTANT_POWER_WEIGHT = 2, ONE_LIGHT = 3, ALL_LIGHTS = 4 };

int renderWith(const HostScene& hs, const trt_params* p, uint32_t seed, int32_t n_spp, int mode, float* out_rgb, uint64_t rays[3])
{
    const bool pick = mode != ALL_LIGHTS && hs.sc.n_lights >= 2;  // fewer than two lights: the flags do nothing, no draw is taken
    const bool near = pick && mode != ONE_LIGHT;
    std::vector<int32_t> rows;
    for (int y = p->y0; y < p->y1; ++y)
        if (p->row_mod <= 1 || ((y / p->row_block) % p->row_mod) == p->row_rem) rows.push_back(y);
    const uint32_t tw = (uint32_t)(p->x1 - p->x0), npix = (uint32_t)rows.size() * tw;
    TileDesc td{};
    td.rows = rows.data();
    td.tile_w = (int32_t)tw; td.x0 = p->x0; td.width = p->width; td.height = p->height;
    td.npix = npix; td.seed = seed; td.spp = (uint32_t)n_spp;
    td.fixed_nee = 1u;
    td.fixed_pixels = (p->flags & TRT_FLAG_FIXED_PIXELS) ? 1u : 0u;
    td.ray_offset = (p->flags & TRT_FLAG_RAY_OFFSET) ? 1u : 0u;
    td.specular_ks = (p->flags & TRT_FLAG_SPECULAR_KS) ? 1u : 0u;
    td.npix_magic = magicOf(npix); td.tile_w_magic = magicOf(tw);
    td.one_light = pick ? 1u : 0u;
    td.near_lights = near ? 1u : 0u;
    uint64_t r_cam = 0, r_sh = 0, r_ind = 0;
    const uint32_t S = (uint32_t)n_spp;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : r_cam, r_sh, r_ind)
    for (long pl = 0; pl < (long)npix; ++pl) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        double acc[3] = {0, 0, 0};
        for (uint32_t sidx = 0; sidx < S; ++sidx) {
            const uint32_t pid = sidx * npix + (uint32_t)pl;
            const uint32_t r = (uint32_t)pl / tw, c = (uint32_t)pl - r * tw;
            const int y = rows[r], x = p->x0 + (int)c;
            Stream rng;
            rng.key = trt_rng_make_key(td.seed, (uint32_t)y * (uint32_t)td.width + (uint32_t)x, sidx);
            rng.ctr = 0;
            const float u1 = rng.next(), u2 = rng.next();
            f3 o, d;
            cameraRay(hs.sc.cam, td.width, td.height, y, x, u1, u2, o, d, td.fixed_pixels != 0u);
            f4 ra = mk4(o.x, o.y, o.z, d.x), rb = mk4(d.y, d.z, u2f(pid), u2f(packMeta(rng.ctr, TRT_META_CAMERA, 0))), bt = mk4(1, 1, 1, 0);
            f3 L = mk3(0, 0, 0);
            r_cam++;
            for (;;) {
                const Hit h = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), ostk, stk, ni, nt)
                                    : traceClosest<ArrayStack, false, 0>(hs.sc, mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), stk, ni, nt);
                const f4 hit4 = mk4(h.t, u2f((uint32_t)h.tri), h.u, h.v);
                ShadeCtx cx;
                shadeBegin(hs.sc, td, 0, ra, rb, bt, hit4, cx);
                if (cx.add_L) L = L + cx.addL;
                const uint32_t n_loop = pick ? 1u : hs.sc.n_lights;
                for (uint32_t lk = 0; lk < n_loop; ++lk) {
                    f3 wo, contrib;
                    float t_max = TRT_INF;
                    uint32_t li = lk;
                    float inv_p = 1.0f;
                    if (!cx.shade_ok || (pick && !(near ? lightPickNear(hs.sc, cx.vx.P, cx.rng, li, inv_p) : lightPick(hs.sc, cx.rng, li, inv_p))) ||
                        !lightSample(hs.sc, cx.vx, *cx.m, li, cx.rng, wo, contrib, true, t_max))
                        continue;
                    if (mode == MUTANT_NO_WEIGHT) inv_p = 1.0f;
                    if (mode == MUTANT_POWER_WEIGHT && near) inv_p = hs.sc.light_sel[hs.sc.n_lights - 1u] / lightWeight(hs.sc.lights[li]);
                    if (pick) contrib = mk3(contrib.x * inv_p, contrib.y * inv_p, contrib.z * inv_p);
                    const f3 w = cx.beta * contrib;
                    r_sh++;
                    // the occlusion test: no light material, no light box
                    const Hit sh = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, rayOrigin(cx, wo), wo, ostk, stk, ni, nt, t_max, true, false, nullptr)
                                         : traceClosest<ArrayStack, false, 0>(hs.sc, rayOrigin(cx, wo), wo, stk, ni, nt, t_max, true, false);
                    if (sh.tri < 0) L = L + w;
                }
                f4 nra, nrb, nbt;
                if (!shadeNext(cx, p->max_depth, nra, nrb, nbt)) break;
                ra = nra; rb = nrb; bt = nbt;
                r_ind++;
            }
            const float spp = (float)n_spp;
            acc[0] += (double)(L.x / spp);
            acc[1] += (double)(L.y / spp);
            acc[2] += (double)(L.z / spp);
        }
        out_rgb[(size_t)pl * 3 + 0] = (float)acc[0];
        out_rgb[(size_t)pl * 3 + 1] = (float)acc[1];
        out_rgb[(size_t)pl * 3 + 2] = (float)acc[2];
    }
    if (rays) { rays[0] = r_cam; rays[1] = r_sh; rays[2] = r_ind; }
    return g_breaches.exchange(0) ? 2 : 0;
}
// the light tables of a SceneDev as a handle holds them: the selection table and the light tree where there is something to select
struct LightTables {
    std::vector<float> sel;
    LightTree tree;
    void attach(SceneDev& sc, uint32_t n_ltris)
    {
        sel.resize(sc.n_lights);
        lightSelTable(sc.lights, sc.n_lights, sel.data());
        buildLightTree(sc.lights, sc.n_lights, sc.light_tris, n_ltris, tree);
        const bool some = sc.n_lights >= 2;
        sc.light_sel = some ? sel.data() : nullptr;
        sc.light_nodes = (some && !tree.nodes.empty()) ? tree.nodes.data() : nullptr;
        sc.n_light_nodes = some ? (uint32_t)tree.nodes.size() : 0u;
        sc.light_root = some ? tree.root : TRT_LIGHT_NONE;
    }
};
struct NearScene {
    HostScene hs;
    LightTables lt;
    explicit NearScene(const trt_scene* s) : hs(s) { lt.attach(hs.sc, s->n_light_tris); }
};
// caller's tables -> lights and triangles in device layout.  verts: 9 floats per light triangle.
struct TableScene {
    std::vector<LightDev> lights;
    std::vector<LightTriDev> ltris;
    SceneDev sc{};
    LightTables lt;
    TableScene(uint32_t n, const float* area, const float* radiance, const uint32_t* tri_first, const uint32_t* tri_count, uint32_t n_ltris, const float* verts)
        : lights(n), ltris(n_ltris)
    {
        for (uint32_t l = 0; l < n; ++l) {
            trt_light t{};
            t.area = area[l];
            t.tri_first = tri_first[l];
            t.tri_count = tri_count[l];
            lights[l] = makeLightDevFrom(t, radiance + 3 * (size_t)l);
        }
        for (uint32_t k = 0; k < n_ltris; ++k) {
            trt_light_tri t{};
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) t.v[v][a] = verts[9 * (size_t)k + 3 * v + a];
            ltris[k] = makeLightTriDev(t);
        }
        sc.lights = lights.data();
        sc.light_tris = ltris.data();
        sc.n_lights = n;
        lt.attach(sc, n_ltris);
    }
};
}  // namespace

// The tile of p (trt_render's packing) -> out_rgb, rays = (camera, shadow, indirect) rays traced.  p->flags must hold TRT_FLAG_FIXED_NEE (the library: TRT_EINVAL).
extern "C" int nearlights_render(const trt_scene* s, const trt_params* p, float* out_rgb, uint64_t rays[3], int mode)
{
    if (!s || !p || !out_rgb || !(p->flags & TRT_FLAG_FIXED_NEE)) return 1;
    NearScene ns(s);
    return renderWith(ns.hs, p, p->seed, p->spp, mode, out_rgb, rays);
}
// n one-sample renders of the tile of p with the seeds p->seed + 1 + k -> out_rgb[n][pixels][3]
extern "C" int nearlights_render_seeds(const trt_scene* s, const trt_params* p, int mode, uint32_t n, float* out_rgb)
{
    if (!s || !p || !out_rgb || !(p->flags & TRT_FLAG_FIXED_NEE)) return 1;
    NearScene ns(s);
    int rows = 0;
    for (int y = p->y0; y < p->y1; ++y)
        if (p->row_mod <= 1 || ((y / p->row_block) % p->row_mod) == p->row_rem) rows++;
    const size_t floats = (size_t)rows * (size_t)(p->x1 - p->x0) * 3;
    for (uint32_t k = 0; k < n; ++k)
        if (int rc = renderWith(ns.hs, p, p->seed + 1u + k, 1, mode, out_rgb + floats * k, nullptr)) return rc;
    return 0;
}

// The light tables of a scene as trt_create reads them: area [L], the light MATERIAL's radiance [L][3], tri_first [L], tri_count [L], verts [n_light_tris][9].
extern "C" int nearlights_scene_tables(const trt_scene* s, float* area, float* radiance, uint32_t* tri_first, uint32_t* tri_count, float* verts)
{
    if (!s) return 1;
    for (uint32_t l = 0; l < s->n_lights; ++l) {
        area[l] = s->lights[l].area;
        for (int k = 0; k < 3; ++k) radiance[3 * (size_t)l + k] = s->materials[s->lights[l].mat].radiance[k];
        tri_first[l] = s->lights[l].tri_first;
        tri_count[l] = s->lights[l].tri_count;
    }
    for (uint32_t k = 0; k < s->n_light_tris; ++k)
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) verts[9 * (size_t)k + 3 * v + a] = s->light_tris[k].v[v][a];
    return 0;
}

// buildLightTree on the caller's tables -> nodes (room for max(n, 2) - 1 records of 64 bytes), info = (root reference, node count, M).
extern "C" int nearlights_tree(uint32_t n, const float* area, const float* radiance, const uint32_t* tri_first, const uint32_t* tri_count, uint32_t n_ltris, const float* verts,
                               void* nodes, uint32_t info[3])
{
    TableScene ts(n, area, radiance, tri_first, tri_count, n_ltris, verts);
    if (ts.lt.tree.nodes.size() + 1u > (n > 2u ? n : 2u)) return 4;
    if (!ts.lt.tree.nodes.empty()) std::memcpy(nodes, ts.lt.tree.nodes.data(), ts.lt.tree.nodes.size() * sizeof(LightNode));
    info[0] = ts.lt.tree.root; info[1] = (uint32_t)ts.lt.tree.nodes.size(); info[2] = ts.lt.tree.n_tree_lights;
    return 0;
}

// lightPickNear on the caller's tables at m points P [m][3].  Point k draws from a stream of its own (key k); with u != null the uniform of level j is
// u[16 k + j] instead (the same per-level function, lightNodeStep, in the loop lightPickNear runs).  Per point: sampled (0 / 1), the index, inv_p, the draws
// taken, and u_used [m][16]: the uniforms of the levels.  -> 3 where lightPickNear on the stream and the loop over the stream's uniforms disagree.
extern "C" int nearlights_pick(uint32_t n, const float* area, const float* radiance, const uint32_t* tri_first, const uint32_t* tri_count, uint32_t n_ltris, const float* verts,
                               uint64_t m, const float* P, const float* u, uint8_t* sampled, uint32_t* index, float* inv_p, uint32_t* draws, float* u_used)
{
    TableScene ts(n, area, radiance, tri_first, tri_count, n_ltris, verts);
    const SceneDev& sc = ts.sc;
    int rc = 0;
    for (uint64_t k = 0; k < m; ++k) {
        const f3 p = mk3(P[3 * k], P[3 * k + 1], P[3 * k + 2]);
        Stream rng;
        rng.key = trt_rng_make_key(0x2EA7u, (uint32_t)k, (uint32_t)(k >> 32));
        rng.ctr = 0;
        uint32_t li_s = 0xFFFFFFFFu;
        float ip_s = 0.0f;
        const bool ok_s = lightPickNear(sc, p, rng, li_s, ip_s);
        for (int j = 0; j < 16; ++j) u_used[16 * k + j] = u ? u[16 * k + j] : trt_rng_uniform(rng.key, (uint32_t)j);
        // the loop of lightPickNear over the given uniforms
        uint32_t li = 0u, taken = 0u;
        float ip = 1.0f;
        bool ok;
        if (n < 2u) {
            ok = n == 1u;
        } else if (sc.light_root == TRT_LIGHT_NONE) {
            ok = false;
        } else {
            uint32_t ref = sc.light_root;
            while (!(ref & TRT_LIGHT_LEAF)) {
                if (ref >= sc.n_light_nodes || taken >= 16u) return 5;
                ref = lightNodeStep(sc.light_nodes[ref], p, u_used[16 * k + taken++], ip);
            }
            li = ref & ~TRT_LIGHT_LEAF;
            ok = fabsf(ip) < __builtin_inff();
            if (!ok) ip = 1.0f;
        }
        if (!u && (ok != ok_s || li != li_s || f2u(ip) != f2u(ip_s) || taken != rng.ctr)) rc = 3;
        sampled[k] = ok ? 1 : 0;
        index[k] = li;
        inv_p[k] = ip;
        draws[k] = u ? taken : rng.ctr;
    }
    return rc;
}
