// hostsim.cpp — TEST INFRASTRUCTURE.  Compiles the device-side path functions
// (tinyraytracing_amd/csrc/trt_path.h: traversal, triangle/box tests,
// shadeBegin / lightSample / shadeNext) with g++ and drives them per path in
// the wavefront kernels' order of operations, so their arithmetic can be checked
// bit-for-bit against the oracle on a machine without a GPU.  It is not a render
// back end: nothing in the product loads this library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <limits>
#include <vector>

// range checks of the traversal (TRT_WALK_CHECK, trt_path.h): a walk that would leave the tree, the triangles or the stack the GPU
// driver has ends its ray and is counted (g_breaches: the entry then returns 2) instead of reading out of range
#define TRT_HOSTSIM_CHECKS 1
#include "trt_path.h"
#include "trt_wide.h"
#include "trt_oct_build.h"
#include "trt_refit.h"
#include "../refit/refit_loops.h"

using namespace trtd;

namespace {
int g_node_kind = 0;  // hostsim_set_node_kind: 0 = exact 4-wide nodes; 1 = the 8-wide compressed nodes of trt_oct.h where the tree allows them
std::atomic<uint64_t> g_breaches{0};  // walks TRT_WALK_CHECK ended: reset when an entry builds its HostScene; the entry returns 2 when it is not 0 at the end
struct ArrayStack {
    uint32_t s[1024];
    uint32_t cap = 1024;       // entries the 4-wide walk can need on this tree: the collapse's stack_need (HostScene::stack())
    uint32_t bvh2_cap = 1024;  // entries the literal walk of the caller's BVH2 can need: its inner depth (k_trace_fix / k_tail size theirs from it)
    void push(int sp, uint32_t v)
    {
        if (sp >= 0 && sp < 1024) s[sp] = v;
        else g_breaches++;
    }
    uint32_t pop(int sp) const { return sp >= 0 && sp < 1024 ? s[sp] : TRT_WIDE_EMPTY; }
    int capacity() const { return (int)cap; }
    int bvh2Capacity() const { return (int)bvh2_cap; }
    void breach() const { g_breaches++; }
};

// a recorder of the parity-mode shadow rays hostsim_render traces (hostsim_shadow_rays)
struct ShadowRec {
    uint64_t cap;
    std::atomic<uint64_t> n{0};
    float *org, *dir;
    int32_t* light;
};
ShadowRec* g_shadow_rec = nullptr;

struct OctArrayStack {
    OctGroup s[256];
    void push(int sp, OctGroup g) { s[sp] = g; }
    OctGroup pop(int sp) const { return s[sp]; }
};

struct HostScene {
    std::vector<TriIsect> isect;
    std::vector<TriShade> shade;
    std::vector<MaterialDev> mats;
    std::vector<TextureDev> tex;
    std::vector<uint8_t> tex_bytes;
    std::vector<float> cum;
    std::vector<LightDev> lights;
    std::vector<LightTriDev> ltris;
    WideTree wide;
    OctTree oct;
    std::vector<f4> leaf_boxes;
    std::vector<LightBox> light_boxes;
    std::vector<uint32_t> plane_bits;
    int nk = 0;  // node kind the traversal walks: 0 exact 4-wide nodes, 1 compressed 8-wide nodes (TRT_NODE_KIND)
    SceneDev sc{};
    uint32_t bvh2_depth = 0;  // inner nodes on the longest root path of the caller's BVH2
    // ---- a scene refitted in place (refit(): what trt_update_geometry leaves of a handle created on the scene this was built from)
    const trt_scene* src = nullptr;        // the scene this was built from: topology, materials and lights never change
    std::vector<trt_bvh_node> nodes2;      // the BVH2 of an intermediate step (refit() without a moved scene)
    std::vector<RefitBox> exact8;  // the 8-wide pass's scratch, kept from one refit to the next as the handle keeps it
    bool oct_left = false;                 // an 8-wide node no longer qualified: on the 4-wide nodes for good
    // a reference stack with the bounds the GPU drivers' stacks are sized by: stack_need entries for the 4-wide walk, the BVH2's inner
    // depth for the literal walk (it pushes at most one entry per inner node on its path)
    ArrayStack stack() const
    {
        ArrayStack k;
        k.cap = wide.stack_need;
        k.bvh2_cap = bvh2_depth;
        return k;
    }
    explicit HostScene(const trt_scene* s) : src(s)
    {
        g_breaches = 0;  // every entry that walks rays builds its scene first: a breach is reported by the entry whose walk made it
        {
            struct Ref { uint32_t node, depth; };
            std::vector<Ref> todo;
            if (s->n_nodes) todo.push_back({0u, 1u});
            while (!todo.empty()) {
                const Ref r = todo.back();
                todo.pop_back();
                if (r.depth > bvh2_depth) bvh2_depth = r.depth;
                if (r.node >= s->n_nodes || r.depth > s->n_nodes) continue;  // (trt_create rejects such a tree; the walk's checks report it here)
                for (uint32_t c : {s->nodes[r.node].child0, s->nodes[r.node].child1})
                    if (!(c & TRT_LEAF_BIT)) todo.push_back({c, r.depth + 1u});
            }
        }
        isect.resize(s->n_tris);
        shade.resize(s->n_tris);
        for (uint32_t i = 0; i < s->n_tris; ++i) {
            const int32_t mat = s->tri_mat[i];
            isect[i] = makeTriIsect(s->tri_v + (size_t)i * 9, mat, s->materials[mat].is_emissive != 0);
            std::memcpy(shade[i].vn, s->tri_vn + (size_t)i * 9, 36);
            std::memcpy(shade[i].vt, s->tri_vt + (size_t)i * 6, 24);
            shade[i].mat = mat;
        }
        mats.resize(s->n_materials);
        for (uint32_t i = 0; i < s->n_materials; ++i) mats[i] = makeMaterialDev(s->materials[i]);
        lights.resize(s->n_lights);
        for (uint32_t i = 0; i < s->n_lights; ++i) lights[i] = makeLightDev(s->lights[i], s->materials);
        ltris.resize(s->n_light_tris);
        for (uint32_t i = 0; i < s->n_light_tris; ++i) ltris[i] = makeLightTriDev(s->light_tris[i]);
        tex.resize(s->n_textures);
        for (uint32_t i = 0; i < s->n_textures; ++i) {
            tex[i].width = s->textures[i].width;
            tex[i].height = s->textures[i].height;
            tex[i].offset = tex_bytes.size();
            const size_t nb = (size_t)tex[i].width * tex[i].height * 3;
            tex_bytes.insert(tex_bytes.end(), s->textures[i].rgb, s->textures[i].rgb + nb);
        }
        sc.nodes = s->nodes;
        wide = collapseBvh(s->nodes, s->n_nodes);
        sc.wnodes = wide.nodes.data();
        sc.n_wnodes = (uint32_t)wide.nodes.size();
        if (g_node_kind != 0) oct = buildOct(s->nodes, s->n_nodes, s->n_tris, isect.data());
        sc.onodes = oct.ok ? oct.nodes.data() : nullptr;
        sc.tri_trav = oct.ok ? oct.tri_trav.data() : nullptr;
        sc.n_onodes = (uint32_t)oct.nodes.size();
        leaf_boxes = leafBoxesOf(s->nodes, s->n_nodes, s->n_tris);
        light_boxes = lightBoxesOf(leaf_boxes, s->tri_mat, s->n_tris, s->lights, s->n_lights);
        sc.leaf_box = leaf_boxes.data();
        sc.leaf_alpha = sceneLeafAlpha(s->nodes, s->n_nodes);
        sc.plane_shift = 32u - wide_detail::planeFilterBuild(s->nodes, s->n_nodes, plane_bits);
        sc.plane_bits = plane_bits.data();
        sc.cull_alpha = wide_detail::boxesNested(s->nodes, s->n_nodes) ? sc.leaf_alpha : std::numeric_limits<float>::infinity();  // as trt_create
        nk = (oct.ok && g_node_kind != 0) ? 1 : 0;
        sc.tri_isect = isect.data();
        sc.tri_shade = shade.data();
        sc.materials = mats.data();
        sc.lights = lights.data();
        sc.light_tris = ltris.data();
        bool mono = true;
        for (uint32_t l = 0; l < s->n_lights; ++l)
            for (uint32_t k = 0; k < s->lights[l].tri_count; ++k) {
                const float c = s->light_tris[s->lights[l].tri_first + k].cum_area;
                if (!(c == c) || (k && c < s->light_tris[s->lights[l].tri_first + k - 1].cum_area)) mono = false;
            }
        cum.resize(s->n_light_tris);
        for (uint32_t k = 0; k < s->n_light_tris; ++k) cum[k] = s->light_tris[k].cum_area;
        sc.light_cum = mono ? cum.data() : nullptr;
        sc.textures = tex.data();
        sc.tex_bytes = tex_bytes.data();
        sc.n_tris = s->n_tris;
        sc.n_nodes = s->n_nodes;
        sc.n_lights = s->n_lights;
        sc.light0_area = s->n_lights ? s->lights[0].area : 0.0f;
        sc.cam = s->camera;
    }

    // The handle's state after trt_update_geometry(tri_v), by the per-node functions of trt_refit.h in the loops of tests/refit/refit_loops.h: triangle
    // records, the 4-wide nodes in their own tree, on node kind 1 the triangle records in node order and the 8-wide nodes.  `order` (refitloops::Order)
    // and `keep_light_boxes` plant driver faults for the sensitivity check; 0 / false is the update.  What the BVH2 of the moved scene decides — its
    // nodes, the leaf boxes, the light boxes, the plane filter, leaf_alpha — is taken from `moved` (the scene Scene.set_vertices left for tri_v) when
    // given, else from this scene's own BVH2 refitted by refitNode2 (an intermediate step).  false: an 8-wide node no longer qualified; the scene
    // walks its 4-wide nodes from here on, as the handle does.
    bool refit(const float* tri_v, const trt_scene* moved, int order, bool keep_light_boxes)
    {
        const uint32_t n = src->n_tris;
        if (nk == 1 && exact8.empty()) {  // the scratch as an earlier update in the right order leaves it: a refit to the boxes a tree has reproduces its nodes
            OctTree seed = oct;
            (void)refitloops::refitOctTree(seed, isect.data(), leaf_boxes.data(), exact8, refitloops::DEEPEST_FIRST);
        }
        for (uint32_t i = 0; i < n; ++i) refitTri(i, tri_v, moved ? moved->tri_vn : nullptr, isect.data(), shade.data());
        if (nodes2.empty()) nodes2.assign(src->nodes, src->nodes + src->n_nodes);
        if (moved) leaf_boxes = leafBoxesOf(moved->nodes, moved->n_nodes, n);
        else refitloops::refit2(nodes2, n, tri_v, leaf_boxes);
        const trt_bvh_node* nodes = moved ? moved->nodes : nodes2.data();
        sc.nodes = nodes;
        sc.leaf_box = leaf_boxes.data();
        refitloops::refitWideTree(wide.nodes, leaf_boxes.data(), order);
        bool still_oct = true;
        if (nk == 1) {
            still_oct = refitloops::refitOctTree(oct, isect.data(), leaf_boxes.data(), exact8, order);
            if (!still_oct) { nk = 0; oct_left = true; }
        }
        std::vector<LightBox> lb = lightBoxesOf(leaf_boxes, src->tri_mat, n, src->lights, src->n_lights);
        for (size_t l = 0; keep_light_boxes && l < lb.size(); ++l)
            for (int a = 0; a < 3; ++a) { lb[l].lo[a] = std::fmin(lb[l].lo[a], light_boxes[l].lo[a]); lb[l].hi[a] = std::fmax(lb[l].hi[a], light_boxes[l].hi[a]); }
        light_boxes = lb;
        sc.plane_shift = 32u - wide_detail::planeFilterBuild(nodes, src->n_nodes, plane_bits);
        sc.plane_bits = plane_bits.data();
        sc.leaf_alpha = sceneLeafAlpha(nodes, src->n_nodes);
        if (sc.cull_alpha != std::numeric_limits<float>::infinity()) sc.cull_alpha = sc.leaf_alpha;  // a tree that did not nest when built stays without distance culling
        return still_oct;
    }
};
}  // namespace

// 0 (default, as trt_create): exact wide nodes; 1: compressed nodes where the tree allows them.  Returns the previous setting.
extern "C" int hostsim_set_node_kind(int nk)
{
    const int old = g_node_kind;
    g_node_kind = nk;
    return old;
}
// 1 when `s` can be walked with the compressed 8-wide nodes (nested, finite boxes; leaves of more than 3 triangles are split into slots)
extern "C" int hostsim_compressible(const trt_scene* s)
{
    std::vector<TriIsect> isect(s->n_tris);
    for (uint32_t i = 0; i < s->n_tris; ++i) isect[i] = makeTriIsect(s->tri_v + (size_t)i * 9, s->tri_mat[i], s->materials[s->tri_mat[i]].is_emissive != 0);
    return buildOct(s->nodes, s->n_nodes, s->n_tris, isect.data()).ok ? 1 : 0;
}
// FNV-1a hashes of the trees the collapses build with `threads` host threads: [0] 4-wide (dynamic programme), [1] 4-wide (greedy),
// [2] 8-wide nodes, [3] their triangle records, [4..6] stack need / dropped boxes / levels — the results must not depend on the thread count.
extern "C" int hostsim_tree_hashes(const trt_scene* s, unsigned threads, uint64_t out[8])
{
    auto fnv = [](const void* p, size_t n) {
        uint64_t h = 1469598103934665603ull;
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
        return h;
    };
    std::vector<TriIsect> isect(s->n_tris);
    for (uint32_t i = 0; i < s->n_tris; ++i) isect[i] = makeTriIsect(s->tri_v + (size_t)i * 9, s->tri_mat[i], s->materials[s->tri_mat[i]].is_emissive != 0);
    const WideTree a = collapseBvh(s->nodes, s->n_nodes, threads), b = collapseBvhGreedy(s->nodes, s->n_nodes, threads);
    const OctTree t = buildOct(s->nodes, s->n_nodes, s->n_tris, isect.data(), threads);
    const std::vector<f4> lb = leafBoxesOf(s->nodes, s->n_nodes, s->n_tris, threads);
    out[0] = fnv(a.nodes.data(), a.nodes.size() * sizeof(WideNode));
    out[1] = fnv(b.nodes.data(), b.nodes.size() * sizeof(WideNode));
    out[2] = t.ok ? fnv(t.nodes.data(), t.nodes.size() * sizeof(OctNode)) : 0;
    out[3] = t.ok ? fnv(t.tri_trav.data(), t.tri_trav.size() * sizeof(TriIsect)) : 0;
    out[4] = ((uint64_t)a.stack_need << 32) | b.stack_need;
    out[5] = a.dropped * 1000003ull + b.dropped;
    out[6] = t.levels;
    out[7] = fnv(lb.data(), lb.size() * sizeof(f4));
    return 0;
}
// nodes / levels of the oct tree (0 when it cannot be built)
extern "C" int hostsim_oct_info(const trt_scene* s, uint64_t out[3])
{
    std::vector<TriIsect> isect(s->n_tris);
    for (uint32_t i = 0; i < s->n_tris; ++i) isect[i] = makeTriIsect(s->tri_v + (size_t)i * 9, s->tri_mat[i], s->materials[s->tri_mat[i]].is_emissive != 0);
    const OctTree t = buildOct(s->nodes, s->n_nodes, s->n_tris, isect.data());
    out[0] = t.ok ? t.nodes.size() : 0; out[1] = t.levels; out[2] = t.tri_trav.size();
    return t.ok ? 0 : 1;
}

extern "C" int hostsim_render(const trt_scene* s, const trt_params* p, float* out_rgb, uint64_t rays[3])
{
    if (!s || !p || !out_rgb) return 1;
    HostScene hs(s);
    std::vector<int32_t> rows;
    for (int y = p->y0; y < p->y1; ++y)
        if (p->row_mod <= 1 || ((y / p->row_block) % p->row_mod) == p->row_rem) rows.push_back(y);
    const uint32_t tw = (uint32_t)(p->x1 - p->x0), npix = (uint32_t)rows.size() * tw;
    TileDesc td;
    td.rows = rows.data();
    td.tile_w = (int32_t)tw; td.x0 = p->x0; td.width = p->width; td.height = p->height;
    td.npix = npix; td.seed = p->seed; td.spp = (uint32_t)p->spp;
    td.fixed_nee = (p->flags & TRT_FLAG_FIXED_NEE) ? 1u : 0u;
    td.fixed_pixels = (p->flags & TRT_FLAG_FIXED_PIXELS) ? 1u : 0u;
    td.ray_offset = (p->flags & TRT_FLAG_RAY_OFFSET) ? 1u : 0u;
    td.specular_ks = (p->flags & TRT_FLAG_SPECULAR_KS) ? 1u : 0u;
    td.npix_magic = magicOf(npix); td.tile_w_magic = magicOf(tw);
    td.grid_ok = 0u;  // the host form of cameraRay divides
    for (double& g : td.grid_rcp) g = 0.0;
    uint64_t r_cam = 0, r_sh = 0, r_ind = 0;
    const uint32_t S = (uint32_t)p->spp;  // one chunk: path id = s * npix + pixel
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : r_cam, r_sh, r_ind)
    for (long pl = 0; pl < (long)npix; ++pl) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        double acc[3] = {0, 0, 0};
        for (uint32_t sidx = 0; sidx < S; ++sidx) {
            const uint32_t pid = sidx * npix + (uint32_t)pl;
            // k_gen_primary
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
                // k_trace_closest
                const Hit h = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), ostk, stk, ni, nt)
                                    : traceClosest<ArrayStack, false, 0>(hs.sc, mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), stk, ni, nt);
                const f4 hit4 = mk4(h.t, u2f((uint32_t)h.tri), h.u, h.v);
                // k_shade
                ShadeCtx cx;
                shadeBegin(hs.sc, td, 0, ra, rb, bt, hit4, cx);
                if (cx.add_L) L = L + cx.addL;
                for (uint32_t li = 0; li < hs.sc.n_lights; ++li) {
                    f3 wo, contrib;
                    const bool fixed = td.fixed_nee != 0u;
                    float t_max = TRT_INF;
                    if (!cx.shade_ok || !lightSample(hs.sc, cx.vx, *cx.m, li, cx.rng, wo, contrib, fixed, t_max)) continue;
                    const f3 w = cx.beta * contrib;
                    r_sh++;
                    if (g_shadow_rec && !fixed) {
                        const uint64_t k = g_shadow_rec->n.fetch_add(1);
                        if (k < g_shadow_rec->cap) {
                            const f3 so = rayOrigin(cx, wo);
                            const float o3[3] = {so.x, so.y, so.z}, d3[3] = {wo.x, wo.y, wo.z};
                            std::memcpy(g_shadow_rec->org + k * 3, o3, 12);
                            std::memcpy(g_shadow_rec->dir + k * 3, d3, 12);
                            g_shadow_rec->light[k] = (int32_t)li;
                        }
                    }
                    // k_trace_shadow
                    const Hit sh = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, rayOrigin(cx, wo), wo, ostk, stk, ni, nt, t_max, fixed, !fixed, &hs.light_boxes[li])
                                         : traceClosest<ArrayStack, false, 0>(hs.sc, rayOrigin(cx, wo), wo, stk, ni, nt, t_max, fixed, !fixed);
                    if (fixed ? sh.tri < 0 : (sh.tri >= 0 && (sh.flags >> 8) == (uint32_t)hs.sc.lights[li].mat)) L = L + w;
                }
                f4 nra, nrb, nbt;
                if (!shadeNext(cx, p->max_depth, nra, nrb, nbt)) break;
                ra = nra; rb = nrb; bt = nbt;
                r_ind++;
            }
            // k_resolve
            const float spp = (float)p->spp;
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

extern "C" int hostsim_trace(const trt_scene* s, uint64_t n, const float* org, const float* dir, float* t, int32_t* tri, float* uv, uint64_t counts[2])
{
    if (!s || !org || !dir || !t || !tri) return 1;
    HostScene hs(s);
    uint64_t ci = 0, ct = 0;
#pragma omp parallel for schedule(static) reduction(+ : ci, ct)
    for (long long i = 0; i < (long long)n; ++i) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        const Hit h = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, true>(hs.sc, ld3(org + i * 3), ld3(dir + i * 3), ostk, stk, ni, nt)
                            : traceClosest<ArrayStack, true, 0>(hs.sc, ld3(org + i * 3), ld3(dir + i * 3), stk, ni, nt);
        t[i] = h.t;
        tri[i] = h.tri;
        if (uv) { uv[i * 2] = h.u; uv[i * 2 + 1] = h.v; }
        ci += ni;
        ct += nt;
    }
    if (counts) { counts[0] = ci; counts[1] = ct; }
    return g_breaches.exchange(0) ? 2 : 0;
}

// The ray queries on the device code, per ray with bound[i] (null: none) as the search's t_init:
//   form 0 — what the per-lane drivers run (k_trace_closest / k_trace_query): traceClosest, or traceClosestOct where the node kind is 1;
//   form 1 — what k_trace_fix runs on the rays of a redo list: the literal walk for rays of raySpecial() whose origin may lie on a box plane,
//            else the exact form (RULE) on the 4-wide nodes.
// `any`: the occlusion query (stop at the first hit nearer than the bound).  Without `any` a hit at or beyond the bound is a miss: the literal
// walk ignores the bound in closest mode, and k_trace_fix clips its result so for QUERY_CLOSEST (the per-lane drivers hand every ray of raySpecial()
// to k_trace_fix).  A miss is (TRT_INF, -1, 0, 0), as storeResult writes it.  Returns 2 when a walk was ended by TRT_WALK_CHECK.
extern "C" int hostsim_query(const trt_scene* s, int form, int any, uint64_t n, const float* org, const float* dir, const float* bound, float* t, int32_t* tri, float* uv)
{
    if (!s || !org || !dir || !t || !tri || form < 0 || form > 1) return 1;
    HostScene hs(s);
#pragma omp parallel for schedule(dynamic, 256)
    for (long long i = 0; i < (long long)n; ++i) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3), inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        const float t_init = bound ? bound[i] : TRT_INF;
        Hit h;
        if (form == 0)
            h = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, o, d, ostk, stk, ni, nt, t_init, any != 0)
                      : traceClosest<ArrayStack, false, 0>(hs.sc, o, d, stk, ni, nt, t_init, any != 0);
        else
            h = (raySpecial(inv) && rayOnABoxPlane(hs.sc, o, inv)) ? traceClosestBvh2Glm<ArrayStack, false>(hs.sc, o, d, stk, ni, nt, t_init, any != 0)
                                                                    : traceClosestPass<ArrayStack, false, 0, true>(hs.sc, o, d, stk, ni, nt, t_init, any != 0);
        if (!any && !(h.t < t_init)) h.tri = -1;
        const bool hit = h.tri >= 0;
        t[i] = hit ? h.t : TRT_INF;
        tri[i] = hit ? h.tri : -1;
        if (uv) { uv[i * 2] = hit ? h.u : 0.0f; uv[i * 2 + 1] = hit ? h.v : 0.0f; }
    }
    return g_breaches.exchange(0) ? 2 : 0;
}

// how many of the rays take the exact form behind the oct traversal (its result failed octResultCounts): tests/test_hostsim_parity.py
extern "C" uint64_t hostsim_oct_fallbacks(const trt_scene* s, uint64_t n, const float* org, const float* dir)
{
    const int old = g_node_kind;
    g_node_kind = 1;
    HostScene hs(s);
    g_node_kind = old;
    if (!hs.nk) return ~0ull;
    uint64_t bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; ++i) {
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3);
        const Hit h = traceOctPass<OctArrayStack, false>(hs.sc, o, d, ostk, ni, nt, TRT_INF, false, false);
        bad += octResultCounts(hs.sc, h.t, h.tri, o, mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z)) ? 0u : 1u;
    }
    return bad;
}

// per-ray work of the closest-hit search on either node kind: visits[i], tests[i] (tools / tests: where do the long traversals come from?)
extern "C" int hostsim_trace_counts(const trt_scene* s, int nk, uint64_t n, const float* org, const float* dir, uint32_t* visits, uint32_t* tests)
{
    const int old = g_node_kind;
    g_node_kind = nk;
    HostScene hs(s);
    g_node_kind = old;
    if (nk && !hs.nk) return 1;
#pragma omp parallel for schedule(dynamic, 256)
    for (long long i = 0; i < (long long)n; ++i) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3);
        if (hs.nk) (void)traceOctPass<OctArrayStack, true>(hs.sc, o, d, ostk, ni, nt, TRT_INF, false, false);
        else (void)traceClosestPass<ArrayStack, true, 0, false>(hs.sc, o, d, stk, ni, nt);
        visits[i] = ni;
        tests[i] = nt;
    }
    return g_breaches.exchange(0) ? 2 : 0;
}

// ---- a handle created on scene `before` and updated to tris[0], .., tris[k - 1] in turn (tests/test_refit_work_cpu.py, tests/test_gpu_refit_work.py): the records and
// the per-ray work of its ray queries, for the counters of TRT_FLAG_COUNT.  `after` = the scene Scene.set_vertices left for tris[k - 1] (ignored when k = 0).
// nk: the node kind the handle was created on.  any: the occlusion query.  bound (may be null): per-ray t_init.  light >= 0 (node kind 1, closest): the rays are
// walked as the parity-mode shadow rays of that light (its light box ends them early, the bound is a hint).  order / keep_light_boxes: see HostScene::refit.
// Records: as hostsim_query form 0.  visits[i] / tests[i]: the first pass of the per-lane search (hostsim_trace_counts' numbers: traceClosestPass / traceOctPass),
// 0 for a ray of raySpecial() — the drivers hand those to k_trace_fix, which does not count.
// Returns 0; 1: bad arguments, or node kind 1 asked of a tree that does not qualify; 2: TRT_WALK_CHECK; 3: an 8-wide node no longer qualified during an update and
// go_on = 0.  With go_on the walk continues on node kind 0, as the handle does; *walked_kind (may be null) = the node kind the rays were walked on.
extern "C" int hostsim_refit_trace_counts(const trt_scene* before, uint32_t k, const float* const* tris, const trt_scene* after, int nk, int any, int go_on, int order,
                                          int keep_light_boxes, int light, uint64_t n, const float* org, const float* dir, const float* bound, float* t, int32_t* tri,
                                          float* uv, uint32_t* visits, uint32_t* tests, int32_t* walked_kind)
{
    if (!before || (k && (!tris || !after)) || !org || !dir || !t || !tri || !visits || !tests) return 1;
    if (k && (after->n_tris != before->n_tris || after->n_nodes != before->n_nodes)) return 1;
    const int old = g_node_kind;
    g_node_kind = nk;
    HostScene hs(before);
    g_node_kind = old;
    if (nk && !hs.nk) return 1;
    for (uint32_t j = 0; j < k; ++j) (void)hs.refit(tris[j], j + 1 == k ? after : nullptr, order, keep_light_boxes != 0);
    if (hs.oct_left && !go_on) return 3;
    if (walked_kind) *walked_kind = hs.nk;
    const LightBox* lbox = (light >= 0 && (size_t)light < hs.light_boxes.size() && hs.nk && !any) ? &hs.light_boxes[(size_t)light] : nullptr;
    const bool redo = lbox != nullptr;
#pragma omp parallel for schedule(dynamic, 256)
    for (long long i = 0; i < (long long)n; ++i) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0, ci = 0, ct = 0;
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3);
        const float t_init = bound ? bound[i] : TRT_INF;
        Hit h = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, o, d, ostk, stk, ni, nt, t_init, any != 0, redo, lbox)
                      : traceClosest<ArrayStack, false, 0>(hs.sc, o, d, stk, ni, nt, t_init, any != 0);
        if (!any && !redo && !(h.t < t_init)) h.tri = -1;
        const bool hit = h.tri >= 0;
        t[i] = hit ? h.t : TRT_INF;
        tri[i] = hit ? h.tri : -1;
        if (uv) { uv[i * 2] = hit ? h.u : 0.0f; uv[i * 2 + 1] = hit ? h.v : 0.0f; }
        if (!raySpecial(mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z))) {
            if (hs.nk) (void)traceOctPass<OctArrayStack, true>(hs.sc, o, d, ostk, ci, ct, t_init, any != 0, redo, lbox);
            else (void)traceClosestPass<ArrayStack, true, 0, false>(hs.sc, o, d, stk, ci, ct, t_init, any != 0);
        }
        visits[i] = ci;
        tests[i] = ct;
    }
    return g_breaches.exchange(0) ? 2 : 0;
}

// The sequence of steps the wave driver takes for one ray on the oct nodes (tools/pool_sim.py: what would grouping rays by phase across the waves
// of a block buy?): per ray up to `cap` bytes, 0 = a node step, k = 1..2 = a leaf step that tests k triangles (the driver tests up to two of
// the lane's group per leaf step).  The loop is traceOctPass's (trt_oct.h) with a tape; `t_init` / `redo` / `light` as for a parity-mode shadow ray
// (light < 0: a closest-hit ray).
extern "C" int hostsim_oct_step_tape_chunk(const trt_scene* s, uint64_t n, const float* org, const float* dir, const float* t_init, int light, uint32_t cap, uint8_t* tape, uint32_t* len, uint32_t per_leaf_step)
{
    const int old = g_node_kind;
    g_node_kind = 1;
    HostScene hs(s);
    g_node_kind = old;
    if (!hs.nk) return 1;
    const LightBox* lbox = light >= 0 && (uint32_t)light < hs.light_boxes.size() ? &hs.light_boxes[(size_t)light] : nullptr;
#pragma omp parallel for schedule(dynamic, 256)
    for (long long i = 0; i < (long long)n; ++i) {
        OctArrayStack stk;
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3);
        uint8_t* out = tape + (size_t)i * cap;
        uint32_t m = 0;
        auto put = [&](uint8_t v) { if (m < cap) out[m] = v; ++m; };
        const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        const OctRay R = makeOctRay(o, d, inv);
        float best_t = t_init ? t_init[i] : TRT_INF, stop_t = -TRT_INF;
        int32_t best_tri = -1;
        uint32_t best_flags = 0u;
        bool skip = false;
        if (lbox) {
            float e;
            if (!boxTest(lbox->lo[0], lbox->lo[1], lbox->lo[2], lbox->hi[0], lbox->hi[1], lbox->hi[2], o, inv, e)) skip = true;
            stop_t = trt_leaf_floor(e, hs.sc.leaf_alpha);
        }
        for (int pass = 0; pass < 2 && !skip; ++pass) {
            int sp = 0;
            OctGroup ng, tg;
            ng.x = 0u; ng.y = 0x80000000u;
            tg.x = 0u; tg.y = 0u;
            bool stop = false;
            for (;;) {
                if (ng.y & 0xFF000000u) {
                    const uint32_t ni = octNextChild(ng, R);
                    if (ng.y & 0xFF000000u) stk.push(sp++, ng);
                    put(0);
                    octVisit(hs.sc.onodes, ni, R, trt_cull_bound(best_t, hs.sc.leaf_alpha), ng, tg);
                }
                uint32_t in_step = 0;
                while (tg.y) {
                    const uint32_t b = (uint32_t)__builtin_ctz(tg.y);
                    tg.y &= tg.y - 1u;
                    const TriIsect T = hs.sc.tri_trav[tg.x + b];
                    float t, un, vn, det;
                    if (triTest(T, o, d, t, un, vn, det)) octFold(t, f2u(T.c.w), f2u(T.c.z), best_t, best_tri, best_flags);
                    if (++in_step == per_leaf_step || !tg.y) { put((uint8_t)in_step); in_step = 0; }
                    if (lbox && best_tri >= 0 && best_t < stop_t && in_step == 0u) { tg.y = 0u; stop = true; }
                }
                if (stop) break;
                if (!(ng.y & 0xFF000000u)) {
                    if (sp == 0) break;
                    ng = stk.pop(--sp);
                }
            }
            if (stop || !t_init || best_tri >= 0 || !(best_t < TRT_INF)) break;
            best_t = TRT_INF;  // nothing in front of the hint: search again without it
        }
        len[i] = m;
    }
    return 0;
}

extern "C" int hostsim_oct_step_tape(const trt_scene* s, uint64_t n, const float* org, const float* dir, const float* t_init, int light, uint32_t cap, uint8_t* tape, uint32_t* len)
{
    return hostsim_oct_step_tape_chunk(s, n, org, dir, t_init, light, cap, tape, len, 2u);  // TRT_OCT_LEAF_LOOP
}

// divMagic(n, d, magicOf(d)) against n / d for a list of numerators: returns the number of mismatches (tests/test_hostsim_parity.py)
extern "C" uint64_t hostsim_div_magic_mismatches(uint32_t d, const uint32_t* n, uint64_t count)
{
    const uint32_t m = magicOf(d);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i) bad += divMagic(n[i], d, m) != n[i] / d ? 1u : 0u;
    return bad;
}

// ---- node by node: the decisions behind the results (tests/test_hostsim_node_claims.py; tests/test_gpu_node_claims.py compares the words of
// tools/node_visit_check.hip, the same functions as gfx950 compiles them, with what these entries return).  The entries work on arrays the test owns
// (nodes, boxes, filter words), so a negative control is a changed copy of the data, never a switch in the headers.
namespace {
inline uint32_t canonBits(float f) { return f != f ? 0x7FC00000u : f2u(f); }  // one NaN: the payload of a NaN is not part of any claim
inline f3 invOf(f3 d) { return mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); }

}  // namespace

// Synthetic 8-wide nodes straight from octQuantise.  kind[i][slot]: 0 empty, 1 an inner child, 2..4 a leaf slot of 1..3 triangles (offsets in slot order).
// ok[i] = 0 where the extent is not representable (the node is left zeroed).
extern "C" int hostsim_oct_quantise_nodes(uint64_t n, const float* blo, const float* bhi, const uint8_t* kind, OctNode* out, uint8_t* ok)
{
    for (uint64_t i = 0; i < n; ++i) {
        float lo[8][3], hi[8][3], p[3];
        uint32_t mask = 0u, imask = 0u, eb[3], qlo[3][8], qhi[3][8], meta[8], off = 0u;
        for (int sl = 0; sl < 8; ++sl) {
            for (int a = 0; a < 3; ++a) { lo[sl][a] = blo[(i * 8 + sl) * 3 + a]; hi[sl][a] = bhi[(i * 8 + sl) * 3 + a]; }
            const uint32_t k = kind[i * 8 + sl];
            meta[sl] = 0u;
            if (!k) continue;
            mask |= 1u << sl;
            if (k == 1u) { imask |= 1u << sl; meta[sl] = 0x20u | (24u + (uint32_t)sl); }
            else { const uint32_t c = k - 1u; meta[sl] = (((1u << c) - 1u) << 5) | off; off += c; }
        }
        std::memset(&out[i], 0, sizeof(OctNode));
        ok[i] = (mask && octQuantise(lo, hi, mask, p, eb, qlo, qhi)) ? 1 : 0;
        if (!ok[i]) continue;
        out[i].q[0] = mk4(p[0], p[1], p[2], u2f(eb[0] | (eb[1] << 8) | (eb[2] << 16) | (imask << 24)));
        out[i].q[1] = mk4(u2f(0u), u2f(0u), u2f(octPack4(meta)), u2f(octPack4(meta + 4)));
        octStoreBounds(out[i], qlo, qhi);
    }
    return 0;
}

// octVisit per (node, ray, cull): words[2 i] = the node group's hit word (bits 24..31 by octant-permuted slot | imask), words[2 i + 1] = the triangle bits
extern "C" int hostsim_oct_visit_cases(const OctNode* nodes, uint64_t n, const uint32_t* node, const float* org, const float* dir, const float* cull, uint32_t* words)
{
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; ++i) {
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3);
        const OctRay R = makeOctRay(o, d, invOf(d));
        OctGroup ng, tg;
        octVisit(nodes, node[i], R, cull[i], ng, tg);
        words[2 * i] = ng.y;
        words[2 * i + 1] = tg.y;
    }
    return 0;
}

// the reference's test (boxTest) of the EXACT box of each of the eight slots of node[i] (slot_box[node][slot] = lo.xyz, hi.xyz: what octQuantise was fed)
extern "C" int hostsim_slot_ref(const float* slot_box, uint64_t n, const uint32_t* node, const float* org, const float* dir, uint8_t* pass, float* entry)
{
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; ++i) {
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3), inv = invOf(d);
        for (int sl = 0; sl < 8; ++sl) {
            const float* b = slot_box + ((size_t)node[i] * 8 + sl) * 6;
            float e;
            pass[i * 8 + sl] = boxTest(b[0], b[1], b[2], b[3], b[4], b[5], o, inv, e) ? 1 : 0;
            entry[i * 8 + sl] = e;
        }
    }
    return 0;
}

// The nodes of an oct tree the REFERENCE's descent reaches: from the root, into an inner slot iff boxTest passes the slot's exact box.  Per ray up to
// `cap` node indices in pair_node[ray][..], count[ray] = how many were reached (more than cap: the rest are dropped).  Rays of raySpecial() reach none:
// traceClosestOct does not send them to these nodes.
extern "C" int hostsim_oct_descent(const OctNode* nodes, const float* slot_box, uint32_t n_nodes, uint64_t n, const float* org, const float* dir, uint32_t cap,
                                   uint32_t* pair_node, uint32_t* count)
{
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(| : bad)
    for (long long i = 0; i < (long long)n; ++i) {
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3), inv = invOf(d);
        uint32_t m = 0;
        std::vector<uint32_t> todo;
        if (!raySpecial(inv) && n_nodes) todo.push_back(0u);
        while (!todo.empty()) {
            const uint32_t ni = todo.back();
            todo.pop_back();
            if (ni >= n_nodes || m > 4u * n_nodes) { bad = 1; break; }
            if (m < cap) pair_node[(size_t)i * cap + m] = ni;
            ++m;
            for (int sl = 0; sl < 8; ++sl) {
                const uint32_t mt = octMeta(nodes[ni], sl);
                if (!mt || !octMetaInner(mt)) continue;
                const float* b = slot_box + ((size_t)ni * 8 + sl) * 6;
                float e;
                if (boxTest(b[0], b[1], b[2], b[3], b[4], b[5], o, inv, e)) todo.push_back(octChildIndex(nodes[ni], sl));
            }
        }
        count[i] = m;
    }
    return bad;
}

// boxTest and boxTestGlm per (box, ray): out[3 i] = verdicts (bit 0 boxTest, bit 1 boxTestGlm), out[3 i + 1] / [3 i + 2] = the bits of their entries
extern "C" int hostsim_box_cases(uint64_t n, const float* box, const float* org, const float* dir, uint32_t* out)
{
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; ++i) {
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3), inv = invOf(d);
        const float* b = box + i * 6;
        float e0, e1;
        const bool p0 = boxTest(b[0], b[1], b[2], b[3], b[4], b[5], o, inv, e0), p1 = boxTestGlm(b[0], b[1], b[2], b[3], b[4], b[5], o, inv, e1);
        out[3 * i] = (p0 ? 1u : 0u) | (p1 ? 2u : 0u);
        out[3 * i + 1] = canonBits(e0);
        out[3 * i + 2] = canonBits(e1);
    }
    return 0;
}

// innerStep on 4-wide node node[i] with an empty private stack: out[6 i ..] = cur, the returned flag, entries pushed, the pushed references in order
extern "C" int hostsim_inner_step_cases(const WideNode* wnodes, uint64_t n, const uint32_t* node, const float* org, const float* dir, const float* cull, uint32_t* out)
{
    SceneDev sc{};
    sc.wnodes = wnodes;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; ++i) {
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3);
        ArrayStack stk;
        stk.s[0] = stk.s[1] = stk.s[2] = 0u;
        uint32_t cur = node[i];
        int sp = 0;
        const bool go = innerStep(sc, cur, sp, stk, o, invOf(d), cull[i]);
        out[6 * i] = cur; out[6 * i + 1] = go ? 1u : 0u; out[6 * i + 2] = (uint32_t)sp;
        out[6 * i + 3] = stk.s[0]; out[6 * i + 4] = stk.s[1]; out[6 * i + 5] = stk.s[2];
    }
    return 0;
}

// trt_leaf_floor / trt_cull_bound element by element
extern "C" void hostsim_leaf_floor_v(uint64_t n, const float* e, const float* alpha, float* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = trt_leaf_floor(e[i], alpha[i]);
}
extern "C" void hostsim_cull_bound_v(uint64_t n, const float* b, const float* alpha, float* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = trt_cull_bound(b[i], alpha[i]);
}

// what a handle derives from the tree: info[0] = leaf_alpha, info[1] = 1 when the boxes nest; light_box[l][6] (may be null)
extern "C" int hostsim_scene_info(const trt_scene* s, float info[2], float* light_box)
{
    HostScene hs(s);
    info[0] = hs.sc.leaf_alpha;
    info[1] = wide_detail::boxesNested(s->nodes, s->n_nodes) ? 1.0f : 0.0f;
    for (size_t l = 0; light_box && l < hs.light_boxes.size(); ++l)
        for (int a = 0; a < 3; ++a) { light_box[l * 6 + a] = hs.light_boxes[l].lo[a]; light_box[l * 6 + 3 + a] = hs.light_boxes[l].hi[a]; }
    return 0;
}

// The culling chain on results: for the hit (t[i], tri[i]) of ray i every box on tri's root path, in the caller's BVH2 (tree 2) and in its 4-wide collapse
// (tree 4), root first: (0) boxTest passes, (1) the entry is not below the one above it, (2) NOT t < trt_leaf_floor(entry), (3) NOT entry >
// trt_cull_bound(t).  Rays traceClosest does not walk with culling (a zero direction
// component AND an origin the plane filter cannot clear) and misses are left out.  counts: [0] rays checked, [1] boxes checked, [2 + k] violations of (k);
// viol[j][8] = kind, tree, node, slot, ray, entry, t, bound of the first 16.  3: the boxes do not nest (nothing is claimed for such a tree).
extern "C" int hostsim_cull_chain(const trt_scene* s, uint64_t n, const float* org, const float* dir, const float* t, const int32_t* tri, uint64_t counts[6],
                                  double* viol)
{
    HostScene hs(s);
    for (int k = 0; k < 6; ++k) counts[k] = 0;
    if (!wide_detail::boxesNested(s->nodes, s->n_nodes)) return 3;
    struct Up { uint32_t node, slot; };
    const Up none{~0u, 0u};
    // tree 2: where each node hangs, which child box holds each triangle
    std::vector<Up> up2(s->n_nodes, none), leaf2(s->n_tris, none), upw(hs.wide.nodes.size(), none), leafw(s->n_tris, none);
    for (uint32_t i = 0; i < s->n_nodes; ++i)
        for (uint32_t k = 0; k < 2; ++k) {
            const uint32_t ref = k ? s->nodes[i].child1 : s->nodes[i].child0;
            if (!(ref & TRT_LEAF_BIT)) { if (ref < s->n_nodes) up2[ref] = Up{i, k}; continue; }
            for (uint32_t j = 0; j < TRT_LEAF_COUNT(ref); ++j)
                if (TRT_LEAF_FIRST(ref) + j < s->n_tris) leaf2[TRT_LEAF_FIRST(ref) + j] = Up{i, k};
        }
    for (uint32_t i = 0; i < hs.wide.nodes.size(); ++i)
        for (uint32_t k = 0; k < TRT_WIDE; ++k) {
            const uint32_t ref = f2u((&hs.wide.nodes[i].q[6].x)[k]);
            if (ref == TRT_WIDE_EMPTY) continue;
            if (!(ref & TRT_LEAF_BIT)) { if (ref < hs.wide.nodes.size()) upw[ref] = Up{i, k}; continue; }
            for (uint32_t j = 0; j < TRT_LEAF_COUNT(ref); ++j)
                if (TRT_LEAF_FIRST(ref) + j < s->n_tris) leafw[TRT_LEAF_FIRST(ref) + j] = Up{i, k};
        }
    const float alpha = hs.sc.leaf_alpha;
    uint64_t n_viol = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const f3 o = ld3(org + i * 3), d = ld3(dir + i * 3), inv = invOf(d);
        if (tri[i] < 0 || (uint32_t)tri[i] >= s->n_tris || (raySpecial(inv) && rayOnABoxPlane(hs.sc, o, inv))) continue;
        counts[0]++;
        const float bound = trt_cull_bound(t[i], alpha);
        for (int tree = 2; tree <= 4; tree += 2) {
            std::vector<Up> path;
            for (Up u = (tree == 2 ? leaf2 : leafw)[(size_t)tri[i]]; u.node != ~0u && path.size() <= s->n_nodes; u = (tree == 2 ? up2 : upw)[u.node]) {
                path.push_back(u);
                if (u.node == 0u) break;
            }
            float above = -__builtin_inff();
            for (size_t k = path.size(); k-- > 0;) {
                const Up u = path[k];
                float lo[3], hi[3], e;
                if (tree == 2) {
                    const trt_bvh_node& nd = s->nodes[u.node];
                    for (int a = 0; a < 3; ++a) { lo[a] = u.slot ? nd.lo1[a] : nd.lo0[a]; hi[a] = u.slot ? nd.hi1[a] : nd.hi0[a]; }
                } else {
                    const f4* q = hs.wide.nodes[u.node].q;
                    for (int a = 0; a < 3; ++a) { lo[a] = (&q[a].x)[u.slot]; hi[a] = (&q[3 + a].x)[u.slot]; }
                }
                const bool pass = boxTest(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], o, inv, e);
                const bool bad[4] = {!pass, e < above, t[i] < trt_leaf_floor(e, alpha), e > bound};
                counts[1]++;
                for (int c = 0; c < 4; ++c) {
                    if (!bad[c]) continue;
                    counts[2 + c]++;
                    if (n_viol < 16 && viol) {
                        const double row[8] = {(double)c, (double)tree, (double)u.node, (double)u.slot, (double)i, (double)e, (double)t[i], (double)bound};
                        std::memcpy(viol + n_viol * 8, row, sizeof row);
                    }
                    n_viol++;
                }
                above = e;
            }
        }
    }
    return 0;
}

// the parity-mode shadow rays of a render (origin, direction, the light each was drawn for), up to cap; returns how many there were (or ~0 on an error)
extern "C" uint64_t hostsim_shadow_rays(const trt_scene* s, const trt_params* p, uint64_t cap, float* org, float* dir, int32_t* light)
{
    ShadowRec rec;
    rec.cap = cap; rec.org = org; rec.dir = dir; rec.light = light;
    std::vector<float> img((size_t)p->width * p->height * 3);
    g_shadow_rec = &rec;
    const int rc = hostsim_render(s, p, img.data(), nullptr);
    g_shadow_rec = nullptr;
    return rc ? ~0ull : rec.n.load();
}

// the plane filter a handle builds over the tree of `s`: the words (up to cap_words) and log2 of its bits (0: cap_words is too small)
extern "C" uint32_t hostsim_plane_filter(const trt_scene* s, uint32_t* bits, uint64_t cap_words)
{
    std::vector<uint32_t> b;
    const uint32_t lg = wide_detail::planeFilterBuild(s->nodes, s->n_nodes, b);
    if (b.size() > cap_words) return 0u;
    std::memcpy(bits, b.data(), b.size() * 4);
    return lg;
}
// planeMaybe(axis[i], x[i]) on a filter of 2^lg bits
extern "C" void hostsim_plane_maybe(const uint32_t* bits, uint32_t lg, uint64_t n, const int32_t* axis, const float* x, uint8_t* out)
{
    SceneDev sc{};
    sc.plane_bits = bits;
    sc.plane_shift = 32u - lg;
    for (uint64_t i = 0; i < n; ++i) out[i] = planeMaybe(sc, axis[i], x[i]) ? 1 : 0;
}

// ---- case by case: the shading functions and the primitives under them (tests/test_shade_cases_cpu.py; tests/test_gpu_shade_cases.py compares the words of
// tools/shade_case_check.hip, the same functions as gfx950 compiles them, with what these entries return).  The section functions are the tool's own.
#include "shade_cases_host.h"

// the words of a whole case file (layout: tools/shade_cases.h), in the tool's order; 2 for a file the tool would refuse
extern "C" int hostsim_shade_case_file(const uint8_t* buf, uint64_t size, uint32_t* out, uint64_t n_words)
{
    return shadecases::runFileHost<shadecases::HeaderFns>(buf, size, out, n_words);
}
// digests first .. first + n - 1 of the tool's modes digest (digestAt) and, behind those, digest-pickers (pickerDigestAt)
extern "C" int hostsim_shade_digests(uint32_t first, uint64_t n, uint64_t* out)
{
    const uint32_t fns = shadecases::digestTotal();
    if ((uint64_t)first + n > (uint64_t)fns + shadecases::pickerDigestTotal()) return 2;
    std::vector<shadecases::DigestPools> pools(1);
    shadecases::digestPoolsFill(pools[0]);
#pragma omp parallel for schedule(dynamic, 64)
    for (long long i = 0; i < (long long)n; ++i) {
        const uint32_t k = first + (uint32_t)i;
        out[i] = k < fns ? shadecases::digestAt(k) : shadecases::pickerDigestAt(pools[0], k - fns);
    }
    return 0;
}
// the table records a handle forms from the caller's (makeMaterialDev)
extern "C" int hostsim_make_material_dev(uint64_t n, const trt_material* m, MaterialDev* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = makeMaterialDev(m[i]);
    return 0;
}
