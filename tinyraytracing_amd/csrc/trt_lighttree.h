// trt_lighttree.h — the host build of the light tree of TRT_FLAG_NEAR_LIGHTS (include/trt.h states the contract; lightPickNear, trt_path.h, descends it).
// One function, buildLightTree, for trt_create, the geometry update and the CPU build of the tests: deterministic, fp32 where the contract says fp32.
//
//   tree lights   the lights with lightWeight() > 0, tri_count > 0, a triangle range inside the table and only finite vertices; M of them, in index order
//   box, centre   the exact min / max over the vertices of the light's triangles; centre = 0.5f * lo + 0.5f * hi per axis
//   split         a list of n >= 2 lights: the axis of the largest extent of the centres' bounds (ties: x, then y, then z), a stable sort by
//                 centre[axis], the first n / 2 lights to the left child, the rest to the right; a list of one light is a leaf
//   numbering     pre-order: a node, its left subtree, its right subtree; M - 1 nodes, depth <= ceil(log2 M) <= 16
//   node          the two children's boxes, weights (the fp32 sum of their lights' weights in the child's list order) and references
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "trt_path.h"

namespace trtd {

struct LightTree {
    std::vector<LightNode> nodes;  // M - 1 for M >= 2, else empty
    uint32_t root = TRT_LIGHT_NONE;  // SceneDev::light_root
    uint32_t n_tree_lights = 0;      // M
};

namespace lighttree {
struct Leaf {
    uint32_t index;
    float lo[3], hi[3], c[3], w;
};
// box and weight of list[first, first + n) in list order -> the slot of a node
inline void summarise(const Leaf* list, uint32_t n, float* lo, float* hi, float& w)
{
    w = 0.0f;
    for (int a = 0; a < 3; ++a) { lo[a] = list[0].lo[a]; hi[a] = list[0].hi[a]; }
    for (uint32_t k = 0; k < n; ++k) {
        w = w + list[k].w;
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], list[k].lo[a]); hi[a] = fmaxf(hi[a], list[k].hi[a]); }
    }
}
// the node of list[0, n), n >= 2 -> its index; the list is sorted in place
inline uint32_t split(Leaf* list, uint32_t n, std::vector<LightNode>& nodes)
{
    float clo[3], chi[3];
    for (int a = 0; a < 3; ++a) { clo[a] = list[0].c[a]; chi[a] = list[0].c[a]; }
    for (uint32_t k = 1; k < n; ++k)
        for (int a = 0; a < 3; ++a) { clo[a] = fminf(clo[a], list[k].c[a]); chi[a] = fmaxf(chi[a], list[k].c[a]); }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
    std::stable_sort(list, list + n, [axis](const Leaf& x, const Leaf& y) { return x.c[axis] < y.c[axis]; });
    const uint32_t nl = n / 2u, nr = n - nl, me = (uint32_t)nodes.size();
    nodes.emplace_back();
    LightNode nd;
    summarise(list, nl, nd.lo0, nd.hi0, nd.w0);
    summarise(list + nl, nr, nd.lo1, nd.hi1, nd.w1);
    nd.child0 = nl == 1u ? (TRT_LIGHT_LEAF | list[0].index) : split(list, nl, nodes);
    nd.child1 = nr == 1u ? (TRT_LIGHT_LEAF | list[nl].index) : split(list + nl, nr, nodes);
    nodes[me] = nd;
    return me;
}
}  // namespace lighttree

// The tree over `lights` (n_lights of them, their triangles in ltris[0, n_ltris)).  Nothing fails: a light that is no tree light is left out.
inline void buildLightTree(const LightDev* lights, uint32_t n_lights, const LightTriDev* ltris, uint32_t n_ltris, LightTree& out)
{
    out.nodes.clear();
    std::vector<lighttree::Leaf> list;
    for (uint32_t l = 0; l < n_lights; ++l) {
        const LightDev& L = lights[l];
        lighttree::Leaf f;
        f.index = l;
        f.w = lightWeight(L);
        if (!(f.w > 0.0f) || L.tri_count == 0u || L.tri_first > n_ltris || L.tri_count > n_ltris - L.tri_first) continue;
        bool finite = true;
        for (int a = 0; a < 3; ++a) { f.lo[a] = ltris[L.tri_first].v[0][a]; f.hi[a] = f.lo[a]; }
        for (uint32_t k = 0; k < L.tri_count; ++k)
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) {
                    const float x = ltris[L.tri_first + k].v[v][a];
                    finite = finite && std::isfinite(x);
                    f.lo[a] = fminf(f.lo[a], x);
                    f.hi[a] = fmaxf(f.hi[a], x);
                }
        if (!finite) continue;
        for (int a = 0; a < 3; ++a) f.c[a] = 0.5f * f.lo[a] + 0.5f * f.hi[a];
        list.push_back(f);
    }
    out.n_tree_lights = (uint32_t)list.size();
    if (list.empty()) { out.root = TRT_LIGHT_NONE; return; }
    if (list.size() == 1u) { out.root = TRT_LIGHT_LEAF | list[0].index; return; }
    out.nodes.reserve(list.size() - 1u);
    out.root = lighttree::split(list.data(), (uint32_t)list.size(), out.nodes);  // 0
}

}  // namespace trtd
