// refit_loops.h — TEST INFRASTRUCTURE.  The host loops around the per-node functions of a geometry update (csrc/trt_refit.h: refitNode2, refitWide,
// refitTriTrav, refitOct), shared by tests/refit/refit_cpu.cpp (node-by-node checks) and tests/hostsim/hostsim.cpp (a HostScene refitted in place).
// What the device's driver does with launches the loops do with lists: the trees are numbered breadth first from node 0, and a refit runs the levels
// deepest first, every node once.  The loops restate only that ORDER; every box is formed by the functions of trt_refit.h.
//
// Order: DEEPEST_FIRST is the update.  The other two are driver faults planted on purpose, for the sensitivity check of tests/test_refit_work_cpu.py —
// each leaves a valid, conservative tree (a stale box is a box of an earlier update), so only the traversal work can show it.
#pragma once
#include <cstring>
#include <vector>

#include "trt_oct_build.h"
#include "trt_refit.h"

namespace refitloops {
using namespace trtd;

enum Order {
    DEEPEST_FIRST = 0,     // children before parents
    SKIP_DEEPEST = 1,      // fault: the deepest level of the 4-wide / 8-wide tree is never covered, its nodes keep the boxes they had
    SHALLOWEST_FIRST = 2,  // fault: parents before children, so an inner slot takes its child's boxes from the previous update
};

// order[level[l] .. level[l + 1]) = the nodes of level l, level 0 = node 0; only nodes a root path reaches are listed
struct Levels {
    std::vector<uint32_t> order, level;
    size_t count() const { return level.size() - 1; }
};

// children(i, emit): calls emit(c) for every inner child c of node i
template <class Children>
inline Levels levelsOf(Children children)
{
    Levels L;
    L.order.push_back(0u);
    L.level.push_back(0u);
    size_t begin = 0;
    while (begin < L.order.size()) {
        const size_t end = L.order.size();
        L.level.push_back((uint32_t)end);
        for (size_t t = begin; t < end; ++t) children(L.order[t], [&](uint32_t c) { L.order.push_back(c); });
        begin = end;
    }
    return L;
}
inline Levels levels2(const trt_bvh_node* nodes)
{
    return levelsOf([&](uint32_t i, auto emit) {
        if (!(nodes[i].child0 & TRT_LEAF_BIT)) emit(nodes[i].child0);
        if (!(nodes[i].child1 & TRT_LEAF_BIT)) emit(nodes[i].child1);
    });
}
inline Levels levels4(const WideNode* wnodes)
{
    return levelsOf([&](uint32_t i, auto emit) {
        const uint32_t* qu = reinterpret_cast<const uint32_t*>(wnodes[i].q);
        for (int k = 0; k < TRT_WIDE; ++k)
            if (qu[24 + k] != TRT_WIDE_EMPTY && !(qu[24 + k] & TRT_LEAF_BIT)) emit(qu[24 + k]);
    });
}
inline Levels levels8(const OctNode* onodes)
{
    return levelsOf([&](uint32_t i, auto emit) {
        for (int sl = 0; sl < 8; ++sl) {
            const uint32_t m = octMeta(onodes[i], sl);
            if (m != 0u && octMetaInner(m)) emit(octChildIndex(onodes[i], sl));
        }
    });
}

// fn(node) for every listed node, level by level in `order`
template <class Fn>
inline void runLevels(const Levels& L, int order, Fn fn)
{
    const size_t n = L.count();
    for (size_t k = 0; k < n; ++k) {
        const size_t l = order == SHALLOWEST_FIRST ? k : n - 1 - k;
        if (order == SKIP_DEEPEST && n > 1 && l == n - 1) continue;
        for (uint32_t t = L.level[l]; t < L.level[l + 1]; ++t) fn(L.order[t]);
    }
}

// BVH2 of the caller refitted to tri_v, with the per-triangle leaf boxes (an empty leaf keeps its box, so they start as the tree's own)
inline void refit2(std::vector<trt_bvh_node>& nodes, uint32_t n_tris, const float* tri_v, std::vector<f4>& leaf_box)
{
    leaf_box = leafBoxesOf(nodes.data(), (uint32_t)nodes.size(), n_tris, 1);
    runLevels(levels2(nodes.data()), DEEPEST_FIRST, [&](uint32_t i) { refitNode2(nodes.data(), i, tri_v, leaf_box.data()); });
}

// the 4-wide nodes in their own tree
inline void refitWideTree(std::vector<WideNode>& wnodes, const f4* leaf_box, int order = DEEPEST_FIRST)
{
    runLevels(levels4(wnodes.data()), order, [&](uint32_t i) { refitWide(wnodes.data(), i, leaf_box); });
}

// The 8-wide nodes and their triangle records; isect = the intersection records of the moved triangles.  exact[node] = the scratch record the
// device keeps from one update to the next (sized here when empty).  slot_box (may be null): [node][slot][6] exact boxes of the nodes that were run.
// false: a node no longer qualified (refitOct) — the loop stops there.
inline bool refitOctTree(OctTree& t, const TriIsect* isect, const f4* leaf_box, std::vector<RefitBox>& exact, int order = DEEPEST_FIRST, float* slot_box = nullptr)
{
    for (uint32_t j = 0; j < t.tri_trav.size(); ++j) refitTriTrav(j, isect, t.tri_trav.data());
    if (exact.size() != t.nodes.size()) exact.assign(t.nodes.size(), RefitBox{});
    bool ok = true;
    runLevels(levels8(t.nodes.data()), order, [&](uint32_t i) {
        if (!ok) return;
        float lo[8][3], hi[8][3];
        std::memset(lo, 0, sizeof(lo));
        std::memset(hi, 0, sizeof(hi));
        if (!refitOct(t.nodes.data(), i, t.tri_trav.data(), leaf_box, exact.data(), lo, hi)) { ok = false; return; }
        if (slot_box)
            for (int sl = 0; sl < 8; ++sl)
                for (int a = 0; a < 3; ++a) { slot_box[((size_t)i * 8 + sl) * 6 + a] = lo[sl][a]; slot_box[((size_t)i * 8 + sl) * 6 + 3 + a] = hi[sl][a]; }
    });
    return ok;
}

}  // namespace refitloops
