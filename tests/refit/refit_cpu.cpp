// refit_cpu.cpp — the per-node functions of a geometry update (csrc/trt_refit.h) run on the host over collapseBvh / buildOct output, for
// tests/test_refit_cpu.py: the same code the HIP kernels wrap, children before parents (the loops: refit_loops.h).
#include <cstring>
#include <vector>

#include "refit_loops.h"

using namespace trtd;
using namespace refitloops;

extern "C" {

// collapseBvh(nodes2) -> `before`; the same nodes refitted in their own tree to tri_v -> `after`; nodes2_out = the refitted BVH2.
// Returns the number of 4-wide nodes, or -1 when it exceeds cap.
int refit_cpu_wide(const trt_bvh_node* nodes2, uint32_t n2, uint32_t n_tris, const float* tri_v, int greedy, trt_bvh_node* nodes2_out, WideNode* before,
                   WideNode* after, uint32_t cap)
{
    std::vector<trt_bvh_node> nodes(nodes2, nodes2 + n2);
    WideTree w = greedy ? collapseBvhGreedy(nodes2, n2, 1) : collapseBvh(nodes2, n2, 1);
    if (w.nodes.size() > cap) return -1;
    std::memcpy(before, w.nodes.data(), w.nodes.size() * sizeof(WideNode));
    std::vector<f4> leaf_box;
    refit2(nodes, n_tris, tri_v, leaf_box);
    std::memcpy(nodes2_out, nodes.data(), n2 * sizeof(trt_bvh_node));
    refitWideTree(w.nodes, leaf_box.data());
    std::memcpy(after, w.nodes.data(), w.nodes.size() * sizeof(WideNode));
    return (int)w.nodes.size();
}

// buildOct(nodes2, triangles of v_build) -> `before`; refitted to tri_v -> `after`; slot_box[node][slot][6] = the exact box (lo, hi) of every
// used slot after the refit; tri_orig[node][slot] = post-BVH index of a leaf slot's first triangle, -1 for an inner or empty slot.
// Returns the number of 8-wide nodes; -1: over cap; -2: buildOct did not build; -3: a node no longer qualified.
int refit_cpu_oct(const trt_bvh_node* nodes2, uint32_t n2, uint32_t n_tris, const float* v_build, const float* tri_v, trt_bvh_node* nodes2_out, OctNode* before,
                  OctNode* after, float* slot_box, int32_t* tri_orig, uint32_t cap)
{
    std::vector<TriIsect> isect(n_tris ? n_tris : 1);
    for (uint32_t i = 0; i < n_tris; ++i) isect[i] = makeTriIsect(v_build + (size_t)i * 9, 0, false);
    OctTree t = buildOct(nodes2, n2, n_tris, isect.data(), 1);
    if (!t.ok) return -2;
    if (t.nodes.size() > cap) return -1;
    std::memcpy(before, t.nodes.data(), t.nodes.size() * sizeof(OctNode));
    std::vector<trt_bvh_node> nodes(nodes2, nodes2 + n2);
    std::vector<f4> leaf_box;
    refit2(nodes, n_tris, tri_v, leaf_box);
    std::memcpy(nodes2_out, nodes.data(), n2 * sizeof(trt_bvh_node));
    for (uint32_t i = 0; i < n_tris; ++i) isect[i] = makeTriIsect(tri_v + (size_t)i * 9, 0, false);
    std::vector<RefitBox> exact;
    if (!refitOctTree(t, isect.data(), leaf_box.data(), exact, DEEPEST_FIRST, slot_box)) return -3;
    runLevels(levels8(t.nodes.data()), DEEPEST_FIRST, [&](uint32_t i) {
        for (int sl = 0; sl < 8; ++sl) {
            const uint32_t m = octMeta(t.nodes[i], sl);
            tri_orig[(size_t)i * 8 + sl] = -1;
            if (m != 0u && !octMetaInner(m)) tri_orig[(size_t)i * 8 + sl] = (int32_t)octTriOrig(f2u(t.tri_trav[f2u(t.nodes[i].q[1].y) + (m & 0x1Fu)].c.w));
        }
    });
    std::memcpy(after, t.nodes.data(), t.nodes.size() * sizeof(OctNode));
    return (int)t.nodes.size();
}

}  // extern "C"
