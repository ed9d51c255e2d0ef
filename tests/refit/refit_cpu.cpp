// refit_cpu.cpp — the per-node functions of a geometry update (csrc/trt_refit.h) run on the host over collapseBvh / buildOct output, for
// tests/test_refit_cpu.py: the same code the HIP kernels wrap, children before parents.
#include <cstring>
#include <vector>

#include "trt_oct_build.h"
#include "trt_refit.h"

using namespace trtd;

namespace {
// BVH2 of the caller refitted to tri_v, with the per-triangle leaf boxes
void refit2(std::vector<trt_bvh_node>& nodes, uint32_t n_tris, const float* tri_v, std::vector<f4>& leaf_box)
{
    leaf_box = leafBoxesOf(nodes.data(), (uint32_t)nodes.size(), n_tris, 1);
    std::vector<uint32_t> order, st{0u};
    while (!st.empty()) {
        const uint32_t i = st.back();
        st.pop_back();
        order.push_back(i);
        if (!(nodes[i].child0 & TRT_LEAF_BIT)) st.push_back(nodes[i].child0);
        if (!(nodes[i].child1 & TRT_LEAF_BIT)) st.push_back(nodes[i].child1);
    }
    for (size_t k = order.size(); k-- > 0;) refitNode2(nodes.data(), order[k], tri_v, leaf_box.data());
}
}  // namespace

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
    std::vector<uint32_t> order, st{0u};
    while (!st.empty()) {
        const uint32_t i = st.back();
        st.pop_back();
        order.push_back(i);
        const uint32_t* qu = reinterpret_cast<const uint32_t*>(w.nodes[i].q);
        for (int k = 0; k < TRT_WIDE; ++k)
            if (qu[24 + k] != TRT_WIDE_EMPTY && !(qu[24 + k] & TRT_LEAF_BIT)) st.push_back(qu[24 + k]);
    }
    for (size_t k = order.size(); k-- > 0;) refitWide(w.nodes.data(), order[k], leaf_box.data());
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
    for (uint32_t j = 0; j < t.tri_trav.size() && n_tris; ++j) refitTriTrav(j, isect.data(), t.tri_trav.data());
    std::vector<uint32_t> order, st{0u};
    while (!st.empty()) {
        const uint32_t i = st.back();
        st.pop_back();
        order.push_back(i);
        for (int sl = 0; sl < 8; ++sl) {
            const uint32_t m = octMeta(t.nodes[i], sl);
            tri_orig[(size_t)i * 8 + sl] = -1;
            if (m == 0u) continue;
            if (octMetaInner(m)) st.push_back(octChildIndex(t.nodes[i], sl));
            else tri_orig[(size_t)i * 8 + sl] = (int32_t)octTriOrig(f2u(t.tri_trav[f2u(t.nodes[i].q[1].y) + (m & 0x1Fu)].c.w));
        }
    }
    std::vector<RefitBox> exact(t.nodes.size());
    for (size_t k = order.size(); k-- > 0;) {
        float lo[8][3], hi[8][3];
        std::memset(lo, 0, sizeof(lo));
        std::memset(hi, 0, sizeof(hi));
        if (!refitOct(t.nodes.data(), order[k], t.tri_trav.data(), leaf_box.data(), exact.data(), lo, hi)) return -3;
        for (int sl = 0; sl < 8; ++sl)
            for (int a = 0; a < 3; ++a) { slot_box[((size_t)order[k] * 8 + sl) * 6 + a] = lo[sl][a]; slot_box[((size_t)order[k] * 8 + sl) * 6 + 3 + a] = hi[sl][a]; }
    }
    std::memcpy(after, t.nodes.data(), t.nodes.size() * sizeof(OctNode));
    return (int)t.nodes.size();
}

}  // extern "C"
