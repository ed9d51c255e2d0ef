// trt_refit.h — per-element functions of a geometry update (trt_update_geometry, include/trt.h): the boxes of a tree recomputed bottom-up
// from moved vertices, topology and leaf order kept.  Plain C++ marked TRT_HD: the HIP kernels (trt_refit_kernels.h) are thin wrappers, the host
// library (trth_scene_set_vertices) and tests/refit/refit_cpu.cpp compile the same functions for the CPU, so every side forms a box by one piece of code.
//
// The rule (include/trt.h): a leaf's box is per axis min(coordinates of its triangles) - 0.001f / max + 0.001f; an inner child's box is the union
// of that child's two boxes; a leaf of 0 triangles keeps the box it has.  min / max are exact and the one add is monotone, so the union of padded
// boxes is the padded union: the boxes nest by construction, and a 4-wide slot that stands for a dropped run of BVH2 nodes gets, as the union of
// the slots below it, bit for bit the BVH2 box it stands for.
//
// Order of work: a node needs its inner children finished.  Every function here does ONE node and reads only nodes of deeper levels, so the
// callers run the tree level by level, deepest first (the device: one launch per level, the kernel boundary is the coherence — what
// trt_lbvh.hip's K4b does for the nodes that span blocks; the LBVH builder, not a refit, measured agent-scope hand-offs per arrival three times slower).
#pragma once
#include "trt_oct.h"

namespace trtd {

#define TRT_REFIT_PAD 0.001f

struct RefitBox {
    float lo[3], hi[3];
};

// false for NaN and +-inf
TRT_HD inline bool refitFinite(float x) { return fabsf(x) <= 3.4028235e38f; }

// triangles [first, first + count), count >= 1
TRT_HD inline RefitBox refitLeafBox(const float* tri_v, uint32_t first, uint32_t count)
{
    RefitBox b;
    const float* v = tri_v + (size_t)first * 9;
    for (int a = 0; a < 3; ++a) b.lo[a] = b.hi[a] = v[a];
    for (uint32_t k = 1; k < 3u * count; ++k)
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = fminf(b.lo[a], v[3 * k + a]);
            b.hi[a] = fmaxf(b.hi[a], v[3 * k + a]);
        }
    for (int a = 0; a < 3; ++a) { b.lo[a] = b.lo[a] - TRT_REFIT_PAD; b.hi[a] = b.hi[a] + TRT_REFIT_PAD; }
    return b;
}

// BVH2 node i: both stored boxes.  leaf_box (may be null): the box of its leaf for every triangle of a leaf child (trt_wide.h leafBoxesOf).
TRT_HD inline void refitNode2(trt_bvh_node* nodes, uint32_t i, const float* tri_v, f4* leaf_box)
{
    trt_bvh_node& nd = nodes[i];
    for (int k = 0; k < 2; ++k) {
        const uint32_t ref = k ? nd.child1 : nd.child0;
        float* lo = k ? nd.lo1 : nd.lo0;
        float* hi = k ? nd.hi1 : nd.hi0;
        if (ref & TRT_LEAF_BIT) {
            const uint32_t first = TRT_LEAF_FIRST(ref), count = TRT_LEAF_COUNT(ref);
            if (count == 0) continue;
            const RefitBox b = refitLeafBox(tri_v, first, count);
            for (int a = 0; a < 3; ++a) { lo[a] = b.lo[a]; hi[a] = b.hi[a]; }
            if (leaf_box)
                for (uint32_t t = first; t < first + count; ++t) {
                    leaf_box[2 * (size_t)t] = mk4(b.lo[0], b.lo[1], b.lo[2], b.hi[0]);
                    leaf_box[2 * (size_t)t + 1] = mk4(b.hi[1], b.hi[2], 0.f, 0.f);
                }
        } else {
            const trt_bvh_node& c = nodes[ref];
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(c.lo0[a], c.lo1[a]); hi[a] = fmaxf(c.hi0[a], c.hi1[a]); }
        }
    }
}

// 4-wide node i in its own tree: a leaf slot from leaf_box of its first triangle, an inner slot as the union of the child node's slots.
// Slot count, leaf references and child indices are read from the node as the traversal reads them (q[6], TRT_WIDE_EMPTY).
TRT_HD inline void refitWide(WideNode* wnodes, uint32_t i, const f4* leaf_box)
{
    float* q = reinterpret_cast<float*>(wnodes[i].q);
    const uint32_t* qu = reinterpret_cast<const uint32_t*>(wnodes[i].q);
    for (int k = 0; k < TRT_WIDE; ++k) {
        const uint32_t ref = qu[6 * 4 + k];
        if (ref == TRT_WIDE_EMPTY) continue;
        RefitBox b;
        if (ref & TRT_LEAF_BIT) {
            if (TRT_LEAF_COUNT(ref) == 0) continue;
            const size_t t = TRT_LEAF_FIRST(ref);
            const f4 x = leaf_box[2 * t], y = leaf_box[2 * t + 1];
            b.lo[0] = x.x; b.lo[1] = x.y; b.lo[2] = x.z; b.hi[0] = x.w; b.hi[1] = y.x; b.hi[2] = y.y;
        } else {
            const float* c = reinterpret_cast<const float*>(wnodes[ref].q);
            const uint32_t* cu = reinterpret_cast<const uint32_t*>(wnodes[ref].q);
            bool any = false;
            for (int j = 0; j < TRT_WIDE; ++j) {
                if (cu[6 * 4 + j] == TRT_WIDE_EMPTY) continue;
                for (int a = 0; a < 3; ++a) {
                    b.lo[a] = any ? fminf(b.lo[a], c[a * 4 + j]) : c[a * 4 + j];
                    b.hi[a] = any ? fmaxf(b.hi[a], c[(3 + a) * 4 + j]) : c[(3 + a) * 4 + j];
                }
                any = true;
            }
            if (!any) continue;
        }
        for (int a = 0; a < 3; ++a) { q[a * 4 + k] = b.lo[a]; q[(3 + a) * 4 + k] = b.hi[a]; }
    }
}

// Triangle i: the 48-B intersection record from the new vertices (material and emissive bit from the record's own flags word, as trt_create wrote
// them), and the vertex normals of the shading record when given (texture coordinates and material stay).
TRT_HD inline void refitTri(uint32_t i, const float* tri_v, const float* tri_vn, TriIsect* isect, TriShade* shade)
{
    const uint32_t fl = f2u(isect[i].c.z);
    isect[i] = makeTriIsect(tri_v + (size_t)i * 9, (int32_t)(fl >> 8), (fl & 1u) != 0);
    if (tri_vn)
        for (int k = 0; k < 9; ++k) shade[i].vn[k] = tri_vn[(size_t)i * 9 + k];
}

// ---- the 8-wide compressed nodes (trt_oct.h) ----------------------------------------------------------------------------------------
// Child j of node i is onodes[child_base + (number of inner slots below j)]; a leaf slot's triangles are tri_trav[tri_base + offset ..].
TRT_HD inline uint32_t octMeta(const OctNode& on, int sl) { return (f2u(sl < 4 ? on.q[1].z : on.q[1].w) >> (8 * (sl & 3))) & 0xFFu; }
TRT_HD inline bool octMetaInner(uint32_t m) { return (m & 0x1Fu) >= 24u; }
TRT_HD inline uint32_t octChildIndex(const OctNode& on, int sl)
{
    const uint32_t imask = f2u(on.q[0].w) >> 24;
    return f2u(on.q[1].x) + trt_popc32(imask & ((1u << sl) - 1u));
}

// 8-wide node i: the exact box of every slot — an inner slot's from exact[child] (the union of the child's slots, written when the child was
// done), a leaf slot's from leaf_box of its first triangle, which is the box of the CALLER's whole leaf (slots of a split leaf all carry it) —
// then frame origin, exponents and bytes by octQuantise, and exact[i] = the union for the parent.  Slots, metas and bases stay.
// false: a coordinate reaches 2^40 or the extent is not representable — the tree no longer qualifies for this node kind (the node is left as it was).
// slot_lo / slot_hi (may be null): the exact boxes by slot, for tests.
TRT_HD inline bool refitOct(OctNode* onodes, uint32_t i, const TriIsect* tri_trav, const f4* leaf_box, RefitBox* exact, float (*slot_lo)[3] = nullptr,
                            float (*slot_hi)[3] = nullptr)
{
    OctNode& on = onodes[i];
    float blo[8][3], bhi[8][3];
    uint32_t mask = 0u;
    RefitBox u;
    for (int sl = 0; sl < 8; ++sl) {
        const uint32_t m = octMeta(on, sl);
        if (m == 0u) continue;
        if (octMetaInner(m)) {
            const RefitBox& c = exact[octChildIndex(on, sl)];
            for (int a = 0; a < 3; ++a) { blo[sl][a] = c.lo[a]; bhi[sl][a] = c.hi[a]; }
        } else {
            const size_t t = octTriOrig(f2u(tri_trav[f2u(on.q[1].y) + (m & 0x1Fu)].c.w));
            const f4 x = leaf_box[2 * t], y = leaf_box[2 * t + 1];
            blo[sl][0] = x.x; blo[sl][1] = x.y; blo[sl][2] = x.z; bhi[sl][0] = x.w; bhi[sl][1] = y.x; bhi[sl][2] = y.y;
        }
        for (int a = 0; a < 3; ++a) {
            u.lo[a] = mask ? fminf(u.lo[a], blo[sl][a]) : blo[sl][a];
            u.hi[a] = mask ? fmaxf(u.hi[a], bhi[sl][a]) : bhi[sl][a];
        }
        mask |= 1u << sl;
        if (slot_lo)
            for (int a = 0; a < 3; ++a) { slot_lo[sl][a] = blo[sl][a]; slot_hi[sl][a] = bhi[sl][a]; }
    }
    if (!mask) return true;
    exact[i] = u;
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(u.lo[a]) < 1.0995116e12f && fabsf(u.hi[a]) < 1.0995116e12f)) return false;  // buildOct's premise: below 2^40
    float p[3];
    uint32_t eb[3], qlo[3][8], qhi[3][8];
    if (!octQuantise(blo, bhi, mask, p, eb, qlo, qhi)) return false;
    on.q[0] = mk4(p[0], p[1], p[2], u2f(eb[0] | (eb[1] << 8) | (eb[2] << 16) | (f2u(on.q[0].w) & 0xFF000000u)));
    octStoreBounds(on, qlo, qhi);
    return true;
}

// Record j of tri_trav: the geometry of its triangle's (already rewritten) intersection record; index / leaf bits kept.
TRT_HD inline void refitTriTrav(uint32_t j, const TriIsect* isect, TriIsect* tri_trav)
{
    const uint32_t w = f2u(tri_trav[j].c.w), leaf_bits = f2u(tri_trav[j].c.z) & 0x1Eu;
    TriIsect T = isect[octTriOrig(w)];
    T.c.z = u2f(f2u(T.c.z) | leaf_bits);
    T.c.w = u2f(w);
    tri_trav[j] = T;
}

// Floats as unsigned integers of the same order, for min / max by integer atomics (order-independent, so deterministic).
TRT_HD inline uint32_t refitOrdered(float f) { const uint32_t u = f2u(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
TRT_HD inline float refitUnordered(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

}  // namespace trtd
