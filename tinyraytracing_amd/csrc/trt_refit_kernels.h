// trt_refit_kernels.h — the __global__ wrappers of trt_refit.h (one element per thread) and the breadth-first numbering the level-by-level
// passes run on.  Every store is an ordinary vector store from plain C++; the only atomics are the list cursor of the numbering, the
// Bloom-filter bits and the light boxes' integer min / max.
#pragma once
#include <hip/hip_runtime.h>

#include "trt_refit.h"

namespace trtd {

constexpr uint32_t REFIT_BLOCK = 256;

// flag[0] |= 1 when a coordinate of tri_v[0 .. n_floats) is NaN or infinite
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_check(const float* __restrict__ tri_v, uint64_t n_floats, uint32_t* __restrict__ flag)
{
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * REFIT_BLOCK + threadIdx.x; i < n_floats; i += (uint64_t)gridDim.x * REFIT_BLOCK) bad = bad || !refitFinite(tri_v[i]);
    if (bad) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_tris(uint32_t n_tris, const float* __restrict__ tri_v, const float* __restrict__ tri_vn, TriIsect* __restrict__ isect,
                                                            TriShade* __restrict__ shade)
{
    const uint32_t i = blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (i < n_tris) refitTri(i, tri_v, tri_vn, isect, shade);
}

// Breadth-first numbering, one level per launch: order[begin .. end) holds the nodes of a level; their inner children are appended at
// *cursor (the host reads it back between launches: that is the next level's end).  Only nodes a root path reaches are listed — those
// trt_create has validated (in range, reached once) — so the list never exceeds n_nodes; `cap` guards the store all the same.
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_bfs2(const trt_bvh_node* __restrict__ nodes, uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                            uint32_t* __restrict__ cursor, uint32_t cap)
{
    const uint32_t t = begin + blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t >= end) return;
    const uint32_t i = order[t];
    if (i >= cap) return;
    const uint32_t ch[2] = {nodes[i].child0, nodes[i].child1};
    for (int k = 0; k < 2; ++k) {
        if (ch[k] & TRT_LEAF_BIT) continue;
        const uint32_t pos = atomicAdd(cursor, 1u);
        if (pos < cap) order[pos] = ch[k];
    }
}
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_bfs4(const WideNode* __restrict__ wnodes, uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                            uint32_t* __restrict__ cursor, uint32_t cap)
{
    const uint32_t t = begin + blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t >= end) return;
    const uint32_t i = order[t];
    if (i >= cap) return;
    const uint32_t* qu = reinterpret_cast<const uint32_t*>(wnodes[i].q);
    for (int k = 0; k < TRT_WIDE; ++k) {
        const uint32_t ref = qu[6 * 4 + k];
        if (ref == TRT_WIDE_EMPTY || (ref & TRT_LEAF_BIT)) continue;
        const uint32_t pos = atomicAdd(cursor, 1u);
        if (pos < cap) order[pos] = ref;
    }
}

// One level of the BVH2 / of the 4-wide tree: the nodes order[begin .. end)
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_level2(trt_bvh_node* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                              const float* __restrict__ tri_v, f4* __restrict__ leaf_box)
{
    const uint32_t t = begin + blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t >= end) return;
    const uint32_t i = order[t];
    if (i < n_nodes) refitNode2(nodes, i, tri_v, leaf_box);
}
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_level4(WideNode* __restrict__ wnodes, uint32_t n_wnodes, const uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                              const f4* __restrict__ leaf_box)
{
    const uint32_t t = begin + blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t >= end) return;
    const uint32_t i = order[t];
    if (i < n_wnodes) refitWide(wnodes, i, leaf_box);
}

__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_bfs8(const OctNode* __restrict__ onodes, uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                            uint32_t* __restrict__ cursor, uint32_t cap)
{
    const uint32_t t = begin + blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t >= end) return;
    const uint32_t i = order[t];
    if (i >= cap) return;
    const uint32_t n = (uint32_t)__popc(f2u(onodes[i].q[0].w) >> 24), base = f2u(onodes[i].q[1].x);
    if (!n) return;
    const uint32_t pos = atomicAdd(cursor, n);
    for (uint32_t k = 0; k < n; ++k)
        if (pos + k < cap) order[pos + k] = base + k;
}
// One level of the 8-wide tree; fail[0] |= 1 when a node no longer qualifies (refitOct)
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_level8(OctNode* __restrict__ onodes, uint32_t n_onodes, const uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                              const TriIsect* __restrict__ tri_trav, const f4* __restrict__ leaf_box, RefitBox* __restrict__ exact,
                                                              uint32_t* __restrict__ fail)
{
    const uint32_t t = begin + blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t >= end) return;
    const uint32_t i = order[t];
    if (i < n_onodes && !refitOct(onodes, i, tri_trav, leaf_box, exact)) atomicOr(fail, 1u);
}
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_tri_trav(uint32_t n, const TriIsect* __restrict__ isect, TriIsect* __restrict__ tri_trav)
{
    const uint32_t j = blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (j < n) refitTriTrav(j, isect, tri_trav);
}

// The filter of planeMaybe() over EVERY node of the array, reached or not, as wide_detail::planeFilterBuild sets it (bits cleared before)
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_planes(const trt_bvh_node* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ bits, uint32_t shift)
{
    const uint32_t n = blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (n >= n_nodes) return;
    const trt_bvh_node& nd = nodes[n];
    for (int a = 0; a < 3; ++a) {
        const float x[4] = {nd.lo0[a], nd.hi0[a], nd.lo1[a], nd.hi1[a]};
        for (int k = 0; k < 4; ++k) {
            const uint32_t h = (planeKey(a, x[k]) * 2246822519u) >> shift;
            atomicOr(&bits[h >> 5], 1u << (h & 31u));
        }
    }
}

// Per light the union of the leaf boxes of the triangles of its material (trt_oct_build.h lightBoxesOf), as ordered integers:
// boxes[6 l + a] = min of lo[a], boxes[6 l + 3 + a] = max of hi[a].  light_of_mat[m] = a light of material m, or -1.
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_light_boxes(uint32_t n_tris, const TriIsect* __restrict__ isect, const f4* __restrict__ leaf_box,
                                                                   const int32_t* __restrict__ light_of_mat, uint32_t n_materials, uint32_t* __restrict__ boxes)
{
    const uint32_t i = blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (i >= n_tris) return;
    const uint32_t m = f2u(isect[i].c.z) >> 8;
    if (m >= n_materials) return;
    const int32_t l = light_of_mat[m];
    if (l < 0) return;
    const f4 a = leaf_box[2 * (size_t)i], b = leaf_box[2 * (size_t)i + 1];
    uint32_t* B = boxes + 6 * (size_t)l;
    atomicMin(&B[0], refitOrdered(a.x)); atomicMin(&B[1], refitOrdered(a.y)); atomicMin(&B[2], refitOrdered(a.z));
    atomicMax(&B[3], refitOrdered(a.w)); atomicMax(&B[4], refitOrdered(b.x)); atomicMax(&B[5], refitOrdered(b.y));
}

}  // namespace trtd
