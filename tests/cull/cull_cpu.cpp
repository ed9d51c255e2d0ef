// CPU build of the camera-ray cull bound (tinyraytracing_amd/csrc/trt_cull.h) next to cameraRay, boxTest and boxTestGlm (trt_path.h), for
// tests/test_cull_cpu.py and tests/cull/cull_san.cpp: the bound itself, and a sweep that forms the camera ray of every culled pixel under
// a set of jitter pairs and counts the rays that break what the bound promises.
#include <stdint.h>

#include "trt_path.h"
#include "trt_cull.h"

using namespace trtd;

namespace {

trt_bvh_node rootOf(const float* boxes)
{
    trt_bvh_node n{};
    for (int k = 0; k < 3; ++k) { n.lo0[k] = boxes[k]; n.hi0[k] = boxes[3 + k]; n.lo1[k] = boxes[6 + k]; n.hi1[k] = boxes[9 + k]; }
    return n;
}

// the jitter pairs of the sweep: the four corners {0, 1 - 2^-24}^2, then n_interior points of a fixed sequence (splitmix64 of `seed`)
float jitter(uint64_t& state)
{
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);  // 24 bits: [0, 1 - 2^-24]
}

}  // namespace

extern "C" {

// out[0..7] = TileDesc::cull, out[8..15] = j_lo, j_hi, i_lo, i_hi, row_lo, row_hi, col_lo, col_hi.  -> 1 active, 0 off (*why says why)
int cull_bound(const trt_camera* cam, int W, int H, int fixed, const float* boxes, uint32_t n_nodes, double margin_pixels, int32_t* out, const char** why)
{
    const trt_bvh_node root = rootOf(boxes);
    const CullBound b = cullBound(*cam, W, H, fixed != 0, n_nodes ? &root : nullptr, n_nodes, margin_pixels);
    for (int k = 0; k < 8; ++k) out[k] = b.v[k];
    const int32_t r[8] = {b.j_lo, b.j_hi, b.i_lo, b.i_hi, b.row_lo, b.row_hi, b.col_lo, b.col_hi};
    for (int k = 0; k < 8; ++k) out[8 + k] = r[k];
    if (why) *why = b.why;
    return b.active ? 1 : 0;
}

// The camera ray of every culled pixel under every jitter pair, formed as the kernels form it (the reciprocal grid where the size allows it),
// and the plain-division form beside it.  counts[0] culled pixels, [1] rays formed, [2] rays that pass a root box under the clean slab test,
// [3] under the literal one, [4] rays with a zero direction component, [5] rays of raySpecial(), [6] rays whose two forms differ.
int cull_sweep(const trt_camera* cam, int W, int H, int fixed, const float* boxes, uint32_t n_nodes, double margin_pixels, uint64_t seed, int n_interior,
               uint64_t* counts)
{
    const trt_bvh_node root = rootOf(boxes);
    const CullBound b = cullBound(*cam, W, H, fixed != 0, n_nodes ? &root : nullptr, n_nodes, margin_pixels);
    for (int k = 0; k < 7; ++k) counts[k] = 0;
    if (!b.active) return 0;
    const double grid[4] = {1.0 / double(W - 1.0), 1.0 / double(H - 1.0), 1.0 / double(W), 1.0 / double(H)};
    const bool grid_ok = W >= 2 && H >= 2 && W <= 65536 && H <= 65536;
    const float top = 1.0f - 1.0f / 16777216.0f;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            if (!cullBoundCulls(b, W, H, i, j)) continue;
            counts[0]++;
            uint64_t state = seed ^ ((uint64_t)i << 32) ^ (uint64_t)j;
            for (int q = 0; q < 4 + n_interior; ++q) {
                const float u1 = q < 4 ? ((q & 1) ? top : 0.0f) : jitter(state), u2 = q < 4 ? ((q & 2) ? top : 0.0f) : jitter(state);
                f3 o, d, o2, d2;
                cameraRay(*cam, W, H, i, j, u1, u2, o, d, fixed != 0, grid_ok ? grid : nullptr);
                cameraRay(*cam, W, H, i, j, u1, u2, o2, d2, fixed != 0, nullptr);
                counts[1]++;
                counts[6] += !(f2u(d.x) == f2u(d2.x) && f2u(d.y) == f2u(d2.y) && f2u(d.z) == f2u(d2.z));
                const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                float e;
                counts[2] += boxTest(root.lo0[0], root.lo0[1], root.lo0[2], root.hi0[0], root.hi0[1], root.hi0[2], o, inv, e) ||
                             boxTest(root.lo1[0], root.lo1[1], root.lo1[2], root.hi1[0], root.hi1[1], root.hi1[2], o, inv, e);
                counts[3] += boxTestGlm(root.lo0[0], root.lo0[1], root.lo0[2], root.hi0[0], root.hi0[1], root.hi0[2], o, inv, e) ||
                             boxTestGlm(root.lo1[0], root.lo1[1], root.lo1[2], root.hi1[0], root.hi1[1], root.hi1[2], o, inv, e);
                counts[4] += d.x == 0.0f || d.y == 0.0f || d.z == 0.0f;
                counts[5] += raySpecial(inv);
            }
        }
    return 1;
}

}  // extern "C"
