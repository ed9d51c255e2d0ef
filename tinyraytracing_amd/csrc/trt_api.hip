// trt_api.hip — C-ABI implementation (include/trt.h) for gfx950: scene upload,
// the wavefront render loop that replaces main.cpp:79-113, and the ray-batch
// traversal entry.  No CPU compute path exists in this library.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <limits>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "trt.h"
#include "trt_kernels.h"
#include "trt_lighttree.h"
#include "trt_cull.h"
#include "trt_sched.h"
#include "trt_wide.h"
#include "trt_oct_build.h"
#include "trt_denoise_kernels.h"
#include "trt_reproject_kernels.h"
#include "trt_moments_kernels.h"
#include "trt_despeckle_kernels.h"
#include "trt_refit_kernels.h"

using namespace trtd;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

#define HIPC(expr)                                                                                         \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return fail(e_ == hipErrorOutOfMemory ? TRT_ENOMEM : TRT_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr uint32_t MAX_TRACE_BLOCKS = 8192;                       // persistent grid cap of the traversal kernels
constexpr uint32_t SPILL_STRIDE = MAX_TRACE_BLOCKS * TRT_TRACE_BLOCK;
constexpr uint32_t MAX_BOUNCES = TRT_MAX_PATH_DEPTH + 2;
// Device layout of the counters: counter c of bounce b lives at d_counts[c * COUNT_STRIDE + b], so the
// counters k_shade bumps in one launch lie 16 KiB apart (different L2 channels: the atomic units work in
// parallel) instead of in one cache line.
constexpr uint32_t COUNT_STRIDE = (MAX_BOUNCES + 2 + 1023u) & ~1023u;
// Counter rows per bounce for a scene of nl lights: [0] = queue length, [1+l] = shadow rays of light l, and the last two rows
// (the pair rows) hold, as one 64-bit word per bounce b, the two counters k_shade reserves with one atomic: low word = length of
// the queue of bounce b + 1, high word = shadow rays of the last light at bounce b.  k_publish_counts also reads row nl (the
// last light's own row, unused), so the pair rows start at nl + 1 or later: 16 rows up to 13 lights, multiples of 16 beyond.
constexpr uint32_t COUNT_ROW_MIN = 16;
inline uint32_t countRows(uint32_t nl) { return std::max(COUNT_ROW_MIN, (nl + 3u + 15u) & ~15u); }
inline unsigned long long* pairCounter(uint32_t* d_counts, uint32_t rows, uint32_t b) { return reinterpret_cast<unsigned long long*>(d_counts + (size_t)(rows - 2u) * COUNT_STRIDE) + b; }
// The most lights a scene may have: the counters take COUNT_STRIDE * 4 B = 16 KiB per light and pass slot (1 GiB per slot at the
// bound), and every light costs a shadow launch per bounce (include/trt.h TRT_MAX_SCENE_LIGHTS).
static_assert(TRT_MAX_SCENE_LIGHTS <= 65535u, "counter area");
constexpr uint32_t MAX_BVH_DEPTH = 256;
// node kind of the persistent traversal kernels when the tree qualifies for both (DESIGN.md §4.1 has the A/B)
#ifndef TRT_DEFAULT_NODE_KIND
#define TRT_DEFAULT_NODE_KIND 1
#endif

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes) return TRT_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        HIPC(hipMalloc(&p, need));
        bytes = need;
        return TRT_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// The bracket of a call that reports three fields of trt_stats (the image-space passes, the geometry update): four events on the call's
// stream — 0 before everything, 1 before the first kernel, 2 behind the last, 3 behind everything — and, once the stream is synchronised,
// the statistics they give.  The events are created on demand and live as long as the bracket.
struct EventBracket {
    hipEvent_t ev[4] = {};
    EventBracket() = default;
    EventBracket(const EventBracket&) = delete;
    ~EventBracket()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create()
    {
        for (hipEvent_t& e : ev)
            if (!e) HIPC(hipEventCreate(&e));
        return TRT_OK;
    }
    int record(int i, hipStream_t stream) { HIPC(hipEventRecord(ev[i], stream)); return TRT_OK; }
    // every field 0 but the `launches` of `kernel_slot`, its kernel_ms (events 1 -> 2) and render_ms (events 0 -> 3); stats may be null
    int fill(trt_stats* stats, int kernel_slot, uint64_t launches) const
    {
        if (!stats) return TRT_OK;
        float k_ms = 0.f, all_ms = 0.f;
        HIPC(hipEventElapsedTime(&k_ms, ev[1], ev[2]));
        HIPC(hipEventElapsedTime(&all_ms, ev[0], ev[3]));
        std::memset(stats, 0, sizeof(*stats));
        stats->launches[kernel_slot] = launches;
        stats->kernel_ms[kernel_slot] = k_ms;
        stats->render_ms = all_ms;
        return TRT_OK;
    }
};

}  // namespace

struct trt_handle {
    int device = 0;
    SceneDev sc{};
    std::vector<void*> scene_allocs;
    std::vector<uint32_t> light_mats;
    std::vector<LightBox> light_boxes;  // per light: the union of the boxes of the leaves that hold its triangles (trt_kernels.h LightBox)
    uint32_t depth = 0;       // stack entries a traversal can need (wide tree), + 1
    uint32_t bvh2_depth = 0;  // depth of the caller's BVH2
    uint32_t shade_tabs = 0;  // which k_shade<TABS> this scene runs
    uint32_t shade_pad_lds = 0;  // TRT_SHADE_PAD_LDS (probe): dynamic LDS bytes added to every k_shade launch — takes blocks off the CU to measure how the kernel's time hangs on its occupancy
    const void* lds_image = nullptr;  // the tables of shade_tabs, packed
    uint32_t lds_image_bytes = 0;
    uint32_t lds_tab[5] = {0, 0, 0, 0, 0};  // bytes of materials / lights / light CDF / light triangles / (tiny scenes) shading triangles that k_shade stages in LDS
    int trace_impl = 3;       // wave driver of the traversal kernels (0 wave-uniform walk of a tiny tree, 3 persistent waves + step scheduler)
    // The wave-uniform walk's faster kernels (trt_kernels.h traceQueueUniform PIPE / HIT8); TRT_SLIM_WALK=0 at trt_create keeps the earlier ones (A/B, tests):
    bool slim_walk = false;   // both walk kernels read the triangles' flag words from an LDS copy
    bool hit8 = false;        // and the render's hit records are 8 bytes (t, bits(tri)); k_shade forms (u, v) itself — needs k_shade<31> (every table in LDS)
    bool bin_walk = false;    // and the closest-hit queue kernel sorts each wave's rays by the leaves they reach (trt_kernels.h traceQueueBinned; TRT_BIN_WALK=0 at
                              // trt_create keeps traceQueueUniform's kernel: A/B, tests)
    bool fuse_primary = false;  // and, with one light, bounce 0 of a tile render is ONE kernel: k_shade's FUSE flavour walks the camera rays itself, no hit record
                                // is written or read (trt_kernels.h fusedWalk; TRT_FUSE_PRIMARY=0 at trt_create keeps the two kernels: A/B, tests)
    // Camera rays that provably miss the root's two child boxes are not formed, walked or resolved (trt_cull.h; tile renders without TRT_FLAG_COUNT).
    // TRT_CULL_PRIMARY=0 at trt_create turns it off (A/B, tests).  root_node is nodes[0] of the caller's BVH2 as the device holds it: trt_create's
    // copy, and after trt_update_geometry the node that call reads back once its refit is through.
    bool cull_primary = true;
    bool root_known = false;
    trt_bvh_node root_node{};
    int node_kind = 0;        // what the persistent traversal kernels walk: 0 exact 128-B 4-wide nodes, 1 compressed 80-B 8-wide nodes (trt_oct.h)
    uint32_t oct_levels = 0;  // nodes on the longest root path of the oct tree
    bool dbg = false;         // TRT_DEBUG at trt_create: every render prints which k_shade variant it runs
    // Grid of the traversal kernels for a queue of n rays.  A persistent wave refills finished lanes from its own slice
    // of the queue, which only pays when the slice holds several batches: aim for rays_per_wave rays per wave, but do
    // not go below the fill_blocks that fill the chip's wave slots, nor above one block per 256 rays.
    // (TRT_TRACE_RPW / TRT_TRACE_FILLB / TRT_TRACE_MAXB in the environment at trt_create: tuning.)  Per handle: no
    // process-wide mutable state in this library.
    uint32_t rays_per_wave = 256, fill_blocks = 2048, max_blocks = 8192;
    uint32_t traceGrid(uint32_t n) const
    {
        uint32_t b = (n + TRT_TRACE_BLOCK - 1) / TRT_TRACE_BLOCK;
        if (rays_per_wave > 64) {
            const uint32_t want = (uint32_t)(((uint64_t)n + 4ull * rays_per_wave - 1) / (4ull * rays_per_wave));
            b = std::min(b, std::max(fill_blocks, want));
        }
        b = std::min(std::max(b, 8u), std::min(max_blocks, 8192u));
        return (b + 7u) & ~7u;  // multiple of 8 for the XCD swizzle; <= MAX_TRACE_BLOCKS (8192) since that is one too
    }
    uint32_t tail_n = 131072;  // queue length at or below which k_tail finishes the pass (TRT_TAIL_N overrides)
    DevBuf arena, spill, small_buf, out_buf, io_buf;
    size_t spill_words_per_slot = 0;
    hipStream_t slot_streams[2] = {nullptr, nullptr};  // one per concurrent pass (trt_render_device)
    int n_slots = 2;                                   // TRT_SLOTS=1 in the environment vetoes TRT_FLAG_OVERLAP
    uint32_t* pinned_counts = nullptr;                 // host-pinned landing zone of the per-bounce queue lengths
    uint32_t count_rows = COUNT_ROW_MIN;               // counter rows per bounce (countRows(n_lights)); the landing zone has 2 * count_rows + 16 words per slot
    uint32_t slot_seq[2] = {0, 0};                     // last sequence number published per slot: monotonic over the handle's life, so a
                                                       // word left behind by an earlier (even a failed) call never equals an expected one
    int fail_at_bounce = -1;                           // TRT_TEST_FAIL_AT_BOUNCE at trt_create: the next render reports an injected failure
                                                       // after issuing that bounce (exercises the error path; consumed once)
    std::vector<hipEvent_t> events;
    // The shadow walks of bounce b beside closest hits and k_shade of bounce b + 1 (renderCore): a second stream for them and the
    // events that tie the two — per bounce parity, [0..1] behind k_shade on the pass's stream, [2..3] behind the last shadow launch on this one.
    // Made once, without timing.  TRT_SHADOW_STREAM=0 at trt_create keeps every kernel of a pass on one stream (A/B, tests).
    hipStream_t side_stream = nullptr;
    hipEvent_t side_events[4] = {nullptr, nullptr, nullptr, nullptr};
    bool shadow_stream = true;
    bool refracts = false;    // a material with Ni > 1: only then k_shade's queue flavour adds to Lacc past bounce 0 (TRANSMISSION, trt_path.h shadeBegin)
    bool dbg_sched = false;   // TRT_DEBUG and TRT_DEBUG_SCHEDULE=1 at trt_create: renderCore prints every operation it enqueues (SchedTrace)
    // trt_update_geometry: what trt_create leaves behind for it costs no device memory; the rest is made at the first update and kept
    uint32_t n_materials = 0, n_light_tris = 0, n_tri_trav = 0;
    bool light_boxes_fixed = false;                    // TRT_SHADOW_STOP=0 at trt_create: every light's box is all of space and stays so
    struct Refit {
        bool ready = false;
        DevBuf order2, order4, order8, exact8, small;  // breadth-first node lists of the BVH2, the 4-wide and the 8-wide tree; per 8-wide node the exact union
                                                       // of its slots; cursor + flags + light boxes
        std::vector<uint32_t> level2, level4, level8;  // level l = order[level[l] .. level[l + 1])
        DevBuf light_of_mat;
        EventBracket bracket;
    } refit;
    ~trt_handle()
    {
        refit.order2.release();
        refit.order4.release();
        refit.order8.release();
        refit.exact8.release();
        refit.small.release();
        refit.light_of_mat.release();
        for (void* p : scene_allocs) (void)hipFree(p);
        arena.release();
        spill.release();
        small_buf.release();
        out_buf.release();
        io_buf.release();
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (hipStream_t st : slot_streams) if (st) (void)hipStreamDestroy(st);
        for (hipEvent_t e : side_events) if (e) (void)hipEventDestroy(e);
        if (side_stream) (void)hipStreamDestroy(side_stream);
        if (pinned_counts) (void)hipHostFree(pinned_counts);
    }
};

namespace {

template <class T>
int upload(trt_handle* h, const T* src, size_t count, const T** dst)
{
    void* p = nullptr;
    const size_t bytes = (std::max<size_t>(count, 1) * sizeof(T) + 15) & ~(size_t)15;  // readable in whole 16-B words
    HIPC(hipMalloc(&p, bytes));
    h->scene_allocs.push_back(p);
    if (count) HIPC(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = (const T*)p;
    return TRT_OK;
}

// Structural check of the flat BVH and its true depth (the kernels size their
// stacks from it): every child reference in range, every leaf range in range,
// no node reachable twice (no cycles / DAGs), and every triangle under child0 has
// a lower index than every triangle under child1 — the post-BVH order of the
// reference (bvh.cpp sorts the triangle array in place and recurses on its two halves),
// which is what lets the between-leaves tie rule "r1 if r1 emissive else r2" (bvh.cpp:168-172)
// be applied by triangle index in any visiting order.
int validateBvh(const trt_scene* s, uint32_t* depth_out, unsigned threads = 1)
{
    // One walk per subtree of a cut of the tree (the cut itself, a few hundred nodes, is walked here first), subtrees side by side on
    // `threads` host threads: marks are atomic bytes, so a node or triangle that two walks reach is caught whichever gets there second.
    const uint32_t nn = s->n_nodes;
    std::unique_ptr<std::atomic<uint8_t>[]> seen(new std::atomic<uint8_t>[nn]);
    std::unique_ptr<std::atomic<uint8_t>[]> tri_seen(new std::atomic<uint8_t>[std::max<uint32_t>(s->n_tris, 1u)]);
    par::forRange(nn, threads, 1u << 20, [&](size_t b, size_t e) { for (size_t i = b; i < e; ++i) seen[i].store(0, std::memory_order_relaxed); });
    par::forRange(s->n_tris, threads, 1u << 20, [&](size_t b, size_t e) { for (size_t i = b; i < e; ++i) tri_seen[i].store(0, std::memory_order_relaxed); });
    // (min, max) triangle index under every inner node: index order of siblings, children before parents
    std::unique_ptr<uint32_t[]> lo(new uint32_t[nn]), hi(new uint32_t[nn]);
    std::unique_ptr<uint8_t[]> has(new uint8_t[nn]);
    // what one node says about itself: its own checks, its inner children appended to `kids`; nullptr or the complaint
    auto visit = [&](uint32_t ni, uint32_t dep, uint32_t* kids, int& n_kids) -> const char* {
        n_kids = 0;
        if (ni >= nn) return "bvh: child index out of range";
        if (seen[ni].exchange(1, std::memory_order_relaxed)) return "bvh: node reachable twice";
        if (dep > MAX_BVH_DEPTH) return "bvh: deeper than 256 levels";
        // A NaN box coordinate is refused: glm::min / glm::max (bvh.cpp:238-242) let a NaN through from their FIRST operand only, so what such a box does to a ray
        // depends on the axis it sits on — a behaviour nobody builds on, and one the kernels' v_min / v_max (which drop a NaN from either side) would have to pay
        // two instructions per slab to mimic.  +-inf and every finite value, nested or not, are fine (tests: poisoned geometry; boxes that do not nest).
        {
            const trt_bvh_node& nd = s->nodes[ni];
            for (int a = 0; a < 3; ++a)
                if (nd.lo0[a] != nd.lo0[a] || nd.hi0[a] != nd.hi0[a] || nd.lo1[a] != nd.lo1[a] || nd.hi1[a] != nd.hi1[a]) return "bvh: a box coordinate is NaN";
        }
        const uint32_t ch[2] = {s->nodes[ni].child0, s->nodes[ni].child1};
        for (uint32_t c : ch) {
            if (c & TRT_LEAF_BIT) {
                const uint32_t first = TRT_LEAF_FIRST(c), count = TRT_LEAF_COUNT(c);
                if ((uint64_t)first + count > s->n_tris) return "bvh: leaf range out of bounds";
                for (uint32_t i = first; i < first + count; ++i)
                    if (tri_seen[i].exchange(1, std::memory_order_relaxed)) return "bvh: triangle in two leaves";
            } else {
                kids[n_kids++] = c;
            }
        }
        return nullptr;
    };
    auto order_rule = [&](uint32_t n) -> const char* {  // children already done
        uint32_t clo[2], chi[2];
        bool chas[2];
        const uint32_t ch[2] = {s->nodes[n].child0, s->nodes[n].child1};
        for (int c = 0; c < 2; ++c) {
            if (ch[c] & TRT_LEAF_BIT) {
                const uint32_t first = TRT_LEAF_FIRST(ch[c]), count = TRT_LEAF_COUNT(ch[c]);
                chas[c] = count != 0;
                clo[c] = first;
                chi[c] = first + count - (count ? 1u : 0u);
            } else {
                chas[c] = has[ch[c]] != 0;
                clo[c] = lo[ch[c]];
                chi[c] = hi[ch[c]];
            }
        }
        if (chas[0] && chas[1] && !(chi[0] < clo[1])) return "bvh: triangles under child0 must precede those under child1 (post-BVH order)";
        has[n] = chas[0] || chas[1];
        lo[n] = std::min(chas[0] ? clo[0] : 0xFFFFFFFFu, chas[1] ? clo[1] : 0xFFFFFFFFu);
        hi[n] = std::max(chas[0] ? chi[0] : 0u, chas[1] ? chi[1] : 0u);
        return nullptr;
    };
    struct Ref { uint32_t node, depth; };
    std::vector<Ref> top{{0u, 1u}};  // the cut: breadth first, parents before children
    size_t head = 0;
    uint32_t max_depth = 0;
    const size_t want = threads > 1 ? (size_t)threads * 16 : 1;
    while (threads > 1 && head < top.size() && top.size() - head < want) {
        const Ref r = top[head++];
        uint32_t kids[2];
        int nk;
        if (const char* why = visit(r.node, r.depth, kids, nk)) return fail(TRT_EINVAL, why);
        max_depth = std::max(max_depth, r.depth);
        for (int k = 0; k < nk; ++k) top.push_back({kids[k], r.depth + 1});
    }
    const size_t n_roots = top.size() - head;
    std::vector<const char*> why_of(n_roots, nullptr);
    std::vector<uint32_t> depth_of(n_roots, 0);
    par::forTasks(n_roots, threads, [&](size_t ti) {
        std::vector<Ref> st{top[head + ti]};
        std::vector<uint32_t> order;
        while (!st.empty()) {
            const Ref r = st.back();
            st.pop_back();
            uint32_t kids[2];
            int nk;
            if (const char* why = visit(r.node, r.depth, kids, nk)) { why_of[ti] = why; return; }
            order.push_back(r.node);
            depth_of[ti] = std::max(depth_of[ti], r.depth);
            for (int k = 0; k < nk; ++k) st.push_back({kids[k], r.depth + 1});
        }
        for (size_t k = order.size(); k-- > 0;)
            if (const char* why = order_rule(order[k])) { why_of[ti] = why; return; }
    });
    for (size_t ti = 0; ti < n_roots; ++ti) {
        if (why_of[ti]) return fail(TRT_EINVAL, why_of[ti]);
        max_depth = std::max(max_depth, depth_of[ti]);
    }
    for (size_t k = head; k-- > 0;)
        if (const char* why = order_rule(top[k].node)) return fail(TRT_EINVAL, why);
    *depth_out = max_depth;
    return TRT_OK;
}

int checkParams(const trt_handle* h, const trt_params* p)
{
    if (!h || !p) return fail(TRT_EINVAL, "null handle/params");
    if (p->width < 2 || p->height < 2) return fail(TRT_EINVAL, "width and height must be >= 2 (x = j/(W-1), main.cpp:88)");
    if (p->spp < 1) return fail(TRT_EINVAL, "spp must be >= 1");
    if (p->x0 < 0 || p->y0 < 0 || p->x1 > p->width || p->y1 > p->height || p->x0 >= p->x1 || p->y0 >= p->y1) return fail(TRT_EINVAL, "tile rectangle outside the image or empty");
    if (p->row_mod > 1 && (p->row_block < 1 || p->row_rem < 0 || p->row_rem >= p->row_mod)) return fail(TRT_EINVAL, "bad row interleave");
    if (p->max_depth < 0) return fail(TRT_EINVAL, "max_depth must be >= 0");
    if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull) return fail(TRT_EINVAL, "image too large");
    return TRT_OK;
}
// The estimator flags of the entries that trace full paths (the AOV and ray-query entries ignore them)
int checkEstimator(const trt_params* p)
{
    if ((p->flags & TRT_FLAG_ONE_LIGHT) && !(p->flags & TRT_FLAG_FIXED_NEE))
        return fail(TRT_EINVAL, "TRT_FLAG_ONE_LIGHT needs TRT_FLAG_FIXED_NEE (rays to different lights share one queue of occlusion tests)");
    if ((p->flags & TRT_FLAG_NEAR_LIGHTS) && !(p->flags & TRT_FLAG_ONE_LIGHT))
        return fail(TRT_EINVAL, "TRT_FLAG_NEAR_LIGHTS needs TRT_FLAG_ONE_LIGHT (it changes how that flag's one light is picked)");
    return TRT_OK;
}

bool rowSelected(const trt_params* p, int y) { return p->row_mod <= 1 || ((y / p->row_block) % p->row_mod) == p->row_rem; }

uint32_t tailGrid(uint32_t n)
{
    uint32_t b = (n + TRT_TRACE_BLOCK - 1) / TRT_TRACE_BLOCK;
    b = std::min(std::max(b, 8u), MAX_TRACE_BLOCKS);
    return (b + 7u) & ~7u;
}
struct Timer {
    trt_handle* h;
    bool on;
    size_t used = 0;
    struct Span { int k; size_t e0, e1; };
    std::vector<Span> spans{};
    static constexpr size_t RESERVED = 3;  // render begin / end / resolve chain
    hipEvent_t get(size_t i)
    {
        while (h->events.size() <= i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            h->events.push_back(e);
        }
        return h->events[i];
    }
    // per-kernel spans only with TRT_FLAG_TIMING; recorded on the stream the kernel is launched on
    size_t mark(hipStream_t stream)
    {
        hipEvent_t e = get(RESERVED + used);
        if (e) (void)hipEventRecord(e, stream);
        return RESERVED + used++;
    }
    void begin(int k, hipStream_t stream) { if (on) spans.push_back({k, mark(stream), 0}); }
    void end(hipStream_t stream) { if (on) spans.back().e1 = mark(stream); }
    template <class F>
    void launch(int k, hipStream_t stream, trt_stats& st, F&& f)
    {
        begin(k, stream);
        f();
        end(stream);
        st.launches[k]++;
    }
};

using ClosestKernel = void (*)(SceneDev, RaySource, f4*, uint32_t, uint32_t*, uint32_t, DeviceStats*, RedoList);
using ShadowKernel = void (*)(SceneDev, ShadowQueue, uint32_t, uint32_t, f4*, uint32_t*, uint32_t, DeviceStats*, uint32_t, RedoList, LightBox);
using FixKernel = void (*)(SceneDev, RaySource, f4*, const f4*, uint32_t, f4*, uint32_t*, uint32_t, RedoList, uint32_t, DeviceStats*);
using ShadeKernel = void (*)(SceneDev, ShadeArgs);
using TailKernel = void (*)(SceneDev, TailArgs);

// Traversal kernels: one set per driver tag (trt_kernels.h: WalkUniform ... WalkOct), the one the scene picked in trt_create.  A kernel family's row
// of a tag is built by one function template, so a new driver is one entry per table and a new family one template.
enum Walk { WALK_UNIFORM, WALK_UNIFORM_FLAGS, WALK_UNIFORM_HIT8, WALK_OCT, WALK_WIDE16, WALK_WIDE_SPILL, N_WALKS };
// traversalOf: the rows of the tables below that a handle runs — `closest` for the kernels that store hit records, `occlusion` for the shadow rays and
// the occlusion query — and whether the closest-hit kernel of its queue is the binned one.  The wave-uniform walk as trt_create set it up: 8-byte
// records with hit8, flags in LDS for the shadow walk with slim_walk.
struct Traversal {
    Walk closest, occlusion;
    bool binned;
};
Traversal traversalOf(const trt_handle* h)
{
    if (h->trace_impl == 0) return {h->hit8 ? WALK_UNIFORM_HIT8 : WALK_UNIFORM, h->slim_walk ? WALK_UNIFORM_FLAGS : WALK_UNIFORM, h->bin_walk};
    const Walk w = h->node_kind == 1 ? WALK_OCT : (h->depth <= 16 ? WALK_WIDE16 : WALK_WIDE_SPILL);
    return {w, w, h->bin_walk};
}
struct ClosestRow { ClosestKernel k[2][3], query; bool redo; };  // [count][primary]; QUERY_CLOSEST; the tag's REDO: k_trace_fix runs behind every launch
struct ShadowRow { ShadowKernel k[2]; ClosestKernel query; bool redo; };  // [count]; QUERY_OCCLUDED
template <class D>
ClosestRow closestRow()
{
    return {{{k_trace_closest<false, D, 0>, k_trace_closest<false, D, 1>, k_trace_closest<false, D, PRIMARY_LIST>},
             {k_trace_closest<true, D, 0>, k_trace_closest<true, D, 1>, k_trace_closest<true, D, PRIMARY_LIST>}},
            k_trace_query<D, QUERY_CLOSEST>, D::REDO};
}
template <class D>
ShadowRow shadowRow()
{
    return {{k_trace_shadow<false, D>, k_trace_shadow<true, D>}, k_trace_query<D, QUERY_OCCLUDED>, D::REDO};
}
// (a form of the wave-uniform walk serves hit records or occlusion, not both: the other table has no row for it)
const ClosestRow closest_rows[N_WALKS] = {closestRow<WalkUniform>(), {}, closestRow<WalkUniformHit8>(), closestRow<WalkOct>(), closestRow<WalkWide16>(), closestRow<WalkWideSpill>()};
const ShadowRow shadow_rows[N_WALKS] = {shadowRow<WalkUniform>(), shadowRow<WalkUniformFlags>(), {}, shadowRow<WalkOct>(), shadowRow<WalkWide16>(), shadowRow<WalkWideSpill>()};
// primary: 0 the queue, 1 the camera rays of a tile, PRIMARY_LIST those of a pixel list.  With h->hit8 the kernel stores 8-byte hit records.
ClosestKernel closestKernel(const trt_handle* h, bool count, int primary)
{
    const Traversal t = traversalOf(h);
    if (t.binned && primary == 0) return count ? k_trace_closest_binned<true> : k_trace_closest_binned<false>;
    return closest_rows[t.closest].k[count][primary];
}
ShadowKernel shadowKernel(const trt_handle* h, bool count) { return shadow_rows[traversalOf(h).occlusion].k[count]; }
// Behind every traversal launch of a per-lane driver: k_trace_fix (a few blocks) traces the rays of the launch's redo list again in the
// exact form (trt_kernels.h, RedoList).  The wave-uniform walk applies the rule on the spot and has no list: nullptr.
FixKernel fixKernel(const trt_handle* h, bool shadow, int primary)
{
    const FixKernel k[4] = {k_trace_fix<false, 0>, k_trace_fix<false, 1>, k_trace_fix<false, PRIMARY_LIST>, k_trace_fix<true, 0>};
    const Traversal t = traversalOf(h);
    return (shadow ? shadow_rows[t.occlusion].redo : closest_rows[t.closest].redo) ? k[shadow ? 3 : primary] : nullptr;
}
// The ray queries (QUERY_CLOSEST, QUERY_OCCLUDED) on the rows of closestKernel / shadowKernel: the same driver, with the counters on (as
// trt_trace_closest); the wave-uniform walk as the render runs it.
ClosestKernel queryKernel(const trt_handle* h, int query)
{
    const Traversal t = traversalOf(h);
    return query == QUERY_OCCLUDED ? shadow_rows[t.occlusion].query : closest_rows[t.closest].query;
}
FixKernel queryFixKernel(const trt_handle* h, int query)
{
    if (!fixKernel(h, query == QUERY_OCCLUDED, 0)) return nullptr;
    return query == QUERY_OCCLUDED ? k_trace_fix<true, 0, QUERY_OCCLUDED> : k_trace_fix<false, 0, QUERY_CLOSEST>;
}
// Bounce 0 of a tile render on a handle with fuse_primary: camera ray, closest hit and shading in one launch
ShadeKernel fusedShadeKernel() { return k_shade<31u, SHADE_ONE, false, TRT_SHADE1_BLOCK, TRT_SHADE1_WAVES, true, true>; }
ShadeKernel shadeKernel(uint32_t tabs, int lights, bool list, bool hit8)
{
    if (hit8) {  // trt_create sets hit8 only with tabs == 31
        const ShadeKernel s[2][5] = {
            {k_shade<31u, SHADE_ONE, false, TRT_SHADE1_BLOCK, TRT_SHADE1_WAVES, true>, k_shade<31u, SHADE_FEW, false, TRT_SHADEN_BLOCK, TRT_SHADEN_WAVES, true>,
             k_shade<31u, SHADE_MANY, false, TRT_SHADEN_BLOCK, TRT_SHADEN_WAVES, true>, k_shade<31u, SHADE_PICK, false, TRT_SHADEP_BLOCK, TRT_SHADEP_WAVES, true>,
             k_shade<31u, SHADE_NEAR, false, TRT_SHADEP_BLOCK, TRT_SHADEP_WAVES, true>},
            {k_shade<31u, SHADE_ONE, true, TRT_SHADE1_BLOCK, TRT_SHADE1_WAVES, true>, k_shade<31u, SHADE_FEW, true, TRT_SHADEN_BLOCK, TRT_SHADEN_WAVES, true>,
             k_shade<31u, SHADE_MANY, true, TRT_SHADEN_BLOCK, TRT_SHADEN_WAVES, true>, k_shade<31u, SHADE_PICK, true, TRT_SHADEP_BLOCK, TRT_SHADEP_WAVES, true>,
             k_shade<31u, SHADE_NEAR, true, TRT_SHADEP_BLOCK, TRT_SHADEP_WAVES, true>}};
        return s[list][lights];
    }
    const ShadeKernel k[5][2][5] = {
        {{k_shade<31u, SHADE_ONE>, k_shade<31u, SHADE_FEW>, k_shade<31u, SHADE_MANY>, k_shade<31u, SHADE_PICK>, k_shade<31u, SHADE_NEAR>},
         {k_shade<31u, SHADE_ONE, true>, k_shade<31u, SHADE_FEW, true>, k_shade<31u, SHADE_MANY, true>, k_shade<31u, SHADE_PICK, true>, k_shade<31u, SHADE_NEAR, true>}},
        {{k_shade<15u, SHADE_ONE>, k_shade<15u, SHADE_FEW>, k_shade<15u, SHADE_MANY>, k_shade<15u, SHADE_PICK>, k_shade<15u, SHADE_NEAR>},
         {k_shade<15u, SHADE_ONE, true>, k_shade<15u, SHADE_FEW, true>, k_shade<15u, SHADE_MANY, true>, k_shade<15u, SHADE_PICK, true>, k_shade<15u, SHADE_NEAR, true>}},
        {{k_shade<7u, SHADE_ONE>, k_shade<7u, SHADE_FEW>, k_shade<7u, SHADE_MANY>, k_shade<7u, SHADE_PICK>, k_shade<7u, SHADE_NEAR>},
         {k_shade<7u, SHADE_ONE, true>, k_shade<7u, SHADE_FEW, true>, k_shade<7u, SHADE_MANY, true>, k_shade<7u, SHADE_PICK, true>, k_shade<7u, SHADE_NEAR, true>}},
        {{k_shade<3u, SHADE_ONE>, k_shade<3u, SHADE_FEW>, k_shade<3u, SHADE_MANY>, k_shade<3u, SHADE_PICK>, k_shade<3u, SHADE_NEAR>},
         {k_shade<3u, SHADE_ONE, true>, k_shade<3u, SHADE_FEW, true>, k_shade<3u, SHADE_MANY, true>, k_shade<3u, SHADE_PICK, true>, k_shade<3u, SHADE_NEAR, true>}},
        {{k_shade<0u, SHADE_ONE>, k_shade<0u, SHADE_FEW>, k_shade<0u, SHADE_MANY>, k_shade<0u, SHADE_PICK>, k_shade<0u, SHADE_NEAR>},
         {k_shade<0u, SHADE_ONE, true>, k_shade<0u, SHADE_FEW, true>, k_shade<0u, SHADE_MANY, true>, k_shade<0u, SHADE_PICK, true>, k_shade<0u, SHADE_NEAR, true>}}};
    return k[tabs == 31u ? 0 : (tabs == 15u ? 1 : (tabs == 7u ? 2 : (tabs == 3u ? 3 : 4)))][list][lights];
}
// (named in this order: named the other way round, k_tail<true, true> / <false, false> build 1 instruction shorter / longer, tools/isa_diff.py)
TailKernel tailKernel(bool count, bool list)
{
    if (list) return count ? k_tail<true, true> : k_tail<false, true>;
    return count ? k_tail<true> : k_tail<false>;
}

void launchTraceClosest(const trt_handle* h, ClosestKernel k, FixKernel fix, hipStream_t stream, uint32_t* spill, const RaySource& src, f4* hit, uint32_t n,
                        DeviceStats* d_stats, RedoList redo)
{
    const dim3 b(TRT_TRACE_BLOCK);
    hipLaunchKernelGGL(k, dim3(h->traceGrid(n)), b, 0, stream, h->sc, src, hit, n, spill, SPILL_STRIDE, d_stats, redo);
    if (fix) hipLaunchKernelGGL(fix, dim3(TRT_FIX_BLOCKS), b, 0, stream, h->sc, src, hit, (const f4*)nullptr, 0u, (f4*)nullptr, spill, SPILL_STRIDE, redo, 0u, d_stats);
}

void launchTraceShadow(const trt_handle* h, ShadowKernel k, FixKernel fix, hipStream_t stream, uint32_t* spill, const ShadowQueue& sq, uint32_t n, uint32_t light_mat,
                       f4* Lacc, DeviceStats* d_stats, uint32_t any, RedoList redo, const LightBox& lbox)
{
    const dim3 b(TRT_TRACE_BLOCK);
    hipLaunchKernelGGL(k, dim3(h->traceGrid(n)), b, 0, stream, h->sc, sq, n, light_mat, Lacc, spill, SPILL_STRIDE, d_stats, any, redo, lbox);
    if (!fix) return;
    const RaySource src{sq.sa, sq.sb, TileDesc{}, 0u};
    hipLaunchKernelGGL(fix, dim3(TRT_FIX_BLOCKS), b, 0, stream, h->sc, src, (f4*)nullptr, (const f4*)sq.sw, light_mat, Lacc, spill, SPILL_STRIDE, redo, any, d_stats);
}

}  // namespace

namespace {
// Everything trt_create derives from the caller's scene on the host — checks, triangle records, the 4-wide and 8-wide collapses, the
// leaf and light boxes, the tuning read from the environment — independent of the device: built once (host threads: trt_wide.h `par`,
// TRT_HOST_THREADS), uploaded to every device of a group (trt_group_create).
struct SceneImage {
    const trt_scene* s = nullptr;
    unsigned threads = 1;
    bool dbg = false;
    uint32_t bvh2_depth = 0;
    int trace_impl = 3;
    int node_kind = 0;
    std::vector<TriIsect> isect;
    std::vector<TriShade> shade;
    WideTree wide;
    OctTree oct;
    std::vector<f4> leaf_boxes;
    std::vector<LightBox> light_boxes;
    std::vector<MaterialDev> mats;
    std::vector<LightDev> lights;
    std::vector<float> light_sel;
    LightTree light_tree;
    std::vector<LightTriDev> ltris;
    std::vector<float> cum;
    bool cum_monotone = true;
    std::vector<TextureDev> tex;
    std::vector<uint8_t> tex_bytes;
    float leaf_alpha = 0.0f;
    float cull_alpha = 0.0f;  // leaf_alpha, or +inf for a tree whose boxes do not nest (SceneDev::cull_alpha)
    std::vector<uint32_t> plane_bits;  // Bloom filter over the box planes (trt_path.h planeMaybe)
    uint32_t plane_lg = 0;
    bool nested = true;
};

struct Lap {  // TRT_DEBUG: where the start-up time of a big scene goes (tools/create_cost.py)
    bool on;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char* what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "trt_create: %-32s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

int buildSceneImage(const trt_scene* s, SceneImage& im)
{
    if (s->n_nodes < 1 || !s->nodes) return fail(TRT_EINVAL, "scene needs at least the root node");
    if (s->n_tris > TRT_MAX_TRIS) return fail(TRT_EINVAL, "too many triangles");
    if (s->n_tris && (!s->tri_v || !s->tri_vn || !s->tri_vt || !s->tri_mat)) return fail(TRT_EINVAL, "null triangle arrays");
    if (s->n_lights > TRT_MAX_SCENE_LIGHTS) return fail(TRT_EINVAL, "more than TRT_MAX_SCENE_LIGHTS (65535) lights");
    if (s->n_materials < 1 || !s->materials) return fail(TRT_EINVAL, "scene needs materials");
    if (s->n_materials >= (1u << 24)) return fail(TRT_EINVAL, "too many materials");
    for (uint32_t i = 0; i < s->n_tris; ++i)
        if (s->tri_mat[i] < 0 || (uint32_t)s->tri_mat[i] >= s->n_materials) return fail(TRT_EINVAL, "triangle material id out of range");
    for (uint32_t i = 0; i < s->n_materials; ++i)
        if (s->materials[i].tex >= (int32_t)s->n_textures) return fail(TRT_EINVAL, "material texture id out of range");
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        const trt_light& L = s->lights[i];
        if (L.mat < 0 || (uint32_t)L.mat >= s->n_materials) return fail(TRT_EINVAL, "light material id out of range");
        if ((uint64_t)L.tri_first + L.tri_count > s->n_light_tris) return fail(TRT_EINVAL, "light triangle range out of bounds");
    }
    for (uint32_t i = 0; i < s->n_textures; ++i)
        if (s->textures[i].width < 1 || s->textures[i].height < 1 || !s->textures[i].rgb) return fail(TRT_EINVAL, "empty texture");
    im.s = s;
    im.dbg = std::getenv("TRT_DEBUG") != nullptr;
    im.threads = par::defaultThreads();
    if (const char* e = std::getenv("TRT_HOST_THREADS")) im.threads = (unsigned)std::min(256, std::max(1, std::atoi(e)));
    Lap lap{im.dbg};
    if (int e = validateBvh(s, &im.bvh2_depth, im.threads)) return e;
    lap("checks, validateBvh");

    // the wave-uniform walk needs a 32-bit reach mask, and it evaluates the nodes in index order: every inner child must
    // come after its parent (all builders here emit parents first; a caller's tree that does not is walked per lane)
    bool tiny = s->n_nodes <= 32 && s->n_tris <= 64;
    for (uint32_t n = 0; tiny && n < s->n_nodes; ++n) {
        const uint32_t ch[2] = {s->nodes[n].child0, s->nodes[n].child1};
        for (uint32_t c : ch)
            if (!(c & TRT_LEAF_BIT) && c <= n) tiny = false;
    }
    im.trace_impl = tiny ? 0 : 3;
    if (const char* e = std::getenv("TRT_TRACE_IMPL")) { if (std::atoi(e) == 3) im.trace_impl = 3; }  // tests: the per-lane driver on a tiny tree too

    // 48-B intersection records and 64-B shading records
    im.isect.resize(s->n_tris);
    im.shade.resize(s->n_tris);
    par::forRange(s->n_tris, im.threads, 65536, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const int32_t mat = s->tri_mat[i];
            im.isect[i] = makeTriIsect(s->tri_v + i * 9, mat, s->materials[mat].is_emissive != 0);
            std::memcpy(im.shade[i].vn, s->tri_vn + i * 9, sizeof(float) * 9);
            std::memcpy(im.shade[i].vt, s->tri_vt + i * 6, sizeof(float) * 6);
            im.shade[i].mat = mat;
        }
    });
    lap("triangle records");
    {   // the 4-wide collapse every per-lane traversal can walk; its stack bound sizes the LDS stack / the spill area
        bool greedy = s->n_tris > 4000000u;  // measured: trt_wide.h
        if (const char* e = std::getenv("TRT_WIDE_GREEDY")) greedy = std::atoi(e) != 0;
        im.wide = greedy ? collapseBvhGreedy(s->nodes, s->n_nodes, im.threads) : collapseBvh(s->nodes, s->n_nodes, im.threads);
        lap("4-wide collapse");
    }
    // the caller's box of every leaf: a hit in front of its own leaf's box does not count (leafEntry(), trt_path.h)
    im.leaf_boxes = leafBoxesOf(s->nodes, s->n_nodes, s->n_tris, im.threads);
    im.light_boxes = lightBoxesOf(im.leaf_boxes, s->tri_mat, s->n_tris, s->lights, s->n_lights);
    if (const char* e = std::getenv("TRT_SHADOW_STOP"))  // 0: all of space as every light's box, i.e. no early end of a shadow ray (A/B)
        if (std::atoi(e) == 0) im.light_boxes.assign(s->n_lights, LightBox{{-3.0e38f, -3.0e38f, -3.0e38f}, {3.0e38f, 3.0e38f, 3.0e38f}});
    im.leaf_alpha = sceneLeafAlpha(s->nodes, s->n_nodes);
    // Culling by distance rests on nested boxes; a foreign tree that breaks the premise is walked without it (every box the ray passes is entered, bvh.cpp:162-166)
    im.nested = wide_detail::boxesNested(s->nodes, s->n_nodes, im.threads);
    im.cull_alpha = im.nested ? im.leaf_alpha : std::numeric_limits<float>::infinity();
    im.plane_lg = wide_detail::planeFilterBuild(s->nodes, s->n_nodes, im.plane_bits, im.threads);
    if (im.dbg && !im.nested) std::fprintf(stderr, "[trt] the boxes of this tree do not nest: traversal without distance culling\n");
    lap("leaf boxes, light boxes");
    // The 8-wide compressed nodes (trt_oct.h) for the persistent traversal kernels, when the tree qualifies (nested, finite; larger
    // leaves are laid out as several slots with the leaf's own box): TRT_NODE_KIND=0/1 in the environment forces either kind (A/B runs, tests).
    bool want_oct = im.trace_impl != 0 && TRT_DEFAULT_NODE_KIND == 1;
    if (const char* e = std::getenv("TRT_NODE_KIND")) want_oct = im.trace_impl != 0 && std::atoi(e) == 1;
    if (want_oct) {
        im.oct = buildOct(s->nodes, s->n_nodes, s->n_tris, im.isect.data(), im.threads);
        im.node_kind = im.oct.ok ? 1 : 0;
        lap("8-wide collapse");
        if (im.dbg) std::fprintf(stderr, "trt_create: oct tree %s (%s): %zu nodes, %u levels, %u leaves of more than 3 triangles split\n", im.oct.ok ? "built" : "not built", im.oct.why, im.oct.nodes.size(), im.oct.levels, im.oct.split_leaves);
    }
    if (im.dbg) std::fprintf(stderr, "trt_create: %zu wide nodes, node kind %d, stack need %u, %u host threads\n", im.wide.nodes.size(), im.node_kind, im.wide.stack_need, im.threads);

    im.mats.resize(s->n_materials);
    for (uint32_t i = 0; i < s->n_materials; ++i) im.mats[i] = makeMaterialDev(s->materials[i]);
    im.lights.resize(s->n_lights);
    for (uint32_t i = 0; i < s->n_lights; ++i) im.lights[i] = makeLightDev(s->lights[i], s->materials);
    im.light_sel.resize(s->n_lights);  // TRT_FLAG_ONE_LIGHT: the running sums of the selection weights (lightPick, trt_path.h)
    lightSelTable(im.lights.data(), s->n_lights, im.light_sel.data());
    im.ltris.resize(s->n_light_tris);
    for (uint32_t i = 0; i < s->n_light_tris; ++i) im.ltris[i] = makeLightTriDev(s->light_tris[i]);
    buildLightTree(im.lights.data(), s->n_lights, im.ltris.data(), s->n_light_tris, im.light_tree);  // TRT_FLAG_NEAR_LIGHTS (lightPickNear, trt_path.h)
    // packed CDF for the bisection in lightSample; only when every light's CDF is non-decreasing and NaN-free
    im.cum.resize(s->n_light_tris);
    for (uint32_t k = 0; k < s->n_light_tris; ++k) im.cum[k] = s->light_tris[k].cum_area;
    for (uint32_t l = 0; l < s->n_lights; ++l)
        for (uint32_t k = 0; k < s->lights[l].tri_count; ++k) {
            const float c = im.cum[s->lights[l].tri_first + k];
            if (!(c == c) || (k && c < im.cum[s->lights[l].tri_first + k - 1])) im.cum_monotone = false;
        }
    im.tex.resize(s->n_textures);
    for (uint32_t i = 0; i < s->n_textures; ++i) {
        im.tex[i].width = s->textures[i].width;
        im.tex[i].height = s->textures[i].height;
        im.tex[i].offset = im.tex_bytes.size();
        const size_t nb = (size_t)im.tex[i].width * im.tex[i].height * 3;
        im.tex_bytes.insert(im.tex_bytes.end(), s->textures[i].rgb, s->textures[i].rgb + nb);
    }
    return TRT_OK;
}

// The device half of trt_create: a handle on `device` from the host image (thread-safe against other devices' calls: touches only
// the handle, the image read-only and this thread's HIP device).
// Makes `device` current after checking that it exists and is a gfx950 (TRT_ENODEV otherwise).
int useDevice(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(TRT_ENODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(TRT_ENODEV, "device ordinal out of range");
    HIPC(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(TRT_ENODEV, std::string("this library is built for gfx950 only, device is ") + prop.gcnArchName);
    return TRT_OK;
}

// The tables k_shade stages, copied into the handle's packed image in LDS layout (trt_create; again after trt_update_geometry rewrote them).
int packLdsImage(trt_handle* h, hipStream_t stream)
{
    const void* src[5] = {h->sc.materials, h->sc.lights, h->sc.light_cum, h->sc.light_tris, h->sc.tri_shade};
    size_t off = 0;
    for (int k = 0; k < 5; ++k)
        if (h->shade_tabs >> k & 1u) {
            const size_t padded = (h->lds_tab[k] + 15u) & ~15u;  // upload() padded the source the same way
            HIPC(hipMemcpyAsync((char*)h->lds_image + off, src[k], padded, hipMemcpyDeviceToDevice, stream));
            off += padded;
        }
    HIPC(hipStreamSynchronize(stream));
    return TRT_OK;
}

int createOnDevice(const SceneImage& im, int device, trt_handle** out)
{
    const trt_scene* s = im.s;
    if (int e = useDevice(device)) return e;

    Lap lap{im.dbg};
    std::unique_ptr<trt_handle> h(new trt_handle);
    h->device = device;
    h->bvh2_depth = im.bvh2_depth;
    if (const char* e = std::getenv("TRT_TAIL_N")) h->tail_n = (uint32_t)std::strtoul(e, nullptr, 10);
    h->sc.refill_min = s->n_tris <= 200000u ? 48u : 32u;
    // a triangle step costs about half a node step: deep trees run it already when 2 lanes at nodes face 3 at leaves
    // (blob-2M, soup-1M -2.6 % per step; the cg22 scenes are 0.7 % better off with the plain majority)
    h->sc.sched_in_w = s->n_tris <= 200000u ? 1u : 2u;
    h->sc.sched_lf_w = s->n_tris <= 200000u ? 1u : 3u;
    if (const char* e = std::getenv("TRT_SCHED_W")) {  // "in:leaf" weights of the scheduler driver (tuning)
        unsigned a = 0, b = 0;
        if (std::sscanf(e, "%u:%u", &a, &b) == 2 && a > 0 && b > 0 && a < 1024 && b < 1024) { h->sc.sched_in_w = a; h->sc.sched_lf_w = b; }
    }
    // leaf steps of the oct driver: two triangles each on trees with leaves of <= 3; a tree whose leaves were split into several slots
    // (the reference's leaf size 8) brings up to 24 triangles per node, all of which have to be tested: four per step there
    // (profiles/r04_leaf8.txt has the sweep)
    h->sc.leaf_loop = im.oct.split_leaves * 8u > s->n_tris / 8u ? 4u : 2u;  // at least an eighth of the triangles in such leaves (8 per leaf assumed)
    if (const char* e = std::getenv("TRT_LEAF_LOOP")) h->sc.leaf_loop = std::min(24u, std::max(1u, (uint32_t)std::strtoul(e, nullptr, 10)));
    if (const char* e = std::getenv("TRT_REFILL_MIN")) h->sc.refill_min = std::min(64u, std::max(1u, (uint32_t)std::strtoul(e, nullptr, 10)));
    if (im.dbg) std::fprintf(stderr, "trt_create: refill_min %u tail_n %u\n", h->sc.refill_min, h->tail_n);
    if (const char* e = std::getenv("TRT_TRACE_RPW")) h->rays_per_wave = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char* e = std::getenv("TRT_TRACE_FILLB")) h->fill_blocks = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char* e = std::getenv("TRT_TRACE_MAXB")) h->max_blocks = std::max(8u, (uint32_t)std::strtoul(e, nullptr, 10));
    h->trace_impl = im.trace_impl;
    h->node_kind = im.node_kind;
    h->oct_levels = im.oct.levels;
    h->dbg = im.dbg;
    h->depth = im.wide.stack_need + 1;
    h->light_boxes = im.light_boxes;

    if (int e = upload(h.get(), im.isect.data(), im.isect.size(), &h->sc.tri_isect)) return e;
    if (int e = upload(h.get(), im.plane_bits.data(), im.plane_bits.size(), &h->sc.plane_bits)) return e;
    h->sc.plane_shift = 32u - im.plane_lg;
    if (int e = upload(h.get(), im.shade.data(), im.shade.size(), &h->sc.tri_shade)) return e;
    if (int e = upload(h.get(), s->nodes, (size_t)s->n_nodes, &h->sc.nodes)) return e;
    h->sc.n_wnodes = (uint32_t)im.wide.nodes.size();
    if (int e = upload(h.get(), im.leaf_boxes.data(), im.leaf_boxes.size(), &h->sc.leaf_box)) return e;
    if (int e = upload(h.get(), im.wide.nodes.data(), im.wide.nodes.size(), &h->sc.wnodes)) return e;
    h->sc.onodes = nullptr;
    h->sc.tri_trav = nullptr;
    if (im.node_kind == 1) {
        h->sc.n_onodes = (uint32_t)im.oct.nodes.size();
        if (int e = upload(h.get(), im.oct.nodes.data(), im.oct.nodes.size(), &h->sc.onodes)) return e;
        if (int e = upload(h.get(), im.oct.tri_trav.data(), im.oct.tri_trav.size(), &h->sc.tri_trav)) return e;
        h->n_tri_trav = (uint32_t)im.oct.tri_trav.size();
    }
    if (int e = upload(h.get(), im.mats.data(), im.mats.size(), &h->sc.materials)) return e;
    if (int e = upload(h.get(), im.lights.data(), im.lights.size(), &h->sc.lights)) return e;
    if (int e = upload(h.get(), im.ltris.data(), im.ltris.size(), &h->sc.light_tris)) return e;
    h->sc.light_cum = nullptr;
    if (im.cum_monotone)
        if (int e = upload(h.get(), im.cum.data(), im.cum.size(), &h->sc.light_cum)) return e;
    h->sc.light_sel = nullptr;  // (fewer than two lights: nothing is ever picked)
    if (s->n_lights >= 2)
        if (int e = upload(h.get(), im.light_sel.data(), im.light_sel.size(), &h->sc.light_sel)) return e;
    // the light tree of TRT_FLAG_NEAR_LIGHTS: room for the n_lights - 1 nodes any later light table of this handle can need (trt_update_geometry keeps n_lights)
    h->sc.light_nodes = nullptr;
    h->sc.n_light_nodes = 0u;
    h->sc.light_root = TRT_LIGHT_NONE;
    if (s->n_lights >= 2) {
        std::vector<LightNode> nodes(im.light_tree.nodes);
        nodes.resize(s->n_lights - 1u, LightNode{});
        if (int e = upload(h.get(), nodes.data(), nodes.size(), &h->sc.light_nodes)) return e;
        h->sc.n_light_nodes = (uint32_t)im.light_tree.nodes.size();
        h->sc.light_root = im.light_tree.root;
    }
    if (int e = upload(h.get(), im.tex.data(), im.tex.size(), &h->sc.textures)) return e;
    if (int e = upload(h.get(), im.tex_bytes.data(), im.tex_bytes.size(), &h->sc.tex_bytes)) return e;
    lap("uploads");
    h->sc.n_tris = s->n_tris;
    h->sc.n_nodes = s->n_nodes;
    h->sc.n_lights = s->n_lights;
    h->n_materials = s->n_materials;
    h->n_light_tris = s->n_light_tris;
    if (const char* e = std::getenv("TRT_SHADOW_STOP")) h->light_boxes_fixed = std::atoi(e) == 0;
    h->sc.light0_area = s->n_lights ? s->lights[0].area : 0.0f;
    h->sc.leaf_alpha = im.leaf_alpha;
    h->sc.cull_alpha = im.cull_alpha;
    h->sc.cam = s->camera;
    for (uint32_t i = 0; i < s->n_lights; ++i) h->light_mats.push_back((uint32_t)s->lights[i].mat);
    {   // which small tables k_shade copies into LDS: in this order while they fit (uploads are padded to 16 B)
        // the per-triangle shading records only for scenes of a few dozen triangles (every block pays for the copy)
        const uint32_t want[5] = {(uint32_t)(s->n_materials * sizeof(MaterialDev)), (uint32_t)(s->n_lights * sizeof(LightDev)),
                                  h->sc.light_cum ? (uint32_t)(s->n_light_tris * sizeof(float)) : 0u, (uint32_t)(s->n_light_tris * sizeof(LightTriDev)),
                                  s->n_tris <= 64 ? (uint32_t)(s->n_tris * sizeof(TriShade)) : 0u};
        uint32_t used = 0;
        for (int k = 0; k < 5; ++k) {
            const uint32_t padded = (want[k] + 15u) & ~15u;
            if (want[k] && used + padded <= TRT_SHADE_LDS_TABLE_BYTES) { h->lds_tab[k] = want[k]; used += padded; }
        }
        if (std::getenv("TRT_SHADE_NO_LDS")) h->lds_tab[0] = h->lds_tab[1] = h->lds_tab[2] = h->lds_tab[3] = h->lds_tab[4] = 0;
        if (std::getenv("TRT_SHADE_NO_LDS_TRIS")) h->lds_tab[4] = 0;
        // k_shade is instantiated for these sets of staged tables; take the largest one that fits
        uint32_t have = 0;
        for (int k = 0; k < 5; ++k) have |= h->lds_tab[k] ? (1u << k) : 0u;
        h->shade_tabs = 0;
        for (uint32_t m : {31u, 15u, 7u, 3u})
            if ((have & m) == m) { h->shade_tabs = m; break; }
        if (im.dbg)
            std::fprintf(stderr, "trt_create: k_shade tables %u (lds bytes: materials %u, lights %u, cdf %u, light tris %u, shading tris %u)\n", h->shade_tabs,
                         h->lds_tab[0], h->lds_tab[1], h->lds_tab[2], h->lds_tab[3], h->lds_tab[4]);
        // the staged tables once more, packed in LDS layout: a block fetches them with one coalesced pass
        size_t total = 0;
        for (int k = 0; k < 5; ++k)
            if (h->shade_tabs >> k & 1u) total += (h->lds_tab[k] + 15u) & ~15u;
        if (total) {
            void* img = nullptr;
            HIPC(hipMalloc(&img, total));
            h->scene_allocs.push_back(img);
            h->lds_image = img;
            h->lds_image_bytes = (uint32_t)total;
            if (int e = packLdsImage(h.get(), nullptr)) return e;
        }
    }
    h->slim_walk = h->trace_impl == 0 && s->n_tris <= 64;  // (trace_impl 0 implies <= 64 triangles: the LDS copies of trt_kernels.h hold 64)
    if (const char* e = std::getenv("TRT_SLIM_WALK")) h->slim_walk = h->slim_walk && std::atoi(e) != 0;
    h->hit8 = h->slim_walk && h->shade_tabs == 31u;
    h->bin_walk = h->hit8;  // (the flags in LDS and the 8-byte records: what traceQueueBinned's kernel is built for)
    if (const char* e = std::getenv("TRT_BIN_WALK")) h->bin_walk = h->bin_walk && std::atoi(e) != 0;
    if (im.dbg) std::fprintf(stderr, "trt_create: slim walk %d, 8-byte hit records %d, binned walk %d\n", (int)h->slim_walk, (int)h->hit8, (int)h->bin_walk);
    h->fuse_primary = h->hit8 && s->n_lights == 1;  // (k_shade's one-light flavour on the 8-byte records: what the FUSE kernel is built for)
    if (const char* e = std::getenv("TRT_FUSE_PRIMARY")) h->fuse_primary = h->fuse_primary && std::atoi(e) != 0;
    if (im.dbg) std::fprintf(stderr, "trt_create: fused primary %d\n", (int)h->fuse_primary);
    h->root_known = s->n_nodes > 0 && s->nodes != nullptr;
    if (h->root_known) h->root_node = s->nodes[0];
    if (const char* e = std::getenv("TRT_CULL_PRIMARY")) h->cull_primary = std::atoi(e) != 0;
    if (im.dbg) std::fprintf(stderr, "trt_create: cull primary %d\n", (int)h->cull_primary);

    // traversal spill area: levels beyond the LDS stack, for the largest grid
    // (k_trace_fix / k_tail walk the caller's BVH2 itself for the rays of raySpecial(), trt_path.h: one entry per level of it)
    const uint32_t stack_levels = std::max(h->depth, h->bvh2_depth + 2u);
    uint32_t spill_levels = stack_levels > (uint32_t)TRT_LDS_STACK_MAX ? stack_levels - TRT_LDS_STACK_MAX + 1 : 1;
    if (h->node_kind == 1 && h->oct_levels > OCT_LDS_LEVELS) spill_levels = std::max(spill_levels, 2u * (h->oct_levels - OCT_LDS_LEVELS + 1));  // two words per level
    h->spill_words_per_slot = (size_t)spill_levels * SPILL_STRIDE;
    if (int e = h->spill.ensure(h->spill_words_per_slot * 2 * sizeof(uint32_t))) return e;  // one area per concurrent pass
    for (hipStream_t& st : h->slot_streams) HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->side_events) HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (const char* e = std::getenv("TRT_SHADOW_STREAM")) h->shadow_stream = std::atoi(e) != 0;
    for (const MaterialDev& m : im.mats) h->refracts = h->refracts || m.Ni > 1.0f;
    if (const char* e = std::getenv("TRT_DEBUG_SCHEDULE")) h->dbg_sched = im.dbg && std::atoi(e) != 0;
    if (im.dbg) std::fprintf(stderr, "trt_create: shadow stream %d\n", (int)h->shadow_stream);
    h->count_rows = countRows(h->sc.n_lights);
    const size_t pinned_words = 2 * (2 * (size_t)h->count_rows + 16);  // per slot: counters + sequence word
    HIPC(hipHostMalloc((void**)&h->pinned_counts, pinned_words * sizeof(uint32_t), hipHostMallocDefault));
    std::memset(h->pinned_counts, 0, pinned_words * sizeof(uint32_t));  // sequence words start at 0; the first one asked for is 1
    if (const char* e = std::getenv("TRT_SLOTS")) h->n_slots = std::atoi(e) >= 2 ? 2 : 1;
    if (const char* e = std::getenv("TRT_TEST_FAIL_AT_BOUNCE")) h->fail_at_bounce = std::atoi(e);
    if (const char* e = std::getenv("TRT_SHADE_PAD_LDS")) {
        h->shade_pad_lds = std::min(100000u, (uint32_t)std::strtoul(e, nullptr, 10));
        // more than 64 KiB per block needs the opt-in; a refusal shows as a launch error, not as a silent no-op
        for (uint32_t tabs : {31u, 15u, 7u, 3u, 0u})
            for (bool list : {false, true})
                for (int lights : {SHADE_ONE, SHADE_FEW, SHADE_MANY, SHADE_PICK, SHADE_NEAR})
                    for (bool hit8 : {false, true})
                        if (!hit8 || tabs == 31u)
                            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(shadeKernel(tabs, lights, list, hit8)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->shade_pad_lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fusedShadeKernel()), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->shade_pad_lds);
    }

    *out = h.release();
    return TRT_OK;
}
}  // namespace

extern "C" {

const char* trt_last_error(void) { return g_err.c_str(); }
int trt_abi_version(void) { return TRT_ABI_VERSION; }

int trt_rows_selected(const trt_params* p)
{
    if (!p) return -1;
    int n = 0;
    for (int y = p->y0; y < p->y1; ++y) n += rowSelected(p, y) ? 1 : 0;
    return n;
}

int trt_create(const trt_scene* s, int device, trt_handle** out)
{
    if (!s || !out) return fail(TRT_EINVAL, "trt_create: null argument");
    *out = nullptr;
    SceneImage im;
    if (int e = buildSceneImage(s, im)) return e;
    return createOnDevice(im, device, out);
}

void trt_destroy(trt_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

// One pass = all bounces of `sc_count` samples of every pixel of the tile.  Up to N_SLOTS passes are in
// flight at once, each on its own stream with its own queues: while one pass sits in the latency-bound
// shade kernel or in the host round trip that reads the queue lengths back, the other keeps the CUs busy
// with traversal.  Passes are independent (every sample has its own RNG stream and its own Lacc entry);
// only the per-pixel accumulation is ordered, so the resolves are issued strictly in pass order.
namespace {
constexpr int N_SLOTS = 2;
struct PassSlot {
    hipStream_t stream = nullptr;
    RayQueue Q[2];
    f4* hit = nullptr;
    f4* Lacc = nullptr;
    ShadowArena shadow{nullptr, 0};   // the shadow queues of every light
    uint32_t* d_counts = nullptr;
    uint32_t* host_counts = nullptr;  // pinned, device-visible: 2 * count_rows counters + the sequence word
    uint32_t seq = 0;                 // last sequence number asked for
    uint32_t* spill = nullptr;
    RedoList redo{nullptr, nullptr};  // rays the traversal kernels hand to k_trace_fix (trt_kernels.h)
    enum State { IDLE, PACK, PACKWAIT, ISSUE, WAIT, RESOLVE } state = IDLE;  // PACK / PACKWAIT: trt_render_rays only (the caller's rays into the queue)
    uint32_t chunk = 0, s0 = 0, sc_count = 0, n_active = 0, b = 0;
    int cur = 0;
    // two-ended shadow queues (trt_sched.h): where this bounce's k_shade writes its records, the interval the latest shadow launches read, and
    // the event behind them while the pass's stream has not yet waited for it
    uint64_t sq_at = 0, rd_at = 0, rd_n = 0;
    int side_ev = -1;
};
// Path ids of one pass run up to 0x7FFF0000 (the queue lengths of k_shade): one sample of every listed pixel must fit.
constexpr uint32_t MAX_PASS_PATHS = 0x7FFF0000u;

// A pass slot's share of the arena, the one statement of a path's footprint: arrays of N 16-B records in this order — two ray queues
// (ra, rb, bt each), the hits, Lacc, three per light (its shadow queue: ShadowArena::queue) — then the redo list, one index per path.
struct SlotLayout {
    static constexpr uint64_t arrays(uint32_t nl) { return 3 * 2 + 1 + 1 + 3ull * nl; }
    static constexpr uint64_t bytesPerPath(uint32_t nl) { return arrays(nl) * sizeof(f4) + sizeof(uint32_t); }
    static size_t bytes(uint64_t N, uint32_t nl) { return (size_t)(N * arrays(nl) + (N + 3) / 4) * sizeof(f4); }  // the redo list in whole 16-B words
    static void carve(PassSlot& S, f4* base, uint64_t N, uint32_t nl)
    {
        auto take = [&](uint64_t k) { f4* r = base; base += k * N; return r; };
        for (RayQueue& q : S.Q) { q.ra = take(1); q.rb = take(1); q.bt = take(1); }
        S.hit = take(1);
        S.Lacc = take(1);
        S.shadow = ShadowArena{take(3 * nl), N};
        S.redo.idx = (uint32_t*)base;
    }
};

// A trt_render_aov pass's share of the arena: N hit records of 16 B (the wave-uniform walk writes 8-byte ones into the first half), then the
// redo list, one index per path.  One pass at a time (TRT_FLAG_OVERLAP does not apply).
struct AovLayout {
    static constexpr uint64_t bytes_per_path = sizeof(f4) + sizeof(uint32_t);
    static size_t bytes(uint64_t N, uint32_t) { return (size_t)(N + (N + 3) / 4) * sizeof(f4); }
    static void carve(f4* base, uint64_t N, f4*& hit, uint32_t*& redo_idx)
    {
        hit = base;
        redo_idx = (uint32_t*)(base + N);
    }
};

// A trt_aov_rays pass's share of the arena: the packed rays (ra, rb: 32 B), the hit records (16 B; the wave-uniform walk writes 8-byte ones
// into the first half), then the redo list, one index per path: TRT_AOV_RAYS_BYTES_PER_PATH.  One pass at a time.
struct AovRaysLayout {
    static constexpr uint64_t bytes_per_path = 3 * sizeof(f4) + sizeof(uint32_t);
    static_assert(bytes_per_path == TRT_AOV_RAYS_BYTES_PER_PATH, "include/trt.h states the figure");
    static size_t bytes(uint64_t N, uint32_t) { return (size_t)(3 * N + (N + 3) / 4) * sizeof(f4); }
    static void carve(f4* base, uint64_t N, f4*& ra, f4*& rb, f4*& hit, uint32_t*& redo_idx)
    {
        ra = base;
        rb = base + N;
        hit = base + 2 * N;
        redo_idx = (uint32_t*)(base + 3 * N);
    }
};

// How a render call splits its samples into passes: `slots` passes in flight at once, each of `chunk` samples of every pixel (the last one
// may hold fewer), N paths and slot_bytes of arena.  Passes are as large as the budget allows: every pass ends in a tail of few, long paths,
// so fewer and larger passes are faster (back 1080p x 256 spp: 3 passes in 32 GiB 101.4 ms, 1 pass in 93 GB 96.8 ms); >= slots_wanted
// passes when the samples allow.  planPasses is false when the budget holds less than one sample of every pixel.
// fp: what a path of the call occupies (SlotLayout for a render, AovLayout for trt_render_aov).
struct PassPlan { int slots; uint32_t chunk, n_chunks; uint64_t N; size_t slot_bytes; };
struct Footprint {
    int max_slots;                             // passes in flight at once
    uint64_t per_path;                         // bytes of arena per path
    size_t (*bytes)(uint64_t N, uint32_t nl);  // the arena of a pass of N paths
    const char* stated;                        // the figure as include/trt.h states it (TRT_ENOMEM's text)
};
Footprint renderFootprint(uint32_t nl)
{
    return Footprint{N_SLOTS, SlotLayout::bytesPerPath(nl), SlotLayout::bytes, "132 + 48 * n_lights bytes per path, 132 + 48 with TRT_FLAG_ONE_LIGHT"};
}
Footprint aovFootprint() { return Footprint{1, AovLayout::bytes_per_path, AovLayout::bytes, "20 bytes per path"}; }
Footprint aovRaysFootprint() { return Footprint{1, AovRaysLayout::bytes_per_path, AovRaysLayout::bytes, "52 bytes per path"}; }
bool planPasses(uint32_t npix, uint32_t n_samples, uint32_t nl, uint64_t budget, int slots_wanted, const Footprint& fp, PassPlan& pl)
{
    const uint64_t cap_paths = std::min<uint64_t>(budget / fp.per_path, MAX_PASS_PATHS);
    uint64_t max_paths = cap_paths;
    if (max_paths < npix) return false;
    if (slots_wanted > 1 && max_paths / slots_wanted >= npix) max_paths /= slots_wanted;  // each slot gets its share of the budget
    pl.slots = (max_paths * slots_wanted <= cap_paths) ? slots_wanted : 1;
    pl.chunk = (uint32_t)std::min<uint64_t>((uint64_t)n_samples, max_paths / npix);
    pl.n_chunks = (n_samples + pl.chunk - 1) / pl.chunk;
    if (pl.slots > 1 && pl.n_chunks < (uint32_t)pl.slots) pl.n_chunks = std::min<uint32_t>((uint32_t)pl.slots, n_samples);
    pl.chunk = (n_samples + pl.n_chunks - 1) / pl.n_chunks;
    pl.n_chunks = (n_samples + pl.chunk - 1) / pl.chunk;
    pl.N = (uint64_t)npix * pl.chunk;
    pl.slot_bytes = fp.bytes(pl.N, nl);
    return true;
}

// Offsets of a buffer's regions, in the order they are added, each at the alignment it asks for.
struct Layout {
    size_t bytes = 0;
    size_t add(size_t n, size_t align)
    {
        const size_t at = (bytes + align - 1) & ~(align - 1);
        bytes = at + n;
        return at;
    }
};

// What one render call traces, and where its per-pixel sums come from and go.  A tile (trt_render*): its selected rows; the sums are the
// caller's host accumulator (in/out) or, without one, start at zero and are dropped; out_dev receives them rounded to float.  A pixel list
// (trt_render_pixels*) of the whole image: pixels, sum and sumsq (may be null) are host arrays (`host`, staged) or device arrays used in place.
// Caller-supplied rays (trt_render_rays*): a list whose entries are the stream ids (`pixels`; null = 0..npix-1, filled on the device) and whose
// bounce-0 rays come from org / dir [samples of the call][npix][3] instead of the camera (host arrays are staged pass by pass).
struct RenderInput {
    bool list = false, host = true, rays = false;
    const float* org = nullptr;
    const float* dir = nullptr;
    std::vector<int32_t> rows;
    const uint32_t* pixels = nullptr;
    uint32_t npix = 0;
    int32_t tile_w = 0, x0 = 0;  // TileDesc
    double* sum = nullptr;
    double* sumsq = nullptr;
    float* out_dev = nullptr;
};

// TRT_FLAG_ONE_LIGHT takes effect on scenes of two or more lights (include/trt.h): the call then has ONE shadow queue whatever the light count
inline bool picksOneLight(const trt_handle* h, const trt_params* p) { return (p->flags & TRT_FLAG_ONE_LIGHT) != 0 && h->sc.n_lights >= 2u; }
// TRT_FLAG_NEAR_LIGHTS: that one light by a descent of the light tree (checkEstimator has seen to TRT_FLAG_ONE_LIGHT)
inline bool picksNearLight(const trt_handle* h, const trt_params* p) { return picksOneLight(h, p) && (p->flags & TRT_FLAG_NEAR_LIGHTS) != 0; }

// The arguments of k_shade that every bounce of a render call shares, its TileDesc among them (d_table: the row table or the list on the device)
ShadeArgs shadeArgsOf(const trt_handle* h, const trt_params* p, const RenderInput& in, const void* d_table, uint32_t rows_lds, DeviceStats* d_stats)
{
    ShadeArgs A;
    TileDesc& td = A.td;
    td.rows = (const int32_t*)d_table;
    td.tile_w = in.tile_w;
    td.x0 = in.x0;
    td.width = p->width;
    td.height = p->height;
    td.npix = in.npix;
    td.seed = p->seed;
    td.spp = (uint32_t)p->spp;
    td.fixed_nee = (p->flags & TRT_FLAG_FIXED_NEE) ? 1u : 0u;
    td.fixed_pixels = (p->flags & TRT_FLAG_FIXED_PIXELS) ? 1u : 0u;
    td.ray_offset = (p->flags & TRT_FLAG_RAY_OFFSET) ? 1u : 0u;
    td.specular_ks = (p->flags & TRT_FLAG_SPECULAR_KS) ? 1u : 0u;
    td.one_light = picksOneLight(h, p) ? 1u : 0u;
    td.near_lights = picksNearLight(h, p) ? 1u : 0u;
    td.npix_magic = magicOf(in.npix);
    td.tile_w_magic = magicOf((uint32_t)td.tile_w);
    td.grid_ok = (p->width >= 2 && p->height >= 2 && p->width <= 65536 && p->height <= 65536) ? 1u : 0u;
    td.grid_rcp[0] = 1.0 / double(p->width - 1.0);
    td.grid_rcp[1] = 1.0 / double(p->height - 1.0);
    td.grid_rcp[2] = 1.0 / double(p->width);
    td.grid_rcp[3] = 1.0 / double(p->height);
    for (int32_t& c : td.cull) c = 0;  // nothing culled: renderCore sets it for the calls that cull
    A.shadow_count_stride = COUNT_STRIDE;
    A.max_depth = p->max_depth;
    A.lds_mat_bytes = h->lds_tab[0];
    A.lds_light_bytes = h->lds_tab[1];
    A.lds_cum_bytes = h->lds_tab[2];
    A.lds_ltri_bytes = h->lds_tab[3];
    A.lds_tshade_bytes = h->lds_tab[4];
    A.lds_image = (const f4*)h->lds_image;
    A.lds_image_words = h->lds_image_bytes / 16u;
    A.rows_lds = rows_lds;
    A.stats = d_stats;
    return A;
}

// The queue lengths of the slot's bounce: spin on the sequence word the device writes after them; the stream is the fallback (and the error path)
int awaitCounts(const PassSlot& S, uint32_t count_rows)
{
    volatile uint32_t* flag = (volatile uint32_t*)S.host_counts + 2 * count_rows;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t spins = 0;
    while (*flag != S.seq) {
        if ((++spins & 0x3FFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            HIPC(hipStreamSynchronize(S.stream));  // long kernels: let the runtime wait; also surfaces a device error
            if (*flag != S.seq) return fail(TRT_EHIP, "queue lengths did not arrive");
            break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return TRT_OK;
}

void addDeviceStats(trt_stats& st, const DeviceStats& ds, const trt_handle* h)
{
    st.shaded_hits = ds.shaded_hits;
    st.wave_steps[0] = ds.wave_inner_steps;
    st.wave_steps[1] = ds.wave_leaf_steps;
    st.rays_shadow += ds.tail_rays_shadow;
    st.rays_indirect += ds.tail_rays_indirect;
    for (int i = 0; i < 2; ++i) { st.inner_visits[i] = ds.inner_visits[i]; st.tri_tests[i] = ds.tri_tests[i]; }
    st.max_bounces = ds.max_depth_hit;
    st.redo_rays = ds.redo_rays;
    st.lane_census[0] = ds.census_inner; st.lane_census[1] = ds.census_leaf; st.lane_census[2] = ds.census_done; st.lane_census[3] = ds.census_iters;
    st.inner_node_bytes = h->trace_impl == 0 ? (uint32_t)sizeof(trt_bvh_node) : (h->node_kind == 1 ? 80u : (uint32_t)sizeof(WideNode));
}

// The drain of a call with work in flight: from arm() on, whatever way the driver is left, nothing may still be running on the caller's
// stream, the slot streams or the handle's side stream when it returns (a late kernel or copy of a failed call would write what the NEXT call on the handle uses, or
// host memory that died with the return).  The destructor synchronises them unless the driver got through and disarmed it.  A driver
// declares it after every host end of an asynchronous copy, so that it is destroyed before them.  `slots` outlive the drain.
struct Drain {
    hipStream_t stream;
    hipStream_t side;  // the handle's side stream (shadow walks of a render): whatever the call was, nothing of the handle's may be left running on it
    PassSlot* slots = nullptr;
    int n_slots = 0;
    bool armed = false;
    Drain(hipStream_t stream_, const trt_handle* h) : stream(stream_), side(h->side_stream) {}
    Drain(const Drain&) = delete;
    void arm(PassSlot* s = nullptr, int n = 0) { slots = s; n_slots = n; armed = true; }
    ~Drain()
    {
        if (!armed) return;
        for (int k = 0; k < n_slots; ++k) (void)hipStreamSynchronize(slots[k].stream);
        if (side) (void)hipStreamSynchronize(side);
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
};

// The frame of a call that traces rays, at its start and its end only: the Timer and the trt_stats the call fills, the block of device
// counters (DeviceStats first) it clears and reads back, the events that bracket it on the caller's stream, and the Drain (the last member:
// it runs before `ds`, the landing place of readBack()'s copy, goes away), armed by begin() or arm() and disarmed by finish().  The
// destructor keeps the slots' sequence numbers monotonic on every way out.
struct CallFrame {
    trt_handle* h;
    Timer tm;
    trt_stats st{};
    DeviceStats* d_stats = nullptr;
    DeviceStats ds;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_resolved = nullptr;  // events 0/1 bracket the call on the stream, 2 chains renderCore's ordered resolves
    Drain drain;
    CallFrame(trt_handle* h_, hipStream_t stream_, bool timing) : h(h_), tm{h_, timing}, drain(stream_, h_) {}
    // the counters: `bytes` from the DeviceStats at `block` on
    int clear(void* block, size_t bytes) { d_stats = (DeviceStats*)block; HIPC(hipMemsetAsync(block, 0, bytes, drain.stream)); return TRT_OK; }
    void arm() { drain.arm(); }
    int begin(PassSlot* s = nullptr, int n = 0)  // the bracket opens, then the drain is armed; with slots there is a resolve chain
    {
        ev_begin = tm.get(0);
        ev_end = tm.get(1);
        if (s) ev_resolved = tm.get(2);
        if (!ev_begin || !ev_end || (s && !ev_resolved)) return fail(TRT_EHIP, "hipEventCreate failed");
        HIPC(hipEventRecord(ev_begin, drain.stream));
        drain.arm(s, n);
        return TRT_OK;
    }
    int readBack()  // the bracket closes (where begin() opened one), the counters are on their way; the driver queues its own results behind them
    {
        if (ev_end) HIPC(hipEventRecord(ev_end, drain.stream));
        HIPC(hipMemcpyAsync(&ds, d_stats, sizeof(ds), hipMemcpyDeviceToHost, drain.stream));
        return TRT_OK;
    }
    int finish(trt_stats* stats_out, uint32_t passes)  // after readBack(): the stream is synchronised, st completed and given to stats_out (may be null)
    {
        HIPC(hipStreamSynchronize(drain.stream));
        HIPC(hipGetLastError());
        drain.armed = false;  // everything this call enqueued has completed
        float ms = 0.f;
        if (ev_end) HIPC(hipEventElapsedTime(&ms, ev_begin, ev_end));
        st.render_ms = ms;
        for (const auto& sp : tm.spans) {
            float k_ms = 0.f;
            if (hipEventElapsedTime(&k_ms, h->events[sp.e0], h->events[sp.e1]) == hipSuccess) st.kernel_ms[sp.k] += k_ms;
        }
        addDeviceStats(st, ds, h);
        st.passes = passes;
        if (stats_out) *stats_out = st;
        return TRT_OK;
    }
    ~CallFrame()
    {
        for (int k = 0; k < drain.n_slots; ++k) h->slot_seq[k] = drain.slots[k].seq;
    }
};

// A pass's slice of the caller's host arrays org / dir (comps floats each) into its staging places on the device; org and dir then point there
int stageRaySlice(const float*& org, const float*& dir, size_t comps, float* stage_org, float* stage_dir, hipStream_t stream)
{
    HIPC(hipMemcpyAsync(stage_org, org, comps * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPC(hipMemcpyAsync(stage_dir, dir, comps * sizeof(float), hipMemcpyHostToDevice, stream));
    org = stage_org;
    dir = stage_dir;
    return TRT_OK;
}

// The passes of a render call and the arena for them.  Default budget: three quarters of what is free on the device (the scene is already
// resident); halved while the arena cannot be had.
// nl: the shadow queues a path of the call has (its lights; 1 under TRT_FLAG_ONE_LIGHT)
int planArena(trt_handle* h, const trt_params* p, uint32_t npix, uint32_t n_samples, bool list, const Footprint& fp, uint32_t nl, PassPlan& plan)
{
    uint64_t budget = p->mem_budget;
    const bool own_budget = budget == 0;
    if (own_budget) {
        size_t free_b = 0, total_b = 0;
        HIPC(hipMemGetInfo(&free_b, &total_b));
        budget = (uint64_t)(free_b + h->arena.bytes) / 4 * 3;
    }
    const int n_slots = (fp.max_slots > 1 && n_samples >= 2 && (p->flags & TRT_FLAG_OVERLAP) && h->n_slots > 1) ? N_SLOTS : 1;
    for (;;) {
        if (!planPasses(npix, n_samples, nl, budget, n_slots, fp, plan))
            return fail(TRT_ENOMEM, std::string(list ? "mem_budget too small for one sample of every listed pixel; render shorter lists"
                                                     : "mem_budget too small for one sample of every pixel of the tile; render smaller tiles") + " (" + fp.stated + ")");
        const int e = h->arena.ensure(plan.slot_bytes * (size_t)plan.slots);
        if (e == TRT_OK) return TRT_OK;
        if (e != TRT_ENOMEM || !own_budget || budget / 2 < fp.per_path * npix) return e;
        (void)hipGetLastError();  // the failed hipMalloc
        budget /= 2;
    }
}

// Host arrays to their places in small_buf (a tile without sums starts them at zero), then a pixel list is checked before any path is traced
int stageInput(const RenderInput& in, const trt_params* p, void* d_table, size_t table_bytes, double* d_sum, double* d_sq, uint32_t* d_list_max, hipStream_t stream)
{
    const size_t acc_bytes = (size_t)in.npix * 3 * sizeof(double);
    if (in.rays && !in.pixels) hipLaunchKernelGGL(k_iota, dim3(std::min<uint32_t>((in.npix + 255) / 256, 1024u)), dim3(256), 0, stream, (uint32_t*)d_table, in.npix);
    else if (in.host) HIPC(hipMemcpyAsync(d_table, in.list ? (const void*)in.pixels : (const void*)in.rows.data(), table_bytes, hipMemcpyHostToDevice, stream));
    if (in.host) {
        if (in.sum) HIPC(hipMemcpyAsync(d_sum, in.sum, acc_bytes, hipMemcpyHostToDevice, stream));
        else HIPC(hipMemsetAsync(d_sum, 0, acc_bytes, stream));
        if (d_sq) HIPC(hipMemcpyAsync(d_sq, in.sumsq, acc_bytes, hipMemcpyHostToDevice, stream));
    }
    if (!in.list || in.rays) return TRT_OK;  // stream ids are any 32 bits
    uint32_t list_max = 0;
    hipLaunchKernelGGL(k_list_max, dim3(std::min<uint32_t>((in.npix + 255) / 256, 1024u)), dim3(256), 0, stream, in.host ? (const uint32_t*)d_table : in.pixels, in.npix, d_list_max);
    HIPC(hipMemcpyAsync(&list_max, d_list_max, sizeof(list_max), hipMemcpyDeviceToHost, stream));
    HIPC(hipStreamSynchronize(stream));
    if ((uint64_t)list_max >= (uint64_t)p->width * (uint64_t)p->height) return fail(TRT_EINVAL, "pixel list holds an entry >= width * height");
    return TRT_OK;
}

// The schedule of a render call as data (TRT_DEBUG with TRT_DEBUG_SCHEDULE=1; tests/sched_graph.py reads it): one line per operation the pass
// loop enqueues — a launch, a memset, a resolve — with its stream (call, slot0, slot1, side), the events that stream was told to wait for since
// its last operation, the event recorded right behind it, and the half-open element ranges it reads and writes, by buffer.  Formed from the
// variables the launches use; "-" is the empty list.
struct SchedTrace {
    enum { CALL = 0, SLOT0 = 1, SIDE = 3 };
    bool on = false;
    std::string pending[4];
    void wait(int s, const char* ev)
    {
        if (!on) return;
        if (!pending[s].empty()) pending[s] += ',';
        pending[s] += ev;
    }
    static std::string iv(const char* buf, uint64_t lo, uint64_t hi) { return std::string(buf) + "[" + std::to_string(lo) + "," + std::to_string(hi) + ")"; }
    static std::string iv(const char* buf, uint32_t k, uint64_t lo, uint64_t hi) { return iv((std::string(buf) + std::to_string(k)).c_str(), lo, hi); }
    void op(const char* what, int s, uint32_t pass, int bounce, int light, const char* record, const std::string& reads, const std::string& writes)
    {
        if (!on) return;
        static const char* const names[4] = {"call", "slot0", "slot1", "side"};
        std::fprintf(stderr, "trt_sched: op=%s pass=%u bounce=%d light=%d stream=%s wait=%s record=%s read=%s write=%s\n", what, pass, bounce, light, names[s],
                     pending[s].empty() ? "-" : pending[s].c_str(), record ? record : "-", reads.empty() ? "-" : reads.c_str(), writes.empty() ? "-" : writes.c_str());
        pending[s].clear();
    }
};
const char* const SIDE_EVENT_NAMES[4] = {"shade0", "shade1", "shadow0", "shadow1"};
inline ShadowQueue queueAt(ShadowQueue q, uint64_t at) { return ShadowQueue{q.sa + at, q.sb + at, q.sw + at}; }

// The render loop behind every render entry: samples [s_begin, s_end) of p->spp of what `in` describes, added in sample order onto
// its per-pixel sums.  The entry points have checked p and the sample range and made h's device current.
int renderCore(trt_handle* h, const trt_params* p, uint32_t s_begin, uint32_t s_end, const RenderInput& in, hipStream_t stream, trt_stats* stats_out)
{
    const uint32_t n_samples = s_end - s_begin, npix = in.npix, count_rows = h->count_rows;
    // nl: the shadow queues of the call — one per light, or the one queue of TRT_FLAG_ONE_LIGHT (rays to whichever light a vertex picked: the occlusion
    // test of TRT_FLAG_FIXED_NEE needs neither the light's material nor its box, so launch 0's arguments serve them all)
    const bool pick = picksOneLight(h, p);
    const uint32_t nl = pick ? 1u : h->sc.n_lights;
    PassPlan plan;
    if (int e = planArena(h, p, npix, n_samples, in.list, renderFootprint(nl), nl, plan)) return e;
    // ---- small_buf: the row table or the staged pixel list, the counters of each slot, the block cleared first (DeviceStats; per slot the
    // length of its redo list and the blocks of k_trace_fix that are through; the list's maximum), the staged sums and sums of squares
    const size_t counts_bytes = (size_t)COUNT_STRIDE * count_rows * sizeof(uint32_t), acc_bytes = (size_t)npix * 3 * sizeof(double);
    const bool own_table = in.host || (in.rays && !in.pixels);  // the table is staged, or (rays without stream ids) filled here
    const size_t table_bytes = !own_table ? 0 : (in.list ? (size_t)npix * sizeof(uint32_t) : in.rows.size() * sizeof(int32_t));
    Layout L;
    const size_t o_table = L.add(table_bytes, 256), o_counts = L.add(counts_bytes * N_SLOTS, 256);
    const size_t o_stats = L.add(sizeof(DeviceStats), 256), o_redo = L.add(2 * N_SLOTS * sizeof(uint32_t), 64), o_list_max = L.add(sizeof(uint32_t), 64);
    const size_t o_pack = L.add(N_SLOTS * sizeof(unsigned long long), 64);  // per slot: the rays k_rays_pack queued (low word; read as k_shade's pair word)
    const size_t o_sum = L.add(in.host ? acc_bytes : 0, 256), o_sumsq = L.add(in.host && in.sumsq ? acc_bytes : 0, sizeof(double));
    if (int e = h->small_buf.ensure(L.bytes)) return e;
    char* sb = (char*)h->small_buf.p;
    DeviceStats* d_stats = (DeviceStats*)(sb + o_stats);
    const void* d_table = own_table ? (const void*)(sb + o_table) : (const void*)in.pixels;
    double* d_sum = in.host ? (double*)(sb + o_sum) : in.sum;
    double* d_sq = !in.sumsq ? nullptr : (in.host ? (double*)(sb + o_sumsq) : in.sumsq);
    PassSlot slots[N_SLOTS];
    CallFrame fr(h, stream, (p->flags & TRT_FLAG_TIMING) != 0);
    Timer& tm = fr.tm;
    trt_stats& st = fr.st;
    if (int e = fr.clear(d_stats, o_sum - o_stats)) return e;
    if (int e = stageInput(in, p, sb + o_table, table_bytes, d_sum, d_sq, (uint32_t*)(sb + o_list_max), stream)) return e;
    for (int k = 0; k < plan.slots; ++k) {
        PassSlot& S = slots[k];
        S.stream = h->slot_streams[k];
        SlotLayout::carve(S, (f4*)((char*)h->arena.p + plan.slot_bytes * (size_t)k), plan.N, nl);
        S.redo.count = (uint32_t*)(sb + o_redo) + 2 * k;
        S.d_counts = (uint32_t*)(sb + o_counts + counts_bytes * (size_t)k);
        S.host_counts = h->pinned_counts + (size_t)k * (2 * count_rows + 16);
        S.seq = h->slot_seq[k];
        S.spill = (uint32_t*)h->spill.p + (size_t)k * h->spill_words_per_slot;
    }
    // k_shade's three flavours (trt_kernels.h): 512-thread blocks at 6 waves per SIMD for one light, 256-thread blocks at 5 for
    // several; more than TRT_MAX_LIGHTS lights find their queues in the arena instead of in the kernel arguments.  The fourth, SHADE_PICK, is
    // TRT_FLAG_ONE_LIGHT's: one queue as for one light, the light drawn per vertex; the fifth, SHADE_NEAR, draws it from the light tree (TRT_FLAG_NEAR_LIGHTS).
    const int lights = pick ? (picksNearLight(h, p) ? SHADE_NEAR : SHADE_PICK) : (nl == 1u ? SHADE_ONE : (nl <= (uint32_t)TRT_MAX_LIGHTS ? SHADE_FEW : SHADE_MANY));
    const uint32_t shade_block = (uint32_t)shadeBlockOf(lights);
    const uint32_t rows_lds = (in.rows.size() <= shadeRowsLds((int)shade_block) && p->height <= 65536) ? (uint32_t)in.rows.size() : 0u;  // 0 for a list
    // the kernels of this call: bounce 0 traces the camera rays of the tile or of the list, later bounces the queue
    const bool count = (p->flags & TRT_FLAG_COUNT) != 0;
    const int camera = in.list ? PRIMARY_LIST : 1;
    const ClosestKernel camera_k = closestKernel(h, count, camera), queue_k = closestKernel(h, count, 0);
    const FixKernel camera_fix = fixKernel(h, false, camera), queue_fix = fixKernel(h, false, 0), shadow_fix = fixKernel(h, true, 0);
    const ShadowKernel shadow_k = shadowKernel(h, count);
    const ShadeKernel shade_k = shadeKernel(h->shade_tabs, lights, in.list, h->hit8);
    const TailKernel tail_k = tailKernel(count, in.list);
    // bounce 0 in one kernel (k_shade's FUSE flavour): tile renders on a handle set up for it; a counting render keeps the two kernels and their counters
    const bool fuse = h->fuse_primary && lights == SHADE_ONE && !in.list && !in.rays && !count;
    ShadeArgs shade_args = shadeArgsOf(h, p, in, d_table, rows_lds, d_stats);
    // camera rays that provably miss the root's two child boxes (trt_cull.h): tile renders only; a counting render keeps the root visit of every ray
    bool culls = false, shade_culls = false;
    TileDesc td_cull = shade_args.td;  // what k_resolve_tile gets
    if (!in.list && !in.rays && !count && !d_sq && h->cull_primary) {
        const CullBound cb = cullBound(h->sc.cam, p->width, p->height, (p->flags & TRT_FLAG_FIXED_PIXELS) != 0, h->root_known ? &h->root_node : nullptr, h->sc.n_nodes);
        culls = cb.active && (cb.v[0] | cb.v[1] | cb.v[2] | cb.v[3]) != 0;  // (a scene that fills the frame: nothing lies outside, the render runs the kernels it ran)
        for (int k = 0; k < 8; ++k) td_cull.cull[k] = cb.v[k];
        // k_shade's FUSE flavour keeps the classes of the tile's columns and rows in LDS: wider or taller tiles are culled in the resolve only
        shade_culls = culls && fuse && in.tile_w <= (int32_t)TRT_SHADE_CULL_COLS && rows_lds != 0u;
        if (shade_culls) shade_args.td = td_cull;
        if (h->dbg) {
            if (cb.active)
                std::fprintf(stderr, "trt_render: cull primary columns [%d, %d] rows [%d, %d] band rows [%d, %d] band columns [%d, %d]\n", cb.j_lo, cb.j_hi, cb.i_lo, cb.i_hi,
                             cb.row_lo, cb.row_hi, cb.col_lo, cb.col_hi);
            else std::fprintf(stderr, "trt_render: cull primary off: %s\n", cb.why);
        }
    } else if (h->dbg && !in.list && !in.rays) {
        std::fprintf(stderr, "trt_render: cull primary off: %s\n", count ? "counting render" : "TRT_CULL_PRIMARY=0");
    }
    // which of the two routes this call takes: 1 = k_shade skips the culled paths itself, 0 = at most k_resolve_tile skips their pixels
    if (h->dbg && !in.list && !in.rays) std::fprintf(stderr, "trt_render: cull in k_shade %d\n", (int)shade_culls);
    const TileDesc& td = shade_args.td;
    if (h->dbg)
        std::fprintf(stderr, "%s: k_shade %s, rows in lds %u, grid_ok %u\n", in.rays ? "trt_render_rays" : (in.list ? "trt_render_pixels" : "trt_render"),
                     lights == SHADE_NEAR ? "near" : lights == SHADE_PICK ? "pick" : (lights == SHADE_ONE ? "one" : (lights == SHADE_FEW ? "few" : "many")), rows_lds, td.grid_ok);
    if (h->dbg) std::fprintf(stderr, "%s: fused primary %d\n", in.rays ? "trt_render_rays" : (in.list ? "trt_render_pixels" : "trt_render"), (int)fuse);
    // The shadow walks of bounce b on the handle's side stream, beside closest hits and k_shade of bounce b + 1.  The loop stays
    // on one stream where per-kernel times or counters are asked for, where k_shade's queue flavour adds to Lacc itself (TRANSMISSION rays: a
    // material with Ni > 1), where closest-hit and shadow launches share a redo list and a spill area (the per-lane drivers), where k_shade
    // computes its queue addresses itself (SHADE_MANY), and where two passes mix already.
    const char* serial_why = nullptr;
    if (!h->shadow_stream) serial_why = "TRT_SHADOW_STREAM=0";
    else if (tm.on) serial_why = "TRT_FLAG_TIMING";
    else if (count) serial_why = "counting render";
    else if (plan.slots != 1) serial_why = "two passes in flight";
    else if (nl == 0) serial_why = "no lights";
    else if (h->refracts) serial_why = "a material with Ni > 1 (k_shade adds to Lacc)";
    else if (h->trace_impl != 0) serial_why = "per-lane walk (shared redo list and spill area)";
    else if (lights == SHADE_MANY) serial_why = "SHADE_MANY (queue addresses formed in k_shade)";
    const bool side = serial_why == nullptr;
    const hipStream_t side_stream = h->side_stream;
    if (h->dbg) {
        const char* entry = in.rays ? "trt_render_rays" : (in.list ? "trt_render_pixels" : "trt_render");
        if (side) std::fprintf(stderr, "%s: shadow stream on\n", entry);
        else std::fprintf(stderr, "%s: shadow stream off: %s\n", entry, serial_why);
    }
    SchedTrace tr;
    tr.on = h->dbg_sched;
    auto slotOf = [&](const PassSlot& S) { return SchedTrace::SLOT0 + (int)(&S - slots); };
    // main stream <- event of the side stream behind the pass's latest shadow launches (once: what follows on the stream is ordered behind it too)
    auto joinSide = [&](PassSlot& S) -> int {
        if (S.side_ev < 0) return TRT_OK;
        HIPC(hipStreamWaitEvent(S.stream, h->side_events[S.side_ev], 0));
        tr.wait(slotOf(S), SIDE_EVENT_NAMES[S.side_ev]);
        S.side_ev = -1;
        return TRT_OK;
    };

    if (int e = fr.begin(slots, plan.slots)) return e;
    const hipEvent_t ev_resolved = fr.ev_resolved;
    if (tr.on) tr.op("clear", SchedTrace::CALL, 0, -1, -1, "begin", "", SchedTrace::iv("stats", 0, 1) + "," + SchedTrace::iv("sum", 0, npix));
    for (int k = 0; k < plan.slots; ++k) {
        HIPC(hipStreamWaitEvent(slots[k].stream, fr.ev_begin, 0));
        tr.wait(SchedTrace::SLOT0 + k, "begin");
    }

    uint32_t next_chunk = 0, resolved_upto = 0;
    auto startPass = [&](PassSlot& S) -> int {
        if (next_chunk >= plan.n_chunks) { S.state = PassSlot::IDLE; return TRT_OK; }
        S.chunk = next_chunk++;
        S.s0 = s_begin + S.chunk * plan.chunk;
        S.sc_count = std::min(plan.chunk, s_end - S.s0);
        S.n_active = npix * S.sc_count;
        S.b = 0;
        S.cur = 0;
        S.rd_n = 0;
        // (the side stream's launches of the slot's previous pass: its resolve, earlier on this stream, has waited for them)
        HIPC(hipMemsetAsync(S.d_counts, 0, counts_bytes, S.stream));
        if (tr.on) tr.op("memset", slotOf(S), S.chunk, -1, -1, nullptr, "", SchedTrace::iv("d_counts", 0, COUNT_STRIDE));
        if (!in.rays) st.rays_camera += S.n_active;  // bounce 0 generates its camera rays inside the traversal and shade kernels
        S.state = in.rays ? PassSlot::PACK : PassSlot::ISSUE;
        return TRT_OK;
    };
    // trt_render_rays: the pass's slice of the caller's arrays -> the slot's queue (k_rays_pack), then the number of valid rays on its way to
    // the host.  Host arrays are staged in the slot's OTHER queue, which nothing uses before bounce 0's k_shade writes it: Q[1].ra / rb / bt
    // are carved one behind the other (SlotLayout), 48 bytes per path for the 24 a ray takes.
    auto issuePack = [&](PassSlot& S) -> int {
        const size_t at = (size_t)(S.s0 - s_begin) * npix * 3, comps = (size_t)S.n_active * 3;
        const float* org = in.org + at;
        const float* dir = in.dir + at;
        if (in.host)
            if (int e = stageRaySlice(org, dir, comps, (float*)S.Q[1].ra, (float*)S.Q[1].ra + comps, S.stream)) return e;
        unsigned long long* packed = (unsigned long long*)(sb + o_pack) + (&S - slots);
        HIPC(hipMemsetAsync(packed, 0, sizeof(*packed), S.stream));
        tm.launch(TRT_K_GEN_PRIMARY, S.stream, st, [&] {
            hipLaunchKernelGGL(k_rays_pack, dim3(std::min<uint32_t>((S.n_active + 255) / 256, 65536u)), dim3(256), 0, S.stream, org, dir, S.n_active, S.Q[0], S.Lacc,
                               (uint32_t*)packed);
        });
        if (tr.on) tr.op("pack", slotOf(S), S.chunk, -1, -1, nullptr, "", SchedTrace::iv("Q", 0, 0, S.n_active) + "," + SchedTrace::iv("Lacc", 0, S.n_active));
        S.seq++;
        hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(64), 0, S.stream, S.d_counts, COUNT_STRIDE, 0u, 1u, packed, (volatile uint32_t*)S.host_counts, 2u * count_rows, S.seq);
        S.state = PassSlot::PACKWAIT;
        return TRT_OK;
    };
    auto completePack = [&](PassSlot& S) -> int {
        if (int e = awaitCounts(S, count_rows)) return e;
        const uint32_t n_valid = S.host_counts[1];
        if (n_valid > S.n_active) return fail(TRT_EHIP, "internal error: more rays queued than given");
        st.rays_camera += n_valid;
        S.n_active = n_valid;
        S.state = n_valid ? PassSlot::ISSUE : PassSlot::RESOLVE;  // no valid entry: the zeroed Lacc is all there is to resolve
        return TRT_OK;
    };
    // trace + shade of the slot's current bounce, then the queue lengths on their way to the host
    auto issueFront = [&](PassSlot& S) -> int {
        const RaySource src{S.Q[S.cur].ra, S.Q[S.cur].rb, td, S.s0};
        const bool generated = S.b == 0 && !in.rays;  // the rays of bounce 0 come from the camera, not from the queue
        const bool fused = fuse && generated;         // ... and k_shade traces them itself
        const int ts = slotOf(S);
        if (!fused) {
            tm.launch(TRT_K_TRACE_CLOSEST, S.stream, st, [&] {
                launchTraceClosest(h, generated ? camera_k : queue_k, generated ? camera_fix : queue_fix, S.stream, S.spill, src, S.hit, S.n_active, d_stats, S.redo);
            });
            if (tr.on) tr.op("closest", ts, S.chunk, (int)S.b, -1, nullptr, generated ? std::string() : SchedTrace::iv("Q", (uint32_t)S.cur, 0, S.n_active), SchedTrace::iv("hit", 0, S.n_active));
        }
        // Where this bounce's shadow records go (trt_sched.h).  On the side route k_shade is ordered behind the shadow walks of bounce b - 2, which
        // read the end it now writes (long through, as a rule), and behind those of bounce b - 1 only where their records reach into its interval.
        S.sq_at = 0;
        if (side) {
            const ShadowPlace place = shadowPlace(plan.N, S.b, S.rd_at, S.rd_n, S.n_active);
            S.sq_at = place.at;
            if (S.b >= 2) {
                HIPC(hipStreamWaitEvent(S.stream, h->side_events[2 + (S.b & 1u)], 0));
                tr.wait(ts, SIDE_EVENT_NAMES[2 + (S.b & 1u)]);
            }
            if (place.wait) {
                HIPC(hipStreamWaitEvent(S.stream, h->side_events[2 + ((S.b - 1u) & 1u)], 0));
                tr.wait(ts, SIDE_EVENT_NAMES[2 + ((S.b - 1u) & 1u)]);
                S.side_ev = -1;  // everything on the side stream so far
            }
        }
        ShadeArgs A = shade_args;
        A.qin = S.Q[S.cur];
        A.hit = S.hit;
        A.n = S.n_active;
        A.qout = S.Q[S.cur ^ 1];
        if (lights == SHADE_MANY) A.sq_arena = S.shadow;
        else
            for (uint32_t l = 0; l < (uint32_t)TRT_MAX_LIGHTS; ++l) A.sq[l] = l < nl ? queueAt(S.shadow.queue(l), S.sq_at) : ShadowQueue{nullptr, nullptr, nullptr};
        A.pair_count = pairCounter(S.d_counts, count_rows, S.b);
        A.shadow_counts = S.d_counts + (size_t)COUNT_STRIDE + S.b;  // light l: + l * COUNT_STRIDE
        A.Lacc = S.Lacc;
        A.s0 = S.s0;
        A.primary = (S.b == 0 && !in.rays) ? 1u : 0u;
        tm.launch(TRT_K_SHADE, S.stream, st, [&] {
            hipLaunchKernelGGL(fused ? fusedShadeKernel() : shade_k, dim3(std::min<uint32_t>((S.n_active + shade_block - 1) / shade_block, 65536u)), dim3(shade_block),
                               h->shade_pad_lds, S.stream, h->sc, A);
        });
        if (side) HIPC(hipEventRecord(h->side_events[S.b & 1u], S.stream));  // what this bounce's shadow launches wait for
        if (tr.on) {
            std::string rd = fused ? std::string() : SchedTrace::iv("hit", 0, S.n_active), wr = SchedTrace::iv("Q", (uint32_t)(S.cur ^ 1), 0, S.n_active);
            if (!generated) rd += std::string(rd.empty() ? "" : ",") + SchedTrace::iv("Q", (uint32_t)S.cur, 0, S.n_active);
            for (uint32_t l = 0; l < nl; ++l) wr += "," + SchedTrace::iv("shadow", l, S.sq_at, S.sq_at + S.n_active);
            wr += "," + SchedTrace::iv("d_counts", S.b, S.b + 1u);
            // Lacc: bounce 0 initialises it (caller-supplied rays: adds to the zeroes of k_rays_pack); later bounces add to it only for TRANSMISSION rays
            if (S.b == 0 || h->refracts) wr += "," + SchedTrace::iv("Lacc", 0, (uint64_t)npix * S.sc_count);
            tr.op("shade", ts, S.chunk, (int)S.b, -1, side ? SIDE_EVENT_NAMES[S.b & 1u] : nullptr, rd, wr);
        }
        // (b, c) and (b + 1, c) of the counters in use -> host_counts[2 * c], [2 * c + 1], then the sequence word
        S.seq++;
        const uint32_t publish_block = std::min(1024u, (2u * (1u + nl) + 63u) & ~63u);
        hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(publish_block), 0, S.stream, S.d_counts, COUNT_STRIDE, S.b, 1u + nl,
                           pairCounter(S.d_counts, count_rows, S.b), (volatile uint32_t*)S.host_counts, 2u * count_rows, S.seq);
        if (tr.on) tr.op("publish", ts, S.chunk, (int)S.b, -1, nullptr, SchedTrace::iv("d_counts", S.b, S.b + 2u), "");
        S.state = PassSlot::WAIT;
        if (h->fail_at_bounce >= 0 && (int)S.b == h->fail_at_bounce) {  // test hook: fail with this bounce's kernels in flight
            h->fail_at_bounce = -1;
            return fail(TRT_EHIP, "injected failure (TRT_TEST_FAIL_AT_BOUNCE)");
        }
        return TRT_OK;
    };
    // queue lengths are back: shadow rays of this bounce, then the next bounce / the tail / the end of the pass
    auto completeBounce = [&](PassSlot& S) -> int {
        if (int e = awaitCounts(S, count_rows)) return e;
        // on the side route: behind this bounce's k_shade by its event, behind the shadow launches of every earlier bounce by the stream's order,
        // light after light — the order of the additions into a path's Lacc is the one stream's
        const hipStream_t shadow_stream = side ? side_stream : S.stream;
        const int ss = side ? (int)SchedTrace::SIDE : slotOf(S);
        uint32_t ns_max = 0, l_last = nl;
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t ns = S.host_counts[2 * (1 + l)];
            if (ns > S.n_active) return fail(TRT_EHIP, "internal error: shadow queue longer than its input");
            ns_max = std::max(ns_max, ns);
            if (ns) l_last = l;
        }
        if (side) {
            HIPC(hipStreamWaitEvent(side_stream, h->side_events[S.b & 1u], 0));
            tr.wait(ss, SIDE_EVENT_NAMES[S.b & 1u]);
        }
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t ns = S.host_counts[2 * (1 + l)];
            if (!ns) continue;
            tm.launch(TRT_K_TRACE_SHADOW, shadow_stream, st, [&] {
                launchTraceShadow(h, shadow_k, shadow_fix, shadow_stream, S.spill, queueAt(S.shadow.queue(l), S.sq_at), ns, h->light_mats[l], S.Lacc, d_stats, td.fixed_nee,
                                  S.redo, h->light_boxes[l]);
            });
            if (side && l == l_last) HIPC(hipEventRecord(h->side_events[2 + (S.b & 1u)], side_stream));
            if (tr.on)
                tr.op("shadow", ss, S.chunk, (int)S.b, (int)l, side && l == l_last ? SIDE_EVENT_NAMES[2 + (S.b & 1u)] : nullptr,
                      SchedTrace::iv("shadow", l, S.sq_at, S.sq_at + ns) + "," + SchedTrace::iv("Lacc", 0, (uint64_t)npix * S.sc_count), SchedTrace::iv("Lacc", 0, (uint64_t)npix * S.sc_count));
            st.rays_shadow += ns;
        }
        if (side) {
            if (l_last != nl) S.side_ev = 2 + (int)(S.b & 1u);  // (a bounce without shadow rays leaves the event of the latest launches in place)
            S.rd_at = S.sq_at;
            S.rd_n = ns_max;
        }
        const uint32_t n_next = S.host_counts[1];
        if (n_next > S.n_active) return fail(TRT_EHIP, "internal error: queue grew");
        st.rays_indirect += n_next;
        S.n_active = n_next;
        S.cur ^= 1;
        S.b++;
        if (S.n_active > 0 && (S.n_active <= h->tail_n || S.b >= MAX_BOUNCES)) {
            // few paths left: finish them in one launch (k_tail) instead of ~3 launches + a host round trip per bounce
            const TailArgs TA{S.Q[S.cur], S.n_active, S.Lacc, td, S.s0, p->max_depth, S.spill, SPILL_STRIDE, h->trace_impl == 0 ? 1u : 0u, d_stats};
            if (int e = joinSide(S)) return e;  // k_tail reads and adds to Lacc: behind every shadow launch of the pass
            tm.launch(TRT_K_TAIL, S.stream, st, [&] { hipLaunchKernelGGL(tail_k, dim3(tailGrid(S.n_active)), dim3(TRT_TRACE_BLOCK), 0, S.stream, h->sc, TA); });
            if (tr.on)
                tr.op("tail", slotOf(S), S.chunk, (int)S.b, -1, nullptr, SchedTrace::iv("Q", (uint32_t)S.cur, 0, S.n_active) + "," + SchedTrace::iv("Lacc", 0, (uint64_t)npix * S.sc_count),
                      SchedTrace::iv("Lacc", 0, (uint64_t)npix * S.sc_count));
            S.n_active = 0;
        }
        S.state = S.n_active ? PassSlot::ISSUE : PassSlot::RESOLVE;
        return TRT_OK;
    };
    // per-pixel accumulation in sample order: pass c is resolved only after pass c-1 (on whichever stream that ran)
    auto tryResolve = [&](PassSlot& S) -> int {
        if (S.chunk != resolved_upto) return TRT_OK;  // an earlier pass is still in flight on the other slot
        if (resolved_upto > 0) {  // recorded by the previous resolve, earlier in host order
            HIPC(hipStreamWaitEvent(S.stream, ev_resolved, 0));
            tr.wait(slotOf(S), "resolved");
        }
        // the resolve reads Lacc, and the slot's next pass overwrites Lacc and the shadow queues: behind every shadow launch of this pass
        if (int e = joinSide(S)) return e;
        tm.launch(TRT_K_RESOLVE, S.stream, st, [&] {
            const dim3 rg(std::min<uint32_t>((npix + 255) / 256, 65536u)), rb(256);
            if (d_sq) hipLaunchKernelGGL(k_resolve_moments, rg, rb, 0, S.stream, S.Lacc, d_sum, d_sq, npix, S.sc_count, (float)p->spp);
            else if (culls) hipLaunchKernelGGL(k_resolve_tile, rg, rb, 0, S.stream, S.Lacc, d_sum, td_cull, S.sc_count, (float)p->spp);
            else hipLaunchKernelGGL(k_resolve, rg, rb, 0, S.stream, S.Lacc, d_sum, npix, S.sc_count, (float)p->spp);
        });
        HIPC(hipEventRecord(ev_resolved, S.stream));
        if (tr.on) tr.op("resolve", slotOf(S), S.chunk, -1, -1, "resolved", SchedTrace::iv("Lacc", 0, (uint64_t)npix * S.sc_count) + "," + SchedTrace::iv("sum", 0, npix), SchedTrace::iv("sum", 0, npix));
        resolved_upto++;
        return startPass(S);
    };

    for (int k = 0; k < plan.slots; ++k)
        if (int e = startPass(slots[k])) return e;
    for (;;) {
        bool any = false;
        for (int k = 0; k < plan.slots; ++k)
            if (slots[k].state == PassSlot::PACK) { if (int e = issuePack(slots[k])) return e; }
        for (int k = 0; k < plan.slots; ++k)
            if (slots[k].state == PassSlot::PACKWAIT) { if (int e = completePack(slots[k])) return e; }
        for (int k = 0; k < plan.slots; ++k)
            if (slots[k].state == PassSlot::ISSUE) { if (int e = issueFront(slots[k])) return e; }
        for (int k = 0; k < plan.slots; ++k) {
            PassSlot& S = slots[k];
            if (S.state == PassSlot::WAIT) { if (int e = completeBounce(S)) return e; }
            if (S.state == PassSlot::RESOLVE) { if (int e = tryResolve(S)) return e; }
            any = any || S.state != PassSlot::IDLE;
        }
        if (!any) break;
    }
    if (resolved_upto != plan.n_chunks) return fail(TRT_EHIP, "internal error: passes left unresolved");

    HIPC(hipStreamWaitEvent(stream, ev_resolved, 0));
    tr.wait(SchedTrace::CALL, "resolved");
    if (in.out_dev) {
        tm.begin(TRT_K_RESOLVE, stream);
        hipLaunchKernelGGL(k_finalize, dim3(std::min<uint32_t>((npix * 3 + 255) / 256, 65536u)), dim3(256), 0, stream, d_sum, in.out_dev, npix * 3);
        tm.end(stream);
    }
    if (tr.on) tr.op(in.out_dev ? "finalize" : "readback", SchedTrace::CALL, 0, -1, -1, nullptr, SchedTrace::iv("sum", 0, npix) + "," + SchedTrace::iv("stats", 0, 1), "");
    st.rows_rendered = in.rows.size();  // 0 for a pixel list
    if (int e = fr.readBack()) return e;
    if (in.host && in.sum) {
        HIPC(hipMemcpyAsync(in.sum, d_sum, acc_bytes, hipMemcpyDeviceToHost, stream));
        if (d_sq) HIPC(hipMemcpyAsync(in.sumsq, d_sq, acc_bytes, hipMemcpyDeviceToHost, stream));
    }
    return fr.finish(stats_out, plan.n_chunks);
}

// p with the whole image as its tile and every row selected: the list entries ignore the caller's tile and row interleave
trt_params wholeImage(trt_params p)
{
    p.x0 = 0; p.y0 = 0; p.x1 = p.width; p.y1 = p.height;
    p.row_block = 1; p.row_mod = 1; p.row_rem = 0;
    return p;
}

// What the sampled-list entries (trt_render_pixels*, trt_render_rays*, trt_aov_rays*) check and do once their trt_params are through, in
// this order: the sample range; `refused`, the entry's complaint about its arrays or null; n entries against the path ids of a pass
// (`too_long`: the entry's words for it); the stats zeroed.  -> empty: nothing to trace, the call is over.
int listCall(int32_t sample_begin, int32_t sample_end, uint32_t n, const char* refused, const char* too_long, trt_stats* stats, bool& empty)
{
    if (sample_begin < 0 || sample_begin > sample_end) return fail(TRT_EINVAL, "sample range must satisfy 0 <= begin <= end");
    if (refused) return fail(TRT_EINVAL, refused);
    if (n > MAX_PASS_PATHS) return fail(TRT_EINVAL, too_long);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    empty = n == 0 || sample_begin == sample_end;
    return TRT_OK;
}

// The tile of p (checked) as a RenderInput: its selected rows, its width and first column, its pixels — at most max_npix
int tileInput(const trt_params* p, RenderInput& in, uint64_t max_npix)
{
    for (int y = p->y0; y < p->y1; ++y)
        if (rowSelected(p, y)) in.rows.push_back(y);
    if (in.rows.empty()) return fail(TRT_EINVAL, "row interleave selects no rows of the tile");
    in.tile_w = p->x1 - p->x0;
    in.x0 = p->x0;
    const uint64_t npix64 = (uint64_t)in.rows.size() * (uint32_t)in.tile_w;
    if (npix64 > max_npix) return fail(TRT_EINVAL, "tile too large");
    in.npix = (uint32_t)npix64;
    return TRT_OK;
}

// A tile of p (checked): samples [s_begin, s_end), onto accum_host's sums when given, rounded into out_dev; without out_dev into the
// handle's out_buf (rows x width) and from there to out_host (trt_render, trt_render_samples)
int renderTile(trt_handle* h, const trt_params* p, uint32_t s_begin, uint32_t s_end, float* out_dev, float* out_host, void* hip_stream, trt_stats* stats,
               double* accum_host)
{
    HIPC(hipSetDevice(h->device));
    RenderInput in;
    if (int e = tileInput(p, in, 0x7FFFFFFFull)) return e;
    const size_t out_bytes = (size_t)in.npix * 3 * sizeof(float);
    if (!out_dev) {
        if (int e = h->out_buf.ensure(out_bytes)) return e;
        out_dev = (float*)h->out_buf.p;
    }
    in.sum = accum_host;
    in.out_dev = out_dev;
    if (int e = renderCore(h, p, s_begin, s_end, in, (hipStream_t)hip_stream, stats)) return e;
    if (out_host) HIPC(hipMemcpy(out_host, out_dev, out_bytes, hipMemcpyDeviceToHost));
    return TRT_OK;
}

// trt_render_aov / _device: the camera rays of every sample of the tile through the render's bounce-0 traversal (k_trace_closest with
// PRIMARY = 1, k_trace_fix behind it), then k_aov adds each pass's first hits onto the seven per-pixel sums in small_buf, and k_finalize
// rounds them into out[0..2] (albedo, normal, depth; device pointers, null = not wanted).  Everything runs on `stream`, one pass at a time.
int aovCore(trt_handle* h, const trt_params* p, const RenderInput& in, float* const out[3], hipStream_t stream, trt_stats* stats_out)
{
    const uint32_t npix = in.npix, spp = (uint32_t)p->spp;
    PassPlan plan;
    if (int e = planArena(h, p, npix, spp, false, aovFootprint(), h->sc.n_lights, plan)) return e;
    // small_buf: the row table, the block cleared first (DeviceStats, the redo list's length and the blocks of k_trace_fix that are through),
    // the sums (albedo, normal: 3 per pixel; depth: 1 per pixel)
    const size_t table_bytes = in.rows.size() * sizeof(int32_t), sum_bytes = (size_t)npix * 7 * sizeof(double);
    Layout L;
    const size_t o_table = L.add(table_bytes, 256), o_stats = L.add(sizeof(DeviceStats), 256), o_redo = L.add(2 * sizeof(uint32_t), 64);
    const size_t o_sum = L.add(sum_bytes, 256);
    if (int e = h->small_buf.ensure(L.bytes)) return e;
    char* sb = (char*)h->small_buf.p;
    DeviceStats* d_stats = (DeviceStats*)(sb + o_stats);
    double* d_sum = (double*)(sb + o_sum);
    CallFrame fr(h, stream, (p->flags & TRT_FLAG_TIMING) != 0);
    Timer& tm = fr.tm;
    trt_stats& st = fr.st;
    if (int e = fr.clear(d_stats, o_sum - o_stats)) return e;
    HIPC(hipMemsetAsync(d_sum, 0, sum_bytes, stream));
    HIPC(hipMemcpyAsync(sb + o_table, in.rows.data(), table_bytes, hipMemcpyHostToDevice, stream));
    f4* hit = nullptr;
    RedoList redo{(uint32_t*)(sb + o_redo), nullptr};
    AovLayout::carve((f4*)h->arena.p, plan.N, hit, redo.idx);
    uint32_t* spill = (uint32_t*)h->spill.p;
    const bool count = (p->flags & TRT_FLAG_COUNT) != 0;
    const ClosestKernel camera_k = closestKernel(h, count, 1);
    const FixKernel camera_fix = fixKernel(h, false, 1);
    const TileDesc td = shadeArgsOf(h, p, in, sb + o_table, 0u, d_stats).td;
    const dim3 rg(std::min<uint32_t>((npix + 255) / 256, 65536u)), rb(256);

    if (int e = fr.begin()) return e;
    const auto aov_k = h->hit8 ? k_aov<true> : k_aov<false>;
    for (uint32_t c = 0; c < plan.n_chunks; ++c) {
        const uint32_t s0 = c * plan.chunk, sc_count = std::min(plan.chunk, spp - s0), n = npix * sc_count;
        const RaySource src{nullptr, nullptr, td, s0};
        tm.launch(TRT_K_TRACE_CLOSEST, stream, st, [&] { launchTraceClosest(h, camera_k, camera_fix, stream, spill, src, hit, n, d_stats, redo); });
        tm.launch(TRT_K_RESOLVE, stream, st, [&] { hipLaunchKernelGGL(aov_k, rg, rb, 0, stream, h->sc, td, s0, (const f4*)hit, d_sum, npix, sc_count, (float)p->spp); });
        st.rays_camera += n;
    }
    tm.begin(TRT_K_RESOLVE, stream);
    const uint32_t per_pixel[3] = {3u, 3u, 1u};
    const size_t sum_at[3] = {0, (size_t)npix * 3, (size_t)npix * 6};
    for (int k = 0; k < 3; ++k)
        if (out[k]) {
            const uint32_t m = npix * per_pixel[k];
            hipLaunchKernelGGL(k_finalize, dim3(std::min<uint32_t>((m + 255) / 256, 65536u)), dim3(256), 0, stream, d_sum + sum_at[k], out[k], m);
        }
    tm.end(stream);
    st.rows_rendered = in.rows.size();
    if (int e = fr.readBack()) return e;
    return fr.finish(stats_out, plan.n_chunks);
}

// The checks of include/trt.h, then aovCore into the caller's device buffers (`host` false) or into out_buf and from there to the host
int renderAov(trt_handle* h, const trt_params* p, float* albedo, float* normal, float* depth, bool host, void* hip_stream, trt_stats* stats)
{
    if (int e = checkParams(h, p)) return e;
    if (!albedo && !normal && !depth) return fail(TRT_EINVAL, "trt_render_aov: every output buffer is null");
    HIPC(hipSetDevice(h->device));
    RenderInput in;
    if (int e = tileInput(p, in, 0x7FFFFFFFull / 7)) return e;
    float* const user[3] = {albedo, normal, depth};
    const size_t floats[3] = {(size_t)in.npix * 3, (size_t)in.npix * 3, (size_t)in.npix};
    float* out[3] = {albedo, normal, depth};
    if (host) {
        if (int e = h->out_buf.ensure((floats[0] + floats[1] + floats[2]) * sizeof(float))) return e;
        float* q = (float*)h->out_buf.p;
        for (int k = 0; k < 3; ++k) {
            out[k] = user[k] ? q : nullptr;
            q += floats[k];
        }
    }
    if (int e = aovCore(h, p, in, out, host ? nullptr : (hipStream_t)hip_stream, stats)) return e;
    if (host)
        for (int k = 0; k < 3; ++k)
            if (user[k]) HIPC(hipMemcpy(user[k], out[k], floats[k] * sizeof(float), hipMemcpyDeviceToHost));
    return TRT_OK;
}

// trt_aov_rays / _device: the checks of include/trt.h, then pass by pass: k_aov_rays_pack turns the pass's slice of the caller's rays into queue
// records in the arena (host arrays are staged in io_buf first, one pass's slice at a time), the queue flavour of the handle's closest-hit kernel
// walks them with k_trace_fix behind it — what trt_trace_closest launches —, and k_aov_rays adds the first hits onto the caller's sums (device
// entry: in place; host entry: copies of the given ones in small_buf, copied back at the end).  Everything runs on one stream, one pass at a time.
int aovRays(trt_handle* h, const trt_params* p, uint32_t n, const float* org, const float* dir, int32_t sample_begin, int32_t sample_end, double* albedo,
            double* normal, double* depth, bool host, void* hip_stream, trt_stats* stats_out)
{
    if (!h || !p) return fail(TRT_EINVAL, "null handle/params");
    if (p->spp < 1) return fail(TRT_EINVAL, "spp must be >= 1");
    const char* const refused = (n > 0 && (!org || !dir)) ? "null ray arrays" : ((!albedo && !normal && !depth) ? "trt_aov_rays: every sum is null" : nullptr);
    bool empty = false;
    if (int e = listCall(sample_begin, sample_end, n, refused, "more rays per sample than the path ids of one pass can number (0x7FFF0000)", stats_out, empty)) return e;
    if (empty) return TRT_OK;
    HIPC(hipSetDevice(h->device));
    hipStream_t stream = host ? nullptr : (hipStream_t)hip_stream;
    const uint32_t n_samples = (uint32_t)(sample_end - sample_begin);
    PassPlan plan;
    if (int e = planArena(h, p, n, n_samples, true, aovRaysFootprint(), h->sc.n_lights, plan)) return e;
    // small_buf: the block cleared first (DeviceStats, the redo list's length and the blocks of k_trace_fix that are through, the number of valid
    // entries), then the host entry's sums (albedo, normal: 3 per entry; depth: 1 per entry)
    double* const user[3] = {albedo, normal, depth};
    const size_t doubles[3] = {(size_t)n * 3, (size_t)n * 3, (size_t)n};
    Layout L;
    const size_t o_stats = L.add(sizeof(DeviceStats), 256), o_redo = L.add(2 * sizeof(uint32_t), 64), o_valid = L.add(sizeof(unsigned long long), 64);
    const size_t o_sum = L.add(host ? (size_t)n * 7 * sizeof(double) : 0, 256);
    if (int e = h->small_buf.ensure(L.bytes)) return e;
    const size_t slice_floats = (size_t)plan.N * 3;  // one pass's org (and dir)
    if (host)
        if (int e = h->io_buf.ensure(2 * slice_floats * sizeof(float))) return e;
    char* sb = (char*)h->small_buf.p;
    DeviceStats* d_stats = (DeviceStats*)(sb + o_stats);
    unsigned long long* d_valid = (unsigned long long*)(sb + o_valid);
    double* sum[3] = {albedo, normal, depth};
    CallFrame fr(h, stream, (p->flags & TRT_FLAG_TIMING) != 0);
    Timer& tm = fr.tm;
    trt_stats& st = fr.st;
    if (int e = fr.clear(d_stats, o_sum - o_stats)) return e;
    if (host) {
        double* q = (double*)(sb + o_sum);
        for (int k = 0; k < 3; ++k) {
            sum[k] = user[k] ? q : nullptr;
            if (user[k]) HIPC(hipMemcpyAsync(q, user[k], doubles[k] * sizeof(double), hipMemcpyHostToDevice, stream));
            q += doubles[k];
        }
    }
    f4 *ra = nullptr, *rb = nullptr, *hit = nullptr;
    RedoList redo{(uint32_t*)(sb + o_redo), nullptr};
    AovRaysLayout::carve((f4*)h->arena.p, plan.N, ra, rb, hit, redo.idx);
    uint32_t* spill = (uint32_t*)h->spill.p;
    const bool count = (p->flags & TRT_FLAG_COUNT) != 0;
    const ClosestKernel queue_k = closestKernel(h, count, 0);
    const FixKernel queue_fix = fixKernel(h, false, 0);
    RaySource src{};
    src.ra = ra;
    src.rb = rb;

    if (int e = fr.begin()) return e;
    const dim3 block(256);
    const auto aov_k = h->hit8 ? k_aov_rays<true> : k_aov_rays<false>;
    for (uint32_t c = 0; c < plan.n_chunks; ++c) {
        const uint32_t s0 = c * plan.chunk, sc_count = std::min(plan.chunk, n_samples - s0), cnt = n * sc_count;
        const size_t at = (size_t)s0 * n * 3, comps = (size_t)cnt * 3;
        const float* d_org = org + at;
        const float* d_dir = dir + at;
        if (host)  // the stream orders this pass's copies behind the last pass's packing
            if (int e = stageRaySlice(d_org, d_dir, comps, (float*)h->io_buf.p, (float*)h->io_buf.p + slice_floats, stream)) return e;
        tm.launch(TRT_K_GEN_PRIMARY, stream, st, [&] {
            hipLaunchKernelGGL(k_aov_rays_pack, dim3(std::min<uint32_t>((cnt + 255) / 256, 65536u)), block, 0, stream, d_org, d_dir, cnt, ra, rb, d_valid);
        });
        tm.launch(TRT_K_TRACE_CLOSEST, stream, st, [&] { launchTraceClosest(h, queue_k, queue_fix, stream, spill, src, hit, cnt, d_stats, redo); });
        tm.launch(TRT_K_RESOLVE, stream, st, [&] {
            const dim3 grid(std::min<uint32_t>((n + 255) / 256, 65536u));
            hipLaunchKernelGGL(aov_k, grid, block, 0, stream, h->sc, (const f4*)ra, (const f4*)rb, (const f4*)hit, sum[0], sum[1], sum[2], n, sc_count, (float)p->spp);
        });
    }
    static_assert(sizeof(st.rays_camera) == sizeof(*d_valid), "the count of valid rays lands in the stats");
    if (int e = fr.readBack()) return e;
    HIPC(hipMemcpyAsync(&st.rays_camera, d_valid, sizeof(*d_valid), hipMemcpyDeviceToHost, stream));
    if (host)
        for (int k = 0; k < 3; ++k)
            if (user[k]) HIPC(hipMemcpyAsync(user[k], sum[k], doubles[k] * sizeof(double), hipMemcpyDeviceToHost, stream));
    return fr.finish(stats_out, plan.n_chunks);
}
}  // namespace

int trt_render_device(trt_handle* h, const trt_params* p, float* out_dev, void* hip_stream, trt_stats* stats_out)
{
    if (int e = checkParams(h, p)) return e;
    if (int e = checkEstimator(p)) return e;
    if (!out_dev) return fail(TRT_EINVAL, "null output buffer");
    return renderTile(h, p, 0u, (uint32_t)p->spp, out_dev, nullptr, hip_stream, stats_out, nullptr);
}

int trt_render_samples(trt_handle* h, const trt_params* p, int32_t sample_begin, int32_t sample_end, double* accum_host, float* out_host, trt_stats* stats)
{
    if (int e = checkParams(h, p)) return e;
    if (int e = checkEstimator(p)) return e;
    if (!accum_host) return fail(TRT_EINVAL, "null accumulator");
    if (sample_begin < 0 || sample_end <= sample_begin || sample_end > p->spp) return fail(TRT_EINVAL, "sample range must satisfy 0 <= begin < end <= spp");
    return renderTile(h, p, (uint32_t)sample_begin, (uint32_t)sample_end, nullptr, out_host, nullptr, stats, accum_host);
}

namespace {
// trt_render_pixels / _device: the checks of include/trt.h, then the render loop on the list.  The tile and row interleave of p are
// ignored (checked as the whole image); sample_end may pass p->spp, which only scales the terms.
int renderPixels(trt_handle* h, const trt_params* p_in, uint32_t n_pixels, const uint32_t* pixels, int32_t sample_begin, int32_t sample_end, double* sum,
                 double* sumsq, void* hip_stream, trt_stats* stats, bool host)
{
    if (!h || !p_in) return fail(TRT_EINVAL, "null handle/params");
    const trt_params p = wholeImage(*p_in);
    if (int e = checkParams(h, &p)) return e;
    if (int e = checkEstimator(&p)) return e;
    bool empty = false;
    if (int e = listCall(sample_begin, sample_end, n_pixels, (n_pixels > 0 && (!pixels || !sum)) ? "null pixel list or sums" : nullptr,
                         "pixel list longer than the path ids of one pass can number (0x7FFF0000)", stats, empty))
        return e;
    if (empty) return TRT_OK;
    HIPC(hipSetDevice(h->device));
    RenderInput in;
    in.list = true;
    in.host = host;
    in.pixels = pixels;
    in.npix = n_pixels;
    in.tile_w = p.width;
    in.sum = sum;
    in.sumsq = sumsq;
    return renderCore(h, &p, (uint32_t)sample_begin, (uint32_t)sample_end, in, (hipStream_t)hip_stream, stats);
}
}  // namespace

int trt_render_pixels(trt_handle* h, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels, int32_t sample_begin, int32_t sample_end,
                      double* sum_host, double* sumsq_host, trt_stats* stats)
{
    return renderPixels(h, p, n_pixels, pixels, sample_begin, sample_end, sum_host, sumsq_host, nullptr, stats, true);
}

int trt_render_pixels_device(trt_handle* h, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels_dev, int32_t sample_begin, int32_t sample_end,
                             double* sum_dev, double* sumsq_dev, void* hip_stream, trt_stats* stats)
{
    return renderPixels(h, p, n_pixels, pixels_dev, sample_begin, sample_end, sum_dev, sumsq_dev, hip_stream, stats, false);
}

namespace {
// trt_render_rays / _device: the checks of include/trt.h, then the render loop on the list of stream ids with the caller's rays as bounce 0.
// width, height, the tile fields and TRT_FLAG_FIXED_PIXELS of p have no meaning here: the loop gets a 2 x 2 image that is never looked at.
int renderRays(trt_handle* h, const trt_params* p_in, uint32_t n, const float* org, const float* dir, const uint32_t* stream_ids, int32_t sample_begin,
               int32_t sample_end, double* sum, double* sumsq, void* hip_stream, trt_stats* stats, bool host)
{
    if (!h || !p_in) return fail(TRT_EINVAL, "null handle/params");
    if (p_in->spp < 1) return fail(TRT_EINVAL, "spp must be >= 1");
    if (p_in->max_depth < 0) return fail(TRT_EINVAL, "max_depth must be >= 0");
    if (int e = checkEstimator(p_in)) return e;
    bool empty = false;
    if (int e = listCall(sample_begin, sample_end, n, (n > 0 && (!org || !dir || !sum)) ? "null ray arrays or sums" : nullptr,
                         "more rays per sample than the path ids of one pass can number (0x7FFF0000)", stats, empty))
        return e;
    if (empty) return TRT_OK;
    trt_params p = *p_in;
    p.width = p.height = 2;
    p = wholeImage(p);
    HIPC(hipSetDevice(h->device));
    RenderInput in;
    in.list = true;
    in.rays = true;
    in.host = host;
    in.org = org;
    in.dir = dir;
    in.pixels = stream_ids;
    in.npix = n;
    in.tile_w = p.width;
    in.sum = sum;
    in.sumsq = sumsq;
    return renderCore(h, &p, (uint32_t)sample_begin, (uint32_t)sample_end, in, (hipStream_t)hip_stream, stats);
}

// What trt_camera_rays* takes of p, checked; the grid reciprocals as shadeArgsOf forms them
int cameraRaysArgs(const trt_camera* cam, const trt_params* p, uint32_t n_pixels, const void* pixels, int32_t sample_begin, int32_t sample_end, const void* org,
                   const void* dir, CameraRaysArgs& A)
{
    if (!cam || !p) return fail(TRT_EINVAL, "null camera/params");
    if (p->width < 1 || p->height < 1) return fail(TRT_EINVAL, "width and height must be >= 1");
    if ((uint64_t)p->width * (uint64_t)p->height > 0x100000000ull) return fail(TRT_EINVAL, "image too large (pixels are 32-bit indices)");
    if (sample_begin < 0 || sample_begin > sample_end) return fail(TRT_EINVAL, "sample range must satisfy 0 <= begin <= end");
    if (n_pixels > 0 && (!pixels || !org || !dir)) return fail(TRT_EINVAL, "null pixel list or ray arrays");
    A.cam = *cam;
    A.width = p->width;
    A.height = p->height;
    A.seed = p->seed;
    A.fixed_pixels = (p->flags & TRT_FLAG_FIXED_PIXELS) ? 1u : 0u;
    A.grid_ok = (p->width >= 2 && p->height >= 2 && p->width <= 65536 && p->height <= 65536) ? 1u : 0u;
    A.grid_rcp[0] = 1.0 / double(p->width - 1.0);
    A.grid_rcp[1] = 1.0 / double(p->height - 1.0);
    A.grid_rcp[2] = 1.0 / double(p->width);
    A.grid_rcp[3] = 1.0 / double(p->height);
    return TRT_OK;
}
}  // namespace

int trt_render_rays(trt_handle* h, const trt_params* p, uint32_t n, const float* org, const float* dir, const uint32_t* stream, int32_t sample_begin,
                    int32_t sample_end, double* sum_host, double* sumsq_host, trt_stats* stats)
{
    return renderRays(h, p, n, org, dir, stream, sample_begin, sample_end, sum_host, sumsq_host, nullptr, stats, true);
}

int trt_render_rays_device(trt_handle* h, const trt_params* p, uint32_t n, const float* org_dev, const float* dir_dev, const uint32_t* stream_dev,
                           int32_t sample_begin, int32_t sample_end, double* sum_dev, double* sumsq_dev, void* hip_stream, trt_stats* stats)
{
    return renderRays(h, p, n, org_dev, dir_dev, stream_dev, sample_begin, sample_end, sum_dev, sumsq_dev, hip_stream, stats, false);
}

int trt_camera_rays(const trt_camera* cam, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels, int32_t sample_begin, int32_t sample_end,
                    float* org_host, float* dir_host)
{
    CameraRaysArgs A;
    if (int e = cameraRaysArgs(cam, p, n_pixels, pixels, sample_begin, sample_end, org_host, dir_host, A)) return e;
    const uint64_t n_image = (uint64_t)p->width * (uint64_t)p->height;
    for (uint32_t i = 0; i < n_pixels; ++i)
        if (pixels[i] >= n_image) return fail(TRT_EINVAL, "pixel list holds an entry >= width * height");
    for (int32_t s = sample_begin; s < sample_end; ++s)
        for (uint32_t i = 0; i < n_pixels; ++i) {
            f3 o, d;
            cameraRayOf(A.cam, A.width, A.height, A.seed, pixels[i], (uint32_t)s, A.fixed_pixels != 0u, A.grid_ok ? A.grid_rcp : nullptr, o, d);
            const size_t at = ((size_t)(s - sample_begin) * n_pixels + i) * 3;
            org_host[at] = o.x; org_host[at + 1] = o.y; org_host[at + 2] = o.z;
            dir_host[at] = d.x; dir_host[at + 1] = d.y; dir_host[at + 2] = d.z;
        }
    return TRT_OK;
}

int trt_camera_rays_device(int device, const trt_camera* cam, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels_dev, int32_t sample_begin,
                           int32_t sample_end, float* org_dev, float* dir_dev, void* hip_stream)
{
    CameraRaysArgs A;
    if (int e = cameraRaysArgs(cam, p, n_pixels, pixels_dev, sample_begin, sample_end, org_dev, dir_dev, A)) return e;
    if (n_pixels == 0 || sample_begin == sample_end) return TRT_OK;
    if (int e = useDevice(device)) return e;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint32_t* d_bad = nullptr;
    HIPC(hipMalloc((void**)&d_bad, sizeof(uint32_t)));
    const uint32_t n_samples = (uint32_t)(sample_end - sample_begin);
    uint32_t bad = 0;
    hipError_t err = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), stream);
    if (err == hipSuccess) {
        const dim3 grid(std::min<uint32_t>((n_pixels + 255) / 256, 8192u), std::min<uint32_t>(n_samples, 64u));
        hipLaunchKernelGGL(k_camera_rays, grid, dim3(256), 0, stream, A, pixels_dev, n_pixels, (uint32_t)sample_begin, n_samples, org_dev, dir_dev, d_bad);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, stream);
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    (void)hipFree(d_bad);
    if (err != hipSuccess) return fail(TRT_EHIP, std::string("trt_camera_rays_device: ") + hipGetErrorString(err));
    if (bad) return fail(TRT_EINVAL, "pixel list holds an entry >= width * height");
    return TRT_OK;
}

int trt_render(trt_handle* h, const trt_params* p, float* out_host, trt_stats* stats)
{
    if (int e = checkParams(h, p)) return e;
    if (int e = checkEstimator(p)) return e;
    if (!out_host) return fail(TRT_EINVAL, "null output buffer");
    return renderTile(h, p, 0u, (uint32_t)p->spp, nullptr, out_host, nullptr, stats, nullptr);
}

int trt_render_aov(trt_handle* h, const trt_params* p, float* albedo_host, float* normal_host, float* depth_host, trt_stats* stats)
{
    return renderAov(h, p, albedo_host, normal_host, depth_host, true, nullptr, stats);
}

int trt_render_aov_device(trt_handle* h, const trt_params* p, float* albedo_dev, float* normal_dev, float* depth_dev, void* hip_stream, trt_stats* stats)
{
    return renderAov(h, p, albedo_dev, normal_dev, depth_dev, false, hip_stream, stats);
}

int trt_aov_rays(trt_handle* h, const trt_params* p, uint32_t n, const float* org, const float* dir, int32_t sample_begin, int32_t sample_end,
                 double* albedo_sum_host, double* normal_sum_host, double* depth_sum_host, trt_stats* stats)
{
    return aovRays(h, p, n, org, dir, sample_begin, sample_end, albedo_sum_host, normal_sum_host, depth_sum_host, true, nullptr, stats);
}

int trt_aov_rays_device(trt_handle* h, const trt_params* p, uint32_t n, const float* org_dev, const float* dir_dev, int32_t sample_begin, int32_t sample_end,
                        double* albedo_sum_dev, double* normal_sum_dev, double* depth_sum_dev, void* hip_stream, trt_stats* stats)
{
    return aovRays(h, p, n, org_dev, dir_dev, sample_begin, sample_end, albedo_sum_dev, normal_sum_dev, depth_sum_dev, false, hip_stream, stats);
}

namespace {
// A ray batch of the query entries: the caller's arrays, on the host or on the handle's device.
struct RayBatch {
    const float* org;
    const float* dir;
    const float* t_max;  // null: TRT_INF for every ray
    float* t;            // closest hits (t, tri, uv); uv may be null
    int32_t* tri;
    float* uv;
    uint8_t* occluded;   // occlusion
    // trt_trace_points*: other coordinates of the handle's triangles and the points on them; t, tri and uv are then null
    const float* tri_v_other = nullptr;
    float* point = nullptr;
};

// The ray-batch entries (trt_trace_closest*, trt_trace_occluded*): the checks of include/trt.h, the rays packed into io_buf (host arrays staged
// there first), one traversal launch with k_trace_fix behind it, then for closest hits k_unpack_hits (trt_trace_points*: k_hit_points) into the
// caller's arrays (device entries) or into io_buf and from there to the host.  query: QUERY_NONE (no bound: trt_trace_closest's own kernels, k_trace_closest), QUERY_CLOSEST or
// QUERY_OCCLUDED (k_trace_query, the bound in rb.w).  Host entries run on the null stream and copy after it is synchronised.
int traceBatch(trt_handle* h, uint64_t n, const RayBatch& io, int query, bool host, hipStream_t stream, trt_stats* stats_out, const char* what)
{
    const bool occ = query == QUERY_OCCLUDED, pts = io.tri_v_other || io.point;
    if (!h || !io.org || !io.dir || (occ ? !io.occluded : pts ? (!io.tri_v_other || !io.point) : (!io.t || !io.tri)))
        return fail(TRT_EINVAL, std::string(what) + ": null argument");
    if (n == 0) return TRT_OK;
    if (n > 0x7FFF0000ull) return fail(TRT_EINVAL, "ray batch too large");
    HIPC(hipSetDevice(h->device));
    const uint32_t n32 = (uint32_t)n;
    const size_t in_bytes = (size_t)n * 3 * sizeof(float), q16 = (size_t)n * sizeof(f4), f_bytes = (size_t)n * sizeof(float);
    // host entries stage the caller's rays (org, dir, t_max) and, once they are packed, the results over them (t, tri, uv; or the bytes)
    const size_t stage_in = 2 * in_bytes + (io.t_max ? f_bytes : 0), stage_out = occ ? (size_t)n : pts ? in_bytes : (io.uv ? 4 : 2) * f_bytes;
    const size_t other_bytes = (size_t)h->sc.n_tris * 9 * sizeof(float);  // tri_v_other of a host call, staged beside the rays
    // io_buf: the packed rays, the hit records (8 bytes on a hit8 scene; none for occlusion), the staging area of a host call, then the block
    // cleared first (DeviceStats, the redo counters) and the redo list
    Layout L;
    const size_t o_ra = L.add(q16, 16), o_rb = L.add(q16, 16), o_hit = L.add(occ ? 0 : (h->hit8 ? q16 / 2 : q16), 16);
    const size_t o_stage = L.add(host ? std::max(stage_in, stage_out) : 0, 16), o_other = L.add(host && pts ? other_bytes : 0, 16);
    const size_t o_stats = L.add(sizeof(DeviceStats), 256), o_redo = L.add(2 * sizeof(uint32_t), 64), o_idx = L.add((size_t)n * sizeof(uint32_t), 256);
    if (int e = h->io_buf.ensure(L.bytes)) return e;
    char* b = (char*)h->io_buf.p;
    f4* ra = (f4*)(b + o_ra);
    f4* rb = (f4*)(b + o_rb);
    f4* hit = (f4*)(b + o_hit);
    char* stage = b + o_stage;
    DeviceStats* d_stats = (DeviceStats*)(b + o_stats);
    const RedoList redo{(uint32_t*)(b + o_redo), (uint32_t*)(b + o_idx)};  // rays for k_trace_fix (trt_kernels.h)
    RayBatch dev = io;  // where the kernels read and write
    CallFrame fr(h, stream, false);  // its Timer for the handle's events 0 and 1, which bracket the traversal alone: no span, no render_ms
    fr.arm();  // from the first copy on something writes io_buf, which the next call on the handle reuses
    if (host) {
        dev.org = (const float*)stage;
        dev.dir = (const float*)(stage + in_bytes);
        dev.t_max = io.t_max ? (const float*)(stage + 2 * in_bytes) : nullptr;
        dev.t = (float*)stage;
        dev.tri = (int32_t*)(stage + f_bytes);
        dev.uv = io.uv ? (float*)(stage + 2 * f_bytes) : nullptr;
        dev.occluded = (uint8_t*)stage;
        if (pts) {
            dev.point = (float*)stage;
            dev.tri_v_other = (const float*)(b + o_other);
            HIPC(hipMemcpyAsync((void*)dev.tri_v_other, io.tri_v_other, other_bytes, hipMemcpyHostToDevice, stream));
        }
        HIPC(hipMemcpyAsync((void*)dev.org, io.org, in_bytes, hipMemcpyHostToDevice, stream));
        HIPC(hipMemcpyAsync((void*)dev.dir, io.dir, in_bytes, hipMemcpyHostToDevice, stream));
        if (io.t_max) HIPC(hipMemcpyAsync((void*)dev.t_max, io.t_max, f_bytes, hipMemcpyHostToDevice, stream));
    }
    if (int e = fr.clear(d_stats, o_idx - o_stats)) return e;
    const dim3 grid(std::min<uint32_t>((n32 + 255) / 256, 65536u)), block(256);
    if (query == QUERY_NONE) hipLaunchKernelGGL(k_pack_rays, grid, block, 0, stream, dev.org, dev.dir, ra, rb, n32);
    else hipLaunchKernelGGL(k_pack_rays_bounded, grid, block, 0, stream, dev.org, dev.dir, dev.t_max, ra, rb, n32);
    hipEvent_t e0 = fr.tm.get(0), e1 = fr.tm.get(1);
    if (!e0 || !e1) return fail(TRT_EHIP, "hipEventCreate failed");
    HIPC(hipEventRecord(e0, stream));
    RaySource src{};
    src.ra = ra;
    src.rb = rb;
    if (query == QUERY_NONE)  // a scene with 8-byte hit records traces the batch with the render's kernel, and k_unpack_hits<true> widens its records
        launchTraceClosest(h, closestKernel(h, true, 0), fixKernel(h, false, 0), stream, (uint32_t*)h->spill.p, src, hit, n32, d_stats, redo);
    else
        launchTraceClosest(h, queryKernel(h, query), queryFixKernel(h, query), stream, (uint32_t*)h->spill.p, src, occ ? (f4*)dev.occluded : hit, n32, d_stats, redo);
    HIPC(hipEventRecord(e1, stream));
    if (pts)
        hipLaunchKernelGGL(h->hit8 ? k_hit_points<true> : k_hit_points<false>, grid, block, 0, stream, h->sc, (const f4*)ra, (const f4*)rb, (const f4*)hit, dev.tri_v_other, dev.point, n32);
    else if (!occ)
        hipLaunchKernelGGL(h->hit8 ? k_unpack_hits<true> : k_unpack_hits<false>, grid, block, 0, stream, h->sc, (const f4*)ra, (const f4*)rb, (const f4*)hit, dev.t, dev.tri, dev.uv, n32);
    if (int e = fr.readBack()) return e;
    if (int e = fr.finish(nullptr, 0)) return e;  // the counters are in fr.st; the caller's stats wait for the bracket's time and the host entry's copies
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, e0, e1));
    if (host) {
        if (occ) HIPC(hipMemcpy(io.occluded, dev.occluded, n, hipMemcpyDeviceToHost));
        else if (pts) HIPC(hipMemcpy(io.point, dev.point, in_bytes, hipMemcpyDeviceToHost));
        else {
            HIPC(hipMemcpy(io.t, dev.t, f_bytes, hipMemcpyDeviceToHost));
            HIPC(hipMemcpy(io.tri, dev.tri, f_bytes, hipMemcpyDeviceToHost));
            if (io.uv) HIPC(hipMemcpy(io.uv, dev.uv, 2 * f_bytes, hipMemcpyDeviceToHost));
        }
    }
    if (stats_out) {
        *stats_out = fr.st;  // what the traversal and fix kernels do not count is zero: d_stats was cleared
        const int k = occ ? TRT_K_TRACE_SHADOW : TRT_K_TRACE_CLOSEST;
        stats_out->kernel_ms[k] = ms;
        stats_out->launches[k] = 1;
        if (occ) stats_out->rays_shadow = n;
    }
    return TRT_OK;
}
}  // namespace

int trt_trace_closest(trt_handle* h, uint64_t n, const float* org, const float* dir, float* t, int32_t* tri, float* uv, trt_stats* stats_out)
{
    return traceBatch(h, n, RayBatch{org, dir, nullptr, t, tri, uv, nullptr}, QUERY_NONE, true, nullptr, stats_out, "trt_trace_closest");
}

int trt_trace_closest_range(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max, float* t, int32_t* tri, float* uv,
                            trt_stats* stats)
{
    return traceBatch(h, n, RayBatch{org, dir, t_max, t, tri, uv, nullptr}, t_max ? QUERY_CLOSEST : QUERY_NONE, true, nullptr, stats, "trt_trace_closest_range");
}

int trt_trace_closest_device(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max, float* t, int32_t* tri, float* uv,
                             void* hip_stream, trt_stats* stats)
{
    return traceBatch(h, n, RayBatch{org, dir, t_max, t, tri, uv, nullptr}, t_max ? QUERY_CLOSEST : QUERY_NONE, false, (hipStream_t)hip_stream, stats,
                      "trt_trace_closest_device");
}

namespace {
// trt_trace_points*: the checks that come before traceBatch's own (a null array, then the triangle count)
int tracePoints(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* tri_v_other, uint32_t n_tris, float* point, bool host,
                hipStream_t stream, trt_stats* stats, const char* what)
{
    if (!h || !org || !dir || !tri_v_other || !point) return fail(TRT_EINVAL, std::string(what) + ": null argument");
    if (n_tris != h->sc.n_tris) return fail(TRT_EINVAL, std::string(what) + ": n_tris differs from the handle's");
    RayBatch io{org, dir, nullptr, nullptr, nullptr, nullptr, nullptr};
    io.tri_v_other = tri_v_other;
    io.point = point;
    return traceBatch(h, n, io, QUERY_NONE, host, stream, stats, what);
}
}  // namespace

int trt_trace_points(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* tri_v_other, uint32_t n_tris, float* point,
                     trt_stats* stats)
{
    return tracePoints(h, n, org, dir, tri_v_other, n_tris, point, true, nullptr, stats, "trt_trace_points");
}

int trt_trace_points_device(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* tri_v_other, uint32_t n_tris, float* point,
                            void* hip_stream, trt_stats* stats)
{
    return tracePoints(h, n, org, dir, tri_v_other, n_tris, point, false, (hipStream_t)hip_stream, stats, "trt_trace_points_device");
}

int trt_trace_occluded(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max, uint8_t* occluded, trt_stats* stats)
{
    return traceBatch(h, n, RayBatch{org, dir, t_max, nullptr, nullptr, nullptr, occluded}, QUERY_OCCLUDED, true, nullptr, stats, "trt_trace_occluded");
}

int trt_trace_occluded_device(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max, uint8_t* occluded, void* hip_stream,
                              trt_stats* stats)
{
    return traceBatch(h, n, RayBatch{org, dir, t_max, nullptr, nullptr, nullptr, occluded}, QUERY_OCCLUDED, false, (hipStream_t)hip_stream, stats,
                      "trt_trace_occluded_device");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ device groups
namespace {
// The five RCCL entry points the gather needs, bound at run time: a single-GPU user of this library never loads RCCL.
struct Rccl {
    void* lib = nullptr;
    int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
    int (*CommDestroy)(void* comm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Gather)(const void* send, void* recv, size_t count, int datatype, int root, void* comm, hipStream_t stream) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load(std::string& err)
    {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("cannot load librccl.so.1: ") + dlerror(); return false; }
        auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) err = std::string("librccl: missing symbol ") + n; return p; };
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
        Gather = reinterpret_cast<decltype(Gather)>(sym("ncclGather"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        return CommInitAll && CommDestroy && GroupStart && GroupEnd && Gather && GetErrorString;
    }
};
constexpr int NCCL_FLOAT32 = 7;  // ncclFloat32 (rccl.h ncclDataType_t)

// packed stripes of rank r (rows in increasing y) -> their rows of the tile image
__global__ __launch_bounds__(256) void k_uninterleave(const float* __restrict__ gathered, float* __restrict__ image, uint32_t tile_rows, uint32_t row_floats,
                                                       uint32_t row_block, uint32_t n_ranks, uint32_t pad_rows)
{
    const uint64_t total = (uint64_t)tile_rows * row_floats;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(i / row_floats), x = (uint32_t)(i - (uint64_t)y * row_floats);
        const uint32_t stripe = y / row_block, rank = stripe % n_ranks;
        const uint32_t packed = (stripe / n_ranks) * row_block + (y - stripe * row_block);  // row of y inside rank's packed buffer
        image[i] = gathered[((uint64_t)rank * pad_rows + packed) * row_floats + x];
    }
}
}  // namespace

// One host thread per device for the life of the group: it binds its device once and renders its stripes whenever the
// group posts a job (trt_group_render used to create and join n threads per call).
struct GroupWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t posted = 0, finished = 0;  // job sequence numbers
    bool quit = false;
    // the job
    trt_handle* h = nullptr;
    trt_params p{};
    float* out = nullptr;
    hipStream_t stream = nullptr;
    bool skip = false;  // more devices than stripes: nothing to render
    // its result
    int rc = TRT_OK;
    std::string msg;
    trt_stats st{};
};

struct trt_group {
    std::vector<trt_handle*> handles;
    std::vector<int> devices;
    bool use_rccl = false;       // every entry another device (or the one-device test switch): RCCL gathers; else device copies (one-GPU rehearsal)
    Rccl rccl;
    std::vector<void*> comms;
    std::vector<hipStream_t> streams;
    std::vector<DevBuf> stripe;  // per rank: its packed stripes, padded to the largest rank's row count
    DevBuf gathered, image;      // on devices[0]
    std::vector<std::unique_ptr<GroupWorker>> workers;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // on devices[0]: around gather + un-interleave
    void startWorkers()
    {
        for (size_t k = 0; k < handles.size(); ++k) {
            workers.emplace_back(new GroupWorker);
            GroupWorker* w = workers.back().get();
            const int dev = devices[k];
            w->th = std::thread([w, dev]() {
                (void)hipSetDevice(dev);
                std::unique_lock<std::mutex> lk(w->mu);
                for (;;) {
                    w->cv.wait(lk, [w]() { return w->quit || w->posted != w->finished; });
                    if (w->quit) return;
                    lk.unlock();
                    if (w->skip) { std::memset(&w->st, 0, sizeof(w->st)); w->rc = TRT_OK; }
                    else {
                        w->rc = trt_render_device(w->h, &w->p, w->out, w->stream, &w->st);
                        if (w->rc) w->msg = trt_last_error();  // thread-local in the worker: carried over by hand
                    }
                    lk.lock();
                    w->finished = w->posted;
                    w->cv.notify_all();
                }
            });
        }
    }
    ~trt_group()
    {
        for (auto& w : workers) {
            { std::lock_guard<std::mutex> lk(w->mu); w->quit = true; }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
        for (size_t k = 0; k < handles.size(); ++k) {
            (void)hipSetDevice(devices[k]);
            if (k < stripe.size()) stripe[k].release();
            if (k < streams.size() && streams[k]) (void)hipStreamDestroy(streams[k]);
            if (k < comms.size() && comms[k]) (void)rccl.CommDestroy(comms[k]);
            trt_destroy(handles[k]);
        }
        if (!devices.empty()) (void)hipSetDevice(devices[0]);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        gathered.release();
        image.release();
        if (rccl.lib) dlclose(rccl.lib);
    }
};

extern "C" {

int trt_group_size(const trt_group* g) { return g ? (int)g->handles.size() : 0; }

void trt_group_destroy(trt_group* g) { delete g; }

int trt_group_create(const trt_scene* scene, int n_devices, const int* devices, trt_group** out)
{
    if (!scene || !devices || !out || n_devices < 1 || n_devices > 64) return fail(TRT_EINVAL, "trt_group_create: bad argument");
    *out = nullptr;
    std::unique_ptr<trt_group> g(new trt_group);
    bool distinct = true;
    for (int a = 0; a < n_devices; ++a)
        for (int b = a + 1; b < n_devices; ++b)
            if (devices[a] == devices[b]) distinct = false;
    const char* force = std::getenv("TRT_GROUP_FORCE_RCCL");  // test switch: a group of one device takes the RCCL route too
    g->use_rccl = distinct && (n_devices > 1 || (force && std::atoi(force) != 0));
    {   // the host half of trt_create once (checks, collapses: seconds for 10 M triangles), the device half per member, side by side
        SceneImage im;
        if (int e = buildSceneImage(scene, im)) return e;
        std::vector<trt_handle*> hs(n_devices, nullptr);
        std::vector<int> rc(n_devices, TRT_OK);
        std::vector<std::string> msg(n_devices);
        std::vector<std::thread> th;
        for (int k = 0; k < n_devices; ++k)
            th.emplace_back([&, k] {
                rc[k] = createOnDevice(im, devices[k], &hs[k]);
                if (rc[k] != TRT_OK) msg[k] = trt_last_error();  // the message lives in this thread
            });
        for (std::thread& t : th) t.join();
        for (int k = 0; k < n_devices; ++k) {
            if (hs[k]) { g->handles.push_back(hs[k]); g->devices.push_back(devices[k]); }  // (owned by the group from here: freed with it on failure)
        }
        for (int k = 0; k < n_devices; ++k)
            if (rc[k] != TRT_OK) return fail(rc[k], msg[k]);  // TRT_ENODEV for an ordinal the node does not have
    }
    g->stripe.resize(n_devices);
    g->streams.assign(n_devices, nullptr);
    for (int k = 0; k < n_devices; ++k) {
        HIPC(hipSetDevice(devices[k]));
        HIPC(hipStreamCreateWithFlags(&g->streams[k], hipStreamNonBlocking));
    }
    HIPC(hipSetDevice(devices[0]));
    HIPC(hipEventCreate(&g->ev0));
    HIPC(hipEventCreate(&g->ev1));
    if (g->use_rccl) {
        std::string err;
        if (!g->rccl.load(err)) return fail(TRT_EHIP, err);
        g->comms.assign(n_devices, nullptr);
        const int rc = g->rccl.CommInitAll(g->comms.data(), n_devices, devices);
        if (rc != 0) return fail(TRT_EHIP, std::string("ncclCommInitAll: ") + g->rccl.GetErrorString(rc));
    }
    g->startWorkers();
    *out = g.release();
    return TRT_OK;
}

int trt_group_render_device(trt_group* g, const trt_params* p_in, float* out_dev0, trt_stats* stats_out, double* gather_ms_out)
{
    if (!g || !p_in || !out_dev0) return fail(TRT_EINVAL, "trt_group_render_device: null argument");
    const int n = (int)g->handles.size();
    trt_params p = *p_in;
    if (p.row_block <= 0) p.row_block = 8;
    p.row_mod = n;
    p.row_rem = 0;
    if (int e = checkParams(g->handles[0], &p)) return e;
    if (int e = checkEstimator(&p)) return e;
    const uint32_t tile_rows = (uint32_t)(p.y1 - p.y0), tw = (uint32_t)(p.x1 - p.x0), row_floats = tw * 3u;
    // Rows are selected on absolute y (stripes are counted from image row 0), and k_uninterleave computes the packed index the
    // same way only if the tile starts on a stripe boundary of rank 0: require that.
    if (p.y0 % (p.row_block * n) != 0) return fail(TRT_EINVAL, "trt_group_render: y0 must be a multiple of row_block * group size");
    uint32_t pad_rows = 0;
    std::vector<uint32_t> rows_of(n);
    for (int k = 0; k < n; ++k) {
        trt_params pk = p;
        pk.row_rem = k;
        rows_of[k] = (uint32_t)std::max(trt_rows_selected(&pk), 0);
        pad_rows = std::max(pad_rows, rows_of[k]);
    }
    const size_t stripe_bytes = (size_t)pad_rows * row_floats * sizeof(float);
    for (int k = 0; k < n; ++k) {
        HIPC(hipSetDevice(g->devices[k]));
        if (int e = g->stripe[k].ensure(stripe_bytes)) return e;
    }
    HIPC(hipSetDevice(g->devices[0]));
    if (int e = g->gathered.ensure(stripe_bytes * (size_t)n)) return e;

    // ---- every device renders its stripes on its own (resident) host thread
    for (int k = 0; k < n; ++k) {
        GroupWorker* w = g->workers[k].get();
        std::lock_guard<std::mutex> lk(w->mu);
        w->h = g->handles[k];
        w->p = p;
        w->p.row_rem = k;
        w->out = (float*)g->stripe[k].p;
        w->stream = g->streams[k];
        w->skip = rows_of[k] == 0;
        w->posted++;
        w->cv.notify_all();
    }
    for (int k = 0; k < n; ++k) {
        GroupWorker* w = g->workers[k].get();
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv.wait(lk, [w]() { return w->posted == w->finished; });
    }
    for (int k = 0; k < n; ++k)
        if (g->workers[k]->rc) return fail(g->workers[k]->rc, "device " + std::to_string(g->devices[k]) + ": " + g->workers[k]->msg);

    // ---- ONE gather to devices[0], then un-interleave there (every worker's stream is idle: trt_render_device synchronises it)
    HIPC(hipSetDevice(g->devices[0]));
    HIPC(hipEventRecord(g->ev0, g->streams[0]));
    const size_t count = (size_t)pad_rows * row_floats;
    if (g->use_rccl) {
        // Between GroupStart and GroupEnd nothing returns: an error is remembered, the group is closed, then it is reported.
        int rc = g->rccl.GroupStart();
        hipError_t herr = hipSuccess;
        if (rc == 0) {
            for (int k = 0; k < n && rc == 0 && herr == hipSuccess; ++k) {
                herr = hipSetDevice(g->devices[k]);
                // (a rank that is not the root receives nothing; it still gets a valid pointer — its own stripe — in case a build of the library checks the argument)
                if (herr == hipSuccess) rc = g->rccl.Gather(g->stripe[k].p, k == 0 ? g->gathered.p : g->stripe[k].p, count, NCCL_FLOAT32, 0, g->comms[k], g->streams[k]);
            }
            const int rc_end = g->rccl.GroupEnd();
            if (rc == 0) rc = rc_end;
        }
        (void)hipSetDevice(g->devices[0]);
        if (herr != hipSuccess) return fail(TRT_EHIP, std::string("hipSetDevice inside the gather: ") + hipGetErrorString(herr));
        if (rc != 0) return fail(TRT_EHIP, std::string("ncclGather: ") + g->rccl.GetErrorString(rc));
    } else {
        for (int k = 0; k < n; ++k)
            HIPC(hipMemcpyAsync((char*)g->gathered.p + stripe_bytes * (size_t)k, g->stripe[k].p, stripe_bytes, hipMemcpyDeviceToDevice, g->streams[0]));
    }
    // the root's share of the gather runs on streams[0]: the kernel below is ordered behind it by the stream
    const uint64_t total = (uint64_t)tile_rows * row_floats;
    hipLaunchKernelGGL(k_uninterleave, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536ull)), dim3(256), 0, g->streams[0], (const float*)g->gathered.p,
                       out_dev0, tile_rows, row_floats, (uint32_t)p.row_block, (uint32_t)n, pad_rows);
    HIPC(hipEventRecord(g->ev1, g->streams[0]));
    HIPC(hipStreamSynchronize(g->streams[0]));
    HIPC(hipGetLastError());
    if (g->use_rccl)  // the senders' stripes may be overwritten by the next render only after their part of the gather has left
        for (int k = 1; k < n; ++k) { HIPC(hipSetDevice(g->devices[k])); HIPC(hipStreamSynchronize(g->streams[k])); }
    HIPC(hipSetDevice(g->devices[0]));
    float gms = 0.f;
    HIPC(hipEventElapsedTime(&gms, g->ev0, g->ev1));
    if (gather_ms_out) *gather_ms_out = gms;
    if (stats_out) {
        trt_stats t;
        std::memset(&t, 0, sizeof(t));
        for (int k = 0; k < n; ++k) {
            const trt_stats& s = g->workers[k]->st;
            t.rays_camera += s.rays_camera; t.rays_shadow += s.rays_shadow; t.rays_indirect += s.rays_indirect; t.shaded_hits += s.shaded_hits;
            for (int i = 0; i < 2; ++i) { t.inner_visits[i] += s.inner_visits[i]; t.tri_tests[i] += s.tri_tests[i]; t.wave_steps[i] += s.wave_steps[i]; }
            for (int i = 0; i < TRT_MAX_KERNELS; ++i) { t.launches[i] += s.launches[i]; t.kernel_ms[i] += s.kernel_ms[i]; }
            t.render_ms = std::max(t.render_ms, s.render_ms);
            t.passes = std::max(t.passes, s.passes);
            t.max_bounces = std::max(t.max_bounces, s.max_bounces);
            t.rows_rendered += s.rows_rendered;
            t.inner_node_bytes = std::max(t.inner_node_bytes, s.inner_node_bytes);
            t.redo_rays += s.redo_rays;
            for (int i = 0; i < 4; ++i) t.lane_census[i] += s.lane_census[i];
        }
        *stats_out = t;
    }
    return TRT_OK;
}

int trt_group_render(trt_group* g, const trt_params* p_in, float* out_host, trt_stats* stats_out, double* gather_ms_out)
{
    if (!g || !p_in || !out_host) return fail(TRT_EINVAL, "trt_group_render: null argument");
    if (p_in->x1 <= p_in->x0 || p_in->y1 <= p_in->y0) return fail(TRT_EINVAL, "tile rectangle outside the image or empty");
    const size_t bytes = (size_t)(p_in->y1 - p_in->y0) * (size_t)(p_in->x1 - p_in->x0) * 3 * sizeof(float);
    HIPC(hipSetDevice(g->devices[0]));
    if (int e = g->image.ensure(bytes)) return e;
    if (int e = trt_group_render_device(g, p_in, (float*)g->image.p, stats_out, gather_ms_out)) return e;
    HIPC(hipSetDevice(g->devices[0]));
    HIPC(hipMemcpy(out_host, g->image.p, bytes, hipMemcpyDeviceToHost));
    return TRT_OK;
}

}  // extern "C"

// ---- trt_denoise / trt_denoise_device ----------------------------------------------------------------------------------------------

namespace {

struct DenoiseIo {
    const float *color, *variance, *albedo, *normal, *depth;
    float* out;
};

// The skeleton the image-space passes share (trt_denoise, trt_reproject, trt_reproject_motion, trt_reproject_moments and their _device
// entries): the planes of one call, each width*height*{1,3,4} floats, its scratch, its four events and its statistics.  A host entry stages
// the present planes through one allocation; a device entry uses the caller's pointers in place and, without scratch, allocates nothing.
// The driver lists its planes once (in / out / scratch return the plane's index), calls begin(), launches on S[index], calls finish().
// Everything is released on every way out.
struct ImageStage {
    enum Kind { IN, OUT, SCRATCH };
    struct Plane {
        Kind kind;
        void* user;     // the caller's array; null for scratch
        size_t bytes;
        bool present;   // an absent plane is neither staged nor copied, and the kernels get a null pointer for it
        void* dev;      // after begin(): the staging (host entries, scratch) or `user`
    };
    const size_t pixels;
    const bool host;
    std::vector<Plane> planes;
    hipStream_t stream = nullptr;
    void* p = nullptr;
    EventBracket bracket;

    ImageStage(int width, int height, bool host_) : pixels((size_t)width * (size_t)height), host(host_) {}
    ImageStage(const ImageStage&) = delete;
    ~ImageStage()
    {
        if (p) (void)hipFree(p);
    }
    int add(Kind kind, const void* user, size_t bytes, bool present)
    {
        planes.push_back(Plane{kind, const_cast<void*>(user), bytes, present, nullptr});
        return (int)planes.size() - 1;
    }
    int in(const float* user, int floats, bool present = true) { return add(IN, user, pixels * floats * sizeof(float), present); }
    int out(float* user, int floats, bool present = true) { return add(OUT, user, pixels * floats * sizeof(float), present); }
    int scratch(size_t bytes) { return add(SCRATCH, nullptr, bytes, true); }
    float* operator[](int i) const { return (float*)planes[i].dev; }

    // One hipMalloc for whatever is staged (256-byte aligned regions, in the order listed), then event 0, the inputs' upload, event 1.
    int begin(hipStream_t stream_)
    {
        stream = stream_;
        Layout L;
        std::vector<size_t> at(planes.size());
        for (size_t i = 0; i < planes.size(); ++i)
            if (staged(planes[i])) at[i] = L.add(planes[i].bytes, 256);
        if (L.bytes) HIPC(hipMalloc(&p, L.bytes));
        if (int e = bracket.create()) return e;
        for (size_t i = 0; i < planes.size(); ++i) planes[i].dev = staged(planes[i]) ? (char*)p + at[i] : planes[i].present ? planes[i].user : nullptr;
        if (int e = bracket.record(0, stream)) return e;
        for (const Plane& b : planes)
            if (b.kind == IN && staged(b)) HIPC(hipMemcpyAsync(b.dev, b.user, b.bytes, hipMemcpyHostToDevice, stream));
        return bracket.record(1, stream);
    }
    // Behind the launches: event 2, the outputs' download, event 3, the wait, and the statistics of the `launches` kernels.
    int finish(trt_stats* stats, uint64_t launches)
    {
        HIPC(hipGetLastError());
        if (int e = bracket.record(2, stream)) return e;
        for (const Plane& b : planes)
            if (b.kind == OUT && staged(b)) HIPC(hipMemcpyAsync(b.user, b.dev, b.bytes, hipMemcpyDeviceToHost, stream));
        if (int e = bracket.record(3, stream)) return e;
        HIPC(hipStreamSynchronize(stream));
        HIPC(hipGetLastError());
        return bracket.fill(stats, TRT_K_DENOISE, launches);
    }

private:
    bool staged(const Plane& b) const { return b.present && (host || b.kind == SCRATCH); }
};

// The checks of include/trt.h; fills the level arguments (step 1) and the number of levels.
int denoiseArgs(const trt_denoise_params* prm, int width, int height, const DenoiseIo& io, trt_dn_args& a, int& levels, const char* what)
{
    if (!io.color || !io.variance || !io.albedo || !io.normal || !io.depth || !io.out) return fail(TRT_EINVAL, std::string(what) + ": null buffer");
    if (width < 1 || height < 1) return fail(TRT_EINVAL, std::string(what) + ": width and height must be >= 1");
    if ((uint64_t)width * (uint64_t)height > TRT_DENOISE_MAX_PIXELS) return fail(TRT_EINVAL, std::string(what) + ": image larger than 2^28 pixels");
    trt_denoise_params d{};
    if (prm) d = *prm;
    if (d.iterations < 0 || d.iterations > TRT_DENOISE_MAX_ITERATIONS) return fail(TRT_EINVAL, std::string(what) + ": iterations must be 0..10");
    if (d.sigma_normal < 0 || d.sigma_normal > 256) return fail(TRT_EINVAL, std::string(what) + ": sigma_normal must be 0..256");
    if (!(d.sigma_depth >= 0.0f) || !(d.sigma_luminance >= 0.0f)) return fail(TRT_EINVAL, std::string(what) + ": sigmas must be >= 0");
    if (d.flags != 0) return fail(TRT_EINVAL, std::string(what) + ": flags must be 0");
    levels = d.iterations ? d.iterations : TRT_DN_ITERATIONS;
    a.width = width;
    a.height = height;
    a.step = 1;
    a.sigma_normal = d.sigma_normal ? d.sigma_normal : TRT_DN_SIGMA_NORMAL;
    a.sigma_depth = d.sigma_depth != 0.0f ? d.sigma_depth : TRT_DN_SIGMA_DEPTH;
    a.sigma_luminance = d.sigma_luminance != 0.0f ? d.sigma_luminance : TRT_DN_SIGMA_LUMINANCE;
    return TRT_OK;
}

// One call: (host: upload) -> k_denoise_prepare -> k_denoise_level per level -> (host: download), all on `stream`.
// TRT_DENOISE_LDS=0 in the environment sends levels 0 and 1 through the global-memory kernel as well (A/B of the LDS tiles; same bits).
int denoise(int device, const trt_denoise_params* prm, int width, int height, const DenoiseIo& io, bool host, hipStream_t stream, trt_stats* stats,
            const char* what)
{
    trt_dn_args a{};
    int levels = 0;
    if (int e = denoiseArgs(prm, width, height, io, a, levels, what)) return e;
    if (int e = useDevice(device)) return e;
    const char* lds_env = std::getenv("TRT_DENOISE_LDS");
    const bool lds = !(lds_env && lds_env[0] == '0');
    const dim3 grid((unsigned)((width + DN_BX - 1) / DN_BX), (unsigned)((height + DN_BY - 1) / DN_BY)), block(DN_BX, DN_BY);
    ImageStage S(width, height, host);
    const size_t r16 = S.pixels * sizeof(trt_dn4);
    const int cv0 = S.scratch(r16), cv1 = S.scratch(r16), guide = S.scratch(r16), auxiliary = S.scratch(r16);
    const int color = S.in(io.color, 3), variance = S.in(io.variance, 1), albedo = S.in(io.albedo, 3), normal = S.in(io.normal, 3), depth = S.in(io.depth, 1);
    const int out = S.out(io.out, 3);
    if (int e = S.begin(stream)) return e;
    trt_dn4* cv[2] = {(trt_dn4*)S[cv0], (trt_dn4*)S[cv1]};
    trt_dn4 *gd = (trt_dn4*)S[guide], *aux = (trt_dn4*)S[auxiliary];
    hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, stream, width, height, S[color], S[variance], S[albedo], S[normal], S[depth], cv[0], gd, aux);
    for (int k = 0; k < levels; ++k) {
        a.step = 1 << k;
        const trt_dn4* in = cv[k & 1];
        trt_dn4* nxt = cv[(k + 1) & 1];
        const bool last = k + 1 == levels;
        const int lds_step = lds && a.step <= 2 ? a.step : 0;
        using LevelKernel = void (*)(trt_dn_args, const trt_dn4*, const trt_dn4*, const trt_dn4*, trt_dn4*, float*);
        static const LevelKernel table[3][2] = {{k_denoise_level<0, false>, k_denoise_level<0, true>},
                                                {k_denoise_level<1, false>, k_denoise_level<1, true>},
                                                {k_denoise_level<2, false>, k_denoise_level<2, true>}};
        hipLaunchKernelGGL(table[lds_step][last ? 1 : 0], grid, block, 0, stream, a, in, (const trt_dn4*)gd, (const trt_dn4*)aux, nxt, S[out]);
    }
    return S.finish(stats, 1 + (uint64_t)levels);
}

}  // namespace

extern "C" {

int trt_denoise(int device, const trt_denoise_params* params, int width, int height, const float* color, const float* variance,
                const float* albedo, const float* normal, const float* depth, float* out, trt_stats* stats)
{
    return denoise(device, params, width, height, DenoiseIo{color, variance, albedo, normal, depth, out}, true, nullptr, stats, "trt_denoise");
}

int trt_denoise_device(int device, const trt_denoise_params* params, int width, int height, const float* color, const float* variance,
                       const float* albedo, const float* normal, const float* depth, float* out, void* hip_stream, trt_stats* stats)
{
    return denoise(device, params, width, height, DenoiseIo{color, variance, albedo, normal, depth, out}, false, (hipStream_t)hip_stream, stats,
                   "trt_denoise_device");
}

}  // extern "C"

// ---- trt_despeckle / trt_despeckle_device ---------------------------------------------------------------------------------------------

namespace {

static_assert(sizeof(trt_despeckle_params) == 12, "trt_despeckle_params is three 4-byte fields (the ctypes mirror holds the same size)");

struct DespeckleIo {
    const float *color, *variance, *albedo, *depth;  // variance: optional, with out_variance
    float *out_color, *out_variance, *out_scale;     // out_scale: optional
};

// One call: (host: upload) -> k_despeckle -> (host: download), all on `stream`.
// TRT_DESPECKLE_LDS=0 in the environment sends the taps to global memory instead of the LDS tile (A/B; same bits).
int despeckle(int device, const trt_despeckle_params* prm, int width, int height, const DespeckleIo& io, bool host, hipStream_t stream, trt_stats* stats,
              const char* what)
{
    trt_ds_args a{};
    const bool required = io.color && io.albedo && io.depth && io.out_color;
    if (const char* msg = trt_ds_check(prm, width, height, required, (io.variance != nullptr) == (io.out_variance != nullptr), a))
        return fail(TRT_EINVAL, std::string(what) + ": " + msg);
    if (int e = useDevice(device)) return e;
    const char* lds_env = std::getenv("TRT_DESPECKLE_LDS");
    const bool lds = !(lds_env && lds_env[0] == '0');
    const bool var = io.variance != nullptr;
    const dim3 grid((unsigned)((width + DS_BX - 1) / DS_BX), (unsigned)((height + DS_BY - 1) / DS_BY)), block(DS_BX, DS_BY);
    ImageStage S(width, height, host);
    const int color = S.in(io.color, 3), variance = S.in(io.variance, 1, var), albedo = S.in(io.albedo, 3), depth = S.in(io.depth, 1);
    const int out_color = S.out(io.out_color, 3), out_variance = S.out(io.out_variance, 1, var), out_scale = S.out(io.out_scale, 1, io.out_scale != nullptr);
    if (int e = S.begin(stream)) return e;
    using Kernel = void (*)(trt_ds_args, const float*, const float*, const float*, const float*, float*, float*, float*);
    static const Kernel table[2][2] = {{k_despeckle<1, false>, k_despeckle<1, true>}, {k_despeckle<2, false>, k_despeckle<2, true>}};
    hipLaunchKernelGGL(table[a.radius - 1][lds ? 1 : 0], grid, block, 0, stream, a, (const float*)S[color], (const float*)S[variance],
                       (const float*)S[albedo], (const float*)S[depth], S[out_color], S[out_variance], S[out_scale]);
    return S.finish(stats, 1);
}

}  // namespace

extern "C" {

int trt_despeckle(int device, const trt_despeckle_params* params, int width, int height, const float* color, const float* variance,
                  const float* albedo, const float* depth, float* out_color, float* out_variance, float* out_scale, trt_stats* stats)
{
    return despeckle(device, params, width, height, DespeckleIo{color, variance, albedo, depth, out_color, out_variance, out_scale}, true, nullptr, stats,
                     "trt_despeckle");
}

int trt_despeckle_device(int device, const trt_despeckle_params* params, int width, int height, const float* color, const float* variance,
                         const float* albedo, const float* depth, float* out_color, float* out_variance, float* out_scale, void* hip_stream,
                         trt_stats* stats)
{
    return despeckle(device, params, width, height, DespeckleIo{color, variance, albedo, depth, out_color, out_variance, out_scale}, false,
                     (hipStream_t)hip_stream, stats, "trt_despeckle_device");
}

}  // extern "C"

// ---- trt_reproject / trt_reproject_device ---------------------------------------------------------------------------------------------

namespace {

struct ReprojectIo {
    const float *color, *variance, *albedo, *normal, *depth;
    const float* prev_point;  // trt_reproject_motion*: W*H*3, required there; null in trt_reproject*
    const float *prev_cv, *prev_len, *prev_normal, *prev_depth;
    float *out_color, *out_variance, *out_cv, *out_len;
};

// The checks of include/trt.h, in its order; fills the kernel's arguments.
int reprojectArgs(const trt_reproject_params* prm, int width, int height, const ReprojectIo& io, bool host, bool motion, trt_rp_args& a, const char* what)
{
    const bool required = io.color && io.variance && io.albedo && io.normal && io.depth && io.out_color && io.out_variance && io.out_cv && io.out_len &&
                          (!motion || io.prev_point);
    const int given = (io.prev_cv ? 1 : 0) + (io.prev_len ? 1 : 0) + (io.prev_normal ? 1 : 0) + (io.prev_depth ? 1 : 0);
    if (const char* msg = trt_rp_check(prm, width, height, required, given, a)) return fail(TRT_EINVAL, std::string(what) + ": " + msg);
    if (!host && ((((uintptr_t)io.out_cv) | ((uintptr_t)io.prev_cv)) & 15u)) return fail(TRT_EINVAL, std::string(what) + ": prev_cv and out_cv must be 16-byte aligned");
    return TRT_OK;
}

// One call: (host: upload) -> k_reproject, or k_reproject_motion with `motion` -> (host: download), all on `stream`.
int reproject(int device, const trt_reproject_params* prm, int width, int height, const ReprojectIo& io, bool host, hipStream_t stream, trt_stats* stats,
              const char* what, bool motion = false)
{
    trt_rp_args a{};
    if (int e = reprojectArgs(prm, width, height, io, host, motion, a, what)) return e;
    if (int e = useDevice(device)) return e;
    const bool hist = a.history != 0;
    const dim3 grid((unsigned)((width + RP_BX - 1) / RP_BX), (unsigned)((height + RP_BY - 1) / RP_BY)), block(RP_BX, RP_BY);
    ImageStage S(width, height, host);
    const int color = S.in(io.color, 3), variance = S.in(io.variance, 1), albedo = S.in(io.albedo, 3), normal = S.in(io.normal, 3), depth = S.in(io.depth, 1);
    const int prev_point = S.in(io.prev_point, 3, motion);
    const int prev_cv = S.in(io.prev_cv, 4, hist), prev_len = S.in(io.prev_len, 1, hist), prev_normal = S.in(io.prev_normal, 3, hist), prev_depth = S.in(io.prev_depth, 1, hist);
    const int out_color = S.out(io.out_color, 3), out_variance = S.out(io.out_variance, 1), out_cv = S.out(io.out_cv, 4), out_len = S.out(io.out_len, 1);
    if (int e = S.begin(stream)) return e;
    const trt_rp_fetch fetch{(const trt_dn4*)S[prev_cv], S[prev_len], S[prev_normal], S[prev_depth]};
    if (motion)
        hipLaunchKernelGGL(k_reproject_motion, grid, block, 0, stream, a, S[color], S[variance], S[albedo], S[normal], S[depth], S[prev_point], fetch,
                           S[out_color], S[out_variance], (trt_dn4*)S[out_cv], S[out_len]);
    else
        hipLaunchKernelGGL(k_reproject, grid, block, 0, stream, a, S[color], S[variance], S[albedo], S[normal], S[depth], fetch, S[out_color],
                           S[out_variance], (trt_dn4*)S[out_cv], S[out_len]);
    return S.finish(stats, 1);
}

}  // namespace

extern "C" {

int trt_reproject(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                  const float* albedo, const float* normal, const float* depth, const float* prev_cv, const float* prev_len,
                  const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance, float* out_cv, float* out_len,
                  trt_stats* stats)
{
    return reproject(device, params, width, height,
                     ReprojectIo{color, variance, albedo, normal, depth, nullptr, prev_cv, prev_len, prev_normal, prev_depth, out_color, out_variance, out_cv, out_len},
                     true, nullptr, stats, "trt_reproject");
}

int trt_reproject_device(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                         const float* albedo, const float* normal, const float* depth, const float* prev_cv, const float* prev_len,
                         const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance, float* out_cv,
                         float* out_len, void* hip_stream, trt_stats* stats)
{
    return reproject(device, params, width, height,
                     ReprojectIo{color, variance, albedo, normal, depth, nullptr, prev_cv, prev_len, prev_normal, prev_depth, out_color, out_variance, out_cv, out_len},
                     false, (hipStream_t)hip_stream, stats, "trt_reproject_device");
}

int trt_reproject_motion(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                         const float* albedo, const float* normal, const float* depth, const float* prev_point, const float* prev_cv,
                         const float* prev_len, const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance,
                         float* out_cv, float* out_len, trt_stats* stats)
{
    const ReprojectIo io{color, variance, albedo, normal, depth, prev_point, prev_cv, prev_len, prev_normal, prev_depth, out_color, out_variance, out_cv, out_len};
    return reproject(device, params, width, height, io, true, nullptr, stats, "trt_reproject_motion", true);
}

int trt_reproject_motion_device(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                                const float* albedo, const float* normal, const float* depth, const float* prev_point, const float* prev_cv,
                                const float* prev_len, const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance,
                                float* out_cv, float* out_len, void* hip_stream, trt_stats* stats)
{
    const ReprojectIo io{color, variance, albedo, normal, depth, prev_point, prev_cv, prev_len, prev_normal, prev_depth, out_color, out_variance, out_cv, out_len};
    return reproject(device, params, width, height, io, false, (hipStream_t)hip_stream, stats, "trt_reproject_motion_device", true);
}

}  // extern "C"

// ---- trt_reproject_moments / trt_reproject_moments_device ------------------------------------------------------------------------------

namespace {

struct MomentsIo {
    const float *color, *albedo, *normal, *depth, *prev_point;  // prev_point: optional
    const float *prev_cv, *prev_len, *prev_normal, *prev_depth, *prev_mom;
    float *out_color, *out_variance, *out_cv, *out_len, *out_mom;
};

// One call: (host: upload) -> k_reproject_moments -> k_moments_variance -> (host: download), all on `stream`.
// TRT_MOMENTS_LDS=0 in the environment sends stage B through its global-memory variant (A/B of the LDS tile; same bits).
int reprojectMoments(int device, const trt_moments_params* prm, int width, int height, const MomentsIo& io, bool host, hipStream_t stream,
                     trt_stats* stats, const char* what)
{
    trt_mv_args a{};
    const bool required = io.color && io.albedo && io.normal && io.depth && io.out_color && io.out_variance && io.out_cv && io.out_len && io.out_mom;
    const int given = (io.prev_cv ? 1 : 0) + (io.prev_len ? 1 : 0) + (io.prev_normal ? 1 : 0) + (io.prev_depth ? 1 : 0) + (io.prev_mom ? 1 : 0);
    if (const char* msg = trt_mv_check(prm, width, height, required, given, a)) return fail(TRT_EINVAL, std::string(what) + ": " + msg);
    if (!host && ((((uintptr_t)io.out_cv) | ((uintptr_t)io.prev_cv) | ((uintptr_t)io.out_mom) | ((uintptr_t)io.prev_mom)) & 15u))
        return fail(TRT_EINVAL, std::string(what) + ": prev_cv, out_cv, prev_mom and out_mom must be 16-byte aligned");
    if (int e = useDevice(device)) return e;
    const bool hist = a.rp.history != 0, motion = io.prev_point != nullptr;
    const char* lds_env = std::getenv("TRT_MOMENTS_LDS");
    const bool lds = !(lds_env && lds_env[0] == '0');
    const dim3 grid((unsigned)((width + MV_BX - 1) / MV_BX), (unsigned)((height + MV_BY - 1) / MV_BY)), block(MV_BX, MV_BY);
    ImageStage S(width, height, host);
    const int color = S.in(io.color, 3), albedo = S.in(io.albedo, 3), normal = S.in(io.normal, 3), depth = S.in(io.depth, 1);
    const int prev_point = S.in(io.prev_point, 3, motion);
    const int prev_cv = S.in(io.prev_cv, 4, hist), prev_len = S.in(io.prev_len, 1, hist), prev_normal = S.in(io.prev_normal, 3, hist), prev_depth = S.in(io.prev_depth, 1, hist);
    const int prev_mom = S.in(io.prev_mom, 4, hist);
    const int out_color = S.out(io.out_color, 3), out_variance = S.out(io.out_variance, 1), out_cv = S.out(io.out_cv, 4), out_len = S.out(io.out_len, 1);
    const int out_mom = S.out(io.out_mom, 4);
    if (int e = S.begin(stream)) return e;
    const trt_mv_fetch fetch{(const trt_dn4*)S[prev_cv], S[prev_len], S[prev_normal], S[prev_depth], (const trt_dn4*)S[prev_mom]};
    hipLaunchKernelGGL(motion ? k_reproject_moments<true> : k_reproject_moments<false>, grid, block, 0, stream, a, S[color], S[albedo], S[normal],
                       S[depth], S[prev_point], fetch, S[out_color], S[out_variance], (trt_dn4*)S[out_cv], S[out_len], (trt_dn4*)S[out_mom]);
    hipLaunchKernelGGL(lds ? k_moments_variance<true> : k_moments_variance<false>, grid, block, 0, stream, a, S[albedo], S[normal], S[depth],
                       (const float*)S[out_len], (const trt_dn4*)S[out_mom], S[out_cv], S[out_variance]);
    return S.finish(stats, 2);
}

}  // namespace

extern "C" {

int trt_reproject_moments(int device, const trt_moments_params* params, int width, int height, const float* color, const float* albedo,
                          const float* normal, const float* depth, const float* prev_point, const float* prev_cv, const float* prev_len,
                          const float* prev_normal, const float* prev_depth, const float* prev_mom, float* out_color, float* out_variance,
                          float* out_cv, float* out_len, float* out_mom, trt_stats* stats)
{
    return reprojectMoments(device, params, width, height,
                            MomentsIo{color, albedo, normal, depth, prev_point, prev_cv, prev_len, prev_normal, prev_depth, prev_mom, out_color,
                                      out_variance, out_cv, out_len, out_mom},
                            true, nullptr, stats, "trt_reproject_moments");
}

int trt_reproject_moments_device(int device, const trt_moments_params* params, int width, int height, const float* color, const float* albedo,
                                 const float* normal, const float* depth, const float* prev_point, const float* prev_cv, const float* prev_len,
                                 const float* prev_normal, const float* prev_depth, const float* prev_mom, float* out_color, float* out_variance,
                                 float* out_cv, float* out_len, float* out_mom, void* hip_stream, trt_stats* stats)
{
    return reprojectMoments(device, params, width, height,
                            MomentsIo{color, albedo, normal, depth, prev_point, prev_cv, prev_len, prev_normal, prev_depth, prev_mom, out_color,
                                      out_variance, out_cv, out_len, out_mom},
                            false, (hipStream_t)hip_stream, stats, "trt_reproject_moments_device");
}

}  // extern "C"

// ---- geometry update (include/trt.h trt_update_geometry; per-element code trt_refit.h) ------------------------------------------------
namespace {

inline dim3 refitGrid(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, (n + REFIT_BLOCK - 1) / REFIT_BLOCK)); }

// What one update keeps on the host from its first enqueue to its last exit: every host end of an asynchronous copy (sources and landing
// places) and the host entry's copy of the vertices on the device.  updateGeometry declares it before its Drain, so on every way out the
// stream is synchronised first and this goes away — the vertices are released — after it.
struct RefitHost {
    std::vector<LightDev> lights;        // sources: the caller's light tables in device layout
    std::vector<LightTriDev> ltris;
    std::vector<float> cum;
    std::vector<float> light_sel;        // the selection table of TRT_FLAG_ONE_LIGHT for the new areas (lightSelTable)
    LightTree light_tree;                // the light tree of TRT_FLAG_NEAR_LIGHTS over the new tables (buildLightTree)
    std::vector<int32_t> light_of_mat;   // source (the first update)
    std::vector<uint32_t> light_box;     // source (the empty boxes), then landing place: 6 ordered keys per light
    uint32_t cursor = 0;                 // landing places: the numbering's node count (the first update), nodes[0], the 8-wide refit's flag
    trt_bvh_node root{};
    uint32_t oct_failed = 0;
    void* v = nullptr;                   // the staged vertices and normals (host entry)
    void* vn = nullptr;
    RefitHost() = default;
    RefitHost(const RefitHost&) = delete;
    ~RefitHost()
    {
        if (v) (void)hipFree(v);
        if (vn) (void)hipFree(vn);
    }
};

// First update of a handle: the breadth-first node lists of both trees (one launch and one 4-byte read-back per level) and the
// material-to-light table.  Nothing a render reads is written.
template <class Bfs>
int refitNumber(Bfs launch, uint32_t n_nodes, uint32_t* d_order, uint32_t* d_cursor, hipStream_t stream, std::vector<uint32_t>& level, uint32_t& cur)
{
    static const uint32_t root[2] = {0u, 1u};  // order[0] = node 0; cursor = 1
    HIPC(hipMemcpyAsync(d_order, &root[0], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIPC(hipMemcpyAsync(d_cursor, &root[1], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    level.assign(1, 0u);
    uint32_t begin = 0, end = 1;
    while (begin < end) {
        level.push_back(end);
        launch(begin, end);
        HIPC(hipMemcpyAsync(&cur, d_cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPC(hipStreamSynchronize(stream));
        if (cur > n_nodes || level.size() > (size_t)MAX_BVH_DEPTH * 2 + 4) return fail(TRT_EHIP, "trt_update_geometry: the handle's tree does not number (internal error)");
        begin = end;
        end = cur;
    }
    return TRT_OK;
}

int refitPrepare(trt_handle* h, hipStream_t stream, RefitHost& H)
{
    trt_handle::Refit& R = h->refit;
    if (R.ready) return TRT_OK;
    const uint32_t nn = h->sc.n_nodes, nw = h->sc.n_wnodes;
    if (int e = R.order2.ensure((size_t)nn * sizeof(uint32_t))) return e;
    if (int e = R.order4.ensure((size_t)std::max(nw, 1u) * sizeof(uint32_t))) return e;
    if (int e = R.small.ensure((size_t)(16 + 6 * (size_t)std::max(h->sc.n_lights, 1u)) * sizeof(uint32_t))) return e;
    if (int e = R.light_of_mat.ensure((size_t)std::max(h->n_materials, 1u) * sizeof(int32_t))) return e;
    uint32_t* cursor = (uint32_t*)R.small.p;
    uint32_t* o2 = (uint32_t*)R.order2.p;
    uint32_t* o4 = (uint32_t*)R.order4.p;
    if (int e = refitNumber([&](uint32_t b, uint32_t en) { hipLaunchKernelGGL(k_refit_bfs2, refitGrid(en - b), dim3(REFIT_BLOCK), 0, stream, h->sc.nodes, o2, b, en, cursor, nn); },
                            nn, o2, cursor, stream, R.level2, H.cursor)) return e;
    if (nw)
        if (int e = refitNumber([&](uint32_t b, uint32_t en) { hipLaunchKernelGGL(k_refit_bfs4, refitGrid(en - b), dim3(REFIT_BLOCK), 0, stream, h->sc.wnodes, o4, b, en, cursor, nw); },
                                nw, o4, cursor, stream, R.level4, H.cursor)) return e;
    if (h->node_kind == 1 && h->sc.onodes) {
        const uint32_t no = h->sc.n_onodes;
        if (int e = R.order8.ensure((size_t)std::max(no, 1u) * sizeof(uint32_t))) return e;
        if (int e = R.exact8.ensure((size_t)std::max(no, 1u) * sizeof(RefitBox))) return e;
        uint32_t* o8 = (uint32_t*)R.order8.p;
        if (int e = refitNumber([&](uint32_t b, uint32_t en) { hipLaunchKernelGGL(k_refit_bfs8, refitGrid(en - b), dim3(REFIT_BLOCK), 0, stream, h->sc.onodes, o8, b, en, cursor, no); },
                                no, o8, cursor, stream, R.level8, H.cursor)) return e;
    }
    std::vector<int32_t>& lom = H.light_of_mat;
    lom.assign(std::max(h->n_materials, 1u), -1);
    for (size_t l = h->light_mats.size(); l-- > 0;)
        if (h->light_mats[l] < h->n_materials) lom[h->light_mats[l]] = (int32_t)l;  // the first light of a material stands for all of them
    HIPC(hipMemcpyAsync(R.light_of_mat.p, lom.data(), lom.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIPC(hipStreamSynchronize(stream));
    HIPC(hipGetLastError());
    R.ready = true;
    return TRT_OK;
}

inline bool refitsOct(const trt_handle* h) { return h->node_kind == 1 && !h->refit.level8.empty(); }  // after refitPrepare
inline bool refitsLightBoxes(const trt_handle* h) { return h->sc.n_lights && !h->light_boxes_fixed; }

// The checks that need no device
int checkUpdate(const trt_handle* h, const trt_geometry_update* u, uint32_t n_tris, const std::string& w)
{
    if (!h || !u) return fail(TRT_EINVAL, w + ": null handle / update");
    if (!u->tri_v && h->sc.n_tris) return fail(TRT_EINVAL, w + ": tri_v is null");
    if (n_tris != h->sc.n_tris) return fail(TRT_EINVAL, w + ": n_tris differs from the handle's (topology cannot change)");
    if ((u->lights == nullptr) != (u->light_tris == nullptr) && (u->lights || h->n_light_tris)) return fail(TRT_EINVAL, w + ": lights and light_tris come together");
    return TRT_OK;
}

// The caller's light tables, when given, checked and in device layout (H.lights, H.ltris, H.cum, H.light_sel, H.light_tree); nothing is enqueued
int updateLightTables(const trt_handle* h, const trt_geometry_update* u, const std::string& w, RefitHost& H)
{
    if (!u->lights) return TRT_OK;
    if (u->n_lights != h->sc.n_lights || u->n_light_tris != h->n_light_tris) return fail(TRT_EINVAL, w + ": light counts differ from the handle's");
    for (uint32_t l = 0; l < u->n_lights; ++l) {
        const trt_light& L = u->lights[l];
        if (L.mat < 0 || (uint32_t)L.mat >= h->n_materials) return fail(TRT_EINVAL, w + ": light material id out of range");
        if ((uint32_t)L.mat != h->light_mats[l]) return fail(TRT_EINVAL, w + ": a light's material differs from the handle's");
        if ((uint64_t)L.tri_first + L.tri_count > u->n_light_tris) return fail(TRT_EINVAL, w + ": light triangle range out of bounds");
    }
    std::vector<MaterialDev> mats(h->n_materials);  // radiance comes from the materials (makeLightDev); they live on the device only
    HIPC(hipMemcpy(mats.data(), h->sc.materials, mats.size() * sizeof(MaterialDev), hipMemcpyDeviceToHost));
    H.lights.resize(u->n_lights);
    for (uint32_t l = 0; l < u->n_lights; ++l) H.lights[l] = makeLightDevFrom(u->lights[l], mats[(size_t)u->lights[l].mat].radiance);
    H.light_sel.resize(u->n_lights);
    lightSelTable(H.lights.data(), u->n_lights, H.light_sel.data());
    H.ltris.resize(u->n_light_tris);
    H.cum.resize(u->n_light_tris);
    for (uint32_t k = 0; k < u->n_light_tris; ++k) { H.ltris[k] = makeLightTriDev(u->light_tris[k]); H.cum[k] = u->light_tris[k].cum_area; }
    buildLightTree(H.lights.data(), u->n_lights, H.ltris.data(), u->n_light_tris, H.light_tree);
    bool monotone = true;
    for (uint32_t l = 0; l < u->n_lights; ++l)
        for (uint32_t k = 0; k < u->lights[l].tri_count; ++k) {
            const float c = H.cum[u->lights[l].tri_first + k];
            if (!(c == c) || (k && c < H.cum[u->lights[l].tri_first + k - 1])) monotone = false;
        }
    // a handle that bisects the packed CDF keeps doing so (k_shade's LDS layout is fixed at trt_create): a CDF it cannot bisect is refused
    if (h->sc.light_cum && !monotone) return fail(TRT_EINVAL, w + ": a light's cumulative areas decrease or are NaN (this handle bisects them)");
    return TRT_OK;
}

// The host entry's vertices (and normals, when given) into device memory of the call's own; d_v and d_vn then point there
int stageVertices(const trt_geometry_update* u, uint32_t n, hipStream_t stream, RefitHost& H, const float*& d_v, const float*& d_vn)
{
    const size_t bytes = (size_t)n * 9 * sizeof(float);
    HIPC(hipMalloc(&H.v, bytes));
    HIPC(hipMemcpyAsync(H.v, u->tri_v, bytes, hipMemcpyHostToDevice, stream));
    d_v = (const float*)H.v;
    if (!u->tri_vn) return TRT_OK;
    HIPC(hipMalloc(&H.vn, bytes));
    HIPC(hipMemcpyAsync(H.vn, u->tri_vn, bytes, hipMemcpyHostToDevice, stream));
    d_vn = (const float*)H.vn;
    return TRT_OK;
}

// Nothing is written before the vertices have passed: one launch, one flag, read back on the spot
int checkVertices(const trt_handle* h, const float* d_v, hipStream_t stream, const std::string& w)
{
    uint32_t* flag = (uint32_t*)h->refit.small.p + 1;
    HIPC(hipMemsetAsync(flag, 0, sizeof(uint32_t), stream));
    const uint64_t nf = (uint64_t)h->sc.n_tris * 9;
    hipLaunchKernelGGL(k_refit_check, dim3((unsigned)std::min<uint64_t>(4096, std::max<uint64_t>(1, (nf + REFIT_BLOCK - 1) / REFIT_BLOCK))), dim3(REFIT_BLOCK), 0, stream, d_v, nf, flag);
    uint32_t bad = 0;
    HIPC(hipMemcpyAsync(&bad, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIPC(hipStreamSynchronize(stream));
    HIPC(hipGetLastError());
    if (bad) return fail(TRT_EINVAL, w + ": a vertex coordinate is NaN or infinite");
    return TRT_OK;
}

// Bottom-up over a tree that refitNumber numbered: launch(begin, end) once per level, the deepest first -> the launches
template <class Launch>
uint64_t refitLevels(const std::vector<uint32_t>& level, Launch launch)
{
    uint64_t launches = 0;
    for (size_t l = level.empty() ? 0 : level.size() - 1; l-- > 0; ++launches) launch(level[l], level[l + 1]);
    return launches;
}

// The refit itself: the triangle records, the caller's BVH2, the 4-wide nodes, the 8-wide nodes of a handle that walks them, the plane
// filter and the light boxes (trt_refit_kernels.h) -> `launches` grows by what was launched
int refitLaunches(trt_handle* h, const float* d_v, const float* d_vn, hipStream_t stream, RefitHost& H, uint64_t& launches)
{
    const trt_handle::Refit& R = h->refit;
    const uint32_t n = h->sc.n_tris, nn = h->sc.n_nodes, nw = h->sc.n_wnodes, nl = h->sc.n_lights;
    const dim3 block(REFIT_BLOCK);
    uint32_t* oct_fail = (uint32_t*)R.small.p + 2;
    uint32_t* lbox = (uint32_t*)R.small.p + 16;
    if (n) {
        hipLaunchKernelGGL(k_refit_tris, refitGrid(n), block, 0, stream, n, d_v, d_vn, (TriIsect*)h->sc.tri_isect, (TriShade*)h->sc.tri_shade);
        ++launches;
    }
    launches += refitLevels(R.level2, [&](uint32_t b, uint32_t e) {
        hipLaunchKernelGGL(k_refit_level2, refitGrid(e - b), block, 0, stream, (trt_bvh_node*)h->sc.nodes, nn, (const uint32_t*)R.order2.p, b, e, d_v, (f4*)h->sc.leaf_box);
    });
    launches += refitLevels(R.level4, [&](uint32_t b, uint32_t e) {
        hipLaunchKernelGGL(k_refit_level4, refitGrid(e - b), block, 0, stream, (WideNode*)h->sc.wnodes, nw, (const uint32_t*)R.order4.p, b, e, h->sc.leaf_box);
    });
    if (refitsOct(h)) {   // the 8-wide nodes: triangle records in node order, then the nodes level by level with their children's exact boxes in scratch
        HIPC(hipMemsetAsync(oct_fail, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_refit_tri_trav, refitGrid(h->n_tri_trav), block, 0, stream, h->n_tri_trav, h->sc.tri_isect, (TriIsect*)h->sc.tri_trav);
        ++launches;
        launches += refitLevels(R.level8, [&](uint32_t b, uint32_t e) {
            hipLaunchKernelGGL(k_refit_level8, refitGrid(e - b), block, 0, stream, (OctNode*)h->sc.onodes, h->sc.n_onodes, (const uint32_t*)R.order8.p, b, e,
                               h->sc.tri_trav, h->sc.leaf_box, (RefitBox*)R.exact8.p, oct_fail);
        });
    }
    if (h->sc.plane_bits) {
        const size_t words = (size_t)((1ull << (32u - h->sc.plane_shift)) / 32);
        HIPC(hipMemsetAsync((void*)h->sc.plane_bits, 0, words * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_refit_planes, refitGrid(nn), block, 0, stream, h->sc.nodes, nn, (uint32_t*)h->sc.plane_bits, h->sc.plane_shift);
        ++launches;
    }
    H.light_box.resize((size_t)6 * nl);
    if (refitsLightBoxes(h)) {
        for (uint32_t l = 0; l < nl; ++l)
            for (int a = 0; a < 3; ++a) { H.light_box[6 * l + a] = refitOrdered(3.0e38f); H.light_box[6 * l + 3 + a] = refitOrdered(-3.0e38f); }
        HIPC(hipMemcpyAsync(lbox, H.light_box.data(), H.light_box.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_refit_light_boxes, refitGrid(n), block, 0, stream, n, h->sc.tri_isect, h->sc.leaf_box, (const int32_t*)R.light_of_mat.p, h->n_materials, lbox);
        ++launches;
    }
    HIPC(hipGetLastError());
    return TRT_OK;
}

// Behind the kernels: what the commit needs comes back (H.root, H.oct_failed, H.light_box), the new light tables go up, k_shade's LDS image follows them
int exchangeTables(trt_handle* h, bool new_lights, hipStream_t stream, RefitHost& H)
{
    const trt_handle::Refit& R = h->refit;
    HIPC(hipMemcpyAsync(&H.root, h->sc.nodes, sizeof(H.root), hipMemcpyDeviceToHost, stream));
    if (refitsOct(h)) HIPC(hipMemcpyAsync(&H.oct_failed, (uint32_t*)R.small.p + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (refitsLightBoxes(h)) HIPC(hipMemcpyAsync(H.light_box.data(), (uint32_t*)R.small.p + 16, H.light_box.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (new_lights) {
        if (!H.lights.empty()) HIPC(hipMemcpyAsync((void*)h->sc.lights, H.lights.data(), H.lights.size() * sizeof(LightDev), hipMemcpyHostToDevice, stream));
        if (!H.ltris.empty()) HIPC(hipMemcpyAsync((void*)h->sc.light_tris, H.ltris.data(), H.ltris.size() * sizeof(LightTriDev), hipMemcpyHostToDevice, stream));
        if (h->sc.light_cum && !H.cum.empty()) HIPC(hipMemcpyAsync((void*)h->sc.light_cum, H.cum.data(), H.cum.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        if (h->sc.light_sel && !H.light_sel.empty()) HIPC(hipMemcpyAsync((void*)h->sc.light_sel, H.light_sel.data(), H.light_sel.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        if (h->sc.light_nodes && !H.light_tree.nodes.empty())  // (n_lights >= 2: the handle has room for n_lights - 1 nodes, and the update keeps n_lights)
            HIPC(hipMemcpyAsync((void*)h->sc.light_nodes, H.light_tree.nodes.data(), H.light_tree.nodes.size() * sizeof(LightNode), hipMemcpyHostToDevice, stream));
    }
    if (h->lds_image) return packLdsImage(h, stream);
    return TRT_OK;
}

// The handle's host state follows what the device now holds: only after the stream has been synchronised without an error
void commitUpdate(trt_handle* h, const trt_geometry_update* u, const RefitHost& H)
{
    const uint32_t nl = h->sc.n_lights;
    h->sc.leaf_alpha = sceneLeafAlpha(&H.root, 1);
    h->root_node = H.root;  // what cullBound() projects from now on (trt_cull.h)
    h->root_known = true;
    if (h->sc.cull_alpha != std::numeric_limits<float>::infinity()) h->sc.cull_alpha = h->sc.leaf_alpha;  // a tree that did not nest at trt_create stays without distance culling
    if (refitsLightBoxes(h))
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t m = h->light_mats[l];
            uint32_t from = l;  // lights of one material share the box of the first of them
            for (uint32_t k = 0; k < l; ++k)
                if (h->light_mats[k] == m) { from = k; break; }
            for (int a = 0; a < 3; ++a) { h->light_boxes[l].lo[a] = refitUnordered(H.light_box[6 * from + a]); h->light_boxes[l].hi[a] = refitUnordered(H.light_box[6 * from + 3 + a]); }
        }
    if (u->lights) h->sc.light0_area = nl ? u->lights[0].area : 0.0f;
    if (u->lights && h->sc.light_nodes) {  // the light tree of the new tables (exchangeTables has sent its nodes)
        h->sc.n_light_nodes = (uint32_t)H.light_tree.nodes.size();
        h->sc.light_root = H.light_tree.root;
    }
    // boxes that reach 2^40 (or an extent the bytes cannot hold): the tree no longer qualifies for the 8-wide nodes — the exact 4-wide ones from here on, for good
    if (refitsOct(h) && H.oct_failed) h->node_kind = 0;
}

// The stages of an update, in the order include/trt.h promises: every check before anything is written.  The bracket (events 0..3 of the
// handle, TRT_K_REFIT) opens before refitPrepare: render_ms of a handle's first update holds the numbering of its trees.
int updateGeometry(trt_handle* h, const trt_geometry_update* u, uint32_t n_tris, bool host, hipStream_t stream, trt_stats* stats, const char* what)
{
    const std::string w(what);
    if (int e = checkUpdate(h, u, n_tris, w)) return e;
    HIPC(hipSetDevice(h->device));
    RefitHost H;  // before the drain: it goes away after the stream has been synchronised
    if (int e = updateLightTables(h, u, w, H)) return e;
    EventBracket& B = h->refit.bracket;
    if (int e = B.create()) return e;
    Drain drain(stream, h);
    drain.arm();
    if (int e = B.record(0, stream)) return e;
    if (int e = refitPrepare(h, stream, H)) return e;
    const float* d_v = u->tri_v;
    const float* d_vn = u->tri_vn;
    if (host && h->sc.n_tris)
        if (int e = stageVertices(u, h->sc.n_tris, stream, H, d_v, d_vn)) return e;
    if (int e = B.record(1, stream)) return e;
    if (int e = checkVertices(h, d_v, stream, w)) return e;
    uint64_t launches = 1;  // k_refit_check
    if (int e = refitLaunches(h, d_v, d_vn, stream, H, launches)) return e;
    if (int e = B.record(2, stream)) return e;
    if (int e = exchangeTables(h, u->lights != nullptr, stream, H)) return e;
    if (int e = B.record(3, stream)) return e;
    HIPC(hipStreamSynchronize(stream));
    HIPC(hipGetLastError());
    drain.armed = false;  // everything this call enqueued has completed
    commitUpdate(h, u, H);
    return B.fill(stats, TRT_K_REFIT, launches);
}

}  // namespace

extern "C" {

int trt_update_geometry(trt_handle* h, const trt_geometry_update* u, uint32_t n_tris, trt_stats* stats)
{
    return updateGeometry(h, u, n_tris, true, nullptr, stats, "trt_update_geometry");
}

int trt_update_geometry_device(trt_handle* h, const trt_geometry_update* u, uint32_t n_tris, void* hip_stream, trt_stats* stats)
{
    return updateGeometry(h, u, n_tris, false, (hipStream_t)hip_stream, stats, "trt_update_geometry_device");
}

}  // extern "C"
