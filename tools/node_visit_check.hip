// node_visit_check.hip — the per-node decisions of the traversal as gfx950 compiles them, one thread per case, for tests/test_gpu_node_claims.py:
//   (i)   octVisit (trt_oct.h) on (node, ray, cull)                      -> the two group words (node hits | imask, triangle bits)
//   (ii)  innerStep (trt_path.h: the packed two-wide slab arithmetic of the device build) on a 4-wide node, empty private stack
//                                                                        -> cur, the returned flag, entries pushed, the pushed references in order
//   (iii) boxTest / boxTestGlm on (box, ray)                             -> verdict bits, the bits of the two entries (any NaN as 0x7FC00000)
// The kernels are thin wrappers: every decision is made by the headers' own functions.  Reads one case file, writes one result file (layouts:
// tests/node_cases.py), one process, one pass; tests/hostsim returns the same words from the CPU build of the same functions.
// usage: node_visit_check <case file> <result file>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "trt_path.h"
#include "trt_oct.h"
#include "trt_wide.h"

using namespace trtd;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

struct Case { uint32_t node; float o[3], d[3], cull; };
struct BoxCase { float lo[3], hi[3], o[3], d[3]; };
static_assert(sizeof(Case) == 32 && sizeof(BoxCase) == 48, "the case file's records");

struct PrivStack {
    uint32_t s[4];
    __device__ void push(int sp, uint32_t v) { if (sp >= 0 && sp < 4) s[sp] = v; }
};

__device__ inline uint32_t canonBits(float f) { return f != f ? 0x7FC00000u : f2u(f); }
__device__ inline f3 invOf(f3 d) { return mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); }

__global__ __launch_bounds__(256) void k_oct_visit(const OctNode* nodes, const Case* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Case c = cases[i];
    const f3 o = ld3(c.o), d = ld3(c.d);
    const OctRay R = makeOctRay(o, d, invOf(d));
    OctGroup ng, tg;
    octVisit(nodes, c.node, R, c.cull, ng, tg);
    out[2 * (size_t)i] = ng.y;
    out[2 * (size_t)i + 1] = tg.y;
}

__global__ __launch_bounds__(256) void k_inner_step(const WideNode* wnodes, const Case* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Case c = cases[i];
    SceneDev sc{};
    sc.wnodes = wnodes;
    PrivStack stk;
    stk.s[0] = stk.s[1] = stk.s[2] = stk.s[3] = 0u;
    uint32_t cur = c.node;
    int sp = 0;
    const bool go = innerStep(sc, cur, sp, stk, ld3(c.o), invOf(ld3(c.d)), c.cull);
    uint32_t* w = out + 6 * (size_t)i;
    w[0] = cur; w[1] = go ? 1u : 0u; w[2] = (uint32_t)sp;
    w[3] = stk.s[0]; w[4] = stk.s[1]; w[5] = stk.s[2];
}

__global__ __launch_bounds__(256) void k_box(const BoxCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BoxCase c = cases[i];
    const f3 o = ld3(c.o), inv = invOf(ld3(c.d));
    float e0, e1;
    const bool p0 = boxTest(c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2], o, inv, e0);
    const bool p1 = boxTestGlm(c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2], o, inv, e1);
    uint32_t* w = out + 3 * (size_t)i;
    w[0] = (p0 ? 1u : 0u) | (p1 ? 2u : 0u);
    w[1] = canonBits(e0);
    w[2] = canonBits(e1);
}

template <class T>
static T* toDevice(const uint8_t* src, size_t count)
{
    T* d = nullptr;
    CK(hipMalloc(&d, count ? count * sizeof(T) : sizeof(T)));
    if (count) CK(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf(size > 0 ? (size_t)size : 0);
    const bool read_ok = size >= 32 && std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    if (!read_ok) { std::fprintf(stderr, "%s: short file\n", argv[1]); return 2; }
    const uint32_t* h = reinterpret_cast<const uint32_t*>(buf.data());
    const uint64_t n_on = h[1], n_oc = h[2], n_wn = h[3], n_ic = h[4], n_bc = h[5];
    const uint64_t want = 32 + n_on * sizeof(OctNode) + n_oc * sizeof(Case) + n_wn * sizeof(WideNode) + n_ic * sizeof(Case) + n_bc * sizeof(BoxCase);
    if (h[0] != 0x4E564331u || want != buf.size() || (n_oc | n_ic | n_bc) >> 28) { std::fprintf(stderr, "%s: not a case file\n", argv[1]); return 2; }
    const uint8_t* p_on = buf.data() + 32;
    const uint8_t* p_oc = p_on + n_on * sizeof(OctNode);
    const uint8_t* p_wn = p_oc + n_oc * sizeof(Case);
    const uint8_t* p_ic = p_wn + n_wn * sizeof(WideNode);
    const uint8_t* p_bc = p_ic + n_ic * sizeof(Case);
    // no kernel reads a node the file does not hold
    for (uint64_t i = 0; i < n_oc; ++i)
        if (reinterpret_cast<const Case*>(p_oc)[i].node >= n_on) { std::fprintf(stderr, "oct case %llu: node out of range\n", (unsigned long long)i); return 2; }
    for (uint64_t i = 0; i < n_ic; ++i)
        if (reinterpret_cast<const Case*>(p_ic)[i].node >= n_wn) { std::fprintf(stderr, "innerStep case %llu: node out of range\n", (unsigned long long)i); return 2; }

    CK(hipSetDevice(0));
    OctNode* d_on = toDevice<OctNode>(p_on, n_on);
    Case* d_oc = toDevice<Case>(p_oc, n_oc);
    WideNode* d_wn = toDevice<WideNode>(p_wn, n_wn);
    Case* d_ic = toDevice<Case>(p_ic, n_ic);
    BoxCase* d_bc = toDevice<BoxCase>(p_bc, n_bc);
    const size_t n_words = 2 * n_oc + 6 * n_ic + 3 * n_bc;
    uint32_t* d_out = nullptr;
    CK(hipMalloc(&d_out, (n_words ? n_words : 1) * 4));
    CK(hipMemset(d_out, 0, (n_words ? n_words : 1) * 4));
    if (n_oc) hipLaunchKernelGGL(k_oct_visit, dim3((uint32_t)((n_oc + 255) / 256)), dim3(256), 0, 0, d_on, d_oc, (uint32_t)n_oc, d_out);
    if (n_ic) hipLaunchKernelGGL(k_inner_step, dim3((uint32_t)((n_ic + 255) / 256)), dim3(256), 0, 0, d_wn, d_ic, (uint32_t)n_ic, d_out + 2 * n_oc);
    if (n_bc) hipLaunchKernelGGL(k_box, dim3((uint32_t)((n_bc + 255) / 256)), dim3(256), 0, 0, d_bc, (uint32_t)n_bc, d_out + 2 * n_oc + 6 * n_ic);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> out(n_words);
    if (n_words) CK(hipMemcpy(out.data(), d_out, n_words * 4, hipMemcpyDeviceToHost));
    std::FILE* g = std::fopen(argv[2], "wb");
    if (!g || std::fwrite(out.data(), 4, out.size(), g) != out.size() || std::fclose(g) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::printf("node_visit_check: %llu octVisit, %llu innerStep, %llu box cases\n", (unsigned long long)n_oc, (unsigned long long)n_ic, (unsigned long long)n_bc);
    return 0;
}
