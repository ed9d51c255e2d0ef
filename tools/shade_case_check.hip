// shade_case_check.hip — the shading functions of trt_path.h and the primitives of trt_prims.h / trt_exact.h under them as gfx950 compiles them (the flags
// of the library), one thread per case, for tests/test_gpu_shade_cases.py.  Sections and their output words: tools/shade_cases.h, which also holds the one
// function per case that both this tool and tests/hostsim call (the light pickers lightPickAt / lightPick / lightWeight, lightNodeStep and lightPickNear among them); the kernels here only pick the case of their thread.  Reads one case file, writes one
// result file, one process, one pass.  Every index the file carries is checked on the host before any launch (shadecases::parse): a bad file is exit
// code 2, and no kernel reads memory the file did not supply.
// usage: shade_case_check <case file> <result file>
//        shade_case_check digest <result file>     the 64-bit digests of the exhaustive sweeps (shade_cases.h: all 2^24 uniforms, ranges of floats)
//        shade_case_check digest-pickers <result file>     those of the light pickers over all 2^24 uniforms (shade_cases.h: pickerDigestAt)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "shade_cases.h"

using namespace shadecases;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

__global__ __launch_bounds__(256) void k_prim(const PrimCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runPrim(cases[i], out + (size_t)W_PRIM * i);
}
__global__ __launch_bounds__(256) void k_cam(const CamCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runCam(cases[i], out + (size_t)W_CAM * i);
}
__global__ __launch_bounds__(256) void k_vert(SceneDev sc, const VertCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runVert<HeaderFns>(sc, cases[i], out + (size_t)W_VERT * i);
}
__global__ __launch_bounds__(256) void k_light(SceneDev sc, const float* cum, const LightCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runLight<HeaderFns>(sc, cum, cases[i], out + (size_t)W_LIGHT * i);
}
__global__ __launch_bounds__(256) void k_next(SceneDev sc, const NextCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runNext<HeaderFns>(sc, cases[i], out + (size_t)W_NEXT * i);
}
__global__ __launch_bounds__(256) void k_dir(const DirCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runDir<HeaderFns>(cases[i], out + (size_t)W_DIR * i);
}
__global__ __launch_bounds__(256) void k_bounce(SceneDev sc, const int32_t* rows, const BounceCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runBounce(sc, rows, cases[i], out + (size_t)W_BOUNCE * i);
}
__global__ __launch_bounds__(256) void k_pick(Pools pl, const PickCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runPick<HeaderFns>(pl, cases[i], out + (size_t)W_PICK * i);
}
__global__ __launch_bounds__(256) void k_step(const StepCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runStep<HeaderFns>(cases[i], out + (size_t)W_STEP * i);
}
__global__ __launch_bounds__(256) void k_near(Pools pl, const NearCase* cases, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) runNear(pl, cases[i], out + (size_t)W_NEAR * i);
}
__global__ __launch_bounds__(256) void k_digest(uint64_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < digestTotal()) out[i] = digestAt(i);
}
__global__ __launch_bounds__(256) void k_picker_digest(const DigestPools* pools, uint64_t* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pickerDigestTotal()) out[i] = pickerDigestAt(*pools, i);
}

template <class T>
static T* toDevice(const void* src, size_t count)
{
    T* d = nullptr;
    CK(hipMalloc(&d, count ? count * sizeof(T) : sizeof(T)));
    if (count) CK(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
static dim3 blocks(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

static int writeFile(const char* path, const void* data, size_t bytes)
{
    std::FILE* g = std::fopen(path, "wb");
    if (!g || std::fwrite(data, 1, bytes, g) != bytes || std::fclose(g) != 0) { std::fprintf(stderr, "cannot write %s\n", path); return 2; }
    return 0;
}

static int digestMode(const char* result, bool pickers)
{
    const size_t n = pickers ? pickerDigestTotal() : digestTotal();
    CK(hipSetDevice(0));
    uint64_t* d_out = nullptr;
    CK(hipMalloc(&d_out, n * 8));
    CK(hipMemset(d_out, 0, n * 8));
    if (pickers) {
        std::vector<DigestPools> pools(1);
        digestPoolsFill(pools[0]);
        const DigestPools* d_pools = toDevice<DigestPools>(pools.data(), 1);
        hipLaunchKernelGGL(k_picker_digest, blocks(n), dim3(256), 0, 0, d_pools, d_out);
    } else {
        hipLaunchKernelGGL(k_digest, blocks(n), dim3(256), 0, 0, d_out);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> out(n);
    CK(hipMemcpy(out.data(), d_out, n * 8, hipMemcpyDeviceToHost));
    if (int e = writeFile(result, out.data(), n * 8)) return e;
    std::printf("shade_case_check: %d streams, %u digests of %d inputs\n", (int)(pickers ? PICKER_STREAMS : DIGEST_STREAMS), (unsigned)n, (int)DIGEST_CHUNK);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file> | digest <result file> | digest-pickers <result file>\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "digest")) return digestMode(argv[2], false);
    if (!std::strcmp(argv[1], "digest-pickers")) return digestMode(argv[2], true);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf(size > 0 ? (size_t)size : 0);
    const bool read_ok = size > 0 && std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    if (!read_ok) { std::fprintf(stderr, "%s: cannot be read\n", argv[1]); return 2; }
    View v;
    if (const char* why = parse(buf.data(), buf.size(), v)) { std::fprintf(stderr, "%s: %s\n", argv[1], why); return 2; }
    const Header& h = v.h;

    CK(hipSetDevice(0));
    SceneDev sc{};
    sc.materials = toDevice<MaterialDev>(v.mat, h.n_mat);
    sc.textures = toDevice<TextureDev>(v.tex, h.n_tex);
    sc.tex_bytes = toDevice<uint8_t>(v.texbytes, h.n_texbytes);
    sc.lights = toDevice<LightDev>(v.lights, h.n_lights);
    sc.light_tris = toDevice<LightTriDev>(v.ltris, h.n_ltris);
    sc.tri_shade = toDevice<TriShade>(v.tshade, h.n_tris);
    sc.tri_isect = toDevice<TriIsect>(v.tisect, h.n_tris);
    sc.n_tris = h.n_tris;
    sc.n_lights = h.n_lights;
    std::vector<float> cum(h.n_ltris);
    for (uint32_t i = 0; i < h.n_ltris; ++i) std::memcpy(&cum[i], v.ltris + (size_t)i * sizeof(LightTriDev) + offsetof(LightTriDev, cum_area), 4);
    const float* d_cum = toDevice<float>(cum.data(), cum.size());
    int32_t rows[BOUNCE_ROWS];
    for (int r = 0; r < BOUNCE_ROWS; ++r) rows[r] = r;
    const int32_t* d_rows = toDevice<int32_t>(rows, BOUNCE_ROWS);
    const PrimCase* d_prim = toDevice<PrimCase>(v.prim, h.n_prim);
    const CamCase* d_cam = toDevice<CamCase>(v.cam, h.n_cam);
    const VertCase* d_vert = toDevice<VertCase>(v.vert, h.n_vert);
    const LightCase* d_light = toDevice<LightCase>(v.light, h.n_light);
    const NextCase* d_next = toDevice<NextCase>(v.next, h.n_next);
    const DirCase* d_dir = toDevice<DirCase>(v.dir, h.n_dir);
    const BounceCase* d_bounce = toDevice<BounceCase>(v.bounce, h.n_bounce);
    Pools pl;
    pl.lights = toDevice<LightDev>(v.plights, h.n_plights);
    pl.sel = toDevice<float>(v.psel, h.n_psel);
    pl.nodes = toDevice<LightNode>(v.pnodes, h.n_pnodes);  // (hipMalloc: aligned for the 16-byte loads of a node)
    pl.sets = toDevice<LightSet>(v.sets, h.n_sets);
    const PickCase* d_pick = toDevice<PickCase>(v.pick, h.n_pick);
    const StepCase* d_step = toDevice<StepCase>(v.step, h.n_step);
    const NearCase* d_near = toDevice<NearCase>(v.near, h.n_near);
    const size_t n_words = (size_t)v.n_words;
    uint32_t* d_out = nullptr;
    CK(hipMalloc(&d_out, (n_words ? n_words : 1) * 4));
    CK(hipMemset(d_out, 0, (n_words ? n_words : 1) * 4));
    uint32_t* o = d_out;
    if (h.n_prim) hipLaunchKernelGGL(k_prim, blocks(h.n_prim), dim3(256), 0, 0, d_prim, h.n_prim, o);
    o += (size_t)W_PRIM * h.n_prim;
    if (h.n_cam) hipLaunchKernelGGL(k_cam, blocks(h.n_cam), dim3(256), 0, 0, d_cam, h.n_cam, o);
    o += (size_t)W_CAM * h.n_cam;
    if (h.n_vert) hipLaunchKernelGGL(k_vert, blocks(h.n_vert), dim3(256), 0, 0, sc, d_vert, h.n_vert, o);
    o += (size_t)W_VERT * h.n_vert;
    if (h.n_light) hipLaunchKernelGGL(k_light, blocks(h.n_light), dim3(256), 0, 0, sc, d_cum, d_light, h.n_light, o);
    o += (size_t)W_LIGHT * h.n_light;
    if (h.n_next) hipLaunchKernelGGL(k_next, blocks(h.n_next), dim3(256), 0, 0, sc, d_next, h.n_next, o);
    o += (size_t)W_NEXT * h.n_next;
    if (h.n_dir) hipLaunchKernelGGL(k_dir, blocks(h.n_dir), dim3(256), 0, 0, d_dir, h.n_dir, o);
    o += (size_t)W_DIR * h.n_dir;
    if (h.n_bounce) hipLaunchKernelGGL(k_bounce, blocks(h.n_bounce), dim3(256), 0, 0, sc, d_rows, d_bounce, h.n_bounce, o);
    o += (size_t)W_BOUNCE * h.n_bounce;
    if (h.n_pick) hipLaunchKernelGGL(k_pick, blocks(h.n_pick), dim3(256), 0, 0, pl, d_pick, h.n_pick, o);
    o += (size_t)W_PICK * h.n_pick;
    if (h.n_step) hipLaunchKernelGGL(k_step, blocks(h.n_step), dim3(256), 0, 0, d_step, h.n_step, o);
    o += (size_t)W_STEP * h.n_step;
    if (h.n_near) hipLaunchKernelGGL(k_near, blocks(h.n_near), dim3(256), 0, 0, pl, d_near, h.n_near, o);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> out(n_words);
    if (n_words) CK(hipMemcpy(out.data(), d_out, n_words * 4, hipMemcpyDeviceToHost));
    if (int e = writeFile(argv[2], out.data(), out.size() * 4)) return e;
    std::printf("shade_case_check: %u prims, %u camera, %u vertex, %u light, %u next, %u direction, %u bounce, %u pick, %u step, %u near cases\n", h.n_prim, h.n_cam, h.n_vert,
                h.n_light, h.n_next, h.n_dir, h.n_bounce, h.n_pick, h.n_step, h.n_near);
    return 0;
}
