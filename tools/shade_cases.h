// shade_cases.h — the case records of tools/shade_case_check.hip and the one function per record that turns a case into its output words, by calling
// trt_path.h / trt_prims.h / trt_exact.h.  Compiled twice from this one source: by hipcc for gfx950 (the tool, one thread per case) and by g++ into
// tests/hostsim (the same words from the CPU build), so the two sides can differ only in what their compilers made of the headers' arithmetic.
// The file layout (tests/shade_cases.py writes it): a 64-B header, the tables (materials, textures, lights, light triangles, shading and
// intersection records of the triangles), the seven case sections of the shading functions, the pools of the light pickers (lights, selection-table floats,
// light-tree nodes, the light sets that name ranges of them), the three case sections of the pickers, the texture bytes.  Every record is a multiple of 16 B.
// Every section function is a template on the set of functions under test (HeaderFns: the headers' own), so that tests/hostsim/shade_mutants.cpp can run
// the same sections on deliberately altered copies without touching the headers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "trt_path.h"

namespace shadecases {
using namespace trtd;

// Two layouts are read.  SHADE_CASES_MAGIC: the one described here, a 96-B header.  SHADE_CASES_MAGIC_1: the layout from before the light pickers — the first
// 64 B of the header, no pools, no picker sections — which parse() reads as a file whose picker counts are all zero.
#define SHADE_CASES_MAGIC 0x53434332u
#define SHADE_CASES_MAGIC_1 0x53434331u
struct Header {
    uint32_t magic, n_prim, n_cam, n_vert, n_light, n_next, n_dir, n_bounce;
    uint32_t n_mat, n_tex, n_texbytes, n_lights, n_ltris, n_tris, pad0, pad1;
    uint32_t n_pick, n_step, n_near, n_plights, n_psel, n_pnodes, n_sets, pad2;  // n_psel: floats, a multiple of 4
};
// op 0: sincos2pi(a)  1: logf(a)  2: expf_neg(a)  3: pow01(a, b)  4: rng_make_key(a, b, c), uniform(key, a & 0xFFFF), u32(key, b)
// 5: sqrt(a), sqrt_rsqrt2(a), rsqrt2(a)   6: div_by((double)a, (double)(uint32)b, 1.0 / b) and the reciprocal, as binary64 halves
struct PrimCase { uint32_t op, a, b, c; };
struct CamCase { trt_camera cam; int32_t W, H, i, j; float u1, u2; uint32_t mode, pad; };  // mode 0: fixed pixels, 1: grid reciprocals, 2: plain divisions
struct VertCase { float o[3], d[3], t, u, v; uint32_t pad[3]; TriShade ts; };
struct LightCase { float P[3], pn[3], wi[3], Kd[3]; uint32_t mat, li, k0, k1, ctr, flags; float light0_area; uint32_t pad; };  // flags: 1 fixed, 2 light_cum present
struct NextCase { float pn[3], I[3]; uint32_t mat, k0, k1, ctr, pad[2]; };
struct DirCase { uint32_t op; float a[3], b[3], x, y; int32_t type; uint32_t pad[2]; };  // op 0: sampleDir(a, type, Ns = x, u_phi = y, u_theta = b[0])  1: refract(a, b, x)  2: reflect(a, b)
struct BounceCase { f4 ra, rb, bt, hit; uint32_t flags; int32_t max_depth; uint32_t seed, s0; };  // flags: 1 ray_offset, 2 specular_ks
// The scene of a picker case: lights [light_first, + n_lights) of the light pool, the selection table of n_lights floats at sel_first of the float pool (SET_NO_TABLE:
// none, lightPickAt scans), nodes [node_first, + n_nodes) of the node pool, `root` in the children's encoding.  Leaf references index the set's lights, inner
// references the set's nodes; an inner reference is greater than the index of the node that holds it (buildLightTree numbers in pre-order), so every descent ends.
#define SHADE_SET_NO_TABLE 0xFFFFFFFFu
struct LightSet { uint32_t light_first, n_lights, sel_first, node_first, n_nodes, root, pad[2]; };
// op 0: lightPickAt(u) on the table  1: lightPickAt(u) by scan (light_sel null)  2: lightPick(stream) on the table  3: lightPick(stream) by scan  4: lightWeight(light li of the set)
struct PickCase { uint32_t op, set, u, k0, k1, ctr, li, pad; };
struct StepCase { LightNode node; float P[3], u, inv_p; uint32_t pad[3]; };  // lightNodeStep(node, P, u, inv_p)
struct NearCase { uint32_t set; float P[3]; uint32_t k0, k1, ctr, pad; };     // lightPickNear(set, P, stream)
static_assert(sizeof(LightSet) == 32 && sizeof(PickCase) == 32 && sizeof(StepCase) == 96 && sizeof(NearCase) == 32 && sizeof(LightDev) == 32 && sizeof(LightNode) == 64,
              "the case file's picker records");
static_assert(sizeof(Header) == 96 && sizeof(PrimCase) == 16 && sizeof(CamCase) == 80 && sizeof(VertCase) == 112 && sizeof(LightCase) == 80 &&
              sizeof(NextCase) == 48 && sizeof(DirCase) == 48 && sizeof(BounceCase) == 80 && sizeof(TextureDev) == 16 && sizeof(TriShade) == 64 && sizeof(TriIsect) == 48,
              "the case file's records");
enum { W_PRIM = 4, W_CAM = 6, W_VERT = 9, W_LIGHT = 9, W_NEXT = 8, W_DIR = 3, W_BOUNCE = 17, W_PICK = 4, W_STEP = 2, W_NEAR = 4 };
// the tile every bounce case belongs to: 64 x 4 pixels, rows 0..3 (pathKey reads the row table: BOUNCE_ROWS entries)
enum { BOUNCE_W = 64, BOUNCE_ROWS = 4 };

// Where the sections lie in a file, after every index it carries has been checked against the tables it carries.
struct View {
    Header h;
    const uint8_t *mat, *tex, *lights, *ltris, *tshade, *tisect, *prim, *cam, *vert, *light, *next, *dir, *bounce, *plights, *psel, *pnodes, *sets, *pick, *step, *near, *texbytes;
    uint64_t n_words;
};

// -> null when the file is sound, else what is wrong with it.  No section function may be called on a file this refuses.
inline const char* parse(const uint8_t* buf, uint64_t size, View& v)
{
    const uint64_t head1 = 64;  // the header of SHADE_CASES_MAGIC_1: what lies before n_pick
    if (size < head1) return "short file";
    memset(&v.h, 0, sizeof(Header));
    memcpy(&v.h, buf, head1);
    const Header& h = v.h;
    if (h.magic != SHADE_CASES_MAGIC && h.magic != SHADE_CASES_MAGIC_1) return "not a case file";
    const uint64_t head = h.magic == SHADE_CASES_MAGIC ? sizeof(Header) : head1;
    if (size < head) return "short file";
    memcpy(&v.h, buf, head);
    const uint32_t counts[] = {h.n_prim, h.n_cam, h.n_vert, h.n_light, h.n_next, h.n_dir, h.n_bounce, h.n_mat, h.n_tex, h.n_lights, h.n_ltris, h.n_tris,
                               h.n_pick, h.n_step, h.n_near, h.n_plights, h.n_psel, h.n_pnodes, h.n_sets};
    for (uint32_t c : counts)
        if (c >> 24) return "a count of 2^24 or more";
    if (h.n_psel & 3u) return "selection-table floats: not a multiple of 4";
    if (h.n_texbytes >> 28 || (h.n_texbytes & 15u)) return "texture bytes: 2^28 or more, or not a multiple of 16";
    const uint8_t* p = buf + head;
    v.mat = p; p += (uint64_t)h.n_mat * sizeof(MaterialDev);
    v.tex = p; p += (uint64_t)h.n_tex * sizeof(TextureDev);
    v.lights = p; p += (uint64_t)h.n_lights * sizeof(LightDev);
    v.ltris = p; p += (uint64_t)h.n_ltris * sizeof(LightTriDev);
    v.tshade = p; p += (uint64_t)h.n_tris * sizeof(TriShade);
    v.tisect = p; p += (uint64_t)h.n_tris * sizeof(TriIsect);
    v.prim = p; p += (uint64_t)h.n_prim * sizeof(PrimCase);
    v.cam = p; p += (uint64_t)h.n_cam * sizeof(CamCase);
    v.vert = p; p += (uint64_t)h.n_vert * sizeof(VertCase);
    v.light = p; p += (uint64_t)h.n_light * sizeof(LightCase);
    v.next = p; p += (uint64_t)h.n_next * sizeof(NextCase);
    v.dir = p; p += (uint64_t)h.n_dir * sizeof(DirCase);
    v.bounce = p; p += (uint64_t)h.n_bounce * sizeof(BounceCase);
    v.plights = p; p += (uint64_t)h.n_plights * sizeof(LightDev);
    v.psel = p; p += (uint64_t)h.n_psel * sizeof(float);
    v.pnodes = p; p += (uint64_t)h.n_pnodes * sizeof(LightNode);
    v.sets = p; p += (uint64_t)h.n_sets * sizeof(LightSet);
    v.pick = p; p += (uint64_t)h.n_pick * sizeof(PickCase);
    v.step = p; p += (uint64_t)h.n_step * sizeof(StepCase);
    v.near = p; p += (uint64_t)h.n_near * sizeof(NearCase);
    v.texbytes = p; p += h.n_texbytes;
    if ((uint64_t)(p - buf) != size) return "the size does not match the header";
    v.n_words = (uint64_t)W_PRIM * h.n_prim + (uint64_t)W_CAM * h.n_cam + (uint64_t)W_VERT * h.n_vert + (uint64_t)W_LIGHT * h.n_light + (uint64_t)W_NEXT * h.n_next +
                (uint64_t)W_DIR * h.n_dir + (uint64_t)W_BOUNCE * h.n_bounce + (uint64_t)W_PICK * h.n_pick + (uint64_t)W_STEP * h.n_step + (uint64_t)W_NEAR * h.n_near;
    // the tables: texture of a material, byte range of a texture, triangle range of a light, material of a triangle
    for (uint32_t i = 0; i < h.n_mat; ++i) {
        MaterialDev m;
        memcpy(&m, v.mat + (uint64_t)i * sizeof m, sizeof m);
        if (m.tex >= 0 && (uint32_t)m.tex >= h.n_tex) return "a material's texture is out of range";
    }
    for (uint32_t i = 0; i < h.n_tex; ++i) {
        TextureDev t;
        memcpy(&t, v.tex + (uint64_t)i * sizeof t, sizeof t);
        if (t.width < 1 || t.height < 1 || t.width > 65536 || t.height > 65536) return "a texture's size is out of range";
        if (t.offset > h.n_texbytes || (uint64_t)t.width * (uint64_t)t.height * 3u > h.n_texbytes - t.offset) return "a texture's bytes are out of range";
    }
    for (uint32_t i = 0; i < h.n_lights; ++i) {
        LightDev l;
        memcpy(&l, v.lights + (uint64_t)i * sizeof l, sizeof l);
        if ((uint64_t)l.tri_first + l.tri_count > h.n_ltris) return "a light's triangles are out of range";
    }
    for (uint32_t i = 0; i < h.n_tris; ++i) {
        TriShade t;
        memcpy(&t, v.tshade + (uint64_t)i * sizeof t, sizeof t);
        if (t.mat < 0 || (uint32_t)t.mat >= h.n_mat) return "a triangle's material is out of range";
    }
    // the cases
    for (uint32_t i = 0; i < h.n_prim; ++i) {
        PrimCase c;
        memcpy(&c, v.prim + (uint64_t)i * sizeof c, sizeof c);
        if (c.op > 6u) return "a primitive case's operation is unknown";
    }
    for (uint32_t i = 0; i < h.n_cam; ++i) {
        CamCase c;
        memcpy(&c, v.cam + (uint64_t)i * sizeof c, sizeof c);
        if (c.mode > 2u) return "a camera case's mode is unknown";
        if (c.mode == 1u && (c.W < 2 || c.H < 2 || c.W > 65536 || c.H > 65536)) return "a camera case asks for the grid reciprocals outside 2..65536";
    }
    for (uint32_t i = 0; i < h.n_vert; ++i) {
        VertCase c;
        memcpy(&c, v.vert + (uint64_t)i * sizeof c, sizeof c);
        if (c.ts.mat < 0 || (uint32_t)c.ts.mat >= h.n_mat) return "a vertex case's material is out of range";
    }
    for (uint32_t i = 0; i < h.n_light; ++i) {
        LightCase c;
        memcpy(&c, v.light + (uint64_t)i * sizeof c, sizeof c);
        if (c.mat >= h.n_mat) return "a light case's material is out of range";
        if (c.li >= h.n_lights) return "a light case's light is out of range";
    }
    for (uint32_t i = 0; i < h.n_next; ++i) {
        NextCase c;
        memcpy(&c, v.next + (uint64_t)i * sizeof c, sizeof c);
        if (c.mat >= h.n_mat) return "a next-ray case's material is out of range";
    }
    for (uint32_t i = 0; i < h.n_dir; ++i) {
        DirCase c;
        memcpy(&c, v.dir + (uint64_t)i * sizeof c, sizeof c);
        if (c.op > 2u) return "a direction case's operation is unknown";
    }
    if (h.n_bounce && !h.n_mat) return "bounce cases without a material";
    for (uint32_t i = 0; i < h.n_bounce; ++i) {
        BounceCase c;
        memcpy(&c, v.bounce + (uint64_t)i * sizeof c, sizeof c);
        const int32_t tri = (int32_t)f2u(c.hit.y);
        if (tri >= 0 && (uint32_t)tri >= h.n_tris) return "a bounce case's triangle is out of range";
    }
    // the light sets: ranges inside their pools, every reference of the root and of every node inside the set, inner references ascending
    for (uint32_t i = 0; i < h.n_sets; ++i) {
        LightSet s;
        memcpy(&s, v.sets + (uint64_t)i * sizeof s, sizeof s);
        if ((uint64_t)s.light_first + s.n_lights > h.n_plights) return "a light set's lights leave the pool";
        if (s.sel_first != SHADE_SET_NO_TABLE && (uint64_t)s.sel_first + s.n_lights > h.n_psel) return "a light set's selection table leaves the pool";
        if ((uint64_t)s.node_first + s.n_nodes > h.n_pnodes) return "a light set's nodes leave the pool";
        if (s.root != TRT_LIGHT_NONE) {
            if (s.root & TRT_LIGHT_LEAF) { if ((s.root & ~TRT_LIGHT_LEAF) >= s.n_lights) return "a light set's root names a light outside the set"; }
            else if (s.root >= s.n_nodes) return "a light set's root is outside the set's nodes";
        }
        for (uint32_t k = 0; k < s.n_nodes; ++k) {
            uint32_t child[2];
            memcpy(child, v.pnodes + ((uint64_t)s.node_first + k) * sizeof(LightNode) + offsetof(LightNode, child0), 8);
            for (uint32_t c : child) {
                if (c & TRT_LIGHT_LEAF) { if ((c & ~TRT_LIGHT_LEAF) >= s.n_lights) return "a leaf reference names a light outside its set"; }
                else if (c <= k) return "an inner reference is not greater than the index of the node that holds it";
                else if (c >= s.n_nodes) return "an inner reference is outside the set's nodes";
            }
        }
    }
    for (uint32_t i = 0; i < h.n_pick; ++i) {
        PickCase c;
        memcpy(&c, v.pick + (uint64_t)i * sizeof c, sizeof c);
        if (c.op > 4u) return "a pick case's operation is unknown";
        if (c.set >= h.n_sets) return "a pick case's light set is out of range";
        LightSet s;
        memcpy(&s, v.sets + (uint64_t)c.set * sizeof s, sizeof s);
        if ((c.op == 0u || c.op == 2u) && s.sel_first == SHADE_SET_NO_TABLE) return "a pick case asks for the table of a set without one";
        if (c.op < 2u && s.n_lights < 2u) return "a pick case calls lightPickAt on fewer than two lights";
        if (c.op == 4u && c.li >= s.n_lights) return "a pick case's light is outside its set";
    }
    for (uint32_t i = 0; i < h.n_near; ++i) {
        NearCase c;
        memcpy(&c, v.near + (uint64_t)i * sizeof c, sizeof c);
        if (c.set >= h.n_sets) return "a near case's light set is out of range";
    }
    return nullptr;
}

// ---- the functions under test ------------------------------------------------------------------------------------------------------------------------
struct HeaderFns {
    static TRT_HD Vertex makeVertex(const SceneDev& sc, const Hit& h, f3 o, f3 d, const TriShade& ts, const MaterialDev& m) { return trtd::makeVertex(sc, h, o, d, ts, m); }
    static TRT_HD bool lightSample(const SceneDev& sc, const Vertex& vx, const MaterialDev& m, uint32_t li, Stream& rng, f3& wo, f3& contrib, bool fixed, float& t_max)
    {
        return trtd::lightSample(sc, vx, m, li, rng, wo, contrib, fixed, t_max);
    }
    static TRT_HD int nextRayFinish(const MaterialDev& m, f3 pn, f3 I, const NextPlan& pl, f3& out) { return trtd::nextRayFinish(m, pn, I, pl, out); }
    static TRT_HD f3 refract(f3 I, f3 N, float eta) { return trtd::refract(I, N, eta); }
    static TRT_HD bool lightPickAt(const SceneDev& sc, float u, uint32_t& li, float& inv_p) { return trtd::lightPickAt(sc, u, li, inv_p); }
    static TRT_HD uint32_t lightNodeStep(const LightNode& n, f3 P, float u, float& inv_p) { return trtd::lightNodeStep(n, P, u, inv_p); }
};

// one NaN: the payload of a NaN is not part of any claim
TRT_HD inline uint32_t canon(float f) { return f != f ? 0x7FC00000u : f2u(f); }
TRT_HD inline void put3(uint32_t* w, f3 a) { w[0] = canon(a.x); w[1] = canon(a.y); w[2] = canon(a.z); }
TRT_HD inline void put64(uint32_t* w, double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    if (x != x) b = 0x7FF8000000000000ull;
    w[0] = (uint32_t)b; w[1] = (uint32_t)(b >> 32);
}

TRT_HD inline void runPrim(const PrimCase& p, uint32_t* w)
{
    const float x = u2f(p.a), y = u2f(p.b);
    w[0] = w[1] = w[2] = w[3] = 0u;
    switch (p.op) {
    case 0: { float c, s; trt_sincos2pi(x, &c, &s); w[0] = canon(c); w[1] = canon(s); } break;
    case 1: w[0] = canon(trt_logf(x)); break;
    case 2: w[0] = canon(trt_expf_neg(x)); break;
    case 3: w[0] = canon(trt_pow01(x, y)); break;
    case 4: {
        const trt_rng_key k = trt_rng_make_key(p.a, p.b, p.c);
        w[0] = k.k0; w[1] = k.k1; w[2] = f2u(trt_rng_uniform(k, p.a & 0xFFFFu)); w[3] = trt_rng_u32(k, p.b);
    } break;
    case 5: {
        float s, r;
        trt_sqrt_rsqrt2(x, &s, &r);
        w[0] = canon(trt_sqrt(x)); w[1] = canon(s); w[2] = canon(r); w[3] = canon(trt_rsqrt2(x));
    } break;
    default: {
        const double a = (double)x, b = (double)p.b, rb = 1.0 / b;
        put64(w, trt_div_by(a, b, rb));
        put64(w + 2, rb);
    } break;
    }
}

TRT_HD inline void runCam(const CamCase& c, uint32_t* w)
{
    // what the host forms once per render (TileDesc::grid_rcp): IEEE binary64 divisions on either side
    const double grid[4] = {1.0 / (c.W - 1.0), 1.0 / (c.H - 1.0), 1.0 / double(c.W), 1.0 / double(c.H)};
    f3 o = mk3(0, 0, 0), d = mk3(0, 0, 0);
    cameraRay(c.cam, c.W, c.H, c.i, c.j, c.u1, c.u2, o, d, c.mode == 0u, c.mode == 1u ? grid : nullptr);
    put3(w, o);
    put3(w + 3, d);
}

template <class F>
TRT_HD inline void runVert(const SceneDev& sc, const VertCase& c, uint32_t* w)
{
    Hit h;
    h.t = c.t; h.tri = 0; h.u = c.u; h.v = c.v; h.flags = 0u;
    const Vertex vx = F::makeVertex(sc, h, ld3(c.o), ld3(c.d), c.ts, sc.materials[c.ts.mat]);
    put3(w, vx.P);
    put3(w + 3, vx.pn);
    put3(w + 6, vx.Kd);
}

// `cum`: the packed CDF of the file's light triangles (SceneDev::light_cum), used by the cases that ask for the bisection
template <class F>
TRT_HD inline void runLight(const SceneDev& sc0, const float* cum, const LightCase& c, uint32_t* w)
{
    SceneDev sc = sc0;
    sc.light_cum = (c.flags & 2u) ? cum : nullptr;
    sc.light0_area = c.light0_area;
    Vertex vx;
    vx.P = ld3(c.P); vx.pn = ld3(c.pn); vx.wi = ld3(c.wi); vx.Kd = ld3(c.Kd); vx.mat = (int32_t)c.mat;
    Stream rng;
    rng.key.k0 = c.k0; rng.key.k1 = c.k1; rng.ctr = c.ctr;
    f3 wo = mk3(0, 0, 0), contrib = mk3(0, 0, 0);
    float t_max = 0.0f;
    const bool emit = F::lightSample(sc, vx, sc.materials[c.mat], c.li, rng, wo, contrib, (c.flags & 1u) != 0u, t_max);
    w[0] = emit ? 1u : 0u;
    put3(w + 1, wo);
    put3(w + 4, contrib);
    w[7] = canon(t_max);
    w[8] = rng.ctr;
}

template <class F>
TRT_HD inline void runNext(const SceneDev& sc, const NextCase& c, uint32_t* w)
{
    Stream rng;
    rng.key.k0 = c.k0; rng.key.k1 = c.k1; rng.ctr = c.ctr;
    const MaterialDev& m = sc.materials[c.mat];
    const NextPlan pl = nextRayDecide(m, ld3(c.pn), ld3(c.I), rng);
    f3 out = mk3(0, 0, 0);
    const int type = F::nextRayFinish(m, ld3(c.pn), ld3(c.I), pl, out);
    w[0] = (uint32_t)pl.kind; w[1] = canon(pl.u_phi); w[2] = canon(pl.u_theta); w[3] = (uint32_t)type;
    put3(w + 4, out);
    w[7] = rng.ctr;
}

template <class F>
TRT_HD inline void runDir(const DirCase& c, uint32_t* w)
{
    f3 r;
    if (c.op == 0u) r = sampleDir(ld3(c.a), c.type, c.x, c.y, c.b[0]);
    else if (c.op == 1u) r = F::refract(ld3(c.a), ld3(c.b), c.x);
    else r = reflect(ld3(c.a), ld3(c.b));
    put3(w, r);
}

// `rows`: BOUNCE_ROWS image rows 0.. (TileDesc::rows)
TRT_HD inline void runBounce(const SceneDev& sc, const int32_t* rows, const BounceCase& c, uint32_t* w)
{
    TileDesc td;
    td.rows = rows;
    td.tile_w = BOUNCE_W; td.x0 = 0; td.width = BOUNCE_W; td.height = BOUNCE_ROWS;
    td.fixed_nee = 0u; td.fixed_pixels = 0u;
    td.ray_offset = c.flags & 1u; td.specular_ks = c.flags & 2u;
    td.npix = BOUNCE_W * BOUNCE_ROWS; td.seed = c.seed; td.spp = 1u;
    td.npix_magic = magicOf(td.npix); td.tile_w_magic = magicOf((uint32_t)td.tile_w);
    td.grid_ok = 0u;
    td.grid_rcp[0] = td.grid_rcp[1] = td.grid_rcp[2] = td.grid_rcp[3] = 0.0;
    ShadeCtx ctx;
    shadeBegin(sc, td, c.s0, c.ra, c.rb, c.bt, c.hit, ctx);
    f4 ra = mk4(0, 0, 0, 0), rb = mk4(0, 0, 0, 0), bt = mk4(0, 0, 0, 0);
    const bool emit = shadeNext(ctx, c.max_depth, ra, rb, bt);
    w[0] = emit ? 1u : 0u;
    w[1] = canon(ra.x); w[2] = canon(ra.y); w[3] = canon(ra.z); w[4] = canon(ra.w);
    w[5] = canon(rb.x); w[6] = canon(rb.y); w[7] = f2u(rb.z); w[8] = f2u(rb.w);  // path id and meta word: bits, not numbers
    w[9] = canon(bt.x); w[10] = canon(bt.y); w[11] = canon(bt.z); w[12] = canon(bt.w);
    w[13] = (ctx.had_hit ? 1u : 0u) | (ctx.shade_ok ? 2u : 0u) | (ctx.add_L ? 4u : 0u);
    put3(w + 14, ctx.addL);
}

// ---- the light pickers ------------------------------------------------------------------------------------------------------------------------
struct Pools {
    const LightDev* lights;
    const float* sel;
    const LightNode* nodes;  // 16-byte aligned
    const LightSet* sets;
};
// the scene a picker sees: nothing but the set's lights, its table where `table`, its tree
TRT_HD inline SceneDev sceneOfSet(const Pools& pl, uint32_t set, bool table)
{
    const LightSet s = pl.sets[set];
    SceneDev sc{};
    sc.lights = pl.lights + s.light_first;
    sc.n_lights = s.n_lights;
    sc.light_sel = table ? pl.sel + s.sel_first : nullptr;
    sc.light_nodes = pl.nodes + s.node_first;
    sc.n_light_nodes = s.n_nodes;
    sc.light_root = s.root;
    return sc;
}
template <class F>
TRT_HD inline void runPick(const Pools& pl, const PickCase& c, uint32_t* w)
{
    const SceneDev sc = sceneOfSet(pl, c.set, c.op == 0u || c.op == 2u);
    Stream rng;
    rng.key.k0 = c.k0; rng.key.k1 = c.k1; rng.ctr = c.ctr;
    uint32_t li = 0u;
    float ip = 0.0f;
    bool ok = false;
    if (c.op == 4u) { li = c.li; ip = lightWeight(sc.lights[c.li]); }
    else if (c.op < 2u) ok = F::lightPickAt(sc, u2f(c.u), li, ip);
    else ok = lightPick(sc, rng, li, ip);
    w[0] = ok ? 1u : 0u; w[1] = li; w[2] = canon(ip); w[3] = rng.ctr;
}
template <class F>
TRT_HD inline void runStep(const StepCase& c, uint32_t* w)
{
    float ip = c.inv_p;
    w[0] = F::lightNodeStep(c.node, ld3(c.P), c.u, ip);
    w[1] = canon(ip);
}
TRT_HD inline void runNear(const Pools& pl, const NearCase& c, uint32_t* w)
{
    const SceneDev sc = sceneOfSet(pl, c.set, false);
    Stream rng;
    rng.key.k0 = c.k0; rng.key.k1 = c.k1; rng.ctr = c.ctr;
    uint32_t li = 0u;
    float ip = 0.0f;
    const bool ok = lightPickNear(sc, ld3(c.P), rng, li, ip);
    w[0] = ok ? 1u : 0u; w[1] = li; w[2] = canon(ip); w[3] = rng.ctr;
}

// ---- digests of exhaustive sweeps ------------------------------------------------------------------------------------------------------------------------
// One 64-bit digest per DIGEST_CHUNK consecutive inputs: the wrapping sum of trt_mix32(word + index) over the output words of the chunk; trt_mix32 is a
// bijection, so one changed word changes the sum.  Streams 0 .. DIGEST_UNIFORM_FNS - 1 run over all 2^24 uniforms u = m 2^-24 the path's stream can produce:
//   0: sincos2pi(u) (two words)   1: sqrt(u)   2: sqrt(1 - u)   3 + k: pow01(u, 1 / (Ns_k + 1)), the exponent as sampleDir forms it   3 + DIGEST_NS + k: pow01(u, Ns_k)
// the others over every float of a range of bit patterns:
//   logf on [2^-126, 2^-125); expf_neg on [-88, -86); trt_sqrt / trt_sqrt_rsqrt2 (three words) on the exponent fields within 2 of trt_exact_domain's two
//   ends: 30 .. 34 and 252 .. 255 (the last holds the infinity and the NaNs);
// and three over 2^20 inputs formed from the index i: logf on the stratified (i + 1/2) 2^-20 of (0, 1), expf_neg on -87 times that, the square roots on the
// bit patterns trt_mix32(i).
// A second table (pickerDigestAt; the tool's mode digest-pickers) holds the light pickers over all 2^24 uniforms again, two words per input (the index with the returned bool in bit 31, or the child reference; the bits of inv_p):
//   PICKER_PICK0 + k: lightPickAt on table k of digestPoolsFill (2, 7, 64 and 256 lights; zero-weight plateaus in 1 and 3, weights across 2^50 in 2 and 3), on the table;
//   PICKER_SCAN0 + k: the same by scan, on the two small tables;   PICKER_STEP0 + j: lightNodeStep(node j, P j, u, 1): ordinary importances, a subnormal importance beside a normal one (r = u s and the divisor of s / imp each subnormal on a part of the uniforms),
//   the fall-back by power (d2 overflows), two equal children (r == imp0 at u = 1/2).
// Their tables are formed on the host from trt_mix32 and constants (digestPoolsFill: exact operations only), so the digest modes still read no file.
enum { DIGEST_NS = 8, DIGEST_UNIFORM_FNS = 3 + 2 * DIGEST_NS, DIGEST_STREAMS = DIGEST_UNIFORM_FNS + 7, DIGEST_CHUNK = 4096, DIGEST_UNIFORM_CHUNKS = (1 << 24) / DIGEST_CHUNK };
enum { DIGEST_PICK_TABLES = 4, DIGEST_PICK_SCANS = 2, DIGEST_STEP_NODES = 4, DIGEST_PICK_MAX = 256 };
enum { PICKER_PICK0 = 0, PICKER_SCAN0 = PICKER_PICK0 + DIGEST_PICK_TABLES, PICKER_STEP0 = PICKER_SCAN0 + DIGEST_PICK_SCANS, PICKER_STREAMS = PICKER_STEP0 + DIGEST_STEP_NODES };
struct DigestPools {
    LightNode nodes[DIGEST_STEP_NODES];
    float P[DIGEST_STEP_NODES][4];
    LightDev lights[DIGEST_PICK_TABLES][DIGEST_PICK_MAX];
    float sel[DIGEST_PICK_TABLES][DIGEST_PICK_MAX];
};
TRT_HD inline uint32_t digestPickLights(uint32_t k) { return k == 0u ? 2u : k == 1u ? 7u : k == 2u ? 64u : 256u; }
// host only: light l of table k has radiance (0.5, 2, 1) and area (1 + (m >> 9)) 2^e, m = trt_mix32(0x5E700000 + 256 k + l), e = -20 in tables 0 and 1,
// (m & 31) - 28 in 2 and 3; area 0 for lights 2, 3 and 6 of table 1 and every fifth light of table 3 (its last among them)
inline void digestPoolsFill(DigestPools& p)
{
    memset(&p, 0, sizeof p);
    for (uint32_t k = 0; k < (uint32_t)DIGEST_PICK_TABLES; ++k) {
        const uint32_t n = digestPickLights(k);
        for (uint32_t l = 0; l < n; ++l) {
            const uint32_t m = trt_mix32(0x5E700000u + 256u * k + l);
            const bool zero = (k == 1u && (l == 2u || l == 3u || l == 6u)) || (k == 3u && l % 5u == 0u);
            LightDev& L = p.lights[k][l];
            L.radiance[0] = 0.5f; L.radiance[1] = 2.0f; L.radiance[2] = 1.0f;
            L.area = zero ? 0.0f : __builtin_ldexpf((float)((m >> 9) + 1u), k < 2u ? -20 : (int)(m & 31u) - 28);
        }
        lightSelTable(p.lights[k], n, p.sel[k]);
    }
    for (uint32_t j = 0; j < (uint32_t)DIGEST_STEP_NODES; ++j) {
        LightNode& n = p.nodes[j];
        n.lo0[0] = -1.0f; n.lo0[1] = 2.0f; n.lo0[2] = -1.0f; n.hi0[0] = 1.0f; n.hi0[1] = 2.5f; n.hi0[2] = 1.0f;
        n.lo1[0] = 4.0f; n.lo1[1] = 2.0f; n.lo1[2] = 0.0f; n.hi1[0] = 5.0f; n.hi1[1] = 3.0f; n.hi1[2] = 1.0f;
        n.w0 = 3.0f; n.w1 = 1.5f;
        n.child0 = TRT_LIGHT_LEAF | 0u; n.child1 = TRT_LIGHT_LEAF | 1u;
        p.P[j][0] = 0.25f; p.P[j][1] = 0.0f; p.P[j][2] = 0.125f;
    }
    p.nodes[1].w0 = 4.0f; p.nodes[1].w1 = 0.25f; p.P[1][0] = 1.0e19f;  // imp0 about 4e-38, imp1 about 2.5e-39: r is subnormal below u = 0.28, the divisor above u = 0.94
    p.P[2][0] = 1.0e20f;
    memcpy(p.nodes[3].lo1, p.nodes[3].lo0, 12); memcpy(p.nodes[3].hi1, p.nodes[3].hi0, 12);
    p.nodes[3].w1 = 3.0f;
}
TRT_HD inline uint32_t digestBase(uint32_t st)
{
    return st < (uint32_t)DIGEST_UNIFORM_FNS ? 0u : st == DIGEST_UNIFORM_FNS ? 0x00800000u : st == DIGEST_UNIFORM_FNS + 1u ? 0xC2AC0000u : st == DIGEST_UNIFORM_FNS + 2u ? 30u << 23 : st == DIGEST_UNIFORM_FNS + 3u ? 252u << 23 : 0u;
}
TRT_HD inline uint32_t digestChunks(uint32_t st)
{
    return st < (uint32_t)DIGEST_UNIFORM_FNS ? (uint32_t)DIGEST_UNIFORM_CHUNKS : st == DIGEST_UNIFORM_FNS ? 2048u : st == DIGEST_UNIFORM_FNS + 1u ? 64u : st == DIGEST_UNIFORM_FNS + 2u ? 5u * 2048u : st == DIGEST_UNIFORM_FNS + 3u ? 4u * 2048u : 256u;
}
TRT_HD inline uint32_t digestTotal()
{
    uint32_t n = 0u;
    for (uint32_t st = 0; st < (uint32_t)DIGEST_STREAMS; ++st) n += digestChunks(st);
    return n;
}
TRT_HD inline float digestNs(uint32_t k)
{
    switch (k) {
    case 0: return 1.5f;
    case 1: return 2.0f;
    case 2: return 10.0f;
    case 3: return 250.0f;
    case 4: return 500.0f;
    case 5: return 1000.0f;
    case 6: return 1.0e4f;
    default: return 1.0e6f;
    }
}
TRT_HD inline uint64_t digestChunk(uint32_t st, uint32_t chunk)
{
    uint64_t sum = 0u;
    const uint32_t U = DIGEST_UNIFORM_FNS;
    const float e = st < 3u ? 0.0f : (st < 3u + DIGEST_NS ? 1.0f / (digestNs(st - 3u) + 1.0f) : digestNs(st - 3u - DIGEST_NS));
    for (uint32_t k = 0; k < DIGEST_CHUNK; ++k) {
        const uint32_t m = digestBase(st) + chunk * DIGEST_CHUNK + k;  // the uniform's numerator, or the input's bits
        if (st >= U) {
            const float strat = ((float)m + 0.5f) * 9.5367431640625e-7f;  // (i + 1/2) 2^-20, exact
            const float x = st < U + 4u ? u2f(m) : st == U + 4u ? strat : st == U + 5u ? -87.0f * strat : u2f(trt_mix32(m));
            if (st == U || st == U + 4u) sum += trt_mix32(canon(trt_logf(x)) + m);
            else if (st == U + 1u || st == U + 5u) sum += trt_mix32(canon(trt_expf_neg(x)) + m);
            else {
                float s, r;
                trt_sqrt_rsqrt2(x, &s, &r);
                sum += trt_mix32(canon(trt_sqrt(x)) + 3u * m);
                sum += trt_mix32(canon(s) + (3u * m + 1u));
                sum += trt_mix32(canon(r) + (3u * m + 2u));
            }
            continue;
        }
        const float u = (float)m * 5.9604644775390625e-8f;
        if (st == 0u) {
            float c, s;
            trt_sincos2pi(u, &c, &s);
            sum += trt_mix32(canon(c) + 2u * m);
            sum += trt_mix32(canon(s) + (2u * m + 1u));
        } else {
            const float r = st == 1u ? trt_sqrt(u) : (st == 2u ? trt_sqrt(1.0f - u) : trt_pow01(u, e));
            sum += trt_mix32(canon(r) + m);
        }
    }
    return sum;
}
// digest number i of the whole set (streams in order) -> its value
TRT_HD inline uint64_t digestAt(uint32_t i)
{
    uint32_t st = 0u;
    while (i >= digestChunks(st)) i -= digestChunks(st++);
    return digestChunk(st, i);
}

// ---- the pickers' table: PICKER_STREAMS streams of DIGEST_UNIFORM_CHUNKS chunks each
TRT_HD inline uint32_t pickerDigestTotal() { return (uint32_t)PICKER_STREAMS * (uint32_t)DIGEST_UNIFORM_CHUNKS; }
TRT_HD inline uint64_t pickerDigestChunk(const DigestPools& pools, uint32_t st, uint32_t chunk)
{
    uint64_t sum = 0u;
    const bool step = st >= (uint32_t)PICKER_STEP0, scan = st >= (uint32_t)PICKER_SCAN0;
    const uint32_t t = step ? st - PICKER_STEP0 : scan ? st - PICKER_SCAN0 : st - PICKER_PICK0;
    SceneDev sc{};
    if (!step) {
        sc.lights = pools.lights[t];
        sc.n_lights = digestPickLights(t);
        sc.light_sel = scan ? nullptr : pools.sel[t];
    }
    for (uint32_t k = 0; k < DIGEST_CHUNK; ++k) {
        const uint32_t m = chunk * DIGEST_CHUNK + k;
        const float u = (float)m * 5.9604644775390625e-8f;
        uint32_t ref = 0u;
        float ip = 1.0f;
        if (step) ref = lightNodeStep(pools.nodes[t], ld3(pools.P[t]), u, ip);
        else if (lightPickAt(sc, u, ref, ip)) ref |= 0x80000000u;
        sum += trt_mix32(ref + 2u * m);
        sum += trt_mix32(canon(ip) + (2u * m + 1u));
    }
    return sum;
}
TRT_HD inline uint64_t pickerDigestAt(const DigestPools& pools, uint32_t i) { return pickerDigestChunk(pools, i / (uint32_t)DIGEST_UNIFORM_CHUNKS, i % (uint32_t)DIGEST_UNIFORM_CHUNKS); }

}  // namespace shadecases
