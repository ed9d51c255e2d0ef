// shade_cases.h — the case records of tools/shade_case_check.hip and the one function per record that turns a case into its output words, by calling
// trt_path.h / trt_prims.h / trt_exact.h.  Compiled twice from this one source: by hipcc for gfx950 (the tool, one thread per case) and by g++ into
// tests/hostsim (the same words from the CPU build), so the two sides can differ only in what their compilers made of the headers' arithmetic.
// The file layout (tests/shade_cases.py writes it): a 64-B header, the tables (materials, textures, lights, light triangles, shading and
// intersection records of the triangles), the seven case sections, the texture bytes.  Every record is a multiple of 16 B.
// Every section function is a template on the set of functions under test (HeaderFns: the headers' own), so that tests/hostsim/shade_mutants.cpp can run
// the same sections on deliberately altered copies without touching the headers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "trt_path.h"

namespace shadecases {
using namespace trtd;

#define SHADE_CASES_MAGIC 0x53434331u
struct Header {
    uint32_t magic, n_prim, n_cam, n_vert, n_light, n_next, n_dir, n_bounce;
    uint32_t n_mat, n_tex, n_texbytes, n_lights, n_ltris, n_tris, pad0, pad1;
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
static_assert(sizeof(Header) == 64 && sizeof(PrimCase) == 16 && sizeof(CamCase) == 80 && sizeof(VertCase) == 112 && sizeof(LightCase) == 80 &&
              sizeof(NextCase) == 48 && sizeof(DirCase) == 48 && sizeof(BounceCase) == 80 && sizeof(TextureDev) == 16 && sizeof(TriShade) == 64 && sizeof(TriIsect) == 48,
              "the case file's records");
enum { W_PRIM = 4, W_CAM = 6, W_VERT = 9, W_LIGHT = 9, W_NEXT = 8, W_DIR = 3, W_BOUNCE = 17 };
// the tile every bounce case belongs to: 64 x 4 pixels, rows 0..3 (pathKey reads the row table: BOUNCE_ROWS entries)
enum { BOUNCE_W = 64, BOUNCE_ROWS = 4 };

// Where the sections lie in a file, after every index it carries has been checked against the tables it carries.
struct View {
    Header h;
    const uint8_t *mat, *tex, *lights, *ltris, *tshade, *tisect, *prim, *cam, *vert, *light, *next, *dir, *bounce, *texbytes;
    uint64_t n_words;
};

// -> null when the file is sound, else what is wrong with it.  No section function may be called on a file this refuses.
inline const char* parse(const uint8_t* buf, uint64_t size, View& v)
{
    if (size < sizeof(Header)) return "short file";
    memcpy(&v.h, buf, sizeof(Header));
    const Header& h = v.h;
    if (h.magic != SHADE_CASES_MAGIC) return "not a case file";
    const uint32_t counts[] = {h.n_prim, h.n_cam, h.n_vert, h.n_light, h.n_next, h.n_dir, h.n_bounce, h.n_mat, h.n_tex, h.n_lights, h.n_ltris, h.n_tris};
    for (uint32_t c : counts)
        if (c >> 24) return "a count of 2^24 or more";
    if (h.n_texbytes >> 28 || (h.n_texbytes & 15u)) return "texture bytes: 2^28 or more, or not a multiple of 16";
    const uint8_t* p = buf + sizeof(Header);
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
    v.texbytes = p; p += h.n_texbytes;
    if ((uint64_t)(p - buf) != size) return "the size does not match the header";
    v.n_words = (uint64_t)W_PRIM * h.n_prim + (uint64_t)W_CAM * h.n_cam + (uint64_t)W_VERT * h.n_vert + (uint64_t)W_LIGHT * h.n_light + (uint64_t)W_NEXT * h.n_next +
                (uint64_t)W_DIR * h.n_dir + (uint64_t)W_BOUNCE * h.n_bounce;
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

// ---- digests of exhaustive sweeps ------------------------------------------------------------------------------------------------------------------------
// One 64-bit digest per DIGEST_CHUNK consecutive inputs: the wrapping sum of trt_mix32(word + index) over the output words of the chunk; trt_mix32 is a
// bijection, so one changed word changes the sum.  Streams 0 .. DIGEST_UNIFORM_FNS - 1 run over all 2^24 uniforms u = m 2^-24 the path's stream can produce:
//   0: sincos2pi(u) (two words)   1: sqrt(u)   2: sqrt(1 - u)   3 + k: pow01(u, 1 / (Ns_k + 1)), the exponent as sampleDir forms it   3 + DIGEST_NS + k: pow01(u, Ns_k)
// the others over every float of a range of bit patterns:
//   logf on [2^-126, 2^-125); expf_neg on [-88, -86); trt_sqrt / trt_sqrt_rsqrt2 (three words) on the exponent fields within 2 of trt_exact_domain's two
//   ends: 30 .. 34 and 252 .. 255 (the last holds the infinity and the NaNs);
// and three over 2^20 inputs formed from the index i: logf on the stratified (i + 1/2) 2^-20 of (0, 1), expf_neg on -87 times that, the square roots on the
// bit patterns trt_mix32(i).
enum { DIGEST_NS = 8, DIGEST_UNIFORM_FNS = 3 + 2 * DIGEST_NS, DIGEST_STREAMS = DIGEST_UNIFORM_FNS + 7, DIGEST_CHUNK = 4096, DIGEST_UNIFORM_CHUNKS = (1 << 24) / DIGEST_CHUNK };
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

}  // namespace shadecases
