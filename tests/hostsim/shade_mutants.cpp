// shade_mutants.cpp — TEST INFRASTRUCTURE.  Deliberately WRONG local copies of three functions of trt_path.h, run through the sections of
// tools/shade_cases.h, for the sensitivity check of tests/test_shade_cases_cpu.py: a corpus that cannot tell these from the headers' own functions
// does not test the decision each of them bends.  Nothing else loads this library; the product headers are untouched.
//   mutant 1: the CDF pick of lightSample compares `rnd <= cum` instead of `rnd < cum` (both the bisection and the scan)
//   mutant 2: refract returns the zero vector for `k <= 0` instead of `k < 0`
//   mutant 3: makeVertex takes the texel column (int)(icol * width) in fp32 instead of binary64
#include "shade_cases_host.h"

using namespace trtd;

namespace {
// lightSample (trt_path.h) with `rnd <= cum` in the pick: for floats, rnd <= cum is rnd < the next float above cum, so the header's own function runs on a copy
// of the light whose cumulative areas EQUAL to this case's rnd are raised by one ulp — the pick alone changes, everything after it is the header's code.
bool lightSampleLe(const SceneDev& sc, const Vertex& vx, const MaterialDev& m, uint32_t li, Stream& rng, f3& wo, f3& contrib, bool fixed, float& t_max)
{
    const LightDev L = sc.lights[li];
    Stream peek = rng;
    const float rnd = peek.next() * (fixed ? L.area : sc.light0_area);
    std::vector<LightTriDev> tris(sc.light_tris + L.tri_first, sc.light_tris + L.tri_first + L.tri_count);
    std::vector<float> cum(L.tri_count);
    for (uint32_t k = 0; k < L.tri_count; ++k) {
        if (rnd == tris[k].cum_area) tris[k].cum_area = nextafterf(tris[k].cum_area, INFINITY);  // rnd <= cum  <=>  rnd < the next float above cum
        cum[k] = tris[k].cum_area;
    }
    SceneDev s2 = sc;
    LightDev L2 = L;
    L2.tri_first = 0;
    s2.lights = &L2;
    s2.light_tris = tris.data();
    if (sc.light_cum) s2.light_cum = cum.data();
    return lightSample(s2, vx, m, 0u, rng, wo, contrib, fixed, t_max);
}
f3 refractLe(f3 I, f3 N, float eta)
{
    const float dn = dot(N, I);
    const float k = 1.0f - eta * eta * (1.0f - dn * dn);
    if (k <= 0.0f) return mk3(0.f, 0.f, 0.f);
    return I * eta - N * (eta * dn + trt_sqrt(k));
}
int nextRayFinishLe(const MaterialDev& m, f3 pn, f3 I, const NextPlan& pl, f3& out)
{
    if (pl.kind != 1) return nextRayFinish(m, pn, I, pl, out);
    const float cos_in = dot(I, pn);
    f3 n;
    float eta;
    if (cos_in > 0.0f) { n = -pn; eta = m.Ni; }
    else { n = pn; eta = m.Ni_inv; }
    const f3 T = refractLe(I, n, eta);
    if (T.x != 0.0f || T.y != 0.0f || T.z != 0.0f) { out = T; return TRT_RAY_TRANSMISSION; }
    out = reflect(I, n);
    return TRT_RAY_SPECULAR;
}
Vertex makeVertexF32(const SceneDev& sc, const Hit& h, f3 o, f3 d, const TriShade& ts, const MaterialDev& m)
{
    Vertex vx = makeVertex(sc, h, o, d, ts, m);
    if (m.tex >= 0) {
        const TextureDev tx = sc.textures[m.tex];
        const float b0 = (1.0f - h.u) - h.v, b1 = h.u, b2 = h.v;
        const float colf = (ts.vt[0] * b0 + ts.vt[2] * b1) + ts.vt[4] * b2;
        const float rowf = (ts.vt[1] * b0 + ts.vt[3] * b1) + ts.vt[5] * b2;
        const double row = rowf;
        const double irow = row - floor(row);
        const float icol = colf - floorf(colf);
        int r = (int)(irow * tx.height), c = (int)(icol * (float)tx.width);
        if (r > tx.height - 1) r = tx.height - 1;
        if (c > tx.width - 1) c = tx.width - 1;
        if (r < 0) r = 0;
        if (c < 0) c = 0;
        const uint8_t* px = sc.tex_bytes + tx.offset + ((size_t)r * tx.width + c) * 3;
        vx.Kd = mk3((float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f);
    }
    return vx;
}

struct PickLe : shadecases::HeaderFns {
    static bool lightSample(const SceneDev& sc, const Vertex& vx, const MaterialDev& m, uint32_t li, Stream& rng, f3& wo, f3& contrib, bool fixed, float& t_max)
    {
        return lightSampleLe(sc, vx, m, li, rng, wo, contrib, fixed, t_max);
    }
};
struct RefractLe : shadecases::HeaderFns {
    static int nextRayFinish(const MaterialDev& m, f3 pn, f3 I, const NextPlan& pl, f3& out) { return nextRayFinishLe(m, pn, I, pl, out); }
    static f3 refract(f3 I, f3 N, float eta) { return refractLe(I, N, eta); }
};
struct TexelF32 : shadecases::HeaderFns {
    static Vertex makeVertex(const SceneDev& sc, const Hit& h, f3 o, f3 d, const TriShade& ts, const MaterialDev& m) { return makeVertexF32(sc, h, o, d, ts, m); }
};
}  // namespace

// mutant 0 is the headers' own functions (the control: the words of hostsim_shade_case_file)
extern "C" int shade_mutant_case_file(int mutant, const uint8_t* buf, uint64_t size, uint32_t* out, uint64_t n_words)
{
    switch (mutant) {
    case 0: return shadecases::runFileHost<shadecases::HeaderFns>(buf, size, out, n_words);
    case 1: return shadecases::runFileHost<PickLe>(buf, size, out, n_words);
    case 2: return shadecases::runFileHost<RefractLe>(buf, size, out, n_words);
    case 3: return shadecases::runFileHost<TexelF32>(buf, size, out, n_words);
    default: return 2;
    }
}
