// shade_mutants.cpp — TEST INFRASTRUCTURE.  Deliberately WRONG local copies of functions of trt_path.h, run through the sections of
// tools/shade_cases.h, for the sensitivity check of tests/test_shade_cases_cpu.py: a corpus that cannot tell these from the headers' own functions
// does not test the decision each of them bends.  Nothing else loads this library; the product headers are untouched.
//   mutant 1: the CDF pick of lightSample compares `rnd <= cum` instead of `rnd < cum` (both the bisection and the scan)
//   mutant 2: refract returns the zero vector for `k <= 0` instead of `k < 0`
//   mutant 3: makeVertex takes the texel column (int)(icol * width) in fp32 instead of binary64
//   mutant 4: the bisection of lightPickAt compares `r <= light_sel[mid]` instead of `r < light_sel[mid]`
//   mutant 5: lightNodeStep picks the first child for `r <= imp0` instead of `r < imp0`
//   mutant 6: lightNodeStep without the flip away from a child whose importance is not > 0
//   mutant 7: lightChildImportance divides by d2 alone, without the fmaxf with r2
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

// lightPickAt (trt_path.h) with the one comparison of its bisection bent; the scan form is the header's
bool lightPickAtLe(const SceneDev& sc, float u, uint32_t& li, float& inv_p)
{
    if (!sc.light_sel) return lightPickAt(sc, u, li, inv_p);
    const uint32_t n = sc.n_lights;
    li = 0u;
    inv_p = 1.0f;
    const float total = sc.light_sel[n - 1u];
    if (!(total > 0.0f && total < __builtin_inff())) return false;
    const float r = u * total;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r <= sc.light_sel[mid]) hi = mid; else lo = mid + 1;
    }
    uint32_t pick = lo;
    if (pick >= n) {
        pick = 0u;
        for (uint32_t l = n; l-- > 0u;)
            if (lightWeight(sc.lights[l]) > 0.0f) { pick = l; break; }
    }
    li = pick;
    inv_p = total / lightWeight(sc.lights[pick]);
    return true;
}
float childImportanceD2(const float* lo, const float* hi, float w, f3 P)
{
    const f3 c = mk3(0.5f * lo[0] + 0.5f * hi[0], 0.5f * lo[1] + 0.5f * hi[1], 0.5f * lo[2] + 0.5f * hi[2]);
    const f3 q = mk3(P.x - c.x, P.y - c.y, P.z - c.z);
    return w / ((q.x * q.x + q.y * q.y) + q.z * q.z);
}
// lightNodeStep (trt_path.h) with one decision bent: LE `r <= imp0`, FLIP the flip kept, R2 the fmaxf with r2 kept
template <bool LE, bool FLIP, bool R2>
uint32_t nodeStepBent(const LightNode& n, f3 P, float u, float& inv_p)
{
    float imp0 = R2 ? lightChildImportance(n.lo0, n.hi0, n.w0, P) : childImportanceD2(n.lo0, n.hi0, n.w0, P);
    float imp1 = R2 ? lightChildImportance(n.lo1, n.hi1, n.w1, P) : childImportanceD2(n.lo1, n.hi1, n.w1, P);
    float s = imp0 + imp1;
    if (!(imp0 >= 0.0f && imp1 >= 0.0f && s > 0.0f && s < __builtin_inff())) {
        imp0 = n.w0; imp1 = n.w1;
        s = imp0 + imp1;
    }
    const float r = u * s;
    bool first = LE ? r <= imp0 : r < imp0;
    if (FLIP && !((first ? imp0 : imp1) > 0.0f)) first = !first;
    inv_p = inv_p * (s / (first ? imp0 : imp1));
    return first ? n.child0 : n.child1;
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
struct BisectLe : shadecases::HeaderFns {
    static bool lightPickAt(const SceneDev& sc, float u, uint32_t& li, float& inv_p) { return lightPickAtLe(sc, u, li, inv_p); }
};
struct StepLe : shadecases::HeaderFns {
    static uint32_t lightNodeStep(const LightNode& n, f3 P, float u, float& inv_p) { return nodeStepBent<true, true, true>(n, P, u, inv_p); }
};
struct StepNoFlip : shadecases::HeaderFns {
    static uint32_t lightNodeStep(const LightNode& n, f3 P, float u, float& inv_p) { return nodeStepBent<false, false, true>(n, P, u, inv_p); }
};
struct StepNoR2 : shadecases::HeaderFns {
    static uint32_t lightNodeStep(const LightNode& n, f3 P, float u, float& inv_p) { return nodeStepBent<false, true, false>(n, P, u, inv_p); }
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
    case 4: return shadecases::runFileHost<BisectLe>(buf, size, out, n_words);
    case 5: return shadecases::runFileHost<StepLe>(buf, size, out, n_words);
    case 6: return shadecases::runFileHost<StepNoFlip>(buf, size, out, n_words);
    case 7: return shadecases::runFileHost<StepNoR2>(buf, size, out, n_words);
    default: return 2;
    }
}
