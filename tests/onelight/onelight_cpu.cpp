// onelight_cpu.cpp — TEST INFRASTRUCTURE.  The CPU build of TRT_FLAG_ONE_LIGHT (include/trt.h): hostsim_render's per-path loop (tests/hostsim/hostsim.cpp,
// included for its HostScene) with the loop over the lights replaced by what k_shade's SHADE_PICK flavour and k_tail do under TileDesc::one_light —
// lightPick (trt_path.h), that light's lightSample, the occlusion test, the contribution times 1 / p.  Sums in k_tail's order.  Nothing in the product loads it.
#include "../hostsim/hostsim.cpp"

// One render of `p` (seed and spp as given) on a scene set up by onelight_render / onelight_render_seeds.
// mode 0: the feature.  1: inv_p forced to 1 (a biased estimator, for the sensitivity check of tests/test_one_light_cpu.py).  2: every light at every vertex,
// TRT_FLAG_FIXED_NEE's estimator — hostsim_render's own loop (the test holds the two to the same bits), here so that a scene is set up once for many renders.
namespace {
int renderWith(const HostScene& hs, const trt_params* p, uint32_t seed, int32_t n_spp, int mode, float* out_rgb, uint64_t rays[3])
{
    const bool pick = mode != 2 && hs.sc.n_lights >= 2;  // fewer than two lights: the flag does nothing, no draw is taken
    std::vector<int32_t> rows;
    for (int y = p->y0; y < p->y1; ++y)
        if (p->row_mod <= 1 || ((y / p->row_block) % p->row_mod) == p->row_rem) rows.push_back(y);
    const uint32_t tw = (uint32_t)(p->x1 - p->x0), npix = (uint32_t)rows.size() * tw;
    TileDesc td{};
    td.rows = rows.data();
    td.tile_w = (int32_t)tw; td.x0 = p->x0; td.width = p->width; td.height = p->height;
    td.npix = npix; td.seed = seed; td.spp = (uint32_t)n_spp;
    td.fixed_nee = 1u;
    td.fixed_pixels = (p->flags & TRT_FLAG_FIXED_PIXELS) ? 1u : 0u;
    td.ray_offset = (p->flags & TRT_FLAG_RAY_OFFSET) ? 1u : 0u;
    td.specular_ks = (p->flags & TRT_FLAG_SPECULAR_KS) ? 1u : 0u;
    td.npix_magic = magicOf(npix); td.tile_w_magic = magicOf(tw);
    td.one_light = pick ? 1u : 0u;
    uint64_t r_cam = 0, r_sh = 0, r_ind = 0;
    const uint32_t S = (uint32_t)n_spp;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : r_cam, r_sh, r_ind)
    for (long pl = 0; pl < (long)npix; ++pl) {
        ArrayStack stk = hs.stack();
        OctArrayStack ostk;
        uint32_t ni = 0, nt = 0;
        double acc[3] = {0, 0, 0};
        for (uint32_t sidx = 0; sidx < S; ++sidx) {
            const uint32_t pid = sidx * npix + (uint32_t)pl;
            const uint32_t r = (uint32_t)pl / tw, c = (uint32_t)pl - r * tw;
            const int y = rows[r], x = p->x0 + (int)c;
            Stream rng;
            rng.key = trt_rng_make_key(td.seed, (uint32_t)y * (uint32_t)td.width + (uint32_t)x, sidx);
            rng.ctr = 0;
            const float u1 = rng.next(), u2 = rng.next();
            f3 o, d;
            cameraRay(hs.sc.cam, td.width, td.height, y, x, u1, u2, o, d, td.fixed_pixels != 0u);
            f4 ra = mk4(o.x, o.y, o.z, d.x), rb = mk4(d.y, d.z, u2f(pid), u2f(packMeta(rng.ctr, TRT_META_CAMERA, 0))), bt = mk4(1, 1, 1, 0);
            f3 L = mk3(0, 0, 0);
            r_cam++;
            for (;;) {
                const Hit h = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), ostk, stk, ni, nt)
                                    : traceClosest<ArrayStack, false, 0>(hs.sc, mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), stk, ni, nt);
                const f4 hit4 = mk4(h.t, u2f((uint32_t)h.tri), h.u, h.v);
                ShadeCtx cx;
                shadeBegin(hs.sc, td, 0, ra, rb, bt, hit4, cx);
                if (cx.add_L) L = L + cx.addL;
                const uint32_t n_loop = pick ? 1u : hs.sc.n_lights;
                for (uint32_t lk = 0; lk < n_loop; ++lk) {
                    f3 wo, contrib;
                    float t_max = TRT_INF;
                    uint32_t li = lk;
                    float inv_p = 1.0f;
                    if (!cx.shade_ok || (pick && !lightPick(hs.sc, cx.rng, li, inv_p)) || !lightSample(hs.sc, cx.vx, *cx.m, li, cx.rng, wo, contrib, true, t_max)) continue;
                    if (mode == 1) inv_p = 1.0f;
                    if (pick) contrib = mk3(contrib.x * inv_p, contrib.y * inv_p, contrib.z * inv_p);
                    const f3 w = cx.beta * contrib;
                    r_sh++;
                    // the occlusion test: no light material, no light box
                    const Hit sh = hs.nk ? traceClosestOct<OctArrayStack, ArrayStack, false>(hs.sc, rayOrigin(cx, wo), wo, ostk, stk, ni, nt, t_max, true, false, nullptr)
                                         : traceClosest<ArrayStack, false, 0>(hs.sc, rayOrigin(cx, wo), wo, stk, ni, nt, t_max, true, false);
                    if (sh.tri < 0) L = L + w;
                }
                f4 nra, nrb, nbt;
                if (!shadeNext(cx, p->max_depth, nra, nrb, nbt)) break;
                ra = nra; rb = nrb; bt = nbt;
                r_ind++;
            }
            const float spp = (float)n_spp;
            acc[0] += (double)(L.x / spp);
            acc[1] += (double)(L.y / spp);
            acc[2] += (double)(L.z / spp);
        }
        out_rgb[(size_t)pl * 3 + 0] = (float)acc[0];
        out_rgb[(size_t)pl * 3 + 1] = (float)acc[1];
        out_rgb[(size_t)pl * 3 + 2] = (float)acc[2];
    }
    if (rays) { rays[0] = r_cam; rays[1] = r_sh; rays[2] = r_ind; }
    return g_breaches.exchange(0) ? 2 : 0;
}
// the scene as a handle holds it: with the selection table where there is something to select
struct PickScene {
    HostScene hs;
    std::vector<float> sel;
    explicit PickScene(const trt_scene* s) : hs(s), sel(s->n_lights)
    {
        lightSelTable(hs.lights.data(), s->n_lights, sel.data());
        hs.sc.light_sel = s->n_lights >= 2 ? sel.data() : nullptr;
    }
};
}  // namespace

// The tile of p (trt_render's packing) -> out_rgb, rays = (camera, shadow, indirect) rays traced.  p->flags must hold TRT_FLAG_FIXED_NEE (the library: TRT_EINVAL).
extern "C" int onelight_render(const trt_scene* s, const trt_params* p, float* out_rgb, uint64_t rays[3], int mutant)
{
    if (!s || !p || !out_rgb || !(p->flags & TRT_FLAG_FIXED_NEE)) return 1;
    PickScene ps(s);
    return renderWith(ps.hs, p, p->seed, p->spp, mutant, out_rgb, rays);
}
// n one-sample renders of the tile of p with the seeds p->seed + 1 + k (what tests/denoise_ref.py's oracle_inputs takes its variances from) -> out_rgb[n][pixels][3]
extern "C" int onelight_render_seeds(const trt_scene* s, const trt_params* p, int mutant, uint32_t n, float* out_rgb)
{
    if (!s || !p || !out_rgb || !(p->flags & TRT_FLAG_FIXED_NEE)) return 1;
    PickScene ps(s);
    int rows = 0;
    for (int y = p->y0; y < p->y1; ++y)
        if (p->row_mod <= 1 || ((y / p->row_block) % p->row_mod) == p->row_rem) rows++;
    const size_t floats = (size_t)rows * (size_t)(p->x1 - p->x0) * 3;
    for (uint32_t k = 0; k < n; ++k)
        if (int rc = renderWith(ps.hs, p, p->seed + 1u + k, 1, mutant, out_rgb + floats * k, nullptr)) return rc;
    return 0;
}

// lightPick on the caller's light tables: n lights of (area, radiance[3]) and m uniforms.  table != 0: SceneDev::light_sel holds the running sums (what a
// handle has); 0: null, the sums are formed by scanning.  Per uniform u[k]: lightPickAt(u[k]) -> sampled (0 / 1), the index, inv_p (with n < 2, where
// nothing is drawn, lightPick's answer).  draws[k]: what lightPick itself took from a stream of its own (key k), whose pick must be lightPickAt's for
// that stream's first uniform (-> 3 where it is not).  cdf_out (n floats, may be null): the running sums of lightSelTable.
extern "C" int onelight_pick(uint32_t n, const float* area, const float* radiance, int table, uint64_t m, const float* u, uint8_t* sampled, uint32_t* index, float* inv_p,
                             uint32_t* draws, float* cdf_out)
{
    std::vector<LightDev> lights(n);
    for (uint32_t l = 0; l < n; ++l) {
        trt_light t{};
        t.area = area[l];
        lights[l] = makeLightDevFrom(t, radiance + 3 * (size_t)l);
    }
    std::vector<float> sel(n);
    lightSelTable(lights.data(), n, sel.data());
    if (cdf_out && n) std::memcpy(cdf_out, sel.data(), n * sizeof(float));
    SceneDev sc{};
    sc.lights = lights.data();
    sc.n_lights = n;
    sc.light_sel = (table && n) ? sel.data() : nullptr;
    int rc = 0;
    for (uint64_t k = 0; k < m; ++k) {
        Stream rng;
        rng.key = trt_rng_make_key(0x0E11u, (uint32_t)k, (uint32_t)(k >> 32));
        rng.ctr = 0;
        uint32_t li = 0xFFFFFFFFu, li_s = 0xFFFFFFFFu;
        float ip = 0.0f, ip_s = 0.0f;
        const bool ok_s = lightPick(sc, rng, li_s, ip_s);
        draws[k] = rng.ctr;
        bool ok = ok_s;
        li = li_s; ip = ip_s;
        if (n >= 2u) {
            uint32_t li_c;
            float ip_c;
            const bool ok_c = lightPickAt(sc, trt_rng_uniform(rng.key, 0), li_c, ip_c);
            if (ok_c != ok_s || li_c != li_s || f2u(ip_c) != f2u(ip_s) || rng.ctr != 1u) rc = 3;
            ok = lightPickAt(sc, u[k], li, ip);
        }
        sampled[k] = ok ? 1 : 0;
        index[k] = li;
        inv_p[k] = ip;
    }
    return rc;
}
