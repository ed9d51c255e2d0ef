// trt_denoise.h — the per-pixel arithmetic of the edge-avoiding a-trous filter (include/trt.h, trt_denoise), written once for the
// kernels (trt_denoise_kernels.h) and for their CPU build (tests/denoise): demodulation, the depth gradient, the variance prefilter, one
// level's tap loop in a fixed order, remodulation.  Plain fp32 operations, no contraction on either side (-ffp-contract=off), exponentials
// by trt_expf_neg and square roots by trt_sqrt: hipcc for gfx950 and g++ on x86-64 give the same bits.
//
// Buffers of one call, one 16-B record per pixel:
//   cv  (c.r, c.g, c.b, var)   demodulated colour and its variance; ping-pong between levels
//   gd  (n.x, n.y, n.z, z)     the guide: normal and depth, as given
//   aux (a.r, a.g, a.b, gz)    the demodulation factor and the depth gradient
// Pixels are read through a fetch object (cv(x, y), gd(x, y), var(x, y)): global memory, or a tile in LDS; the arithmetic does not change.
#ifndef TRT_DENOISE_H
#define TRT_DENOISE_H

#include <stdint.h>
#include <math.h>

#include "trt.h"
#include "trt_prims.h"
#include "trt_exact.h"

struct alignas(16) trt_dn4 {
    float x, y, z, w;
};

// The resolved parameters of one level (trt_denoise_params with its defaults filled in).
struct trt_dn_args {
    int width, height;
    int step;             // 2^level
    int sigma_normal;     // 1..256
    float sigma_depth;
    float sigma_luminance;
};

#define TRT_DN_ITERATIONS 5
#define TRT_DN_SIGMA_NORMAL 128
#define TRT_DN_SIGMA_DEPTH 1.0f
#define TRT_DN_SIGMA_LUMINANCE 4.0f
#define TRT_DN_CENTRE 0.140625f  // h_2^2 = (3/8)^2

static inline TRT_HD bool trt_dn_hit(float z) { return z < TRT_INF; }

static inline TRT_HD float trt_dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

static inline TRT_HD bool trt_dn_inside(int x, int y, int w, int h) { return x >= 0 && x < w && y >= 0 && y < h; }

// h_i of the 5-tap B3 spline kernel {1/16, 1/4, 3/8, 1/4, 1/16}
static inline TRT_HD float trt_dn_h(int i) { return i == 2 ? 0.375f : (i == 1 || i == 3) ? 0.25f : 0.0625f; }

// The Euclidean length of a tap offset (i-2, j-2), d2 = its squared length in {1, 2, 4, 5, 8}: the correctly rounded square roots.
static inline TRT_HD float trt_dn_radius(int d2)
{
    return d2 == 1 ? 1.0f : d2 == 2 ? 1.41421353816986083984375f : d2 == 4 ? 2.0f : d2 == 5 ? 2.2360680103302001953125f : 2.8284270763397216796875f;
}
// Slot of that length among the five (the per-pixel depth denominators are formed once per slot).
static inline TRT_HD int trt_dn_radius_slot(int d2) { return d2 == 1 ? 0 : d2 == 2 ? 1 : d2 == 4 ? 2 : d2 == 5 ? 3 : 4; }

// Step 1. a = albedo with non-positive channels replaced by 1 (.w unused, 0).
static inline TRT_HD trt_dn4 trt_dn_factor(float ar, float ag, float ab)
{
    trt_dn4 a;
    a.x = ar > 0.0f ? ar : 1.0f;
    a.y = ag > 0.0f ? ag : 1.0f;
    a.z = ab > 0.0f ? ab : 1.0f;
    a.w = 0.0f;
    return a;
}
// c = color / a, var = variance / max(lum(a), 1e-6)^2.
static inline TRT_HD trt_dn4 trt_dn_demodulate(float cr, float cg, float cb, float variance, const trt_dn4& a)
{
    const float l = trt_dn_lum(a.x, a.y, a.z);
    const float m = l > 1e-6f ? l : 1e-6f;
    trt_dn4 c;
    c.x = cr / a.x;
    c.y = cg / a.y;
    c.z = cb / a.z;
    c.w = variance / (m * m);
    return c;
}
// Step 4. out = c * a.
static inline TRT_HD void trt_dn_remodulate(const trt_dn4& c, const trt_dn4& a, float* out3)
{
    out3[0] = c.x * a.x;
    out3[1] = c.y * a.y;
    out3[2] = c.z * a.z;
}

// Step 2, one axis: the smaller |z_q - z_p| over the axis neighbours that are in-image hits (ha / hb say which are); 0 if neither.
static inline TRT_HD float trt_dn_axis(float zp, bool ha, float za, bool hb, float zb)
{
    const float da = fabsf(za - zp), db = fabsf(zb - zp);
    if (ha && hb) return db < da ? db : da;
    return ha ? da : hb ? db : 0.0f;
}
// gz of pixel (x, y); depth(x, y) reads the depth of an in-image pixel.
template <class Depth>
static inline TRT_HD float trt_dn_depth_gradient(const Depth& depth, int x, int y, int w, int h)
{
    const float zp = depth(x, y);
    const bool l = x > 0, r = x + 1 < w, u = y > 0, d = y + 1 < h;
    const float zl = l ? depth(x - 1, y) : 0.0f, zr = r ? depth(x + 1, y) : 0.0f;
    const float zu = u ? depth(x, y - 1) : 0.0f, zd = d ? depth(x, y + 1) : 0.0f;
    const float gx = trt_dn_axis(zp, l && trt_dn_hit(zl), zl, r && trt_dn_hit(zr), zr);
    const float gy = trt_dn_axis(zp, u && trt_dn_hit(zu), zu, d && trt_dn_hit(zd), zd);
    return gy > gx ? gy : gx;
}

// b^e for an integer e >= 1 by repeated squaring (e = 128: seven squarings and one exact product with 1).
static inline TRT_HD float trt_dn_powi(float b, int e)
{
    float r = 1.0f;
    for (;;) {
        if (e & 1) r = r * b;
        e >>= 1;
        if (!e) break;
        b = b * b;
    }
    return r;
}

// G3(var) at (x, y): the 3x3 binomial [1/4, 1/2, 1/4]^2 over the in-image pixels, renormalised (the weights and their sum are exact).
template <class F>
static inline TRT_HD float trt_dn_prefilter(const F& f, int x, int y, int w, int h)
{
    float acc = 0.0f, ws = 0.0f;
    TRT_UNROLL
    for (int j = -1; j <= 1; ++j) {
        TRT_UNROLL
        for (int i = -1; i <= 1; ++i) {
            if (!trt_dn_inside(x + i, y + j, w, h)) continue;
            const float k = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
            acc = acc + k * f.var(x + i, y + j);
            ws = ws + k;
        }
    }
    return acc / ws;
}

// Step 3, one level at pixel (x, y): the new (c, var).  gz = the pixel's depth gradient.  Taps in the order j = 0..4 (rows), i = 0..4.
// The two exponent denominators are formed once per pixel (the luminance one) and once per tap distance (the depth ones), and the
// quotients are taken as products with their reciprocals.
template <class F>
static inline TRT_HD trt_dn4 trt_dn_level(const F& f, int x, int y, float gz, const trt_dn_args& a)
{
    const trt_dn4 gp = f.gd(x, y);
    const trt_dn4 cp = f.cv(x, y);
    if (!trt_dn_hit(gp.w)) return cp;
    const float sd = trt_sqrt(trt_dn_prefilter(f, x, y, a.width, a.height));
    const float lp = trt_dn_lum(cp.x, cp.y, cp.z);
    const float inv_l = 1.0f / (a.sigma_luminance * sd + 1e-6f);
    const float zs = (a.sigma_depth * gz) * (float)a.step;  // sigma_z gz s: |q - p| = s * radius, and s is a power of two
    const float zn = 1e-3f * gp.w;
    float inv_z[5];
    TRT_UNROLL
    for (int k = 0; k < 5; ++k) inv_z[k] = 1.0f / (zs * trt_dn_radius(k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 4 : k == 3 ? 5 : 8) + zn);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, ws = 0.0f;
    TRT_UNROLL
    for (int j = 0; j < 5; ++j) {
        const int qy = y + a.step * (j - 2);
        if (qy < 0 || qy >= a.height) continue;
        TRT_UNROLL
        for (int i = 0; i < 5; ++i) {
            const int qx = x + a.step * (i - 2);
            if (qx < 0 || qx >= a.width) continue;
            float w;
            trt_dn4 cq;
            if (i == 2 && j == 2) {
                w = TRT_DN_CENTRE;
                cq = cp;
            } else {
                const trt_dn4 gq = f.gd(qx, qy);
                if (!trt_dn_hit(gq.w)) continue;
                cq = f.cv(qx, qy);
                const float dn = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float wn = trt_dn_powi(dn > 0.0f ? dn : 0.0f, a.sigma_normal);
                const int d2 = (i - 2) * (i - 2) + (j - 2) * (j - 2);
                const float wz = trt_expf_neg(-(fabsf(gp.w - gq.w) * inv_z[trt_dn_radius_slot(d2)]));
                const float wl = trt_expf_neg(-(fabsf(lp - trt_dn_lum(cq.x, cq.y, cq.z)) * inv_l));
                w = (((trt_dn_h(i) * trt_dn_h(j)) * wn) * wz) * wl;
            }
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
            ws = ws + w;
        }
    }
    trt_dn4 o;
    o.x = sr / ws;
    o.y = sg / ws;
    o.z = sb / ws;
    o.w = sv / (ws * ws);
    return o;
}

// Pixels of row-major buffers of `width` pixels: the global-memory fetch of the kernels and the CPU build.
struct trt_dn_fetch {
    const trt_dn4* cvb;
    const trt_dn4* gdb;
    int width;
    TRT_HD trt_dn4 cv(int x, int y) const { return cvb[(size_t)y * (size_t)width + (size_t)x]; }
    TRT_HD trt_dn4 gd(int x, int y) const { return gdb[(size_t)y * (size_t)width + (size_t)x]; }
    TRT_HD float var(int x, int y) const { return cvb[(size_t)y * (size_t)width + (size_t)x].w; }
};
struct trt_dn_depth {
    const float* z;
    int width;
    TRT_HD float operator()(int x, int y) const { return z[(size_t)y * (size_t)width + (size_t)x]; }
};

#endif  // TRT_DENOISE_H
