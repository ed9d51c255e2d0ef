// trt_moments.h — the per-pixel arithmetic of trt_reproject_moments (include/trt.h): trt_reproject with the luminance's first two moments
// carried along, and the variance estimated from them.  Written once for the kernels (trt_moments_kernels.h) and for their CPU build
// (tests/moments).  trt_reproject.h's and trt_denoise.h's functions are used as they are (projection, tap tests, blend, demodulation, depth
// gradient, the integer power); plain fp32 operations in one fixed order, no contraction on either side (-ffp-contract=off), roots by
// trt_sqrt and exponentials by trt_expf_neg: hipcc for gfx950 and g++ on x86-64 give the same bits.
//
// The history of one pixel is trt_reproject's 36 bytes and one more 16-byte record, mom = (m1, m2, s, 0): the accumulated moments of the
// demodulated luminance and the sum of the squared frame weights behind them.
//   stage A  trt_mv_pixel    one pixel: trt_rp_pixel / trt_rp_pixel_motion with mom gathered and blended beside cv; the variance of a pixel
//                            on the temporal route
//   stage B  trt_mv_spatial  a pixel not on that route: the variance from a 7 x 7 window over this frame's mom, with trt_denoise's normal
//                            and depth weights
// trt_mv_temporal is the one predicate by which both stages tell the routes apart.
#ifndef TRT_MOMENTS_H
#define TRT_MOMENTS_H

#include "trt_reproject.h"

#define TRT_MV_MIN_DOF 0.1f   // the least 1 - (sum of squared weights) from which a variance is estimated: below it the divisor is noise
#define TRT_MV_RADIUS 3       // stage B's window is (2 R + 1)^2
#define TRT_MV_MIN_FRAMES 4

// trt_moments_params with its defaults filled in.
struct trt_mv_args {
    trt_rp_args rp;
    int sigma_normal;
    float sigma_depth;
    float min_frames;
};

// Every check of include/trt.h that needs no device, in its order.  required = every input and output buffer is there, given = how many of
// the five history buffers are.  Fills `a`.  nullptr, or what is wrong.
static inline const char* trt_mv_check(const trt_moments_params* p, int width, int height, bool required, int given, trt_mv_args& a)
{
    if (!p) return "null params";
    if (!required) return "null buffer";
    if (given != 0 && given != 5) return "partial history (prev_cv, prev_len, prev_normal, prev_depth and prev_mom: all or none)";
    if (width < 1 || height < 1) return "width and height must be >= 1";
    if ((unsigned long long)width * (unsigned long long)height > TRT_DENOISE_MAX_PIXELS) return "image larger than 2^28 pixels";
    if (const char* msg = trt_rp_resolve(p->rp, a.rp)) return msg;
    if (p->min_frames < 0 || p->min_frames > 255) return "min_frames must be 0..255";
    if (p->sigma_normal < 0 || p->sigma_normal > 256) return "sigma_normal must be 0..256";
    if (!(p->sigma_depth >= 0.0f)) return "sigma_depth must be >= 0";
    a.rp.width = width;
    a.rp.height = height;
    a.rp.history = given == 5;
    a.min_frames = (float)(p->min_frames ? p->min_frames : TRT_MV_MIN_FRAMES);
    a.sigma_normal = p->sigma_normal ? p->sigma_normal : TRT_DN_SIGMA_NORMAL;
    a.sigma_depth = p->sigma_depth != 0.0f ? p->sigma_depth : TRT_DN_SIGMA_DEPTH;
    return nullptr;
}

// Step 6's condition: the pixel's variance comes from its own history.  len and s are the pixel's NEW history length and weight sum, so
// stage B decides from what stage A wrote.  A pixel without history has s = 1 and is never on this route, whatever min_frames.
static inline TRT_HD bool trt_mv_temporal(const trt_mv_args& a, float depth, float len, float s)
{
    return trt_dn_hit(depth) && len >= a.min_frames && 1.0f - s >= TRT_MV_MIN_DOF;
}

// max(0, m2 - m1^2) / dof
static inline TRT_HD float trt_mv_estimate(float m1, float m2, float dof)
{
    const float d = m2 - m1 * m1;
    return (d > 0.0f ? d : 0.0f) / dof;
}

// What step 4 finds around (fx, fy): trt_rp_gather with the weighted mean of mom.xyz beside those of cv.xyz and the length (cv.w, the
// history's variance, is not needed: the variance is estimated anew every frame).
struct trt_mv_history {
    trt_dn4 cv, mom;
    float len;
    bool found;
};

// trt_rp_gather's taps, tests, weights and operations; per accepted tap mom is read last.
template <class H>
static inline TRT_HD trt_mv_history trt_mv_gather(const trt_rp_args& a, const H& hist, float fx, float fy, float zp, const float* np)
{
    trt_mv_history r;
    r.cv = trt_dn4{0.0f, 0.0f, 0.0f, 0.0f};
    r.mom = trt_dn4{0.0f, 0.0f, 0.0f, 0.0f};
    r.len = 0.0f;
    r.found = false;
    if (!(fx > -1.0f && fx < (float)a.width && fy > -1.0f && fy < (float)a.height)) return r;
    const float flx = floorf(fx), fly = floorf(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float wx = fx - flx, wy = fy - fly;
    float ws = 0.0f;
    TRT_UNROLL
    for (int j = 0; j < 2; ++j) {
        TRT_UNROLL
        for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i, qy = y0 + j;
            const float w = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
            if (!(w > 0.0f) || !trt_dn_inside(qx, qy, a.width, a.height)) continue;
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float zq = hist.depth(q);
            if (!trt_dn_hit(zq)) continue;
            float nq[3];
            hist.normal(q, nq);
            if (!trt_rp_tap_ok(a, zp, np, zq, nq)) continue;
            const trt_dn4 c = hist.cv(q);
            r.cv.x = r.cv.x + w * c.x;
            r.cv.y = r.cv.y + w * c.y;
            r.cv.z = r.cv.z + w * c.z;
            r.len = r.len + w * hist.len(q);
            const trt_dn4 m = hist.mom(q);
            r.mom.x = r.mom.x + w * m.x;
            r.mom.y = r.mom.y + w * m.y;
            r.mom.z = r.mom.z + w * m.z;
            ws = ws + w;
        }
    }
    if (!(ws >= TRT_RP_MIN_WEIGHT)) return r;
    r.cv.x = r.cv.x / ws;
    r.cv.y = r.cv.y / ws;
    r.cv.z = r.cv.z / ws;
    r.len = r.len / ws;
    r.mom.x = r.mom.x / ws;
    r.mom.y = r.mom.y / ws;
    r.mom.z = r.mom.z / ws;
    r.found = true;
    return r;
}

// One pixel's results of stage A.  cv.w and variance are final for a miss (0) and for a pixel on the temporal route; for any other hit
// pixel they are 0 until stage B has written them.
struct trt_mv_pixel_out {
    float color[3];
    float variance;
    trt_dn4 cv;
    float len;
    trt_dn4 mom;
};

// Steps 1 to 6 at pixel (x, y).  MOTION: steps 3' and 4' from prev_point[3] (x and y are then not used), else steps 3 and 4.
template <bool MOTION, class H>
static inline TRT_HD trt_mv_pixel_out trt_mv_pixel(const trt_mv_args& a, const H& hist, int x, int y, const float* color, const float* albedo,
                                                   const float* normal, float depth, const float* prev_point)
{
    trt_mv_pixel_out o;
    const trt_dn4 f = trt_dn_factor(albedo[0], albedo[1], albedo[2]);
    const trt_dn4 c = trt_dn_demodulate(color[0], color[1], color[2], 0.0f, f);
    const float l = trt_dn_lum(c.x, c.y, c.z);
    const float ll = l * l;
    // step 2: no history — the input's bits, a history of one frame
    o.color[0] = color[0];
    o.color[1] = color[1];
    o.color[2] = color[2];
    o.variance = 0.0f;
    o.cv = c;
    o.len = 1.0f;
    o.mom = trt_dn4{l, ll, 1.0f, 0.0f};
    if (!a.rp.history || !trt_dn_hit(depth)) return o;
    float fx, fy, zp;
    if (MOTION ? !trt_rp_project_point(a.rp, prev_point, fx, fy, zp) : !trt_rp_project(a.rp, x, y, depth, fx, fy, zp)) return o;
    const trt_mv_history h = trt_mv_gather(a.rp, hist, fx, fy, zp, normal);
    if (!h.found) return o;
    o.cv = trt_rp_blend(a.rp, c, h.cv, h.len, o.len);
    trt_dn_remodulate(o.cv, f, o.color);
    // trt_rp_blend's alpha', formed again by its operations
    const float r = 1.0f / o.len;
    const float al = a.rp.alpha > r ? a.rp.alpha : r;
    const float be = 1.0f - al;
    o.mom.x = h.mom.x + al * (l - h.mom.x);
    o.mom.y = h.mom.y + al * (ll - h.mom.y);
    o.mom.z = (al * al) + (be * be) * h.mom.z;
    o.cv.w = 0.0f;
    if (!trt_mv_temporal(a, depth, o.len, o.mom.z)) return o;
    o.cv.w = trt_mv_estimate(o.mom.x, o.mom.y, 1.0f - o.mom.z) * o.mom.z;
    const float la = trt_dn_lum(f.x, f.y, f.z);
    const float m = la > 1e-6f ? la : 1e-6f;
    o.variance = o.cv.w * (m * m);
    return o;
}

// Stage B at the hit pixel (x, y): var'.  The fetch reads THIS frame's pixels, in the image only: gd(x, y) = (n.x, n.y, n.z, z),
// mom(x, y) = stage A's record, f(x, y) = z (for trt_dn_depth_gradient).  Taps in the order dy = -R..R (rows), dx = -R..R.
template <class F>
static inline TRT_HD float trt_mv_spatial(const trt_mv_args& a, const F& f, int x, int y)
{
    const int W = a.rp.width, H = a.rp.height;
    const trt_dn4 gp = f.gd(x, y);
    const trt_dn4 mp = f.mom(x, y);
    const float zs = a.sigma_depth * trt_dn_depth_gradient(f, x, y, W, H);
    const float zn = 1e-3f * gp.w;
    float s1 = 0.0f, s2 = 0.0f, sw2 = 0.0f, ws = 0.0f;
    for (int dy = -TRT_MV_RADIUS; dy <= TRT_MV_RADIUS; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -TRT_MV_RADIUS; dx <= TRT_MV_RADIUS; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            float w;
            trt_dn4 mq;
            if (dx == 0 && dy == 0) {
                w = 1.0f;
                mq = mp;
            } else {
                const trt_dn4 gq = f.gd(qx, qy);
                if (!trt_dn_hit(gq.w)) continue;
                const float dn = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float wn = trt_dn_powi(dn > 0.0f ? dn : 0.0f, a.sigma_normal);
                const float dist = trt_sqrt((float)(dx * dx + dy * dy));
                const float wz = trt_expf_neg(-(fabsf(gp.w - gq.w) / (zs * dist + zn)));
                w = wn * wz;
                mq = f.mom(qx, qy);
            }
            s1 = s1 + w * mq.x;
            s2 = s2 + w * mq.y;
            sw2 = sw2 + (w * w) * mq.z;
            ws = ws + w;
        }
    }
    const float M1 = s1 / ws, M2 = s2 / ws;
    const float dof = 1.0f - sw2 / (ws * ws);
    // too few independent taps behind the pixel's edges (an isolated pixel: W2 = s_p): nothing can be estimated, and the conservative
    // choice is a standard deviation as large as the value itself
    const float v = dof >= TRT_MV_MIN_DOF ? trt_mv_estimate(M1, M2, dof) : M1 * M1;
    return v * mp.z;
}

// out_variance from var' and the albedo
static inline TRT_HD float trt_mv_remodulate_variance(float var, const float* albedo)
{
    const trt_dn4 f = trt_dn_factor(albedo[0], albedo[1], albedo[2]);
    const float la = trt_dn_lum(f.x, f.y, f.z);
    const float m = la > 1e-6f ? la : 1e-6f;
    return var * (m * m);
}

// The history in row-major global memory with 16-byte aligned cv and mom records: the fetch of stage A's kernel.
struct trt_mv_fetch {
    const trt_dn4* cvb;
    const float* lenb;
    const float* normalb;
    const float* depthb;
    const trt_dn4* momb;
    TRT_HD trt_dn4 cv(size_t q) const { return cvb[q]; }
    TRT_HD trt_dn4 mom(size_t q) const { return momb[q]; }
    TRT_HD float len(size_t q) const { return lenb[q]; }
    TRT_HD float depth(size_t q) const { return depthb[q]; }
    TRT_HD void normal(size_t q, float* n) const
    {
        n[0] = normalb[3 * q];
        n[1] = normalb[3 * q + 1];
        n[2] = normalb[3 * q + 2];
    }
};

// This frame's pixels in row-major global memory: stage B's fetch without a tile (TRT_MOMENTS_LDS=0).
struct trt_mv_frame {
    const trt_dn4* momb;
    const float* normalb;
    const float* depthb;
    int width;
    TRT_HD size_t at(int x, int y) const { return (size_t)y * (size_t)width + (size_t)x; }
    TRT_HD trt_dn4 mom(int x, int y) const { return momb[at(x, y)]; }
    TRT_HD float operator()(int x, int y) const { return depthb[at(x, y)]; }
    TRT_HD trt_dn4 gd(int x, int y) const
    {
        const size_t q = at(x, y);
        return trt_dn4{normalb[3 * q], normalb[3 * q + 1], normalb[3 * q + 2], depthb[q]};
    }
};

#endif  // TRT_MOMENTS_H
