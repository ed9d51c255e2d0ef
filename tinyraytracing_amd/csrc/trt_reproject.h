// trt_reproject.h — the per-pixel arithmetic of trt_reproject (include/trt.h): the temporal half of the denoiser.  Written once for the
// kernel (trt_reproject_kernels.h) and for its CPU build (tests/reproject): demodulation (trt_denoise.h's functions, so that the history and
// the filter share one domain), the pixel's world point, its place in the previous image, the four bilinear taps with their tests, the
// blend.  Plain fp32 operations in one fixed order, no contraction on either side (-ffp-contract=off), the two normalisations by trt_sqrt:
// hipcc for gfx950 and g++ on x86-64 give the same bits.
//
// The history of one pixel is 36 bytes in four buffers: cv (c.r, c.g, c.b, var) as trt_denoise.h defines it, the history length, and the
// previous frame's own normal and depth.  Pixels are read through a fetch object (depth(q), normal(q), cv(q), len(q), q = y * width + x).
#ifndef TRT_REPROJECT_H
#define TRT_REPROJECT_H

#include <stdint.h>
#include <math.h>
#include <string.h>

#include "trt_denoise.h"

#define TRT_RP_ALPHA 0.2f
#define TRT_RP_DEPTH_TOLERANCE 0.1f
#define TRT_RP_NORMAL_THRESHOLD 0.9f
#define TRT_RP_MAX_HISTORY 255.0f
#define TRT_RP_MIN_WEIGHT 0.01f  // the least sum of bilinear weights of accepted taps that still counts as history

// trt_reproject_params with its defaults filled in, and what is the same for every pixel.
struct trt_rp_args {
    int width, height;
    int fixed;    // TRT_FLAG_FIXED_PIXELS: which pixel grid the cameras use
    int same;     // cur and prev are byte-identical: no geometry, the pixel is its own source
    int history;  // the caller gave a history
    float alpha, depth_tolerance, max_history;
    float normal_threshold2;  // normal_threshold^2
    trt_camera cur, prev;
};

// The checks of include/trt.h on the parameters alone; fills `a` (width, height and history are the caller's to set).  nullptr, or what is wrong.
static inline const char* trt_rp_resolve(const trt_reproject_params& p, trt_rp_args& a)
{
    if (!(p.alpha >= 0.0f && p.alpha <= 1.0f)) return "alpha must be in [0, 1]";
    if (!(p.depth_tolerance >= 0.0f)) return "depth_tolerance must be >= 0";
    if (!(p.normal_threshold >= 0.0f && p.normal_threshold <= 1.0f)) return "normal_threshold must be in [0, 1]";
    if (!(p.max_history == 0.0f || p.max_history >= 1.0f)) return "max_history must be 0 or >= 1";
    if (p.flags & ~TRT_FLAG_FIXED_PIXELS) return "flags may hold TRT_FLAG_FIXED_PIXELS only";
    a.fixed = (p.flags & TRT_FLAG_FIXED_PIXELS) ? 1 : 0;
    a.same = memcmp(&p.cur, &p.prev, sizeof(trt_camera)) == 0 ? 1 : 0;
    a.alpha = p.alpha != 0.0f ? p.alpha : TRT_RP_ALPHA;
    a.depth_tolerance = p.depth_tolerance != 0.0f ? p.depth_tolerance : TRT_RP_DEPTH_TOLERANCE;
    const float thr = p.normal_threshold != 0.0f ? p.normal_threshold : TRT_RP_NORMAL_THRESHOLD;
    a.normal_threshold2 = thr * thr;
    a.max_history = p.max_history != 0.0f ? p.max_history : TRT_RP_MAX_HISTORY;
    a.cur = p.cur;
    a.prev = p.prev;
    return nullptr;
}

// Every check of include/trt.h that needs no device, in its order, for the entry points and the CPU build alike.  required = every input
// and output buffer is there, given = how many of the four history buffers are.  Fills `a` completely.  nullptr, or what is wrong.
static inline const char* trt_rp_check(const trt_reproject_params* p, int width, int height, bool required, int given, trt_rp_args& a)
{
    if (!p) return "null params";
    if (!required) return "null buffer";
    if (given != 0 && given != 4) return "partial history (prev_cv, prev_len, prev_normal and prev_depth: all or none)";
    if (width < 1 || height < 1) return "width and height must be >= 1";
    if ((unsigned long long)width * (unsigned long long)height > TRT_DENOISE_MAX_PIXELS) return "image larger than 2^28 pixels";
    if (const char* msg = trt_rp_resolve(*p, a)) return msg;
    a.width = width;
    a.height = height;
    a.history = given == 4;
    return nullptr;
}

static inline TRT_HD float trt_rp_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// a . (b x c)
static inline TRT_HD float trt_rp_det(const float* a, const float* b, const float* c)
{
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// Steps 3 and 4: where pixel (x, y) of the current frame, seen at distance `depth`, lay in the previous image: continuous pixel coordinates
// (fx, fy) and the depth zp the previous frame would have stored.  false: no such place (behind the previous eye, a degenerate camera, or
// anything that is not a number).  fx and fy may lie far outside the image; trt_rp_gather rejects those before any conversion to int.
static inline TRT_HD bool trt_rp_project(const trt_rp_args& a, int x, int y, float depth, float& fx, float& fy, float& zp)
{
    if (a.same) {
        fx = (float)x;
        fy = (float)y;
        zp = depth;
        return true;
    }
    const float W = (float)a.width, H = (float)a.height;
    float s, t;
    if (a.fixed) {
        s = ((float)x + 0.5f) / W;
        t = ((float)(a.height - 1 - y) + 0.5f) / H;
    } else {
        s = (float)x / (W - 1.0f);
        t = (float)(a.height - y) / (H - 1.0f);  // Q1
    }
    float d[3], v[3], A[3];
    TRT_UNROLL
    for (int k = 0; k < 3; ++k) d[k] = ((a.cur.lower_left_corner[k] + a.cur.horizontal[k] * s) + a.cur.vertical[k] * t) - a.cur.eye[k];
    const float dl = trt_sqrt(trt_rp_dot(d, d));
    TRT_UNROLL
    for (int k = 0; k < 3; ++k) {
        const float P = a.cur.eye[k] + (d[k] / dl) * depth;
        v[k] = P - a.prev.eye[k];
        A[k] = a.prev.lower_left_corner[k] - a.prev.eye[k];
    }
    // v = k A + (k s') horizontal + (k t') vertical, by Cramer's rule
    const float det = trt_rp_det(A, a.prev.horizontal, a.prev.vertical);
    if (det == 0.0f) return false;
    const float k = trt_rp_det(v, a.prev.horizontal, a.prev.vertical) / det;
    if (!(k > 0.0f)) return false;
    const float sp = (trt_rp_det(A, v, a.prev.vertical) / det) / k;
    const float tp = (trt_rp_det(A, a.prev.horizontal, v) / det) / k;
    if (a.fixed) {
        fx = sp * W - 0.5f;
        fy = ((float)(a.height - 1) + 0.5f) - tp * H;
    } else {
        fx = sp * (W - 1.0f);
        fy = H - tp * (H - 1.0f);
    }
    zp = trt_sqrt(trt_rp_dot(v, v));
    return true;
}

// Step 5, one tap: does the previous frame's pixel (normal nq, depth zq) show the surface that the current pixel (normal np, reprojected
// depth zp) shows?  Normals are means of unit vectors, so the cosine test is taken on squares: no square root.
static inline TRT_HD bool trt_rp_tap_ok(const trt_rp_args& a, float zp, const float* np, float zq, const float* nq)
{
    if (!trt_dn_hit(zq)) return false;
    if (!(fabsf(zp - zq) <= a.depth_tolerance * zp)) return false;
    const float dn = trt_rp_dot(np, nq);
    if (!(dn > 0.0f)) return false;
    return dn * dn >= (a.normal_threshold2 * trt_rp_dot(np, np)) * trt_rp_dot(nq, nq);
}

// What step 5 finds around (fx, fy): the weighted means of cv and of the history length over the accepted taps.
struct trt_rp_history {
    trt_dn4 cv;
    float len;
    bool found;
};

// Taps in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).  A tap of weight 0 is not read (so a still camera reads its
// own pixel only).  Per tap the depth is read first, then the normal, then cv and the length: a rejected tap costs 4 or 16 bytes, not 36.
template <class H>
static inline TRT_HD trt_rp_history trt_rp_gather(const trt_rp_args& a, const H& hist, float fx, float fy, float zp, const float* np)
{
    trt_rp_history r;
    r.cv = trt_dn4{0.0f, 0.0f, 0.0f, 0.0f};
    r.len = 0.0f;
    r.found = false;
    // also false for a NaN; after this floorf(f) lies in [-1, size - 1] and converts exactly
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
            r.cv.w = r.cv.w + w * c.w;
            r.len = r.len + w * hist.len(q);
            ws = ws + w;
        }
    }
    if (!(ws >= TRT_RP_MIN_WEIGHT)) return r;
    r.cv.x = r.cv.x / ws;
    r.cv.y = r.cv.y / ws;
    r.cv.z = r.cv.z / ws;
    r.cv.w = r.cv.w / ws;
    r.len = r.len / ws;
    r.found = true;
    return r;
}

// Step 6: the new frame's demodulated (c, var) blended into the history's (c_h, var_h) of length n_h.  -> the new cv; n = the new length.
static inline TRT_HD trt_dn4 trt_rp_blend(const trt_rp_args& a, const trt_dn4& c, const trt_dn4& h, float n_h, float& n)
{
    const float n1 = n_h + 1.0f;
    n = n1 < a.max_history ? n1 : a.max_history;
    const float r = 1.0f / n;
    const float al = a.alpha > r ? a.alpha : r;
    const float be = 1.0f - al;
    trt_dn4 o;
    o.x = h.x + al * (c.x - h.x);
    o.y = h.y + al * (c.y - h.y);
    o.z = h.z + al * (c.z - h.z);
    o.w = (al * al) * c.w + (be * be) * h.w;
    return o;
}

// One pixel's results: what goes on to trt_denoise (color, variance) and the next frame's history (cv, len).
struct trt_rp_pixel_out {
    float color[3];
    float variance;
    trt_dn4 cv;
    float len;
};

// Steps 1 to 7 at pixel (x, y).
template <class H>
static inline TRT_HD trt_rp_pixel_out trt_rp_pixel(const trt_rp_args& a, const H& hist, int x, int y, const float* color, float variance,
                                                   const float* albedo, const float* normal, float depth)
{
    trt_rp_pixel_out o;
    const trt_dn4 f = trt_dn_factor(albedo[0], albedo[1], albedo[2]);
    const trt_dn4 c = trt_dn_demodulate(color[0], color[1], color[2], variance, f);
    // steps 2 and 7: no history — the input's bits
    o.color[0] = color[0];
    o.color[1] = color[1];
    o.color[2] = color[2];
    o.variance = variance;
    o.cv = c;
    o.len = 1.0f;
    if (!a.history || !trt_dn_hit(depth)) return o;
    float fx, fy, zp;
    if (!trt_rp_project(a, x, y, depth, fx, fy, zp)) return o;
    const trt_rp_history h = trt_rp_gather(a, hist, fx, fy, zp, normal);
    if (!h.found) return o;
    o.cv = trt_rp_blend(a, c, h.cv, h.len, o.len);
    trt_dn_remodulate(o.cv, f, o.color);
    const float l = trt_dn_lum(f.x, f.y, f.z);
    const float m = l > 1e-6f ? l : 1e-6f;
    o.variance = o.cv.w * (m * m);
    return o;
}

// ---- trt_reproject_motion: the surface may have moved ------------------------------------------------------------------------------------
// Steps 3 and 4 with the world point given: `point` is where the surface seen through the pixel was at the time of the history frame
// (trt_trace_points on the geometry of that time).  From v = point - prev.eye on, trt_rp_project's operations in trt_rp_project's order, so
// the point that function forms itself gives that function's bits.  a.cur and a.same are not used: a still camera does not mean a still
// surface.  false: no such place — anything that is not a number (a miss of trt_trace_points is three NaNs), a point behind or on the
// previous eye, a degenerate camera, a z' that is not finite (a point some 1e19 away, whose |v|^2 leaves fp32).
static inline TRT_HD bool trt_rp_project_point(const trt_rp_args& a, const float* point, float& fx, float& fy, float& zp)
{
    const float W = (float)a.width, H = (float)a.height;
    float v[3], A[3];
    TRT_UNROLL
    for (int k = 0; k < 3; ++k) {
        v[k] = point[k] - a.prev.eye[k];
        A[k] = a.prev.lower_left_corner[k] - a.prev.eye[k];
    }
    const float det = trt_rp_det(A, a.prev.horizontal, a.prev.vertical);
    if (det == 0.0f) return false;
    const float k = trt_rp_det(v, a.prev.horizontal, a.prev.vertical) / det;
    if (!(k > 0.0f)) return false;
    const float sp = (trt_rp_det(A, v, a.prev.vertical) / det) / k;
    const float tp = (trt_rp_det(A, a.prev.horizontal, v) / det) / k;
    if (a.fixed) {
        fx = sp * W - 0.5f;
        fy = ((float)(a.height - 1) + 0.5f) - tp * H;
    } else {
        fx = sp * (W - 1.0f);
        fy = H - tp * (H - 1.0f);
    }
    zp = trt_sqrt(trt_rp_dot(v, v));
    return zp <= 3.4028235e38f;
}

// Steps 1 to 7 of one pixel (where it lies in the current image does not matter) with steps 3 and 4 taken from prev_point[3]: trt_rp_pixel's functions in trt_rp_pixel's order otherwise.
template <class H>
static inline TRT_HD trt_rp_pixel_out trt_rp_pixel_motion(const trt_rp_args& a, const H& hist, const float* color, float variance,
                                                          const float* albedo, const float* normal, float depth, const float* prev_point)
{
    trt_rp_pixel_out o;
    const trt_dn4 f = trt_dn_factor(albedo[0], albedo[1], albedo[2]);
    const trt_dn4 c = trt_dn_demodulate(color[0], color[1], color[2], variance, f);
    o.color[0] = color[0];
    o.color[1] = color[1];
    o.color[2] = color[2];
    o.variance = variance;
    o.cv = c;
    o.len = 1.0f;
    if (!a.history || !trt_dn_hit(depth)) return o;
    float fx, fy, zp;
    if (!trt_rp_project_point(a, prev_point, fx, fy, zp)) return o;
    const trt_rp_history h = trt_rp_gather(a, hist, fx, fy, zp, normal);
    if (!h.found) return o;
    o.cv = trt_rp_blend(a, c, h.cv, h.len, o.len);
    trt_dn_remodulate(o.cv, f, o.color);
    const float l = trt_dn_lum(f.x, f.y, f.z);
    const float m = l > 1e-6f ? l : 1e-6f;
    o.variance = o.cv.w * (m * m);
    return o;
}

// The history in row-major global memory with 16-byte aligned cv records: the fetch of the kernel (the CPU build reads cv float by float).
struct trt_rp_fetch {
    const trt_dn4* cvb;
    const float* lenb;
    const float* normalb;
    const float* depthb;
    TRT_HD trt_dn4 cv(size_t q) const { return cvb[q]; }
    TRT_HD float len(size_t q) const { return lenb[q]; }
    TRT_HD float depth(size_t q) const { return depthb[q]; }
    TRT_HD void normal(size_t q, float* n) const
    {
        n[0] = normalb[3 * q];
        n[1] = normalb[3 * q + 1];
        n[2] = normalb[3 * q + 2];
    }
};

#endif  // TRT_REPROJECT_H
