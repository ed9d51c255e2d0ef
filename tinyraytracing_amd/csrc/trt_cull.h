// trt_cull.h — which camera rays of a tile render provably miss the scene: a pixel rectangle and two guard bands, formed on the
// host once per render call (renderCore) from the handle's camera and the two child boxes of the root of the caller's BVH2.
// Plain C++ in binary64, no device code: tests/cull compiles it with g++ next to cameraRay / boxTest / boxTestGlm (trt_path.h).
//
// A camera ray of pixel (i, j) = (row, column) is CULLED iff the pixel lies outside the rectangle [j_lo, j_hi] x [i_lo, i_hi] and
// in neither band (a band of rows, a band of columns).  A culled ray misses both root boxes under the clean slab test (boxTest)
// and under the literal one (boxTestGlm), for every jitter, and none of its direction components is zero: it returns the miss
// record whichever driver walks it, contributes +0.0 to its pixel and is not a ray of raySpecial() (trt_stats::redo_rays).
//
// The rectangle.  cameraRay forms d = normalize(((llc + hor s) + ver t) - eye).  For a point p in front of the camera,
// p - eye = lambda ((llc - eye) + hor s + ver t) has one solution (s, t, lambda > 0): the central projection of p onto the image
// plane.  It maps segments to segments, so the rays that can reach a convex box all of whose corners lie in front have their
// (s, t) in the hull of the eight projected corners, hence in the bounding rectangle of those.  A pixel column (row) is kept
// where its s (t) interval — cameraRay's own three grid forms: Q1's row shift (H - i) / (H - 1), Q2's jitter of 1 / W on a
// 1 / (W - 1) grid, and the `fixed` form — widened by the margin below, meets that rectangle.
//
// The roundings, and the bound on them that the margin rests on (u = 2^-24, fp32):
//   s, t         (float)x, (float)y: |ds| <= u |s|, and |s|, |t| < 3 for every W, H >= 2.  The binary64 grid itself is exact to
//                2^-52.  Both are covered by widening every interval by 2^-21 (>= 3 u with slack).
//   direction    component k of ((llc + hor s) + ver t) - eye takes two products and three sums, each rounded relative to a value of
//                at most S_k = |llc_k| + 3 |hor_k| + 3 |ver_k| + |eye_k|; normalize() multiplies by one rounded factor (a common
//                scale, which a slab test does not see) and rounds each product once more.  Together below e_k = 2^-20 S_k per
//                component, in units of the un-normalised direction D.  A ray along D + e that meets a box at p = eye + tau (D + e)
//                has the exact ray's point eye + tau D within tau |e| of p, and tau <= lambda_max, the largest lambda of a
//                corner: the exact ray meets the box grown by lambda_max max_k e_k on every side.
//   slab test    t = (plane - o) * (1 / d): three roundings, relative error below 2^-22.  That is the exact quotient for a plane
//                moved to o + (plane - o)(1 + eps): the test is exact on a box whose planes are shifted by at most
//                2^-22 |plane - o|.  No product can underflow to a wrong sign (|1 / d| >= 1), and none is NaN, the
//                zero-direction guard keeping every 1 / d finite.
// So what is projected is grown on axis k by
//   pad_k = 2 lambda_max max e + 2^-21 max(|lo_k - eye_k|, |hi_k - eye_k|),
// lambda_max and the distances taken over the union of the two child boxes, the factor 2 leaving room for lambda_max to grow with
// the box (checked: culling is off where it does not suffice), and every pixel interval is widened outwards by one full pixel
// pitch (1 / (W - 1), 1 / (H - 1): the larger of the two grids') plus 2^-21.  The eight corners of the padded union decide whether
// culling is on; the rectangle comes from the two boxes cut into slabs (below), each padded the same way, a subset of that union.
//
// Culling is off (nothing is culled) when: the tree has no inner node; W or H is below 2; a box coordinate or a camera
// component is not finite; the 3 x 3 system of a corner is singular or a corner has lambda <= 0 (eye inside or beside the box,
// box behind the camera); the padding does not converge; or a slanted zero set touches the culled area (below).
//
// Zero-direction guard.  D_k = (llc_k - eye_k) + hor_k s + ver_k t is affine in (s, t).  It counts as possibly zero where
// |D_k| <= g_k = max(2^-20 S_k, 2^-90 sum S): the sum of its fp32 roundings with slack, and large enough that D_k (1 / len)
// (len <= sum S) stays above 2^-91, far from underflow and from the 2.9e-39 below which 1 / d is infinite.  With hor_k == 0 the
// zero set is a band of rows, with ver_k == 0 a band of columns: they go into the guard bands (the bands of the three components
// merged into one interval of rows and one of columns).  A zero set that is slanted, or a component that is constant and within
// g_k, turns culling off if it comes within g_k anywhere on the culled side of the frame.
#pragma once
#include <math.h>
#include <stdint.h>

#include "trt.h"

namespace trtd {

struct CullBound {
    bool active;        // false: nothing is culled, `why` says why
    const char* why;
    // inclusive, in image pixels; a band with lo > hi is empty.  Meaningful only when active.
    int32_t j_lo, j_hi, i_lo, i_hi;
    int32_t row_lo, row_hi, col_lo, col_hi;
    // TileDesc::cull (trt_path.h): columns culled on the left, on the right, rows at the top, at the bottom, then (first, count) of
    // the band of rows and of the band of columns.  All zero = nothing culled.
    int32_t v[8];
};

namespace cull_detail {

inline void colS(int W, bool fixed, int j, double& a, double& b)
{
    if (fixed) { a = double(j) / double(W); b = (double(j) + 1.0) / double(W); }
    else { const double c = double(j) / double(W - 1.0); a = c - 0.5 / double(W); b = c + 0.5 / double(W); }
}
inline void rowT(int H, bool fixed, int i, double& a, double& b)
{
    if (fixed) { a = double(H - 1 - i) / double(H); b = double(H - i) / double(H); }
    else { const double c = double(H - i) / double(H - 1.0); a = c - 0.5 / double(H); b = c + 0.5 / double(H); }
}
// s rises with the column, t falls with the row.  Columns whose widened interval meets [lo, hi]: [first, last], empty when first > last.
inline void colsMeeting(int W, bool fixed, double m, double lo, double hi, int& first, int& last)
{
    int a = 0, b = W;  // first column with b_j + m >= lo
    while (a < b) { const int j = a + (b - a) / 2; double x0, x1; colS(W, fixed, j, x0, x1); if (x1 + m >= lo) b = j; else a = j + 1; }
    first = a;
    a = 0; b = W;      // first column with a_j - m > hi
    while (a < b) { const int j = a + (b - a) / 2; double x0, x1; colS(W, fixed, j, x0, x1); if (x0 - m > hi) b = j; else a = j + 1; }
    last = a - 1;
}
inline void rowsMeeting(int H, bool fixed, double m, double lo, double hi, int& first, int& last)
{
    int a = 0, b = H;  // first row with a_i - m <= hi
    while (a < b) { const int i = a + (b - a) / 2; double x0, x1; rowT(H, fixed, i, x0, x1); if (x0 - m <= hi) b = i; else a = i + 1; }
    first = a;
    a = 0; b = H;      // first row with b_i + m < lo
    while (a < b) { const int i = a + (b - a) / 2; double x0, x1; rowT(H, fixed, i, x0, x1); if (x1 + m < lo) b = i; else a = i + 1; }
    last = a - 1;
}
// least |a0 + a1 s + a2 t| over [s0, s1] x [t0, t1]
inline double minAbsAffine(double a0, double a1, double a2, double s0, double s1, double t0, double t1)
{
    const double v[4] = {a0 + a1 * s0 + a2 * t0, a0 + a1 * s1 + a2 * t0, a0 + a1 * s0 + a2 * t1, a0 + a1 * s1 + a2 * t1};
    double lo = v[0], hi = v[0];
    for (int k = 1; k < 4; ++k) { lo = fmin(lo, v[k]); hi = fmax(hi, v[k]); }
    if (!(lo > 0.0) && !(hi < 0.0)) return 0.0;  // (a NaN lands here too)
    return fmin(fabs(lo), fabs(hi));
}
// (s, t, lambda) of point p: hor s + ver t - mu (p - eye) = -(llc - eye), lambda = 1 / mu.  False: singular, not finite or not in front.
inline bool project(const double A[3], const double hor[3], const double ver[3], const double q[3], double& s, double& t, double& lambda)
{
    const double c0[3] = {hor[0], hor[1], hor[2]}, c1[3] = {ver[0], ver[1], ver[2]}, c2[3] = {-q[0], -q[1], -q[2]}, r[3] = {-A[0], -A[1], -A[2]};
    auto det3 = [](const double* a, const double* b, const double* c) {
        return a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]);
    };
    auto len3 = [](const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
    const double det = det3(c0, c1, c2), scale = len3(c0) * len3(c1) * len3(c2);
    if (!(fabs(det) > 1e-9 * scale)) return false;
    s = det3(r, c1, c2) / det;
    t = det3(c0, r, c2) / det;
    const double mu = det3(c0, c1, r) / det;
    if (!(mu > 0.0)) return false;
    lambda = 1.0 / mu;
    return isfinite(s) && isfinite(t) && isfinite(lambda);
}

}  // namespace cull_detail

// `root`: nodes[0] of the caller's BVH2, null or n_nodes == 0 when there is none (or its boxes are not known).
// `margin_pixels`: the pixel pitches every interval is widened by; 1 everywhere but in the test that shows the margin is needed.
inline CullBound cullBound(const trt_camera& cam, int W, int H, bool fixed, const trt_bvh_node* root, uint32_t n_nodes, double margin_pixels = 1.0)
{
    using namespace cull_detail;
    CullBound R{};
    R.active = false;
    R.row_lo = R.col_lo = 0; R.row_hi = R.col_hi = -1;
    auto off = [&](const char* why) { R.active = false; R.why = why; for (int k = 0; k < 8; ++k) R.v[k] = 0; return R; };
    if (!root || n_nodes == 0) return off("no inner node");
    if (W < 2 || H < 2) return off("image narrower than two pixels");
    double eye[3], A[3], hor[3], ver[3], S[3], lo[3], hi[3], Ssum = 0.0;
    for (int k = 0; k < 3; ++k) {
        eye[k] = cam.eye[k]; hor[k] = cam.horizontal[k]; ver[k] = cam.vertical[k];
        A[k] = double(cam.lower_left_corner[k]) - eye[k];
        S[k] = fabs(double(cam.lower_left_corner[k])) + 3.0 * fabs(hor[k]) + 3.0 * fabs(ver[k]) + fabs(eye[k]);
        Ssum += S[k];
        // (the slab test takes the two planes of an axis in either order: a box given with lo > hi is the box between them, not an empty one)
        lo[k] = fmin(fmin(double(root->lo0[k]), double(root->hi0[k])), fmin(double(root->lo1[k]), double(root->hi1[k])));
        hi[k] = fmax(fmax(double(root->lo0[k]), double(root->hi0[k])), fmax(double(root->lo1[k]), double(root->hi1[k])));
        // (fmin / fmax drop a NaN: look at all four)
        if (!isfinite(double(root->lo0[k])) || !isfinite(double(root->lo1[k])) || !isfinite(double(root->hi0[k])) || !isfinite(double(root->hi1[k])))
            return off("root boxes not finite");
        if (!isfinite(S[k])) return off("camera not finite");
    }
    const double e_max = ldexp(fmax(S[0], fmax(S[1], S[2])), -20);
    // lambda_max of the boxes as given, the padding from it, then the padded box
    double s_lo = 0, s_hi = 0, t_lo = 0, t_hi = 0, lam[2] = {0.0, 0.0};
    double pad[3] = {0.0, 0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass) {
        for (int c = 0; c < 8; ++c) {
            double q[3];
            for (int k = 0; k < 3; ++k) q[k] = ((c >> k & 1) ? hi[k] + pad[k] : lo[k] - pad[k]) - eye[k];
            double s, t, l;
            if (!project(A, hor, ver, q, s, t, l)) return off("a corner of the root boxes is not in front of the camera");
            if (c == 0) { s_lo = s_hi = s; t_lo = t_hi = t; }
            s_lo = fmin(s_lo, s); s_hi = fmax(s_hi, s); t_lo = fmin(t_lo, t); t_hi = fmax(t_hi, t);
            lam[pass] = fmax(lam[pass], l);
        }
        if (pass == 0)
            for (int k = 0; k < 3; ++k) pad[k] = 2.0 * lam[0] * e_max + ldexp(fmax(fabs(lo[k] - eye[k]), fabs(hi[k] - eye[k])), -21);
    }
    if (!(lam[1] <= 2.0 * lam[0])) return off("padding does not converge");
    const double pitch_s = 1.0 / double(W - 1.0), pitch_t = 1.0 / double(H - 1.0), fp = ldexp(1.0, -21);
    const double m_s = margin_pixels * pitch_s + fp, m_t = margin_pixels * pitch_t + fp;
    // the frame's (s, t) range
    double fs0, fs1, ft0, ft1, x0, x1;
    colS(W, fixed, 0, fs0, x1); colS(W, fixed, W - 1, x0, fs1);
    rowT(H, fixed, H - 1, ft0, x1); rowT(H, fixed, 0, x0, ft1);
    fs0 -= fabs(m_s); fs1 += fabs(m_s); ft0 -= fabs(m_t); ft1 += fabs(m_t);
    // The rectangle of the union's corners is valid but wide where a box reaches towards the camera beside the frame (a ceiling that starts
    // in front of the room: its near end lies above the frame and projects wider than anything in it).  Each of the two boxes is therefore
    // cut into CULL_SLICES slabs along the axis closest to the viewing direction, every slab (padded as the union is) is projected on its
    // own, and a slab whose rectangle misses the frame altogether — no ray of the frame can reach it — is left out of the union of rectangles.
    {
        constexpr int CULL_SLICES = 64;
        const double w[3] = {hor[1] * ver[2] - hor[2] * ver[1], hor[2] * ver[0] - hor[0] * ver[2], hor[0] * ver[1] - hor[1] * ver[0]};
        const int ax = fabs(w[0]) >= fabs(w[1]) ? (fabs(w[0]) >= fabs(w[2]) ? 0 : 2) : (fabs(w[1]) >= fabs(w[2]) ? 1 : 2);
        bool any = false;
        double rs0 = 0, rs1 = 0, rt0 = 0, rt1 = 0;
        for (int bx = 0; bx < 2; ++bx) {
            double blo[3], bhi[3];
            for (int k = 0; k < 3; ++k) {
                const double p0 = bx ? double(root->lo1[k]) : double(root->lo0[k]), p1 = bx ? double(root->hi1[k]) : double(root->hi0[k]);
                blo[k] = fmin(p0, p1); bhi[k] = fmax(p0, p1);
            }
            const double a0 = blo[ax], a1 = bhi[ax];
            for (int n = 0; n < CULL_SLICES; ++n) {
                blo[ax] = a0 + (a1 - a0) * (double(n) / CULL_SLICES);
                bhi[ax] = n + 1 == CULL_SLICES ? a1 : a0 + (a1 - a0) * (double(n + 1) / CULL_SLICES);
                double c_s0 = 0, c_s1 = 0, c_t0 = 0, c_t1 = 0;
                for (int c = 0; c < 8; ++c) {
                    double q[3], s, t, l;
                    for (int k = 0; k < 3; ++k) q[k] = ((c >> k & 1) ? bhi[k] + pad[k] : blo[k] - pad[k]) - eye[k];
                    if (!project(A, hor, ver, q, s, t, l)) return off("a corner of the root boxes is not in front of the camera");  // (inside the padded union: cannot happen)
                    if (c == 0) { c_s0 = c_s1 = s; c_t0 = c_t1 = t; }
                    c_s0 = fmin(c_s0, s); c_s1 = fmax(c_s1, s); c_t0 = fmin(c_t0, t); c_t1 = fmax(c_t1, t);
                }
                if (c_s1 < fs0 || c_s0 > fs1 || c_t1 < ft0 || c_t0 > ft1) continue;
                if (!any) { rs0 = c_s0; rs1 = c_s1; rt0 = c_t0; rt1 = c_t1; any = true; }
                rs0 = fmin(rs0, c_s0); rs1 = fmax(rs1, c_s1); rt0 = fmin(rt0, c_t0); rt1 = fmax(rt1, c_t1);
            }
        }
        if (any) { s_lo = rs0; s_hi = rs1; t_lo = rt0; t_hi = rt1; }
        else { s_lo = t_lo = 1.0; s_hi = t_hi = 0.0; }  // nothing of the boxes on the frame
    }
    int j_lo, j_hi, i_lo, i_hi;
    colsMeeting(W, fixed, m_s, s_lo, s_hi, j_lo, j_hi);
    rowsMeeting(H, fixed, m_t, t_lo, t_hi, i_lo, i_hi);
    if (!(s_lo <= s_hi) || j_lo > j_hi || i_lo > i_hi) { j_lo = W; j_hi = W - 1; i_lo = H; i_hi = H - 1; }  // the boxes lie off the frame: everything is outside
    struct Side { bool any; double s0, s1, t0, t1; } side[4];
    {
        double a, b;
        side[0] = {j_lo > 0, fs0, fs0, ft0, ft1};
        if (side[0].any) { colS(W, fixed, j_lo - 1, a, b); side[0].s1 = b + fabs(m_s); }
        side[1] = {j_hi < W - 1, fs1, fs1, ft0, ft1};
        if (side[1].any) { colS(W, fixed, j_hi + 1, a, b); side[1].s0 = a - fabs(m_s); }
        side[2] = {i_lo > 0, fs0, fs1, ft1, ft1};
        if (side[2].any) { rowT(H, fixed, i_lo - 1, a, b); side[2].t0 = a - fabs(m_t); }
        side[3] = {i_hi < H - 1, fs0, fs1, ft0, ft0};
        if (side[3].any) { rowT(H, fixed, i_hi + 1, a, b); side[3].t1 = b + fabs(m_t); }
    }
    for (int k = 0; k < 3; ++k) {
        const double g = fmax(ldexp(S[k], -20), ldexp(Ssum, -90));
        if (minAbsAffine(A[k], hor[k], ver[k], fs0, fs1, ft0, ft1) > g) continue;  // no zero of this component on the frame
        if (hor[k] == 0.0 && ver[k] != 0.0) {
            const double z0 = (-A[k] - g) / ver[k], z1 = (-A[k] + g) / ver[k];
            int a, b;
            rowsMeeting(H, fixed, m_t, fmin(z0, z1), fmax(z0, z1), a, b);
            if (a <= b) { if (R.row_lo > R.row_hi) { R.row_lo = a; R.row_hi = b; } else { R.row_lo = a < R.row_lo ? a : R.row_lo; R.row_hi = b > R.row_hi ? b : R.row_hi; } }
            continue;
        }
        if (ver[k] == 0.0 && hor[k] != 0.0) {
            const double z0 = (-A[k] - g) / hor[k], z1 = (-A[k] + g) / hor[k];
            int a, b;
            colsMeeting(W, fixed, m_s, fmin(z0, z1), fmax(z0, z1), a, b);
            if (a <= b) { if (R.col_lo > R.col_hi) { R.col_lo = a; R.col_hi = b; } else { R.col_lo = a < R.col_lo ? a : R.col_lo; R.col_hi = b > R.col_hi ? b : R.col_hi; } }
            continue;
        }
        for (const Side& sd : side)
            if (sd.any && !(minAbsAffine(A[k], hor[k], ver[k], sd.s0, sd.s1, sd.t0, sd.t1) > g)) return off("a slanted zero set of a direction component touches the culled area");
    }
    R.active = true;
    R.why = "";
    R.j_lo = j_lo; R.j_hi = j_hi; R.i_lo = i_lo; R.i_hi = i_hi;
    R.v[0] = j_lo; R.v[1] = W - 1 - j_hi; R.v[2] = i_lo; R.v[3] = H - 1 - i_hi;
    R.v[4] = R.row_lo > R.row_hi ? 0 : R.row_lo; R.v[5] = R.row_lo > R.row_hi ? 0 : R.row_hi - R.row_lo + 1;
    R.v[6] = R.col_lo > R.col_hi ? 0 : R.col_lo; R.v[7] = R.col_lo > R.col_hi ? 0 : R.col_hi - R.col_lo + 1;
    return R;
}

// the predicate of the kernels (pixelCulled, trt_path.h) on the host
inline bool cullBoundCulls(const CullBound& R, int W, int H, int i, int j)
{
    const bool out = j < R.v[0] || j >= W - R.v[1] || i < R.v[2] || i >= H - R.v[3];
    const bool band = (uint32_t)(i - R.v[4]) < (uint32_t)R.v[5] || (uint32_t)(j - R.v[6]) < (uint32_t)R.v[7];
    return out && !band;
}

}  // namespace trtd
