"""trt_reproject_motion and trt_trace_points (include/trt.h) for the tests, beside reproject_ref.py (whose names are used, not repeated):
  - cpu(): the CPU build of trt_rp_pixel_motion (tests/motion/libmotion_cpu.so), which the GPU must match bit for bit; project_point();
  - hit_points(): the CPU build of hitPoint, and hit_points_np(): its formula in numpy float32;
  - restate(): the motion contract in numpy float64 — reproject_ref.restate with steps 3 and 4 replaced by the given points;
  - pixel_points(): the point trt_rp_project forms for every pixel, in fp32 in its operations and order (the link between the two entries);
  - center_rays64(): step 3's rays in float64; displaced points and an object mask for the animated cases."""
import ctypes as C
import os

import numpy as np

import reproject_ref as R
from tinyraytracing_amd import _abi

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "motion", "libmotion_cpu.so")
fp = R.fp
NAN_BITS = 0x7FC00000
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.reproject_motion_cpu.argtypes = [C.POINTER(_abi.ReprojectParams), C.c_int, C.c_int] + [fp] * 14
        L.motion_cpu_project_point.argtypes = [C.POINTER(_abi.ReprojectParams), C.c_int, C.c_int, fp, fp]
        L.motion_cpu_hit_points.argtypes = [fp, C.c_uint32, C.POINTER(C.c_int32), fp, fp]
        L.motion_cpu_hit_points.restype = None
        _lib = L
    return _lib


def cpu(color, variance, albedo, normal, depth, prev_point, cur, prev=None, history=None, **kw):
    """The CPU build: dict(color, variance, cv, length) float32, T.reproject_motion's result."""
    bufs = [R._f32(color), R._f32(variance), R._f32(albedo), R._f32(normal), R._f32(depth), R._f32(prev_point)]
    bufs += [None] * 4 if history is None else [R._f32(history[k]) for k in R.HISTORY_KEYS]
    h, w = bufs[0].shape[:2]
    assert bufs[5].shape == (h, w, 3)
    out = {"color": np.empty((h, w, 3), np.float32), "variance": np.empty((h, w), np.float32), "cv": np.empty((h, w, 4), np.float32),
           "length": np.empty((h, w), np.float32)}
    p = R.params(cur, prev, **kw)
    rc = lib().reproject_motion_cpu(C.byref(p), w, h, *[R._ptr(b) for b in bufs], *[R._ptr(out[k]) for k in R.OUT_KEYS])
    assert rc == 0
    return out


def project_point(p, w, h, point):
    """Steps 3' and 4' of the CPU build for one point: (fx, fy, z') or None."""
    out = (C.c_float * 3)()
    rc = lib().motion_cpu_project_point(C.byref(p), w, h, R._ptr(R._f32(point)), out)
    assert rc >= 0
    return tuple(out) if rc else None


def hit_points(tri_v_other, tri, uv):
    """The CPU build of k_hit_points' arithmetic: float32 [n, 3]."""
    v, tri, uv = R._f32(tri_v_other), np.ascontiguousarray(tri, np.int32), R._f32(uv)
    out = np.empty((len(tri), 3), np.float32)
    lib().motion_cpu_hit_points(R._ptr(v), len(tri), tri.ctypes.data_as(C.POINTER(C.c_int32)), R._ptr(uv), R._ptr(out))
    return out


def hit_points_np(tri_v_other, tri, uv):
    """include/trt.h's formula in numpy float32, operation by operation: w = (1 - u) - v, point_k = (w a_k + u b_k) + v c_k; a miss is NaN with
    the bits 0x7FC00000."""
    f = np.float32
    v9 = np.asarray(tri_v_other, f)[np.maximum(tri, 0)]
    u, v = uv[:, 0:1].astype(f), uv[:, 1:2].astype(f)
    w = (f(1.0) - u) - v
    p = ((w * v9[:, 0] + u * v9[:, 1]) + v * v9[:, 2]).astype(f)
    out = np.where((tri >= 0)[:, None], p.view(np.uint32), np.uint32(NAN_BITS)).astype(np.uint32)
    return out.view(f)


def pixel_points(cam, w, h, depth, flags):
    """P_k = cur.eye_k + (d_k / dl) * depth of trt_rp_project, fp32 in its order (numpy's float32 +, *, / and sqrt round as the C code's)."""
    f = np.float32
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    with np.errstate(all="ignore"):
        if flags & R.FIXED:
            s = (x.astype(f) + f(0.5)) / f(w)
            t = ((h - 1 - y).astype(f) + f(0.5)) / f(h)
        else:
            s = x.astype(f) / (f(w) - f(1.0))
            t = (h - y).astype(f) / (f(h) - f(1.0))
        eye, llc, hor, ver = (np.array(list(getattr(cam, k)), f) for k in ("eye", "lower_left_corner", "horizontal", "vertical"))
        d = ((llc + hor * s[..., None]) + ver * t[..., None]) - eye
        dl = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        return (eye + (d / dl[..., None]) * np.asarray(depth, f)[..., None]).astype(f)


def center_rays64(cam, w, h, flags):
    """Step 3's rays in float64: (eye [3], dir [h * w, 3] unnormalised)."""
    eye, llc, hor, ver = R.camera_arrays(cam)
    s, t = R.pixel_grid(w, h, flags & R.FIXED)
    with np.errstate(all="ignore"):
        return eye, (llc + s[..., None] * hor + t[..., None] * ver - eye).reshape(h * w, 3)


def smooth_field_points(cam, w, h, depth, flags, seed, footprints=3.0):
    """The moved-camera points of `cam` displaced per pixel by a smooth field of up to `footprints` pixel footprints at the pixel's depth,
    along the camera's image axes.  float32 [h, w, 3]; misses (depth >= TRT_INF) become NaN."""
    eye, d = center_rays64(cam, w, h, flags)
    _, llc, hor, ver = R.camera_arrays(cam)
    z = np.asarray(depth, np.float64)
    with np.errstate(all="ignore"):
        dn = d.reshape(h, w, 3) / np.linalg.norm(d.reshape(h, w, 3), axis=2, keepdims=True)
        P = eye + z[..., None] * dn
        axis = np.cross(hor, ver)
        focal = abs(np.dot(llc - eye, axis)) / np.linalg.norm(axis)  # the image plane's distance from the eye
        foot = z / focal * np.linalg.norm(hor) / max(w, 2)  # one pixel step at this depth, roughly
        rng = np.random.default_rng(seed + 991)
        ph = rng.uniform(0.0, 2 * np.pi, 4)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        ax = np.sin(xx * 0.21 + yy * 0.13 + ph[0]) * np.cos(yy * 0.17 + ph[1])
        ay = np.cos(xx * 0.11 - yy * 0.19 + ph[2]) * np.sin(xx * 0.15 + ph[3])
        P = P + (footprints * foot * ax)[..., None] * (hor / np.linalg.norm(hor)) + (footprints * foot * ay)[..., None] * (ver / np.linalg.norm(ver))
    P = np.where((z < R.INF)[..., None], P, np.nan)
    return P.astype(np.float32)


def restate(color, variance, albedo, normal, depth, prev_point, cur, prev=None, history=None, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9,
            max_history=255.0, flags=0):
    """The motion contract in float64: reproject_ref.restate's steps 1, 2, 5, 6 and 7 (written out again here: that function takes no
    points), steps 3' and 4' from prev_point.  `cur` is not used; byte-identical cameras are no special case.  -> dict(color, variance, cv,
    length) float64 and edge [h, w] as reproject_ref.restate flags it."""
    EDGE, MIN_WEIGHT, INF, LUMA = R.EDGE, R.MIN_WEIGHT, R.INF, R.LUMA
    color, albedo, normal = (np.asarray(x, np.float64) for x in (color, albedo, normal))
    variance, z, P = np.asarray(variance, np.float64), np.asarray(depth, np.float64), np.asarray(prev_point, np.float64)
    alpha, depth_tolerance = alpha or R.DEFAULTS["alpha"], depth_tolerance or R.DEFAULTS["depth_tolerance"]
    normal_threshold, max_history = normal_threshold or R.DEFAULTS["normal_threshold"], max_history or R.DEFAULTS["max_history"]
    h, w = z.shape
    prev = cur if prev is None else prev
    a = np.where(albedo > 0, albedo, 1.0)
    m2 = np.maximum(a @ LUMA, 1e-6) ** 2
    c = color / a
    var = variance / m2
    out = {"color": color.copy(), "variance": variance.copy(), "cv": np.concatenate([c, var[..., None]], axis=2), "length": np.ones((h, w))}
    edge = np.zeros((h, w), bool)
    out["edge"] = edge
    if history is None:
        return out
    pcv, plen, pn, pz = (np.asarray(history[k], np.float64) for k in R.HISTORY_KEYS)
    hit = z < INF
    with np.errstate(all="ignore"):
        # 3'. / 4'. the given point in the previous image
        peye, pllc, phor, pver = R.camera_arrays(prev)
        v = P - peye
        finite = np.isfinite(v).all(axis=2)
        M = np.stack([pllc - peye, phor, pver], axis=1)
        if np.isfinite(M).all() and np.linalg.det(M) != 0.0:
            sol = np.where(finite[..., None], v, np.nan) @ np.linalg.inv(M).T
        else:
            sol = np.full((h, w, 3), np.nan)
        k = sol[..., 0]
        sp, tp = sol[..., 1] / k, sol[..., 2] / k
        if flags & R.FIXED:
            fx, fy = sp * w - 0.5, (h - 1 + 0.5) - tp * h
        else:
            fx, fy = sp * (w - 1.0), h - tp * (h - 1.0)
        zp = np.linalg.norm(v, axis=2)
        # 1.8e19 = sqrt(FLT_MAX): beyond it |v|^2 is not finite in fp32, z' = sqrt(inf), and the contract gives such a point no history
        ok = hit & finite & (k > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h) & (zp < 1.8e19)
        edge |= ok & ((np.abs(fx - np.rint(fx)) < EDGE) | (np.abs(fy - np.rint(fy)) < EDGE))
        fx, fy, zp = (np.where(ok, q, 0.0) for q in (fx, fy, zp))
        # 5. taps
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        wx, wy = fx - x0, fy - y0
        ws, sc, sl = np.zeros((h, w)), np.zeros((h, w, 4)), np.zeros((h, w))
        n2 = np.sum(normal * normal, axis=2)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                wt = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
                cand = ok & (wt > 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                zq, nq = pz[qy, qx], pn[qy, qx]
                cand &= zq < INF
                dz, bound = np.abs(zp - zq), depth_tolerance * zp
                dn = np.sum(normal * nq, axis=2)
                lhs, rhs = dn * dn, normal_threshold ** 2 * n2 * np.sum(nq * nq, axis=2)
                edge |= cand & (np.abs(dz - bound) <= EDGE * bound)
                edge |= cand & (dz <= bound) & ((np.abs(lhs - rhs) <= EDGE * rhs) | (np.abs(dn) <= EDGE * np.sqrt(rhs)))
                good = cand & (dz <= bound) & (dn > 0) & (lhs >= rhs)
                wt = np.where(good, wt, 0.0)
                ws += wt
                sc += wt[..., None] * np.where(good[..., None], pcv[qy, qx], 0.0)
                sl += wt * np.where(good, plen[qy, qx], 0.0)
        edge |= ok & (np.abs(ws - MIN_WEIGHT) <= EDGE)
        found = ok & (ws >= MIN_WEIGHT)
        wsafe = np.where(found, ws, 1.0)
        ch, nh = sc / wsafe[..., None], sl / wsafe
        # 6. blend
        n = np.minimum(nh + 1.0, max_history)
        edge |= found & (np.abs(1.0 / n - alpha) <= EDGE)
        al = np.maximum(alpha, 1.0 / n)
        cb = ch[..., :3] + al[..., None] * (c - ch[..., :3])
        vb = al ** 2 * var + (1.0 - al) ** 2 * ch[..., 3]
    f3 = found[..., None]
    out["cv"] = np.where(f3, np.concatenate([cb, vb[..., None]], axis=2), out["cv"])
    out["length"] = np.where(found, n, 1.0)
    out["color"] = np.where(f3, cb * a, color)
    out["variance"] = np.where(found, vb * m2, variance)
    out["fx"], out["fy"] = fx, fy
    return out


def moved_object(scene, delta):
    """back: the inner object (refit_ref.move_inner_object's selection) translated by `delta`, not rotated.  -> (vertices, mask)."""
    import refit_ref
    return refit_ref.move_inner_object(scene, delta=delta, rotate_deg=0.0)


def project64(points, prev, w, h, flags):
    """Steps 3' and 4' in float64 for points [h, w, 3]: (fx, fy), NaN where there is no place in the previous image."""
    peye, pllc, phor, pver = R.camera_arrays(prev)
    with np.errstate(all="ignore"):
        sol = (np.asarray(points, np.float64) - peye) @ np.linalg.inv(np.stack([pllc - peye, phor, pver], axis=1)).T
        k = np.where(sol[..., 0] > 0, sol[..., 0], np.nan)
        sp, tp = sol[..., 1] / k, sol[..., 2] / k
        if flags & R.FIXED:
            return sp * w - 0.5, (h - 1 + 0.5) - tp * h
        return sp * (w - 1.0), h - tp * (h - 1.0)


def features(org, dirs, t, tri, tri_v, w, h):
    """Feature buffers of centre rays from their closest hits, in numpy: depth = t |dir| (TRT_INF on a miss) and the triangle's geometric
    normal turned towards the eye (0 on a miss).  -> (normal [h, w, 3], depth [h, w]) float32."""
    hit = tri >= 0
    v = np.asarray(tri_v, np.float64)[np.maximum(tri, 0)]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    n = np.where((np.sum(n * dirs, axis=1) > 0)[:, None], -n, n)
    depth = np.where(hit, t.astype(np.float64) * np.linalg.norm(dirs.astype(np.float64), axis=1), R.INF)
    return R._f32(np.where(hit[:, None], n, 0.0).reshape(h, w, 3)), R._f32(depth.reshape(h, w))


def follow_case(trace_closest, trace_points, update, reproject_motion, reproject, scene, w, h, v1, sel, center_rays):
    """`History follows the surface' (tests/test_gpu_motion.py), with the entries under test handed in so that the oracle and the CPU build
    can stand in for them: frame 0 on the scene's vertices v0, update(v1), frame 1; prev_cv.rgb = frame 0's centre-hit positions.
    -> dict of what the test asserts on."""
    import tinyraytracing_amd as T
    flags = R.FIXED
    cam = T.Camera.from_buffer_copy(scene.flat.contents.camera)
    v0 = scene.arrays()["tri_v"]
    org, dirs = center_rays(cam, w, h, flags)
    t0, tri0, uv0 = trace_closest(org, dirs)
    S = hit_points_np(v0, tri0, uv0).reshape(h, w, 3)  # the position buffer: what frame 0 saw, where
    n0, z0 = features(org, dirs, t0, tri0, v0, w, h)
    update(v1)
    t1, tri1, uv1 = trace_closest(org, dirs)
    n1, z1 = features(org, dirs, t1, tri1, v1, w, h)
    P = trace_points(org, dirs, v0).reshape(h, w, 3)
    hist = {"cv": R._f32(np.concatenate([np.nan_to_num(S), np.zeros((h, w, 1))], axis=2)), "length": np.full((h, w), 1000.0, np.float32), "normal": n0, "depth": z0}
    cur = (np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.ones((h, w, 3), np.float32), n1, z1)
    kw = dict(alpha=1e-6, max_history=1e6, flags=flags)
    out = {"motion": reproject_motion(*cur, P, cam, cam, history=hist, **kw), "still": reproject(*cur, cam, cam, history=hist, **kw)}
    # where the history comes from, by the float64 projection of the points, and whether its four taps lie on one triangle of frame 0
    fx, fy = project64(P, cam, w, h, flags)
    ok = np.isfinite(fx) & np.isfinite(fy) & (fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1)
    x0, y0 = np.where(ok, np.floor(fx), 0).astype(int), np.where(ok, np.floor(fy), 0).astype(int)
    T0 = tri0.reshape(h, w)
    taps = [T0[y0, x0], T0[y0, x0 + 1], T0[y0 + 1, x0], T0[y0 + 1, x0 + 1]]
    one_tri = ok & (taps[0] >= 0) & (taps[0] == taps[1]) & (taps[0] == taps[2]) & (taps[0] == taps[3])
    d = lambda a, b: np.linalg.norm(a.astype(np.float64) - b.astype(np.float64), axis=-1)  # noqa: E731
    a, b, c, e = S[y0, x0], S[y0, x0 + 1], S[y0 + 1, x0], S[y0 + 1, x0 + 1]
    with np.errstate(all="ignore"):
        spread = np.max([d(a, b), d(c, e), d(a, c), d(b, e)], axis=0)  # the largest distance between neighbouring stored positions
    res = {"object": (sel[np.maximum(tri0, 0)] & (tri0 >= 0) & sel[np.maximum(tri1, 0)] & (tri1 >= 0)).reshape(h, w), "tol": 2.0 * spread, "P": P}
    for k, o in out.items():
        n = o["length"].astype(np.float64)
        with np.errstate(all="ignore"):
            mean = o["cv"][..., :3].astype(np.float64) / (1.0 - 1.0 / n)[..., None]
            res[k + "_err"] = np.linalg.norm(mean - P.astype(np.float64), axis=2)
        res[k + "_found"] = n > 1
    res["qualify"] = res["motion_found"] & one_tri
    return res
