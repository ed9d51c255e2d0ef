"""trt_reproject (include/trt.h) twice over, for the tests:
  - cpu(): the CPU build of the kernel's per-pixel code (tests/reproject/libreproject_cpu.so from tinyraytracing_amd/csrc/trt_reproject.h),
    which the GPU must match bit for bit, and its building blocks (project, tap_ok, blend);
  - restate(): the contract of include/trt.h written out again in numpy float64, independently of that code, with a per-pixel flag
    "a decision sits on its edge" for the pixels where fp32 and float64 may legitimately decide differently.
And inputs for them: random frames with a history that partly passes the tests, cameras orbiting the shipped scenes, a fronto-parallel
plane with analytic depths."""
import ctypes as C
import os

import numpy as np

import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reproject", "libreproject_cpu.so")
fp = C.POINTER(C.c_float)
LUMA = np.array([0.2126, 0.7152, 0.0722])
INF = float(np.float32(_abi.TRT_INF))
FIXED = _abi.TRT_FLAG_FIXED_PIXELS
EDGE = 1e-3
MIN_WEIGHT = 0.01
DEFAULTS = dict(alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9, max_history=255.0)
OUT_KEYS = ("color", "variance", "cv", "length")
HISTORY_KEYS = ("cv", "length", "normal", "depth")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.reproject_cpu.argtypes = [C.POINTER(_abi.ReprojectParams), C.c_int, C.c_int] + [fp] * 13
        L.reproject_cpu_project.argtypes = [C.POINTER(_abi.ReprojectParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, fp]
        L.reproject_cpu_tap_ok.argtypes = [C.POINTER(_abi.ReprojectParams), C.c_float, fp, C.c_float, fp]
        L.reproject_cpu_blend.argtypes = [C.POINTER(_abi.ReprojectParams), fp, fp, C.c_float, fp]
        _lib = L
    return _lib


def params(cur=None, prev=None, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9, max_history=255.0, flags=0):
    p = _abi.ReprojectParams()
    if cur is not None:
        p.cur = cur
        p.prev = cur if prev is None else prev
    p.alpha, p.depth_tolerance, p.normal_threshold, p.max_history, p.flags = alpha, depth_tolerance, normal_threshold, max_history, flags
    return p


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(fp)


def cpu(color, variance, albedo, normal, depth, cur, prev=None, history=None, **kw):
    """The CPU build: dict(color [h, w, 3], variance [h, w], cv [h, w, 4], length [h, w]) float32, T.reproject's result."""
    bufs = [_f32(color), _f32(variance), _f32(albedo), _f32(normal), _f32(depth)]
    bufs += [None] * 4 if history is None else [_f32(history[k]) for k in HISTORY_KEYS]
    h, w = bufs[0].shape[:2]
    out = {"color": np.empty((h, w, 3), np.float32), "variance": np.empty((h, w), np.float32), "cv": np.empty((h, w, 4), np.float32),
           "length": np.empty((h, w), np.float32)}
    p = params(cur, prev, **kw)
    rc = lib().reproject_cpu(C.byref(p), w, h, *[_ptr(b) for b in bufs], *[_ptr(out[k]) for k in OUT_KEYS])
    assert rc == 0
    return out


def project(p, w, h, x, y, depth):
    """Steps 3 and 4 of the CPU build for one pixel: (fx, fy, z') or None."""
    out = (C.c_float * 3)()
    rc = lib().reproject_cpu_project(C.byref(p), w, h, x, y, depth, out)
    assert rc >= 0
    return tuple(out) if rc else None


def tap_ok(p, zp, n_p, zq, n_q):
    rc = lib().reproject_cpu_tap_ok(C.byref(p), zp, _ptr(_f32(n_p)), zq, _ptr(_f32(n_q)))
    assert rc >= 0
    return bool(rc)


def blend(p, c4, h4, n_h):
    """Step 6 of the CPU build: (cv' [4], N)."""
    out = (C.c_float * 5)()
    assert lib().reproject_cpu_blend(C.byref(p), _ptr(_f32(c4)), _ptr(_f32(h4)), n_h, out) == 0
    return np.array(out[:4], np.float32), float(out[4])


def camera_arrays(cam):
    """(eye, llc, horizontal, vertical) of a Camera as float64 vectors"""
    return tuple(np.array(list(getattr(cam, k)), np.float64) for k in ("eye", "lower_left_corner", "horizontal", "vertical"))


def pixel_grid(w, h, fixed):
    """(s, t) [h, w] of the pixel centres: step 3 of the contract"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        if fixed:
            return (x + 0.5) / w, (h - 1 - y + 0.5) / h
        return x / (w - 1.0), (h - y) / (h - 1.0)


def restate(color, variance, albedo, normal, depth, cur, prev=None, history=None, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9,
            max_history=255.0, flags=0):
    """include/trt.h's contract in float64.  -> dict(color, variance, cv, length) float64 and edge: bool [h, w], set where a decision of the
    pixel sits within EDGE of its threshold (fx or fy near an integer, a depth or normal test near its bound, W_s near 0.01, 1/N near alpha).
    With byte-identical cameras fx = x and fy = y by definition, not by arithmetic, and are not flagged."""
    color, albedo, normal = (np.asarray(x, np.float64) for x in (color, albedo, normal))
    variance, z = np.asarray(variance, np.float64), np.asarray(depth, np.float64)
    alpha, depth_tolerance = alpha or DEFAULTS["alpha"], depth_tolerance or DEFAULTS["depth_tolerance"]
    normal_threshold, max_history = normal_threshold or DEFAULTS["normal_threshold"], max_history or DEFAULTS["max_history"]
    h, w = z.shape
    prev = cur if prev is None else prev
    # 1. demodulate
    a = np.where(albedo > 0, albedo, 1.0)
    m2 = np.maximum(a @ LUMA, 1e-6) ** 2
    c = color / a
    var = variance / m2
    out = {"color": color.copy(), "variance": variance.copy(), "cv": np.concatenate([c, var[..., None]], axis=2), "length": np.ones((h, w))}
    edge = np.zeros((h, w), bool)
    out["edge"] = edge
    if history is None:
        return out
    pcv, plen, pn, pz = (np.asarray(history[k], np.float64) for k in HISTORY_KEYS)
    hit = z < INF
    with np.errstate(all="ignore"):
        # 3. / 4. world point, previous image
        if bytes(cur) == bytes(prev):
            fx, fy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
            zp, ok = z.copy(), hit.copy()
        else:
            eye, llc, hor, ver = camera_arrays(cur)
            peye, pllc, phor, pver = camera_arrays(prev)
            s, t = pixel_grid(w, h, flags & FIXED)
            d = llc + s[..., None] * hor + t[..., None] * ver - eye
            d = d / np.linalg.norm(d, axis=2, keepdims=True)
            v = eye + z[..., None] * d - peye
            M = np.stack([pllc - peye, phor, pver], axis=1)
            if np.isfinite(M).all() and np.linalg.det(M) != 0.0:
                sol = np.where(np.isfinite(v).all(axis=2)[..., None], v, np.nan) @ np.linalg.inv(M).T
            else:
                sol = np.full((h, w, 3), np.nan)
            k = sol[..., 0]
            sp, tp = sol[..., 1] / k, sol[..., 2] / k
            if flags & FIXED:
                fx, fy = sp * w - 0.5, (h - 1 + 0.5) - tp * h
            else:
                fx, fy = sp * (w - 1.0), h - tp * (h - 1.0)
            zp = np.linalg.norm(v, axis=2)
            ok = hit & (k > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
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
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def random_frames(h, w, seed, miss_frac=0.1):
    """A current frame (denoise_ref.random_inputs) and a history whose feature buffers are the frame's own, disturbed so that a part of
    the taps fails each test (history lengths are not whole numbers, which would put 1 / N on alpha = 0.2 in every eleventh pixel): depths off by up to 15 %, normals tilted by up to about 35 degrees, a few previous misses.
    -> ((color, variance, albedo, normal, depth), history dict), float32."""
    import denoise_ref as D
    cur = D.random_inputs(h, w, seed, miss_frac=miss_frac)
    rng = np.random.default_rng(seed + 77)
    normal, depth = cur[3].astype(np.float64), cur[4].astype(np.float64)
    pz = np.where(depth < INF, depth * (1.0 + rng.uniform(-0.15, 0.15, size=(h, w))), INF)
    pz[rng.random((h, w)) < 0.05] = INF
    pn = normal + rng.normal(scale=0.25, size=(h, w, 3)) * np.linalg.norm(normal, axis=2, keepdims=True)
    pn[pz >= INF] = 0.0
    hist = {"cv": np.concatenate([rng.uniform(0.0, 1.0, size=(h, w, 3)), rng.uniform(1e-4, 5e-3, size=(h, w, 1))], axis=2),
            "length": rng.uniform(1.0, 12.0, size=(h, w)), "normal": pn, "depth": pz}
    return cur, {k: _f32(v) for k, v in hist.items()}


def nearby_cameras(w, h, seed):
    """Two look_at cameras a few degrees and a few percent of the scene size (depths of random_frames: 2 .. 50) apart."""
    rng = np.random.default_rng(seed)
    eye = np.array([0.5, 1.0, 6.0]) + rng.uniform(-0.5, 0.5, 3)
    target = rng.uniform(-0.5, 0.5, 3)
    fov = rng.uniform(35.0, 60.0)
    cur = T.look_at(eye, target, (0.0, 1.0, 0.0), fov, w, h)
    prev = T.look_at(eye + rng.uniform(-0.15, 0.15, 3), target + rng.uniform(-0.2, 0.2, 3), (rng.uniform(-0.03, 0.03), 1.0, 0.0), fov, w, h)
    return cur, prev


# eye, the point the eye orbits (on the camera's axis, inside the scene), fovy: the shipped scenes' own views
VIEWS = {"staircase": ((6.9118194580078125, 1.6516278982162476, 2.5541365146636963), (2.328019380569458, 1.6516276597976685, 0.33640459179878235), 42.9957),
         "back": ((278.0, 273.0, -800.0), (278.0, 273.0, 280.0), 39.3077),
         "veach-mis": ((28.2792, 5.2, 1.23612e-06), (0.0, 2.8, 0.0), 20.1143)}


def orbit_camera(name, degrees, w, h):
    """The scene's own view with the eye turned by `degrees` about the vertical axis through the point it looks at."""
    eye, target, fov = VIEWS[name]
    eye, target = np.array(eye), np.array(target)
    a = np.radians(degrees)
    r = eye - target
    r = np.array([np.cos(a) * r[0] + np.sin(a) * r[2], r[1], -np.sin(a) * r[0] + np.cos(a) * r[2]])
    return T.look_at(target + r, target, (0.0, 1.0, 0.0), fov, w, h)


def plane_camera(ex, ey, w, h, vw=1.2):
    """A camera at (ex, ey, 0) looking down -z: viewport vw x vw h / w at distance 1, axes along x and y."""
    vh = vw * h / w
    cam = _abi.Camera()
    for name, a in (("eye", (ex, ey, 0.0)), ("lower_left_corner", (ex - vw / 2, ey - vh / 2, -1.0)), ("horizontal", (vw, 0.0, 0.0)), ("vertical", (0.0, vh, 0.0))):
        setattr(cam, name, _abi.c_float3(*[float(np.float32(x)) for x in a]))
    return cam


def plane_depth(w, h, dist, fixed, vw=1.2):
    """The depth buffer plane_camera sees of the plane z = -dist: the distance along the unit ray through each pixel centre (the same
    for every eye position, the plane being parallel to the image)."""
    s, t = pixel_grid(w, h, fixed)
    vh = vw * h / w
    d = np.stack([(s - 0.5) * vw, (t - 0.5) * vh, -np.ones_like(s)], axis=2)
    return _f32(dist * np.linalg.norm(d, axis=2))


def pixel_footprint(w, h, dist, fixed, vw=1.2):
    """The size (x, y) of one pixel step on the plane z = -dist"""
    vh = vw * h / w
    return (vw * dist / w, vh * dist / h) if fixed else (vw * dist / (w - 1), vh * dist / (h - 1))
