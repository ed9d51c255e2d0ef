"""trt_reproject_moments (include/trt.h) twice over, for the tests, beside reproject_ref.py and motion_ref.py (whose names are used):
  - cpu(): the CPU build of the kernels' per-pixel code (tests/moments/libmoments_cpu.so from tinyraytracing_amd/csrc/trt_moments.h), which
    the GPU must match bit for bit;
  - restate(): the contract written out again in numpy float64, both stages, with a per-pixel flag "a decision sits on its edge" (the tap
    tests as reproject_ref flags them, the route predicate, the two 1 - sum-of-squares guards);
  - inputs: random frames whose planes have unit normals (so that stage B's windows hold more than their centre), a history with moments,
    and the flat-plane sequence of the derived estimates."""
import ctypes as C
import os

import numpy as np

import reproject_ref as R
from tinyraytracing_amd import _abi

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "moments", "libmoments_cpu.so")
fp = R.fp
MIN_DOF = 0.1
RADIUS = 3
HISTORY_KEYS = R.HISTORY_KEYS + ("mom",)
OUT_KEYS = R.OUT_KEYS + ("mom",)
DEFAULTS = dict(R.DEFAULTS, min_frames=4, sigma_normal=128, sigma_depth=1.0)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.reproject_moments_cpu.argtypes = [C.POINTER(_abi.MomentsParams), C.c_int, C.c_int] + [fp] * 15
        L.moments_cpu_defaults.argtypes = [C.POINTER(_abi.MomentsParams), fp]
        _lib = L
    return _lib


def params(cur=None, prev=None, min_frames=4, sigma_normal=128, sigma_depth=1.0, **kw):
    p = _abi.MomentsParams()
    p.rp = R.params(cur, prev, **kw)
    p.min_frames, p.sigma_normal, p.sigma_depth = min_frames, sigma_normal, sigma_depth
    return p


def empty_outputs(h, w):
    return {"color": np.empty((h, w, 3), np.float32), "variance": np.empty((h, w), np.float32), "cv": np.empty((h, w, 4), np.float32),
            "length": np.empty((h, w), np.float32), "mom": np.empty((h, w, 4), np.float32)}


def cpu(color, albedo, normal, depth, cur, prev=None, history=None, prev_point=None, **kw):
    """The CPU build: dict(color, variance, cv, length, mom) float32, T.reproject_moments' result."""
    bufs = [R._f32(color), R._f32(albedo), R._f32(normal), R._f32(depth), None if prev_point is None else R._f32(prev_point)]
    bufs += [None] * 5 if history is None else [R._f32(history[k]) for k in HISTORY_KEYS]
    h, w = bufs[0].shape[:2]
    out = empty_outputs(h, w)
    p = params(cur, prev, **kw)
    rc = lib().reproject_moments_cpu(C.byref(p), w, h, *[R._ptr(b) for b in bufs], *[R._ptr(out[k]) for k in OUT_KEYS])
    assert rc == 0
    return out


def next_history(out, normal, depth):
    return {"cv": out["cv"], "length": out["length"], "normal": R._f32(normal), "depth": R._f32(depth), "mom": out["mom"]}


def depth_gradient(z, hit):
    """trt_denoise's step 2: per axis the smaller |z_q - z_p| over the axis neighbours that are in-image hits (0 if none); the larger axis."""
    h, w = z.shape

    def axis(ax):
        best = np.full((h, w), np.inf)
        for sh in (1, -1):
            zq, hq = np.roll(z, sh, axis=ax), np.roll(hit, sh, axis=ax)
            idx = np.arange(z.shape[ax])
            valid = (idx - sh >= 0) & (idx - sh < z.shape[ax])
            valid = valid[:, None] if ax == 0 else valid[None, :]
            with np.errstate(all="ignore"):
                d = np.where(hq & valid, np.abs(zq - z), np.inf)
            best = np.minimum(best, d)
        return np.where(np.isfinite(best), best, 0.0)

    return np.maximum(axis(1), axis(0))


def spatial(mom, length, normal, depth, min_frames=4, sigma_normal=128, sigma_depth=1.0):
    """Stage B in float64 on the given stage-A records.  -> (var' [h, w], NaN where stage B does not run; edge [h, w])."""
    mom, n, z = np.asarray(mom, np.float64), np.asarray(normal, np.float64), np.asarray(depth, np.float64)
    length = np.asarray(length, np.float64)
    h, w = z.shape
    hit = z < R.INF
    with np.errstate(all="ignore"):
        dof_t = 1.0 - mom[..., 2]
        temporal = hit & (length >= min_frames) & (dof_t >= MIN_DOF)
        edge = hit & ((np.abs(length - min_frames) <= R.EDGE) | (np.abs(dof_t - MIN_DOF) <= R.EDGE))
        gz = depth_gradient(np.where(hit, z, 0.0), hit)
        s1, s2, sw2, ws = (np.zeros((h, w)) for _ in range(4))
        yy, xx = np.mgrid[0:h, 0:w]
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                qy, qx = yy + dy, xx + dx
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                if dx == 0 and dy == 0:
                    wt = np.ones((h, w))
                else:
                    dn = np.maximum(np.sum(n * n[qy, qx], axis=2), 0.0)
                    den = sigma_depth * gz * np.sqrt(dx * dx + dy * dy) + 1e-3 * z
                    wz = np.exp(-np.abs(z - z[qy, qx]) / den)
                    wt = np.where(inside & hit[qy, qx], dn ** sigma_normal * np.nan_to_num(wz), 0.0)
                wt = np.where(hit, wt, 0.0)
                mq = mom[qy, qx]
                s1 += wt * np.where(wt > 0, mq[..., 0], 0.0)
                s2 += wt * np.where(wt > 0, mq[..., 1], 0.0)
                sw2 += wt * wt * np.where(wt > 0, mq[..., 2], 0.0)
                ws += wt
        wsafe = np.where(ws > 0, ws, 1.0)
        M1, M2, dof = s1 / wsafe, s2 / wsafe, 1.0 - sw2 / (wsafe * wsafe)
        edge |= hit & ~temporal & (np.abs(dof - MIN_DOF) <= R.EDGE)
        v = np.where(dof >= MIN_DOF, np.maximum(M2 - M1 * M1, 0.0) / np.where(dof >= MIN_DOF, dof, 1.0), M1 * M1)
        var = np.where(hit & ~temporal, v * mom[..., 2], np.nan)
    return var, edge


def restate(color, albedo, normal, depth, cur, prev=None, history=None, prev_point=None, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9,
            max_history=255.0, flags=0, min_frames=4, sigma_normal=128, sigma_depth=1.0, stage_a=None):
    """The contract in float64.  -> dict(color, variance, cv, length, mom) float64, edge [h, w] bool, temporal [h, w] bool.
    stage_a: None, or (mom, length) float32 as a build under test returned them: stage B is then restated on THOSE records, so that a
    neighbour whose own decisions sit on an edge does not take its whole window out of the comparison (stage A is compared on its own)."""
    color, albedo, normal = (np.asarray(x, np.float64) for x in (color, albedo, normal))
    z = np.asarray(depth, np.float64)
    alpha, depth_tolerance = alpha or DEFAULTS["alpha"], depth_tolerance or DEFAULTS["depth_tolerance"]
    normal_threshold, max_history = normal_threshold or DEFAULTS["normal_threshold"], max_history or DEFAULTS["max_history"]
    min_frames, sigma_normal, sigma_depth = min_frames or 4, sigma_normal or 128, sigma_depth or 1.0
    h, w = z.shape
    prev = cur if prev is None else prev
    INF, EDGE = R.INF, R.EDGE
    a = np.where(albedo > 0, albedo, 1.0)
    m2a = np.maximum(a @ R.LUMA, 1e-6) ** 2
    c = color / a
    l = c @ R.LUMA
    hit = z < INF
    cv3, length = c.copy(), np.ones((h, w))
    mom = np.stack([l, l * l, np.ones((h, w)), np.zeros((h, w))], axis=2)
    out_color = color.copy()
    edge = np.zeros((h, w), bool)
    if history is not None:
        pcv, plen, pn, pz, pmom = (np.asarray(history[k], np.float64) for k in HISTORY_KEYS)
        with np.errstate(all="ignore"):
            peye, pllc, phor, pver = R.camera_arrays(prev)
            if prev_point is None and bytes(cur) == bytes(prev):
                fx, fy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
                zp, ok = z.copy(), hit.copy()
            else:
                if prev_point is None:
                    eye, llc, hor, ver = R.camera_arrays(cur)
                    s, t = R.pixel_grid(w, h, flags & R.FIXED)
                    d = llc + s[..., None] * hor + t[..., None] * ver - eye
                    v = eye + z[..., None] * (d / np.linalg.norm(d, axis=2, keepdims=True)) - peye
                else:
                    v = np.asarray(prev_point, np.float64) - peye
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
                ok = hit & finite & (k > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h) & (zp < 1.8e19)
                edge |= ok & ((np.abs(fx - np.rint(fx)) < EDGE) | (np.abs(fy - np.rint(fy)) < EDGE))
            fx, fy, zp = (np.where(ok, q, 0.0) for q in (fx, fy, zp))
            x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
            wx, wy = fx - x0, fy - y0
            ws, sc, sl, sm = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w, 3))
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
                    sc += wt[..., None] * np.where(good[..., None], pcv[qy, qx][..., :3], 0.0)
                    sl += wt * np.where(good, plen[qy, qx], 0.0)
                    sm += wt[..., None] * np.where(good[..., None], pmom[qy, qx][..., :3], 0.0)
            edge |= ok & (np.abs(ws - R.MIN_WEIGHT) <= EDGE)
            found = ok & (ws >= R.MIN_WEIGHT)
            wsafe = np.where(found, ws, 1.0)
            ch, nh, mh = sc / wsafe[..., None], sl / wsafe, sm / wsafe[..., None]
            n = np.minimum(nh + 1.0, max_history)
            edge |= found & (np.abs(1.0 / n - alpha) <= EDGE)
            al = np.maximum(alpha, 1.0 / n)
            cb = ch + al[..., None] * (c - ch)
            m1 = mh[..., 0] + al * (l - mh[..., 0])
            m2 = mh[..., 1] + al * (l * l - mh[..., 1])
            s_ = al * al + (1.0 - al) ** 2 * mh[..., 2]
        f3 = found[..., None]
        cv3 = np.where(f3, cb, c)
        length = np.where(found, n, 1.0)
        out_color = np.where(f3, cb * a, color)
        mom = np.where(f3, np.stack([m1, m2, s_, np.zeros((h, w))], axis=2), mom)
    with np.errstate(all="ignore"):
        dof = 1.0 - mom[..., 2]
        temporal = hit & (length >= min_frames) & (dof >= MIN_DOF)
        var_t = np.maximum(mom[..., 1] - mom[..., 0] ** 2, 0.0) / np.where(temporal, dof, 1.0) * mom[..., 2]
    b_mom, b_len = (mom, length) if stage_a is None else stage_a
    var_s, edge_b = spatial(b_mom, b_len, normal, z, min_frames, sigma_normal, sigma_depth)
    edge |= edge_b
    var = np.where(temporal, var_t, np.where(hit, np.nan_to_num(var_s), 0.0))
    return {"color": out_color, "variance": var * m2a, "cv": np.concatenate([cv3, var[..., None]], axis=2), "length": length, "mom": mom,
            "edge": edge, "temporal": temporal}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def random_frames(h, w, seed, miss_frac=0.1, nan_depths=3):
    """reproject_ref.random_frames with the current frame's normals brought to unit length (a plane's pixels then weigh each other with
    wn = 1 in stage B), a few NaN depths planted, and moments added to the history: m1 in (0.3, 1.2), m2 = m1^2 + up to 0.05,
    s in (0.12, 1).  -> ((color, albedo, normal, depth), history dict), float32."""
    (color, _, albedo, normal, depth), hist = R.random_frames(h, w, seed, miss_frac=miss_frac)
    rng = np.random.default_rng(seed + 555)
    nl = np.linalg.norm(normal.astype(np.float64), axis=2, keepdims=True)
    normal = R._f32(np.where(nl > 0, normal / np.where(nl > 0, nl, 1.0), 0.0))
    depth = depth.copy()
    if h * w > 16:
        for _ in range(nan_depths):
            depth[rng.integers(0, h), rng.integers(0, w)] = np.nan
    m1 = rng.uniform(0.3, 1.2, size=(h, w))
    hist["mom"] = R._f32(np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.05, size=(h, w)), rng.uniform(0.12, 1.0, size=(h, w)), np.zeros((h, w))], axis=2))
    return (color, albedo, normal, depth), hist


def flat_sequence(h, w, frames, seed, sigma=0.2):
    """The derived cases' frames: a flat plane (unit normal (0, 0, 1), constant depth 5, albedo 1) under a still camera with the luminance
    l = 1 + sigma g, g seeded Gaussian, the same in the three channels.  -> list of (color, albedo, normal, depth) float32, and the camera."""
    rng = np.random.default_rng(seed)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1.0
    albedo, depth = np.ones((h, w, 3), np.float32), np.full((h, w), 5.0, np.float32)
    out = []
    for _ in range(frames):
        l = 1.0 + sigma * rng.normal(size=(h, w))
        out.append((R._f32(np.repeat(l[..., None], 3, axis=2)), albedo, normal, depth))
    return out, R.plane_camera(0.0, 0.0, w, h)
