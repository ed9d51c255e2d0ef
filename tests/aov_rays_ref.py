"""CPU restatement of trt_aov_rays (include/trt.h): the closest hits of the caller's rays from one batched oracle_trace, the first-hit
features of aov_ref.first_hit_features, entries that trt_render_rays' validity rule refuses counted as misses (they are never handed to the
oracle as given), and the contract's accumulation: per channel v = value / (float)spp as a float, sum += (double)v in increasing sample."""
import numpy as np

import aov_ref
import oracle_lib as O

F32 = np.float32
KEYS = ("albedo", "normal", "depth")
MISS = (np.zeros(3, F32), np.zeros(3, F32), aov_ref.TRT_INF)


def valid_entries(org, dirs):
    """rayValid (trt_path.h): all six components finite and the direction not (0, 0, 0).  org, dirs [..., 3] -> bool [...]."""
    org, dirs = np.asarray(org, F32), np.asarray(dirs, F32)
    return np.isfinite(org).all(axis=-1) & np.isfinite(dirs).all(axis=-1) & (dirs != 0).any(axis=-1)


def zero_sums(n):
    return {"albedo": np.zeros((n, 3), np.float64), "normal": np.zeros((n, 3), np.float64), "depth": np.zeros(n, np.float64)}


def accumulate(albedo, normal, depth, valid, spp, sums=None):
    """The sums of the contract from per-ray features [S, n, 3], [S, n, 3], [S, n] (float32) and valid [S, n]: an invalid entry adds the
    miss's terms.  sums: the in/out dict (None = zeros).  -> the dict."""
    albedo, normal, depth = np.array(albedo, F32), np.array(normal, F32), np.array(depth, F32)
    n_samples, n = depth.shape
    albedo[~valid], normal[~valid], depth[~valid] = MISS
    sums = zero_sums(n) if sums is None else sums
    scale = F32(spp)
    for s in range(n_samples):
        for k, vals in (("albedo", albedo), ("normal", normal), ("depth", depth)):
            if sums.get(k) is not None:
                sums[k] += (vals[s] / scale).astype(F32).astype(np.float64)
    return sums


def aov_rays(scene, org, dirs, spp, sums=None):
    """What trt_aov_rays leaves in `sums` (None = zeros) for org / dirs [S, n, 3] on `scene`, at the scale spp."""
    org, dirs = np.ascontiguousarray(org, F32), np.ascontiguousarray(dirs, F32)
    n_samples, n = org.shape[0], org.shape[1]
    valid = valid_entries(org, dirs)
    # the oracle sees the valid rays only; every other entry keeps the miss record
    t = np.full(n_samples * n, aov_ref.TRT_INF, F32)
    tri = np.full(n_samples * n, -1, np.int32)
    uv = np.zeros((n_samples * n, 2), F32)
    sel = np.nonzero(valid.reshape(-1))[0]
    if len(sel):
        t[sel], tri[sel], uv[sel] = O.trace(scene.flat, org.reshape(-1, 3)[sel], dirs.reshape(-1, 3)[sel])
    albedo, normal, depth = aov_ref.first_hit_features(scene, t, tri, uv)
    return accumulate(albedo.reshape(n_samples, n, 3), normal.reshape(n_samples, n, 3), depth.reshape(n_samples, n), valid, spp, sums)
