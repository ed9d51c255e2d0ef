"""What the ray queries of include/trt.h return, restated on the oracle's closest hit — no oracle code of their own.

Whether a hit is accepted does not depend on the bound (the leaf-box rule, and the emissive tie rules: at equal t every tied candidate lies
on the same side of it).  So with (t0, tri0, uv0) = oracle_lib.trace(flat, org, dir) and bound = t_max > TRT_T_MIN ? min(t_max, TRT_INF)
: TRT_T_MIN:
  trt_trace_closest_range = (t0, tri0, uv0) where tri0 >= 0 and t0 < bound, else (TRT_INF, -1, 0, 0);
  trt_trace_occluded      = tri0 >= 0 and t0 < bound.
"""
import numpy as np

import oracle_lib as O

TRT_INF = np.float32(114514.0)
TRT_T_MIN = np.float32(0.0005)


def bound(t_max, n):
    """The per-ray bound the library searches below (t_max None: TRT_INF for every ray)."""
    if t_max is None:
        return np.full(n, TRT_INF, np.float32)
    m = np.asarray(t_max, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.where(m > TRT_T_MIN, np.minimum(m, TRT_INF), TRT_T_MIN).astype(np.float32)


def bounds_for(t0, seed=5):
    """Per ray: a random fraction in [0, 1.5] of t0, exactly t0, nextafter(t0, inf), NaN, +-inf, 0, TRT_T_MIN, 1e30 (t0: the unbounded hit)."""
    rng = np.random.default_rng(seed)
    n = len(t0)
    k = np.arange(n) % 12
    frac = (rng.random(n) * 1.5).astype(np.float32) * t0
    choices = [frac, frac, frac, t0, np.nextafter(t0, np.float32(np.inf)), np.full(n, np.nan, np.float32), np.full(n, np.inf, np.float32),
               np.full(n, -np.inf, np.float32), np.zeros(n, np.float32), np.full(n, TRT_T_MIN, np.float32), np.full(n, 1e30, np.float32), frac]
    return np.choose(k, choices).astype(np.float32)


def inside(ref, t_max):
    t0, tri0, _ = ref
    with np.errstate(invalid="ignore"):
        return (tri0 >= 0) & (t0 < bound(t_max, len(t0)))


def closest(ref, t_max):
    """ref = (t0, tri0, uv0) of oracle_lib.trace -> (t, tri, uv) of trt_trace_closest_range."""
    t0, tri0, uv0 = ref
    hit = inside(ref, t_max)
    return (np.where(hit, t0, TRT_INF).astype(np.float32), np.where(hit, tri0, -1).astype(np.int32),
            np.where(hit[:, None], uv0, np.float32(0)).astype(np.float32))


def occluded(ref, t_max):
    """ref = (t0, tri0, uv0) of oracle_lib.trace -> the bools of trt_trace_occluded."""
    return inside(ref, t_max)


def trace(flat, org, direction, t_max):
    """Both answers straight from the oracle: (closest record, occluded)."""
    ref = O.trace(flat, org, direction)
    return closest(ref, t_max), occluded(ref, t_max)
