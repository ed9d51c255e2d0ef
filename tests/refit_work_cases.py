"""The scenes, moves and ray batches on which the traversal WORK of an updated handle is held to a reference (tests/test_refit_work_cpu.py proves on
hostsim that every batch is sensitive to the driver faults it is meant to catch; tests/test_gpu_refit_work.py runs the same batches on the MI355X).

Per scene: S0 as loaded; `shrink` — an object at another size about its centroid (refit_ref.shrink_about_centroid), `smooth` — refit_ref.smooth_displace,
`light` — light 0's triangles far out along +y (refit_ref.light_far_away).  The moved scenes are what Scene.set_vertices leaves, one per (scene, move)."""
import numpy as np

import raygen
import refit_ref as RR
import scene_util as SU
import tinyraytracing_amd as T

W, H, SPP = 96, 64, 4
SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE, "blob": T.SEED_BLOB}
LARGE = ("veach-mis", "staircase", "blob")
# smooth_displace's amplitude: a few percent of the scene's size (blob and back measure 556 units, the other two about ten)
SMOOTH_AMP = {"back": 12.0, "blob": 12.0, "veach-mis": 0.4, "staircase": 0.4}
_scenes, _rays = {}, {}


def load(name):
    """A new Scene object of the named scene (every call: the moved scenes are moved in place)."""
    return T.Scene.named("blob", W, H, n=20000) if name == "blob" else T.Scene.named(name, W, H)


def shrink_mask(name, s0):
    """What `shrink` scales.  back: the cube on the floor.  The others: the triangles wholly inside the middle 80 % of the bounds — at 40 % and 60 % the deepest
    level of the 4-wide trees of blob and staircase is not touched, and a skipped deepest level then costs nothing (measured on hostsim)."""
    if name == "back":
        return RR.move_inner_object(s0)[1]
    return RR.central_object(s0.arrays()["tri_v"], 0.8)


def vertices(name, move):
    """The vertex set of `move`: 'S0', 'shrink', 'smooth', 'light', or 'grow' (back only: the cube at three times its size — back's tree has four BVH2 nodes and
    keeps one collapse under every shrink and every smooth displacement tried, amplitudes 12 to 400, so that is the move on which a fresh handle's work differs)."""
    s0 = scene(name, "S0")
    v0 = s0.arrays()["tri_v"]
    if move == "S0":
        return v0.copy()
    if move == "shrink":
        return RR.shrink_about_centroid(v0, shrink_mask(name, s0), 0.5)
    if move == "grow":
        assert name == "back"
        return RR.shrink_about_centroid(v0, shrink_mask(name, s0), 3.0)
    if move == "smooth":
        return RR.smooth_displace(v0, SMOOTH_AMP[name])
    if move == "light":
        return RR.light_far_away(s0, 0)[0]
    raise KeyError(move)


def scene(name, move="S0"):
    """The scene Scene.set_vertices leaves for `move` (cached; do not move it)."""
    key = (name, move)
    if key not in _scenes:
        s = load(name)
        if move != "S0":
            s.set_vertices(vertices(name, move))
        _scenes[key] = s
    return _scenes[key]


def rays(name, n_random=50000):
    """(org, dir, plain): random rays through the bounds of S0, its primary rays and axis-parallel rays; plain = the rays without a zero direction
    component — the others go to k_trace_fix, which is compiled without counters, so work is compared on the plain ones and records on all."""
    if name not in _rays:
        s = scene(name)
        lo, hi = raygen.scene_bounds(s)
        sets = [raygen.random_rays(n_random, lo, hi, seed=21), raygen.primary_rays(s, W, H), SU.axis_rays(s, 48)]
        o, d = np.concatenate([x[0] for x in sets]).astype(np.float32), np.concatenate([x[1] for x in sets]).astype(np.float32)
        with np.errstate(divide="ignore"):
            plain = np.isfinite(np.float32(1.0) / d).all(1)  # not raySpecial() (trt_path.h)
        assert 50000 <= len(o) <= 200000 and 0 < (~plain).sum() < len(o) // 10
        _rays[name] = (np.ascontiguousarray(o), np.ascontiguousarray(d), plain)
    return _rays[name]


def bounds(name):
    """One t_max per ray, about half of them in front of the hit (the bounded queries)."""
    o = rays(name)[0]
    lo, hi = raygen.scene_bounds(scene(name))
    return (np.random.default_rng(9).random(len(o)) * np.float32(np.linalg.norm(hi - lo))).astype(np.float32)
