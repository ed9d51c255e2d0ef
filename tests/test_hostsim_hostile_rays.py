"""Hostile rays on foreign trees, on the device code compiled for the CPU (tests/hostsim, built with the range checks of TRT_WALK_CHECK).

Every tree a caller can hand over — the loaders' trees, trees whose boxes do not nest (several seeds and amounts, a deep soup among them),
trees whose children come before their parents, LBVH trees and the reference's own tree — meets every family of hostile rays (non-finite
and adversarial rays, grazing rays, axis-aligned rays, directions that are the zero vector), on both node kinds where the tree allows the
compressed one.  Every way a ray gets walked is asked: the closest hit of the per-lane drivers, the bounded closest hit and the occlusion
test of the queries, and k_trace_fix's composition (the literal walk or the exact form) with and without a bound.  The answers must be the
oracle's (query_ref.py for the bounded ones) bit for bit, and no walk may leave its tree, its triangles or the GPU driver's stack."""
import numpy as np
import pytest

import hostsim_lib as H
import lbvh_ref
import oracle_lib as O
import query_ref as Q
import raygen
import scene_util as SU
import tinyraytracing_amd as T


def _non_nesting(base, count, seed, amount, **kw):
    def make():
        s = T.Scene.named(base, 64, 36, **kw)
        assert SU.shrink_some_boxes(s, count, seed=seed, amount=amount) > 0
        return s
    return make


def _reversed(base):
    def make():
        s = T.Scene.named(base, 64, 36)
        assert SU.renumber_nodes_reversed(s) > 0
        return s
    return make


def _lbvh(base, leaf_num=2):
    """A shipped scene with the tree of the GPU builder, from its plain restatement (lbvh_ref.build: the same nodes and order as
    trt_build_lbvh), adopted the way Scene.named(..., builder="lbvh") adopts the device's."""
    def make():
        import ctypes as C
        import os
        from tinyraytracing_amd._abi import BvhNode
        d = os.path.join(T.SCENES_DIR, base)
        s = T.Scene.load(os.path.join(d, base + ".xml"), os.path.join(d, base + ".obj"), os.path.join(d, base + ".mtl"), d, 64, 36)
        n = s.info["n_triangles"]
        v = np.empty(n * 9, np.float32)
        s._check(s._lib.trth_scene_vertices(s._h, v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
        raw, n_nodes, order, depth = lbvh_ref.build(v.reshape(n, 9), leaf_num)
        nodes = (BvhNode * n_nodes).from_buffer_copy(raw)
        order = np.ascontiguousarray(order, np.uint32)
        s._check(s._lib.trth_scene_adopt_bvh(s._h, nodes, n_nodes, order.ctypes.data_as(C.POINTER(C.c_uint32)), depth))
        s._built = True
        return s
    return make


TREES = {
    "back": lambda: T.Scene.named("back", 64, 36),
    "veach-mis": lambda: T.Scene.named("veach-mis", 64, 36),
    "staircase": lambda: T.Scene.named("staircase", 64, 36),
    "non-nesting-staircase-60": _non_nesting("staircase", 60, 3, 0.35),
    "non-nesting-staircase-400": _non_nesting("staircase", 400, 11, 0.6),
    "non-nesting-veach-mis-150": _non_nesting("veach-mis", 150, 5, 0.2),
    "non-nesting-back-20": _non_nesting("back", 20, 2, 0.5),
    "non-nesting-soup": _non_nesting("soup", 3000, 7, 0.45, n=60000),
    "reversed-staircase": _reversed("staircase"),
    "reversed-veach-mis": _reversed("veach-mis"),
    "lbvh-staircase": _lbvh("staircase"),
    "lbvh-veach-mis": _lbvh("veach-mis", 8),
    "reference-tree-veach-mis": lambda: SU.load_with_reference_tree("veach-mis", 64, 36),
    "reference-tree-staircase": lambda: SU.load_with_reference_tree("staircase", 64, 36),
}


def ray_families(s):
    """name -> (org, dir): every hostile family of raygen / scene_util on this tree."""
    return {"non_finite": raygen.non_finite_rays(s, 4000),
            "adversarial": raygen.adversarial_rays(s, 4000),
            "grazing": raygen.grazing_rays(s.flat, 2000),
            "axis": SU.axis_rays(s, 48),
            "zero_direction": raygen.zero_direction_rays(s, 2400)}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check(tag, fam, got, want, occlusion=False):
    """got / want: (t, tri, uv) over the concatenated families; the first family with a difference is named."""
    bad = (got[1] != want[1]) if occlusion else ((got[1] != want[1]) | (_bits(got[0]) != _bits(want[0]))
                                                 | (_bits(got[2]) != _bits(want[2])).any(1))
    if bad.any():
        names = [f for f, _ in fam]
        first = int(np.nonzero(bad)[0][0])
        which = {names[i]: int(bad[a:b].sum()) for i, (a, b) in enumerate(_spans(fam)) if bad[a:b].any()}
        pytest.fail(f"{tag}: {int(bad.sum())} rays differ from the oracle {which}; first: ray {first}, got {got[1][first]} t={got[0][first]!r}, "
                    f"want {want[1][first]} t={want[0][first]!r}")


def _spans(fam):
    a = 0
    for _, n in fam:
        yield a, a + n
        a += n


_cache = {}


def case(tree):
    if tree not in _cache:
        s = TREES[tree]()
        rays = ray_families(s)
        org = np.concatenate([o for o, _ in rays.values()])
        dirs = np.concatenate([d for _, d in rays.values()])
        fam = [(k, len(o)) for k, (o, _) in rays.items()]
        ref = O.trace(s.flat, org, dirs)
        _cache.clear()  # one tree at a time: the soup is large
        _cache[tree] = (s, org, dirs, fam, ref)
    return _cache[tree]


NODE_KINDS = [0, 1]


@pytest.mark.parametrize("nk", NODE_KINDS)
@pytest.mark.parametrize("tree", list(TREES))
def test_hostile_rays_on_every_tree_walk_like_the_oracle(tree, nk):
    s, org, dirs, fam, ref = case(tree)
    # a tree that does not qualify for the compressed nodes is walked on the 4-wide ones whatever the node kind says (trt_create and the hostsim)
    nk_eff = nk if nk == 0 or H.compressible(s.flat) else 0
    tm = Q.bounds_for(ref[0])
    b = Q.bound(tm, len(org))
    old = H.set_node_kind(nk)
    try:
        t, tri, uv, _ = H.trace(s.flat, org, dirs)
        _check(f"{tree} nk={nk_eff} closest", fam, (t, tri, uv), ref)
        # the queries on the per-lane drivers' walk: closest hit below the bound, and occlusion below it
        _check(f"{tree} nk={nk_eff} closest below t_max", fam, H.query(s.flat, org, dirs, b), Q.closest(ref, tm))
        occ = H.query(s.flat, org, dirs, b, any=True)[1] >= 0
        _check(f"{tree} nk={nk_eff} occluded", fam, (None, occ, None), (None, Q.occluded(ref, tm), None), occlusion=True)
        _check(f"{tree} nk={nk_eff} occluded, no bound", fam, (None, H.query(s.flat, org, dirs, None, any=True)[1] >= 0, None),
               (None, ref[1] >= 0, None), occlusion=True)
        if nk == 0:
            # k_trace_fix's walk of a redo list (the literal walk or the exact form on the 4-wide nodes, whatever the node kind)
            _check(f"{tree} fix closest", fam, H.query(s.flat, org, dirs, None, form=1), ref)
            _check(f"{tree} fix closest below t_max", fam, H.query(s.flat, org, dirs, b, form=1), Q.closest(ref, tm))
            occ = H.query(s.flat, org, dirs, b, any=True, form=1)[1] >= 0
            _check(f"{tree} fix occluded", fam, (None, occ, None), (None, Q.occluded(ref, tm), None), occlusion=True)
    finally:
        H.set_node_kind(old)


def test_zero_direction_rays_cover_what_they_claim():
    """raygen.zero_direction_rays: every direction is a zero vector, all eight sign patterns meet every kind of origin, and the kinds are there
    (inside the scene's box, outside it, on a plane of the tree's boxes, non-finite)."""
    s = T.Scene.named("staircase", 64, 36)
    org, d = raygen.zero_direction_rays(s, 2400)
    assert not np.abs(d).any()
    signs = (np.signbit(d) * np.array([1, 2, 4])).sum(1)
    kind = np.arange(len(org)) % 4
    for k in range(4):
        assert set(signs[kind == k].tolist()) == set(range(8)), k
    lo, hi = raygen.scene_bounds(s)
    fin = np.isfinite(org).all(1)
    inside = fin & (org >= lo).all(1) & (org <= hi).all(1)
    hostile = (~np.isfinite(org) | (np.abs(org) == np.float32(1e38))).any(1)
    assert inside[kind == 0].all() and not inside[kind == 1].any() and hostile[kind == 3].all() and fin[kind != 3].all()
    planes = raygen.box_planes(s.flat)
    on = np.array([any(np.isin(org[i, a], planes[a]) for a in range(3)) for i in np.nonzero(kind == 2)[0]])
    assert on.all()

