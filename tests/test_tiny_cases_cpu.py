"""The corpus of tests/tiny_cases.py is valid and decisive — checked on the CPU oracle alone, no GPU.

This checks the corpus, not the kernels.  For every case: the oracle and the device code compiled for the CPU (hostsim) agree bit for bit; the property
the case states of itself holds on the oracle's first hits along the pixel-centre rays (the tied, stacked, node-31 or triangle-63 triangle wins at least
HALF_WAVE rays, and it is the triangle tiny_cases.rule_winner names from the built tree); and the negative control — a changed copy of the data — changes
the oracle's picture in the pixels of those rays.  Where the control leaves the light alone (two plain materials swapped) it changes ONLY pixels with a
sample path that has a vertex on the tied triangles (oracle_lib.debug_path); a control that takes a triangle out of the light changes every lit pixel.

All of these are conditions on inputs, asserted: a case that misses one tests nothing and is to be replaced, not loosened.
"""
import numpy as np
import pytest

import hostsim_lib as H
import oracle_lib as O
import tiny_cases as TC
import tinyraytracing_amd as T

HALF_WAVE = 32
SEED = 0x71E5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def first_hits(s, c):
    org, dirs = TC.centre_rays(s, c.w, c.h)
    t, tri, uv = O.trace(s.flat, org, dirs)
    return org, dirs, t, tri


def pixels_with_a_vertex_on(s, p, group):
    """[h, w] bool: some sample path of the pixel has a vertex on a triangle of `group`"""
    out = np.zeros((p.height, p.width), bool)
    for y in range(p.height):
        for x in range(p.width):
            for k in range(p.spp):
                path = O.debug_path(s.flat, p, x, y, k, 64)
                if np.isin(path[:, 1].astype(np.int64), group).any():
                    out[y, x] = True
                    break
    return out


def tied_at_equal_t(s, d, group, org, dirs, rays):
    """Every triangle of the group is hit at bit-equal t along each of `rays` (O.tri_test, the reference's triangle test)"""
    for r in rays:
        ts = []
        for i in group:
            hit, out = O.tri_test(d.tri_v[i], org[r], dirs[r])
            assert hit, (r, i)
            ts.append(out[:1].view(np.uint32)[0])
        assert len(set(ts)) == 1, (r, ts)
    return len(group)


@pytest.mark.parametrize("case", TC.CASES, ids=[c.name for c in TC.CASES])
def test_case_is_valid_and_decisive(case, tmp_path):
    c, want = case, case.want
    s = c.make(tmp_path)
    d = TC.describe(s)
    assert d.n_lights == 1 and len(set(d.mat)) <= 5
    assert 32 <= c.w <= 64 and 24 <= c.h <= 48 and 4 <= c.spp <= 8 and (c.w * c.h * c.spp) % 512 != 0 and c.w * c.h * c.spp > 512
    if c.qualifies:
        assert d.n_tris <= 64 and d.n_nodes <= 32
    else:
        assert d.n_tris == 65 or d.n_nodes == 33  # one beyond, no further

    # the corpus itself: oracle == device code on the CPU, image bits and ray counts
    refs = {}
    for flags in (0, T.TRT_FLAG_FIXED_NEE):
        p = T.make_params(c.w, c.h, c.spp, SEED, flags=flags)
        ref, ost = O.render(s.flat, p)
        img, rays = H.render(s.flat, p)
        assert np.array_equal(bits(ref), bits(img)), (c.name, flags)
        assert rays == [ost.rays_camera, ost.rays_shadow, ost.rays_indirect], (c.name, flags)
        refs[flags] = (ref, ost)
    p = T.make_params(c.w, c.h, c.spp, SEED)
    ref, ost = refs[0]

    org, dirs, t, tri = first_hits(s, c)
    group = max(d.groups, key=lambda g: int(np.isin(tri, g).sum())) if d.groups else []  # (the vertex eye has two pairs: the one that is seen)
    on = np.isin(tri, group)
    zero = (dirs == 0).any(axis=1)
    decisive = int(on.sum())
    on_px = on.reshape(c.h, c.w)

    if c.kind in ("tie", "stack", "limit", "grazing", "shrunk"):
        winner = TC.rule_winner(d, group)
        assert decisive >= HALF_WAVE, decisive
        assert set(np.unique(tri[on]).tolist()) == {winner}, (np.unique(tri[on]), winner)
        n_leaves = len({d.leaf[i] for i in group})
        if "leaves" in want:
            assert want["leaves"][0] <= n_leaves <= want["leaves"][1], n_leaves
        assert tied_at_equal_t(s, d, group, org, dirs, np.nonzero(on)[0]) == len(group)
    if c.kind == "tie":
        assert len(group) == 2
        if want.get("nodes") == 2:
            assert len({d.leaf[i][0] for i in group}) == 2  # the tie meets at the fold of two subtrees
        if want.get("both_emissive"):
            assert all(d.emissive[i] for i in group) and len({d.mat[i] for i in group}) == 2
        if want.get("eye_in_leaf_box"):
            f = s.flat.contents
            eye = list(f.camera.eye)
            for i in group:
                k, slot = d.leaf[i]
                lo, hi = (f.nodes[k].lo0, f.nodes[k].hi0) if slot == 0 else (f.nodes[k].lo1, f.nodes[k].hi1)
                assert all(lo[a] < eye[a] < hi[a] for a in range(3))
    if c.kind == "stack":
        assert len(group) == 9 and [d.emissive[i] for i in group].count(True) == 1
        assert winner == sorted(group)[want["position"]] and d.emissive[winner]  # the second, sixth or ninth candidate of every such ray
    if c.kind == "limit":
        if "n_nodes" in want:
            assert d.n_nodes == want["n_nodes"]
        assert d.n_tris == want["n_tris"] and d.n_nodes <= want.get("max_nodes", 32)
        if "winner_node" in want:
            assert d.leaf[winner][0] == want["winner_node"] == d.n_nodes - 1
        if "winner_tri" in want:
            assert winner == want["winner_tri"] == d.n_tris - 1
            assert min(cnt for _, cnt in d.leaves.values()) >= 2  # leaf size 2 or more
        if want.get("leaf_of_15"):
            assert 15 in [cnt for _, cnt in d.leaves.values()]
    if c.kind == "beyond":
        assert d.n_tris == want["n_tris"] and (d.n_nodes == want["n_nodes"] if "n_nodes" in want else d.n_nodes <= want["max_nodes"])
        assert int((tri >= 0).sum()) >= HALF_WAVE
    if c.kind == "grazing":
        angle = np.abs(dirs[on, 2]) / np.linalg.norm(dirs[on], axis=1)  # the stack lies in the plane z = 0
        assert float(angle.max()) <= want["max_angle"], float(angle.max())
    if c.kind == "camera-vertex":
        f = s.flat.contents
        assert f.nodes[0].hi0[1] == f.camera.eye[1]  # the eye lies ON a plane of the first pair's box
        assert int((zero & (tri >= 0)).sum()) >= 64, int((zero & (tri >= 0)).sum())
        decisive = int((zero & (tri >= 0)).sum())
        on_px = (zero & (tri >= 0)).reshape(c.h, c.w)
    if c.kind == "camera-away":
        assert not (tri >= 0).any() and ost.shaded_hits == 0 and ost.rays_shadow == 0 and not ref.any()
        assert refs[T.TRT_FLAG_FIXED_NEE][1].shaded_hits == 0
    if c.kind != "camera-away":
        assert int((tri >= 0).sum()) >= HALF_WAVE and ost.shaded_hits > 0 and ost.rays_shadow > 0 and ost.rays_indirect > 0

    # the negative control
    if c.kind == "shrunk":
        u = c.control(tmp_path)
        assert not H.scene_info(s.flat)[1] and H.scene_info(u.flat)[1]  # the boxes no longer nest
        _, _, t_u, tri_u = first_hits(u, c)
        differ = (tri != tri_u) | (bits(t) != bits(t_u))
        assert int(differ.sum()) >= 8, int(differ.sum())  # the shrinking decides first hits
        ref_u, _ = O.render(u.flat, p)
        assert (ref_u != ref).any(axis=2)[differ.reshape(c.h, c.w)].any()
        print(f"{c.name}: {decisive} rays on the stack, {int(differ.sum())} first hits changed by the shrinking")
        return
    if c.control is None:
        assert c.kind in ("beyond", "camera-away")
        print(f"{c.name}: {int((tri >= 0).sum())} rays with a hit")
        return
    s2 = c.control(tmp_path)
    d2 = TC.describe(s2)
    assert np.array_equal(d2.tri_v, d.tri_v) and d2.children == d.children, "the control changes materials only"
    ref2, _ = O.render(s2.flat, p)
    changed = (ref2 != ref).any(axis=2)
    assert int((changed & on_px).sum()) >= HALF_WAVE, int((changed & on_px).sum())
    only = d2.emissive == d.emissive and sorted(d2.mat) == sorted(d.mat) and not any(d.emissive[i] for i in group)
    if only:  # the light is the same: nothing but paths through the tied triangles can tell the two scenes apart
        reach = pixels_with_a_vertex_on(s, p, group) | pixels_with_a_vertex_on(s2, p, group)
        assert not (changed & ~reach).any(), int((changed & ~reach).sum())
    print(f"{c.name}: {decisive} decisive rays, the control changes {int((changed & on_px).sum())} of their pixels and {int(changed.sum())} in all"
          + (", none without a path through the tie" if only else ""))


def test_the_corpus_covers_what_it_claims():
    names = [c.name for c in TC.CASES]
    for prefix, n in (("ties-in-leaf-", 4), ("ties-between-leaves-", 6), ("ties-between-subtrees-", 1), ("deep-stack-winner-", 3), ("deep-stack-across-leaves-", 3),
                      ("node-31", 1), ("tri-63", 1), ("one-beyond-", 2), ("boxes-that-do-not-nest", 1), ("camera-", 3), ("grazing", 1)):
        assert sum(x.startswith(prefix) for x in names) == n, prefix
    assert sum(not c.qualifies for c in TC.CASES) == 2


def test_rule_winner_on_a_hand_made_tree():
    """rule_winner against the rule spelled out by hand: inside a leaf the last emissive, else the first; between children child0's iff emissive"""
    d = TC.Description()
    leaf = lambda first, count: TC.LEAF_BIT | (count << 27) | first  # noqa: E731
    d.children = [(1, 2), (leaf(0, 2), leaf(2, 1)), (leaf(3, 2), leaf(5, 1))]
    for em, want in (([0] * 6, 5), ([1, 0, 0, 0, 0, 0], 0), ([0, 0, 1, 0, 0, 0], 2), ([0, 1, 1, 0, 0, 0], 1), ([0, 0, 0, 1, 1, 0], 4), ([0, 0, 0, 0, 0, 1], 5),
                     ([0, 0, 1, 0, 1, 1], 2)):
        d.emissive = [bool(x) for x in em]
        assert TC.rule_winner(d, range(6)) == want, em
    d.emissive = [False] * 6
    assert TC.rule_winner(d, [0, 1]) == 0 and TC.rule_winner(d, [0, 3, 4]) == 3
