"""The reference of the GPU BVH builder (tests/lbvh_ref.py) and the tree checker (tests/bvh_check.py), without a GPU.

The reference is checked on hand-worked inputs whose trees are written out here; the checker must reject trees broken in each of the
ways it exists to catch, and accept the reference's own trees and those of the host builders, bit for bit.
"""
import numpy as np
import pytest

import bvh_check as B
import lbvh_cases as L
import lbvh_ref as R
import scene_util as SU
import tinyraytracing_amd as T

P = np.float32(0.001)


def words(nodes):
    return np.frombuffer(nodes, np.uint32).reshape(-1, 16)


def boxes(nodes):
    return np.frombuffer(nodes, np.float32).reshape(-1, 16)[:, :12].reshape(-1, 2, 2, 3)


def leaf(first, count):
    return 0x80000000 | (count << 27) | first


def box(lo, hi):
    return np.array([np.float32(lo) - P, np.float32(hi) + P])


# ---------------------------------------------------------------- hand-worked inputs
# Point triangles at x = 8, 0, 4, 2 (y = z = 0), in that caller order.  The centre frame is [0, 8] on x (scale 2^21 / 8 = 2^18) and flat
# on y and z (scale 0): x quantises to 0, 2^19, 2^20 and 2^21 - 1 (clamped), i.e. Morton keys 0, 2^59, 2^62 and 0x4924...924 | 2^62.
# Sorted positions 0..3 hold x = 0, 2, 4, 8 (caller 1, 3, 2, 0).  The root [0, 3] splits at bit 62 between positions 1 and 2: inner
# node 1 = [0, 1] (bit 59), inner node 2 = [2, 3].
FOUR_X = [8.0, 0.0, 4.0, 2.0]


def _four_points():
    return np.array([[x, 0, 0] * 3 for x in FOUR_X], np.float32)


@pytest.mark.parametrize("cluster", ["0", None])
def test_reference_on_four_points(cluster):
    """Leaf 1: every inner node stays.  By default (clusters of 2 below 50 k triangles) the two pairs are the clusters, the SAH top over
    them is one node with the same split, and the in-cluster nodes follow it: both paths give the same three nodes."""
    v = _four_points()
    st = {}
    nodes, nn, order, depth = R.build(v, 1, cluster, st)
    assert st["path"] == ("radix" if cluster == "0" else "clusters")
    assert order.tolist() == [1, 3, 2, 0] and nn == 3 and depth == 2
    w, b = words(nodes), boxes(nodes)
    assert w[:, 12:].tolist() == [[1, 2, 0, 0], [leaf(0, 1), leaf(1, 1), 0, 0], [leaf(2, 1), leaf(3, 1), 0, 0]]
    yz = box(0, 0)
    want = {(0, 0): (0, 2), (0, 1): (4, 8), (1, 0): (0, 0), (1, 1): (2, 2), (2, 0): (4, 4), (2, 1): (8, 8)}
    for (i, k), (lo, hi) in want.items():
        assert np.array_equal(b[i, k, :, 0], box(lo, hi)), (i, k)
        assert np.array_equal(b[i, k, :, 1:], np.stack([yz] * 2, 1)), (i, k)
    B.check_bvh(v, nodes, nn, order, 1, depth)


def test_reference_on_equal_codes():
    """Five equal triangles: one Morton key, the tree split by position alone — the root [0, 4] at the highest bit of 0 ^ 4 (child0 =
    inner node 3 = [0, 3], child1 = position 4), node 3 into [0, 1] and [2, 3].  With leaf 2 those two are leaves: two nodes, depth 2."""
    v = np.tile(np.array([1, 1, 1, 2, 1, 1, 1, 3, 1], np.float32), (5, 1))
    nodes, nn, order, depth = R.build(v, 2, "0")
    assert order.tolist() == [0, 1, 2, 3, 4] and nn == 2 and depth == 2
    w, b = words(nodes), boxes(nodes)
    assert w[:, 12:14].tolist() == [[1, leaf(4, 1)], [leaf(0, 2), leaf(2, 2)]]
    want = np.array([[1, 1, 1], [2, 3, 1]], np.float32)
    want[0] -= P
    want[1] += P
    assert np.array_equal(b, np.broadcast_to(want, b.shape))
    B.check_bvh(v, nodes, nn, order, 2, depth)
    # the default path: clusters of 2 (nodes [0, 1], [2, 3] and position 4), all centres equal -> the SAH top's costs tie and the first
    # split on axis 0 wins: cluster 0 | clusters 1, 2 -> then 1 | 2
    nodes, nn, order, depth = R.build(v, 2, None)
    assert nn == 2 and depth == 2
    assert words(nodes)[:, 12:14].tolist() == [[leaf(0, 2), 1], [leaf(2, 2), leaf(4, 1)]]
    B.check_bvh(v, nodes, nn, order, 2, depth)


def test_reference_single_leaf_root_and_empty_scene():
    v = _four_points()[:3]
    nodes, nn, order, depth = R.build(v, 8)
    w, b = words(nodes), boxes(nodes)
    assert nn == 1 and depth == 1 and order.tolist() == [0, 1, 2]
    assert w[0, 12:].tolist() == [leaf(0, 3), leaf(0, 0), 0, 0]
    assert np.array_equal(b[0, 0, :, 0], box(0, 8)) and np.array_equal(b[0, 1], b[0, 0])
    B.check_bvh(v, nodes, nn, order, 8, depth)
    nodes, nn, order, depth = R.build(np.zeros((0, 9), np.float32), 2)
    assert nn == 1 and order.size == 0 and words(nodes)[0, 12:14].tolist() == [leaf(0, 0), leaf(0, 0)]
    assert np.array_equal(boxes(nodes)[0], np.broadcast_to(np.array([[-P] * 3, [P] * 3]), (2, 2, 3)))
    B.check_bvh(np.zeros((0, 9), np.float32), nodes, nn, order, 2, depth)


def test_cluster_tiers():
    assert [R.cluster_for(n, 2) for n in (49_999, 50_000, 499_999, 500_000, 3_999_999, 4_000_000)] == [2, 16, 16, 128, 128, 2048]
    assert R.cluster_for(10, 8, "3") == 8 and R.cluster_for(10, 8, "0") == 0 and R.cluster_for(10, 2, "-5") == 0


def test_ladder_is_a_chain():
    """The ladder's radix tree is a chain: the root splits the codes 2^62 and 2^63 - 1 (one node) from 0, 2^0, ..., 2^61, a chain of 62 nodes
    below it — with one triangle per rung and leaf 1, 64 inner nodes of 65 triangles, 63 levels deep."""
    v = L.ladder(1)
    nodes, nn, order, depth = R.build(v, 1, "0")
    assert nn == 64 and depth == 63
    B.check_bvh(v, nodes, nn, order, 1, depth)


# ---------------------------------------------------------------- the checker rejects what it exists to catch
def _tree():
    v = L.soup(3000, seed=21)
    nodes, nn, order, depth = R.build(v, 4, "0")
    return v, bytearray(nodes), nn, order.copy(), depth


def _first_leaf(w):
    i, k = np.argwhere((w[:, 12:14] & 0x80000000) != 0)[0]
    return i, k


def test_checker_rejects_a_box_one_ulp_too_small():
    v, nodes, nn, order, depth = _tree()
    B.check_bvh(v, bytes(nodes), nn, order, 4, depth)
    f = np.frombuffer(nodes, np.float32).reshape(-1, 16)
    f[7, 9 + 1] = np.nextafter(f[7, 9 + 1], np.float32(-np.inf))  # node 7, hi1.y
    with pytest.raises(B.BvhError, match=r"node 7 child1 hi\[1\]"):
        B.check_bvh(v, bytes(nodes), nn, order, 4, depth)


def test_checker_rejects_a_triangle_outside_its_leaf_box():
    v, nodes, nn, order, depth = _tree()
    w = np.frombuffer(nodes, np.uint32).reshape(-1, 16)
    i, k = _first_leaf(w)
    moved = v.copy()
    moved[order[w[i, 12 + k] & 0x07FFFFFF], 0] += np.float32(0.5)  # its first vertex's x leaves the box
    with pytest.raises(B.BvhError, match=r"node \d+ child\d (lo|hi)\[0\] .* the exact padded bound"):  # (its leaf or an ancestor, top first)
        B.check_bvh(moved, bytes(nodes), nn, order, 4, depth)


def test_checker_rejects_a_triangle_in_two_leaves():
    v, nodes, nn, order, depth = _tree()
    w = np.frombuffer(nodes, np.uint32).reshape(-1, 16)
    i, k = _first_leaf(w)
    first = int(w[i, 12 + k] & 0x07FFFFFF)
    w[i, 12 + k] = leaf(first + 1 if first == 0 else first - 1, int((w[i, 12 + k] >> 27) & 15))  # slides onto a neighbour's triangle
    with pytest.raises(B.BvhError, match=r"triangle position \d+ lies in (2|0) leaves"):
        B.check_bvh(v, bytes(nodes), nn, order, 4, depth)


def test_checker_rejects_an_order_that_is_not_a_permutation():
    v, nodes, nn, order, depth = _tree()
    order[5] = order[6]
    with pytest.raises(B.BvhError, match="not a permutation"):
        B.check_bvh(v, bytes(nodes), nn, order, 4, depth)


def test_checker_rejects_a_wrong_depth():
    v, nodes, nn, order, depth = _tree()
    for d in (depth - 1, depth + 1):
        with pytest.raises(B.BvhError, match=f"reported depth {d}"):
            B.check_bvh(v, bytes(nodes), nn, order, 4, d)


def test_checker_rejects_swapped_children_and_oversized_leaves():
    v, nodes, nn, order, depth = _tree()
    w = np.frombuffer(nodes, np.uint32).reshape(-1, 16)
    w2 = w.copy()
    w2[0, 12], w2[0, 13] = w[0, 13], w[0, 12]
    w2[0, 0:6], w2[0, 6:12] = w[0, 6:12], w[0, 0:6]
    with pytest.raises(B.BvhError, match="node 0: child0's triangles"):
        B.check_bvh(v, w2.tobytes(), nn, order, 4, depth)
    with pytest.raises(B.BvhError, match=r"leaf of \d+ triangles \(leaf_num 1\)"):
        B.check_bvh(v, bytes(nodes), nn, order, 1, depth)


# ---------------------------------------------------------------- the reference's own trees, the host builders' trees
@pytest.mark.parametrize("cluster", [None, "0", "48"])
@pytest.mark.parametrize("case", list(L.HOSTILE))
def test_checker_accepts_the_reference_trees(case, cluster):
    v = L.HOSTILE[case]()
    st = {}
    nodes, nn, order, depth = R.build(v, 2, cluster, st)
    B.check_bvh(v, nodes, nn, order, 2, depth)
    if cluster is None:  # TopBuilder's two fallbacks are reached (the GPU module requires the device to reach them alike)
        if case in ("identical_100k", "ladder_x60", "flat_yz"):
            assert st["top_median_at_depth"] > 0, st
        if case in ("near_1e30", "infinities", "extent_overflow"):
            assert st["top_fallback"] > 0, st


@pytest.mark.parametrize("leaf_num", [1, 2, 8, 15])
@pytest.mark.parametrize("builder", ["sweep", "binned", "auto"])
def test_checker_on_host_builders(builder, leaf_num):
    for name in ("staircase", "veach-mis"):
        s = T.Scene.named(name, 64, 36, leaf_num=leaf_num, builder=builder)
        f = s.flat.contents
        B.check_bvh(np.ctypeslib.as_array(f.tri_v, shape=(f.n_tris * 9,)), f.nodes, f.n_nodes, np.arange(f.n_tris), leaf_num, f.bvh_depth)
        s.close()


@pytest.mark.parametrize("name", ["back", "staircase"])
def test_checker_on_the_reference_builders_tree(name):
    s = SU.load_with_reference_tree(name)
    f = s.flat.contents
    B.check_bvh(np.ctypeslib.as_array(f.tri_v, shape=(f.n_tris * 9,)), f.nodes, f.n_nodes, np.arange(f.n_tris), 8, f.bvh_depth)
    s.close()


def test_checker_on_a_host_builders_single_leaf_root():
    """The pinned box of the empty leaf: the host builder gives child1 the box of child0."""
    d = T.SCENES_DIR + "/back"
    s = T.Scene.load(d + "/back.xml", d + "/back.obj", d + "/back.mtl", d, 16, 16)
    s._check(s._lib.trth_scene_drop_tris(s._h, 6, 12))
    s.build_bvh(15, "auto")
    f = s.flat.contents
    assert f.n_nodes == 1 and f.n_tris <= 15
    B.check_bvh(np.ctypeslib.as_array(f.tri_v, shape=(f.n_tris * 9,)), f.nodes, f.n_nodes, np.arange(f.n_tris), 15, f.bvh_depth)
    s.close()
