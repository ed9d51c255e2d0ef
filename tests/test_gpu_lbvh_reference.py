"""The GPU BVH builder (trt_build_lbvh) node for node against a plain reference of its construction — MI355X only.

Every other test of the builder walks the tree it returns, so a wrong box there is walked by the oracle too and goes unseen.  Here the
builder's output — nodes as raw bytes (reserved words included), node count, triangle order and depth — must EQUAL what tests/lbvh_ref.py
computes from the documented construction, and tests/bvh_check.py, which knows no builder, must accept the tree: exact padded boxes,
every triangle in one leaf, post-BVH order, the reported depth.  The inputs walk the builder's size-dependent paths (one block of 1024
positions, the spanning nodes' rounds, n <= leaf_num, the cluster tiers and overrides, the plain radix tree) and hostile distributions.
"""
import ctypes as C

import numpy as np
import pytest

import bvh_check as B
import lbvh_cases as L
import lbvh_ref as R
from tinyraytracing_amd import _abi

pytestmark = pytest.mark.gpu
TRT_EINVAL = 1
FIELDS = ("lo0", "hi0", "lo1", "hi1", "child0", "child1", "reserved")


def gpu_build(v, leaf_num, capacity=None):
    """trt_build_lbvh on device 0: (rc, nodes bytes, n_nodes, order, depth).  Unwritten node words and order entries are poisoned."""
    b = _abi.load_build()
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 9)
    n = v.shape[0]
    cap = max(n, 2) - 1 if capacity is None else capacity
    buf = np.full(max(cap, 1) * 64, 0xA5, np.uint8)
    order = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    nn, depth = C.c_uint32(0), C.c_uint32(0)
    rc = b.trt_build_lbvh(v.ctypes.data_as(C.POINTER(C.c_float)), n, leaf_num, 0, C.cast(buf.ctypes.data, C.POINTER(_abi.BvhNode)), cap,
                          C.byref(nn), order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(depth), None)
    return rc, buf[:nn.value * 64].tobytes(), nn.value, order[:n].copy(), depth.value


def _first_difference(got, want):
    g = np.frombuffer(got, np.uint32).reshape(-1, 16)
    w = np.frombuffer(want, np.uint32).reshape(-1, 16)
    m = min(len(g), len(w))
    bad = np.argwhere(g[:m] != w[:m])
    if not bad.size:
        return f"node counts {len(g)} / {len(w)}"
    i, k = bad[0]
    field = FIELDS[min(k // 3, 4) if k < 12 else 4 + (k - 12) if k < 14 else 6]
    return (f"{len(bad)} words differ; first: node {i} word {k} ({field}) device {g[i, k]:#010x} reference {w[i, k]:#010x}; "
            f"device node {g[i].tolist()} reference node {w[i].tolist()}")


def compare(v, leaf_num, cluster_env, monkeypatch):
    """Builds on the device with TRT_LBVH_CLUSTER = cluster_env (None: unset), requires the reference's exact output and the checker's
    approval; returns the reference's stats."""
    if cluster_env is None:
        monkeypatch.delenv("TRT_LBVH_CLUSTER", raising=False)
    else:
        monkeypatch.setenv("TRT_LBVH_CLUSTER", cluster_env)
    rc, nodes, nn, order, depth = gpu_build(v, leaf_num)
    assert rc == 0, _abi.load_build().trt_build_last_error()
    st = {}
    r_nodes, r_nn, r_order, r_depth = R.build(v, leaf_num, cluster_env, st)
    assert np.array_equal(order, r_order), f"order differs at positions {np.flatnonzero(order != r_order)[:8].tolist()} ({st})"
    assert nn == r_nn, (nn, r_nn, st)
    assert nodes == r_nodes, _first_difference(nodes, r_nodes) + f" ({st})"
    assert depth == r_depth, (depth, r_depth, st)
    B.check_bvh(v, nodes, nn, order, leaf_num, depth)
    return st


BLOCK_EDGES = [0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 3073]


@pytest.mark.parametrize("cluster", ["0", None])
@pytest.mark.parametrize("leaf", [1, 2, 8, 15])
def test_block_edges(leaf, cluster, monkeypatch):
    """One block of 1024 positions (the root finished in K4a), one position past it (K4b), two and three blocks; n <= leaf_num (one
    root with an empty child1), leaf_num + 1 (the smallest real tree)."""
    for n in sorted(set(BLOCK_EDGES + [leaf, leaf + 1])):
        st = compare(L.soup(n, seed=n), leaf, cluster, monkeypatch)
        want = "one leaf" if n <= leaf else "radix" if cluster == "0" or n <= R.cluster_for(n, leaf) else "clusters"
        assert st["path"] == want, (n, st)


@pytest.mark.parametrize("n,cluster,leaf,want_cluster", [
    (49_999, None, 2, 2), (50_000, None, 2, 16),            # the default tiers either side of 50 k
    (300_000, "128", 2, 128), (300_000, "2048", 2, 2048),   # the 4 M and 10 M tiers' cluster sizes, through the override
    (20_000, "3", 8, 8), (20_000, "8", 8, 8),              # an override below leaf_num is raised to it; equal to it
    (3_000, "5000", 2, 5000),                              # a cluster as large as the scene: the radix tree as it is
])
def test_cluster_tiers_and_overrides(n, cluster, leaf, want_cluster, monkeypatch):
    st = compare(L.soup(n, seed=11), leaf, cluster, monkeypatch)
    assert st["cluster"] == want_cluster
    assert st["path"] == ("radix" if n <= want_cluster else "clusters")


@pytest.mark.parametrize("cluster", [None, "0"])
@pytest.mark.parametrize("case", list(L.HOSTILE))
def test_hostile_inputs(case, cluster, monkeypatch):
    """Equal codes, flat axes, the 63-level chain, overflowing and infinite extents, coordinates beyond 3e38, tiny extents, -0.0.
    The builder's output only: trt_create may refuse some of these trees (infinite coordinates)."""
    st = compare(L.HOSTILE[case](), 2, cluster, monkeypatch)
    if cluster is None:  # which of TopBuilder's fallbacks these inputs reach (restated in tests/test_lbvh_reference.py)
        if case in ("identical_100k", "ladder_x60", "flat_yz"):
            assert st["top_median_at_depth"] > 0, st
        if case in ("near_1e30", "infinities", "extent_overflow"):
            assert st["top_fallback"] > 0, st


@pytest.mark.parametrize("name,n,leaf", [("back", None, 2), ("back", None, 8), ("veach-mis", None, 2), ("veach-mis", None, 8),
                                         ("staircase", None, 2), ("staircase", None, 8), ("soup", 50_000, 2), ("blob", 150_000, 2),
                                         ("blob", 1_000_000, 2)])
def test_real_scenes(name, n, leaf, monkeypatch):
    compare(L.scene_vertices(name, n), leaf, None, monkeypatch)


def test_two_builds_are_identical(monkeypatch):
    """A tree with spanning nodes (K4b rounds) and clusters, and a larger one: built twice, the same bytes."""
    monkeypatch.delenv("TRT_LBVH_CLUSTER", raising=False)
    for v in (L.ladder(60), L.soup(300_000, seed=12)):
        a, b = gpu_build(v, 2), gpu_build(v, 2)
        assert a[0] == 0 and b[0] == 0
        assert a[1] == b[1] and a[2:3] == b[2:3] and np.array_equal(a[3], b[3]) and a[4] == b[4]


@pytest.mark.parametrize("cluster", [None, "0"])
def test_node_capacity_is_exact(cluster, monkeypatch):
    """node_capacity == n_nodes is enough; one less is TRT_EINVAL naming node_capacity, on both paths."""
    if cluster is None:
        monkeypatch.delenv("TRT_LBVH_CLUSTER", raising=False)
    else:
        monkeypatch.setenv("TRT_LBVH_CLUSTER", cluster)
    v = L.soup(5000, seed=13)
    rc, nodes, nn, order, depth = gpu_build(v, 2)
    assert rc == 0
    rc2, nodes2, nn2, order2, depth2 = gpu_build(v, 2, capacity=nn)
    assert rc2 == 0 and (nodes2, nn2, depth2) == (nodes, nn, depth) and np.array_equal(order2, order)
    rc3 = gpu_build(v, 2, capacity=nn - 1)[0]
    assert rc3 == TRT_EINVAL and b"node_capacity" in _abi.load_build().trt_build_last_error()
