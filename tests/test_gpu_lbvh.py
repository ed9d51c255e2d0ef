"""The GPU BVH builder (include/trt_build.h, libtrt_lbvh.so) — MI355X only.

What is checked: the tree it returns is one trt_create accepts (validateBvh: indices, every triangle in exactly one leaf, post-BVH
triangle order), with leaves of <= leaf_num triangles and nested boxes (so it qualifies for the 8-wide nodes); the triangles it
orders are a permutation; and — the parity bar of every caller's tree — the HIP path on that tree is bit-identical to the oracle
walking the same tree, hits and images.  Quality is reported against the host SAH builder (node visits per ray), not asserted to
a bar an LBVH cannot meet: it is the fast builder, not the good one.
"""
import ctypes as C
import os

import numpy as np
import pytest

import bvh_check as B
import oracle_lib as O
import raygen
import tinyraytracing_amd as T

pytestmark = pytest.mark.gpu
LEAF_BIT = 0x80000000


def _tree_facts(s):
    f = s.flat.contents
    nodes = np.ctypeslib.as_array(C.cast(f.nodes, C.POINTER(C.c_uint32)), shape=(f.n_nodes, 16))
    refs = nodes[:, 12:14].reshape(-1)
    leaves = refs[(refs & LEAF_BIT) != 0]
    counts = (leaves >> 27) & 15
    return f.n_nodes, int(counts.max()), int(counts.sum())


@pytest.mark.parametrize("cluster", [None, "0", "48"])
@pytest.mark.parametrize("name,kw,leaf", [("veach-mis", {}, 2), ("staircase", {}, 2), ("staircase", {}, 8), ("soup", {"n": 50000}, 1), ("blob", {"n": 150000}, 2)])
def test_lbvh_tree_is_valid_and_renders_like_the_oracle_on_it(name, kw, leaf, cluster, monkeypatch):
    """cluster: TRT_LBVH_CLUSTER — default (the top of the tree by SAH over clusters of <= 2048 triangles), "0" (the radix tree as it is),
    "48" (many small clusters: a deep SAH top, single-triangle clusters, clusters that are leaves)."""
    if cluster is not None:
        monkeypatch.setenv("TRT_LBVH_CLUSTER", cluster)
    s = T.Scene.named(name, 96, 54, leaf_num=leaf, builder="lbvh", **kw)
    n_tris = s.info["n_triangles"]
    n_nodes, biggest_leaf, in_leaves = _tree_facts(s)
    assert biggest_leaf <= leaf and in_leaves == n_tris and n_nodes <= max(n_tris, 2) - 1
    r = T.Renderer(s, 0)  # trt_create: validateBvh, the collapses
    lo, hi = raygen.scene_bounds(s)
    org, dirs = raygen.random_rays(100000, lo - 1, hi + 1, seed=5)
    t0, tri0, uv0 = O.trace(s.flat, org, dirs)
    t1, tri1, uv1 = r.trace_closest(org, dirs)
    assert np.array_equal(tri0, tri1) and np.array_equal(t0, t1) and np.array_equal(uv0, uv1)
    p = T.make_params(96, 54, 4, 321)
    img, st = r.render(p)
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(img, ref)
    assert (st.rays_camera, st.rays_shadow, st.rays_indirect) == (ost.rays_camera, ost.rays_shadow, ost.rays_indirect)
    assert st.inner_node_bytes == 80, "nested boxes: the tree takes the 8-wide nodes (leaves of more than 3 triangles as several slots)"
    r.close()
    s.close()


def test_lbvh_on_coincident_triangles_and_tiny_inputs():
    """Equal Morton codes (every triangle twice: the soup added two times with one seed) are told apart by position: a valid tree, the
    same image as the oracle on it.  A scene that fits one leaf gets the root with an empty second child, like the host builder."""
    d = os.path.join(T.SCENES_DIR, "back")
    s = T.Scene.load(os.path.join(d, "back.xml"), os.path.join(d, "back.obj"), os.path.join(d, "back.mtl"), d, 64, 36)
    s._check(s._lib.trth_scene_drop_tris(s._h, 6, 12))
    s._check(s._lib.trth_scene_add_soup(s._h, 7, 3000))
    s._check(s._lib.trth_scene_add_soup(s._h, 7, 3000))
    s.build_bvh(2, "lbvh")
    r = T.Renderer(s, 0)
    p = T.make_params(64, 36, 4, 9)
    img, _ = r.render(p)
    ref, _ = O.render(s.flat, p)
    assert np.array_equal(img, ref)
    r.close()
    s.close()
    p = T.make_params(64, 36, 4, 9)
    for drop, leaf, one_leaf in ((0, 15, False), (12, 15, True)):
        s2 = T.Scene.load(os.path.join(d, "back.xml"), os.path.join(d, "back.obj"), os.path.join(d, "back.mtl"), d, 64, 36)
        if drop:
            s2._check(s2._lib.trth_scene_drop_tris(s2._h, 6, drop))
        s2.build_bvh(leaf, "lbvh")
        n_nodes, biggest, total = _tree_facts(s2)
        assert biggest <= leaf and total == s2.info["n_triangles"]
        if one_leaf:
            assert s2.info["n_triangles"] <= leaf and n_nodes == 1
        r = T.Renderer(s2, 0)
        img, _ = r.render(p)
        assert np.array_equal(img, O.render(s2.flat, p)[0])
        r.close()
        s2.close()


def test_lbvh_quality_and_speed_are_on_record(capsys):
    """Node visits and triangle tests per ray of the LBVH tree against the host SAH tree on the 150 k-triangle mesh (COUNT kernels), and the
    builder's own time: printed for the record (tools/lbvh_cost.py does the 10 M case), with a loose sanity bound only."""
    res = {}
    for b in ("auto", "lbvh", "radix"):
        if b == "radix":
            os.environ["TRT_LBVH_CLUSTER"] = "0"
        s = T.Scene.named("blob", 320, 180, leaf_num=2, builder="lbvh" if b == "radix" else b, n=150000)
        os.environ.pop("TRT_LBVH_CLUSTER", None)
        r = T.Renderer(s, 0)
        _, st = r.render(T.make_params(320, 180, 4, 11, flags=T.TRT_FLAG_COUNT))
        rays = st.rays_camera + st.rays_shadow + st.rays_indirect
        res[b] = ((st.inner_visits[0] + st.inner_visits[1]) / rays, (st.tri_tests[0] + st.tri_tests[1]) / rays, getattr(s, "build_ms", None))
        r.close()
        s.close()
    with capsys.disabled():
        print(f"\nblob-150k: visits / tests per ray  SAH {res['auto'][0]:.2f} / {res['auto'][1]:.2f}   LBVH with SAH top {res['lbvh'][0]:.2f} / {res['lbvh'][1]:.2f}   "
              f"plain radix tree {res['radix'][0]:.2f} / {res['radix'][1]:.2f}   build (device ms, call ms) {res['lbvh'][2]} / {res['radix'][2]}")
    # round 4: clusters of 16 on scenes of 50-500 k triangles: +1.2 % node visits against the host SAH tree (round 3's 2048: +11.7 %; profiles/r04_lbvh_quality.txt);
    # the bar is VERDICT r03's "blob-150k <= +5 %" with the slack of this test's smaller image
    assert res["lbvh"][0] < 1.06 * res["auto"][0] and res["radix"][0] < 3.0 * res["auto"][0]
    # staircase: Morton pairs under a full SAH (clusters of 2 below 50 k triangles): +8.0 % (round 3: +20.7 %; the verdict's bar: <= +10 %)
    st_res = {}
    for b in ("auto", "lbvh"):
        s = T.Scene.named("staircase", 320, 180, leaf_num=2, builder=b)
        r = T.Renderer(s, 0)
        _, st = r.render(T.make_params(320, 180, 4, 11, flags=T.TRT_FLAG_COUNT))
        st_res[b] = (st.inner_visits[0] + st.inner_visits[1]) / (st.rays_camera + st.rays_shadow + st.rays_indirect)
        r.close()
        s.close()
    with capsys.disabled():
        print(f"staircase: visits per ray  SAH {st_res['auto']:.2f}   LBVH with SAH top {st_res['lbvh']:.2f} ({(st_res['lbvh'] / st_res['auto'] - 1) * 100:+.1f} %)")
    assert st_res["lbvh"] < 1.12 * st_res["auto"]


def test_config5_ten_million_triangles_built_on_the_device_tiles_vs_oracle():
    """Config 5's scene at full size with the tree built on the GPU (the device part: tens of milliseconds; the times are printed for the record),
    a tree tests/bvh_check.py accepts (its triangles in the adopted leaf order), a tree trt_create accepts and collapses into 8-wide nodes, tiles of the 4K image bit-identical to the oracle on the same tree."""
    d = os.path.join(T.SCENES_DIR, "back")
    s = T.Scene.load(os.path.join(d, "back.xml"), os.path.join(d, "back.obj"), os.path.join(d, "back.mtl"), d, 3840, 2160)
    s._check(s._lib.trth_scene_drop_tris(s._h, 6, 12))
    s._check(s._lib.trth_scene_add_blob(s._h, T.SEED_BLOB, 10_000_000))
    import torch
    before = torch.cuda.current_device()
    s.build_bvh(2, "lbvh")
    assert torch.cuda.current_device() == before  # trt_build_lbvh restores the caller's device on every exit path
    assert s.info["n_triangles"] >= 10_000_000
    print(f"\nconfig 5, tree built on the device: {s.build_ms[0]:.1f} ms of kernels and host SAH top, {s.build_ms[1]:.1f} ms for the call with its copies")
    assert s.build_ms[0] < 500.0, s.build_ms  # device part only, loosely (tens of ms); the call's wall clock depends on the host's share of cores and PCIe
    # the tree itself, by the builder-independent checker: exact padded boxes, every triangle in one leaf, post-BVH order, the reported depth
    f = s.flat.contents
    B.check_bvh(np.ctypeslib.as_array(f.tri_v, shape=(f.n_tris * 9,)), f.nodes, f.n_nodes, np.arange(f.n_tris), 2, f.bvh_depth)
    r = T.Renderer(s, 0)
    try:
        for (x0, y0) in ((1900, 1000), (2300, 1500)):
            pt = T.make_params(3840, 2160, 16, T.SEED_BLOB, tile=(x0, y0, x0 + 16, y0 + 8))
            img, st = r.render(pt)
            ref, ost = O.render(s.flat, pt)
            assert np.array_equal(img, ref), (x0, y0)
            assert st.rays == ost.rays and st.inner_node_bytes == 80
    finally:
        r.close()
        s.close()


def test_cli_gpu_bvh(tmp_path):
    """tinyrt --gpu-bvh: the C++ host entry (trt::render with RenderOpts::gpu_builder) builds on the device, gathers the flat arrays through the
    returned permutation (the Triangle objects stay where they are) and renders; the PNG has the bytes of the same render through the Python harness on the same device-built tree."""
    import subprocess
    exe = os.path.join(T.REPO_ROOT, "tinyraytracing_amd", "lib", "tinyrt")
    d = os.path.join(T.SCENES_DIR, "staircase")
    out = str(tmp_path / "cli.png")
    r = subprocess.run([exe, d, os.path.join(d, "staircase.mtl"), os.path.join(d, "staircase.xml"), os.path.join(d, "staircase.obj"), "4", "--width", "96", "--height", "54",
                        "--leaf", "2", "--gpu-bvh", "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    s = T.Scene.named("staircase", 96, 54, leaf_num=2, builder="lbvh")
    rr = T.Renderer(s, 0)
    img, _ = rr.render(T.make_params(96, 54, 4, 0x5EED0001))
    ref = str(tmp_path / "py.png")
    T.imshow(img, ref)
    assert open(out, "rb").read() == open(ref, "rb").read()
    rr.close()
    s.close()


def test_builder_refuses_what_it_cannot_return():
    """A node array that is too small is an error with a message, not an overrun; the reported depth is what trt_create measures on the tree."""
    from tinyraytracing_amd import _abi
    b = _abi.load_build()
    rng = np.random.default_rng(2)
    n = 5000
    v = (rng.random((n, 3, 3), dtype=np.float32) * 0.05 + rng.random((n, 1, 3), dtype=np.float32)).astype(np.float32).reshape(-1)
    order = np.empty(n, np.uint32)
    nn, depth = C.c_uint32(0), C.c_uint32(0)
    small = (_abi.BvhNode * 16)()
    rc = b.trt_build_lbvh(v.ctypes.data_as(C.POINTER(C.c_float)), n, 2, 0, small, 16, C.byref(nn), order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(depth), None)
    assert rc == 1 and b"node_capacity" in b.trt_build_last_error()
    nodes = (_abi.BvhNode * (n - 1))()
    ms = (C.c_double * 2)()
    rc = b.trt_build_lbvh(v.ctypes.data_as(C.POINTER(C.c_float)), n, 2, 0, nodes, n - 1, C.byref(nn), order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(depth), ms)
    assert rc == 0 and 0 < nn.value <= n - 1 and sorted(order.tolist()) == list(range(n)) and ms[1] >= ms[0] > 0
    # the depth it reports = the longest chain of inner nodes from the root
    kids = {}
    for i in range(nn.value):
        kids[i] = [c for c in (nodes[i].child0, nodes[i].child1) if not (c & LEAF_BIT)]
    deepest, stack = 0, [(0, 1)]
    while stack:
        i, d = stack.pop()
        deepest = max(deepest, d)
        stack.extend((c, d + 1) for c in kids[i])
    assert deepest == depth.value
