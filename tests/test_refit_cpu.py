"""Geometry updates without a GPU: the new entries exist on every layer, and Scene.set_vertices (the host restatement the GPU tests compare
against) refits the flat tree exactly as refit_ref.py's numpy restatement of the rule says, rebuilds the light tables as the loader would,
and leaves a scene it is given its own vertices bit for bit as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from hostsim_lib import OCT_DT
import raygen
import refit_ref as RR
import scene_util as SU
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "trt.h")).read()
    for sym in ("trt_update_geometry", "trt_update_geometry_device"):
        assert re.search(r"\bint %s\(" % sym, hdr)
        assert sym in _abi.HIP_SYMBOLS
        assert hasattr(_abi.load_hip(), sym)
    assert "typedef struct trt_geometry_update" in hdr and re.search(r"TRT_K_REFIT = 7\b", hdr)
    assert _abi.TRT_K_REFIT == 7 < _abi.TRT_MAX_KERNELS
    host_hdr = open(os.path.join(ROOT, "include", "trt_host.h")).read()
    assert re.search(r"\bint trth_scene_set_vertices\(", host_hdr)
    assert "trth_scene_set_vertices" in _abi.HOST_SYMBOLS and hasattr(_abi.load_host(), "trth_scene_set_vertices")
    assert _abi.load_hip().trt_abi_version() == 5
    # the struct as the C compiler lays it out: four pointers and two 32-bit counts
    assert C.sizeof(_abi.GeometryUpdate) == 4 * C.sizeof(C.c_void_p) + 8


def test_null_arguments_are_einval_without_a_device():
    lib = _abi.load_hip()
    upd = _abi.GeometryUpdate()
    assert lib.trt_update_geometry(None, C.byref(upd), 0, None) == 1
    assert lib.trt_update_geometry_device(None, C.byref(upd), 0, None, None) == 1
    assert lib.trt_update_geometry(None, None, 0, None) == 1
    assert b"null" in lib.trt_last_error()


def _scene(name):
    if name == "soup":
        return T.Scene.named("soup", 64, 36, n=5000)
    if name == "blob":
        return T.Scene.named("blob", 64, 36, n=20000)
    if name.endswith("@ref8"):
        return SU.load_with_reference_tree(name[:-5], 64, 36)
    return T.Scene.named(name, 64, 36, leaf_num=2)


def _moved(name, s):
    v = s.arrays()["tri_v"]
    return RR.jitter(v) if name == "soup" else RR.smooth_displace(v)


@pytest.mark.parametrize("foreign", ["as built", "renumbered", "shrunk"])
@pytest.mark.parametrize("name", ["back", "veach-mis", "staircase", "soup", "blob", "back@ref8", "veach-mis@ref8"])
def test_set_vertices_matches_the_restatement(name, foreign):
    s = _scene(name)
    if foreign == "renumbered":
        SU.renumber_nodes_reversed(s)
    elif foreign == "shrunk":
        SU.shrink_some_boxes(s, 8)
    before = RR.nodes_of(s)
    v = _moved(name, s)
    want, order = RR.refit(before, v)
    s.set_vertices(v)
    got = RR.nodes_of(s)
    assert RR.same_bits(s.arrays()["tri_v"], v)
    assert RR.same_bits(got["child0"], before["child0"]) and RR.same_bits(got["child1"], before["child1"])
    assert RR.same_bits(got, want), "a node differs from the numpy restatement of the rule"
    assert RR.root_paths_contain(got, v)


def test_round_trip_leaves_every_builders_tree_and_light_tables_as_they_were():
    for make in (lambda: T.Scene.named("back", 64, 36, builder="sweep"), lambda: T.Scene.named("staircase", 64, 36, builder="binned"),
                 lambda: T.Scene.named("veach-mis", 64, 36), lambda: T.Scene.named("lamps", 64, 36), lambda: SU.load_with_reference_tree("back", 64, 36)):
        s = make()
        f = s.flat.contents
        a = s.arrays()
        nodes = RR.nodes_of(s)
        lt = C.string_at(f.light_tris, f.n_light_tris * C.sizeof(_abi.LightTri))
        li = C.string_at(f.lights, f.n_lights * C.sizeof(_abi.Light))
        s.set_vertices(a["tri_v"], a["tri_vn"])
        f = s.flat.contents
        assert RR.same_bits(RR.nodes_of(s), nodes)
        assert C.string_at(f.light_tris, f.n_light_tris * C.sizeof(_abi.LightTri)) == lt
        assert C.string_at(f.lights, f.n_lights * C.sizeof(_abi.Light)) == li


def _room(tmp_path, name, lamp_y):
    lines, faces = [], []
    b = 1
    for (x0, x1, z0, z1, y, mat) in ((-2, 2, -2, 2, -1.0, "white"), (-0.5, 0.25, -0.5, 0.5, lamp_y, "lamp"), (0.25, 0.75, -0.25, 0.5, lamp_y, "lamp")):
        lines += [f"v {x0} {y} {z0}", f"v {x1} {y} {z0}", f"v {x1} {y} {z1}", f"v {x0} {y} {z1}"]
        faces += [f"usemtl {mat}", f"f {b}/1/1 {b+1}/1/1 {b+2}/1/1", f"f {b}/1/1 {b+2}/1/1 {b+3}/1/1"]
        b += 4
    obj = "\n".join(lines + ["vt 0 0", "vn 0 1 0"] + faces) + "\n"
    SU.write_scene(tmp_path, name, obj, SU.MTL_BASIC, lights=[("lamp", (10, 10, 10))])
    return SU.load(tmp_path, name, leaf_num=1)


def test_moved_light_tables_equal_those_of_a_scene_loaded_with_the_moved_vertices(tmp_path):
    s = _room(tmp_path, "room_a", 1.0)
    a = s.arrays()
    lamp = [i for i in range(s.info["n_materials"]) if s.material_name(i) == "lamp"]
    v = a["tri_v"].copy()
    sel = np.isin(a["tri_mat"], lamp)
    assert sel.sum() == 4
    v[sel, :, 1] = np.float32(0.375)
    s.set_vertices(v)
    t = _room(tmp_path, "room_b", 0.375)
    fs, ft = s.flat.contents, t.flat.contents
    assert fs.n_lights == ft.n_lights == 1 and fs.n_light_tris == ft.n_light_tris == 4
    assert C.string_at(fs.light_tris, 4 * C.sizeof(_abi.LightTri)) == C.string_at(ft.light_tris, 4 * C.sizeof(_abi.LightTri))
    assert C.string_at(fs.lights, C.sizeof(_abi.Light)) == C.string_at(ft.lights, C.sizeof(_abi.Light))
    assert s.light_area(0) == t.light_area(0)


def test_set_vertices_refuses_non_finite_and_wrong_sizes():
    s = T.Scene.named("back", 64, 36)
    v = s.arrays()["tri_v"]
    nodes = RR.nodes_of(s)
    bad = v.copy()
    bad[3, 1, 2] = np.inf
    with pytest.raises(T.TrtError):
        s.set_vertices(bad)
    with pytest.raises(T.TrtError):
        s.set_vertices(v[:-1])
    assert RR.same_bits(RR.nodes_of(s), nodes) and RR.same_bits(s.arrays()["tri_v"], v)


def test_oracle_renders_a_moved_scene_and_a_moved_back_one_as_before():
    s = T.Scene.named("back", 32, 24)
    p = T.make_params(32, 24, 4, T.SEED_BACK)
    a = s.arrays()
    img0, _ = O.render(s.flat, p)
    v, sel = RR.move_inner_object(s)
    s.set_vertices(v)
    img1, _ = O.render(s.flat, p)
    assert np.abs(img1 - img0).max() > 0  # the cube went somewhere else
    o, d = raygen.primary_rays(s, 32, 24)
    t, tri, uv = O.trace(s.flat, o, d)[:3]
    assert sel[tri[tri >= 0]].any()
    s.set_vertices(a["tri_v"], a["tri_vn"])
    img2, _ = O.render(s.flat, p)
    assert RR.same_bits(img2, img0)


# ---- the per-node functions of the 4-wide and 8-wide passes on the host (tests/refit/librefit_cpu.so) ------------------------------------
WIDE_DT = np.dtype([("box", "<f4", (6, 4)), ("ref", "<u4", 4), ("pad", "<u4", 4)])
assert WIDE_DT.itemsize == 128 and OCT_DT.itemsize == 80
LEAF = RR.LEAF


def _refit_lib():
    lib = C.CDLL(os.path.join(ROOT, "tests", "refit", "librefit_cpu.so"))
    lib.refit_cpu_wide.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.refit_cpu_oct.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


def _bvh2_boxes_by_range(nodes):
    """(first triangle, last triangle) of every child of every reached node -> its stored box (lo, hi), bytes."""
    out = {}

    def walk(i):
        lo_t, hi_t = None, None
        for k in (0, 1):
            ref = int(nodes["child%d" % k][i])
            if ref & LEAF:
                first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
                r = (first, first + count - 1) if count else None
            else:
                r = walk(ref)
            if r is not None:
                out[r] = np.concatenate([nodes["lo%d" % k][i], nodes["hi%d" % k][i]]).tobytes()
                lo_t = r[0] if lo_t is None else min(lo_t, r[0])
                hi_t = r[1] if hi_t is None else max(hi_t, r[1])
        return None if lo_t is None else (lo_t, hi_t)

    import sys
    sys.setrecursionlimit(10000)
    walk(0)
    return out


def _wide_case(s, v, greedy=0):
    lib = _refit_lib()
    nodes = RR.nodes_of(s)
    n2, n = len(nodes), s.flat.contents.n_tris
    v = np.ascontiguousarray(v, np.float32)
    out2 = np.zeros(n2, RR.NODE_DT)
    before, after = np.zeros(n2, WIDE_DT), np.zeros(n2, WIDE_DT)
    nw = lib.refit_cpu_wide(nodes.ctypes.data, n2, n, v.ctypes.data, greedy, out2.ctypes.data, before.ctypes.data, after.ctypes.data, n2)
    assert nw > 0
    return nodes, out2, before[:nw], after[:nw]


@pytest.mark.parametrize("greedy", [0, 1])
@pytest.mark.parametrize("name", ["back", "veach-mis", "blob", "back@ref8"])
def test_wide_refit_slots_are_the_bvh2_boxes_and_the_original_vertices_reproduce_the_collapse(name, greedy):
    s = _scene(name)
    v0 = s.arrays()["tri_v"]
    nodes, out2, before, after = _wide_case(s, v0, greedy)
    assert RR.same_bits(out2, nodes) and RR.same_bits(after, before), "a refit with the tree's own vertices must reproduce collapseBvh's nodes"
    v = _moved(name, s)
    nodes, out2, before, after = _wide_case(s, v, greedy)
    want, _ = RR.refit(nodes, v)
    assert RR.same_bits(out2, want)
    assert RR.same_bits(after["ref"], before["ref"])
    by_range = _bvh2_boxes_by_range(want)

    def slot_range(i, k):
        ref = int(after["ref"][i][k])
        if ref & LEAF:
            first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
            return (first, first + count - 1) if count else None
        rs = [r for r in (slot_range(ref, j) for j in range(4) if after["ref"][ref][j] != 0xFFFFFFFF) if r]
        return (min(r[0] for r in rs), max(r[1] for r in rs)) if rs else None

    checked = 0
    for i in range(len(after)):
        for k in range(4):
            if after["ref"][i][k] == 0xFFFFFFFF:
                continue
            r = slot_range(i, k)
            if r is None:
                continue
            assert after["box"][i][:, k].tobytes() == by_range[r], f"4-wide node {i} slot {k}: not the BVH2 box of triangles {r}"
            checked += 1
    assert checked >= len(after)


def _oct_case(s, v):
    lib = _refit_lib()
    nodes = RR.nodes_of(s)
    n2, n = len(nodes), s.flat.contents.n_tris
    v0 = np.ascontiguousarray(s.arrays()["tri_v"], np.float32)
    v = np.ascontiguousarray(v, np.float32)
    cap = 4 * n2 + 8
    out2 = np.zeros(n2, RR.NODE_DT)
    before, after = np.zeros(cap, OCT_DT), np.zeros(cap, OCT_DT)
    slot_box, tri_orig = np.zeros((cap, 8, 6), np.float32), np.zeros((cap, 8), np.int32)
    no = lib.refit_cpu_oct(nodes.ctypes.data, n2, n, v0.ctypes.data, v.ctypes.data, out2.ctypes.data, before.ctypes.data, after.ctypes.data,
                           slot_box.ctypes.data, tri_orig.ctypes.data, cap)
    assert no > 0, no
    return nodes, out2, before[:no], after[:no], slot_box[:no], tri_orig[:no]


@pytest.mark.parametrize("name", ["veach-mis", "blob", "staircase", "veach-mis@ref8"])
def test_oct_refit_contains_the_exact_boxes_and_uses_buildocts_quantiser(name):
    s = _scene(name)
    nodes, out2, before, after, slot_box, tri_orig = _oct_case(s, s.arrays()["tri_v"])
    assert RR.same_bits(after, before), "a refit with the tree's own vertices must reproduce buildOct's nodes: one quantiser"
    v = _moved(name, s)
    nodes, out2, before, after, slot_box, tri_orig = _oct_case(s, v)
    want, _ = RR.refit(nodes, v)
    assert RR.same_bits(out2, want)
    for f in ("child_base", "tri_base", "meta"):
        assert RR.same_bits(after[f], before[f])
    assert RR.same_bits(after["ew"] >> 24, before["ew"] >> 24)
    # the restatement's box of the leaf every triangle lies in
    leaf_of = {}
    for i in range(len(want)):
        for k in (0, 1):
            ref = int(want["child%d" % k][i])
            if ref & LEAF:
                for t in range(ref & 0x07FFFFFF, (ref & 0x07FFFFFF) + ((ref >> 27) & 15)):
                    leaf_of[t] = np.concatenate([want["lo%d" % k][i], want["hi%d" % k][i]])
    meta = after["meta"]
    used = meta != 0
    inner = used & ((meta & 0x1F) >= 24)
    imask = (after["ew"] >> 24).astype(np.uint32)
    n_checked = 0
    for i in range(len(after)):
        for sl in range(8):
            if not used[i, sl]:
                continue
            if inner[i, sl]:
                c = int(after["child_base"][i]) + bin(int(imask[i]) & ((1 << sl) - 1)).count("1")
                cu = used[c]
                exact = np.concatenate([slot_box[c][cu][:, :3].min(0), slot_box[c][cu][:, 3:].max(0)])
            else:
                exact = leaf_of[int(tri_orig[i, sl])]  # a split leaf's slots carry the whole leaf's box
            assert slot_box[i, sl].tobytes() == exact.astype(np.float32).tobytes()
            n_checked += 1
    assert n_checked > len(after)
    # stored box contains exact box, in binary64: p + qlo s <= lo, p + qhi s >= hi
    for a in range(3):
        e = ((after["ew"] >> (8 * a)) & 0xFF).astype(np.int64)
        sc = np.ldexp(1.0, (e - 127).astype(np.int32))[:, None]
        p = after["p"][:, a].astype(np.float64)[:, None]
        qlo, qhi = after["q"][:, a, :].astype(np.float64), after["q"][:, 3 + a, :].astype(np.float64)
        lo, hi = slot_box[:, :, a].astype(np.float64), slot_box[:, :, 3 + a].astype(np.float64)
        assert np.all((p + qlo * sc <= lo)[used]) and np.all((p + qhi * sc >= hi)[used])
        assert np.all(qlo[~used] == 255) and np.all(qhi[~used] == 0)
