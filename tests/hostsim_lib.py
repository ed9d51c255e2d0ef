"""ctypes binding of tests/hostsim/libhostsim.so (device-side path functions compiled for the CPU)."""
import ctypes as C
import os

import numpy as np

import tinyraytracing_amd as T
from tinyraytracing_amd._abi import Params, SceneFlat

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libhostsim.so")
fp = C.POINTER(C.c_float)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.hostsim_render.argtypes = [C.POINTER(SceneFlat), C.POINTER(Params), fp, C.POINTER(C.c_uint64)]
        L.hostsim_trace.argtypes = [C.POINTER(SceneFlat), C.c_uint64, fp, fp, fp, C.POINTER(C.c_int32), fp, C.POINTER(C.c_uint64)]
        L.hostsim_set_node_kind.argtypes = [C.c_int]
        L.hostsim_compressible.argtypes = [C.POINTER(SceneFlat)]
        L.hostsim_trace_counts.argtypes = [C.POINTER(SceneFlat), C.c_int, C.c_uint64, fp, fp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.hostsim_oct_fallbacks.restype = C.c_uint64
        L.hostsim_oct_fallbacks.argtypes = [C.POINTER(SceneFlat), C.c_uint64, fp, fp]
        L.hostsim_oct_info.argtypes = [C.POINTER(SceneFlat), C.POINTER(C.c_uint64)]
        L.hostsim_tree_hashes.argtypes = [C.POINTER(SceneFlat), C.c_uint, C.POINTER(C.c_uint64)]
        L.hostsim_query.argtypes = [C.POINTER(SceneFlat), C.c_int, C.c_int, C.c_uint64, fp, fp, fp, fp, C.POINTER(C.c_int32), fp]
        _lib = L
    return _lib


def set_node_kind(nk):
    """0 = exact 4-wide nodes, 1 = compressed 80-B 8-wide nodes (trt_oct.h) wherever the tree qualifies; returns the old setting."""
    return lib().hostsim_set_node_kind(int(nk))


def compressible(flat):
    return bool(lib().hostsim_compressible(flat))


# what the entries return when a walk was ended by a range check (TRT_WALK_CHECK, trt_path.h): it would have read out of range on the GPU
BREACH = 2


def _ok(rc, what):
    assert rc != BREACH, f"{what}: a traversal left its tree, its triangles or the GPU driver's stack (TRT_WALK_CHECK)"
    assert rc == 0, f"{what}: returned {rc}"


def render(flat, p):
    rows = len(T.rows_selected(p))
    out = np.empty((rows, p.x1 - p.x0, 3), np.float32)
    rays = (C.c_uint64 * 3)()
    _ok(lib().hostsim_render(flat, C.byref(p), out.ctypes.data_as(fp), rays), "hostsim_render")
    return out, [int(x) for x in rays]


def trace(flat, org, direction):
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    n = org.shape[0]
    t = np.empty(n, np.float32)
    tri = np.empty(n, np.int32)
    uv = np.empty((n, 2), np.float32)
    cnt = (C.c_uint64 * 2)()
    rc = lib().hostsim_trace(flat, n, org.ctypes.data_as(fp), direction.ctypes.data_as(fp), t.ctypes.data_as(fp),
                             tri.ctypes.data_as(C.POINTER(C.c_int32)), uv.ctypes.data_as(fp), cnt)
    _ok(rc, "hostsim_trace")
    return t, tri, uv, [int(x) for x in cnt]


def query(flat, org, direction, bound=None, any=False, form=0):
    """The ray queries on the device code: (t, tri, uv) per ray, a miss as (TRT_INF, -1, 0, 0); with `any` only tri >= 0 means anything.
    bound: the per-ray bound the library searches below (query_ref.bound of t_max), None = unbounded.  form 0: what the per-lane
    drivers walk (node kind of set_node_kind); form 1: what k_trace_fix walks (the literal walk or the exact form on the 4-wide nodes)."""
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    n = org.shape[0]
    b = None if bound is None else np.ascontiguousarray(bound, np.float32).reshape(n)
    t = np.empty(n, np.float32)
    tri = np.empty(n, np.int32)
    uv = np.empty((n, 2), np.float32)
    rc = lib().hostsim_query(flat, int(form), int(bool(any)), n, org.ctypes.data_as(fp), direction.ctypes.data_as(fp),
                             None if b is None else b.ctypes.data_as(fp), t.ctypes.data_as(fp), tri.ctypes.data_as(C.POINTER(C.c_int32)), uv.ctypes.data_as(fp))
    _ok(rc, "hostsim_query")
    return t, tri, uv


def trace_counts(flat, node_kind, org, direction):
    """Per-ray work of the closest-hit search on node kind 0 / 1: (inner-node visits, triangle tests)."""
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    n = org.shape[0]
    v = np.zeros(n, np.uint32)
    t = np.zeros(n, np.uint32)
    u32 = C.POINTER(C.c_uint32)
    rc = lib().hostsim_trace_counts(flat, int(node_kind), n, org.ctypes.data_as(fp), direction.ctypes.data_as(fp), v.ctypes.data_as(u32), t.ctypes.data_as(u32))
    assert rc != 1, "node kind 1 asked of a tree that does not qualify"
    _ok(rc, "hostsim_trace_counts")
    return v, t


# ---- a handle created on one scene and updated (tests/test_refit_work_cpu.py, tests/test_gpu_refit_work.py) ------------------------------------------
NO_LONGER_OCT = 3  # what refit_trace_counts reports when an update left an 8-wide node that no longer qualifies and go_on is not set
# the driver faults tests/refit/refit_loops.h can plant (refitloops::Order; LIGHT_UNION: the previous light boxes are kept and united with the new ones)
ALTER_NONE, ALTER_SKIP_DEEPEST, ALTER_SHALLOWEST_FIRST, ALTER_LIGHT_UNION = 0, 1, 2, 3


class RefitWork:
    """rc: 0 or NO_LONGER_OCT (then nothing else is set); kind: the node kind the rays were walked on; t, tri, uv: the records; visits, tests:
    per-ray work of the first pass of the search, 0 for the rays with a zero direction component (the drivers hand those to k_trace_fix uncounted)."""

    def __init__(self, rc, kind=None, t=None, tri=None, uv=None, visits=None, tests=None):
        self.rc, self.kind, self.t, self.tri, self.uv, self.visits, self.tests = rc, kind, t, tri, uv, visits, tests

    def sums(self):
        return int(self.visits.sum(dtype=np.uint64)), int(self.tests.sum(dtype=np.uint64))


def refit_trace_counts(flat_before, tri_vs, flat_after, node_kind, org, direction, any=False, bound=None, go_on=False, alter=ALTER_NONE, light=-1):
    """What a handle created on `flat_before` (node kind 0 / 1) answers after being updated to each of tri_vs ([n, 3, 3] float32) in turn, and the
    work it does: HostScene::refit (tests/hostsim/hostsim.cpp) runs the per-node functions of csrc/trt_refit.h in place; flat_after is the scene
    Scene.set_vertices left for tri_vs[-1] (None with an empty list: the handle as created).  any: the occlusion query; bound: per-ray t_init;
    go_on: continue on node kind 0 when an 8-wide node no longer qualified, as the handle does; light >= 0 (node kind 1, closest): walk the rays as
    that light's parity-mode shadow rays.  -> RefitWork."""
    org, direction = _rays(org, direction)
    n = org.shape[0]
    vs = [np.ascontiguousarray(v, np.float32).reshape(-1, 3, 3) for v in tri_vs]
    n_tris = flat_before.contents.n_tris
    assert all(v.shape[0] == n_tris for v in vs) and (flat_after is not None or not vs)
    ptrs = (C.c_void_p * max(len(vs), 1))(*[v.ctypes.data for v in vs])
    b = None if bound is None else np.ascontiguousarray(bound, np.float32).reshape(n)
    t, tri, uv = np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 2), np.float32)
    visits, tests = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    kind = C.c_int32(-1)
    f = lib().hostsim_refit_trace_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(SceneFlat), C.c_uint32, _vp, C.POINTER(SceneFlat), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _vp, _vp, _vp, _vp, _vp,
                  _vp, _vp, _vp, C.POINTER(C.c_int32)]
    order, keep = (0, 1) if alter == ALTER_LIGHT_UNION else (int(alter), 0)
    rc = f(flat_before, len(vs), C.cast(ptrs, _vp), flat_after, int(node_kind), int(bool(any)), int(bool(go_on)), order, keep, int(light), n, org.ctypes.data,
           direction.ctypes.data, None if b is None else b.ctypes.data, t.ctypes.data, tri.ctypes.data, uv.ctypes.data, visits.ctypes.data, tests.ctypes.data, C.byref(kind))
    if rc == NO_LONGER_OCT:
        return RefitWork(rc)
    assert rc != 1, "bad arguments, or node kind 1 asked of a tree that does not qualify"
    _ok(rc, "hostsim_refit_trace_counts")
    return RefitWork(0, int(kind.value), t, tri, uv, visits, tests)


def oct_fallbacks(flat, org, direction):
    """How many of the rays end the oct traversal on a result that fails the check (and take the exact form)."""
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    return int(lib().hostsim_oct_fallbacks(flat, org.shape[0], org.ctypes.data_as(fp), direction.ctypes.data_as(fp)))


def oct_info(flat):
    """(nodes, levels, triangle records) of the oct tree, or None when the tree does not qualify."""
    out = (C.c_uint64 * 3)()
    return None if lib().hostsim_oct_info(flat, out) else tuple(int(x) for x in out)


def tree_hashes(flat, threads):
    """Hashes of the 4-wide trees (both collapses), the 8-wide tree, its triangle records and the leaf boxes, built with `threads` host threads."""
    out = (C.c_uint64 * 8)()
    assert lib().hostsim_tree_hashes(flat, int(threads), out) == 0
    return [int(x) for x in out]


# ---- node by node (tests/test_hostsim_node_claims.py, tests/test_gpu_node_claims.py): the entries work on arrays the caller owns ----------------------
OCT_DT = np.dtype([("p", "<f4", 3), ("ew", "<u4"), ("child_base", "<u4"), ("tri_base", "<u4"), ("meta", "u1", 8), ("q", "u1", (6, 8))])
assert OCT_DT.itemsize == 80
_vp = C.c_void_p


def _rays(org, direction):
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    assert org.shape == direction.shape
    return org, direction


def _call(name, *args):
    f = getattr(lib(), name)
    f.restype = C.c_int
    f.argtypes = [(_vp if isinstance(a, np.ndarray) or a is None else (C.c_uint64 if isinstance(a, int) else type(a))) for a in args]
    return f(*[(a.ctypes.data if isinstance(a, np.ndarray) else a) for a in args])


def oct_quantise_nodes(blo, bhi, kind):
    """Synthetic 8-wide nodes from octQuantise: blo / bhi [n, 8, 3] exact boxes, kind [n, 8] (0 empty, 1 inner, 2..4 a leaf slot of 1..3 triangles).
    -> (nodes [n] of OCT_DT, ok [n])."""
    blo, bhi = np.ascontiguousarray(blo, np.float32), np.ascontiguousarray(bhi, np.float32)
    kind = np.ascontiguousarray(kind, np.uint8)
    n = kind.shape[0]
    nodes, ok = np.zeros(n, OCT_DT), np.zeros(n, np.uint8)
    assert _call("hostsim_oct_quantise_nodes", n, blo, bhi, kind, nodes, ok) == 0
    return nodes, ok.astype(bool)


def oct_visit_cases(nodes, node, org, direction, cull):
    """octVisit per case -> words [n, 2] (node group word, triangle bits)."""
    org, direction = _rays(org, direction)
    node, cull = np.ascontiguousarray(node, np.uint32), np.ascontiguousarray(cull, np.float32)
    assert len(node) == len(cull) == len(org) and (len(node) == 0 or int(node.max()) < len(nodes))
    words = np.zeros((len(node), 2), np.uint32)
    assert _call("hostsim_oct_visit_cases", np.ascontiguousarray(nodes), len(node), node, org, direction, cull, words) == 0
    return words


def slot_ref(slot_box, node, org, direction):
    """boxTest of the exact box of every slot of node[i] -> (passes [n, 8] bool, entry [n, 8] float32)."""
    org, direction = _rays(org, direction)
    node = np.ascontiguousarray(node, np.uint32)
    slot_box = np.ascontiguousarray(slot_box, np.float32)
    assert len(node) == 0 or int(node.max()) < len(slot_box)
    ok, e = np.zeros((len(node), 8), np.uint8), np.zeros((len(node), 8), np.float32)
    assert _call("hostsim_slot_ref", slot_box, len(node), node, org, direction, ok, e) == 0
    return ok.astype(bool), e


def oct_descent(nodes, slot_box, org, direction, cap=256):
    """(node, ray) pairs the reference's descent of the oct tree reaches (a child iff boxTest passes its exact box) -> (node [m], ray [m])."""
    org, direction = _rays(org, direction)
    n = len(org)
    pair, cnt = np.zeros((n, cap), np.uint32), np.zeros(n, np.uint32)
    assert _call("hostsim_oct_descent", np.ascontiguousarray(nodes), np.ascontiguousarray(slot_box, np.float32), C.c_uint32(len(nodes)), n, org, direction,
                 C.c_uint32(cap), pair, cnt) == 0
    keep = np.arange(cap)[None, :] < np.minimum(cnt, cap)[:, None]
    return pair[keep], np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, cap))[keep]


def box_cases(box, org, direction):
    """boxTest / boxTestGlm per (box [n, 6] lo hi, ray) -> words [n, 3]: verdict bits, entry bits of each (one NaN)."""
    org, direction = _rays(org, direction)
    box = np.ascontiguousarray(box, np.float32).reshape(-1, 6)
    out = np.zeros((len(box), 3), np.uint32)
    assert _call("hostsim_box_cases", len(box), box, org, direction, out) == 0
    return out


def inner_step_cases(wnodes, node, org, direction, cull):
    """innerStep on 4-wide node node[i], empty stack -> words [n, 6]: cur, flag, pushes, the pushed references."""
    org, direction = _rays(org, direction)
    node, cull = np.ascontiguousarray(node, np.uint32), np.ascontiguousarray(cull, np.float32)
    assert len(node) == 0 or int(node.max()) < len(wnodes)
    out = np.zeros((len(node), 6), np.uint32)
    assert _call("hostsim_inner_step_cases", np.ascontiguousarray(wnodes), len(node), node, org, direction, cull, out) == 0
    return out


def leaf_floor(e, alpha):
    e, alpha = np.ascontiguousarray(e, np.float32), np.ascontiguousarray(np.broadcast_to(np.float32(alpha), np.shape(e)), np.float32)
    out = np.zeros(e.shape, np.float32)
    _call("hostsim_leaf_floor_v", e.size, e, alpha, out)
    return out


def cull_bound(b, alpha):
    b, alpha = np.ascontiguousarray(b, np.float32), np.ascontiguousarray(np.broadcast_to(np.float32(alpha), np.shape(b)), np.float32)
    out = np.zeros(b.shape, np.float32)
    _call("hostsim_cull_bound_v", b.size, b, alpha, out)
    return out


def scene_info(flat):
    """(leaf_alpha, nested, light boxes [n_lights, 6]) as a handle derives them."""
    n = flat.contents.n_lights
    info, lb = np.zeros(2, np.float32), np.zeros((max(n, 1), 6), np.float32)
    assert _call("hostsim_scene_info", flat, info, lb) == 0
    return np.float32(info[0]), bool(info[1]), lb[:n]


CHAIN_KINDS = ("boxTest fails", "entry below the box above", "t < floor(entry)", "entry > cull bound")


def cull_chain(flat, org, direction, t, tri):
    """The culling chain on results -> (counts dict, text of the first violations).  None for a tree whose boxes do not nest."""
    org, direction = _rays(org, direction)
    t, tri = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(tri, np.int32)
    counts, viol = np.zeros(6, np.uint64), np.zeros((16, 8), np.float64)
    rc = _call("hostsim_cull_chain", flat, len(t), org, direction, t, tri, counts, viol)
    if rc == 3:
        return None
    assert rc == 0, rc
    bad = [int(x) for x in counts[2:]]
    text = "; ".join(f"{CHAIN_KINDS[int(v[0])]}: tree {int(v[1])} node {int(v[2])} slot {int(v[3])} ray {int(v[4])} o={org[int(v[4])]} d={direction[int(v[4])]} "
                     f"entry={v[5]!r} t={v[6]!r} bound={v[7]!r}" for v in viol[:min(sum(bad), 16)])
    return {"rays": int(counts[0]), "boxes": int(counts[1]), "bad": bad}, text


def shadow_rays(flat, p, cap=1 << 22):
    """The parity-mode shadow rays of a render -> (org, dir, light)."""
    org, d, light = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32), np.zeros(cap, np.int32)
    f = lib().hostsim_shadow_rays
    f.restype = C.c_uint64
    f.argtypes = [C.POINTER(SceneFlat), C.POINTER(Params), C.c_uint64, _vp, _vp, _vp]
    n = int(f(flat, C.byref(p), cap, org.ctypes.data, d.ctypes.data, light.ctypes.data))
    assert n <= cap, n
    return org[:n], d[:n], light[:n]


def plane_filter(flat):
    """(words, log2 bits) of the plane filter planeFilterBuild makes for the scene's tree."""
    cap = max(1 << 5, (64 * flat.contents.n_nodes * 2) // 32 + 64)
    bits = np.zeros(cap, np.uint32)
    f = lib().hostsim_plane_filter
    f.restype = C.c_uint32
    f.argtypes = [C.POINTER(SceneFlat), _vp, C.c_uint64]
    lg = int(f(flat, bits.ctypes.data, cap))
    assert lg >= 10
    return bits[: (1 << lg) // 32].copy(), lg


def plane_maybe(bits, lg, axis, x):
    axis, x = np.ascontiguousarray(axis, np.int32), np.ascontiguousarray(x, np.float32)
    assert axis.shape == x.shape and len(bits) == (1 << lg) // 32
    out = np.zeros(x.shape, np.uint8)
    lib().hostsim_plane_maybe.restype = None
    lib().hostsim_plane_maybe.argtypes = [_vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp]
    lib().hostsim_plane_maybe(np.ascontiguousarray(bits, np.uint32).ctypes.data, lg, x.size, axis.ctypes.data, x.ctypes.data, out.ctypes.data)
    return out.astype(bool)


# ---- case by case (tests/test_shade_cases_cpu.py, tests/test_gpu_shade_cases.py): the sections of tools/shade_cases.h from the CPU build --------------------
MUTANTS_SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libshade_mutants.so")
_mutants = None


def make_material_dev(raw):
    """makeMaterialDev on [n] trt_material records (shade_cases.RAW_MAT_DT) -> [n] 96-B device records as bytes of shade_cases.MAT_DT."""
    raw = np.ascontiguousarray(raw)
    assert raw.dtype.itemsize == 64
    out = np.zeros((len(raw), 96), np.uint8)
    assert _call("hostsim_make_material_dev", len(raw), raw, out) == 0
    return out.reshape(-1)


def shade_case_words(file_bytes, n_words, mutant=None):
    """The output words of a whole case file (shade_cases.case_bytes), in the tool's order; None for a file the tool refuses (exit code 2).
    mutant 1..7: the same sections on the altered copies of tests/hostsim/shade_mutants.cpp (0: its copy of the headers' own)."""
    buf = np.frombuffer(file_bytes, np.uint8)
    out = np.zeros(n_words, np.uint32)
    if mutant is None:
        rc = _call("hostsim_shade_case_file", buf, len(buf), out, int(n_words))
    else:
        global _mutants
        if _mutants is None:
            _mutants = C.CDLL(MUTANTS_SO)
        f = _mutants.shade_mutant_case_file
        f.restype, f.argtypes = C.c_int, [C.c_int, _vp, C.c_uint64, _vp, C.c_uint64]
        rc = f(int(mutant), buf.ctypes.data, len(buf), out.ctypes.data, int(n_words))
    assert rc in (0, 2), rc
    return out if rc == 0 else None


def shade_digests(first=0, count=None):
    """Digests first .. first + count - 1 of the tool's digest mode (shade_cases.DIGEST_STREAMS)."""
    import shade_cases as SC
    count = SC.DIGEST_TOTAL - first if count is None else count
    out = np.zeros(count, np.uint64)
    f = lib().hostsim_shade_digests
    f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_uint64, _vp]
    assert f(int(first), int(count), out.ctypes.data) == 0
    return out
