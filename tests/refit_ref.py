"""The box rule of a geometry update (include/trt.h, trt_update_geometry) restated in numpy, independent of the C++: a leaf's box is
min / max of its triangles' coordinates -+ float32(0.001), an inner child's box the union of that child's two boxes, a leaf of 0 triangles
keeps its box.  Walks from the root by child references, so it does not care how the nodes are numbered; nodes no path reaches stay."""
import ctypes as C

import numpy as np

PAD = np.float32(0.001)
LEAF = 0x80000000
NODE_DT = np.dtype([("lo0", "<f4", 3), ("hi0", "<f4", 3), ("lo1", "<f4", 3), ("hi1", "<f4", 3), ("child0", "<u4"), ("child1", "<u4"), ("reserved", "<u4", 2)])


def nodes_of(scene):
    """The flat tree of a Scene as a structured numpy array (a copy)."""
    f = scene.flat.contents
    return np.frombuffer(C.string_at(f.nodes, f.n_nodes * 64), NODE_DT).copy()


def refit(nodes, tri_v):
    """-> a copy of `nodes` with the boxes of the rule for the vertices tri_v [n, 3, 3] (float32)."""
    out = nodes.copy()
    v = np.asarray(tri_v, np.float32).reshape(-1, 3, 3)
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        for c in (int(out["child0"][i]), int(out["child1"][i])):
            if not c & LEAF:
                stack.append(c)
    assert len(set(order)) == len(order)
    for i in reversed(order):  # children before parents
        for k in (0, 1):
            ref = int(out["child%d" % k][i])
            if ref & LEAF:
                first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
                if count == 0:
                    continue
                p = v[first:first + count].reshape(-1, 3)
                lo, hi = p.min(0) - PAD, p.max(0) + PAD
            else:
                lo = np.minimum(out["lo0"][ref], out["lo1"][ref])
                hi = np.maximum(out["hi0"][ref], out["hi1"][ref])
            out["lo%d" % k][i], out["hi%d" % k][i] = lo.astype(np.float32), hi.astype(np.float32)
    return out, order


def root_paths_contain(nodes, tri_v):
    """Every triangle lies inside every box on its root path."""
    v = np.asarray(tri_v, np.float32).reshape(-1, 3, 3)
    stack = [(0, np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32))]
    while stack:
        i, lo_in, hi_in = stack.pop()  # the tightest box above: with nested boxes, containment in it is containment in all
        for k in (0, 1):
            ref = int(nodes["child%d" % k][i])
            lo, hi = nodes["lo%d" % k][i], nodes["hi%d" % k][i]
            if not (np.all(lo >= lo_in) and np.all(hi <= hi_in)):
                return False
            if ref & LEAF:
                first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
                if count and not (np.all(v[first:first + count] >= lo) and np.all(v[first:first + count] <= hi)):
                    return False
            else:
                stack.append((ref, lo, hi))
    return True


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


# ---- moves used by the CPU and the GPU tests -------------------------------------------------------------------------------------
def smooth_displace(tri_v, amp=12.0):
    """A smooth function of position: shared vertices stay shared."""
    v = np.asarray(tri_v, np.float32)
    d = np.stack([np.sin(v[..., 1] * 0.013) * amp, np.cos(v[..., 2] * 0.011 + 1.0) * amp * 0.5, np.sin(v[..., 0] * 0.017 + 2.0) * amp], -1)
    return (v + d.astype(np.float32)).astype(np.float32)


def jitter(tri_v, seed=5, amp=3.0):
    rng = np.random.default_rng(seed)
    v = np.asarray(tri_v, np.float32)
    return (v + rng.uniform(-amp, amp, v.shape).astype(np.float32)).astype(np.float32)


def move_material(scene, name, delta=None, rotate_deg=0.0):
    """The scene's vertices with the triangles of material `name` rotated about the y axis through their centre and translated."""
    a = scene.arrays()
    v = a["tri_v"].copy()
    ids = [i for i in range(scene.info["n_materials"]) if scene.material_name(i) == name]
    sel = np.isin(a["tri_mat"], ids)
    assert sel.any(), name
    p = v[sel].reshape(-1, 3)
    c = p.mean(0)
    t = np.float32(np.deg2rad(rotate_deg))
    R = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]], np.float32)
    p = (p - c) @ R.T + c + (np.zeros(3, np.float32) if delta is None else np.asarray(delta, np.float32))
    v[sel] = p.astype(np.float32).reshape(-1, 3, 3)
    return v, sel


def move_inner_object(scene, delta=(25.0, 0.0, -30.0), rotate_deg=20.0, margin=20.0):
    """`back`-like rooms: the triangles that keep `margin` away from the room's x and z bounds and from its ceiling (the cube standing on the
    floor of `back`), rotated about the y axis through their centre and translated.  -> (vertices, mask of the moved triangles)."""
    a = scene.arrays()
    v = a["tri_v"].copy()
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    sel = ((v[..., 0].min(1) > lo[0] + margin) & (v[..., 0].max(1) < hi[0] - margin) & (v[..., 2].min(1) > lo[2] + margin) &
           (v[..., 2].max(1) < hi[2] - margin) & (v[..., 1].max(1) < hi[1] - margin))
    assert sel.any()
    q = v[sel].reshape(-1, 3)
    c = q.mean(0)
    t = np.float32(np.deg2rad(rotate_deg))
    R = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]], np.float32)
    v[sel] = ((q - c) @ R.T + c + np.asarray(delta, np.float32)).astype(np.float32).reshape(-1, 3, 3)
    return v, sel
