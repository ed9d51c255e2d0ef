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


def shrink_about_centroid(tri_v, sel, factor=0.5):
    """The triangles `sel` (a mask) scaled by `factor` about the centroid of their vertices: an object at half its size, so every box above it
    must get smaller — a box an update leaves as it was is then a loose box, and a loose box is more traversal work.  One formula per
    coordinate, so a vertex gets the same position in every triangle that shares it."""
    v = np.asarray(tri_v, np.float32).copy()
    sel = np.asarray(sel, bool)
    assert sel.any()
    p = v[sel].reshape(-1, 3)
    c = p.mean(0, dtype=np.float64).astype(np.float32)
    v[sel] = (c + (p - c) * np.float32(factor)).astype(np.float32).reshape(-1, 3, 3)
    return v


def central_object(tri_v, fraction=0.5):
    """Mask of the triangles that lie wholly in the middle `fraction` of the scene's bounds on every axis: the part shrink_about_centroid shrinks
    on scenes that are one object (blob) or have no movable one by name."""
    v = np.asarray(tri_v, np.float32)
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    mid, half = (lo + hi) * np.float32(0.5), (hi - lo) * np.float32(0.5 * fraction)
    sel = (np.abs(v - mid) <= half).all((1, 2))
    assert sel.any() and not sel.all()
    return sel


def light_far_away(scene, light=0, distance=40.0):
    """The scene's vertices with the triangles of light `light`'s material translated by `distance` scene diagonals, from the light's centroid through
    the centre of the scene's bounds and out on the other side: far out, so the light's box and every box above its leaves grow by that much and
    moving back must shrink them again — and a light box that kept the far position as well (a union) holds the whole way there, the scene
    included, so no shadow ray starts outside it.  -> (vertices, mask of the moved triangles)."""
    a = scene.arrays()
    v = a["tri_v"].copy()
    f = scene.flat.contents
    assert light < f.n_lights
    sel = a["tri_mat"] == f.lights[light].mat
    assert sel.any() and not sel.all()
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    way = ((lo + hi) * 0.5 - v[sel].reshape(-1, 3).mean(0)).astype(np.float64)
    way /= np.linalg.norm(way)
    v[sel] = (v[sel] + (way * distance * np.linalg.norm(hi - lo)).astype(np.float32)).astype(np.float32)
    return v, sel


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
