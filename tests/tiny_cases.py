"""A deterministic corpus of tiny one-light scenes for the wave-uniform walk (trt_kernels.h: uniformWalkImpl / flushPending, k_tail's uniformWalk,
traceQueueBinned, fusedWalk): geometry on which the tie rule, a full candidate queue, the size limits the route is chosen by, a tree whose boxes do
not nest and cameras that break the walks' wave votes DECIDE the result.  Imported by tests/test_tiny_cases_cpu.py (the corpus is valid and decisive,
on the oracle alone) and tests/test_gpu_tiny_cases.py (every route of the kernels, route asserted, bits equal).

The stage is a floor, a lamp above it and a STACK: coincident triangles (the same nine coordinates, so every ray gets bit-equal t from each) that
face the camera.  Every case has exactly one light ("lamp": a triangle of the stack that is emissive carries that material too), at most 64
triangles unless it is a one-beyond case, and five materials.

The builders reorder triangles, so a case describes itself from the built flat scene (describe()): which triangles are tied, which leaf and node
each is in, which are emissive — never from the order of the OBJ file.  rule_winner() states the reference's two-level tie rule
(interactBVHNode, bvh.cpp:211-229: inside a leaf the first candidate stays unless a later one is emissive; traverseBVH, bvh.cpp:168-172: between
the two children the first wins iff it is emissive) on that description, for rays that meet every triangle of the stack.
"""
import ctypes as C
import os

import numpy as np

import scene_util as SU
import tinyraytracing_amd as T
from tinyraytracing_amd._abi import BvhNode

LEAF_BIT = 0x80000000
RADIANCE = (20.0, 16.0, 12.0)

MTL = """newmtl white
Kd 0.7 0.7 0.7
Ks 0 0 0
Ns 1
Ni 1
newmtl red
Kd 0.8 0.1 0.1
Ks 0 0 0
Ns 1
Ni 1
newmtl green
Kd 0.1 0.8 0.1
Ks 0 0 0
Ns 1
Ni 1
newmtl blue
Kd 0.1 0.1 0.8
Ks 0 0 0
Ns 1
Ni 1
newmtl lamp
Kd 0 0 0
Ks 0 0 0
Ns 1
Ni 1
"""

# ---- geometry: a triangle is (material, three vertices, normal); written with coordinates of its own, so coincident ones are the same floats
FLOOR = [("white", ((-3, 0, -2), (3, 0, 4), (3, 0, -2)), (0, 1, 0)), ("white", ((-3, 0, -2), (-3, 0, 4), (3, 0, 4)), (0, 1, 0))]
LAMP = [("lamp", ((-1, 3.2, 1), (1, 3.2, 1), (1, 3.2, 3)), (0, -1, 0)), ("lamp", ((-1, 3.2, 1), (1, 3.2, 3), (-1, 3.2, 3)), (0, -1, 0))]
STACK_V = ((-1.5, 0.2, 0), (1.5, 0.2, 0), (0, 2.6, 0))
EYE, LOOKAT = (0, 1.4, 6), (0, 1.2, 0)


def stack(mats, v=STACK_V):
    return [(m, v, (0, 0, 1)) for m in mats]


def small(k, z=-1.5):
    """The k-th of a row of little triangles that stand on the floor behind the stack (fill for the trees of 33 and 64 triangles)"""
    x = -2.9 + 0.1 * k
    return ("blue" if k % 2 else "green", ((x, 0.05, z), (x + 0.08, 0.05, z), (x + 0.04, 0.4, z)), (0, 0, 1))


def obj_text(tris):
    lines, faces, normals = ["vt 0 0"], [], []
    for k, (mat, v, n) in enumerate(tris):
        if n not in normals:
            normals.append(n)
            lines.append("vn %r %r %r" % tuple(float(x) for x in n))
        for p in v:
            lines.append("v %r %r %r" % tuple(float(x) for x in p))
        ni = normals.index(n) + 1
        faces += [f"usemtl {mat}", f"f {3 * k + 1}/1/{ni} {3 * k + 2}/1/{ni} {3 * k + 3}/1/{ni}"]
    return "\n".join(lines + faces) + "\n"


def adopt_tree(scene, tree, pad=1e-3):
    """Gives an unbuilt scene the BVH `tree`: a list of triangle indices (file order) is a leaf, a pair (child0, child1) an inner node.  Nodes are
    numbered parents first, child0's subtree before child1's; a leaf's box is its triangles' box padded by `pad`, an inner child's box the union of
    that child's two boxes; the triangles take the order of the leaves.  Adopted the way a caller's own tree arrives (caterpillar_tree does the same
    for a chain)."""
    n = scene.info["n_triangles"]
    v = np.empty(n * 9, np.float32)
    scene._check(scene._lib.trth_scene_vertices(scene._h, v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
    v = v.reshape(n, 3, 3)
    lo, hi = v.min(axis=1) - np.float32(pad), v.max(axis=1) + np.float32(pad)
    rows, order = [], []

    def place(t):
        if isinstance(t, list):
            assert 1 <= len(t) <= 15
            first = len(order)
            order.extend(t)
            return LEAF_BIT | (len(t) << 27) | first, lo[t].min(axis=0), hi[t].max(axis=0), 0
        me = len(rows)
        rows.append(None)
        a, b = place(t[0]), place(t[1])
        rows[me] = (a, b)
        return me, np.minimum(a[1], b[1]), np.maximum(a[2], b[2]), 1 + max(a[3], b[3])

    root = place(tree)
    assert root[0] == 0 and sorted(order) == list(range(n)), "the tree must hold every triangle once"
    nodes = (BvhNode * len(rows))()
    for nd, (a, b) in zip(nodes, rows):
        nd.lo0[:], nd.hi0[:], nd.child0 = a[1].tolist(), a[2].tolist(), a[0]
        nd.lo1[:], nd.hi1[:], nd.child1 = b[1].tolist(), b[2].tolist(), b[0]
    perm = np.array(order, np.uint32)
    scene._check(scene._lib.trth_scene_adopt_bvh(scene._h, nodes, len(rows), perm.ctypes.data_as(C.POINTER(C.c_uint32)), root[3]))
    scene._built = True
    return scene


def chain(leaves):
    """A caterpillar: node i has child0 = leaves[i] and child1 = node i + 1; the last node holds the last two leaves"""
    return (leaves[0], chain(leaves[1:])) if len(leaves) > 2 else (leaves[0], leaves[1])


def balanced(leaves):
    h = len(leaves) // 2
    return leaves[0] if len(leaves) == 1 else (balanced(leaves[:h]), balanced(leaves[h:]))


def build(tmp, name, tris, tree, w=33, h=25, fovy=40.0, eye=EYE, lookat=LOOKAT):
    """tree: a leaf size for the host builder (SAH; coincident triangles keep their file order), or a tree for adopt_tree"""
    d = os.path.join(str(tmp), name)
    os.makedirs(d, exist_ok=True)
    SU.write_scene(d, name, obj_text(tris), MTL, lights=[("lamp", RADIANCE)], w=w, h=h, fovy=fovy, eye=eye, lookat=lookat)
    if isinstance(tree, int):
        return SU.load(d, name, leaf_num=tree)
    s = T.Scene.load(os.path.join(d, name + ".xml"), os.path.join(d, name + ".obj"), os.path.join(d, name + ".mtl"), d)
    return adopt_tree(s, tree)


# ---- what a built scene says about itself
class Description:
    """tri_v [n, 9], mat [n] (material names), emissive [n], leaf [n] = (node, child slot), leaves {(node, slot): (first, count)}, groups: lists of
    triangle indices with bit-equal coordinates (two or more), largest first"""


def describe(scene):
    f = scene.flat.contents
    d = Description()
    n = d.n_tris = int(f.n_tris)
    d.n_nodes = int(f.n_nodes)
    d.tri_v = np.ctypeslib.as_array(C.cast(f.tri_v, C.POINTER(C.c_float)), (n, 9)).copy()
    ids = [int(f.tri_mat[i]) for i in range(n)]
    d.mat = [scene.material_name(m) for m in ids]
    d.emissive = [bool(f.materials[m].is_emissive) for m in ids]
    d.n_lights = int(f.n_lights)
    d.leaf, d.leaves, d.children = [None] * n, {}, []
    for k in range(d.n_nodes):
        refs = (int(f.nodes[k].child0), int(f.nodes[k].child1))
        d.children.append(refs)
        for c, ref in enumerate(refs):
            if ref & LEAF_BIT:
                first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
                d.leaves[(k, c)] = (first, count)
                for i in range(first, first + count):
                    d.leaf[i] = (k, c)
    by_v = {}
    for i in range(n):
        by_v.setdefault(d.tri_v[i].tobytes(), []).append(i)
    d.groups = sorted((g for g in by_v.values() if len(g) > 1), key=len, reverse=True)
    return d


def rule_winner(d, group):
    """The triangle the reference returns for a ray that meets every triangle of `group` at one distance and nothing nearer (and passes the boxes
    above them): leaf by leaf the first stays unless a later one is emissive (then the last emissive one), and at an inner node child0's result
    wins iff it is emissive."""
    group = set(group)

    def visit(ref):
        if ref & LEAF_BIT:
            first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
            best = None
            for i in range(first, first + count):
                if i in group and (best is None or d.emissive[i]):
                    best = i
            return best
        r1, r2 = visit(d.children[ref][0]), visit(d.children[ref][1])
        if r1 is None or r2 is None:
            return r2 if r1 is None else r1
        return r1 if d.emissive[r1] else r2

    return visit(0)


def centre_rays(scene, w, h):
    """The rays through the pixel centres (the reference's grid) -> (org, dir) [h * w, 3], pixel y * w + x"""
    return T.center_rays(scene.flat.contents.camera, w, h)


# ---- the cases
class Case:
    """name; make(tmp) -> the scene; control(tmp) -> the changed copy of the negative control (or None); kind: what the case states of itself
    (tests/test_tiny_cases_cpu.py checks it per kind); qualifies: trt_create takes the wave-uniform walk, 8-byte records, the binned walk, the fused
    bounce 0; w, h, spp of its renders."""

    def __init__(self, name, kind, make, control=None, qualifies=True, w=33, h=25, spp=4, **want):
        self.name, self.kind, self.make, self.control, self.qualifies, self.w, self.h, self.spp, self.want = name, kind, make, control, qualifies, w, h, spp, want

    def __repr__(self):
        return self.name


CASES = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


GLOW = (2.0, 9.0, 30.0)


def make_glow(scene, name="blue"):
    """Makes material `name` emissive IN PLACE in the flat scene without making it a light: a second kind of emitter under ONE light (a scene the
    loaders do not produce and the C-ABI accepts; the radiance a path keeps is the hit material's, pathTracing.cpp:9-12).  Two emissive triangles at one
    distance then show in the picture which of them won."""
    f = scene.flat.contents
    m = next(f.materials[i] for i in range(f.n_materials) if scene.material_name(i) == name)
    m.is_emissive = 1
    m.radiance[:] = GLOW
    return scene


def _stage(name, mats, tree, glow=False, **kw):
    def make(tmp):
        s = build(tmp, name, FLOOR + LAMP + stack(mats), tree, **kw)
        return make_glow(s) if glow else s
    return make


# ties inside a leaf: the stack is triangles 4 and 5 of the file; with leaf size 15 the whole scene is one leaf
# ties between leaves under one node: floor | (lamp | (A | B)); under two inner nodes: (floor | A) | (B | lamp)
IN_LEAF = 15
UNDER_ONE_NODE = ([0, 1], ([2, 3], ([4], [5])))
UNDER_TWO_NODES = (([0, 1], [4]), ([5], [2, 3]))
PAIRS = {"red-green": ("red", "green"), "green-red": ("green", "red"), "red-lamp": ("red", "lamp"), "lamp-red": ("lamp", "red")}


def _control_of(pair):
    """The negative control of a tied pair: the two materials swapped; where one is the lamp the emitter wins in either order, so there a plain material
    takes its place (the picture must show that the emissive triangle, not its partner, was the hit)"""
    return tuple("white" if m == "lamp" else m for m in pair) if "lamp" in pair else pair[::-1]


for pid, pair in PAIRS.items():
    _add(f"ties-in-leaf-{pid}", "tie", _stage(f"til-{pid}", pair, IN_LEAF), control=_stage(f"til-{pid}-control", _control_of(pair), IN_LEAF), leaves=(1, 1))
for pid, pair in PAIRS.items():
    _add(f"ties-between-leaves-{pid}", "tie", _stage(f"tbl-{pid}", pair, UNDER_ONE_NODE), control=_stage(f"tbl-{pid}-control", _control_of(pair), UNDER_ONE_NODE),
         leaves=(2, 2))
# two emissive triangles: triangles of the one light are one material and no picture can tell them apart, so the second emitter is make_glow's
for pid, (a, b) in {"lamp-glow": ("lamp", "blue"), "glow-lamp": ("blue", "lamp")}.items():
    _add(f"ties-between-leaves-{pid}", "tie", _stage(f"tbl-{pid}", (a, b), UNDER_ONE_NODE, glow=True),
         control=_stage(f"tbl-{pid}-swapped", (b, a), UNDER_ONE_NODE, glow=True), leaves=(2, 2), both_emissive=True)
_add("ties-between-subtrees-red-green", "tie", _stage("tbs-red-green", ("red", "green"), UNDER_TWO_NODES),
     control=_stage("tbs-green-red", ("green", "red"), UNDER_TWO_NODES), leaves=(2, 2), nodes=2)

# nine coincident triangles: every ray that hits them has nine candidates, so a lane's queue of four is flushed twice inside the leaf (or between
# the leaves).  The winner is the only emissive one: the second, the sixth or the ninth candidate; the control puts a plain material in its place.
NINE = {"winner-2": ("red", "lamp", "green", "blue", "green", "blue", "green", "blue", "green"),
        "winner-6": ("red", "green", "blue", "green", "blue", "lamp", "green", "blue", "green"),
        "winner-9": ("red", "green", "blue", "green", "blue", "green", "blue", "green", "lamp")}
for vid, mats in NINE.items():
    plain = tuple("white" if m == "lamp" else m for m in mats)
    _add(f"deep-stack-{vid}", "stack", _stage(f"ds-{vid}", mats, IN_LEAF), control=_stage(f"ds-{vid}-plain", plain, IN_LEAF), leaves=(1, 1), position=mats.index("lamp"))
for vid, mats in NINE.items():
    plain = tuple("white" if m == "lamp" else m for m in mats)
    _add(f"deep-stack-across-leaves-{vid}", "stack", _stage(f"dsl-{vid}", mats, 2), control=_stage(f"dsl-{vid}-plain", plain, 2), leaves=(5, 9), position=mats.index("lamp"))


def _node31(n_small, name):
    """A caterpillar of n_small + 5 inner nodes on n_small + 6 triangles, the stack (red, green) in the last node's two leaves"""
    tris = FLOOR + LAMP + [small(k) for k in range(n_small)] + stack(("red", "green"))
    return lambda tmp: build(tmp, name, tris, chain([[k] for k in range(len(tris))]))


def _node31_swapped(tmp):
    tris = FLOOR + LAMP + [small(k) for k in range(27)] + stack(("green", "red"))
    return build(tmp, "node31-swapped", tris, chain([[k] for k in range(len(tris))]))


_add("node-31", "limit", _node31(27, "node31"), control=_node31_swapped, n_nodes=32, n_tris=33, winner_node=31)
_add("one-beyond-33-nodes", "beyond", _node31(28, "node32"), qualifies=False, n_nodes=33, n_tris=34)


def _tri63(n_small, name, mats=("red", "lamp")):
    """floor, lamp, n_small little triangles (a leaf of exactly 15, then leaves of 2 and one of 3 or 4), the stack (red, lamp) in the last leaf: with
    58 little ones 64 triangles under 24 inner nodes, and the emissive triangle 63 wins the stack's rays by the rule inside a leaf"""
    tris = FLOOR + LAMP + [small(k) for k in range(n_small)] + stack(mats)
    s0 = 4
    leaves = [[0, 1], [2, 3], list(range(s0, s0 + 15))]
    rest = list(range(s0 + 15, s0 + n_small))
    while len(rest) > 4:
        leaves.append(rest[:2])
        rest = rest[2:]
    leaves += [rest, [s0 + n_small, s0 + n_small + 1]]
    return lambda tmp: build(tmp, name, tris, balanced(leaves))


_add("tri-63", "limit", _tri63(58, "tri63"), control=_tri63(58, "tri63-plain", ("red", "white")), n_tris=64, max_nodes=32, winner_tri=63, leaf_of_15=True)
_add("one-beyond-65-triangles", "beyond", _tri63(59, "tri64"), qualifies=False, n_tris=65, max_nodes=32)

# boxes that do not nest: the 64-triangle tree with stored boxes of inner children pulled in (scene_util.shrink_some_boxes); seed and amount are
# chosen so that the shrinking changes first hits (tests/test_tiny_cases_cpu.py asserts that it does)
SHRINK = dict(n=6, seed=3, amount=0.35)


def _shrunk(tmp):
    s = _tri63(58, "shrunk")(tmp)
    assert SU.shrink_some_boxes(s, **SHRINK) > 0
    return s


_add("boxes-that-do-not-nest", "shrunk", _shrunk, control=_tri63(58, "unshrunk"))

# cameras.  The vertex eye: a pair of coincident triangles at coordinates of 7e4 (tests/test_hostsim_parity.py _vertex_eye_scene: the pad of the boxes is below
# one ulp there, so the vertex IS a corner of its leaf's box), the eye ON their third vertex, looking horizontally: llc + vertical * t - eye cancels to an
# exactly zero d.y for whole rows of pixels, whose rays start on a box plane (0 * inf in the slab test) and end on a second pair 3000 away, the backdrop, under a lamp.
FAR_V = ((71246.609375, 79342.484375, -881.6929931640625), (72923.890625, 77794.8359375, 476.5187683105469), (74036.484375, 79794.8046875, -4266.68115234375))
FAR_LOOKAT = (72738.140625, 79794.8046875, -1562.1846923828125)  # eye + 3000 * normalize(-1951, 0, 4064)
FAR_BACKDROP = ((73549.4921875, 79194.8046875, -1172.6812744140625), (71926.7890625, 79194.8046875, -1951.6881103515625), (72738.140625, 80894.8046875, -1562.1846923828125))
FAR_NORMAL = (0.43278154730796814, -0.0, -0.9014988541603088)  # of the backdrop: towards the eye
FAR_LAMP = ((73787.59375, 80594.8046875, -3055.048095703125), (73246.6953125, 80594.8046875, -3314.717041015625), (73257.4765625, 80594.8046875, -2643.983154296875))  # halfway, 800 above the line of sight, facing down
VERTEX_EYE = dict(w=63, h=47, fovy=12.0, eye=FAR_V[2], lookat=FAR_LOOKAT)


def _vertex_eye(mats, name):
    tris = stack(("red", "green"), FAR_V) + [(m, FAR_BACKDROP, FAR_NORMAL) for m in mats] + [("lamp", FAR_LAMP, (0, -1, 0))]
    return lambda tmp: build(tmp, name, tris, ([0, 1], ([2, 3], [4])), **VERTEX_EYE)


_add("camera-eye-on-a-vertex", "camera-vertex", _vertex_eye(("red", "green"), "veye"), control=_vertex_eye(("green", "red"), "veye-swapped"), w=63, h=47)
INSIDE = dict(eye=(0, 1.0, 0.0006), lookat=(0, 0.4, -3))  # inside the padded box of the stack's leaf, 0.0006 in front of its plane
_add("camera-eye-inside-the-stack-box", "tie", _stage("inside", ("red", "green"), UNDER_ONE_NODE, **INSIDE),
     control=_stage("inside-swapped", ("green", "red"), UNDER_ONE_NODE, **INSIDE), leaves=(2, 2), eye_in_leaf_box=True)
_add("camera-turned-away", "camera-away", _stage("away", ("red", "green"), UNDER_ONE_NODE, eye=EYE, lookat=(0, 1.4, 12)))
# grazing: the eye 0.0015 in front of the stack's plane and 2 away from its centre (1e-3 rad), a view of one degree along the plane
GRAZE = dict(eye=(-2.0, 0.8, 0.0015), lookat=(-1.2, 0.8, 0), fovy=1.0, w=63, h=47)
_add("grazing", "grazing", _stage("graze", ("red", "green"), UNDER_ONE_NODE, **GRAZE), control=_stage("graze-swapped", ("green", "red"), UNDER_ONE_NODE, **GRAZE),
     leaves=(2, 2), w=63, h=47, max_angle=2e-3)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def aimed_rays(scene, n=4096, seed=0x7E):
    """`n` rays aimed at the tied triangles (points inside them, the groups in turn) from random origins around them; a third of the rays have one
    direction component set to zero (raySpecial: the literal slab test, the queue kernels' parked-ray rewalk)"""
    d = describe(scene)
    rng = np.random.default_rng(seed)
    tris = np.stack([d.tri_v[g[0]].reshape(3, 3).astype(np.float64) for g in d.groups])
    k = np.arange(n)
    tri = tris[k % len(tris)]
    extent = np.abs(tri - tri.mean(axis=1, keepdims=True)).max(axis=(1, 2))
    target = np.einsum("nk,nkc->nc", rng.dirichlet((1.0, 1.0, 1.0), n), tri)
    org = target + rng.normal(size=(n, 3)) * 2.0 * extent[:, None]
    dirs = (target - org).astype(np.float32)
    zero = k % 3 == 0
    dirs[zero, (k[zero] // 3) % 3] = 0.0
    return org.astype(np.float32), dirs
