"""An independent checker of a flat BVH (trt.h, trt_bvh_node) against the triangles it was built over.

It depends on no builder: every property follows from the node array, the triangle order and the vertices alone.
  - `order` is a permutation of the caller's triangles;
  - every node is reached from root 0 exactly once, and there are at most max(n, 2) - 1 of them;
  - every triangle position lies in exactly one leaf of 1..leaf_num triangles (the one exception: the empty child1 of a
    single-leaf root), and the triangles under child0 precede those under child1 (the post-BVH order trt_create relies on);
  - every child box is, bit for bit, fl(min - 0.001f) / fl(max + 0.001f) of the vertices of the triangles under it
    (bvh.cpp:31-40).  x -> fl(x - c) is monotone, so padding the exact bounds equals the minimum of the padded triangles:
    the rule is the same whichever way a builder pads.  The empty leaf of a single-leaf root carries child0's box, as the
    host builder gives it (and [-0.001, 0.001] for an empty scene);
  - the reported depth is the longest chain of inner nodes.
Vectorised level by level: config 5's 10 M-triangle tree takes well under a minute.
"""
import ctypes as C

import numpy as np

LEAF_BIT = 0x80000000
PAD = np.float32(0.001)
NODE_WORDS = 16  # 64 B: lo0, hi0, lo1, hi1 (3 floats each), child0, child1, reserved[2]


class BvhError(AssertionError):
    pass


def node_words(nodes, n_nodes):
    """(n_nodes, 16) uint32 view of a node array given as bytes, a numpy array or a ctypes array / pointer of trt_bvh_node."""
    if isinstance(nodes, (bytes, bytearray, memoryview)):
        a = np.frombuffer(nodes, np.uint32)
    elif isinstance(nodes, np.ndarray):
        a = nodes.view(np.uint32).reshape(-1)
    else:
        a = np.ctypeslib.as_array(C.cast(nodes, C.POINTER(C.c_uint32)), shape=(n_nodes * NODE_WORDS,))
    if a.size < n_nodes * NODE_WORDS:
        raise BvhError(f"node array holds {a.size // NODE_WORDS} nodes, n_nodes = {n_nodes}")
    return a[:n_nodes * NODE_WORDS].reshape(n_nodes, NODE_WORDS)


def _fail(msg):
    raise BvhError(msg)


def check_bvh(tri_v, nodes, n_nodes, order, leaf_num, depth):
    """tri_v: the vertices in the CALLER's order ((n, 9) or (n, 3, 3) float32); nodes/n_nodes: the tree; order[i] = caller index of
    the triangle at position i; depth: the reported depth.  Raises BvhError naming the first node or position that breaks a rule."""
    v = np.ascontiguousarray(tri_v, np.float32).reshape(-1, 3, 3)
    n = v.shape[0]
    order = np.asarray(order, np.int64).reshape(-1)
    if order.size != n:
        _fail(f"order has {order.size} entries for {n} triangles")
    if n and (order.min() < 0 or order.max() >= n or np.bincount(order, minlength=n).max() != 1):
        bad = np.flatnonzero(np.bincount(order[(order >= 0) & (order < n)], minlength=n) != 1)
        _fail(f"order is not a permutation (caller index {bad[:5].tolist()} not taken exactly once)")
    if n_nodes < 1 or n_nodes > max(n, 2) - 1:
        _fail(f"n_nodes = {n_nodes}, must be in 1..{max(n, 2) - 1}")
    w = node_words(nodes, n_nodes)
    boxes = w[:, :12].view(np.float32)
    refs = w[:, 12:14].astype(np.int64)
    is_leaf = (refs & LEAF_BIT) != 0
    first = refs & 0x07FFFFFF
    count = (refs >> 27) & 15
    single_leaf_root = bool(n_nodes == 1 and is_leaf[0].all() and n <= leaf_num)

    # ---- reachability, level by level (every inner reference is to a later level's node, visited once)
    inner_ref = np.where(is_leaf, -1, refs)
    if (inner_ref >= n_nodes).any():
        i, k = np.argwhere(inner_ref >= n_nodes)[0]
        _fail(f"node {i} child{k} refers to node {inner_ref[i, k]} of {n_nodes}")
    seen = np.zeros(n_nodes, np.int64)
    seen[0] = 1
    levels = [np.array([0], np.int64)]
    while True:
        kids = inner_ref[levels[-1]].reshape(-1)
        kids = kids[kids >= 0]
        if kids.size == 0:
            break
        np.add.at(seen, kids, 1)
        if seen[kids].max() > 1:
            _fail(f"node {int(kids[np.argmax(seen[kids] > 1)])} is reached more than once")
        levels.append(kids)
        if len(levels) > n_nodes:
            _fail("the tree has a cycle")
    if (seen == 0).any():
        _fail(f"node {int(np.flatnonzero(seen == 0)[0])} is not reachable from the root")
    if depth != len(levels):
        _fail(f"reported depth {depth}, the longest chain of inner nodes is {len(levels)}")

    # ---- leaves: sizes, and every position in exactly one of them
    empty_ok = np.zeros_like(is_leaf)
    if single_leaf_root:
        empty_ok[0, 1] = True
        if n == 0:
            empty_ok[0, 0] = True
    bad = is_leaf & ~empty_ok & ((count < 1) | (count > leaf_num))
    if bad.any():
        i, k = np.argwhere(bad)[0]
        _fail(f"node {i} child{k}: leaf of {count[i, k]} triangles (leaf_num {leaf_num})")
    if single_leaf_root and (first[0, 1] != 0 or count[0, 1] != 0 or (n == 0 and (first[0, 0] != 0 or count[0, 0] != 0))):
        _fail("node 0: the empty leaf of a single-leaf root must be (first 0, count 0)")
    real = is_leaf & ~((count == 0) & empty_ok)
    lf, lc = first[real], count[real]
    if (lf + lc > n).any():
        i, k = np.argwhere(real & (first + count > n))[0]
        _fail(f"node {i} child{k}: leaf [{first[i, k]}, +{count[i, k]}) runs past {n} triangles")
    cover = np.zeros(n + 1, np.int64)
    np.add.at(cover, lf, 1)
    np.add.at(cover, lf + lc, -1)
    cover = np.cumsum(cover)[:n]
    if n and (cover != 1).any():
        p = int(np.flatnonzero(cover != 1)[0])
        _fail(f"triangle position {p} lies in {int(cover[p])} leaves")

    # ---- bottom-up: each child's triangle range [lo, hi) and exact bounds; post-BVH order and boxes
    tb_lo = np.fmin(v[:, 0], np.fmin(v[:, 1], v[:, 2]))[order]  # per position
    tb_hi = np.fmax(v[:, 0], np.fmax(v[:, 1], v[:, 2]))[order]
    c_lo = np.zeros((n_nodes, 2), np.int64)  # position range under each child
    c_hi = np.zeros((n_nodes, 2), np.int64)
    c_min = np.zeros((n_nodes, 2, 3), np.float32)
    c_max = np.zeros((n_nodes, 2, 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if lf.size:
            srt = np.argsort(lf, kind="stable")
            starts = lf[srt]
            mn = np.fmin.reduceat(tb_lo, starts, axis=0)
            mx = np.fmax.reduceat(tb_hi, starts, axis=0)
            idx = np.argwhere(real)[srt]
            c_lo[idx[:, 0], idx[:, 1]] = starts
            c_hi[idx[:, 0], idx[:, 1]] = starts + lc[srt]
            c_min[idx[:, 0], idx[:, 1]] = mn
            c_max[idx[:, 0], idx[:, 1]] = mx
        for lev in reversed(levels):
            for k in (0, 1):
                sel = lev[~is_leaf[lev, k]]
                ch = inner_ref[sel, k]
                c_lo[sel, k] = c_lo[ch].min(1)
                c_hi[sel, k] = c_hi[ch].max(1)
                c_min[sel, k] = np.fmin(c_min[ch, 0], c_min[ch, 1])
                c_max[sel, k] = np.fmax(c_max[ch, 0], c_max[ch, 1])
        # contiguity follows from exact cover once the range holds as many triangles as it is long; then the order of the two children
        sizes = np.where(real, count, 0)
        for lev in reversed(levels):
            for k in (0, 1):
                sel = lev[~is_leaf[lev, k]]
                sizes[sel, k] = sizes[inner_ref[sel, k]].sum(1)
        nonempty = ~(is_leaf & (count == 0))
        gap = nonempty & (c_hi - c_lo != sizes)
        if gap.any():
            i, k = np.argwhere(gap)[0]
            _fail(f"node {i} child{k}: its triangles are not contiguous (positions [{c_lo[i, k]}, {c_hi[i, k]}) hold {sizes[i, k]})")
        both = nonempty.all(1)
        bad = both & (c_hi[:, 0] > c_lo[:, 1])
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            _fail(f"node {i}: child0's triangles [{c_lo[i, 0]}, {c_hi[i, 0]}) do not precede child1's [{c_lo[i, 1]}, {c_hi[i, 1]})")
        want_lo = c_min - PAD
        want_hi = c_max + PAD
    if single_leaf_root:  # the empty leaf carries child0's box; an empty scene's root is [-0.001, 0.001]
        if n == 0:
            want_lo[0, :] = -PAD
            want_hi[0, :] = PAD
        want_lo[0, 1] = want_lo[0, 0]
        want_hi[0, 1] = want_hi[0, 0]
    got = boxes.reshape(n_nodes, 2, 2, 3)  # [node, child, lo/hi, axis]
    for k in (0, 1):
        for side, want in ((0, want_lo), (1, want_hi)):
            bad = got[:, k, side].view(np.uint32) != want[:, k].view(np.uint32)
            if bad.any():
                i, a = np.argwhere(bad)[0]
                what = "lo" if side == 0 else "hi"
                _fail(f"node {i} child{k} {what}[{a}] = {got[i, k, side, a]!r} ({got[i, k, side, a:a + 1].view(np.uint32)[0]:#010x}), "
                      f"the exact padded bound is {want[i, k, a]!r} ({want[i, k, a:a + 1].view(np.uint32)[0]:#010x})")
    return len(levels)
