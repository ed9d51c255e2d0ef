"""A plain float32 restatement of the GPU BVH builder (include/trt_build.h, tinyraytracing_amd/csrc/trt_lbvh.hip), written from
what those files document, not from how the kernels compute it.  The builder is deterministic and compiled without contraction,
so this reproduces its output bit for bit: nodes (reserved words included), node count, triangle order and depth.

  triangle boxes      fminf / fmaxf over the three vertices (NaN dropped: np.fmin / np.fmax)
  centre              0.5f * lo + 0.5f * hi; the frame is the min and max of the centres
  Morton code         scale = 2^21 / extent (0 unless the extent is > 0 and finite), t = (c - lo) * scale clamped to [0, 2^21 - 1]
                      (NaN -> 0) and truncated; key = spread(x) << 2 | spread(y) << 1 | spread(z)
  sort                stable by key (rocprim's radix sort of (key, index) pairs)
  radix tree          split top-down at the highest bit in which the ends of a range differ, positions breaking equal keys; the
                      root is 0, a node split at g has children g and g + 1, a one-position child is a triangle
  radix path          (TRT_LBVH_CLUSTER=0 or n <= cluster) inner nodes of more than leaf_num triangles, numbered by an exclusive
                      scan in inner-node order
  cluster path        the maximal subtrees of <= cluster triangles under an exact sweep-SAH tree over them (TopBuilder)
It is not a port of the kernels' search (Karras' doubling and bisection): a shared mistake would hide.
"""
import sys

import numpy as np

LEAF_BIT = 0x80000000
PAD = np.float32(0.001)
BIG = np.float32(3.0e38)  # TopBuilder's initial bounds in its sweeps
FLT_MAX = np.finfo(np.float32).max
TOP_MEDIAN_DEPTH = 48


def cluster_for(n, leaf_num, env=None):
    """Cluster size the builder uses: tiers 2 / 16 / 128 / 2048 switching at 50 k, 500 k and 4 M triangles; TRT_LBVH_CLUSTER
    (`env`, a string as in the environment) overrides; a cluster smaller than a leaf is raised to leaf_num; 0 = the radix tree."""
    c = 2 if n < 50000 else 16 if n < 500000 else 128 if n < 4000000 else 2048
    if env is not None:
        try:
            c = max(0, int(env))
        except ValueError:
            c = 0
    if c and c < leaf_num:
        c = leaf_num
    return c


def make_leaf(first, count):
    return (LEAF_BIT | (np.asarray(count, np.int64) << 27) | np.asarray(first, np.int64)).astype(np.uint32)


def spread21(x):
    x = x.astype(np.uint64) & np.uint64(0x1FFFFF)
    for sh, m in ((32, 0x001F00000000FFFF), (16, 0x001F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(m)
    return x


def morton_keys(tri_v):
    """Triangle boxes (n, 3) lo / hi and the 63-bit keys."""
    v = np.ascontiguousarray(tri_v, np.float32).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = np.fmin(v[:, 0], np.fmin(v[:, 1], v[:, 2]))
        hi = np.fmax(v[:, 0], np.fmax(v[:, 1], v[:, 2]))
        c = np.float32(0.5) * lo + np.float32(0.5) * hi
        flo = np.fmin.reduce(c, axis=0, initial=np.inf).astype(np.float32)
        fhi = np.fmax.reduce(c, axis=0, initial=-np.inf).astype(np.float32)
        ext = fhi - flo
        scale = np.where((ext > 0) & np.isfinite(ext), np.float32(2097152.0) / np.where(ext > 0, ext, 1), 0).astype(np.float32)
        t = (c - flo) * scale
        t = np.fmin(np.fmax(t, np.float32(0)), np.float32(2097151.0))
    q = t.astype(np.uint32)
    keys = (spread21(q[:, 0]) << np.uint64(2)) | (spread21(q[:, 1]) << np.uint64(1)) | spread21(q[:, 2])
    return lo, hi, keys


def _highest_bit(x):
    """Index of the highest set bit of nonzero uint64 values."""
    x = x.astype(np.uint64)
    r = np.zeros(x.shape, np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        big = x >= (np.uint64(1) << np.uint64(sh))
        r += np.where(big, sh, 0)
        x = np.where(big, x >> np.uint64(sh), x)
    return r


def radix_tree(keys_sorted):
    """The radix tree over (key, position).  Returns, per inner node 0..n-2: left, right (LEAF_BIT | position for a triangle),
    first, last, level (root 1), and the parent of every inner node (-1 at the root)."""
    n = keys_sorted.size
    ni = n - 1
    left = np.zeros(ni, np.int64)
    right = np.zeros(ni, np.int64)
    first = np.zeros(ni, np.int64)
    last = np.zeros(ni, np.int64)
    level = np.zeros(ni, np.int64)
    parent = np.full(ni, -1, np.int64)
    idx, lo, hi = np.array([0]), np.array([0]), np.array([n - 1])
    lev = 1
    while idx.size:
        first[idx], last[idx], level[idx] = lo, hi, lev
        ka, kb = keys_sorted[lo], keys_sorted[hi]
        g = np.empty(idx.size, np.int64)
        diff = ka != kb
        if diff.any():
            b = _highest_bit(ka[diff] ^ kb[diff]).astype(np.uint64)
            thr = kb[diff] & ~((np.uint64(1) << b) - np.uint64(1))  # hi's prefix down to the differing bit, zeros below
            g[diff] = np.searchsorted(keys_sorted, thr, side="left") - 1
        if (~diff).any():
            a, z = lo[~diff], hi[~diff]
            b = _highest_bit((a ^ z).astype(np.uint64))
            g[~diff] = (z & ~((np.int64(1) << b) - 1)) - 1
        assert ((g >= lo) & (g < hi)).all()
        left[idx] = np.where(g == lo, LEAF_BIT | g, g)
        right[idx] = np.where(g + 1 == hi, LEAF_BIT | (g + 1), g + 1)
        nxt_i, nxt_lo, nxt_hi = [], [], []
        m = g > lo
        parent[g[m]] = idx[m]
        nxt_i.append(g[m]); nxt_lo.append(lo[m]); nxt_hi.append(g[m])
        m = g + 1 < hi
        parent[g[m] + 1] = idx[m]
        nxt_i.append(g[m] + 1); nxt_lo.append(g[m] + 1); nxt_hi.append(hi[m])
        idx, lo, hi = np.concatenate(nxt_i), np.concatenate(nxt_lo), np.concatenate(nxt_hi)
        lev += 1
    return left, right, first, last, level, parent


def node_boxes(left, right, level, plo, phi):
    """Bounds of every inner node: the reduction over its range, bottom-up (plo / phi per sorted position)."""
    ni = left.size
    nlo = np.zeros((ni, 3), np.float32)
    nhi = np.zeros((ni, 3), np.float32)
    by_level = np.argsort(-level, kind="stable")
    bounds = np.flatnonzero(np.diff(level[by_level])) + 1
    for grp in np.split(by_level, bounds):
        los, his = [], []
        for ch in (left[grp], right[grp]):
            leaf = (ch & LEAF_BIT) != 0
            pos = ch & ~LEAF_BIT
            los.append(np.where(leaf[:, None], plo[np.where(leaf, pos, 0)], nlo[np.where(leaf, 0, ch)]))
            his.append(np.where(leaf[:, None], phi[np.where(leaf, pos, 0)], nhi[np.where(leaf, 0, ch)]))
        nlo[grp] = np.fmin(los[0], los[1])
        nhi[grp] = np.fmax(his[0], his[1])
    return nlo, nhi


def _emit(left, right, first, last, keep, new_index, nlo, nhi, plo, phi, sel, base, shift_of):
    """Flat nodes (len(sel), 16 words) for the kept inner nodes `sel`: children as k_emit / k_emit_clusters give them."""
    w = np.zeros((sel.size, 16), np.uint32)
    f = w[:, :12].view(np.float32)
    sh = shift_of[sel]
    for k, ch in enumerate((left[sel], right[sel])):
        leaf = (ch & LEAF_BIT) != 0
        pos = ch & ~LEAF_BIT
        inner = np.where(leaf, 0, ch)
        lo = np.where(leaf[:, None], plo[np.where(leaf, pos, 0)], nlo[inner])
        hi = np.where(leaf[:, None], phi[np.where(leaf, pos, 0)], nhi[inner])
        f[:, 6 * k:6 * k + 3] = lo - PAD
        f[:, 6 * k + 3:6 * k + 6] = hi + PAD
        cnt = last[inner] - first[inner] + 1
        ref = np.where(leaf, make_leaf(pos + sh, 1),
                       np.where(keep[inner], base + new_index[inner], make_leaf(first[inner] + sh, cnt)))
        w[:, 12 + k] = ref.astype(np.uint32)
    return w


class TopBuilder:
    """Exact sweep SAH over the clusters (cost = half-area x triangles), in float32 and in the C++ operation order; preorder numbering.
    `median_at_depth` / `fallback` count the nodes split by the depth-48 median and by the median no finite cost beat."""

    def __init__(self, clo, chi, ccount):
        self.clo, self.chi, self.cnt = clo, chi, ccount.astype(np.uint64)
        m = clo.shape[0]
        cen = np.float32(0.5) * clo + np.float32(0.5) * chi
        self.ord = [np.lexsort((np.arange(m), cen[:, a])) for a in range(3)]
        self.side = np.zeros(m, np.uint8)
        self.nodes = []  # [child0, child1, lo0, hi0, lo1, hi1]
        self.leaf_order = []
        self.top_depth = np.zeros(m, np.int64)
        self.median_at_depth = 0
        self.fallback = 0

    @staticmethod
    def half_area(lo, hi):
        x, y, z = (hi[..., 0] - lo[..., 0]), (hi[..., 1] - lo[..., 1]), (hi[..., 2] - lo[..., 2])
        return x * y + x * z + y * z

    def _costs(self, o):
        lo, hi, cnt = self.clo[o], self.chi[o], self.cnt[o]
        # prefix over o[0..i-1] and suffix over o[i..m-1], each started from +-3e38 as in the sweeps
        plo = np.fmin.accumulate(np.concatenate([np.full((1, 3), BIG, np.float32), lo[:-1]]), axis=0)[1:]
        phi = np.fmax.accumulate(np.concatenate([np.full((1, 3), -BIG, np.float32), hi[:-1]]), axis=0)[1:]
        slo = np.fmin.accumulate(np.concatenate([np.full((1, 3), BIG, np.float32), lo[:0:-1]]), axis=0)[:0:-1]
        shi = np.fmax.accumulate(np.concatenate([np.full((1, 3), -BIG, np.float32), hi[:0:-1]]), axis=0)[:0:-1]
        pc = np.cumsum(cnt[:-1]).astype(np.float32)
        sc = np.cumsum(cnt[:0:-1])[::-1].astype(np.float32)
        return self.half_area(plo, phi) * pc + self.half_area(slo, shi) * sc  # [i - 1] = cost of the split before o[i]

    def build(self, lo, hi, depth):
        if hi - lo == 1:
            c = int(self.ord[0][lo])
            self.leaf_order.append(c)
            self.top_depth[c] = depth
            return ~c, self.clo[c], self.chi[c]
        m = hi - lo
        best, best_axis, best_mid = FLT_MAX, -1, lo + m // 2
        if depth < TOP_MEDIAN_DEPTH:
            for a in range(3):
                with np.errstate(invalid="ignore", over="ignore"):
                    cost = self._costs(self.ord[a][lo:hi])
                cost = np.where(np.isnan(cost), np.float32(np.inf), cost)
                i = int(np.argmin(cost))
                if cost[i] < best:
                    best, best_axis, best_mid = cost[i], a, lo + i + 1
        else:
            self.median_at_depth += 1
        if best_axis < 0:
            if depth < TOP_MEDIAN_DEPTH:
                self.fallback += 1
            best_axis, best_mid = 0, lo + m // 2
        seg = self.ord[best_axis][lo:hi]
        self.side[seg[:best_mid - lo]] = 0
        self.side[seg[best_mid - lo:]] = 1
        for a in range(3):
            if a != best_axis:
                s = self.ord[a][lo:hi]
                sd = self.side[s]
                self.ord[a][lo:hi] = np.concatenate([s[sd == 0], s[sd == 1]])
        me = len(self.nodes)
        self.nodes.append(None)
        c0, l0, h0 = self.build(lo, best_mid, depth + 1)
        c1, l1, h1 = self.build(best_mid, hi, depth + 1)
        self.nodes[me] = (c0, c1, l0, h0, l1, h1)
        return me, np.fmin(l0, l1), np.fmax(h0, h1)


def build(tri_v, leaf_num, cluster_env=None, stats=None):
    """(nodes as bytes, n_nodes, order, depth) of trt_build_lbvh(tri_v, n, leaf_num, ...) with TRT_LBVH_CLUSTER = cluster_env (None: unset).
    `stats`, a dict, receives the path taken and TopBuilder's branch counts."""
    v = np.ascontiguousarray(tri_v, np.float32).reshape(-1, 9)
    n = v.shape[0]
    if stats is None:
        stats = {}
    plo_c, phi_c, keys = morton_keys(v) if n else (np.zeros((0, 3), np.float32),) * 2 + (np.zeros(0, np.uint64),)
    if n <= leaf_num:  # one root: child0 = every triangle, child1 = an empty leaf with the same box (as host/bvh.cpp)
        stats["path"] = "one leaf"
        lo = np.fmin.reduce(plo_c, axis=0) if n else np.zeros(3, np.float32)
        hi = np.fmax.reduce(phi_c, axis=0) if n else np.zeros(3, np.float32)
        w = np.zeros(16, np.uint32)
        f = w[:12].view(np.float32)
        f[0:3] = f[6:9] = lo - PAD
        f[3:6] = f[9:12] = hi + PAD
        w[12] = make_leaf(0, n)
        w[13] = make_leaf(0, 0)
        return w.tobytes(), 1, np.arange(n, dtype=np.uint32), 1
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    plo, phi = plo_c[order], phi_c[order]  # per sorted position
    left, right, first, last, level, parent = radix_tree(ks)
    nlo, nhi = node_boxes(left, right, level, plo, phi)
    cnt = last - first + 1
    ni = n - 1
    cluster = cluster_for(n, leaf_num, cluster_env)
    stats["cluster"] = cluster
    if not cluster or n <= cluster:
        stats["path"] = "radix"
        keep = cnt > leaf_num
        new_index = np.cumsum(keep) - keep
        sel = np.flatnonzero(keep)
        w = np.zeros((sel.size, 16), np.uint32)
        w[new_index[sel]] = _emit(left, right, first, last, keep, new_index, nlo, nhi, plo, phi, sel, 0, np.zeros(ni, np.int64))
        return w.tobytes(), int(sel.size), order.astype(np.uint32), int(level[keep].max())
    stats["path"] = "clusters"
    # clusters: inner nodes of <= cluster triangles under a top node, and single triangles right under one; numbered by first position
    top = cnt > cluster
    croot_inner = np.flatnonzero(~top & (parent >= 0) & top[np.maximum(parent, 0)])
    leaf_parent = np.empty(n, np.int64)
    for ch in (left, right):
        lf = (ch & LEAF_BIT) != 0
        leaf_parent[ch[lf] & ~LEAF_BIT] = np.flatnonzero(lf)
    single = np.flatnonzero(top[leaf_parent])
    c_first = np.concatenate([first[croot_inner], single])
    c_root = np.concatenate([croot_inner, LEAF_BIT | single])
    srt = np.argsort(c_first, kind="stable")
    c_first, c_root = c_first[srt], c_root[srt]
    nc = c_first.size
    c_leaf = (c_root & LEAF_BIT) != 0
    c_inner = np.where(c_leaf, 0, c_root)
    c_count = np.where(c_leaf, 1, cnt[c_inner])
    c_lo = np.where(c_leaf[:, None], plo[np.where(c_leaf, c_first, 0)], nlo[c_inner])
    c_hi = np.where(c_leaf[:, None], phi[np.where(c_leaf, c_first, 0)], nhi[c_inner])
    assert c_count.sum() == n and nc >= 2
    stats["n_clusters"] = nc
    tb = TopBuilder(c_lo, c_hi, c_count)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10000))
    try:
        tb.build(0, nc, 0)
    finally:
        sys.setrecursionlimit(limit)
    stats["top_nodes"] = len(tb.nodes)
    stats["top_median_at_depth"] = tb.median_at_depth
    stats["top_fallback"] = tb.fallback
    T = len(tb.nodes)
    new_first = np.zeros(nc, np.int64)
    new_first[tb.leaf_order] = np.concatenate([[0], np.cumsum(c_count[tb.leaf_order])[:-1]])
    shift = new_first - c_first
    cl_of_pos = np.searchsorted(c_first, np.arange(n), side="right") - 1
    keep = (cnt > leaf_num) & (cnt <= cluster)
    new_index = np.cumsum(keep) - keep
    sel = np.flatnonzero(keep)
    n_in = sel.size
    assert T + n_in <= ni
    w = np.zeros((T + n_in, 16), np.uint32)
    w[T + new_index[sel]] = _emit(left, right, first, last, keep, new_index, nlo, nhi, plo, phi, sel, T, shift[cl_of_pos[first]])
    cidx = np.where(~c_leaf & keep[c_inner], new_index[c_inner], -1)
    f = w[:, :12].view(np.float32)
    for k, (c0, c1, l0, h0, l1, h1) in enumerate(tb.nodes):
        for s, (c, lo, hi) in enumerate(((c0, l0, h0), (c1, l1, h1))):
            f[k, 6 * s:6 * s + 3] = lo - PAD
            f[k, 6 * s + 3:6 * s + 6] = hi + PAD
            if c >= 0:
                ref = c
            else:
                c = ~c
                ref = T + cidx[c] if cidx[c] >= 0 else int(make_leaf(new_first[c], c_count[c]))
            w[k, 12 + s] = ref
    order2 = np.empty(n, np.int64)
    order2[np.arange(n) + shift[cl_of_pos]] = order
    # kept nodes from a cluster's root down, deepest per cluster
    cdepth = np.zeros(nc, np.int64)
    croot_level = np.where(c_leaf, 0, level[c_inner])
    cid = cl_of_pos[first[sel]]
    np.maximum.at(cdepth, cid, level[sel] - croot_level[cid] + 1)
    depth = int((tb.top_depth + cdepth).max())
    return w.tobytes(), T + n_in, order2.astype(np.uint32), depth

