"""Cases and properties of the node-by-node checks (test_hostsim_node_claims.py on the CPU build, test_gpu_node_claims.py on gfx950's words):
synthetic 8-wide nodes, rays aimed at the corners, edges and faces of boxes, the superset property of trt_oct.h's header (1) evaluated on octVisit's
words, and the case file of tools/node_visit_check."""
import numpy as np

INF = np.float32(np.inf)


def ordered(x):
    """float32 -> int64 that orders like the floats and steps by one per ulp."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)


def synthetic_nodes(n, seed=1):
    """Exact boxes for n 8-wide nodes -> (blo [n, 8, 3], bhi, kind [n, 8]).  Node extents 2^-20 .. 2^34, centres 0 or up to 2^38 away, by node index:
    i % 8 == 1 a single used slot, == 2 all eight, == 3 every slot flat on ONE plane of an axis (extent 0: that axis's exponent byte at its floor of 1),
    == 4 extents of 1e-40 about 0 (the floor again, by size); every fourth slot elsewhere is flat on one axis."""
    rng = np.random.default_rng(seed)
    ext = np.ldexp(1.0, rng.integers(-20, 35, n))
    centre = np.where(rng.random((n, 3)) < 0.4, 0.0, np.ldexp(rng.uniform(0.5, 1.0, (n, 3)), rng.integers(-4, 39, (n, 3))) * rng.choice([-1.0, 1.0], (n, 3)))
    k = np.arange(n)
    ext[k % 8 == 4] = 1e-40
    centre[k % 8 == 4] = 0.0
    u = rng.random((n, 8, 3))
    lo = centre[:, None, :] + ext[:, None, None] * (u - 0.5)
    hi = lo + ext[:, None, None] * rng.random((n, 8, 3)) * (1.0 - u)
    flat = rng.random((n, 8)) < 0.25
    ax = rng.integers(0, 3, (n, 8))
    for a in range(3):
        sel = flat & (ax == a)
        hi[..., a][sel] = lo[..., a][sel]
    plane = k % 8 == 3
    lo[plane, :, 0] = lo[plane, :1, 0]
    hi[plane, :, 0] = lo[plane, :1, 0]
    used = rng.random((n, 8)) < 0.7
    used[k % 8 == 2] = True
    one = k % 8 == 1
    used[one] = False
    used[one, rng.integers(0, 8, one.sum())] = True
    used[~used.any(1), 0] = True
    kind = np.where(used, rng.integers(1, 5, (n, 8)), 0).astype(np.uint8)
    blo, bhi = lo.astype(np.float32), hi.astype(np.float32)
    bhi = np.maximum(bhi, blo)
    return blo, bhi, kind


def rays_at_boxes(box, seed=2, tiny=(1 / 3, -38.0, -30.0)):
    """One ray per box [m, 6] (lo, hi) aimed at a corner (a third), a point of an edge or of a face of it, from 2^-6 .. 2^24 extents away; the share tiny[0] (a third)
    of the directions have one or two components of 10^tiny[1] .. 10^tiny[2] (1e-38 .. 1e-30: products with them overflow; the reciprocal is finite down to 2.94e-39), a fifth of the origins lie exactly
    on a plane of the box.  -> (org, dir, far): far = the origin is at least 2^20 extents away."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, np.float64).reshape(-1, 6)
    m = len(box)
    lo, hi = box[:, :3], box[:, 3:]
    free = rng.integers(0, 3, m)  # coordinates of the target that are NOT on a plane: 0 corner, 1 edge, 2 face
    pick = np.where(rng.random((m, 3)) < 0.5, lo, hi)
    order = np.argsort(rng.random((m, 3)), axis=1)
    inside = lo + (hi - lo) * rng.random((m, 3))
    is_free = np.zeros((m, 3), bool)
    for j in range(2):
        np.put_along_axis(is_free, order[:, j:j + 1], (free > j)[:, None], axis=1)
    target = np.where(is_free, inside, pick)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    small = rng.random(m) < tiny[0]
    ta = rng.integers(0, 3, m)
    tv = 10.0 ** rng.uniform(tiny[1], tiny[2], m) * rng.choice([-1.0, 1.0], m)
    d[small, ta[small]] = tv[small]
    two = small & (rng.random(m) < 0.3)
    d[two, (ta[two] + 1) % 3] = 10.0 ** rng.uniform(tiny[1], tiny[2], two.sum())
    ext = np.maximum((hi - lo).max(1), np.abs(box).max(1) * 2.0 ** -24)
    ext = np.where(ext > 0, ext, 1e-30)
    k = rng.integers(-6, 25, m)
    o = target - d * (ext * np.ldexp(1.0, k))[:, None]
    on = rng.random(m) < 0.2
    oa = rng.integers(0, 3, m)
    o[on, oa[on]] = pick[on, oa[on]]
    d32 = d.astype(np.float32)
    d32 = np.where((d32 == 0) & (d != 0), np.float32(1.2e-38) * np.sign(d), d32).astype(np.float32)  # never a zero component: those rays go elsewhere
    with np.errstate(over="ignore"):
        o32 = o.astype(np.float32)
    o32 = np.where(np.isfinite(o32), o32, np.float32(0)).astype(np.float32)
    return o32, d32, (k >= 20) & ~on


def superset(nodes, slot_box, node, org, dirs, cull, words, passes, entry, far=None, chunk=1 << 18):
    """trt_oct.h, header (1), on octVisit's words: where boxTest passes a used slot's exact box and NOT entry > cull, the slot's bit(s) are set — bit
    24 + (slot ^ (7 - octant)) of the node word for an inner slot, every triangle bit of the slot for a leaf slot.
    -> (counts, text of the first misses).  counts: reference passes that reach the property in total / with a finite cull within one ulp of the entry / on a
    box that is flat on an axis / with an overflowed plane product / from an origin 2^20 extents away, and the misses."""
    counts = dict(passes=0, near_cull=0, flat=0, overflow=0, far=0, misses=0)
    shown = []
    n = len(node)
    far = np.zeros(n, bool) if far is None else far
    for c0 in range(0, n, chunk):
        s = slice(c0, min(n, c0 + chunk))
        nd = nodes[node[s]]
        meta = nd["meta"].astype(np.uint32)
        used = meta != 0
        inner = used & ((meta & 0x1F) >= 24)
        d = dirs[s]
        perm = 7 - ((d[:, 0] < 0) * 4 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 1)
        sl = np.arange(8, dtype=np.uint32)[None, :]
        w = words[s].astype(np.uint32)
        inner_set = ((w[:, :1] >> (24 + (sl ^ perm[:, None].astype(np.uint32)))) & 1) == 1
        bits = (meta >> 5) << (meta & 0x1F)
        leaf_set = (w[:, 1:2] & bits) == bits
        e, cu = entry[s], cull[s][:, None]
        need = passes[s] & used & ~(e > cu)
        miss = need & ~np.where(inner, inner_set, leaf_set)
        b = slot_box[node[s]].astype(np.float32)
        o = org[s]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            inv = (np.float32(1) / d)[:, None, :]
            prod = np.concatenate([(b[:, :, :3] - o[:, None, :]) * inv, (b[:, :, 3:] - o[:, None, :]) * inv], axis=2)
        counts["passes"] += int(need.sum())
        counts["near_cull"] += int((need & np.isfinite(cu) & (np.abs(ordered(e) - ordered(np.broadcast_to(cu, e.shape))) <= 1)).sum())
        counts["flat"] += int((need & (b[:, :, :3] == b[:, :, 3:]).any(2)).sum())
        counts["overflow"] += int((need & ~np.isfinite(prod).all(2)).sum())
        counts["far"] += int((need & far[s][:, None]).sum())
        counts["misses"] += int(miss.sum())
        for i, j in zip(*np.nonzero(miss)):
            if len(shown) < 8:
                g = c0 + i
                shown.append(f"node {node[g]} slot {j} ({'inner' if inner[i, j] else 'leaf'}) o={org[g]!r} d={dirs[g]!r} cull={cull[g]!r} entry={e[i, j]!r} "
                             f"box={b[i, j]!r} words={w[i, 0]:#010x},{w[i, 1]:#010x} node={nd[i]!r}")
    return counts, "\n".join(shown)


def culls_for(passes, entry, used, t_hit_bound, rng):
    """Per (node, ray) pair the culls of the checks: +inf, the bound of the oracle's hit (t_hit_bound, +inf for a miss), and the entry of one passing used
    slot with the floats next to it.  A cull is the bound of a hit at b >= 0, so it is never negative: below 0 it is 0.
    -> (index into the pairs [m], cull [m])."""
    n = len(passes)
    ok = passes & used
    r = rng.random(ok.shape) * ok
    slot = r.argmax(1)
    has = ok.any(1)
    e = entry[np.arange(n), slot]
    idx = [np.arange(n), np.arange(n)]
    cull = [np.full(n, INF, np.float32), np.asarray(t_hit_bound, np.float32)]
    sel = np.nonzero(has & ~np.isnan(e))[0]
    for v in (e[sel], np.nextafter(e[sel], -INF), np.nextafter(e[sel], INF)):
        idx.append(sel)
        cull.append(np.maximum(v, np.float32(0)).astype(np.float32))
    return np.concatenate(idx), np.concatenate(cull)


# Box cases whose boxTest entry is a zero reached through fminf / fmaxf of zeros of OPPOSITE sign, with the words gfx950 returns (verdicts, entry of boxTest,
# entry of boxTestGlm): libm's fminf / fmaxf pick the other zero (trt_prims.h, trt_fminf).
ZERO_SIGN_BOXES = np.array([[-11.3386, 5.6083, 1.5194, -11.3341, 5.61095, 1.5327301], [1.92175, 5.6075, 1.53984, 1.9280001, 5.6098, 1.5528301]], np.float32)
ZERO_SIGN_ORG = np.array([[-11.3386, 5.61095, 1.5288149], [1.9219372, 5.6098, 1.5528301]], np.float32)
ZERO_SIGN_DIR = np.array([[5.9830661e-36, -0.68456084, 0.036713440], [-0.92275566, 0.32315806, -np.inf]], np.float32)
ZERO_SIGN_WORDS = np.array([[3, 0x00000000, 0x00000000], [0, 0x80000000, 0x80000000]], np.uint32)


# ---- the case file of tools/node_visit_check -----------------------------------------------------------------------------------------------------------
# header: eight uint32 (magic, oct nodes, oct cases, 4-wide nodes, innerStep cases, box cases, 0, 0); the oct nodes (80 B each); the oct cases (node, o.xyz,
# d.xyz, cull: 32 B); the 4-wide nodes (128 B); the innerStep cases (as the oct cases); the box cases (lo.xyz, hi.xyz, o.xyz, d.xyz: 48 B).
# result: two words per oct case, six per innerStep case, three per box case, in that order (what hostsim_lib's *_cases return).
MAGIC = 0x4E564331
CASE_DT = np.dtype([("node", "<u4"), ("o", "<f4", 3), ("d", "<f4", 3), ("cull", "<f4")])
BOX_DT = np.dtype([("box", "<f4", 6), ("o", "<f4", 3), ("d", "<f4", 3)])


def _cases(node, org, dirs, cull):
    c = np.zeros(len(node), CASE_DT)
    c["node"], c["o"], c["d"], c["cull"] = node, org, dirs, cull
    return c


def write_case_file(path, onodes, oct_cases, wnodes, inner_cases, box, box_org, box_dir):
    oc, ic = _cases(*oct_cases), _cases(*inner_cases)
    bc = np.zeros(len(box), BOX_DT)
    bc["box"], bc["o"], bc["d"] = box, box_org, box_dir
    assert onodes.dtype.itemsize == 80 and wnodes.dtype.itemsize == 128
    assert len(oc) == 0 or int(oc["node"].max()) < len(onodes)
    assert len(ic) == 0 or int(ic["node"].max()) < len(wnodes)
    with open(path, "wb") as f:
        f.write(np.array([MAGIC, len(onodes), len(oc), len(wnodes), len(ic), len(bc), 0, 0], "<u4").tobytes())
        for a in (onodes, oc, wnodes, ic, bc):
            f.write(np.ascontiguousarray(a).tobytes())
    return len(oc), len(ic), len(bc)


def read_result_file(path, n_oct, n_inner, n_box):
    w = np.fromfile(path, "<u4")
    assert len(w) == 2 * n_oct + 6 * n_inner + 3 * n_box, (len(w), n_oct, n_inner, n_box)
    a, b = 2 * n_oct, 2 * n_oct + 6 * n_inner
    return w[:a].reshape(-1, 2), w[a:b].reshape(-1, 6), w[b:].reshape(-1, 3)
