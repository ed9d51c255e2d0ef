#!/usr/bin/env python3
"""What would binning rays by leaf mask buy the wave-uniform walk (trt_kernels.h traceQueueBinned)?  CPU only.

The walk tests every triangle of a leaf as soon as one lane of the wave reaches it, so a wave pays for the union of its rays' leaves.  This
takes queues like the render's — camera rays, bounce-1 and bounce-3 extension rays (cosine-weighted about the hit's geometric normal), bounce-0
and bounce-2 shadow rays (toward a uniform point of a light triangle) — in path-id order (pixel order of one sample: what k_shade's per-block
compaction roughly keeps), computes each ray's leaf mask with the walk's own slab test in float32, and counts wave-level triangle steps per wave:
  today           64-lane waves in queue order;
  binned 256      each 256-ray block sorted by mask (the kernel's 8-bit key), then cut into waves;
  binned 1024     the same within 1024-ray blocks.
Directions are a model of the render's sampling (the oracle's trace gives the hits), so the numbers are estimates of the distribution, not
the render's exact queues.  usage: tools/bin_potential.py [scene] [rows] [leaf]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import tinyraytracing_amd as T  # noqa: E402

LEAF_BIT = 0x80000000
VALU_PER_TRI_STEP = 40  # wave instructions per wave-level triangle step (triCandidateParts, votes, LDS park: DESIGN.md §4.1)


def tree(flat):
    f = flat.contents
    nodes = []
    for k in range(f.n_nodes):
        nd = f.nodes[k]
        nodes.append(((np.array(nd.lo0, np.float32), np.array(nd.hi0, np.float32)), (np.array(nd.lo1, np.float32), np.array(nd.hi1, np.float32)),
                      (nd.child0, nd.child1)))
    return nodes


def box_hit(lo, hi, o, inv):
    # slabResult (trt_path.h): t1 >= t0 and t1 > 0, in float32
    with np.errstate(invalid="ignore", over="ignore"):
        tin = (hi[None, :] - o) * inv
        tout = (lo[None, :] - o) * inv
        t1 = np.minimum(np.maximum(tin[:, 0], tout[:, 0]), np.minimum(np.maximum(tin[:, 1], tout[:, 1]), np.maximum(tin[:, 2], tout[:, 2])))
        t0 = np.maximum(np.minimum(tin[:, 0], tout[:, 0]), np.maximum(np.minimum(tin[:, 1], tout[:, 1]), np.minimum(tin[:, 2], tout[:, 2])))
    return (t1 >= t0) & (t1 > 0)


def leaf_masks(nodes, o, d):
    """bit k = the ray reaches the k-th leaf in walk order (node index, child 0 before child 1); and each leaf's triangle count."""
    with np.errstate(divide="ignore"):
        inv = (np.float32(1.0) / d).astype(np.float32)
    n = len(o)
    reach = np.zeros((len(nodes), n), bool)
    reach[0] = True
    mask = np.zeros(n, np.uint64)
    counts = []
    for ni, (b0, b1, ch) in enumerate(nodes):
        for (lo, hi), ref in zip((b0, b1), ch):
            h = reach[ni] & box_hit(lo, hi, o, inv)
            if ref & LEAF_BIT:
                mask |= h.astype(np.uint64) << np.uint64(len(counts))
                counts.append((ref >> 27) & 15)
            else:
                reach[ref] |= h
    return mask, np.array(counts)


def key_of(mask, n_leaves):
    if n_leaves <= 8:
        return (mask & np.uint64(0xFF)).astype(np.int64)
    run = (n_leaves + 7) // 8
    key = np.zeros(len(mask), np.int64)
    for k in range(8):
        key |= (((mask >> np.uint64(k * run)) & np.uint64((1 << run) - 1)) != 0).astype(np.int64) << k
    return key


def wave_tests(mask, counts, block):
    """wave-level triangle steps per wave of 64 rays (the triangles of the union of its rays' leaves), with the rays of each `block` sorted by
    key first (block 0: queue order)."""
    m = mask.copy()
    if block:
        key = key_of(m, len(counts))
        for s in range(0, len(m), block):
            m[s:s + block] = m[s:s + block][np.argsort(key[s:s + block], kind="stable")]
    pad = (-len(m)) % 64
    w = np.concatenate([m, np.zeros(pad, np.uint64)]).reshape(-1, 64)
    union = np.bitwise_or.reduce(w, axis=1)
    tests = sum(((union >> np.uint64(k)) & np.uint64(1)).astype(np.int64) * int(c) for k, c in enumerate(counts))
    return float(tests.sum()) / (len(m) / 64)


def lane_tests(mask, counts):
    return float(sum(((mask >> np.uint64(k)) & np.uint64(1)).astype(np.int64) * int(c) for k, c in enumerate(counts)).mean())


def cosine_dirs(nrm, rng):
    u1, u2 = rng.random(len(nrm)), rng.random(len(nrm))
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0, 1, 0]]), np.array([[1, 0, 0]]))
    t = np.cross(nrm, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    d = t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + nrm * np.sqrt(1 - u1)[:, None]
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "back"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    leaf = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    w, h = 1920, 1080
    s = T.Scene.named(name, w, h, leaf_num=leaf)
    f = s.flat.contents
    nodes = tree(s.flat)
    tv = s.arrays()["tri_v"]
    rng = np.random.default_rng(5)
    cam = f.camera
    eye, llc = np.array(cam.eye, np.float32), np.array(cam.lower_left_corner, np.float32)
    hor, ver = np.array(cam.horizontal, np.float32), np.array(cam.vertical, np.float32)
    i0 = (h - rows) // 2  # a band of rows through the middle of the image, in pixel order
    ii, jj = np.meshgrid(np.arange(i0, i0 + rows), np.arange(w), indexing="ij")
    u = (jj.ravel() + rng.random(ii.size)) / w
    v = (ii.ravel() + rng.random(ii.size)) / h
    d = llc[None, :] + u[:, None] * hor[None, :] + v[:, None] * ver[None, :] - eye[None, :]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.broadcast_to(eye, d.shape).astype(np.float32).copy()
    lt = np.array([np.array(f.light_tris[k].v, np.float32) for k in range(f.n_light_tris)])
    queues = {}
    cur_o, cur_d = o, d
    for bounce in range(4):
        if bounce in (0,):
            queues["camera rays (bounce 0)"] = (cur_o, cur_d)
        elif bounce in (1, 3):
            queues[f"bounce-{bounce} extension rays"] = (cur_o, cur_d)
        t, tri, _ = O.trace(s.flat, cur_o, cur_d)
        hit = tri >= 0
        P = (cur_o[hit] + cur_d[hit] * t[hit, None]).astype(np.float32)
        V = tv[tri[hit]]
        nrm = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.where((nrm * cur_d[hit]).sum(1, keepdims=True) > 0, -nrm, nrm)
        if bounce in (0, 2):
            k = rng.integers(0, len(lt), len(P))
            a, b = rng.random(len(P)), rng.random(len(P))
            sa = np.sqrt(a)
            q = lt[k, 0] * (1 - sa)[:, None] + lt[k, 1] * (sa * (1 - b))[:, None] + lt[k, 2] * (sa * b)[:, None]
            sd = q - P
            sd = (sd / np.linalg.norm(sd, axis=1, keepdims=True)).astype(np.float32)
            queues[f"bounce-{bounce} shadow rays"] = (P, sd)
        cur_o, cur_d = P, cosine_dirs(nrm, rng)
    print(f"# {name}, leaf {leaf}: {len(nodes)} inner nodes; rows {i0}..{i0 + rows - 1} of {w}x{h}, one sample, queues in path-id order")
    print(f"# wave-level triangle steps per wave of 64 rays; ray = the triangles of one ray's own leaves (the per-lane counter); saved = wave instructions"
          f" per wave at {VALU_PER_TRI_STEP} per step, binned within 256 rays")
    print(f"{'queue':30s} {'rays':>8s} {'ray':>6s} {'today':>7s} {'bin256':>7s} {'bin1024':>8s} {'cut256':>7s} {'cut1024':>8s} {'saved':>6s}")
    for label, (qo, qd) in queues.items():
        mask, counts = leaf_masks(nodes, qo, qd)
        lane = lane_tests(mask, counts)
        t0, t1, t2 = wave_tests(mask, counts, 0), wave_tests(mask, counts, 256), wave_tests(mask, counts, 1024)
        saved = (t0 - t1) * VALU_PER_TRI_STEP
        print(f"{label:30s} {len(qo):8d} {lane:6.2f} {t0:7.2f} {t1:7.2f} {t2:8.2f} {100 * (1 - t1 / t0):6.1f}% {100 * (1 - t2 / t0):7.1f}% {saved:6.0f}")
    print(f"# leaves in walk order: {[int(c) for c in counts]} triangles")


if __name__ == "__main__":
    main()
