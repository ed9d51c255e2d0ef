#!/usr/bin/env python3
"""Cost of the ray queries (include/trt.h: trt_trace_closest*, trt_trace_occluded*) — profiles/ray_queries.txt.

For each scene (back, staircase) and ray set (2^24 incoherent rays: origins uniform in the scene's box, directions uniform on the sphere; the
1920x1080 camera rays through pixel centres), three queries: unbounded closest hit, closest hit bounded at 0.5 t0 (t0: the unbounded hit),
occlusion (unbounded).  Each through the host entry (numpy arrays: the PCIe trips included) and the device entry (torch tensors in HBM), --reps
times; printed: the traversal kernel's time as the library reports it (kernel_ms, median) and the call's wall time (median), as Mrays/s.
Run it under `rocprofv3 --kernel-trace --stats -- python3 tools/query_cost.py` for the per-kernel table.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyraytracing_amd as T  # noqa: E402

K_CLOSEST, K_SHADOW = 1, 3


def incoherent(s, n, seed=11):
    v = s.arrays()["tri_v"].reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(seed)
    org = (rng.random((n, 3), np.float32) * (hi - lo) + lo).astype(np.float32)
    d = rng.standard_normal((n, 3), np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return org, d.astype(np.float32)


def primary(s, w, h):
    cam = s.flat.contents.camera
    eye, llc = np.array(cam.eye, np.float32), np.array(cam.lower_left_corner, np.float32)
    hor, ver = np.array(cam.horizontal, np.float32), np.array(cam.vertical, np.float32)
    j, i = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    u, v = ((j + 0.5) / w).reshape(-1, 1), ((h - 1 - i + 0.5) / h).reshape(-1, 1)
    d = llc + u * hor + v * ver - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(eye, d.shape).astype(np.float32).copy(), d.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=24)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    for name in ("back", "staircase"):
        s = T.Scene.named(name, 1920, 1080)
        r = T.Renderer(s, 0)
        for set_name, (o, d) in (("incoherent 2^%d" % a.log2n, incoherent(s, 1 << a.log2n)), ("primary 1920x1080", primary(s, 1920, 1080))):
            n = len(o)
            t0 = r.trace_closest(o, d)[0]
            half = (np.float32(0.5) * t0).astype(np.float32)
            og, dg, hg = (torch.from_numpy(x).to(dev) for x in (o, d, half))
            t, tri, uv = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.float32, device=dev)
            occ = torch.empty(n, dtype=torch.uint8, device=dev)
            hit_frac = {"closest": float((r.trace_closest(o, d)[1] >= 0).mean()), "closest 0.5 t0": float((r.trace_closest(o, d, t_max=half)[1] >= 0).mean()),
                        "occluded": float(r.trace_occluded(o, d).mean())}
            runs = {
                ("closest", "host"): lambda: r.trace_closest(o, d, want_stats=True)[3],
                ("closest", "device"): lambda: r.trace_closest_into(og, dg, t, tri, uv),
                ("closest 0.5 t0", "host"): lambda: r.trace_closest(o, d, want_stats=True, t_max=half)[3],
                ("closest 0.5 t0", "device"): lambda: r.trace_closest_into(og, dg, t, tri, uv, t_max=hg),
                ("occluded", "host"): lambda: r.trace_occluded(o, d, want_stats=True)[1],
                ("occluded", "device"): lambda: r.trace_occluded_into(og, dg, occ),
            }
            for (query, entry), call in runs.items():
                k = K_SHADOW if query == "occluded" else K_CLOSEST
                call()
                kms, wall, visits = [], [], 0
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    w0 = time.perf_counter()
                    st = call()
                    wall.append((time.perf_counter() - w0) * 1e3)
                    kms.append(st.kernel_ms[k])
                    visits = st.inner_visits[1 if k == K_SHADOW else 0]
                km, wm = float(np.median(kms)), float(np.median(wall))
                rec = {"scene": name, "rays": set_name, "n": n, "query": query, "entry": entry, "kernel_ms": round(km, 3), "kernel_mrays_s": round(n / km / 1e3, 1),
                       "call_ms": round(wm, 3), "call_mrays_s": round(n / wm / 1e3, 1), "hit_fraction": round(hit_frac[query], 4),
                       "inner_visits_per_ray": round(visits / n, 2)}
                print(json.dumps(rec), flush=True)
        r.close()
        s.close()


if __name__ == "__main__":
    main()
