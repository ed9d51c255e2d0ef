"""What a geometry update costs beside the trt_create it replaces: for each scene the wall time of trt_create, the device time of
trt_update_geometry_device (best of 10 after a warm-up, total and kernels only), and the Mrays/s of trace_closest on the updated handle (A)
and on a fresh handle of the moved scene (B).  Writes profiles/refit_cost.txt.  The one condition checked: the update is the faster one.

    python tools/refit_cost.py [--scenes blob:2000000,blob:10000000,soup:1000000,staircase] [--out profiles/refit_cost.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tinyraytracing_amd as T  # noqa: E402


def mrays(r, org, dirs, reps=5):
    import torch
    dev = torch.device("cuda", r.device)
    o, d = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
    n = o.shape[0]
    t, tri = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    r.trace_closest_into(o, d, t, tri)
    best = min(r.trace_closest_into(o, d, t, tri).kernel_ms[1] for _ in range(reps))
    return n / best / 1e3


def main():
    import torch
    import raygen
    import refit_ref as RR
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="blob:2000000,blob:10000000,soup:1000000,staircase")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_cost.txt"))
    args = ap.parse_args()
    lines = ["scene            tris   create_ms  update_ms  kernels_ms  launches  first_update_wall_ms  create/update  Mrays/s A   Mrays/s B"]
    ok = True
    T.Renderer(T.Scene.named("back", 64, 36), 0).close()  # the process's HIP runtime, context and code objects are up before anything is timed
    for spec in args.scenes.split(","):
        name, _, n = spec.partition(":")
        s = T.Scene.named(name, 64, 36, n=int(n)) if n else T.Scene.named(name, 64, 36)
        create_ms = 1e30
        for _ in range(2):  # best of two: the first one also pages the scene's host arrays in
            t0 = time.perf_counter()
            A = T.Renderer(s, 0)
            create_ms = min(create_ms, (time.perf_counter() - t0) * 1e3)
            if _ == 0:
                A.close()
        a = s.arrays()
        v = RR.jitter(a["tri_v"], amp=0.5) if name == "soup" else RR.smooth_displace(a["tri_v"], amp=0.2 if name == "staircase" else 6.0)
        s.set_vertices(v)
        dev = torch.device("cuda", 0)
        dv = torch.from_numpy(v).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A.update_geometry_from(dv, lights_from=s)  # allocates and numbers the trees (one launch and one read-back per level)
        first = (time.perf_counter() - t0) * 1e3
        runs = [A.update_geometry_from(dv, lights_from=s) for _ in range(10)]
        best = min(runs, key=lambda st: st.render_ms)
        B = T.Renderer(s, 0)
        lo, hi = raygen.scene_bounds(s)
        org, dirs = raygen.random_rays(2_000_000, lo, hi, seed=3)
        ma, mb = mrays(A, org, dirs), mrays(B, org, dirs)
        lines.append(f"{spec:14s} {a['tri_v'].shape[0]:8d} {create_ms:10.1f} {best.render_ms:10.3f} {best.kernel_ms[T.TRT_K_REFIT]:11.3f} "
                     f"{best.launches[T.TRT_K_REFIT]:9d} {first:21.3f} {create_ms / best.render_ms:14.0f} {ma:11.1f} {mb:11.1f}")
        print(lines[-1], flush=True)
        ok = ok and best.render_ms < create_ms
        A.close()
        B.close()
    lines.append("(A = the updated handle, B = a fresh handle of the moved scene: the same node kind, the same boxes.)")
    # what a refit does not do: the tree under a large deformation against a tree rebuilt for the moved triangles
    s = T.Scene.named("blob", 64, 36, n=2000000)
    A = T.Renderer(s, 0)
    v = RR.smooth_displace(s.arrays()["tri_v"], amp=60.0)
    s.set_vertices(v)
    A.update_geometry(s)
    lo, hi = raygen.scene_bounds(s)
    org, dirs = raygen.random_rays(1_000_000, lo, hi, seed=3)
    st_a = A.trace_closest(org, dirs, want_stats=True)[3]
    s.build_bvh(T.DEFAULT_LEAF)  # the moved triangles, a new tree
    R = T.Renderer(s, 0)
    st_r = R.trace_closest(org, dirs, want_stats=True)[3]
    lines.append(f"blob 2 M displaced by up to 60 units (box 556): node visits per ray {st_a.inner_visits[0] / 1e6:.2f} on the refit tree, "
                 f"{st_r.inner_visits[0] / 1e6:.2f} on a rebuilt one; triangle tests {st_a.tri_tests[0] / 1e6:.2f} / {st_r.tri_tests[0] / 1e6:.2f}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("an update was not faster than trt_create")


if __name__ == "__main__":
    main()
