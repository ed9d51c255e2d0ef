#!/usr/bin/env python3
"""What a pixel list costs, and what adaptive sampling buys (profiles/pixels_cost_1080p.txt).

1. Mrays/s of trt_render_pixels over every pixel of the image (tile order, [0, spp), sums of squares on) against trt_render of the
   same image, in alternating runs, on back, veach-mis and staircase.  Both numbers are the call's device time (trt_stats.render_ms:
   first traversal launch to last resolve); the host entry's copies of the list and the sums lie outside it.
2. veach-mis: the mean per-pixel error estimate (tinyraytracing_amd/adaptive.py) of a fixed --fixed-spp render, then
   render_adaptive (on the device) at a few thresholds around it: wall time, device time, rays, and the mean error reached.

    python3 tools/pixels_cost.py [--width 1920 --height 1080 --spp 64 --runs 3 --fixed-spp 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyraytracing_amd as T  # noqa: E402
from tinyraytracing_amd import adaptive  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}


def all_pixels(p):
    return np.arange(p.width * p.height, dtype=np.uint32)


def list_vs_render(name, a):
    s = T.Scene.named(name, a.width, a.height)
    r = T.Renderer(s, 0)
    p = T.make_params(a.width, a.height, a.spp, SEEDS[name])
    pix = all_pixels(p)
    r.render(p)  # warm-up: code objects, arena
    r.render_pixels(p, pix, 0, a.spp)
    rows = []
    for i in range(a.runs):
        _, st_r = r.render(p)
        _, _, st_l = r.render_pixels(p, pix, 0, a.spp)
        assert (st_r.rays_camera, st_r.rays_shadow, st_r.rays_indirect) == (st_l.rays_camera, st_l.rays_shadow, st_l.rays_indirect)
        rows.append((st_r.rays / st_r.render_ms / 1e3, st_l.rays / st_l.render_ms / 1e3, st_r.render_ms, st_l.render_ms))
    r.close()
    rr = np.array(rows)
    out = {"scene": name, "size": f"{a.width}x{a.height}", "spp": a.spp, "rays": int(st_r.rays),
           "render_mrays": [round(x, 1) for x in rr[:, 0]], "pixels_mrays": [round(x, 1) for x in rr[:, 1]],
           "render_ms": [round(x, 2) for x in rr[:, 2]], "pixels_ms": [round(x, 2) for x in rr[:, 3]],
           "pixels_over_render_median": round(float(np.median(rr[:, 1] / rr[:, 0])), 4)}
    print(json.dumps(out), flush=True)


def adaptive_vs_fixed(a):
    import torch
    s = T.Scene.named("veach-mis", a.width, a.height)
    r = T.Renderer(s, 0)
    p = T.make_params(a.width, a.height, a.fixed_spp, SEEDS["veach-mis"])
    r.render(T.make_params(a.width, a.height, 4, SEEDS["veach-mis"]))  # warm-up
    times = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        _, st_f = r.render(p)
        times.append((time.perf_counter() - t0, st_f.render_ms))
    su, sq, _ = r.render_pixels(p, all_pixels(p), 0, a.fixed_spp)
    target = float(np.mean(adaptive.relative_error(su, sq, np.full(su.shape[0], a.fixed_spp))))
    print(json.dumps({"fixed": {"spp": a.fixed_spp, "wall_s": [round(t, 4) for t, _ in times], "render_ms": [round(m, 2) for _, m in times],
                                "rays": int(st_f.rays), "mean_rel_error": round(target, 5)}}), flush=True)
    for f in a.factors:
        thr = target * f
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = r.render_adaptive(p, thr, a.min_spp, a.max_spp, a.batch, on_device=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        err = float(res.error.mean())
        n = res.counts.double()
        print(json.dumps({"adaptive": {"threshold": round(thr, 5), "min_spp": a.min_spp, "max_spp": a.max_spp, "batch": a.batch,
                                       "wall_s": round(wall, 4), "render_ms_sum": round(res.stats.render_ms, 2), "rounds": res.rounds,
                                       "rays": int(res.stats.rays), "mean_spp": round(float(n.mean()), 2),
                                       "at_max_spp": int((res.counts == a.max_spp).sum()), "mean_rel_error": round(err, 5),
                                       "reaches_fixed_error": err <= target, "wall_over_fixed": round(wall / min(t for t, _ in times), 3)}}),
              flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scenes", default="back,veach-mis,staircase")
    ap.add_argument("--fixed-spp", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--factors", default="1.0,1.3,1.6")
    a = ap.parse_args()
    a.factors = [float(x) for x in a.factors.split(",")]
    for name in filter(None, a.scenes.split(",")):  # --scenes "": the adaptive part only
        list_vs_render(name, a)
    adaptive_vs_fixed(a)


if __name__ == "__main__":
    main()
