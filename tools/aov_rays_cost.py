#!/usr/bin/env python3
"""What first-hit feature buffers through caller-supplied rays cost (profiles/aov_rays_cost.txt).

A camera that moves on a resident handle gets its albedo, normal and depth as Renderer.render_camera_aov does: per batch of samples one
trt_camera_rays_device call (the rays into device arrays) and one trt_aov_rays_device call (the rays packed into queue records, walked by
the queue flavour of the closest-hit kernel, accumulated by k_aov_rays).  This tool times that loop on the device — HIP events around the
whole loop on torch's current stream, ray generation included, and the summed trt_stats.render_ms of the trt_aov_rays_device calls — with
every sample in one call and with one sample per call, against ONE trt_render_aov_device call of the same workload on the SAME handle,
whose camera rays never leave the registers.  Both sides use the handle's own camera, so they trace the same rays and must give the same
buffers; the tool checks that.  Best of --runs after a warm-up run.

    python3 tools/aov_rays_cost.py [--width 1920 --height 1080 --spp 16 --runs 10 --scenes back,soup]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "soup": T.SEED_SOUP, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}
KEYS = ("albedo", "normal", "depth")


def timed(torch, runs, call):
    """Best device time (HIP events on the current stream) and best summed render_ms of `runs` calls after one warm-up call; the last result."""
    ev_ms, st_ms, out = [], [], None
    for i in range(runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out, st = call()
        e1.record()
        torch.cuda.synchronize()
        if i:
            ev_ms.append(e0.elapsed_time(e1))
            st_ms.append(st.render_ms)
    return min(ev_ms), min(st_ms), out, st


def measure(name, a):
    import torch
    dev = torch.device("cuda", 0)
    s = T.Scene.named(name, a.width, a.height)
    r = T.Renderer(s, 0)
    p = T.make_params(a.width, a.height, a.spp, SEEDS[name])
    cam = s.flat.contents.camera
    n = a.width * a.height
    bufs = {"albedo": torch.empty((a.height, a.width, 3), dtype=torch.float32, device=dev), "normal": torch.empty((a.height, a.width, 3), dtype=torch.float32, device=dev),
            "depth": torch.empty((a.height, a.width), dtype=torch.float32, device=dev)}
    stream = torch.cuda.current_stream(dev).cuda_stream
    base_ev, base_ms, ref, st = timed(torch, a.runs, lambda: (bufs, r.render_aov_into(p, stream_ptr=stream, **bufs)))
    ref = {k: v.clone() for k, v in ref.items()}
    rows = []
    for k in (a.spp, 1):
        ev, ms, out, st_k = timed(torch, a.runs, lambda: r.render_camera_aov(p, cam, samples_per_call=k, want_stats=True, on_device=True))
        assert st_k.rays_camera == n * a.spp == st.rays_camera, "the two sides traced different rays"
        for key in KEYS:
            assert torch.equal(out[key].view(torch.int32), ref[key].view(torch.int32)), f"{key}: the two sides gave different buffers"
        rows.append({"samples_per_call": k, "loop_device_ms": round(ev, 3), "aov_rays_render_ms_sum": round(ms, 3),
                     "kernel_launches": {"pack": int(st_k.launches[0]), "trace_closest": int(st_k.launches[1]), "resolve": int(st_k.launches[4])},
                     "loop_over_render_aov": round(ev / base_ev, 4), "render_ms_over_render_aov": round(ms / base_ms, 4)})
    r.close()
    return {"scene": name, "size": f"{a.width}x{a.height}", "spp": a.spp, "rays": n * a.spp, "runs": a.runs,
            "render_aov_device_ms": round(base_ev, 3), "render_aov_render_ms": round(base_ms, 3), "render_camera_aov": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--scenes", default="back,soup")
    a = ap.parse_args()
    for name in [x for x in a.scenes.split(",") if x]:
        print(json.dumps(measure(name, a)), flush=True)


if __name__ == "__main__":
    main()
