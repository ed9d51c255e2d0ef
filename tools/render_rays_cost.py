#!/usr/bin/env python3
"""What rendering through caller-supplied rays costs (profiles/render_rays_cost.txt).

A camera that moves on a resident handle renders as Renderer.render_camera does: per batch of samples one trt_camera_rays_device call
(the rays into device arrays) and one trt_render_rays_device call (bounce 0 read from those arrays through the ray queue).  This tool times
that loop — wall time around the whole loop, device tensors in, device sums out, and the summed trt_stats.render_ms — against ONE
trt_render_device call of the same workload, whose camera rays never leave the registers.

The baseline is meant to be the PARENT commit's library: --baseline-lib names a libtrt_hip.so built from it, and the baseline runs in a
child process that binds only the entries that library has.  Without --baseline-lib the child loads this tree's library (the render
kernels of the two are the same code objects; tools/kernel_meta.py shows it).

    python3 tools/render_rays_cost.py [--baseline-lib PATH] [--width 1920 --height 1080 --spp 16 --runs 5 --scenes back,soup]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinyraytracing_amd as T  # noqa: E402
from tinyraytracing_amd import _abi  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "soup": T.SEED_SOUP, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}


def baseline_child(a):
    """trt_render_device of the library at a.baseline_lib (or this tree's), bound by hand: an older library lacks the newer entries."""
    import torch
    _abi._bind_to_torch_hip_runtime()
    lib = C.CDLL(a.baseline_lib or os.path.join(_abi.LIB_DIR, "libtrt_hip.so"))
    lib.trt_last_error.restype = C.c_char_p
    lib.trt_create.argtypes = [C.POINTER(_abi.SceneFlat), C.c_int, C.POINTER(C.c_void_p)]
    lib.trt_render_device.argtypes = [C.c_void_p, C.POINTER(_abi.Params), C.c_void_p, C.c_void_p, C.POINTER(_abi.Stats)]
    lib.trt_destroy.argtypes = [C.c_void_p]
    lib.trt_destroy.restype = None
    dev = torch.device("cuda", 0)
    for name in a.scene_list:
        s = T.Scene.named(name, a.width, a.height)
        h = C.c_void_p()
        if lib.trt_create(s.flat, 0, C.byref(h)) != 0:
            raise SystemExit(f"trt_create failed: {lib.trt_last_error().decode()}")
        p = T.make_params(a.width, a.height, a.spp, SEEDS[name])
        out = torch.empty((a.height, a.width, 3), dtype=torch.float32, device=dev)
        st = _abi.Stats()
        wall, ms = [], []
        for i in range(a.runs + 1):  # the first run warms up: code objects, arena
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if lib.trt_render_device(h, C.byref(p), C.c_void_p(out.data_ptr()), None, C.byref(st)) != 0:
                raise SystemExit(f"trt_render_device failed: {lib.trt_last_error().decode()}")
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(st.render_ms)
        lib.trt_destroy(h)
        print(json.dumps({"baseline": name, "wall_ms": wall, "render_ms": ms, "rays": int(st.rays_camera + st.rays_shadow + st.rays_indirect),
                          "checksum": float(out.double().sum().item())}), flush=True)


def camera_loop(name, a, base):
    import torch
    s = T.Scene.named(name, a.width, a.height)
    r = T.Renderer(s, 0)
    p = T.make_params(a.width, a.height, a.spp, SEEDS[name])
    cam = s.flat.contents.camera  # the handle's own camera: the same image, so the same rays, as the baseline
    rows = []
    for k in a.batches:
        wall, ms = [], []
        for i in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img, st = r.render_camera(p, cam, samples_per_call=k, want_stats=True, on_device=True)
            torch.cuda.synchronize()
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(st.render_ms)
        assert int(st.rays) == base["rays"], "the two sides traced different rays"
        assert float(img.double().sum().item()) == base["checksum"], "the two sides rendered different images"
        rows.append({"samples_per_call": k, "wall_ms": [round(x, 2) for x in wall], "render_ms_sum": [round(x, 2) for x in ms],
                     "wall_over_baseline_wall": round(float(np.median(wall) / np.median(base["wall_ms"])), 4),
                     "device_over_baseline_device": round(float(np.median(ms) / np.median(base["render_ms"])), 4)})
    r.close()
    return {"scene": name, "size": f"{a.width}x{a.height}", "spp": a.spp, "rays": base["rays"],
            "baseline_lib": a.baseline_lib or "this tree's", "baseline_wall_ms": [round(x, 2) for x in base["wall_ms"]],
            "baseline_render_ms": [round(x, 2) for x in base["render_ms"]], "camera_loop": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scenes", default="back,soup")
    ap.add_argument("--batches", default="1,4,16", help="samples per trt_render_rays_device call")
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--baseline-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.scene_list = [x for x in a.scenes.split(",") if x]
    a.batches = [int(x) for x in a.batches.split(",")]
    if a.baseline_child:
        return baseline_child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-child", "--width", str(a.width), "--height", str(a.height), "--spp", str(a.spp),
           "--runs", str(a.runs), "--scenes", a.scenes, "--baseline-lib", a.baseline_lib]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    base = {}
    for line in out.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            base[rec["baseline"]] = rec
    for name in a.scene_list:
        print(json.dumps(camera_loop(name, a, base[name])), flush=True)


if __name__ == "__main__":
    main()
