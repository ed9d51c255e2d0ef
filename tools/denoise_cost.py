"""Cost of trt_denoise_device next to a render (profiles/denoise_cost_1080p.txt): per scene, the inputs of a 16-spp render_denoised at
1920x1080 are put on the device once, then trt_denoise_device runs 1, 3 and 5 levels (and the 5 levels once more with TRT_DENOISE_LDS=0:
every level from global memory), best of `--reps` after one warm-up call, next to trt_render of the same scene at 16 spp.
ms = device time from the entry's own hipEvents (kernel_ms[TRT_K_DENOISE]).  Run it under rocprofv3 --kernel-trace --stats for the
per-kernel view."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "staircase": T.SEED_STAIRCASE, "veach-mis": 0x5EED0002}
KEYS = ("color", "variance", "albedo", "normal", "depth")


def best(fn, reps):
    fn()
    return min((fn() for _ in range(reps)), key=lambda st: st.kernel_ms[T.TRT_K_DENOISE] or st.render_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="back,staircase")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    n = a.width * a.height
    print(f"{a.width}x{a.height} ({n / 1e6:.2f} Mpixels), best of {a.reps} after a warm-up; ms = device time of the call's kernels (hipEvents)")
    print("  bytes = each level's compulsory traffic: cv in + guide + aux + cv out = 64 B per pixel (the last level writes 12 B of RGB instead of 16),")
    print("          plus 56 B in and 64 B out for the prepare kernel; the taps re-read cv and the guide 25x through L2 / LDS")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, a.width, a.height)
        r = T.Renderer(s, 0)
        p = T.make_params(a.width, a.height, a.spp, SEEDS[name], flags=T.TRT_FLAG_TIMING)
        full = min((r.render(p)[1] for _ in range(3)), key=lambda st: st.render_ms)
        out = r.render_denoised(T.make_params(a.width, a.height, a.spp, SEEDS[name]))
        ins = [torch.from_numpy(np.ascontiguousarray(out[k])).to(dev) for k in KEYS]
        res = torch.empty((a.height, a.width, 3), dtype=torch.float32, device=dev)
        print(f"{name}: trt_render {a.spp} spp {full.render_ms:8.3f} ms; hit pixels {100 * np.mean(out['depth'] < T._abi.TRT_INF):.1f} %")
        ms = {}
        for levels in (1, 3, 5):
            st = best(lambda: T.denoise_into(*ins, res, iterations=levels), a.reps)
            ms[levels] = st.kernel_ms[T.TRT_K_DENOISE]
            nbytes = n * (120 + 64 * levels - 4)
            print(f"  trt_denoise_device {levels} level{'s' if levels > 1 else ' '}  {ms[levels]:8.4f} ms  ({100 * ms[levels] / full.render_ms:5.2f} % of the render;"
                  f" compulsory bytes {nbytes / 1e6:6.1f} MB = {nbytes / ms[levels] / 1e6:6.0f} GB/s)")
        os.environ["TRT_DENOISE_LDS"] = "0"
        st = best(lambda: T.denoise_into(*ins, res, iterations=5), a.reps)
        del os.environ["TRT_DENOISE_LDS"]
        print(f"  trt_denoise_device 5 levels, no LDS tiles {st.kernel_ms[T.TRT_K_DENOISE]:8.4f} ms")
        per = (ms[5] - ms[1]) / 4
        print(f"  per wide level (steps 2..16, (5 levels - 1 level) / 4): {per:7.4f} ms = {n / per / 1e6:7.1f} Gpixels/s; level 0 + prepare {ms[1]:7.4f} ms")
        host = T.denoise(*(out[k] for k in KEYS), want_stats=True)[1]
        print(f"  trt_denoise (host buffers, 5 levels): {host.render_ms:8.3f} ms with the copies, {host.kernel_ms[T.TRT_K_DENOISE]:7.4f} ms kernels")
        del ins, res
        r.close()


if __name__ == "__main__":
    main()
