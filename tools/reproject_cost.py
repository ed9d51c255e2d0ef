"""Cost of trt_reproject_device (profiles/reproject_cost_1080p.txt): per scene two frames of a TemporalAccumulator at 1920x1080, the
camera orbited by one degree between them, and the first camera's frame once more with another seed are left on the device;
trt_reproject_device then blends the moved frame, and the still camera's second frame, into the first frame's history, best of `--reps` after one warm-up call, beside trt_denoise_device at 5 levels on the same frame in the same run.
ms = device time from the entry's own hipEvents (kernel_ms[TRT_K_DENOISE]).  The bytes a call must move are counted from the shapes:
44 B per pixel of the current frame in, 36 B out, and the 36 B of a history pixel once (the four taps of neighbouring pixels share their
reads through L2); the rate is set against the 4.8 TB/s k_denoise_prepare reaches on this chip."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import reproject_ref  # noqa: E402  (tests/: the orbit around the shipped scenes' views, shared with the tests)
import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "staircase": T.SEED_STAIRCASE}
PREPARE_RATE = 4.8e12
IN_BYTES, OUT_BYTES, HISTORY_BYTES = 44, 36, 36


def best(fn, reps):
    fn()
    return min((fn() for _ in range(reps)), key=lambda st: st.kernel_ms[T.TRT_K_DENOISE])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="back,staircase")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    n = a.width * a.height
    print(f"{a.width}x{a.height} ({n / 1e6:.2f} Mpixels), {a.spp} spp, best of {a.reps} after a warm-up; ms = device time of the call's kernels (hipEvents)")
    print(f"  bytes = {IN_BYTES} B in + {OUT_BYTES} B out per pixel, + {HISTORY_BYTES} B of history per pixel once; the taps gather up to 4 x 36 B through L2")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, a.width, a.height)
        r = T.Renderer(s, 0)
        acc = T.TemporalAccumulator(r, T.make_params(a.width, a.height, a.spp, SEEDS[name]))
        cams = [reproject_ref.orbit_camera(name, k, a.width, a.height) for k in (0.0, 1.0)]
        f0 = acc.frame(cams[0], on_device=True)
        hist = {"cv": acc._history["cv"], "length": acc._history["length"], "normal": f0["normal"], "depth": f0["depth"]}
        f1 = acc.frame(cams[1], on_device=True)
        # the first camera once more with another seed: a still camera's second frame
        again = T.TemporalAccumulator(r, T.make_params(a.width, a.height, a.spp, SEEDS[name] + 1000))
        f0b = again.frame(cams[0], on_device=True)
        keys = ("color", "variance", "albedo", "normal", "depth")
        outs = [torch.empty_like(f1["color"]), torch.empty_like(f1["variance"]), torch.empty_like(hist["cv"]), torch.empty_like(f1["variance"])]
        hit = (f1["depth"] < T._abi.TRT_INF)
        used = float((f1["history_length"][hit] > 1).float().mean())
        print(f"{name}: hit pixels {100 * float(hit.float().mean()):.1f} %, {100 * used:.1f} % of them found their history after the move")
        for what, frame, cur, h, prev in (("first frame (no history)", f1, cams[1], None, None), ("still camera", f0b, cams[0], hist, cams[0]),
                                          ("camera moved by 1 degree", f1, cams[1], hist, cams[0])):
            ins = [frame[k] for k in keys]
            st = best(lambda: T.reproject_into(*ins, cur, prev, *outs, history=h), a.reps)
            ms = st.kernel_ms[T.TRT_K_DENOISE]
            found = float((outs[3][frame["depth"] < T._abi.TRT_INF] > 1).float().mean()) if h is not None else 0.0
            nbytes = n * (IN_BYTES + OUT_BYTES + (HISTORY_BYTES if h is not None else 0))
            rate = nbytes / (ms * 1e-3)
            print(f"  trt_reproject_device, {what:26s} {ms:8.4f} ms  ({nbytes / 1e6:6.1f} MB = {rate / 1e9:6.0f} GB/s, {100 * rate / PREPARE_RATE:5.1f} % of k_denoise_prepare's 4.8 TB/s;"
                  f" {100 * found:5.1f} % of the hit pixels found their history)")
        res = torch.empty_like(f1["color"])
        st = best(lambda: T.denoise_into(f1["accumulated"], f1["accumulated_variance"], f1["albedo"], f1["normal"], f1["depth"], res, iterations=5), a.reps)
        print(f"  trt_denoise_device 5 levels on the same frame      {st.kernel_ms[T.TRT_K_DENOISE]:8.4f} ms")
        r.close()


if __name__ == "__main__":
    main()
