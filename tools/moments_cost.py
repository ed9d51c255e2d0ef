"""Cost of trt_reproject_moments_device (profiles/moments_cost_1080p.txt): per scene a TemporalAccumulator(variance="moments") at
1920x1080 and one sample per pixel renders four frames under a still camera, a fifth, and a sixth with the camera orbited by one degree;
the frames and the histories stay on the device.  trt_reproject_moments_device is then timed on a first frame (no history: every hit pixel
through stage B), on the still camera's fifth frame and on the moved camera's frame (stage B's blocks vote and return wherever the history
is four frames long), best of `--reps` after one warm-up call, with stage B's LDS tile and without it (TRT_MOMENTS_LDS=0), beside
trt_reproject_device on the same buffers and trt_denoise_device at 5 levels on the same frame in the same run.
ms = device time from the entry's own hipEvents (kernel_ms[TRT_K_DENOISE]: both kernels).  The bytes a call must move are counted from
the shapes: 32 B per pixel of the current frame in, 52 B out, the 52 B of a history pixel once, and stage B's 12 B per pixel (depth,
length, s) for the vote; the rate is set against the 4.8 TB/s k_denoise_prepare reaches on this chip."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import reproject_ref  # noqa: E402  (tests/: the orbit around the shipped scenes' views, shared with the tests)
import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "staircase": T.SEED_STAIRCASE}
PREPARE_RATE = 4.8e12
IN_BYTES, OUT_BYTES, HISTORY_BYTES, VOTE_BYTES = 32, 52, 52, 12


def best(fn, reps):
    fn()
    return min((fn() for _ in range(reps)), key=lambda st: st.kernel_ms[T.TRT_K_DENOISE])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="back,staircase")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_cost_1080p.txt"))
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.width * a.height
    say(f"{a.width}x{a.height} ({n / 1e6:.2f} Mpixels), 1 spp, best of {a.reps} after a warm-up; ms = device time of the call's kernels (hipEvents)")
    say(f"  bytes = {IN_BYTES} B in + {OUT_BYTES} B out + {VOTE_BYTES} B for stage B's vote per pixel, + {HISTORY_BYTES} B of history per pixel once; the taps gather up to 4 x 52 B through L2")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, a.width, a.height)
        r = T.Renderer(s, 0)
        acc = T.TemporalAccumulator(r, T.make_params(a.width, a.height, 1, SEEDS[name]), variance="moments")
        cams = [reproject_ref.orbit_camera(name, k, a.width, a.height) for k in (0.0, 1.0)]
        for _ in range(4):
            acc.frame(cams[0], on_device=True)
        hist4 = dict(acc._history)
        f5 = acc.frame(cams[0], on_device=True)
        hist5 = dict(acc._history)
        f6 = acc.frame(cams[1], on_device=True)
        keys = ("color", "albedo", "normal", "depth")
        outs = [torch.empty_like(f6["color"]), torch.empty_like(f6["depth"]), torch.empty_like(hist5["cv"]), torch.empty_like(f6["depth"]), torch.empty_like(hist5["cv"])]
        hit6 = f6["depth"] < T._abi.TRT_INF
        say(f"{name}: hit pixels {100 * float(hit6.float().mean()):.1f} %")
        for what, frame, cur, h, prev in (("first frame (no history)", f6, cams[1], None, None), ("still camera, fifth frame", f5, cams[0], hist4, cams[0]),
                                          ("camera moved by 1 degree", f6, cams[1], hist5, cams[0])):
            ins = [frame[k] for k in keys]
            hit = frame["depth"] < T._abi.TRT_INF
            for lds in ("1", "0"):
                os.environ["TRT_MOMENTS_LDS"] = lds
                st = best(lambda: T.reproject_moments_into(*ins, cur, prev, *outs, history=h), a.reps)
                ms = st.kernel_ms[T.TRT_K_DENOISE]
                route = hit & (outs[3] >= 4) & (1.0 - outs[4][..., 2] >= 0.1)
                nbytes = n * (IN_BYTES + OUT_BYTES + VOTE_BYTES + (HISTORY_BYTES if h is not None else 0))
                rate = nbytes / (ms * 1e-3)
                say(f"  trt_reproject_moments_device, {what:26s} {'LDS tile' if lds == '1' else 'global  '} {ms:8.4f} ms  ({nbytes / 1e6:6.1f} MB = {rate / 1e9:6.0f} GB/s, "
                    f"{100 * rate / PREPARE_RATE:5.1f} % of k_denoise_prepare's 4.8 TB/s; {100 * float(route.sum()) / max(1.0, float(hit.sum())):5.1f} % of the hit pixels on the temporal route)")
            os.environ.pop("TRT_MOMENTS_LDS")
            h4 = None if h is None else {k: h[k] for k in T.HISTORY_KEYS}
            st = best(lambda: T.reproject_into(ins[0], frame["accumulated_variance"], *ins[1:], cur, prev, *outs[:4], history=h4), a.reps)
            say(f"  trt_reproject_device,         {what:26s}          {st.kernel_ms[T.TRT_K_DENOISE]:8.4f} ms")
        res = torch.empty_like(f6["color"])
        st = best(lambda: T.denoise_into(f6["accumulated"], f6["accumulated_variance"], f6["albedo"], f6["normal"], f6["depth"], res, iterations=5), a.reps)
        say(f"  trt_denoise_device 5 levels on the same frame                          {st.kernel_ms[T.TRT_K_DENOISE]:8.4f} ms")
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
