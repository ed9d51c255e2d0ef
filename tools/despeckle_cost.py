"""Cost and effect of trt_despeckle_device (profiles/despeckle_cost_1080p.txt).
Cost: per scene a TemporalAccumulator(variance="moments") at 1920x1080 and one sample per pixel renders a frame and a second one with the
camera orbited by one degree; the frames and the history stay on the device.  trt_despeckle_device is then timed on the second frame at
R = 1 and R = 2, with the LDS tile and without it (TRT_DESPECKLE_LDS=0), best of `--reps` after one warm-up call, beside
trt_reproject_device on the same frame with the first frame's history (a moved camera) and trt_denoise_device at 5 levels in the same run.
ms = device time from the entry's own hipEvents (kernel_ms[TRT_K_DENOISE]).  The bytes a call must move are counted from the shapes: 28 B
per pixel in (colour, albedo, depth), 16 B out (colour, scale); the rate is set against the 4.8 TB/s k_denoise_prepare reaches on this chip
(DESIGN.md 7.1).
Effect: per scene 8 frames of a one-degree-per-frame orbit at `--quality-size` and one sample per pixel on the moments route, with and
without the clamp (the same seeds), against a render of the last camera at `--quality-spp` samples: the tonemapped MSE of the last frame's
denoised image, tonemap clip(min(x, 1e3), 0)^(1/2.2) over all pixels and channels, and the ratio of the two images' mean values."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import reproject_ref  # noqa: E402  (tests/: the orbit around the shipped scenes' views, shared with the tests)
import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "staircase": T.SEED_STAIRCASE}
PREPARE_RATE = 4.8e12
IN_BYTES, OUT_BYTES = 28, 16


def best(fn, reps):
    fn()
    return min((fn() for _ in range(reps)), key=lambda st: st.kernel_ms[T.TRT_K_DENOISE])


def tonemapped_mse(image, reference):
    tm = lambda x: np.clip(np.minimum(np.asarray(x, np.float64), 1e3), 0.0, None) ** (1 / 2.2)  # noqa: E731
    return float(np.mean((tm(image) - tm(reference)) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="back,staircase")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quality-size", default="320x240")
    ap.add_argument("--quality-spp", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despeckle_cost_1080p.txt"))
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.width * a.height
    say(f"{a.width}x{a.height} ({n / 1e6:.2f} Mpixels), 1 spp, best of {a.reps} after a warm-up; ms = device time of the call's kernels (hipEvents)")
    say(f"  bytes = {IN_BYTES} B in (colour, albedo, depth) + {OUT_BYTES} B out (colour, scale) per pixel")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, a.width, a.height)
        r = T.Renderer(s, 0)
        acc = T.TemporalAccumulator(r, T.make_params(a.width, a.height, 1, SEEDS[name]), variance="moments")
        cams = [reproject_ref.orbit_camera(name, k, a.width, a.height) for k in (0.0, 1.0)]
        acc.frame(cams[0], on_device=True)
        hist = {k: acc._history[k] for k in T.HISTORY_KEYS}
        f = acc.frame(cams[1], on_device=True)
        out_color, out_scale = torch.empty_like(f["color"]), torch.empty_like(f["depth"])
        hit = f["depth"] < T._abi.TRT_INF
        say(f"{name}: hit pixels {100 * float(hit.float().mean()):.1f} %")
        for radius in (1, 2):
            for lds in ("1", "0"):
                os.environ["TRT_DESPECKLE_LDS"] = lds
                st = best(lambda: T.despeckle_into(f["color"], f["albedo"], f["depth"], out_color, out_scale=out_scale, radius=radius), a.reps)
                ms = st.kernel_ms[T.TRT_K_DENOISE]
                nbytes = n * (IN_BYTES + OUT_BYTES)
                rate = nbytes / (ms * 1e-3)
                touched = float((out_scale != 1.0).sum()) / max(1.0, float(hit.sum()))
                say(f"  trt_despeckle_device R = {radius}, {'LDS tile' if lds == '1' else 'global  '} {ms:8.4f} ms  ({nbytes / 1e6:6.1f} MB = {rate / 1e9:6.0f} GB/s, "
                    f"{100 * rate / PREPARE_RATE:5.1f} % of k_denoise_prepare's 4.8 TB/s; {100 * touched:5.2f} % of the hit pixels clamped or replaced)")
            os.environ.pop("TRT_DESPECKLE_LDS")
        outs = [torch.empty_like(f["color"]), torch.empty_like(f["depth"]), torch.empty_like(hist["cv"]), torch.empty_like(f["depth"])]
        st = best(lambda: T.reproject_into(f["color"], f["accumulated_variance"], f["albedo"], f["normal"], f["depth"], cams[1], cams[0], *outs, history=hist), a.reps)
        say(f"  trt_reproject_device, camera moved by 1 degree      {st.kernel_ms[T.TRT_K_DENOISE]:8.4f} ms")
        res = torch.empty_like(f["color"])
        st = best(lambda: T.denoise_into(f["accumulated"], f["accumulated_variance"], f["albedo"], f["normal"], f["depth"], res, iterations=5), a.reps)
        say(f"  trt_denoise_device 5 levels on the same frame       {st.kernel_ms[T.TRT_K_DENOISE]:8.4f} ms")
        r.close()
        s.close()
    qw, qh = (int(x) for x in a.quality_size.split("x"))
    say(f"effect: {a.frames} frames of a 1-degree-per-frame orbit at {qw}x{qh}, 1 spp, variance=\"moments\", against {a.quality_spp} spp of the last camera; R = 1, sigma 3")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, qw, qh)
        r = T.Renderer(s, 0)
        p = T.make_params(qw, qh, 1, SEEDS[name])
        plain, clamp = T.TemporalAccumulator(r, p, variance="moments"), T.TemporalAccumulator(r, p, variance="moments", despeckle=True)
        touched = []
        for k in range(a.frames):
            cam = reproject_ref.orbit_camera(name, float(k), qw, qh)
            a_out, b_out = plain.frame(cam), clamp.frame(cam)
            touched.append(float((b_out["despeckle_scale"] != 1.0).sum()) / max(1, int((b_out["depth"] < T._abi.TRT_INF).sum())))
        ref = r.render_camera(T.make_params(qw, qh, a.quality_spp, SEEDS[name] + 0x1000), cam, samples_per_call=64)
        for key in ("accumulated", "denoised"):
            ma, mb = tonemapped_mse(a_out[key], ref), tonemapped_mse(b_out[key], ref)
            ea, eb = float(a_out[key].astype(np.float64).mean()), float(b_out[key].astype(np.float64).mean())
            say(f"  {name:10s} {key:11s} tonemapped MSE without the clamp {ma:.5f}, with it {mb:.5f} (ratio {mb / ma:.3f}); mean with / without {eb / ea:.4f}")
        say(f"  {name:10s} {100 * float(np.mean(touched)):.2f} % of the hit pixels clamped per frame; mean of the {a.quality_spp}-spp render {float(np.asarray(ref, np.float64).mean()):.5f}, "
            f"of the denoised image without the clamp {float(a_out['denoised'].astype(np.float64).mean()):.5f}")
        r.close()
        s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f_:
        f_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
