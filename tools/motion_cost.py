"""Cost of the motion vectors (profiles/motion_cost_1080p.txt): per scene, at 1920x1080 under the scene's own, still camera,
  - trt_trace_points_device on the centre rays (T.center_rays on the device): the traversal alone (kernel_ms[TRT_K_TRACE_CLOSEST], the entry's
    own hipEvents) and the whole call between two events on its stream (ray packing, traversal, k_hit_points);
  - trt_reproject_motion_device beside trt_reproject_device on the same frame and history in the same run (kernel_ms[TRT_K_DENOISE]), for a
    still scene (a second frame with another seed; the points are the frame's own hit points) and after an object moved
    (trt_update_geometry; the points lie on the previous vertices).
Best of `--reps` after one warm-up call.  Bytes per pixel as tools/reproject_cost.py counts them, plus the 12 B of the point."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import refit_ref  # noqa: E402  (tests/: the moves the refit tests use)
import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "staircase": T.SEED_STAIRCASE}
IN_BYTES, OUT_BYTES, HISTORY_BYTES, POINT_BYTES = 44, 36, 36, 12
KEYS = ("color", "variance", "albedo", "normal", "depth")


def moved(name, s):
    if name == "back":
        return refit_ref.move_inner_object(s, delta=(25.0, 0.0, 0.0), rotate_deg=0.0)[0]
    return refit_ref.move_material(s, "Wood", delta=(0.05, 0.0, 0.0))[0]


def best(fn, reps, slot):
    fn()
    return min((fn() for _ in range(reps)), key=lambda st: st.kernel_ms[slot])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="back,staircase")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    w, h, n = a.width, a.height, a.width * a.height
    dev = torch.device("cuda", 0)
    print(f"{w}x{h} ({n / 1e6:.2f} Mpixels), {a.spp} spp, best of {a.reps} after a warm-up; ms = device time (hipEvents)")
    print(f"  reproject bytes = {IN_BYTES} B in + {OUT_BYTES} B out per pixel + {HISTORY_BYTES} B of history once; the motion entry reads {POINT_BYTES} B more")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, w, h)
        r = T.Renderer(s, 0)
        cam = T.Camera.from_buffer_copy(s.flat.contents.camera)
        v0 = torch.from_numpy(s.arrays()["tri_v"]).to(dev)
        acc = T.TemporalAccumulator(r, T.make_params(w, h, a.spp, SEEDS[name]))
        f0 = acc.frame(cam, on_device=True)
        stream = torch.cuda.current_stream(dev).cuda_stream  # the events below are recorded on it: every timed entry runs there too
        # the history a first frame leaves: reproject_into without one
        hist = {"cv": torch.empty((h, w, 4), dtype=torch.float32, device=dev), "length": torch.empty_like(f0["variance"]), "normal": f0["normal"],
                "depth": f0["depth"]}
        T.reproject_into(*[f0[k] for k in KEYS], cam, None, torch.empty_like(f0["color"]), torch.empty_like(f0["variance"]), hist["cv"], hist["length"],
                         stream_ptr=stream)
        org, dirs = T.center_rays(cam, w, h, 0, device=dev)
        point = torch.empty((n, 3), dtype=torch.float32, device=dev)
        outs = [torch.empty_like(f0["color"]), torch.empty_like(f0["variance"]), torch.empty_like(hist["cv"]), torch.empty_like(f0["variance"])]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        print(f"{name}: {len(v0)} triangles")
        for state in ("still scene", "an object moved"):
            if state != "still scene":
                r.update_geometry(moved(name, s))
            frame = T.TemporalAccumulator(r, T.make_params(w, h, a.spp, SEEDS[name] + 1000)).frame(cam, on_device=True)
            calls = []

            def trace():
                e0.record()
                st = r.trace_points_into(org, dirs, v0, point, stream_ptr=stream)
                e1.record()
                torch.cuda.synchronize(dev)
                calls.append(e0.elapsed_time(e1))
                return st
            st = best(trace, a.reps, 1)
            hit = ~torch.isnan(point[:, 0])
            print(f"  {state}: trt_trace_points_device on the centre rays   traversal {st.kernel_ms[1]:8.4f} ms, whole call {min(calls[1:]):8.4f} ms "
                  f"({100 * float(hit.float().mean()):.1f} % of the rays hit)")
            ins = [frame[k] for k in KEYS]
            rows = (("trt_reproject_device", lambda: T.reproject_into(*ins, cam, cam, *outs, history=hist, stream_ptr=stream), 0),
                    ("trt_reproject_motion_device", lambda: T.reproject_motion_into(*ins, point.view(h, w, 3), cam, cam, *outs, history=hist, stream_ptr=stream), POINT_BYTES))
            for what, fn, extra in rows:
                st = best(fn, a.reps, T.TRT_K_DENOISE)
                ms = st.kernel_ms[T.TRT_K_DENOISE]
                found = float((outs[3][frame["depth"] < T._abi.TRT_INF] > 1).float().mean())
                nbytes = n * (IN_BYTES + OUT_BYTES + HISTORY_BYTES + extra)
                print(f"  {state}: {what:28s} {ms:8.4f} ms  ({nbytes / 1e6:6.1f} MB = {nbytes / (ms * 1e-3) / 1e9:6.0f} GB/s; "
                      f"{100 * found:5.1f} % of the hit pixels found a history)")
        r.close()


if __name__ == "__main__":
    main()
