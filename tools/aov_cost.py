"""Cost of trt_render_aov next to trt_render (profiles/aov_cost_1080p_16spp.txt): per scene, the AOV call at 16 spp, a full render at 16 spp,
and a render cut after its camera rays (max_depth 1: its trace_closest time is bounce 0 alone), every one with TRT_FLAG_TIMING, best of
`--reps` after one warm-up call.  Run it under rocprofv3 --kernel-trace --stats for the per-kernel view."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinyraytracing_amd as T  # noqa: E402

SEEDS = {"back": T.SEED_BACK, "staircase": T.SEED_STAIRCASE, "veach-mis": 0x5EED0002}


def best(fn, reps):
    fn()
    runs = [fn() for _ in range(reps)]
    return min(runs, key=lambda st: st.render_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="back,staircase")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    k_tr, k_res = T.KERNEL_NAMES.index("trace_closest"), T.KERNEL_NAMES.index("resolve")
    print(f"{a.width}x{a.height}, {a.spp} spp, best of {a.reps}; ms = device time (TRT_FLAG_TIMING), ns/ray = trace_closest ms / camera rays")
    for name in a.scenes.split(","):
        s = T.Scene.named(name, a.width, a.height)
        r = T.Renderer(s, 0)
        p = T.make_params(a.width, a.height, a.spp, SEEDS[name], flags=T.TRT_FLAG_TIMING)
        aov = best(lambda: r.render_aov(p, want_stats=True)[1], a.reps)
        full = best(lambda: r.render(p)[1], a.reps)
        p1 = T.make_params(a.width, a.height, a.spp, SEEDS[name], flags=T.TRT_FLAG_TIMING, max_depth=1)
        b0 = best(lambda: r.render(p1)[1], a.reps)
        print(f"{name}: {s.flat.contents.n_tris} triangles, inner node bytes {aov.inner_node_bytes}, redo rays {aov.redo_rays}, passes {aov.passes}")
        print(f"  trt_render_aov         total {aov.render_ms:8.3f} ms  trace_closest {aov.kernel_ms[k_tr]:8.3f} ms ({1e6 * aov.kernel_ms[k_tr] / aov.rays_camera:.3f} ns/ray)"
              f"  k_aov + finalize {aov.kernel_ms[k_res]:7.3f} ms ({100 * aov.kernel_ms[k_res] / aov.kernel_ms[k_tr]:.1f} % of the traversal)")
        print(f"  trt_render max_depth 1 total {b0.render_ms:8.3f} ms  trace_closest {b0.kernel_ms[k_tr]:8.3f} ms ({1e6 * b0.kernel_ms[k_tr] / b0.rays_camera:.3f} ns/ray, bounce 0)")
        print(f"  trt_render             total {full.render_ms:8.3f} ms  ({full.rays / full.render_ms / 1e3:.0f} Mrays/s); AOV call = {100 * aov.render_ms / full.render_ms:.1f} % of the render")
        r.close()


if __name__ == "__main__":
    main()
