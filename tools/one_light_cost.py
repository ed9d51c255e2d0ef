#!/usr/bin/env python3
"""What TRT_FLAG_ONE_LIGHT costs and buys on one MI355X -> profiles/one_light_cost.txt (a GPU run; nothing here is asserted).

  (1) per render: `lamps` n = 8, 16, 64 and `staircase` at 1920 x 1080 x 64 spp with TRT_FLAG_FIXED_NEE alone (every light at every vertex)
      and with TRT_FLAG_ONE_LIGHT: ms per render (two timed renders after a warm-up), Mrays/s, launches, passes, shadow rays;
  (2) per kernel: kernel_ms of one TRT_FLAG_TIMING render each;
  (3) at equal device time: the one-light spp whose render time is closest to the all-lights 64-spp time, and both images' tonemapped MSE
      at 320 x 180 against an all-lights render at 4096 spp with another seed;
  (4) with --ab LIB: the same one-light renders on another build of the HIP library (make variants: the 256-thread arm of k_shade's SHADE_PICK),
      in a child process each (TRT_HIP_LIB is read when the library is loaded).

    python tools/one_light_cost.py [--out profiles/one_light_cost.txt] [--quick] [--ab tinyraytracing_amd/lib/variants/libtrt_hip_shadep256.so]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SCENES = [("lamps", {"n": 8}), ("lamps", {"n": 16}), ("lamps", {"n": 64}), ("staircase", {})]
SEED, SEED_REF = 0x5EED0002, 0x5EED0A11


def label(name, kw):
    return f"{name} n={kw['n']}" if kw else name


def timed(r, p, repeats=2):
    r.render(p)  # warm-up
    return [r.render(p)[1] for _ in range(repeats)]


def per_render(T, w, h, spp, quick):
    """-> rows for (1) and (2), and the per-scene all-lights / one-light times for (3)."""
    K = {n: i for i, n in enumerate(T.KERNEL_NAMES)}
    rows, kernels, times = [], [], {}
    for name, kw in SCENES:
        s = T.Scene.named(name, w, h, **kw)
        r = T.Renderer(s, 0)
        for what, flags in (("all lights", T.TRT_FLAG_FIXED_NEE), ("one light", T.TRT_FLAG_FIXED_NEE | T.TRT_FLAG_ONE_LIGHT)):
            p = T.make_params(w, h, spp, SEED, flags=flags)
            sts = timed(r, p)
            ms = [st.render_ms for st in sts]
            st = sts[-1]
            rows.append(f"{label(name, kw):12s} {s.info['n_lights']:3d} lights  {what:10s}  {ms[0]:8.2f} / {ms[1]:8.2f} ms   {st.rays / ms[1] / 1e3:9.0f} Mrays/s   "
                        f"passes {st.passes}   shadow rays {st.rays_shadow:13d}   launches closest {st.launches[K['trace_closest']]}, shade {st.launches[K['shade']]}, "
                        f"shadow {st.launches[K['trace_shadow']]}, resolve {st.launches[K['resolve']]}, tail {st.launches[K['tail']]}")
            times[(label(name, kw), what)] = min(ms)
            tst = r.render(T.make_params(w, h, spp, SEED, flags=flags | T.TRT_FLAG_TIMING))[1]
            km = [tst.kernel_ms[K[k]] for k in ("trace_closest", "shade", "trace_shadow", "resolve", "tail")]
            kernels.append(f"{label(name, kw):12s} {what:10s}  " + ", ".join(f"{x:8.2f}" for x in km) + f"   shadow {100 * km[2] / max(sum(km), 1e-9):5.1f} %")
        r.close()
        s.close()
    return rows, kernels, times


def equal_time(T, times, spp, quick):
    """(3): time per sample scales with the pixel count, so the spp chosen at full size is used at 320 x 180."""
    out = []
    w, h = 320, 180
    ref_spp = 256 if quick else 4096
    for name, kw in SCENES:
        lab = label(name, kw)
        t_all, t_one = times[(lab, "all lights")], times[(lab, "one light")]
        one_spp = max(1, int(round(spp * t_all / t_one)))
        s = T.Scene.named(name, w, h, **kw)
        r = T.Renderer(s, 0)
        ref = r.render(T.make_params(w, h, ref_spp, SEED_REF, flags=T.TRT_FLAG_FIXED_NEE))[0]
        a = r.render(T.make_params(w, h, spp, SEED, flags=T.TRT_FLAG_FIXED_NEE))[0]
        b = r.render(T.make_params(w, h, one_spp, SEED, flags=T.TRT_FLAG_FIXED_NEE | T.TRT_FLAG_ONE_LIGHT))[0]
        tm = lambda x: T.tonemap(x).astype(np.float64) / 255.0  # noqa: E731
        mse = lambda x: float(((tm(x) - tm(ref)) ** 2).mean())  # noqa: E731
        out.append(f"{lab:12s} all lights {spp:4d} spp: MSE {mse(a):.3e}    one light {one_spp:4d} spp (x{t_all / t_one:5.2f} samples in the same time): MSE {mse(b):.3e}"
                   f"    ratio {mse(b) / max(mse(a), 1e-30):.3f}")
        r.close()
        s.close()
    return out, ref_spp


def child(w, h, spp):
    """--child: the one-light renders only, as one JSON line (run under another TRT_HIP_LIB by --ab)."""
    import tinyraytracing_amd as T
    res = {}
    for name, kw in SCENES:
        s = T.Scene.named(name, w, h, **kw)
        r = T.Renderer(s, 0)
        p = T.make_params(w, h, spp, SEED, flags=T.TRT_FLAG_FIXED_NEE | T.TRT_FLAG_ONE_LIGHT)
        res[label(name, kw)] = [st.render_ms for st in timed(r, p, 3)]
        K = T.KERNEL_NAMES.index("shade")
        res[label(name, kw)].append(r.render(T.make_params(w, h, spp, SEED, flags=p.flags | T.TRT_FLAG_TIMING))[1].kernel_ms[K])
        r.close()
        s.close()
    print("AB " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "one_light_cost.txt"))
    ap.add_argument("--quick", action="store_true", help="960 x 540 x 16 spp and a 256-spp reference: a rehearsal")
    ap.add_argument("--ab", default=None, help="another build of libtrt_hip.so to time the one-light renders on")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    w, h, spp = (960, 540, 16) if a.quick else (1920, 1080, 64)
    if a.child:
        return child(w, h, spp)
    import tinyraytracing_amd as T
    rows, kernels, times = per_render(T, w, h, spp, a.quick)
    eq, ref_spp = equal_time(T, times, spp, a.quick)
    text = [f"TRT_FLAG_ONE_LIGHT on one MI355X: {w} x {h} x {spp} spp, seed {SEED:#x}, default budget (tools/one_light_cost.py).",
            "All lights = TRT_FLAG_FIXED_NEE alone; one light = TRT_FLAG_FIXED_NEE | TRT_FLAG_ONE_LIGHT.", "",
            "(1) Per render: two timed renders after a warm-up.", ""] + rows + [
            "", "(2) kernel_ms of a TRT_FLAG_TIMING render (trace_closest, shade, trace_shadow, resolve, tail) and the shadow share of their sum.", ""] + kernels + [
            "", f"(3) At equal device time: tonemapped MSE at 320 x 180 against an all-lights render at {ref_spp} spp with another seed.", ""] + eq
    if a.ab:
        text += ["", f"(4) k_shade SHADE_PICK block size: the default build against {os.path.relpath(a.ab, ROOT)}; one-light renders, three timed renders each, then k_shade's kernel_ms.", ""]
        for what, lib in (("default", None), ("other", a.ab)):
            env = dict(os.environ)
            if lib:
                env["TRT_HIP_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--quick"] if a.quick else [])
            run = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
            line = next((x for x in run.stdout.splitlines() if x.startswith("AB ")), None)
            if run.returncode != 0 or line is None:
                text.append(f"{what}: the child failed ({run.returncode}): {run.stderr[-400:]}")
                continue
            for lab, v in json.loads(line[3:]).items():
                text.append(f"{what:8s} {lab:12s}  " + " / ".join(f"{x:8.2f}" for x in v[:3]) + f" ms   k_shade {v[3]:8.2f} ms")
    body = "\n".join(text) + "\n"
    print(body)
    with open(a.out, "w") as f:
        f.write(body)


if __name__ == "__main__":
    main()
