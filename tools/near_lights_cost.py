#!/usr/bin/env python3
"""What TRT_FLAG_NEAR_LIGHTS costs and buys on one MI355X -> profiles/near_lights_cost.txt (a GPU run; nothing here is asserted).

  (1) per render: `lamps` n = 8, 16, 64 and `staircase` at 1920 x 1080 x 64 spp with TRT_FLAG_FIXED_NEE alone (every light at every vertex), with
      TRT_FLAG_ONE_LIGHT and with TRT_FLAG_NEAR_LIGHTS: ms per render (two timed renders after a warm-up), Mrays/s, launches, passes, shadow rays;
  (2) per kernel: kernel_ms of one TRT_FLAG_TIMING render each;
  (3) at equal device time: for ONE_LIGHT and for NEAR the spp whose render time is closest to the all-lights 64-spp time, and the images' tonemapped
      MSE at 320 x 180 against an all-lights render at 4096 spp with another seed (section (3) of profiles/one_light_cost.txt with a NEAR column);
  (4) with --remarks LOG [--parent-remarks LOG]: VGPRs, scratch, spills and LDS of every k_shade<.., SHADE_NEAR, ..> instantiation and of k_tail, from the
      compiler's -Rpass-analysis=kernel-resource-usage output of a build of this tree (and of the parent's, for the kernels whose figures changed);
      with --isa-diff FILE: the summary of tools/isa_diff.py's comparison of the two builds, copied in;
  (5) with --parent-lib LIB: python bench.py --gpus 1 --steps 5 --warmup 2 on the parent's build of the HIP library and on this one, alternating;
  (6) with --parent-lib LIB: the same alternation for a ONE_LIGHT render of `lamps` n = 64 (ONE_LIGHT itself must not pay for NEAR).

The tool itself never opens the GPU: every GPU step is a child process of its own under its own time limit, one after the other, and after a child that
fails or runs out of time no further child is started (what was measured until then is written out).

    python tools/near_lights_cost.py [--out profiles/near_lights_cost.txt] [--quick] [--parent-lib LIB] [--remarks LOG --parent-remarks LOG] [--isa-diff FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = [("lamps", {"n": 8}), ("lamps", {"n": 16}), ("lamps", {"n": 64}), ("staircase", {})]
SEED, SEED_REF = 0x5EED0002, 0x5EED0A11  # those of tools/one_light_cost.py
ONE_LIGHT_RATIOS = {"lamps n=8": 1.510, "lamps n=16": 1.221, "lamps n=64": 0.968, "staircase": 1.111}  # profiles/one_light_cost.txt (3)


def label(name, kw):
    return f"{name} n={kw['n']}" if kw else name


def modes(T):
    fixed = T.TRT_FLAG_FIXED_NEE
    return (("all lights", fixed), ("one light", fixed | T.TRT_FLAG_ONE_LIGHT), ("near", fixed | T.TRT_FLAG_ONE_LIGHT | T.TRT_FLAG_NEAR_LIGHTS))


def timed(r, p, repeats=2):
    r.render(p)  # warm-up
    return [r.render(p)[1] for _ in range(repeats)]


# ---- the children: one GPU step each, one JSON line on stdout ---------------------------------------------------------------------------------

def step_render(w, h, spp, which):
    """(1) and (2) for scene SCENES[which]."""
    import tinyraytracing_amd as T
    K = {n: i for i, n in enumerate(T.KERNEL_NAMES)}
    name, kw = SCENES[which]
    s = T.Scene.named(name, w, h, **kw)
    r = T.Renderer(s, 0)
    rows, kernels, times = [], [], {}
    for what, flags in modes(T):
        p = T.make_params(w, h, spp, SEED, flags=flags)
        sts = timed(r, p)
        ms = [st.render_ms for st in sts]
        st = sts[-1]
        rows.append(f"{label(name, kw):12s} {s.info['n_lights']:3d} lights  {what:10s}  {ms[0]:8.2f} / {ms[1]:8.2f} ms   {st.rays / ms[1] / 1e3:9.0f} Mrays/s   "
                    f"passes {st.passes}   shadow rays {st.rays_shadow:13d}   launches closest {st.launches[K['trace_closest']]}, shade {st.launches[K['shade']]}, "
                    f"shadow {st.launches[K['trace_shadow']]}, resolve {st.launches[K['resolve']]}, tail {st.launches[K['tail']]}")
        times[what] = min(ms)
        tst = r.render(T.make_params(w, h, spp, SEED, flags=flags | T.TRT_FLAG_TIMING))[1]
        km = [tst.kernel_ms[K[k]] for k in ("trace_closest", "shade", "trace_shadow", "resolve", "tail")]
        kernels.append(f"{label(name, kw):12s} {what:10s}  " + ", ".join(f"{x:8.2f}" for x in km) + f"   shadow {100 * km[2] / max(sum(km), 1e-9):5.1f} %")
    r.close()
    s.close()
    print("STEP " + json.dumps({"rows": rows, "kernels": kernels, "times": times}))


def step_equal(spp, which, t_all, t_one, t_near, ref_spp):
    """(3) for scene SCENES[which]: time per sample scales with the pixel count, so the spp chosen at full size is used at 320 x 180."""
    import numpy as np
    import tinyraytracing_amd as T
    w, h = 320, 180
    name, kw = SCENES[which]
    s = T.Scene.named(name, w, h, **kw)
    r = T.Renderer(s, 0)
    (_, f_all), (_, f_one), (_, f_near) = modes(T)
    ref = r.render(T.make_params(w, h, ref_spp, SEED_REF, flags=f_all))[0]
    tm = lambda x: T.tonemap(x).astype(np.float64) / 255.0  # noqa: E731
    mse = lambda x: float(((tm(x) - tm(ref)) ** 2).mean())  # noqa: E731
    one_spp, near_spp = max(1, int(round(spp * t_all / t_one))), max(1, int(round(spp * t_all / t_near)))
    a = mse(r.render(T.make_params(w, h, spp, SEED, flags=f_all))[0])
    b = mse(r.render(T.make_params(w, h, one_spp, SEED, flags=f_one))[0])
    c = mse(r.render(T.make_params(w, h, near_spp, SEED, flags=f_near))[0])
    c_same = mse(r.render(T.make_params(w, h, one_spp, SEED, flags=f_near))[0])  # NEAR at ONE_LIGHT's sample count: the selection alone
    r.close()
    s.close()
    lab = label(name, kw)
    print("STEP " + json.dumps({"line": f"{lab:12s} all lights {spp:4d} spp: MSE {a:.3e}    one light {one_spp:4d} spp: MSE {b:.3e} ratio {b / max(a, 1e-30):.3f}"
                                        f" (one-light profile: {ONE_LIGHT_RATIOS[lab]:.3f})    near {near_spp:4d} spp: MSE {c:.3e} ratio {c / max(a, 1e-30):.3f}"
                                        f"    near at {one_spp} spp: MSE {c_same:.3e}", "one": b / max(a, 1e-30), "near": c / max(a, 1e-30)}))


def step_one_light(w, h, spp):
    """(6): three timed ONE_LIGHT renders of lamps n = 64 and k_shade's kernel_ms, on whatever TRT_HIP_LIB names."""
    import tinyraytracing_amd as T
    s = T.Scene.named("lamps", w, h, n=64)
    r = T.Renderer(s, 0)
    p = T.make_params(w, h, spp, SEED, flags=T.TRT_FLAG_FIXED_NEE | T.TRT_FLAG_ONE_LIGHT)
    ms = [st.render_ms for st in timed(r, p, 3)]
    shade = r.render(T.make_params(w, h, spp, SEED, flags=p.flags | T.TRT_FLAG_TIMING))[1].kernel_ms[T.KERNEL_NAMES.index("shade")]
    r.close()
    s.close()
    print("STEP " + json.dumps({"ms": ms, "shade": shade}))


# ---- the parent: spawns the children, writes the profile ----------------------------------------------------------------------------------------

class Stopped(Exception):
    pass


def child(args, limit, env=None, prefix="STEP "):
    """One GPU step under its own time limit -> the JSON of its result line.  Raises Stopped when it fails: nothing more is started then."""
    try:
        run = subprocess.run([sys.executable] + args, capture_output=True, text=True, env=env, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise Stopped(f"{' '.join(args[1:])}: no result within {limit} s")
    line = next((x for x in run.stdout.splitlines() if x.startswith(prefix)), None)
    if run.returncode != 0 or line is None:
        raise Stopped(f"{' '.join(args[1:])}: exit status {run.returncode}: {run.stderr[-400:]}")
    return json.loads(line if prefix == "{" else line[len(prefix):])  # ("{": bench.py's result line is the JSON itself)


def resources(path):
    """-Rpass-analysis=kernel-resource-usage output -> {mangled kernel name: {VGPRs, ScratchSize, VGPRs Spill, SGPRs Spill, LDS Size, Occupancy}}."""
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize|LDS Size|Occupancy)( \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(3))
    return out


def short(mangled):
    return re.sub(r"^_ZN4trtd\d+", "", mangled)[:mangled.index("EEEv") - 8]


def section_resources(remarks, parent_remarks):
    text = []
    this = resources(remarks)
    parent = resources(parent_remarks) if parent_remarks else {}
    fmt = lambda v: f"VGPRs {v['VGPRs']:3d}  scratch {v['ScratchSize']} B  VGPRs spilled {v['VGPRs Spill']}  SGPRs spilled {v['SGPRs Spill']:2d}  LDS {v['LDS Size']:5d} B  waves per SIMD {v['Occupancy']}"  # noqa: E731
    near = {n: v for n, v in this.items() if re.match(r"_ZN4trtd7k_shadeILj\d+ELi4E", n)}
    text.append(f"k_shade<TABS, SHADE_NEAR, LIST, BLOCK, WAVES, HIT8, FUSE>: {len(near)} instantiations (mangled: TABS, 4, LIST, block, waves asked, HIT8, FUSE)")
    for n in sorted(near):
        text.append(f"  {short(n):42s} {fmt(near[n])}")
    text.append("k_tail<COUNT, LIST> (a run-time branch on TileDesc::near_lights in its light loop):")
    for n in sorted(x for x in this if "k_tailI" in x):
        text.append(f"  {short(n):42s} {fmt(this[n])}" + (f"    parent: {fmt(parent[n])}" if n in parent and parent[n] != this[n] else ""))
    if parent:
        changed = sorted(n for n in this if n in parent and parent[n] != this[n] and "k_tailI" not in n)
        text.append(f"Of the {len(parent)} kernels the parent's build has, {len(parent) - len(changed) - sum('k_tailI' in n for n in parent)} keep every figure above; k_tail x 4 (above) and these differ:")
        for n in changed:
            text.append(f"  {short(n):42s} {fmt(this[n])}")
            text.append(f"  {'parent':42s} {fmt(parent[n])}")
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_lights_cost.txt"))
    ap.add_argument("--quick", action="store_true", help="960 x 540 x 16 spp and a 256-spp reference: a rehearsal")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's build of libtrt_hip.so, for (5) and (6)")
    ap.add_argument("--remarks", default=None)
    ap.add_argument("--parent-remarks", default=None)
    ap.add_argument("--isa-diff", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step: render:K, equal:K:t_all:t_one:t_near:ref_spp, one_light")
    a = ap.parse_args()
    w, h, spp = (960, 540, 16) if a.quick else (1920, 1080, 64)
    if a.step:
        kind, *rest = a.step.split(":")
        if kind == "render":
            return step_render(w, h, spp, int(rest[0]))
        if kind == "equal":
            return step_equal(spp, int(rest[0]), float(rest[1]), float(rest[2]), float(rest[3]), int(rest[4]))
        return step_one_light(w, h, spp)
    me = [os.path.abspath(__file__)] + (["--quick"] if a.quick else [])
    ref_spp = 256 if a.quick else 4096
    rows, kernels, eq, bench, one64, verdict = [], [], [], [], [], []
    stopped = None
    try:
        times = []
        for k in range(len(SCENES)):
            res = child(me + ["--step", f"render:{k}"], 600)
            rows += res["rows"]
            kernels += res["kernels"]
            times.append(res["times"])
        for k in range(len(SCENES)):
            t = times[k]
            res = child(me + ["--step", f"equal:{k}:{t['all lights']}:{t['one light']}:{t['near']}:{ref_spp}"], 900)
            eq.append(res["line"])
            verdict.append((label(*SCENES[k]), res["one"], res["near"]))
        if a.parent_lib:
            libs = (("parent", os.path.abspath(a.parent_lib)), ("this", None))
            for _ in range(3):
                for what, lib in libs:
                    env = dict(os.environ)
                    if lib:
                        env["TRT_HIP_LIB"] = lib
                    res = child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], 600, env=env, prefix="{")
                    bench.append((what, res))
            for _ in range(3):
                for what, lib in libs:
                    env = dict(os.environ)
                    if lib:
                        env["TRT_HIP_LIB"] = lib
                    res = child(me + ["--step", "one_light"], 600, env=env)
                    one64.append((what, res))
    except Stopped as e:
        stopped = str(e)
    text = [f"TRT_FLAG_NEAR_LIGHTS on one MI355X: {w} x {h} x {spp} spp, seed {SEED:#x}, default budget (tools/near_lights_cost.py).",
            "All lights = TRT_FLAG_FIXED_NEE alone; one light = | TRT_FLAG_ONE_LIGHT; near = | TRT_FLAG_ONE_LIGHT | TRT_FLAG_NEAR_LIGHTS.", "",
            "(1) Per render: two timed renders after a warm-up.", ""] + rows + [
            "", "(2) kernel_ms of a TRT_FLAG_TIMING render (trace_closest, shade, trace_shadow, resolve, tail) and the shadow share of their sum.", ""] + kernels + [
            "", f"(3) At equal device time: tonemapped MSE at 320 x 180 against an all-lights render at {ref_spp} spp with another seed; ratio = MSE / all-lights MSE.", ""] + eq
    for lab, one, near in verdict:
        text.append(f"{lab:12s} near {'is below' if near < one else 'is NOT below'} one light ({near:.3f} against {one:.3f})")
    text += ["", "(4) Resource usage (hipcc --offload-arch=gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage).", ""]
    text += section_resources(a.remarks, a.parent_remarks) if a.remarks else ["not collected in this run (--remarks)"]
    if a.isa_diff:
        text += ["", "tools/isa_diff.py, the parent's device code against this tree's:", ""] + open(a.isa_diff).read().rstrip("\n").splitlines()
    text += ["", "(5) No regression: python bench.py --gpus 1 --steps 5 --warmup 2, the parent commit's HIP library (TRT_HIP_LIB) and this tree's alternating.", ""]
    if bench:
        key = "value" if "value" in bench[0][1] else None
        for what, res in bench:
            text.append(f"{what:8s} " + (f"{res[key]:12.2f} {res.get('unit', '')}" if key else json.dumps(res)[:200]) + (f"    {res['ms_per_step']:.3f} ms per step" if "ms_per_step" in res else ""))
        if key:
            par, this = [r[key] for wh, r in bench if wh == "parent"], [r[key] for wh, r in bench if wh == "this"]
            if par and this:
                mp, mt = sum(par) / len(par), sum(this) / len(this)
                text.append(f"Means {mp:.1f} (parent) and {mt:.1f} (this): {100 * (mt / mp - 1):+.2f} %; the parent's own repeats span {min(par):.1f} ... {max(par):.1f}: "
                            f"the mean of this tree lies {'inside' if min(par) <= mt <= max(par) else ('ABOVE' if mt > max(par) else 'BELOW')} that spread ({key}).")
    else:
        text.append("not measured in this run (--parent-lib)")
    text += ["", "(6) ONE_LIGHT does not pay for NEAR: a ONE_LIGHT render of lamps n=64, three timed renders and k_shade's kernel_ms, the same alternation.", ""]
    for what, res in one64:
        text.append(f"{what:8s} " + " / ".join(f"{x:8.2f}" for x in res["ms"]) + f" ms   k_shade {res['shade']:8.2f} ms")
    if not one64:
        text.append("not measured in this run (--parent-lib)")
    if stopped:
        text += ["", f"STOPPED: {stopped}", "No further GPU step was started; the sections above hold what had been measured."]
    body = "\n".join(text) + "\n"
    print(body)
    with open(a.out, "w") as f:
        f.write(body)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
