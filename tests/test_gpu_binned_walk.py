"""The binned walk of the closest-hit queue kernel (trt_kernels.h traceQueueBinned: each wave's rays sorted by the leaves they reach before
any triangle is tested) against the kernel TRT_BIN_WALK=0 keeps — MI355X only.

Binning changes only which lane holds a ray, so every render, counter and ray batch must come out bit-identical with the switch on and
off, and equal to the CPU oracle.  Which kernels ran is read from the TRT_DEBUG line of trt_create and asserted first.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def renderer(s, binned, capfd, monkeypatch, env=None):
    env = dict(env or {}, TRT_DEBUG="1", TRT_BIN_WALK="1" if binned else "0")
    capfd.readouterr()
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        r = T.Renderer(s, 0)
    got = re.findall(r"trt_create: slim walk (\d), 8-byte hit records (\d), binned walk (\d)", capfd.readouterr().err)
    assert got == [("1", "1", "1" if binned else "0")], got
    return r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


STAT_FIELDS = ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "max_bounces", "redo_rays")


def stats_of(st, count):
    out = [getattr(st, f) for f in STAT_FIELDS]
    if count:
        out += list(st.inner_visits) + list(st.tri_tests)
    return out


def leaves(s):
    f = s.flat.contents
    return sum(1 for k in range(f.n_nodes) for c in (f.nodes[k].child0, f.nodes[k].child1) if c & 0x80000000)


CASES = [  # (scene, n added lamps, w, h, spp, flags)
    ("back", None, 128, 128, 16, 0),
    ("back", None, 256, 144, 8, T.TRT_FLAG_COUNT),
    ("back", None, 96, 64, 16, T.TRT_FLAG_FIXED_NEE),
    ("lamps", 2, 64, 36, 8, T.TRT_FLAG_COUNT),       # 3 lights, more than 5 leaves
    ("lamps", 9, 64, 36, 8, T.TRT_FLAG_FIXED_NEE),   # 10 lights, more than 8 leaves: a key bit stands for a run of leaves
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}{c[1] or ''}-{c[2]}x{c[3]}x{c[4]}-f{c[5]}" for c in CASES])
def test_render_binned_equals_unbinned_and_oracle(case, capfd, monkeypatch):
    name, lamps, w, h, spp, flags = case
    s = get_scene(name, w, h, n=lamps) if lamps else get_scene(name, w, h)
    if lamps:
        assert leaves(s) > (8 if lamps > 2 else 5)
    p = T.make_params(w, h, spp, 0xB1 + spp, flags=flags)
    out = []
    for binned in (True, False):
        r = renderer(s, binned, capfd, monkeypatch)
        try:
            out.append(r.render(p))
        finally:
            r.close()
    (img_b, st_b), (img_u, st_u) = out
    assert np.array_equal(bits(img_b), bits(img_u)), "binned and unbinned walks differ"
    count = bool(flags & T.TRT_FLAG_COUNT)
    assert stats_of(st_b, count) == stats_of(st_u, count)
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(bits(img_b), bits(ref)), f"max abs diff to the oracle {float(np.abs(img_b - ref).max())}"
    assert (st_b.rays_camera, st_b.rays_shadow, st_b.rays_indirect, st_b.shaded_hits, st_b.max_bounces) == \
        (ost.rays_camera, ost.rays_shadow, ost.rays_indirect, ost.shaded_hits, ost.max_bounces)


@pytest.mark.parametrize("per_axis", [64, 300_000])
def test_ray_batch_with_zero_direction_components(per_axis, capfd, monkeypatch):
    """Axis-aligned rays are parked and walked again with the literal slab test (ray batches run the closest-hit queue kernel); with
    300 000 per axis a wave meets more than its list holds and goes over its share of the queue once more."""
    s = get_scene("back", 64, 36)
    org, dirs = SU.axis_rays(s, per_axis)
    t0, tri0, uv0 = O.trace(s.flat, org, dirs)
    got = []
    for binned in (True, False):
        r = renderer(s, binned, capfd, monkeypatch)
        try:
            got.append(r.trace_closest(org, dirs, want_stats=True))
        finally:
            r.close()
    (t1, tri1, uv1, st1), (t2, tri2, uv2, st2) = got
    assert st1.redo_rays == st2.redo_rays == 6 * per_axis
    assert list(st1.inner_visits) == list(st2.inner_visits) and list(st1.tri_tests) == list(st2.tri_tests)
    for t, tri, uv in ((t1, tri1, uv1), (t2, tri2, uv2)):
        assert np.array_equal(tri, tri0) and np.array_equal(bits(t), bits(t0)) and np.array_equal(bits(uv), bits(uv0))


def test_headline_step_outputs_equal(tmp_path):
    """One full-size headline step (bench.py's default workload) with the switch on and off: equal --dump-outputs arrays."""
    dirs = {}
    for v in ("1", "0"):
        d = tmp_path / f"bin{v}"
        env = dict(os.environ, TRT_BIN_WALK=v)
        subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-outputs", str(d)],
                       cwd=ROOT, env=env, check=True, timeout=600, stdout=subprocess.DEVNULL)
        dirs[v] = d
    names = sorted(x.name for x in dirs["1"].iterdir())
    assert names and names == sorted(x.name for x in dirs["0"].iterdir())
    for name in names:
        a, b = np.load(dirs["1"] / name), np.load(dirs["0"] / name)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), name
