"""Scenes of more than 8 lights on the HIP path (k_shade's SHADE_MANY flavour, counter rows sized by the light count) — MI355X only.

Bar: bit-exact against the CPU oracle, as in test_gpu_parity.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu
TOL = 0.0


def assert_same_image(a, b, what=""):
    assert a.shape == b.shape, what
    assert np.isfinite(a).all(), what
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert d.max() <= TOL, f"{what}: max abs diff {d.max()} in {int((d.max(-1) > TOL).sum())} pixels"


def assert_same_counts(st, ost, what=""):
    got = (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits, st.max_bounces)
    want = (ost.rays_camera, ost.rays_shadow, ost.rays_indirect, ost.shaded_hits, ost.max_bounces)
    assert got == want, f"{what}: {got} != {want}"


def bytes_per_path(n_lights):
    return 132 + 48 * n_lights  # trt.h trt_light: the render loop's bytes_per_path (queues, hit, Lacc, redo list, shadow queues)


def render_fresh(scene, p, env, monkeypatch):
    """A Renderer created under `env` (read at trt_create), one render, closed again."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = T.Renderer(scene, 0)
    try:
        return r.render(p)
    finally:
        r.close()
        for k in env:
            monkeypatch.delenv(k)


# 1. every estimator mode, 9 / 17 / 65 lights; TRT_TAIL_N=0 keeps every bounce in the queue kernels (k_shade, not k_tail)
MODES = {"parity": 0, "fixed_nee": T.TRT_FLAG_FIXED_NEE, "ray_offset": T.TRT_FLAG_RAY_OFFSET,
         "fixed": T.TRT_FLAG_FIXED_PIXELS | T.TRT_FLAG_FIXED_NEE}


@pytest.mark.parametrize("k", [8, 16, 64])
@pytest.mark.parametrize("mode", list(MODES))
def test_many_lights_match_oracle_in_every_mode(k, mode, monkeypatch):
    s = get_scene("lamps", 64, 36, n=k)
    assert s.info["n_lights"] == k + 1 > 8
    p = T.make_params(64, 36, 4, 0x1A3B5, flags=MODES[mode])
    img, st = render_fresh(s, p, {"TRT_TAIL_N": "0"}, monkeypatch)
    ref, ost = O.render(s.flat, p)
    assert_same_image(img, ref, f"lamps {k + 1} lights, {mode}")
    assert_same_counts(st, ost, f"lamps {k + 1} lights, {mode}")
    assert st.launches[T.KERNEL_NAMES.index("tail")] == 0
    assert st.rays_shadow > 0 and img.max() > 0.0


# 2. every traversal kind
@pytest.mark.parametrize("env", [{"TRT_NODE_KIND": "0"}, {"TRT_NODE_KIND": "1"}, {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}],
                         ids=["nodes4", "oct", "impl3_small_scene"])
def test_many_lights_on_every_traversal_kind(env, monkeypatch):
    # 8 lamps: 55 triangles, a tree the wave-uniform walk would take (TRT_TRACE_IMPL=3 forces the persistent driver on it);
    # 24 lamps: a tree that the persistent driver walks anyway
    for k in (8, 24):
        s = get_scene("lamps", 64, 36, n=k)
        p = T.make_params(64, 36, 4, 77, flags=T.TRT_FLAG_COUNT)
        img, st = render_fresh(s, p, dict(env, TRT_TAIL_N="0"), monkeypatch)
        ref, ost = O.render(s.flat, p)
        assert_same_image(img, ref, f"{env} {k + 1} lights")
        assert_same_counts(st, ost, f"{env} {k + 1} lights")
        if k == 24:
            assert st.inner_node_bytes == (80 if env["TRT_NODE_KIND"] == "1" else 128)


# 3. the tail both ways
def test_many_lights_tail_either_way(monkeypatch):
    s = get_scene("lamps", 64, 36, n=32)
    p = T.make_params(64, 36, 8, 0x7A11)
    ref, ost = O.render(s.flat, p)
    tail = T.KERNEL_NAMES.index("tail")
    img_t, st_t = render_fresh(s, p, {"TRT_TAIL_N": str(1 << 30)}, monkeypatch)  # k_tail takes every bounce after the first
    img_q, st_q = render_fresh(s, p, {"TRT_TAIL_N": "0"}, monkeypatch)        # the queue kernels take them all
    assert st_t.launches[tail] >= 1 and st_q.launches[tail] == 0
    assert st_q.launches[T.KERNEL_NAMES.index("shade")] > st_t.launches[T.KERNEL_NAMES.index("shade")]
    for img, st, what in ((img_t, st_t, "k_tail"), (img_q, st_q, "queue kernels")):
        assert_same_image(img, ref, what)
        assert_same_counts(st, ost, what)


# 4. 301 lights: 604 counters to publish (a 64-thread block publishes 32 per pass of its loop), light tables beyond the LDS staging
def test_301_lights_small_image(monkeypatch):
    s = get_scene("lamps", 32, 18, n=300)
    f = s.flat.contents
    assert f.n_lights == 301 and 2 * (1 + f.n_lights) > 32
    assert f.n_light_tris * 80 > 24 * 1024  # the light-triangle table alone (80-B records) exceeds k_shade's 24-KB LDS staging (TRT_SHADE_LDS_TABLE_BYTES)
    for flags in (0, T.TRT_FLAG_FIXED_NEE):
        p = T.make_params(32, 18, 2, 0x301, flags=flags)
        img, st = render_fresh(s, p, {"TRT_TAIL_N": "0"}, monkeypatch)
        ref, ost = O.render(s.flat, p)
        assert_same_image(img, ref, f"301 lights, flags {flags}")
        assert_same_counts(st, ost, f"301 lights, flags {flags}")


# 5. passes and slots
def test_many_lights_passes_overlap_and_sample_ranges(renderer_factory):
    s = get_scene("lamps", 48, 27, n=40)
    nl = s.info["n_lights"]
    r = renderer_factory(s)
    p = T.make_params(48, 27, 6, 0xB0D6E7)
    one, st1 = r.render(p)
    ref, ost = O.render(s.flat, p)
    assert_same_image(one, ref, "one pass")
    assert_same_counts(st1, ost, "one pass")
    assert st1.passes == 1
    budget = bytes_per_path(nl) * 48 * 27 * 2  # two samples of every pixel per pass
    multi, stm = r.render(T.make_params(48, 27, 6, 0xB0D6E7, mem_budget=budget))
    assert stm.passes >= 3
    assert_same_image(multi, one, "passes")
    assert_same_counts(stm, ost, "passes")
    over, sto = r.render(T.make_params(48, 27, 6, 0xB0D6E7, flags=T.TRT_FLAG_OVERLAP, mem_budget=budget))
    assert sto.passes >= 3
    assert_same_image(over, one, "overlapped passes")
    assert_same_counts(sto, ost, "overlapped passes")
    acc, rays = None, 0
    for a, b in ((0, 1), (1, 4), (4, 6)):
        img, acc, st = r.render_samples(p, a, b, acc)
        rays += st.rays
    assert_same_image(img, one, "sample ranges")
    assert rays == ost.rays


# 6. a device group (device 0 twice) equals the single-device render
def test_many_lights_device_group_equals_single_render(renderer_factory):
    s = get_scene("lamps", 64, 40, n=20)
    p = T.make_params(64, 40, 4, 0x6E0)
    ref, st = renderer_factory(s).render(p)
    g = T.GroupRenderer(s, [0, 0])
    try:
        pg = T.make_params(64, 40, 4, 0x6E0)
        pg.row_block = 4
        img, gst, _ = g.render(pg)
    finally:
        g.close()
    assert_same_image(img, ref, "group of two")
    assert (gst.rays_camera, gst.rays_shadow, gst.rays_indirect, gst.shaded_hits) == (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits)


# 7. a scene of more than 8 lights written as XML / OBJ / MTL: the library and the tinyrt CLI
def _write_lamp_grid(tmp_path, n_lamps=11):
    obj = ["vt 0 0", "vn 0 1 0", "vn 0 -1 0", "v -4 0 -4", "v 4 0 -4", "v 4 0 4", "v -4 0 4",
           "v -1 0.01 -1", "v 1 0.01 -1", "v 1 1 -1", "v -1 1 -1"]  # floor, and a wall that shadows some lamps
    faces = ["usemtl white", "f 1/1/1 3/1/1 2/1/1", "f 1/1/1 4/1/1 3/1/1", "usemtl shiny", "f 5/1/1 6/1/1 7/1/1", "f 5/1/1 7/1/1 8/1/1"]
    mtl = SU.MTL_BASIC
    lights = []
    vb = 9
    for i in range(n_lamps):
        x, z, h, e = -3.0 + 0.6 * i, -2.0 + 0.37 * (i % 5), 2.0 + 0.15 * (i % 3), 0.2 + 0.05 * (i % 4)
        obj += [f"v {x - e} {h} {z - e}", f"v {x + e} {h} {z - e}", f"v {x + e} {h} {z + e}", f"v {x - e} {h} {z + e}"]
        faces += [f"usemtl lamp{i}", f"f {vb}/1/2 {vb + 1}/1/2 {vb + 2}/1/2", f"f {vb}/1/2 {vb + 2}/1/2 {vb + 3}/1/2"]
        vb += 4
        mtl += f"newmtl lamp{i}\nKd 0 0 0\nKs 0 0 0\nNs 1\nNi 1\n"
        lights.append((f"lamp{i}", (3.0 + i, 10.0 - 0.5 * i, 2.0 + 0.25 * i)))
    SU.write_scene(tmp_path, "grid", "\n".join(obj + faces) + "\n", mtl, lights=lights, w=64, h=48, fovy=50, eye=(0, 3, 7), lookat=(0, 0.5, 0))
    return lights


def test_written_many_light_scene_library_and_cli(tmp_path):
    lights = _write_lamp_grid(tmp_path)
    s = SU.load(tmp_path, "grid")
    assert s.info["n_lights"] == len(lights) > 8
    r = T.Renderer(s, 0)
    p = T.make_params(64, 48, 8, 77)
    try:
        img, st = r.render(p)
    finally:
        r.close()
    ref, ost = O.render(s.flat, p)
    assert_same_image(img, ref, "written scene")
    assert_same_counts(st, ost, "written scene")
    exe = os.path.join(os.path.dirname(T.__file__), "lib", "tinyrt")
    d = str(tmp_path)
    out = str(tmp_path / "grid.png")
    run = subprocess.run([exe, d, os.path.join(d, "grid.mtl"), os.path.join(d, "grid.xml"), os.path.join(d, "grid.obj"), "8", "--leaf", "2",
                          "--seed", "77", "--out", out], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode()
    T.imshow(img, str(tmp_path / "lib.png"))
    assert open(out, "rb").read() == open(str(tmp_path / "lib.png"), "rb").read()


# 8. a budget below one sample of every pixel: TRT_ENOMEM, and the handle still renders
def test_many_lights_budget_too_small_then_render(renderer_factory):
    s = get_scene("lamps", 64, 36, n=16)
    nl = s.info["n_lights"]
    r = renderer_factory(s)
    lib = T._abi.load_hip()
    out = np.zeros((36, 64, 3), np.float32)
    tiny = T.make_params(64, 36, 4, 9, mem_budget=bytes_per_path(nl) * 64 * 36 - 1)
    assert lib.trt_render(r._h, C.byref(tiny), out.ctypes.data_as(C.POINTER(C.c_float)), None) == 3  # TRT_ENOMEM
    assert "render smaller tiles" in lib.trt_last_error().decode()
    with pytest.raises(T.TrtError, match="mem_budget too small"):
        r.render(tiny)
    p = T.make_params(64, 36, 4, 9, mem_budget=bytes_per_path(nl) * 64 * 36)  # exactly one sample per pass
    img, st = r.render(p)
    ref, ost = O.render(s.flat, p)
    assert st.passes == 4
    assert_same_image(img, ref, "after TRT_ENOMEM")
    assert_same_counts(st, ost, "after TRT_ENOMEM")
