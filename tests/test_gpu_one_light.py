"""TRT_FLAG_ONE_LIGHT on the MI355X: bit parity with the CPU build (tests/onelight: hostsim's loop with the light loop replaced by lightPick ->
lightSample -> occlusion test) on every entry that traces full paths and on every route the host loop can take; the shape of the work (at most
one shadow ray per shaded vertex, one shadow launch per bounce, one-light path memory); the cases where the flag does nothing; the estimator
against all-lights under the statistical criterion of tests/test_one_light_cpu.py; the selection table after trt_update_geometry."""
import ctypes as C

import numpy as np
import pytest

import onelight_lib as OL
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu
W, H, SPP, SEED = 32, 18, 4, 0x01E1
FLAG_SETS = {"one_light": OL.FLAGS, "offset_pixels": OL.FLAGS | T.TRT_FLAG_RAY_OFFSET | T.TRT_FLAG_FIXED_PIXELS}
SCENES = {"lamps1": ("lamps", {"n": 1}), "lamps7": ("lamps", {"n": 7}), "lamps8": ("lamps", {"n": 8}), "lamps64": ("lamps", {"n": 64}),
          "staircase": ("staircase", {}), "veach-mis": ("veach-mis", {})}
K = {n: i for i, n in enumerate(T.KERNEL_NAMES)}
_refs = {}
_handles = {}


def scene(key):
    name, kw = SCENES[key]
    return get_scene(name, W, H, **kw)


def params(flags, **kw):
    return T.make_params(W, H, SPP, SEED, flags=flags, **kw)


def cpu(key, flags, tile=None, rows=None):
    """The CPU build's render, computed once per case and shared."""
    k = (key, flags, tile, rows)
    if k not in _refs:
        _refs[k] = OL.render(scene(key).flat, T.make_params(W, H, SPP, SEED, tile=tile, rows=rows, flags=flags))
    return _refs[k]


def handle(key, env, monkeypatch):
    """One Renderer per (scene, environment at trt_create)."""
    k = (key, tuple(sorted(env.items())))
    if k not in _handles:
        for n, v in env.items():
            monkeypatch.setenv(n, v)
        _handles[k] = T.Renderer(scene(key), 0)
        for n in env:
            monkeypatch.delenv(n)
    return _handles[k]


def same(img, st, ref, what):
    want, rays = ref
    assert img.shape == want.shape and img.tobytes() == want.tobytes(), f"{what}: image differs from the CPU build in {int((img != want).any(-1).sum())} pixels"
    assert [st.rays_camera, st.rays_shadow, st.rays_indirect] == rays, f"{what}: rays {[st.rays_camera, st.rays_shadow, st.rays_indirect]} != {rays}"


# ---- bit parity: every scene, both flag sets, every entry; queue kernels (TRT_TAIL_N=0: k_shade's SHADE_PICK at every bounce) and k_tail ----

@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("key", list(SCENES))
def test_every_entry_matches_the_cpu_build(key, flags, monkeypatch):
    fl = FLAG_SETS[flags]
    s = scene(key)
    assert s.info["n_lights"] >= 2
    ref = cpu(key, fl)
    for env in ({"TRT_TAIL_N": "0"}, {}):
        r = handle(key, env, monkeypatch)
        img, st = r.render(params(fl))
        same(img, st, ref, f"{key} {flags} trt_render {env}")
        assert (st.launches[K["tail"]] == 0) == bool(env)
        assert st.rays_shadow <= st.shaded_hits
    r = handle(key, {"TRT_TAIL_N": "0"}, monkeypatch)
    # a tile with interleaved rows
    tile, rows = (3, 2, 29, 17), (2, 2, 1)
    img, st = r.render(params(fl, tile=tile, rows=rows))
    same(img, st, cpu(key, fl, tile, rows), f"{key} {flags} tile")
    # trt_render_pixels: every pixel twice, shuffled
    rng = np.random.default_rng(5)
    pixels = rng.permutation(np.concatenate([np.arange(W * H), np.arange(W * H)])).astype(np.uint32)
    want = ref[0].reshape(-1, 3)[pixels]
    sums, _, st = r.render_pixels(params(fl), pixels, 0, SPP)
    assert sums.astype(np.float32).tobytes() == want.tobytes(), f"{key} {flags} trt_render_pixels"
    assert [st.rays_camera, st.rays_shadow, st.rays_indirect] == [2 * x for x in ref[1]]
    # trt_render_rays on trt_camera_rays of the same pixels, with the pixels as stream ids
    cam = s.flat.contents.camera
    org, d = T.camera_rays(cam, params(fl), pixels, 0, SPP)
    rsums, _, rst = r.render_rays(params(fl), org, d, streams=pixels)
    assert rsums.tobytes() == sums.tobytes(), f"{key} {flags} trt_render_rays"
    assert [rst.rays_camera, rst.rays_shadow, rst.rays_indirect] == [st.rays_camera, st.rays_shadow, st.rays_indirect]
    # trt_group_render on a group of one device
    g = T.GroupRenderer(s, [0])
    try:
        img, gst, _ = g.render(params(fl))
    finally:
        g.close()
    same(img, gst, ref, f"{key} {flags} trt_group_render")


ROUTES = {
    "persistent_driver_on_a_small_tree": ({"TRT_TRACE_IMPL": "3", "TRT_TAIL_N": "0"}, 0, False),
    "persistent_driver_oct": ({"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1", "TRT_TAIL_N": "0"}, 0, False),
    "tail_takes_everything": ({"TRT_TAIL_N": str(1 << 30)}, 0, False),
    "shadow_stream_off": ({"TRT_SHADOW_STREAM": "0", "TRT_TAIL_N": "0"}, 0, False),
    "shadow_stream_on": ({"TRT_SHADOW_STREAM": "1", "TRT_TAIL_N": "64"}, 0, False),
    "overlap": ({"TRT_TAIL_N": "0"}, T.TRT_FLAG_OVERLAP, True),
    "two_passes": ({"TRT_TAIL_N": "64"}, 0, True),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("key", ["lamps8", "lamps64", "staircase"])
def test_forced_routes_match_the_cpu_build(key, route, monkeypatch, capfd):
    env, extra, two_passes = ROUTES[route]
    r = handle(key, dict(env, TRT_DEBUG="1"), monkeypatch)
    budget = 180 * W * H * 2 if two_passes else 0  # two samples of every pixel per pass
    capfd.readouterr()
    img, st = r.render(params(OL.FLAGS | extra, mem_budget=budget))
    err = capfd.readouterr().err
    same(img, st, cpu(key, OL.FLAGS), f"{key} {route}")
    assert "k_shade pick" in err and "fused primary 0" in err, err
    if two_passes:  # (two samples of every pixel fit the budget; with TRT_FLAG_OVERLAP each of the two slots gets half of it)
        assert st.passes == (4 if extra & T.TRT_FLAG_OVERLAP else 2)
    if route == "shadow_stream_on" and key == "lamps8":  # (the side stream runs beside the wave-uniform walk of a tiny tree only)
        assert "shadow stream on" in err, err
    if route in ("shadow_stream_off", "overlap"):  # (two passes one after the other keep the side stream; two in flight do not)
        assert "shadow stream off" in err, err
    if route == "tail_takes_everything":
        assert st.launches[K["tail"]] >= 1 and st.launches[K["shade"]] == 1
    if "TRT_TRACE_IMPL" in env:
        assert st.inner_node_bytes in (80, 128)  # a per-lane driver, not the wave-uniform walk


# ---- the shape of the work -------------------------------------------------------------------------------------------------------------

def test_work_is_that_of_a_one_light_scene(monkeypatch):
    r = handle("lamps64", {"TRT_TAIL_N": "0"}, monkeypatch)
    paths = W * H * SPP
    img, st = r.render(params(OL.FLAGS, mem_budget=180 * paths))
    assert st.passes == 1
    assert 0 < st.rays_shadow <= st.shaded_hits
    assert 0 < st.launches[K["trace_shadow"]] <= st.launches[K["trace_closest"]]
    _, all_st = r.render(params(T.TRT_FLAG_FIXED_NEE))
    assert all_st.rays_shadow > 20 * st.rays_shadow and all_st.launches[K["trace_shadow"]] > 20 * st.launches[K["trace_shadow"]]
    lib = T._abi.load_hip()
    out = np.zeros((H, W, 3), np.float32)
    p = params(T.TRT_FLAG_FIXED_NEE, mem_budget=180 * paths)
    assert lib.trt_render(r._h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_float)), None) == 3  # TRT_ENOMEM
    assert "TRT_FLAG_ONE_LIGHT" in lib.trt_last_error().decode()


# ---- where the flag does nothing, and where it is refused ---------------------------------------------------------------------------------

def test_one_light_scene_renders_fixed_nee_bit_for_bit(monkeypatch):
    s = get_scene("back", W, H)
    for env in ({"TRT_TAIL_N": "0"}, {}):
        for n, v in env.items():
            monkeypatch.setenv(n, v)
        r = T.Renderer(s, 0)
        for n in env:
            monkeypatch.delenv(n)
        try:
            a, sa = r.render(params(OL.FLAGS))
            b, sb = r.render(params(T.TRT_FLAG_FIXED_NEE))
        finally:
            r.close()
        assert a.tobytes() == b.tobytes() and b.max() > 0
        assert (sa.rays_camera, sa.rays_shadow, sa.rays_indirect, sa.shaded_hits) == (sb.rays_camera, sb.rays_shadow, sb.rays_indirect, sb.shaded_hits)
    ref, rays = OL.render(s.flat, params(OL.FLAGS))
    assert a.tobytes() == ref.tobytes() and [sa.rays_camera, sa.rays_shadow, sa.rays_indirect] == rays


def test_scene_without_lights_renders(tmp_path):
    obj = "vt 0 0\nvn 0 0 1\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1/1/1 2/1/1 3/1/1\nf 1/1/1 3/1/1 4/1/1\n"
    SU.write_scene(tmp_path, "dark", obj, SU.MTL_BASIC, lights=(), w=W, h=H)
    s = SU.load(tmp_path, "dark")
    assert s.info["n_lights"] == 0
    r = T.Renderer(s, 0)
    try:
        img, st = r.render(params(OL.FLAGS))
    finally:
        r.close()
    assert not img.any() and st.rays_shadow == 0 and st.shaded_hits > 0


def test_flag_without_fixed_nee_is_einval_on_every_entry_and_the_handle_goes_on(monkeypatch):
    r = handle("lamps8", {"TRT_TAIL_N": "0"}, monkeypatch)
    bad = params(T.TRT_FLAG_ONE_LIGHT)
    pixels = np.arange(8, dtype=np.uint32)
    org, d = T.camera_rays(scene("lamps8").flat.contents.camera, params(OL.FLAGS), pixels, 0, 1)
    calls = [lambda: r.render(bad), lambda: r.render_samples(bad, 0, 1), lambda: r.render_pixels(bad, pixels, 0, 1),
             lambda: r.render_rays(bad, org, d, streams=pixels)]
    for call in calls:
        with pytest.raises(T.TrtError, match="TRT_FLAG_ONE_LIGHT needs TRT_FLAG_FIXED_NEE"):
            call()
    lib = T._abi.load_hip()
    out = np.zeros((H, W, 3), np.float32)
    assert lib.trt_render(r._h, C.byref(bad), out.ctypes.data_as(C.POINTER(C.c_float)), None) == 1  # TRT_EINVAL
    g = T.GroupRenderer(scene("lamps8"), [0])
    try:
        with pytest.raises(T.TrtError, match="TRT_FLAG_ONE_LIGHT needs TRT_FLAG_FIXED_NEE"):
            g.render(bad)
    finally:
        g.close()
    r.render_aov(bad)  # the feature entries ignore the estimator flags
    img, st = r.render(params(OL.FLAGS))
    same(img, st, cpu("lamps8", OL.FLAGS), "after TRT_EINVAL")


# ---- unbiased on the device ----------------------------------------------------------------------------------------------------------------

def _device_moments(r, flags, seed, n):
    """Mean luminance per pixel and an upper bound of the variance of that mean from trt_render_pixels' moments of n samples.  The moments hold no
    covariances between the channels, so the variance of the luminance is bounded by Cauchy-Schwarz: sd(sum a_c X_c) <= sum a_c sd(X_c).  (The
    bound never understates the variance: the criterion's |z| can only shrink under it, and tests/test_one_light_cpu.py's mutant still fails it.)"""
    p = T.make_params(24, 16, n, seed, flags=flags)
    sums, sumsq, _ = r.render_pixels(p, np.arange(24 * 16, dtype=np.uint32), 0, n)
    mean = sums @ OL.LUMA  # sums of L / n
    var_c = np.maximum(sumsq / n - (sums / n) ** 2, 0.0) * (n / (n - 1.0)) * n  # per channel: the variance of the mean radiance (v = L / n: var(L) / n = var(v) n), as mean_luminance_variance
    sd = np.sqrt(var_c) @ OL.LUMA
    return mean, sd * sd


def test_one_light_is_unbiased_against_all_lights_on_the_device(monkeypatch):
    """N = 8 samples per pixel, the N of tests/test_one_light_cpu.py, at 24 x 16 on lamps n = 8."""
    from test_one_light_cpu import N, SEED_A, SEED_B, SEED_C
    s = get_scene("lamps", 24, 16, n=8)
    monkeypatch.setenv("TRT_TAIL_N", "0")
    r = T.Renderer(s, 0)
    monkeypatch.delenv("TRT_TAIL_N")
    try:
        one = _device_moments(r, OL.FLAGS, SEED_C, N)
        ref_a = _device_moments(r, T.TRT_FLAG_FIXED_NEE, SEED_A, N)
        ref_b = _device_moments(r, T.TRT_FLAG_FIXED_NEE, SEED_B, N)
    finally:
        r.close()
    a, b = OL.criterion(*one, *ref_a), OL.criterion(*ref_a, *ref_b)
    print(f"device N={N}: one-light vs all-lights {a}, all-lights vs all-lights {b}")
    assert a[2] > 100
    assert OL.passes(a[0], a[1]), a
    assert OL.passes(b[0], b[1]), b
    # the same bound on the CPU build's samples rejects the estimator without the division by the probability
    q = T.make_params(24, 16, 1, SEED_C, flags=OL.FLAGS)
    ones = OL.render_seeds(s.flat, q, N, OL.MUTANT_NO_WEIGHT).astype(np.float64).reshape(N, -1, 3)
    sd = np.sqrt(ones.var(axis=0, ddof=1)) @ OL.LUMA
    c = OL.criterion((ones @ OL.LUMA).mean(axis=0), sd * sd / N, *ref_a)
    assert not OL.passes(c[0], c[1]), c


# ---- trt_update_geometry rebuilds the selection table -------------------------------------------------------------------------------------

def test_update_geometry_that_scales_a_lamp(monkeypatch):
    s = T.Scene.named("lamps", W, H, n=8)
    f = s.flat.contents
    a = s.arrays()
    lamp = a["tri_mat"] == f.lights[3].mat
    assert 0 < lamp.sum() < len(lamp)
    v = a["tri_v"].copy()
    c = v[lamp].reshape(-1, 3).mean(axis=0)
    v[lamp] = (c + (v[lamp] - c) * np.float32(2.5)).astype(np.float32)
    monkeypatch.setenv("TRT_TAIL_N", "0")
    r = T.Renderer(s, 0)
    try:
        before, _ = r.render(params(OL.FLAGS))
        area_before = f.lights[3].area
        s.set_vertices(v)
        assert s.flat.contents.lights[3].area > 6.0 * area_before
        r.update_geometry(s)
        after, st = r.render(params(OL.FLAGS))
        fresh = T.Renderer(s, 0)
        try:
            want, wst = fresh.render(params(OL.FLAGS))
        finally:
            fresh.close()
    finally:
        r.close()
    assert after.tobytes() == want.tobytes()
    assert (st.rays_shadow, st.rays_indirect) == (wst.rays_shadow, wst.rays_indirect)
    assert after.tobytes() != before.tobytes()
    ref, rays = OL.render(s.flat, params(OL.FLAGS))
    assert after.tobytes() == ref.tobytes() and [st.rays_camera, st.rays_shadow, st.rays_indirect] == rays


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------

def test_tinyrt_one_light_sets_both_flags(tmp_path):
    import os
    import subprocess
    s = T.Scene.named("veach-mis", leaf_num=2)
    w, h = s.info["width"], s.info["height"]
    r = T.Renderer(s, 0)
    try:
        img, _ = r.render(T.make_params(w, h, 2, 77, flags=OL.FLAGS))
        plain, _ = r.render(T.make_params(w, h, 2, 77, flags=T.TRT_FLAG_FIXED_NEE))
    finally:
        r.close()
    assert img.tobytes() != plain.tobytes()
    exe = os.path.join(os.path.dirname(T.__file__), "lib", "tinyrt")
    d = os.path.join(T.SCENES_DIR, "veach-mis")
    out = str(tmp_path / "cli.png")
    run = subprocess.run([exe, d, os.path.join(d, "veach-mis.mtl"), os.path.join(d, "veach-mis.xml"), os.path.join(d, "veach-mis.obj"), "2", "--leaf", "2",
                          "--seed", "77", "--one-light", "--out", out], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode()
    T.imshow(img, str(tmp_path / "lib.png"))
    assert open(out, "rb").read() == open(str(tmp_path / "lib.png"), "rb").read()
