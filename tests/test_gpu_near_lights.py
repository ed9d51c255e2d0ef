"""TRT_FLAG_NEAR_LIGHTS on the MI355X: bit parity with the CPU build (tests/nearlights: hostsim's loop with the light picked by lightPickNear on
buildLightTree's tree) on every entry that traces full paths and on every route the host loop can take, the flavour of k_shade asserted; the flag
rules; the shape of the work (TRT_FLAG_ONE_LIGHT's); the tree after trt_update_geometry; the estimator against all-lights under the statistical
criterion of tests/test_near_lights_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import near_cases as NC
import nearlights_lib as NL
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu
W, H, SPP, SEED = 32, 18, 4, 0x2EA7
FLAG_SETS = {"near": NL.FLAGS, "offset_pixels": NL.FLAGS | T.TRT_FLAG_RAY_OFFSET | T.TRT_FLAG_FIXED_PIXELS}
NAMED = {"lamps1": ("lamps", {"n": 1}), "lamps7": ("lamps", {"n": 7}), "lamps8": ("lamps", {"n": 8}), "lamps64": ("lamps", {"n": 64}), "lamps300": ("lamps", {"n": 300}),
         "staircase": ("staircase", {}), "veach-mis": ("veach-mis", {})}
PARITY_SCENES = ["lamps1", "lamps7", "lamps64", "lamps300", "staircase", "veach-mis"] + list(NC.CASES)
K = {n: i for i, n in enumerate(T.KERNEL_NAMES)}
_refs = {}
_handles = {}


def scene(key):
    if key in NAMED:
        name, kw = NAMED[key]
        return get_scene(name, W, H, **kw)
    return NC.scene(key, W, H)


def params(flags, **kw):
    return T.make_params(W, H, SPP, SEED, flags=flags, **kw)


def cpu(key, flags, tile=None, rows=None):
    """The CPU build's render, computed once per case and shared."""
    k = (key, flags, tile, rows)
    if k not in _refs:
        _refs[k] = NL.render(scene(key).flat, T.make_params(W, H, SPP, SEED, tile=tile, rows=rows, flags=flags))
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


# ---- bit parity: every scene, both flag sets, every entry; queue kernels (TRT_TAIL_N=0: k_shade's SHADE_NEAR at every bounce) and k_tail ----

@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("key", PARITY_SCENES)
def test_every_entry_matches_the_cpu_build(key, flags, monkeypatch, capfd):
    fl = FLAG_SETS[flags]
    s = scene(key)
    assert s.info["n_lights"] >= 2
    ref = cpu(key, fl)
    one, _ = NL.render(s.flat, params(fl), NL.ONE_LIGHT)
    assert one.tobytes() != ref[0].tobytes(), "the descent picks what power alone picks: the case shows nothing"
    for env in ({"TRT_TAIL_N": "0", "TRT_DEBUG": "1"}, {}):
        r = handle(key, env, monkeypatch)
        capfd.readouterr()
        img, st = r.render(params(fl))
        err = capfd.readouterr().err
        same(img, st, ref, f"{key} {flags} trt_render {env}")
        assert (st.launches[K["tail"]] == 0) == bool(env)
        assert st.rays_shadow <= st.shaded_hits
        if env:
            assert "k_shade near" in err, err
    r = handle(key, {"TRT_TAIL_N": "0", "TRT_DEBUG": "1"}, monkeypatch)
    # a tile with interleaved rows
    tile, rows = (3, 2, 29, 17), (2, 2, 1)
    img, st = r.render(params(fl, tile=tile, rows=rows))
    same(img, st, cpu(key, fl, tile, rows), f"{key} {flags} tile")
    # trt_render_pixels: every pixel twice, shuffled
    rng = np.random.default_rng(5)
    pixels = rng.permutation(np.concatenate([np.arange(W * H), np.arange(W * H)])).astype(np.uint32)
    want = ref[0].reshape(-1, 3)[pixels]
    capfd.readouterr()
    sums, _, st = r.render_pixels(params(fl), pixels, 0, SPP)
    assert "k_shade near" in capfd.readouterr().err
    assert sums.astype(np.float32).tobytes() == want.tobytes(), f"{key} {flags} trt_render_pixels"
    assert [st.rays_camera, st.rays_shadow, st.rays_indirect] == [2 * x for x in ref[1]]
    # trt_render_rays on trt_camera_rays of the same pixels, with the pixels as stream ids
    cam = s.flat.contents.camera
    org, d = T.camera_rays(cam, params(fl), pixels, 0, SPP)
    rsums, _, rst = r.render_rays(params(fl), org, d, streams=pixels)
    assert "k_shade near" in capfd.readouterr().err
    assert rsums.tobytes() == sums.tobytes(), f"{key} {flags} trt_render_rays"
    assert [rst.rays_camera, rst.rays_shadow, rst.rays_indirect] == [st.rays_camera, st.rays_shadow, st.rays_indirect]
    # trt_group_render on a group of one device
    g = T.GroupRenderer(s, [0])
    try:
        img, gst, _ = g.render(params(fl))
    finally:
        g.close()
    same(img, gst, ref, f"{key} {flags} trt_group_render")


# the forced routes of tests/test_gpu_one_light.py: (environment at trt_create, extra flags, two passes)
ROUTES = {
    "persistent_driver_on_a_small_tree": ({"TRT_TRACE_IMPL": "3", "TRT_TAIL_N": "0"}, 0, False),
    "persistent_driver_oct": ({"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1", "TRT_TAIL_N": "0"}, 0, False),
    "tail_takes_everything": ({"TRT_TAIL_N": str(1 << 30)}, 0, False),
    "shadow_stream_off": ({"TRT_SHADOW_STREAM": "0", "TRT_TAIL_N": "0"}, 0, False),
    "shadow_stream_on": ({"TRT_SHADOW_STREAM": "1", "TRT_TAIL_N": "64"}, 0, False),
    "overlap": ({"TRT_TAIL_N": "0"}, T.TRT_FLAG_OVERLAP, True),
    "two_passes": ({"TRT_TAIL_N": "64"}, 0, True),
}


def test_routes_are_those_of_the_one_light_test():
    import test_gpu_one_light as G1
    assert ROUTES == G1.ROUTES


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("key", ["lamps8", "lamps64", "staircase", "corridor16"])
def test_forced_routes_match_the_cpu_build(key, route, monkeypatch, capfd):
    env, extra, two_passes = ROUTES[route]
    r = handle(key, dict(env, TRT_DEBUG="1"), monkeypatch)
    budget = 180 * W * H * 2 if two_passes else 0  # two samples of every pixel per pass
    capfd.readouterr()
    img, st = r.render(params(NL.FLAGS | extra, mem_budget=budget))
    err = capfd.readouterr().err
    same(img, st, cpu(key, NL.FLAGS), f"{key} {route}")
    assert "k_shade near" in err and "fused primary 0" in err, err
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
    # the same handle without the flag: TRT_FLAG_ONE_LIGHT's flavour and render
    import onelight_lib as OL
    capfd.readouterr()
    img, st = r.render(params(OL.FLAGS | extra, mem_budget=budget))
    assert "k_shade pick" in capfd.readouterr().err
    want, rays = NL.render(scene(key).flat, params(OL.FLAGS), NL.ONE_LIGHT)
    assert img.tobytes() == want.tobytes() and [st.rays_camera, st.rays_shadow, st.rays_indirect] == rays


# ---- the flag rules ------------------------------------------------------------------------------------------------------------------------

def test_flag_without_one_light_is_einval_on_every_entry_and_the_handle_goes_on(monkeypatch):
    r = handle("lamps8", {"TRT_TAIL_N": "0"}, monkeypatch)
    pixels = np.arange(8, dtype=np.uint32)
    org, d = T.camera_rays(scene("lamps8").flat.contents.camera, params(NL.FLAGS), pixels, 0, 1)
    lib = T._abi.load_hip()
    out = np.zeros((H, W, 3), np.float32)
    for bad in (params(T.TRT_FLAG_NEAR_LIGHTS | T.TRT_FLAG_FIXED_NEE), params(T.TRT_FLAG_NEAR_LIGHTS)):
        calls = [lambda: r.render(bad), lambda: r.render_samples(bad, 0, 1), lambda: r.render_pixels(bad, pixels, 0, 1),
                 lambda: r.render_rays(bad, org, d, streams=pixels)]
        for call in calls:
            with pytest.raises(T.TrtError, match="TRT_FLAG_NEAR_LIGHTS needs TRT_FLAG_ONE_LIGHT"):
                call()
        assert lib.trt_render(r._h, C.byref(bad), out.ctypes.data_as(C.POINTER(C.c_float)), None) == 1  # TRT_EINVAL
        g = T.GroupRenderer(scene("lamps8"), [0])
        try:
            with pytest.raises(T.TrtError, match="TRT_FLAG_NEAR_LIGHTS needs TRT_FLAG_ONE_LIGHT"):
                g.render(bad)
        finally:
            g.close()
        r.render_aov(bad)  # the feature entries ignore the estimator flags
    with pytest.raises(T.TrtError, match="TRT_FLAG_ONE_LIGHT needs TRT_FLAG_FIXED_NEE"):
        r.render(params(T.TRT_FLAG_NEAR_LIGHTS | T.TRT_FLAG_ONE_LIGHT))
    img, st = r.render(params(NL.FLAGS))
    same(img, st, cpu("lamps8", NL.FLAGS), "after TRT_EINVAL")


def test_one_light_scene_renders_fixed_nee_bit_for_bit(monkeypatch):
    s = get_scene("back", W, H)
    for env in ({"TRT_TAIL_N": "0"}, {}):
        for n, v in env.items():
            monkeypatch.setenv(n, v)
        r = T.Renderer(s, 0)
        for n in env:
            monkeypatch.delenv(n)
        try:
            a, sa = r.render(params(NL.FLAGS))
            b, sb = r.render(params(T.TRT_FLAG_FIXED_NEE))
        finally:
            r.close()
        assert a.tobytes() == b.tobytes() and b.max() > 0
        assert (sa.rays_camera, sa.rays_shadow, sa.rays_indirect, sa.shaded_hits) == (sb.rays_camera, sb.rays_shadow, sb.rays_indirect, sb.shaded_hits)
    ref, rays = NL.render(s.flat, params(NL.FLAGS))
    assert a.tobytes() == ref.tobytes() and [sa.rays_camera, sa.rays_shadow, sa.rays_indirect] == rays


# ---- the shape of the work -------------------------------------------------------------------------------------------------------------

def test_work_is_that_of_a_one_light_scene(monkeypatch):
    r = handle("lamps64", {"TRT_TAIL_N": "0"}, monkeypatch)
    paths = W * H * SPP
    img, st = r.render(params(NL.FLAGS, mem_budget=180 * paths))
    assert st.passes == 1  # 132 + 48 bytes per path suffice
    assert 0 < st.rays_shadow <= st.shaded_hits
    assert 0 < st.launches[K["trace_shadow"]] <= st.launches[K["trace_closest"]]  # one shadow launch per bounce
    same(img, st, cpu("lamps64", NL.FLAGS), "at 180 bytes per path")


# ---- trt_update_geometry rebuilds the tree ---------------------------------------------------------------------------------------------------

def test_update_geometry_that_moves_the_lamps(monkeypatch, tmp_path):
    d = tmp_path / "moving"
    d.mkdir()
    NC.write_case(str(d), "corridor16", W, H)
    import scene_util as SU
    s = SU.load(str(d), "corridor16")
    monkeypatch.setenv("TRT_TAIL_N", "0")
    r = T.Renderer(s, 0)
    try:
        before, bst = r.render(params(NL.FLAGS))
        same(before, bst, cpu("corridor16", NL.FLAGS), "before the update")
        # lights == NULL and unmoved emitters: the tree is not touched, the render unchanged
        r.update_geometry(s.arrays()["tri_v"])
        again, ast = r.render(params(NL.FLAGS))
        assert again.tobytes() == before.tobytes() and (ast.rays_shadow, ast.rays_indirect) == (bst.rays_shadow, bst.rays_indirect)
        s.set_vertices(NC.moved_lamps(s))
        r.update_geometry(s)
        after, st = r.render(params(NL.FLAGS))
        fresh = T.Renderer(s, 0)
        try:
            want, wst = fresh.render(params(NL.FLAGS))
        finally:
            fresh.close()
    finally:
        r.close()
    assert after.tobytes() == want.tobytes()
    assert (st.rays_shadow, st.rays_indirect) == (wst.rays_shadow, wst.rays_indirect)
    assert after.tobytes() != before.tobytes()
    ref, rays = NL.render(s.flat, params(NL.FLAGS))
    assert after.tobytes() == ref.tobytes() and [st.rays_camera, st.rays_shadow, st.rays_indirect] == rays


# ---- unbiased on the device ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lamps", "staircase", "corridor"])
def test_near_is_unbiased_against_all_lights_on_the_device(name, monkeypatch):
    """The N and the scenes of tests/test_near_lights_cpu.py at 24 x 16, with the moments (and their Cauchy-Schwarz bound) of tests/test_gpu_one_light.py."""
    from test_gpu_one_light import _device_moments
    from test_near_lights_cpu import CRITERION_SCENES, SEED_A, SEED_B, SEED_C, criterion_scene
    n = CRITERION_SCENES[name]
    monkeypatch.setenv("TRT_TAIL_N", "0")
    r = T.Renderer(criterion_scene(name), 0)
    monkeypatch.delenv("TRT_TAIL_N")
    try:
        near = _device_moments(r, NL.FLAGS, SEED_C, n)
        ref_a = _device_moments(r, T.TRT_FLAG_FIXED_NEE, SEED_A, n)
        ref_b = _device_moments(r, T.TRT_FLAG_FIXED_NEE, SEED_B, n)
    finally:
        r.close()
    a, b = NL.criterion(*near, *ref_a), NL.criterion(*ref_a, *ref_b)
    print(f"device {name} N={n}: near vs all-lights {a}, all-lights vs all-lights {b}")
    assert a[2] >= (40 if name == "corridor" else 100)
    assert NL.passes(a[0], a[1]), a
    assert NL.passes(b[0], b[1]), b


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------

def test_tinyrt_near_lights_sets_the_three_flags(tmp_path):
    s = T.Scene.named("veach-mis", leaf_num=2)
    w, h = s.info["width"], s.info["height"]
    r = T.Renderer(s, 0)
    try:
        img, _ = r.render(T.make_params(w, h, 2, 77, flags=NL.FLAGS))
        one, _ = r.render(T.make_params(w, h, 2, 77, flags=T.TRT_FLAG_ONE_LIGHT | T.TRT_FLAG_FIXED_NEE))
    finally:
        r.close()
    assert img.tobytes() != one.tobytes()
    exe = os.path.join(os.path.dirname(T.__file__), "lib", "tinyrt")
    d = os.path.join(T.SCENES_DIR, "veach-mis")
    out = str(tmp_path / "cli.png")
    run = subprocess.run([exe, d, os.path.join(d, "veach-mis.mtl"), os.path.join(d, "veach-mis.xml"), os.path.join(d, "veach-mis.obj"), "2", "--leaf", "2",
                          "--seed", "77", "--near-lights", "--out", out], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode()
    T.imshow(img, str(tmp_path / "lib.png"))
    assert open(out, "rb").read() == open(str(tmp_path / "lib.png"), "rb").read()
