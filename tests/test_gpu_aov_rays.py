"""trt_aov_rays / trt_aov_rays_device, Renderer.render_camera_aov and Renderer.render_camera_denoised (first-hit feature buffers along
caller-supplied rays) — MI355X only.

Bars, all bit-exact:
  1. the built-in camera through the new entry: the rays of trt_camera_rays from zeros leave, rounded to float, trt_render_aov's buffers —
     the wave-uniform walk with 8-byte hits, the 4-wide and 8-wide per-lane walks, textures and split leaves, an LBVH tree;
  2. a moved camera on a handle created with another one: the sums are tests/aov_rays_ref.py's, render_camera_aov gives the same bits, and
     so does trt_render_aov on a fresh handle of the scene copy with that camera;
  3. rays no pinhole makes (4096 directions of random length from one point): depth is trt_trace_closest's t, albedo and normal the helper's;
  4. the lengths where packing and per-entry indexing can go wrong, invalid entries wherever a wave or a block can trip over them;
  5. resumption, sample_end > spp, several passes, TRT_ENOMEM, the device entry with every NULL combination, the refusals, the launch counts;
  6. a render, a ray batch and trt_render_aov do not change around calls of the new entry;
  7. render_camera_denoised is render_denoised with the handle's own camera, and consistent with its parts with a moved one.
"""
import ctypes as C

import numpy as np
import pytest

import aov_rays_ref as R
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd._abi import SceneFlat

pytestmark = pytest.mark.gpu

W, H = 64, 36
SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}
KEYS = R.KEYS
K_GEN, K_TRACE, K_RESOLVE = (T.KERNEL_NAMES.index(k) for k in ("gen_primary", "trace_closest", "resolve"))


def fresh_renderer(s, env, monkeypatch):
    """A Renderer created under `env` (read at trt_create)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return T.Renderer(s, 0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def tile_pixels(p):
    ys = np.asarray(T.rows_selected(p), np.int64)
    xs = np.arange(p.x0, p.x1, dtype=np.int64)
    return (ys[:, None] * p.width + xs[None, :]).reshape(-1).astype(np.uint32)


def assert_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    view = np.uint64 if a.dtype == np.float64 else np.uint32
    bad = np.ascontiguousarray(a).view(view) != np.ascontiguousarray(b).view(view)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}: {a[tuple(np.argwhere(bad)[0])]} != {b[tuple(np.argwhere(bad)[0])]}"


def assert_sums(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in got:
        assert_bits(got[k], want[k], f"{what}: {k}")


def as_buffers(sums, shape=(H, W)):
    """(float)sum in the shape of trt_render_aov's buffers"""
    return {k: sums[k].astype(np.float32).reshape(shape + ((3,) if k != "depth" else ())) for k in KEYS}


def moved_camera():
    # the Cornell box of `back` from up and to the right of its own camera, turned towards the lower left, slightly rolled
    return T.look_at((420.0, 390.0, -650.0), (230.0, 200.0, 280.0), (0.08, 1.0, 0.02), 47.0, W, H)


class SceneView:
    """The flat description of a scene (the arrays stay the scene's) seen through another camera, for Renderer()."""

    def __init__(self, s, cam):
        self._scene = s
        self._flat = SceneFlat.from_buffer_copy(s.flat.contents)
        self._flat.camera = cam
        self.flat = C.pointer(self._flat)


_rays = {}


def builtin_rays(name, spp, flags=0):
    """The rays of the scene's own camera over the whole image, computed once per (scene, spp, flags)"""
    key = (name, spp, flags)
    if key not in _rays:
        s = get_scene(name, W, H)
        p = T.make_params(W, H, spp, SEEDS[name], flags=flags)
        _rays[key] = T.camera_rays(s.flat.contents.camera, p, tile_pixels(p), 0, spp)
    return _rays[key]


# ---- 1. the built-in camera through the new entry --------------------------------------------------------------------------------
KINDS = {"default": {}, "wide4": {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, "oct8": {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}}
SPP1 = {"back": 8, "veach-mis": 4, "staircase": 4}
CASES1 = [(n, k, 0) for n in ("back", "veach-mis", "staircase") for k in KINDS] + \
         [("back", "default", T.TRT_FLAG_FIXED_PIXELS), ("staircase", "default", T.TRT_FLAG_FIXED_PIXELS | T.TRT_FLAG_COUNT | T.TRT_FLAG_TIMING)]


@pytest.mark.parametrize("name,kind,flags", CASES1, ids=[f"{n}/{k}/{f}" for n, k, f in CASES1])
def test_builtin_camera_rays_equal_render_aov(name, kind, flags, monkeypatch):
    s = get_scene(name, W, H)
    spp = SPP1[name]
    p = T.make_params(W, H, spp, SEEDS[name], flags=flags)
    org, dirs = builtin_rays(name, spp, flags & T.TRT_FLAG_FIXED_PIXELS)
    r = fresh_renderer(s, KINDS[kind], monkeypatch)
    try:
        want, st_ref = r.render_aov(p, want_stats=True)
        got, st = r.render_aov_rays(p, org, dirs, want_stats=True)
    finally:
        r.close()
    assert want["albedo"].any() and want["normal"].any()
    assert_sums(as_buffers(got), want, f"{name}/{kind}: (float)sum vs trt_render_aov")
    assert st.rays_camera == W * H * spp == st_ref.rays_camera and st.rays_shadow == 0 and st.rays_indirect == 0
    assert st.rows_rendered == 0 and st.passes == 1 and st.inner_node_bytes == st_ref.inner_node_bytes
    assert st.launches[K_GEN] == st.launches[K_TRACE] == st.launches[K_RESOLVE] == st.passes
    if flags & T.TRT_FLAG_COUNT:
        assert st.tri_tests[0] == st_ref.tri_tests[0] > 0 and st.inner_visits[0] == st_ref.inner_visits[0]
    if flags & T.TRT_FLAG_TIMING:
        assert st.kernel_ms[K_TRACE] > 0 and st.kernel_ms[K_GEN] > 0 and st.kernel_ms[K_RESOLVE] > 0 and st.render_ms > 0


def test_builtin_camera_rays_on_an_lbvh_tree():
    s = T.Scene.named("veach-mis", W, H, builder="lbvh")
    p = T.make_params(W, H, 4, SEEDS["veach-mis"])
    org, dirs = builtin_rays("veach-mis", 4)  # the camera does not depend on the tree
    r = T.Renderer(s, 0)
    try:
        assert_sums(as_buffers(r.render_aov_rays(p, org, dirs)), r.render_aov(p), "lbvh: (float)sum vs trt_render_aov")
    finally:
        r.close()


# ---- 2. a moved camera on a resident handle -------------------------------------------------------------------------------------
def test_moved_camera(renderer_factory):
    s = get_scene("back", W, H)
    r = renderer_factory(s)  # created with the scene's own camera
    cam = moved_camera()
    spp = 6
    p = T.make_params(W, H, spp, SEEDS["back"])
    org, dirs = T.camera_rays(cam, p, tile_pixels(p), 0, spp)
    got = r.render_aov_rays(p, org, dirs)
    assert_sums(got, R.aov_rays(s, org, dirs, spp), "moved camera: sums vs the restatement")
    own = r.render_aov(p)
    assert (as_buffers(got)["depth"] != own["depth"]).any(), "the moved camera must see other buffers"
    for k in (4, 1):  # 4 + 2 samples, and one at a time
        bufs, st = r.render_camera_aov(p, cam, samples_per_call=k, want_stats=True)
        assert_sums(bufs, as_buffers(got), f"render_camera_aov, {k} samples per call")
        assert st.rays_camera == W * H * spp and st.passes == (spp + k - 1) // k
    dev = r.render_camera_aov(p, cam, on_device=True)
    assert all(v.is_cuda for v in dev.values())
    assert_sums({k: v.cpu().numpy() for k, v in dev.items()}, as_buffers(got), "render_camera_aov, on_device")
    fresh = T.Renderer(SceneView(s, cam), 0)
    try:
        assert_sums(fresh.render_aov(p), as_buffers(got), "trt_render_aov of a handle created with the moved camera")
    finally:
        fresh.close()
    assert_sums(r.render_aov(p), own, "trt_render_aov afterwards")


def test_render_camera_aov_on_a_sub_tile_with_fixed_pixels(renderer_factory):
    s = get_scene("staircase", W, H)
    r = renderer_factory(s)
    p = T.make_params(W, H, 5, SEEDS["staircase"], tile=(5, 3, 50, 31), rows=(2, 3, 1), flags=T.TRT_FLAG_FIXED_PIXELS)
    assert_sums(r.render_camera_aov(p, s.flat.contents.camera, samples_per_call=2), r.render_aov(p), "interleaved sub-tile")


# ---- 3. rays no pinhole makes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["back", "staircase"])
def test_rays_of_any_length_from_one_point(name, renderer_factory):
    s = get_scene(name, W, H)
    r = renderer_factory(s)
    rng = np.random.default_rng(33)
    n = 4096
    # back: inside the Cornell box, above the cube; staircase: where its camera stands
    eye = np.array([278.0, 400.0, 150.0], np.float32) if name == "back" else np.array(list(s.flat.contents.camera.eye), np.float32)
    d = rng.normal(size=(n, 3))
    dirs = (d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.01, 300.0, (n, 1))).astype(np.float32)[None]
    org = np.tile(eye, (1, n, 1))
    p = T.make_params(W, H, 1, SEEDS[name])
    t, tri, _ = r.trace_closest(org[0], dirs[0])
    got, st = r.render_aov_rays(p, org, dirs, want_stats=True)
    assert (tri >= 0).sum() > n // 2 and st.rays_camera == n
    assert_bits(got["depth"], t.astype(np.float64), f"{name}: depth vs trt_trace_closest's t")
    want = R.aov_rays(s, org, dirs, 1)
    assert_sums(got, want, f"{name}: sums vs the restatement")


# ---- 4. shapes where packing and per-entry indexing can go wrong ---------------------------------------------------------------
def poison(org, dirs, idx, k):
    """Entry idx made invalid in one of six ways"""
    nan, inf = np.float32("nan"), np.float32("inf")
    if k % 6 == 0:
        org[idx, 1] = nan
    elif k % 6 == 1:
        dirs[idx, 0] = inf
    elif k % 6 == 2:
        dirs[idx] = 0.0
    elif k % 6 == 3:
        dirs[idx, 2] = nan
    elif k % 6 == 4:
        org[idx, 0] = -inf
    else:
        dirs[idx] = (-0.0, 0.0, -0.0)


def random_sums(n, rng):
    return {"albedo": rng.uniform(0.5, 2.0, (n, 3)), "normal": rng.uniform(-1.0, 1.0, (n, 3)), "depth": rng.uniform(0.5, 2.0, n)}


def copy_sums(sums):
    return {k: v.copy() for k, v in sums.items()}


@pytest.mark.parametrize("name", ["back", "veach-mis"])  # 8-byte and 16-byte hit records
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_list_lengths_and_invalid_entries(n, name, renderer_factory):
    s = get_scene(name, W, H)
    r = renderer_factory(s)
    spp, n_samples = 4, 3
    p = T.make_params(W, H, spp, SEEDS[name])
    full_o, full_d = builtin_rays(name, 4)
    org, dirs = full_o[:n_samples, 700:700 + n].copy(), full_d[:n_samples, 700:700 + n].copy()  # the middle rows: hits and misses
    rng = np.random.default_rng(n)
    start = random_sums(n, rng)
    clean, clean_st = r.render_aov_rays(p, org, dirs, sums=copy_sums(start), want_stats=True)
    assert clean_st.rays_camera == n * n_samples and clean_st.passes == 1
    assert_sums(clean, R.aov_rays(s, org, dirs, spp, sums=copy_sums(start)), f"n = {n}: clean sums vs the restatement")
    # lane 0, lane 63, the first and the last thread of a block of the packing kernel, the last entry; sample 1 (entry index 1 * n + e:
    # another lane and another block than e) loses more, sample 2 nothing
    marks = [np.r_[0, 63, 64, 255, 256, n - 1], np.r_[0, 1, 62, 63, 127, 128, 255, 256, 511, 512, n - 2, n - 1], np.r_[:0]]
    bad = [np.unique(m[(m >= 0) & (m < n)]) for m in marks]
    dirty_o, dirty_d = org.copy(), dirs.copy()
    for k in range(n_samples):
        for j, idx in enumerate(bad[k]):
            poison(dirty_o[k], dirty_d[k], idx, j + k)
    got, st = r.render_aov_rays(p, dirty_o, dirty_d, sums=copy_sums(start), want_stats=True)
    assert st.rays_camera == n * n_samples - len(bad[0]) - len(bad[1])
    valid = np.setdiff1d(np.arange(n), np.union1d(bad[0], bad[1]))
    for k in KEYS:
        assert_bits(got[k][valid], clean[k][valid], f"n = {n}: {k} of the entries that stayed valid")
    # the invalid ones: exactly the miss's terms for that sample, the traced ones for the others
    feats = R.aov_rays(s, dirty_o, dirty_d, spp, sums=copy_sums(start))
    assert_sums(got, feats, f"n = {n}: sums with invalid entries vs the restatement")
    only = np.setdiff1d(bad[0], bad[1])  # invalid in sample 0 only
    if len(only):
        miss0 = R.accumulate(np.zeros((1, n, 3), np.float32), np.zeros((1, n, 3), np.float32), np.zeros((1, n), np.float32), np.zeros((1, n), bool), spp,
                             sums=copy_sums(start))
        rest, _ = r.render_aov_rays(p, org[1:], dirs[1:], sample_begin=1, sums=miss0, want_stats=True)
        for k in KEYS:
            assert_bits(got[k][only], rest[k][only], f"n = {n}: {k}, invalid in the first sample only")


def test_nothing_valid_and_odd_directions(renderer_factory):
    s = get_scene("veach-mis", W, H)
    r = renderer_factory(s)
    spp = 3
    p = T.make_params(W, H, spp, SEEDS["veach-mis"])
    n = 65
    eye = np.array(list(s.flat.contents.camera.eye), np.float32)
    org = np.tile(eye, (2, n, 1))
    dirs = np.zeros((2, n, 3), np.float32)
    dirs[1, ::2, 0] = np.float32("nan")
    start = random_sums(n, np.random.default_rng(5))
    got, st = r.render_aov_rays(p, org, dirs, sums=copy_sums(start), want_stats=True)
    miss = R.accumulate(np.ones((2, n, 3), np.float32), np.ones((2, n, 3), np.float32), np.ones((2, n), np.float32), np.zeros((2, n), bool), spp,
                        sums=copy_sums(start))
    assert_sums(got, miss, "no valid entry: the miss sums")
    assert st.rays_camera == 0 and st.passes == 1 and st.launches[K_TRACE] == 1
    # a single zero component, axis-aligned, non-unit and denormal components are valid
    tiny = np.float32(1e-42)
    dirs = np.array([[5, 0, 0], [0, -2, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 0], [0, 1, 0], [0.001, 0.002, -0.0005], [300, -200, 100], [0, 0.3, -0.9],
                     [tiny, 0.2, -1.0], [0.1, -tiny, -1.0]], np.float32)[None]
    o8 = org[:1, :dirs.shape[1]].copy()
    o8[0, 9, 1] += tiny
    got, st = r.render_aov_rays(p, o8, dirs, want_stats=True)
    assert st.rays_camera == dirs.shape[1]
    t, tri, _ = r.trace_closest(o8[0], dirs[0])
    assert (tri >= 0).any()
    assert_bits(got["depth"], (t / np.float32(spp)).astype(np.float32).astype(np.float64), "odd directions: depth vs trt_trace_closest's t")
    assert_sums(got, R.aov_rays(s, o8, dirs, spp), "odd directions: sums vs the restatement")


# ---- 5. plumbing ----------------------------------------------------------------------------------------------------------------
def test_resumption_passes_and_budget(renderer_factory):
    s = get_scene("staircase", W, H)
    r = renderer_factory(s)
    spp = 4
    p = T.make_params(W, H, spp, SEEDS["staircase"])
    n = 777
    pix = np.random.default_rng(5).permutation(np.arange(W * H, dtype=np.uint32))[:n]
    org, dirs = T.camera_rays(moved_camera_of(s), p, pix, 0, 6)  # sample_end > spp: spp only scales the terms
    whole, st = r.render_aov_rays(p, org, dirs, want_stats=True)
    assert st.passes == 1 and st.rays_camera == 6 * n
    assert_sums(whole, R.aov_rays(s, org, dirs, spp), "[0, 6) at spp = 4 vs the restatement")
    part = r.render_aov_rays(p, org[:3], dirs[:3])
    part = r.render_aov_rays(p, org[3:], dirs[3:], sample_begin=3, sums=part)
    assert_sums(part, whole, "[0, 3) then [3, 6) vs [0, 6)")
    small = T.make_params(W, H, spp, SEEDS["staircase"], mem_budget=n * T.AOV_RAYS_BYTES_PER_PATH * 2)
    got, st = r.render_aov_rays(small, org, dirs, want_stats=True)
    assert st.passes >= 3 and st.launches[K_GEN] == st.launches[K_TRACE] == st.launches[K_RESOLVE] == st.passes
    assert_sums(got, whole, "two samples per pass vs one pass")
    tight = T.make_params(W, H, spp, SEEDS["staircase"], mem_budget=n * T.AOV_RAYS_BYTES_PER_PATH - 1)
    with pytest.raises(T.TrtError, match=r"\(3\)"):
        r.render_aov_rays(tight, org, dirs)
    assert_sums(r.render_aov_rays(p, org, dirs), whole, "after TRT_ENOMEM")


def moved_camera_of(s):
    """The scene's own camera, two units to the right and one up"""
    from tinyraytracing_amd._abi import Camera, c_float3
    c = s.flat.contents.camera
    cam = Camera.from_buffer_copy(c)
    h = np.array(list(c.horizontal), np.float32)
    v = np.array(list(c.vertical), np.float32)
    shift = (h / np.linalg.norm(h) * 2.0 + v / np.linalg.norm(v)).astype(np.float32)
    cam.eye = c_float3(*[float(x) for x in np.array(list(c.eye), np.float32) + shift])
    cam.lower_left_corner = c_float3(*[float(x) for x in np.array(list(c.lower_left_corner), np.float32) + shift])
    return cam


def test_device_entry_on_a_side_stream_and_null_outputs(renderer_factory):
    import torch
    s = get_scene("back", W, H)
    r = renderer_factory(s)
    spp = 5
    p = T.make_params(W, H, spp, SEEDS["back"])
    n = 611
    pix = np.random.default_rng(9).choice(np.arange(W * H, dtype=np.uint32), n, replace=True).astype(np.uint32)
    org, dirs = T.camera_rays(moved_camera(), p, pix, 0, spp)
    sentinel = -7.0
    shapes = {"albedo": (n, 3), "normal": (n, 3), "depth": (n,)}
    ref = r.render_aov_rays(p, org, dirs, sums={k: np.full(shapes[k], sentinel) for k in KEYS})  # in/out: the sums start at the sentinel
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    t_org, t_dir = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
    for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
        bufs = {k: torch.full(shapes[k], sentinel, dtype=torch.float64, device=dev) for k in KEYS}
        torch.cuda.synchronize()
        st = r.render_aov_rays_into(p, t_org, t_dir, stream_ptr=side.cuda_stream, **{k: bufs[k] for k, w in zip(KEYS, want) if w})
        assert st.rays_camera == n * spp
        for k, w in zip(KEYS, want):
            got = bufs[k].cpu().numpy()
            if w:
                assert_bits(got, ref[k], f"{want}: {k}")
            else:
                assert (got == sentinel).all(), f"{want}: {k} was not asked for and was written"
    # in/out on the device: [0, 2) then [2, 5) from zeros is the host's [0, 5) from zeros
    zero = r.render_aov_rays(p, org, dirs)
    bufs = {k: torch.zeros(shapes[k], dtype=torch.float64, device=dev) for k in KEYS}
    r.render_aov_rays_into(p, t_org[:2].contiguous(), t_dir[:2].contiguous(), **bufs)
    r.render_aov_rays_into(p, t_org[2:].contiguous(), t_dir[2:].contiguous(), sample_begin=2, **bufs)
    assert_sums({k: v.cpu().numpy() for k, v in bufs.items()}, zero, "device resume")
    with pytest.raises(T.TrtError, match="at least one"):
        r.render_aov_rays_into(p, t_org, t_dir)
    with pytest.raises(T.TrtError, match="contiguous"):
        r.render_aov_rays_into(p, t_org.transpose(0, 1), t_dir, depth=bufs["depth"])
    with pytest.raises(T.TrtError, match="float64"):
        r.render_aov_rays_into(p, t_org, t_dir, depth=bufs["depth"].to(torch.float32))


def test_refusals_leave_the_handle_usable(renderer_factory):
    s = get_scene("back", W, H)
    r = renderer_factory(s)
    lib = r._lib
    spp = 4
    p = T.make_params(W, H, spp, SEEDS["back"])
    pix = np.random.default_rng(1).permutation(np.arange(W * H, dtype=np.uint32))[:50]
    org, dirs = T.camera_rays(s.flat.contents.camera, p, pix, 0, spp)
    a, nr, z = np.zeros((50, 3)), np.zeros((50, 3)), np.zeros(50)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    o_p, d_p, a_p, n_p, z_p = org.ctypes.data_as(fp), dirs.ctypes.data_as(fp), a.ctypes.data_as(dp), nr.ctypes.data_as(dp), z.ctypes.data_as(dp)
    st = T.Stats()

    def call(n, o, d, b, e, al, no, de, params=p, handle=r._h):
        return lib.trt_aov_rays(handle, None if params is None else C.byref(params), n, o, d, b, e, al, no, de, C.byref(st))

    no_spp = T.make_params(W, H, 0, SEEDS["back"])
    refusals = {
        "null handle": call(50, o_p, d_p, 0, 2, a_p, n_p, z_p, handle=None),
        "null params": call(50, o_p, d_p, 0, 2, a_p, n_p, z_p, params=None),
        "null org": call(50, None, d_p, 0, 2, a_p, n_p, z_p),
        "null dir": call(50, o_p, None, 0, 2, a_p, n_p, z_p),
        "all sums null": call(50, o_p, d_p, 0, 2, None, None, None),
        "begin < 0": call(50, o_p, d_p, -1, 2, a_p, n_p, z_p),
        "begin > end": call(50, o_p, d_p, 3, 2, a_p, n_p, z_p),
        "spp < 1": call(50, o_p, d_p, 0, 2, a_p, n_p, z_p, params=no_spp),
        # checked before an array is read or any memory is sized by it
        "path-id range": call(0x7FFF0001, o_p, d_p, 0, 1, a_p, n_p, z_p),
    }
    for what, rc in refusals.items():
        assert rc == 1, f"{what}: returned {rc}, not TRT_EINVAL"
    assert not a.any() and not nr.any() and not z.any(), "a refused call wrote the sums"
    # no-ops: nothing listed, or an empty range
    assert call(0, None, None, 0, 4, a_p, None, None) == 0
    assert call(50, o_p, d_p, 3, 3, a_p, n_p, z_p) == 0 and not a.any() and not z.any()
    # everything else of p means nothing here
    odd = T.make_params(W, H, spp, 12345, max_depth=3, flags=T.TRT_FLAG_OVERLAP | T.TRT_FLAG_FIXED_NEE | T.TRT_FLAG_FIXED_PIXELS)
    odd.width, odd.height, odd.x1, odd.y1, odd.max_depth = 0, -3, 0, 0, -1
    assert call(50, o_p, d_p, 0, spp, a_p, n_p, z_p, params=odd) == 0
    want = r.render_aov_rays(p, org, dirs)
    assert_sums({"albedo": a, "normal": nr, "depth": z}, want, "ignored fields of p")
    assert_sums(want, R.aov_rays(s, org, dirs, spp), "after refusals: sums vs the restatement")


# ---- 6. neighbours undisturbed --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["back", "staircase"])
def test_neighbours_do_not_change_around_the_new_entry(name, renderer_factory):
    s = get_scene(name, W, H)
    r = renderer_factory(s)
    p = T.make_params(W, H, 4, SEEDS[name])
    org, dirs = builtin_rays(name, 4)

    def neighbours():
        img, _ = r.render(p)
        t, tri, uv = r.trace_closest(org[0], dirs[0])
        return img, t, tri.view(np.float32), uv, r.render_aov(p)

    before = neighbours()
    first = r.render_aov_rays(p, org, dirs)
    r.render_aov_rays(T.make_params(W, H, 4, SEEDS[name], mem_budget=W * H * T.AOV_RAYS_BYTES_PER_PATH), org[:3], dirs[:3], sums={"depth": np.zeros(W * H)})
    r.render_aov_rays(p, org[:1, :65], dirs[:1, :65])
    after = neighbours()
    for b, a, what in zip(before[:4], after[:4], ("trt_render", "t", "tri", "uv")):
        assert_bits(a, b, f"{name}: {what} around trt_aov_rays")
    assert_sums(after[4], before[4], f"{name}: trt_render_aov around trt_aov_rays")
    assert_sums(r.render_aov_rays(p, org, dirs), first, f"{name}: trt_aov_rays again")


# ---- 7. render_camera_denoised --------------------------------------------------------------------------------------------------
DENOISED = ("color", "variance", "albedo", "normal", "depth", "denoised")


@pytest.mark.parametrize("name", ["back", "staircase"])
def test_render_camera_denoised_with_the_handles_camera_is_render_denoised(name, renderer_factory):
    s = get_scene(name, W, H)
    r = renderer_factory(s)
    p = T.make_params(W, H, 8, SEEDS[name])
    want = r.render_denoised(p)
    got = r.render_camera_denoised(p, s.flat.contents.camera, samples_per_call=3)
    assert sorted(got) == sorted(want)
    for k in DENOISED:
        assert_bits(got[k], want[k], f"{name}: {k}")
    assert (got["denoised"] != got["color"]).any()
    assert got["stats"].rays_camera == want["stats"].rays_camera


def test_render_camera_denoised_with_a_moved_camera(renderer_factory):
    s = get_scene("back", W, H)
    r = renderer_factory(s)
    cam = moved_camera()
    p = T.make_params(W, H, 8, SEEDS["back"])
    out = r.render_camera_denoised(p, cam, aov_spp=4)
    assert_bits(out["color"], r.render_camera(p, cam, samples_per_call=8), "color vs render_camera")
    pix = tile_pixels(p)
    org, dirs = T.camera_rays(cam, p, pix, 0, 8)
    sums, sumsq, _ = r.render_rays(p, org, dirs, streams=pix)
    assert_bits(out["variance"], T.mean_luminance_variance(sums, sumsq, 8).reshape(H, W), "variance vs render_rays' moments")
    aov = r.render_camera_aov(T.make_params(W, H, 4, SEEDS["back"]), cam)
    for k in KEYS:
        assert_bits(out[k], aov[k], f"{k} vs render_camera_aov at aov_spp")
    assert_bits(out["denoised"], T.denoise(out["color"], out["variance"], out["albedo"], out["normal"], out["depth"]), "denoised vs trt_denoise of the buffers")
    with pytest.raises(T.TrtError, match="spp must be >= 2"):
        r.render_camera_denoised(T.make_params(W, H, 1, SEEDS["back"]), cam)
