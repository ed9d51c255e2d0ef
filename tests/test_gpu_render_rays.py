"""trt_render_rays / trt_render_rays_device, trt_camera_rays_device and Renderer.render_camera (full paths along caller-supplied rays) —
MI355X only.

Bars, all bit-exact:
  1. the built-in camera through the new entry: the rays of trt_camera_rays with stream = the tile's pixels leave trt_render_pixels' sum and
     sumsq, and (float)sum is trt_render's image — every scene kind and traversal kind; no tail, two passes in flight, several passes;
  2. a moved camera on a handle created with another one: the image is oracle_render's of the scene copy with that camera, a sparse list's
     moments are the oracle's per-sample radiance restated in float64, and Renderer.render_camera gives the same image;
  3. rays no pinhole produces (64 directions from a point inside the box, stream ids all over the 32 bits) against oracle_debug_path on a
     degenerate camera whose every pixel is that ray;
  4. the shapes where packing can go wrong, and invalid entries wherever a wave or a block can trip over them;
  5. the device entries, sumsq = NULL, resumption, the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd._abi import Camera, SceneFlat, c_float3

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 8
SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE, "lamps": T.SEED_LAMPS}


def scene(name):
    return get_scene("lamps", W, H, n=17) if name == "lamps" else get_scene(name, W, H)  # lamps: 18 lights (k_shade's SHADE_MANY)


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
    bad = a.view(np.uint64 if a.dtype == np.float64 else np.uint32) != b.view(np.uint64 if b.dtype == np.float64 else np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}: {a[tuple(np.argwhere(bad)[0])]} != {b[tuple(np.argwhere(bad)[0])]}"


def flat_with_camera(s, cam):
    """A copy of the flat scene description (the arrays stay s's) seen through `cam`."""
    f = SceneFlat.from_buffer_copy(s.flat.contents)
    f.camera = cam
    return f


def radiance(flat, p, x, y, k):
    """L of sample k of pixel (x, y) of image p.width x p.height: the oracle's path, vertex by vertex, and the radiance it ends with"""
    return O.debug_path(C.byref(flat), p, int(x), int(y), int(k), max_vertices=4096)[-1, 4:7].astype(np.float32)


def add_moments(su, sq, i, L, spp):
    v = (L / np.float32(spp)).astype(np.float64)
    su[i] += v
    sq[i] += v * v


def moved_camera():
    # the Cornell box of `back` from up and to the right of its own camera, turned towards the lower left, slightly rolled
    return T.look_at((420.0, 390.0, -650.0), (230.0, 200.0, 280.0), (0.08, 1.0, 0.02), 47.0, W, H)


# ---- 1. the built-in camera through the new entry --------------------------------------------------------------------------------
KINDS = {"default": {}, "wide4": {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, "oct8": {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}}
CASES1 = [(n, k, "plain") for n in ("back", "veach-mis", "staircase", "lamps") for k in KINDS] + [("veach-mis", "default", r) for r in ("no_tail", "overlap", "passes")]


@pytest.mark.parametrize("name,kind,run", CASES1, ids=["/".join(c) for c in CASES1])
def test_builtin_camera_rays_equal_render_pixels(name, kind, run, monkeypatch):
    s = scene(name)
    env = dict(KINDS[kind])
    if run == "no_tail":
        env["TRT_TAIL_N"] = "0"
    flags, budget = 0, 0
    if run == "overlap":
        flags = T.TRT_FLAG_OVERLAP
    if run == "passes":
        budget = W * H * 3 * (132 + 48 * s.info["n_lights"])  # three samples of every entry per pass: the footprint of trt_render_pixels
    p = T.make_params(W, H, SPP, SEEDS[name], flags=flags, mem_budget=budget)
    pix = tile_pixels(p)
    org, dirs = T.camera_rays(s.flat.contents.camera, p, pix, 0, SPP)
    r = fresh_renderer(s, env, monkeypatch)
    try:
        img, _ = r.render(p)
        want_s, want_q, st_ref = r.render_pixels(p, pix, 0, SPP)
        sums, sumsq, st = r.render_rays(p, org, dirs, streams=pix)
    finally:
        r.close()
    what = f"{name}/{kind}/{run}"
    assert_bits(sums, want_s, f"{what}: sum vs trt_render_pixels")
    assert_bits(sumsq, want_q, f"{what}: sumsq vs trt_render_pixels")
    assert_bits(sums.astype(np.float32).reshape(H, W, 3), img, f"{what}: (float)sum vs trt_render")
    assert (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits, st.max_bounces) == \
        (st_ref.rays_camera, st_ref.rays_shadow, st_ref.rays_indirect, st_ref.shaded_hits, st_ref.max_bounces)
    assert st.rays_camera == W * H * SPP and st.rows_rendered == 0
    assert st.passes == st_ref.passes
    assert st.launches[0] == st.passes and st_ref.launches[0] == 0  # TRT_K_GEN_PRIMARY: one packing launch per pass, here only
    if run == "passes":
        assert st.passes == 3
    if run == "no_tail":
        assert st.launches[T._abi.KERNEL_NAMES.index("tail")] == 0


# ---- 2. a moved camera on a resident handle -------------------------------------------------------------------------------------
def test_moved_camera_equals_the_oracle_on_the_scene_with_that_camera(renderer_factory):
    s = scene("back")
    r = renderer_factory(s)  # created with the scene's own camera
    cam = moved_camera()
    flat = flat_with_camera(s, cam)
    p = T.make_params(W, H, SPP, SEEDS["back"])
    pix = tile_pixels(p)
    org, dirs = T.camera_rays(cam, p, pix, 0, SPP)
    sums, _, st = r.render_rays(p, org, dirs, streams=pix)
    ref, ost = O.render(C.byref(flat), p)
    own, _ = r.render(p)
    assert (ref != own).any() and ref.any(), "the moved camera must see another image"
    assert_bits(sums.astype(np.float32).reshape(H, W, 3), ref, "moved camera: image vs oracle_render")
    assert (st.rays_camera, st.rays_shadow, st.rays_indirect) == (ost.rays_camera, ost.rays_shadow, ost.rays_indirect)
    # a sparse list, per sample, with the sums of squares
    sel = np.random.default_rng(21).permutation(pix)[:48]
    o2, d2 = T.camera_rays(cam, p, sel, 2, 7)
    got_s, got_q, _ = r.render_rays(p, o2, d2, streams=sel, sample_begin=2)
    want_s, want_q = np.zeros((len(sel), 3)), np.zeros((len(sel), 3))
    for i, q in enumerate(sel):
        for k in range(2, 7):
            add_moments(want_s, want_q, i, radiance(flat, p, q % W, q // W, k), SPP)
    assert_bits(got_s, want_s, "moved camera, sparse: sum")
    assert_bits(got_q, want_q, "moved camera, sparse: sumsq")


def test_render_camera_gives_the_moved_cameras_image(renderer_factory):
    """The device loop (rays generated and rendered on the device): three samples at a time (3 + 3 + 2), and one at a time."""
    s = scene("back")
    r = renderer_factory(s)
    cam = moved_camera()
    p = T.make_params(W, H, SPP, SEEDS["back"])
    ref, _ = O.render(C.byref(flat_with_camera(s, cam)), p)
    own, _ = r.render(p)
    assert_bits(r.render_camera(p, cam, samples_per_call=3), ref, "render_camera, 3 samples per call")
    img, st = r.render_camera(p, cam, want_stats=True)
    assert_bits(img, ref, "render_camera, 1 sample per call")
    assert st.rays_camera == W * H * SPP and st.passes == SPP
    dimg = r.render_camera(p, cam, samples_per_call=SPP, on_device=True)
    assert dimg.is_cuda
    assert_bits(dimg.cpu().numpy(), ref, "render_camera, on_device")
    # ... and the handle still renders its own camera
    assert_bits(r.render(p)[0], own, "trt_render after render_camera")


def test_render_camera_on_a_sub_tile_with_fixed_pixels(renderer_factory):
    s = scene("veach-mis")
    r = renderer_factory(s)
    c = s.flat.contents.camera
    eye = np.array(list(c.eye), np.float32)
    cam = Camera.from_buffer_copy(c)
    cam.eye = c_float3(*[float(x) for x in eye + np.array([1.5, 0.75, -2.0], np.float32)])
    p = T.make_params(W, H, SPP, SEEDS["veach-mis"], tile=(5, 3, 50, 31), rows=(2, 3, 1), flags=T.TRT_FLAG_FIXED_PIXELS | T.TRT_FLAG_FIXED_NEE)
    ref, _ = O.render(C.byref(flat_with_camera(s, cam)), p)
    assert_bits(r.render_camera(p, cam, samples_per_call=5), ref, "render_camera on an interleaved sub-tile")


# ---- 3. rays no pinhole produces ------------------------------------------------------------------------------------------------
def sphere_directions(n, rng):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)


def ray_camera(eye, d):
    """A camera whose EVERY pixel is the ray (eye, normalize((eye + d) - eye)): no extent, the corner one direction away from the eye."""
    cam = Camera()
    cam.eye = c_float3(*[float(x) for x in eye])
    cam.lower_left_corner = c_float3(*[float(x) for x in (eye + d).astype(np.float32)])
    cam.horizontal = c_float3(0.0, 0.0, 0.0)
    cam.vertical = c_float3(0.0, 0.0, 0.0)
    return cam


@pytest.mark.parametrize("flags", [0, T.TRT_FLAG_FIXED_NEE | T.TRT_FLAG_RAY_OFFSET], ids=["parity", "fixed_nee+ray_offset"])
def test_rays_from_inside_the_box_match_the_oracle(flags, renderer_factory):
    s = scene("back")
    r = renderer_factory(s)
    rng = np.random.default_rng(33)
    n, s0, s1 = 64, 3, 6
    eye = np.array([278.0, 400.0, 150.0], np.float32)  # inside the Cornell box, above the cube
    ds = sphere_directions(n, rng)
    # stream ids of the test's choice, all over the 32 bits.  The oracle keys a path by y * width + x: a 65536 x 65536 image reaches every id
    # with x = id & 0xFFFF, y = id >> 16, so no id needs replacing.
    ids = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ids[:4] = [0, 1, 0x80000000, 0xFFFFFFFF]
    big = T.make_params(65536, 65536, SPP, SEEDS["back"], flags=flags)
    p = T.make_params(W, H, SPP, SEEDS["back"], flags=flags)  # width and height mean nothing to trt_render_rays
    org = np.empty((s1 - s0, n, 3), np.float32)
    dirs = np.empty_like(org)
    want_s, want_q = np.zeros((n, 3)), np.zeros((n, 3))
    L = O.lib()
    for i in range(n):
        cam = ray_camera(eye, ds[i])
        o, d = T.camera_rays(cam, big, [ids[i]], s0, s1)
        org[:, i], dirs[:, i] = o[:, 0], d[:, 0]
        x, y = int(ids[i]) & 0xFFFF, int(ids[i]) >> 16
        flat = flat_with_camera(s, cam)
        for k in range(s0, s1):
            # the terms on the CPU first: the oracle's camera gives this very ray for this pixel and sample
            u1, u2 = L.oracle_prims_uniform(big.seed, int(ids[i]), k, 0), L.oracle_prims_uniform(big.seed, int(ids[i]), k, 1)
            oo, od = O.camera_ray(cam, 65536, 65536, y, x, u1, u2)
            assert (oo.view(np.uint32) == org[k - s0, i].view(np.uint32)).all() and (od.view(np.uint32) == dirs[k - s0, i].view(np.uint32)).all()
            add_moments(want_s, want_q, i, radiance(flat, big, x, y, k), SPP)
    assert np.allclose(np.linalg.norm(dirs, axis=2), 1.0, atol=1e-6) and np.abs(dirs[0] - ds).max() < 1e-4
    sums, sumsq, st = r.render_rays(p, org, dirs, streams=ids, sample_begin=s0)
    assert want_s.any()
    assert_bits(sums, want_s, "sphere rays: sum")
    assert_bits(sumsq, want_q, "sphere rays: sumsq")
    assert st.rays_camera == n * (s1 - s0)


# ---- 4. shapes where packing can go wrong ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 2305])
def test_list_lengths_one_sample_and_default_stream_ids(n, renderer_factory):
    """n = 1, under and over a wave, and ten blocks of the packing kernel with one entry in the last; one sample with sample_begin > 0."""
    s = scene("back")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["back"])
    pix = (np.arange(n) % (W * H)).astype(np.uint32)
    cam = s.flat.contents.camera
    org, dirs = T.camera_rays(cam, p, pix, 5, 6)
    want_s, want_q, _ = r.render_pixels(p, pix, 5, 6)
    sums, sumsq, st = r.render_rays(p, org, dirs, streams=pix, sample_begin=5)
    assert want_s.any() or n == 1
    assert_bits(sums, want_s, f"n = {n}: sum")
    assert_bits(sumsq, want_q, f"n = {n}: sumsq")
    assert st.rays_camera == n and st.passes == 1
    # stream = NULL is stream[i] = i
    ids = np.arange(n, dtype=np.uint32)
    a_s, a_q, _ = r.render_rays(p, org, dirs, streams=ids, sample_begin=5)
    b_s, b_q, _ = r.render_rays(p, org, dirs, streams=None, sample_begin=5)
    assert_bits(b_s, a_s, f"n = {n}: stream = NULL, sum")
    assert_bits(b_q, a_q, f"n = {n}: stream = NULL, sumsq")
    if n <= W * H:  # there i is the pixel itself
        assert_bits(b_s, want_s, f"n = {n}: stream = NULL vs trt_render_pixels")


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


@pytest.mark.parametrize("overlap", [False, True], ids=["one_pass", "two_passes_in_flight"])
def test_invalid_entries_do_not_disturb_the_others(overlap, renderer_factory):
    s = scene("veach-mis")
    r = renderer_factory(s)
    n = 2305
    p = T.make_params(W, H, SPP, SEEDS["veach-mis"], flags=T.TRT_FLAG_OVERLAP if overlap else 0)
    pix = (np.arange(n) % (W * H)).astype(np.uint32)
    rng = np.random.default_rng(44)
    org, dirs = T.camera_rays(s.flat.contents.camera, p, pix, 5, 7)
    # lane 0, lane 63, across a wave boundary, across a block boundary of the packing kernel, a whole wave, the last entry;
    # sample 6 also loses a whole block, and gets entry 0 back
    bad = [np.r_[0, 63, 127, 128, 255, 256, 320:384, n - 1], np.r_[63, 127, 128, 255, 256, 320:384, 512:768, n - 1]]
    dirty_o, dirty_d = org.copy(), dirs.copy()
    for k in range(2):
        for j, idx in enumerate(bad[k]):
            poison(dirty_o[k], dirty_d[k], idx, j + k)
    s_in, q_in = rng.uniform(0.5, 2.0, (n, 3)), rng.uniform(0.5, 2.0, (n, 3))  # the sums are in/out
    clean_s, clean_q, clean_st = r.render_rays(p, org, dirs, streams=pix, sample_begin=5, sums=s_in.copy(), sumsq=q_in.copy())
    only6_s, only6_q, _ = r.render_rays(p, org[1:], dirs[1:], streams=pix, sample_begin=6, sums=s_in.copy(), sumsq=q_in.copy())
    got_s, got_q, st = r.render_rays(p, dirty_o, dirty_d, streams=pix, sample_begin=5, sums=s_in.copy(), sumsq=q_in.copy())
    never = np.intersect1d(bad[0], bad[1])
    once0 = np.setdiff1d(bad[0], bad[1])   # invalid in sample 5 only: what sample 6 alone leaves
    once1 = np.setdiff1d(bad[1], bad[0])
    valid = np.setdiff1d(np.arange(n), np.union1d(bad[0], bad[1]))
    assert len(once0) == 1 and len(once1) == 256 and len(never) == 70
    assert_bits(got_s[valid], clean_s[valid], "valid entries: sum")
    assert_bits(got_q[valid], clean_q[valid], "valid entries: sumsq")
    assert_bits(got_s[never], s_in[never], "invalid entries: sum left as given")
    assert_bits(got_q[never], q_in[never], "invalid entries: sumsq left as given")
    assert_bits(got_s[once0], only6_s[once0], "invalid in the first sample only: sum")
    assert_bits(got_q[once0], only6_q[once0], "invalid in the first sample only: sumsq")
    first5_s, first5_q, _ = r.render_rays(p, org[:1], dirs[:1], streams=pix, sample_begin=5, sums=s_in.copy(), sumsq=q_in.copy())
    assert_bits(got_s[once1], first5_s[once1], "invalid in the second sample only: sum")
    assert_bits(got_q[once1], first5_q[once1], "invalid in the second sample only: sumsq")
    assert clean_st.rays_camera == 2 * n
    assert st.rays_camera == 2 * n - len(bad[0]) - len(bad[1])
    assert st.passes == (2 if overlap else 1)


def test_nothing_valid_and_odd_directions(renderer_factory):
    s = scene("back")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["back"])
    n = 65
    org = np.tile(np.array([278.0, 400.0, 150.0], np.float32), (2, n, 1))
    dirs = np.zeros((2, n, 3), np.float32)
    dirs[1, ::2, 0] = np.float32("nan")
    s_in = np.random.default_rng(5).uniform(0.5, 2.0, (n, 3))
    got_s, got_q, st = r.render_rays(p, org, dirs, sums=s_in.copy(), sumsq=s_in.copy())
    assert_bits(got_s, s_in, "no valid entry: sum")
    assert_bits(got_q, s_in, "no valid entry: sumsq")
    assert st.rays_camera == 0 and st.rays_shadow == 0 and st.rays_indirect == 0 and st.passes == 1
    # non-unit and axis-aligned directions are not errors
    dirs = np.array([[5, 0, 0], [0, -2, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 0], [0, 1, 0], [0.001, 0.002, -0.0005], [300, -200, 100]], np.float32)[None]
    got_s, got_q, st = r.render_rays(p, org[:1, :8], dirs)
    assert st.rays_camera == 8 and np.isfinite(got_s).all() and np.isfinite(got_q).all()
    unit = [2, 3, 4, 5]  # the unit ones have the oracle's radiance
    for i in unit:
        cam = ray_camera(org[0, i], dirs[0, i])
        o, d = T.camera_rays(cam, p, [i], 0, 1)
        assert (d[0, 0] == dirs[0, i]).all()
        want_s, want_q = np.zeros((1, 3)), np.zeros((1, 3))
        add_moments(want_s, want_q, 0, radiance(flat_with_camera(s, cam), p, i % W, i // W, 0), SPP)
        assert_bits(got_s[i:i + 1], want_s, f"axis-aligned direction {i}")


# ---- 5. other behaviour ---------------------------------------------------------------------------------------------------------
def test_device_entries_match_host_entries(renderer_factory):
    import torch
    s = scene("lamps")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["lamps"], flags=T.TRT_FLAG_OVERLAP)
    cam = moved_camera()
    pix = np.random.default_rng(9).choice(np.arange(W * H, dtype=np.uint32), 611, replace=True).astype(np.uint32)
    n = len(pix)
    org, dirs = T.camera_rays(cam, p, pix, 0, 5)
    h_s, h_q, h_st = r.render_rays(p, org, dirs, streams=pix)
    dev = torch.device("cuda", 0)
    t_pix = torch.from_numpy(pix.astype(np.int32)).to(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        t_org = torch.empty((5, n, 3), dtype=torch.float32, device=dev)
        t_dir = torch.empty_like(t_org)
        T.camera_rays_into(cam, p, t_pix, 0, 5, t_org, t_dir, device=0, stream_ptr=side.cuda_stream)
        d_s = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        d_q = torch.zeros_like(d_s)
        d_st = r.render_rays_into(p, t_org, t_dir, d_s, d_q, streams=t_pix, stream_ptr=side.cuda_stream)
    assert_bits(t_org.cpu().numpy(), org, "device camera rays: org")
    assert_bits(t_dir.cpu().numpy(), dirs, "device camera rays: dir")
    assert_bits(d_s.cpu().numpy(), h_s, "device sum")
    assert_bits(d_q.cpu().numpy(), h_q, "device sumsq")
    assert (d_st.rays_camera, d_st.rays_shadow, d_st.rays_indirect) == (h_st.rays_camera, h_st.rays_shadow, h_st.rays_indirect)
    # in/out on the device: resume from the host's sums; no stream ids: 0..n-1
    o2, d2 = T.camera_rays(cam, p, pix, 5, 8)
    r.render_rays_into(p, torch.from_numpy(o2).to(dev), torch.from_numpy(d2).to(dev), d_s, d_q, streams=t_pix, sample_begin=5)
    f_o, f_d = T.camera_rays(cam, p, pix, 0, 8)
    f_s, f_q, _ = r.render_rays(p, f_o, f_d, streams=pix)
    assert_bits(d_s.cpu().numpy(), f_s, "device resume sum")
    assert_bits(d_q.cpu().numpy(), f_q, "device resume sumsq")
    e_s = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    r.render_rays_into(p, t_org, t_dir, e_s)  # sumsq and streams left out
    g_s, _, _ = r.render_rays(p, org, dirs)
    assert_bits(e_s.cpu().numpy(), g_s, "device, stream = NULL, sumsq = NULL")
    # wrong tensors are refused in Python; a pixel outside the image by the kernel
    with pytest.raises(T.TrtError, match="contiguous"):
        r.render_rays_into(p, t_org.transpose(0, 1), t_dir, e_s)
    with pytest.raises(T.TrtError, match="float64"):
        r.render_rays_into(p, t_org, t_dir, e_s.to(torch.float32))
    t_bad = t_pix.clone()
    t_bad[300] = W * H
    with pytest.raises(T.TrtError, match=r"\(1\).*width \* height"):
        T.camera_rays_into(cam, p, t_bad, 0, 5, t_org, t_dir)


def test_sumsq_may_be_null_and_resumption(renderer_factory):
    s = scene("staircase")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["staircase"])
    pix = np.random.default_rng(5).permutation(np.arange(W * H, dtype=np.uint32))[:300]
    org, dirs = T.camera_rays(moved_camera_of(s), p, pix, 0, 13)
    a_s, a_q, _ = r.render_rays(p, org[:8], dirs[:8], streams=pix)
    b_s, b_q, _ = r.render_rays(p, org[:3], dirs[:3], streams=pix)
    b_s, b_q, _ = r.render_rays(p, org[3:8], dirs[3:8], streams=pix, sample_begin=3, sums=b_s, sumsq=b_q)
    assert_bits(b_s, a_s, "[0,3) + [3,8) vs [0,8): sum")
    assert_bits(b_q, a_q, "[0,3) + [3,8) vs [0,8): sumsq")
    # sample_end past p.spp: p.spp only scales the terms
    c_s, c_q, _ = r.render_rays(p, org[8:], dirs[8:], streams=pix, sample_begin=8, sums=a_s.copy(), sumsq=a_q.copy())
    flat = flat_with_camera(s, moved_camera_of(s))
    want_s, want_q = a_s.copy(), a_q.copy()
    for i, q in enumerate(pix[:24]):
        for k in range(8, 13):
            add_moments(want_s, want_q, i, radiance(flat, p, q % W, q // W, k), SPP)
    assert_bits(c_s[:24], want_s[:24], "past spp: sum")
    assert_bits(c_q[:24], want_q[:24], "past spp: sumsq")
    su = np.zeros((len(pix), 3))
    st = T.Stats()
    fp = C.POINTER(C.c_float)
    rc = r._lib.trt_render_rays(r._h, C.byref(p), len(pix), org.ctypes.data_as(fp), dirs.ctypes.data_as(fp), pix.ctypes.data_as(C.POINTER(C.c_uint32)), 0, 8,
                                su.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(st))
    assert rc == 0
    assert_bits(su, a_s, "sum without sumsq")


def moved_camera_of(s):
    """The scene's own camera, two units to the right and one up"""
    c = s.flat.contents.camera
    cam = Camera.from_buffer_copy(c)
    h = np.array(list(c.horizontal), np.float32)
    v = np.array(list(c.vertical), np.float32)
    shift = (h / np.linalg.norm(h) * 2.0 + v / np.linalg.norm(v)).astype(np.float32)
    cam.eye = c_float3(*[float(x) for x in np.array(list(c.eye), np.float32) + shift])
    cam.lower_left_corner = c_float3(*[float(x) for x in np.array(list(c.lower_left_corner), np.float32) + shift])
    return cam


def test_refusals_leave_the_handle_usable(renderer_factory):
    s = scene("back")
    r = renderer_factory(s)
    lib = r._lib
    p = T.make_params(W, H, SPP, SEEDS["back"])
    pix = np.random.default_rng(1).permutation(np.arange(W * H, dtype=np.uint32))[:50]
    org, dirs = T.camera_rays(s.flat.contents.camera, p, pix, 0, 4)
    su, sq = np.zeros((50, 3)), np.zeros((50, 3))
    fp, dp, up = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    o_p, d_p, s_p, q_p, i_p = org.ctypes.data_as(fp), dirs.ctypes.data_as(fp), su.ctypes.data_as(dp), sq.ctypes.data_as(dp), pix.ctypes.data_as(up)
    st = T.Stats()

    def call(n, o, d, b, e, sums, sumsq, params=p, handle=r._h):
        return lib.trt_render_rays(handle, None if params is None else C.byref(params), n, o, d, i_p, b, e, sums, sumsq, C.byref(st))

    no_spp = T.make_params(W, H, 0, SEEDS["back"])
    refusals = {
        "null handle": call(50, o_p, d_p, 0, 2, s_p, q_p, handle=None),
        "null params": call(50, o_p, d_p, 0, 2, s_p, q_p, params=None),
        "null org": call(50, None, d_p, 0, 2, s_p, q_p),
        "null dir": call(50, o_p, None, 0, 2, s_p, q_p),
        "null sums": call(50, o_p, d_p, 0, 2, None, q_p),
        "begin < 0": call(50, o_p, d_p, -1, 2, s_p, q_p),
        "begin > end": call(50, o_p, d_p, 3, 2, s_p, q_p),
        "spp < 1": call(50, o_p, d_p, 0, 2, s_p, q_p, params=no_spp),
        # checked before an array is read or any memory is sized by it
        "path-id range": call(0x7FFF0001, o_p, d_p, 0, 1, s_p, q_p),
    }
    for what, rc in refusals.items():
        assert rc == 1, f"{what}: returned {rc}, not TRT_EINVAL"
    assert not su.any() and not sq.any(), "a refused call wrote the sums"
    # no-ops: nothing listed, or an empty range
    assert call(0, None, None, 0, 4, None, None) == 0
    assert call(50, o_p, d_p, 3, 3, s_p, q_p) == 0 and not su.any()
    # the budget cannot hold one sample of every entry
    tight = T.make_params(W, H, SPP, SEEDS["back"], mem_budget=49 * 180)
    assert call(50, o_p, d_p, 0, 2, s_p, q_p, params=tight) == 3
    # a size the built-in camera refuses means nothing here
    odd = T.make_params(W, H, SPP, SEEDS["back"])
    odd.width, odd.height, odd.x1, odd.y1 = 0, -3, 0, 0
    assert call(50, o_p, d_p, 0, 4, s_p, q_p, params=odd) == 0
    # still renders right: the new entry, and the built-in camera
    want_s, want_q, _ = r.render_pixels(p, pix, 0, 4)
    assert_bits(su, want_s, "ignored width / height: sum")
    sums, sumsq, _ = r.render_rays(p, org, dirs, streams=pix)
    assert_bits(sums, want_s, "after refusals: sum")
    assert_bits(sumsq, want_q, "after refusals: sumsq")
    img, _ = r.render(p)
    ref, _ = O.render(s.flat, p)
    assert_bits(img, ref, "after refusals: trt_render")
