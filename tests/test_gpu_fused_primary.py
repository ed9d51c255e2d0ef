"""Bounce 0 in one kernel (trt_kernels.h: k_shade's FUSE flavour walks the camera rays itself, no hit record is written or read) against the
two kernels TRT_FUSE_PRIMARY=0 keeps, and against the CPU oracle — MI355X only.

The fused walk folds the same candidates in the same order, so every image and counter must come out bit-identical with the switch on
and off, and equal to the oracle's.  Which route ran is read from the TRT_DEBUG lines (trt_create: fused primary ...; trt_render: fused
primary ...) and asserted first.

Everything here is the Cornell box (`back`, `lamps`), which has no two triangles at one distance and one or two candidates per wave: geometry on which
the walk's tie rule, its size limits and hostile cameras decide the picture is in tests/test_gpu_tiny_cases.py (the corpus of tests/tiny_cases.py).
"""
import ctypes as C
import re

import numpy as np
import pytest

import oracle_lib as O
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd import dist as D
from tinyraytracing_amd._abi import Camera, SceneFlat, c_float3

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "max_bounces", "redo_rays")
ORACLE_FIELDS = STAT_FIELDS[:5]
BYTES_PER_PATH = 132 + 48  # arena bytes of one path of a one-light render (SlotLayout)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


class WithCamera:
    """`scene` seen through another camera: a copy of its flat description (the arrays stay the scene's)."""

    def __init__(self, scene, cam):
        self._scene = scene
        self._flat = SceneFlat.from_buffer_copy(scene.flat.contents)
        self._flat.camera = cam
        self.flat = C.pointer(self._flat)
        self.info = scene.info


def handle(s, fused, capfd, monkeypatch, env=None, want=None):
    """A Renderer created with TRT_FUSE_PRIMARY set; `want`: what trt_create must report (default: the switch)."""
    env = dict(env or {}, TRT_DEBUG="1", TRT_FUSE_PRIMARY="1" if fused else "0")
    capfd.readouterr()
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        r = T.Renderer(s, 0)
    got = re.findall(r"trt_create: fused primary (\d)", capfd.readouterr().err)
    assert got == ["1" if (fused if want is None else want) else "0"], got
    return r


def routes(capfd, entry="trt_render"):
    """The route of every render call since the last look: 1 = bounce 0 ran fused"""
    return [int(x) for x in re.findall(entry + r": fused primary (\d)", capfd.readouterr().err)]


def render_both(s, p, capfd, monkeypatch, env=None, want_fused=True):
    """(image, Stats) of p with the switch on and off, the route of each asserted"""
    out = []
    for fused in (True, False):
        r = handle(s, fused, capfd, monkeypatch, env)
        try:
            out.append(r.render(p))
            assert routes(capfd) == [1 if (fused and want_fused) else 0]
        finally:
            r.close()
    return out


def check_threefold(s, p, capfd, monkeypatch, env=None):
    (img_f, st_f), (img_u, st_u) = render_both(s, p, capfd, monkeypatch, env)
    assert np.array_equal(bits(img_f), bits(img_u)), "the fused and the two-kernel bounce 0 differ"
    assert [getattr(st_f, f) for f in STAT_FIELDS] == [getattr(st_u, f) for f in STAT_FIELDS]
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(bits(img_f), bits(ref)), f"max abs diff to the oracle {float(np.abs(img_f - ref).max())}"
    assert [getattr(st_f, f) for f in ORACLE_FIELDS] == [getattr(ost, f) for f in ORACLE_FIELDS]
    return st_f


PLAIN = [(128, 128, 16, 0, {}), (96, 64, 16, T.TRT_FLAG_FIXED_NEE, {}), (96, 64, 16, T.TRT_FLAG_FIXED_PIXELS, {}), (96, 64, 16, T.TRT_FLAG_RAY_OFFSET, {}),
         (96, 64, 16, 0, {"TRT_TAIL_N": "64"})]  # the last one: queue bounces (binned walk, k_shade on 8-byte records) behind the fused bounce 0


@pytest.mark.parametrize("case", PLAIN, ids=[f"{c[0]}x{c[1]}x{c[2]}-f{c[3]}" + ("-queue" if c[4] else "") for c in PLAIN])
def test_plain_renders(case, capfd, monkeypatch):
    w, h, spp, flags, env = case
    st = check_threefold(get_scene("back", w, h), T.make_params(w, h, spp, 0xF7 + spp + flags, flags=flags), capfd, monkeypatch, env)
    assert st.rays_camera == w * h * spp and st.shaded_hits > 0 and st.rays_shadow > 0 and st.rays_indirect > 0


@pytest.mark.parametrize("w,h,spp", [(7, 5, 3), (33, 17, 1), (64, 64, 1)], ids=["105-paths", "561-paths", "4096-paths"])
def test_tile_edges(w, h, spp, capfd, monkeypatch):
    """Less than one 512-path tile, one tile and a remainder (its last wave holds one path), whole tiles only"""
    check_threefold(get_scene("back", w, h), T.make_params(w, h, spp, 0x7E + w), capfd, monkeypatch)


def test_row_subset_of_a_rank(capfd, monkeypatch):
    """The rows dist.shard_params deals to rank 1 of 3: the row table is not the identity"""
    w, h = 48, 40
    p = D.shard_params(w, h, 4, 0x5A, 1, 3)
    rows = T.rows_selected(p)
    assert 0 < len(rows) < h and rows[0] != 0
    check_threefold(get_scene("back", w, h), p, capfd, monkeypatch)


@pytest.mark.parametrize("overlap", [False, True], ids=["passes", "overlap"])
def test_several_passes(overlap, capfd, monkeypatch):
    """A small mem_budget: four passes of two samples; with TRT_FLAG_OVERLAP two of them in flight"""
    w, h, spp = 64, 48, 8
    slots = 2 if overlap else 1
    p = T.make_params(w, h, spp, 0xBEE, flags=T.TRT_FLAG_OVERLAP if overlap else 0, mem_budget=slots * 2 * w * h * BYTES_PER_PATH)
    st = check_threefold(get_scene("back", w, h), p, capfd, monkeypatch)
    assert st.passes == 4


def back_with(cam, w, h):
    return WithCamera(get_scene("back", w, h), cam)


def test_camera_that_sees_nothing(capfd, monkeypatch):
    w, h = 40, 24
    c = get_scene("back", w, h).flat.contents.camera
    eye, llc = np.array(list(c.eye), np.float32), np.array(list(c.lower_left_corner), np.float32)
    cam = Camera.from_buffer_copy(c)
    cam.lower_left_corner = c_float3(*[float(x) for x in (eye - (llc - eye))])  # turned round: the box lies behind it
    cam.horizontal = c_float3(*[-float(x) for x in c.horizontal])
    cam.vertical = c_float3(*[-float(x) for x in c.vertical])
    st = check_threefold(back_with(cam, w, h), T.make_params(w, h, 4, 0xA11), capfd, monkeypatch)
    assert (st.shaded_hits, st.rays_shadow, st.rays_indirect) == (0, 0, 0)


def test_light_seen_directly(capfd, monkeypatch):
    """From a corner of the floor, looking up at the ceiling light: the camera rays in the middle of the image end on the emitter (shadeBegin's bounce-0
    emissive branch), the others on the ceiling and the walls"""
    w, h = 40, 24
    cam = T.look_at((200.0, 60.0, 60.0), (278.0, 548.0, 279.5), (0.0, 0.0, 1.0), 40.0, w, h)
    s = back_with(cam, w, h)
    p = T.make_params(w, h, 4, 0x116)
    st = check_threefold(s, p, capfd, monkeypatch)
    assert st.shaded_hits > 0
    ref, _ = O.render(s.flat, p)
    assert int((ref.max(axis=2) > 30.0).sum()) >= 16  # the light's own radiance (34, 24, 8) where it is seen directly


def test_zero_x_component_everywhere(capfd, monkeypatch):
    """`horizontal` is the zero vector and lower_left_corner.x == eye.x: every camera ray has d.x == 0 and takes the literal slab test — whole waves of them,
    and with 16 blocks for the 10240 camera rays (TRT_TRACE_FILLB) 160 per wave of the camera kernel, more than the 128 it parks"""
    w, h, spp = 32, 20, 16
    c = get_scene("back", w, h).flat.contents.camera
    cam = Camera.from_buffer_copy(c)
    cam.horizontal = c_float3(0.0, 0.0, 0.0)
    cam.lower_left_corner = c_float3(float(c.eye[0]), float(c.lower_left_corner[1]), float(c.lower_left_corner[2]))
    assert float(c.vertical[0]) == 0.0
    s = back_with(cam, w, h)
    p = T.make_params(w, h, spp, 0x0E0)
    org, dirs = T.camera_rays(cam, p, np.arange(w * h, dtype=np.uint32), 0, spp)
    assert not dirs[..., 0].any()
    st = check_threefold(s, p, capfd, monkeypatch, {"TRT_TRACE_FILLB": "8"})
    assert st.redo_rays >= st.rays_camera == w * h * spp and st.shaded_hits > 0


def test_which_route_ran(capfd, monkeypatch):
    """TRT_FLAG_TIMING runs the fused route and books it under `shade`: one closest-hit launch fewer than shade launches; TRT_FLAG_COUNT keeps the two kernels,
    and their counters are the oracle's"""
    w, h, spp = 64, 48, 4
    s = get_scene("back", w, h)
    k_closest, k_shade = T.KERNEL_NAMES.index("trace_closest"), T.KERNEL_NAMES.index("shade")
    p = T.make_params(w, h, spp, 0x71, flags=T.TRT_FLAG_TIMING)
    (img_f, st_f), (img_u, st_u) = render_both(s, p, capfd, monkeypatch, {"TRT_TAIL_N": "64"})
    assert st_f.launches[k_shade] > 2 and st_f.launches[k_shade] == st_u.launches[k_shade]
    assert st_f.launches[k_closest] == st_f.launches[k_shade] - 1
    assert st_u.launches[k_closest] == st_u.launches[k_shade]
    assert np.array_equal(bits(img_f), bits(img_u))
    pc = T.make_params(w, h, spp, 0x71, flags=T.TRT_FLAG_COUNT)
    (img_c, st_c), (img_d, st_d) = render_both(s, pc, capfd, monkeypatch, want_fused=False)
    ref, ost = O.render(s.flat, pc)
    for img, st in ((img_c, st_c), (img_d, st_d)):
        assert np.array_equal(bits(img), bits(ref)) and np.array_equal(bits(img), bits(img_f))
        assert list(st.inner_visits) == list(ost.inner_visits) and list(st.tri_tests) == list(ost.tri_tests)
        assert [getattr(st, f) for f in ORACLE_FIELDS] == [getattr(ost, f) for f in ORACLE_FIELDS]


@pytest.mark.parametrize("name,lamps", [("lamps", 2), ("veach-mis", None)], ids=["three-lights", "veach-mis"])
def test_scenes_that_must_not_fuse(name, lamps, capfd, monkeypatch):
    w, h = 64, 36
    s = get_scene(name, w, h, n=lamps) if lamps else get_scene(name, w, h)
    assert s.info["n_lights"] > 1
    p = T.make_params(w, h, 4, 0x2F)
    r = handle(s, True, capfd, monkeypatch, want=False)
    try:
        img, st = r.render(p)
        assert routes(capfd) == [0]
    finally:
        r.close()
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(bits(img), bits(ref))
    assert [getattr(st, f) for f in ORACLE_FIELDS] == [getattr(ost, f) for f in ORACLE_FIELDS]


def test_calls_that_must_not_fuse(capfd, monkeypatch):
    """A pixel list and caller-supplied rays (render_camera) on a handle that fuses its tile renders: both keep the two kernels and return what they returned"""
    w, h, spp = 48, 30, 4
    s = get_scene("back", w, h)
    p = T.make_params(w, h, spp, 0xCA11)
    pix = np.arange(w * h, dtype=np.uint32)[::-1].copy()
    got = []
    for fused in (True, False):
        r = handle(s, fused, capfd, monkeypatch)
        try:
            img, _ = r.render(p)
            assert routes(capfd) == [1 if fused else 0]
            sums, sumsq, st = r.render_pixels(p, pix, 0, spp)
            assert routes(capfd, "trt_render_pixels") == [0]
            cam_img, cst = r.render_camera(p, s.flat.contents.camera, samples_per_call=2, want_stats=True)
            assert routes(capfd, "trt_render_rays") == [0, 0]
            got.append((img, sums, sumsq, [getattr(st, f) for f in STAT_FIELDS], cam_img, [getattr(cst, f) for f in STAT_FIELDS]))
        finally:
            r.close()
    a, b = got
    for x, y in zip(a, b):
        assert (np.array_equal(bits(x), bits(y)) if isinstance(x, np.ndarray) else x == y)
    assert np.array_equal(bits(a[4]), bits(a[0]))  # render_camera's contract: the image of a handle created with that camera
