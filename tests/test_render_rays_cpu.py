"""The host side of trt_render_rays (include/trt.h) — no GPU needed.

  - trt_camera_rays against the oracle's Camera::getRay (oracle_camera_ray_mode) fed with the stream's draws 0 and 1, bit for bit;
  - the per-ray functions k_rays_pack wraps, compiled for the host (tests/render_rays/librays_cpu.so): rayRecord writes cameraRecord's bits,
    and the validity predicate;
  - the new symbols in the header and the ctypes mirror, ABI version unchanged; look_at.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0007


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def some_camera():
    return T.look_at((278.0, 273.0, -800.0), (270.0, 260.0, 0.0), (0.1, 1.0, 0.0), 39.3, 64, 36)


def oracle_rays(cam, p, pixels, s0, s1):
    fixed = bool(p.flags & T.TRT_FLAG_FIXED_PIXELS)
    org = np.empty((s1 - s0, len(pixels), 3), np.float32)
    dirs = np.empty_like(org)
    L = O.lib()
    for s in range(s0, s1):
        for i, q in enumerate(pixels):
            u1, u2 = L.oracle_prims_uniform(p.seed, int(q), s, 0), L.oracle_prims_uniform(p.seed, int(q), s, 1)
            org[s - s0, i], dirs[s - s0, i] = O.camera_ray(cam, p.width, p.height, int(q) // p.width, int(q) % p.width, u1, u2, fixed=fixed)
    return org, dirs


# sizes: the smallest images, the suite's 64 x 36 (every pixel), and an image wider than 65536 (outside the range of the reciprocal pixel grid)
CASES = {
    "1x1": (1, 1, [0]),
    "2x2": (2, 2, [0, 1, 2, 3, 3, 0]),
    "64x36": (64, 36, list(range(64 * 36))),
    "65537x3": (65537, 3, [0, 1, 65536, 65537, 2 * 65537 + 12345, 3 * 65537 - 1]),
}


@pytest.mark.parametrize("fixed", [False, True], ids=["parity", "fixed_pixels"])
@pytest.mark.parametrize("case", list(CASES))
def test_camera_rays_are_the_oracles_camera_rays(case, fixed):
    w, h, pixels = CASES[case]
    p = T.make_params(w, h, 8, SEED, flags=T.TRT_FLAG_FIXED_PIXELS if fixed else 0)
    cam = some_camera()
    s0, s1 = (3, 5) if len(pixels) > 100 else (2, 7)  # ranges that do not start at 0
    org, dirs = T.camera_rays(cam, p, pixels, s0, s1)
    want_o, want_d = oracle_rays(cam, p, pixels, s0, s1)
    assert org.shape == (s1 - s0, len(pixels), 3)
    assert (bits(org) == bits(want_o)).all()
    bad = bits(dirs) != bits(want_d)
    assert not bad.any(), f"{int(bad.sum())} direction words differ, first at {np.argwhere(bad)[0]}"
    if case == "64x36":
        assert np.isfinite(dirs).all() and np.allclose(np.linalg.norm(dirs, axis=2), 1.0, atol=1e-6)


def test_camera_rays_range_and_refusals():
    p = T.make_params(64, 36, 8, SEED)
    cam = some_camera()
    pixels = np.array([5, 64 * 36 - 1, 700], np.uint32)
    a_o, a_d = T.camera_rays(cam, p, pixels, 0, 6)
    b_o, b_d = T.camera_rays(cam, p, pixels, 4, 6)
    assert (bits(a_o[4:]) == bits(b_o)).all() and (bits(a_d[4:]) == bits(b_d)).all()
    e_o, e_d = T.camera_rays(cam, p, pixels, 3, 3)
    assert e_o.shape == (0, 3, 3)
    lib = _abi.load_hip()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    out_o, out_d = np.full((2, 3, 3), 7.0, np.float32), np.full((2, 3, 3), 7.0, np.float32)

    def call(cam_p, par, n, pix, b, e):
        return lib.trt_camera_rays(cam_p, par, n, pix, b, e, out_o.ctypes.data_as(fp), out_d.ctypes.data_as(fp))

    bad = pixels.copy()
    bad[2] = 64 * 36
    small = T.make_params(64, 36, 8, SEED)
    small.height = 0
    refusals = {
        "pixel >= width*height": call(C.byref(cam), C.byref(p), 3, bad.ctypes.data_as(up), 0, 2),
        "null camera": call(None, C.byref(p), 3, pixels.ctypes.data_as(up), 0, 2),
        "null params": call(C.byref(cam), None, 3, pixels.ctypes.data_as(up), 0, 2),
        "null pixels": call(C.byref(cam), C.byref(p), 3, None, 0, 2),
        "begin < 0": call(C.byref(cam), C.byref(p), 3, pixels.ctypes.data_as(up), -1, 2),
        "begin > end": call(C.byref(cam), C.byref(p), 3, pixels.ctypes.data_as(up), 3, 2),
        "height < 1": call(C.byref(cam), C.byref(small), 3, pixels.ctypes.data_as(up), 0, 2),
    }
    for what, rc in refusals.items():
        assert rc == 1, f"{what}: returned {rc}, not TRT_EINVAL"
    assert (out_o == 7.0).all() and (out_d == 7.0).all(), "a refused call wrote the rays"
    assert call(C.byref(cam), C.byref(p), 0, None, 0, 2) == 0


# ---- the per-ray device functions on the host -----------------------------------------------------------------------------------
def _rays_lib():
    lib = C.CDLL(os.path.join(ROOT, "tests", "render_rays", "librays_cpu.so"))
    lib.rays_cpu_records.argtypes = [C.POINTER(_abi.Camera), C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.rays_cpu_meta.argtypes = [C.c_uint32, C.c_void_p]
    lib.rays_cpu_valid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return lib


@pytest.mark.parametrize("fixed", [0, 1])
def test_ray_record_writes_the_camera_records_bits(fixed):
    lib = _rays_lib()
    cam = some_camera()
    p = T.make_params(64, 36, 8, SEED, flags=T.TRT_FLAG_FIXED_PIXELS if fixed else 0)
    for (y, x, s, pid) in [(0, 0, 0, 0), (17, 31, 5, 12345), (35, 63, 7, 0x7FFEFFFF)]:
        a, b = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
        lib.rays_cpu_records(C.byref(cam), 64, 36, SEED, fixed, y, x, s, pid, a.ctypes.data, b.ctypes.data)
        assert (a == b).all(), (y, x, s, pid)
        assert a[6] == pid
        meta = np.zeros(3, np.uint32)
        lib.rays_cpu_meta(int(b[7]), meta.ctypes.data)
        assert tuple(meta) == (2, 3, 0), "next draw 2, camera type, depth 0"
        # ... and the ray in it is trt_camera_rays' ray
        org, dirs = T.camera_rays(cam, p, [y * 64 + x], s, s + 1)
        assert (a[0:3] == bits(org[0, 0])).all() and (a[3:6] == bits(dirs[0, 0])).all()


def test_validity_predicate():
    lib = _rays_lib()
    one, den, tiny = 1.0, 1e-45, 1.2e-38
    nan, inf = float("nan"), float("inf")
    rays = [  # (org, dir, valid)
        ((0, 0, 0), (0, 0, 1), True),
        ((1, 2, 3), (0, 0, 0), False),           # zero direction
        ((1, 2, 3), (-0.0, 0.0, -0.0), False),   # ... of either sign
        ((1, 2, 3), (0, 1, 1), True),            # a single zero component
        ((1, 2, 3), (0, 0, den), True),          # denormals
        ((den, -den, tiny), (den, den, den), True),
        ((nan, 0, 0), (0, 0, 1), False), ((0, nan, 0), (0, 0, 1), False), ((0, 0, nan), (0, 0, 1), False),
        ((0, 0, 0), (nan, 0, 1), False), ((0, 0, 0), (0, nan, 1), False), ((0, 0, 0), (0, 1, nan), False),
        ((inf, 0, 0), (0, 0, 1), False), ((0, -inf, 0), (0, 0, 1), False), ((0, 0, inf), (0, 0, 1), False),
        ((0, 0, 0), (inf, 0, 1), False), ((0, 0, 0), (0, -inf, 1), False), ((0, 0, 0), (0, 1, inf), False),
        ((3.4e38, -3.4e38, 0), (3.4e38, one, 0), True),  # the largest finite values
        ((0, 0, 0), (5, 0, 0), True),            # non-unit, axis-aligned
    ]
    org = np.array([r[0] for r in rays], np.float32)
    dirs = np.array([r[1] for r in rays], np.float32)
    # a NaN with a payload and a set sign bit
    org = np.vstack([org, np.array([[0, 0, 0]], np.float32)])
    dirs = np.vstack([dirs, np.array([0xFFC12345, 0, 0x3F800000], np.uint32).view(np.float32)[None]])
    want = np.array([r[2] for r in rays] + [False], np.uint8)
    got = np.zeros(len(want), np.uint8)
    lib.rays_cpu_valid(org.ctypes.data, dirs.ctypes.data, len(want), got.ctypes.data)
    assert (got == want).all(), np.nonzero(got != want)[0]


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_header_and_mirror_list_the_new_entries():
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    assert re.search(r"#define TRT_ABI_VERSION 5\b", text) and _abi.TRT_ABI_VERSION == 5
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _abi.load_hip()
    assert lib.trt_abi_version() == 5
    for name in ("trt_render_rays", "trt_render_rays_device", "trt_camera_rays", "trt_camera_rays_device"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _abi.HIP_SYMBOLS and hasattr(lib, name), name
    for name in ("render_rays", "render_rays_into", "render_camera"):
        assert callable(getattr(T.Renderer, name))
    assert callable(T.camera_rays) and callable(T.camera_rays_into) and callable(T.look_at)


def test_render_rays_refuses_before_touching_a_device():
    """Every refusal of trt_render_rays is made on the host: with a null handle they cannot have needed a GPU."""
    lib = _abi.load_hip()
    assert lib.trt_render_rays(None, None, 0, None, None, None, 0, 0, None, None, None) == 1
    assert b"null handle" in lib.trt_last_error()


def test_look_at():
    eye, target, up = np.array([3.0, 2.0, -7.0], np.float32), np.array([0.5, 1.0, 2.0], np.float32), (0.0, 1.0, 0.0)
    w, h, fovy = 64, 36, 40.0
    cam = T.look_at(eye, target, up, fovy, w, h)
    hor, ver, llc = (np.array(list(getattr(cam, k)), np.float64) for k in ("horizontal", "vertical", "lower_left_corner"))
    assert (np.array(list(cam.eye), np.float32) == eye).all()
    view = (target - eye).astype(np.float64)
    view /= np.linalg.norm(view)
    # an orthogonal basis: horizontal, vertical and the view direction
    assert abs(hor @ ver) < 1e-5 * np.linalg.norm(hor) * np.linalg.norm(ver)
    assert abs(hor @ view) < 1e-5 * np.linalg.norm(hor) and abs(ver @ view) < 1e-5 * np.linalg.norm(ver)
    assert ver @ np.array(up) > 0  # up is up
    assert np.allclose(np.cross(hor, ver) / (np.linalg.norm(hor) * np.linalg.norm(ver)), -view, atol=1e-5)  # right-handed: u x v = w = -view
    # the centre ray points at the target
    centre = llc + 0.5 * hor + 0.5 * ver - eye
    assert np.allclose(centre / np.linalg.norm(centre), view, atol=1e-5)
    # field of view and aspect ratio
    assert np.isclose(np.linalg.norm(ver), 2.0 * np.tan(np.radians(fovy) / 2.0), rtol=1e-6)
    assert np.isclose(np.linalg.norm(hor) / np.linalg.norm(ver), w / h, rtol=1e-6)
    # the shipped scene's own camera (scene.cpp: eye, lookat, up, fovy from back.xml) comes out of it
    s = T.Scene.named("back", w, h)
    sc = s.flat.contents.camera
    back = T.look_at((278.0, 273.0, -800.0), (278.0, 273.0, -799.0), (0.0, 1.0, 0.0), 39.3077, w, h)
    for k in ("eye", "horizontal", "vertical", "lower_left_corner"):
        assert np.allclose(list(getattr(back, k)), list(getattr(sc, k)), rtol=1e-4, atol=1e-3), k
