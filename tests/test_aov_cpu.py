"""trt_render_aov without a GPU: the restatement in tests/aov_ref.py against the oracle's own path (its vertex 0 is the camera ray's first
hit), the exported symbols and the argument checks of the C ABI and the Python wrapper, and the PFM writer of libtrt_host.so."""
import ctypes as C
import os

import numpy as np
import pytest

import aov_ref
import oracle_lib as O
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi
from conftest import get_scene

SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}


@pytest.mark.parametrize("flags", [0, T.TRT_FLAG_FIXED_PIXELS])
@pytest.mark.parametrize("name", ["back", "veach-mis", "staircase"])
def test_restated_camera_ray_and_first_hit_are_vertex_0_of_the_oracle_path(name, flags):
    W, H = 48, 32
    s = get_scene(name, W, H)
    p = T.make_params(W, H, 8, SEEDS[name], flags=flags)
    rng = np.random.default_rng(7 + flags)
    n = 300
    ys, xs, ss = rng.integers(0, H, n), rng.integers(0, W, n), rng.integers(0, 64, n)
    org, dirs = aov_ref.camera_rays(s.flat, p, ys, xs, ss)
    t, tri, uv = O.trace(s.flat, org, dirs)
    hits = 0
    for i in range(n):
        v0 = O.debug_path(s.flat, p, int(xs[i]), int(ys[i]), int(ss[i]), max_vertices=1)[0]
        assert np.float32(v0[0]).tobytes() == t[i].tobytes() and int(v0[1]) == int(tri[i]), (i, v0[:4], t[i], tri[i])
        if tri[i] >= 0:
            hits += 1
            assert v0[2:4].astype(np.float32).tobytes() == uv[i].tobytes(), (i, v0[2:4], uv[i])
    assert hits > n // 4
    # the features of those hits: unit normals (up to rounding) and albedo in [0, 1]; a miss is all zero at TRT_INF
    albedo, normal, depth = aov_ref.first_hit_features(s, t, tri, uv)
    hit = tri >= 0
    assert np.allclose(np.linalg.norm(normal[hit], axis=1), 1.0, atol=1e-5)
    assert (albedo >= 0).all() and (albedo <= 1).all()
    assert (albedo[~hit] == 0).all() and (normal[~hit] == 0).all() and (depth[~hit] == np.float32(114514.0)).all()
    assert np.array_equal(depth[hit], t[hit])


def test_staircase_albedo_comes_from_its_textures():
    """staircase has textured materials: some first hits take their albedo from a texel, not from Kd."""
    s = get_scene("staircase", 48, 32)
    p = T.make_params(48, 32, 2, SEEDS["staircase"])
    ys, xs, ss, _ = aov_ref.tile_samples(p)
    org, dirs = aov_ref.camera_rays(s.flat, p, ys, xs, ss)
    t, tri, uv = O.trace(s.flat, org, dirs)
    albedo, _, _ = aov_ref.first_hit_features(s, t, tri, uv)
    f = s.flat.contents
    mats = s.arrays()["tri_mat"][tri[tri >= 0]]
    textured = np.array([f.materials[m].tex >= 0 for m in mats])
    assert textured.any()
    texel = albedo[tri >= 0][textured]
    assert len(np.unique(texel, axis=0)) > 4  # many different texels, not one Kd


def test_aov_symbols_are_exported():
    hip = C.CDLL(os.path.join(_abi.LIB_DIR, "libtrt_hip.so"))
    host = C.CDLL(os.path.join(_abi.LIB_DIR, "libtrt_host.so"))
    for n in ("trt_render_aov", "trt_render_aov_device"):
        assert hasattr(hip, n) and n in _abi.HIP_SYMBOLS
    assert hasattr(host, "trth_write_pfm") and "trth_write_pfm" in _abi.HOST_SYMBOLS


def test_render_aov_refuses_null_handle_params_and_outputs():
    lib = _abi.load_hip()
    p = T.make_params(16, 16, 1, 1)
    buf = (C.c_float * (16 * 16 * 3))()
    assert lib.trt_render_aov(None, C.byref(p), buf, buf, buf, None) == 1
    assert lib.trt_render_aov(C.c_void_p(1), None, buf, buf, buf, None) == 1
    assert lib.trt_render_aov(None, C.byref(p), None, None, None, None) == 1
    assert lib.trt_render_aov_device(None, C.byref(p), None, None, None, None, None) == 1
    assert lib.trt_render_aov_device(C.c_void_p(1), None, None, None, None, None, None) == 1
    assert b"null" in lib.trt_last_error()


def _read_pfm(path):
    data = open(path, "rb").read()
    magic, dims, scale, rest = data.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    ch = 3 if magic == b"PF" else 1
    assert magic in (b"PF", b"Pf") and float(scale) == -1.0
    a = np.frombuffer(rest, dtype="<f4")
    assert a.size == w * h * ch
    return magic, scale, a.reshape((h, w, ch) if ch == 3 else (h, w))


def test_pfm_writer_round_trips_header_row_order_and_bits(tmp_path):
    rng = np.random.default_rng(3)
    rgb = rng.standard_normal((5, 7, 3)).astype(np.float32)
    rgb[0, 0] = [np.inf, -0.0, np.float32(1e-45)]
    depth = rng.random((5, 7)).astype(np.float32)
    T.write_pfm(str(tmp_path / "c.pfm"), rgb)
    T.write_pfm(str(tmp_path / "d.pfm"), depth)
    raw = open(tmp_path / "c.pfm", "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n")
    assert open(tmp_path / "d.pfm", "rb").read().startswith(b"Pf\n7 5\n-1.0\n")
    magic, _, back = _read_pfm(str(tmp_path / "c.pfm"))
    assert back[::-1].tobytes() == rgb.tobytes()  # the file's first row is the image's bottom row
    assert raw[len(b"PF\n7 5\n-1.0\n"):][:4 * 21] == rgb[4].astype("<f4").tobytes()
    magic, _, back = _read_pfm(str(tmp_path / "d.pfm"))
    assert magic == b"Pf" and back[::-1].tobytes() == depth.tobytes()
    lib = _abi.load_host()
    assert lib.trth_write_pfm(os.fsencode(str(tmp_path / "e.pfm")), 7, 5, 2, rgb.ctypes.data_as(C.POINTER(C.c_float))) != 0
    assert lib.trth_write_pfm(os.fsencode(str(tmp_path / "e.pfm")), 7, 5, 3, None) != 0
    assert lib.trth_write_pfm(os.fsencode(str(tmp_path / "nodir" / "e.pfm")), 7, 5, 3, rgb.ctypes.data_as(C.POINTER(C.c_float))) != 0


class _NoCallLib:
    """The HIP library with trt_render_aov_device replaced by a tripwire: argument checks must refuse before any call."""

    def __init__(self):
        self._real = _abi.load_hip()
        self.calls = 0

    def trt_rows_selected(self, p):
        return self._real.trt_rows_selected(p)

    def trt_render_aov_device(self, *a):
        self.calls += 1
        raise AssertionError("trt_render_aov_device called")


def test_render_aov_into_checks_tensors_before_any_call():
    import torch
    r = T.Renderer.__new__(T.Renderer)
    r._lib, r._h, r.device = _NoCallLib(), None, 0
    p = T.make_params(8, 6, 1, 1, tile=(0, 0, 4, 6))  # 6 rows x 4 columns
    good_cpu = torch.zeros(6 * 4 * 3, dtype=torch.float32)
    bad = [dict(),
           dict(albedo=torch.zeros(6 * 4 * 3, dtype=torch.float64)),
           dict(normal=torch.zeros(6 * 4 * 3 - 1, dtype=torch.float32)),
           dict(depth=good_cpu),  # host memory, not the renderer's device
           dict(albedo=np.zeros(6 * 4 * 3, np.float32)),
           dict(albedo=torch.zeros((6 * 4 * 3, 2), dtype=torch.float32)[:, 0])]  # not contiguous
    for kw in bad:
        with pytest.raises(T.TrtError):
            r.render_aov_into(p, **kw)
    assert r._lib.calls == 0
