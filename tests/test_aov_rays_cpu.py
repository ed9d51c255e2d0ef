"""The host side of trt_aov_rays (include/trt.h) — no GPU needed.

  - the two entries in the header, in the library and in the ctypes mirror, the ABI version unchanged, the per-path figure stated once;
  - the refusal that needs no device;
  - the Python wrappers refuse wrong shapes, dtypes and all-None outputs before the library is called;
  - the accumulation of tests/aov_rays_ref.py on a hand-made hit list that mixes a hit, a miss and an invalid entry.
"""
import os
import re

import numpy as np
import pytest

import aov_rays_ref as R
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_header_library_and_mirror_list_the_entries():
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    assert re.search(r"#define TRT_ABI_VERSION 5\b", text) and _abi.TRT_ABI_VERSION == 5
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _abi.load_hip()
    assert lib.trt_abi_version() == 5
    for name in ("trt_aov_rays", "trt_aov_rays_device"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _abi.HIP_SYMBOLS and hasattr(lib, name), name
    for name in ("render_aov_rays", "render_aov_rays_into", "render_camera_aov", "render_camera_denoised"):
        assert callable(getattr(T.Renderer, name)), name
    m = re.search(r"#define TRT_AOV_RAYS_BYTES_PER_PATH (\d+)u?\b", code)
    assert m and int(m.group(1)) == T.AOV_RAYS_BYTES_PER_PATH == 52  # a 32-byte packed ray, a 16-byte hit, a 4-byte redo entry


def test_refusals_need_no_device():
    """Every refusal of trt_aov_rays is made on the host: with a null handle it cannot have needed a GPU."""
    lib = _abi.load_hip()
    assert lib.trt_aov_rays(None, None, 0, None, None, 0, 0, None, None, None, None) == 1
    assert b"null handle" in lib.trt_last_error()
    p = T.make_params(64, 36, 4, 1)
    assert lib.trt_aov_rays_device(None, p, 0, None, None, 0, 0, None, None, None, None, None) == 1
    assert b"null handle" in lib.trt_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it has to refuse")


def _bare_renderer():
    r = T.Renderer.__new__(T.Renderer)  # no trt_create: the checks under test come before any call into the library
    r._lib, r._h, r.device = _NoLibrary(), None, 0
    return r


def test_host_wrapper_refuses_wrong_arrays():
    r = _bare_renderer()
    p = T.make_params(64, 36, 4, 1)
    org, dirs = np.zeros((2, 5, 3), F32), np.ones((2, 5, 3), F32)
    with pytest.raises(T.TrtError, match=r"shape \(S, n, 3\)"):
        r.render_aov_rays(p, org, dirs[:, :4])
    with pytest.raises(T.TrtError, match=r"shape \(S, n, 3\)"):
        r.render_aov_rays(p, np.zeros((2, 5, 2), F32), np.zeros((2, 5, 2), F32))
    with pytest.raises(T.TrtError, match="at least one"):
        r.render_aov_rays(p, org, dirs, sums={"albedo": None, "depth": None})
    with pytest.raises(T.TrtError, match="at least one"):
        r.render_aov_rays(p, org, dirs, sums={})
    with pytest.raises(T.TrtError, match="keys"):
        r.render_aov_rays(p, org, dirs, sums={"colour": np.zeros((5, 3))})
    with pytest.raises(T.TrtError, match="depth must be a contiguous float64"):
        r.render_aov_rays(p, org, dirs, sums={"depth": np.zeros(5, F32)})
    with pytest.raises(T.TrtError, match="albedo must be a contiguous float64"):
        r.render_aov_rays(p, org, dirs, sums={"albedo": np.zeros((5,), np.float64)})
    with pytest.raises(T.TrtError, match="normal must be a contiguous float64"):
        r.render_aov_rays(p, org, dirs, sums={"normal": np.zeros((3, 5), np.float64).T})


def test_device_wrapper_refuses_wrong_tensors():
    torch = pytest.importorskip("torch")
    r = _bare_renderer()
    p = T.make_params(64, 36, 4, 1)
    org = torch.zeros((2, 5, 3), dtype=torch.float32)  # host tensors: never a device tensor of this handle
    with pytest.raises(T.TrtError, match="at least one"):
        r.render_aov_rays_into(p, org, org)
    with pytest.raises(T.TrtError, match=r"shape \(S, n, 3\)"):
        r.render_aov_rays_into(p, org[0], org[0], depth=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(T.TrtError, match=r"shape \(S, n, 3\)"):
        r.render_aov_rays_into(p, np.zeros((2, 5, 3), F32), org, depth=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(T.TrtError, match="org must be a contiguous float32 tensor on cuda:0"):
        r.render_aov_rays_into(p, org, org, depth=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(T.TrtError, match="spp must be >= 2"):
        r.render_camera_denoised(T.make_params(64, 36, 1, 1), T.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0), 40.0, 64, 36))
    with pytest.raises(T.TrtError, match="interleave"):
        r.render_camera_denoised(T.make_params(64, 36, 4, 1, rows=(2, 3, 1)), T.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0), 40.0, 64, 36))


def test_validity_rule():
    nan, inf = F32("nan"), F32("inf")
    org = np.array([[0, 0, 0], [nan, 0, 0], [0, 0, 0], [0, 0, 0], [0, -inf, 0], [1e-45, 0, 0], [0, 0, 0]], F32)
    dirs = np.array([[0, 0, 1], [0, 0, 1], [0, inf, 0], [0, 0, 0], [1, 1, 1], [0, 1e-45, 0], [-0.0, 0.0, -0.0]], F32)
    assert R.valid_entries(org, dirs).tolist() == [True, False, False, False, False, True, False]


def test_accumulation_on_a_hand_made_hit_list():
    """Three entries over three samples at spp = 3: entry 0 always hits, entry 1 always misses, entry 2 hits, is invalid, hits.  1/3 is not a
    binary fraction, so the float division and the double additions are both visible in the bits."""
    spp = 3
    alb = np.zeros((3, 3, 3), F32)
    nrm = np.zeros((3, 3, 3), F32)
    dep = np.full((3, 3), R.aov_ref.TRT_INF, F32)
    valid = np.ones((3, 3), bool)
    hit_a, hit_n = np.array([0.7, 0.1, 0.25], F32), np.array([0.6, -0.8, 0.0], F32)
    for s in range(3):
        alb[s, 0], nrm[s, 0], dep[s, 0] = hit_a, hit_n, F32(10.0 + s)
        alb[s, 2], nrm[s, 2], dep[s, 2] = hit_a, hit_n, F32(5.5)
    valid[1, 2] = False  # what the hit list says for an invalid entry is not looked at: it counts as a miss
    start = R.zero_sums(3)
    start["depth"][:] = 1.0
    got = R.accumulate(alb, nrm, dep, valid, spp, sums={k: v.copy() for k, v in start.items()})
    third = F32(spp)
    inf_term = np.float64(F32(R.aov_ref.TRT_INF) / third)

    def total(terms, begin=0.0):
        acc = np.float64(begin)
        for v in terms:
            acc = acc + np.float64(F32(v) / third)
        return acc

    for c in range(3):
        assert got["albedo"][0, c] == total([hit_a[c]] * 3) and got["normal"][0, c] == total([hit_n[c]] * 3)
        assert got["albedo"][1, c] == 0.0 and got["normal"][1, c] == 0.0
        assert got["albedo"][2, c] == total([hit_a[c], 0.0, hit_a[c]]) and got["normal"][2, c] == total([hit_n[c], 0.0, hit_n[c]])
    assert got["depth"][0] == total([10.0, 11.0, 12.0], 1.0)
    assert got["depth"][1] == (np.float64(1.0) + inf_term) + inf_term + inf_term
    assert got["depth"][2] == total([5.5, R.aov_ref.TRT_INF, 5.5], 1.0)
    assert got["albedo"][0, 0] != np.float64(hit_a[0]), "three float thirds do not add up to the value: the order of operations shows"
    # a sum that is not wanted is left out, the others do not change
    part = R.accumulate(alb, nrm, dep, valid, spp, sums={"depth": start["depth"].copy()})
    assert list(part) == ["depth"] and (part["depth"] == got["depth"]).all()
