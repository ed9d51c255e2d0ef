"""trt_denoise without a GPU: the CPU build of the filter's per-pixel code (tests/denoise, the code the kernels run) against the float64
restatement of include/trt.h in tests/denoise_ref.py, on random guides, on oracle renders and on edge cases; the argument checks of both C
entries, of T.denoise and of tinyrt --denoise; the new symbols are declared, exported and mirrored."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("h,w,seed,kw", [
    (24, 32, 1, {}),
    (33, 17, 2, {"iterations": 3, "sigma_normal": 16, "sigma_depth": 2.5, "sigma_luminance": 1.5}),
    (40, 40, 3, {"iterations": 1}),
    (19, 45, 4, {"iterations": 10, "sigma_normal": 1}),
    (31, 29, 5, {"iterations": 7, "sigma_normal": 256, "sigma_depth": 0.25, "sigma_luminance": 8.0}),
])
def test_cpu_build_matches_the_restatement_on_random_guides(h, w, seed, kw):
    x = D.random_inputs(h, w, seed)
    got = D.cpu(*x, **kw)
    D.assert_close(got, D.restate(*x, **kw), what=f"{h}x{w} {kw}")
    assert np.abs(got - x[0]).max() > 1e-3  # it filtered something


@pytest.mark.parametrize("name", ["back", "staircase"])
def test_cpu_build_matches_the_restatement_on_oracle_renders(name):
    x = D.oracle_inputs(name, 24, 18)
    assert (x[4] < D.INF).any() and (x[1] > 0).any()
    for kw in ({}, {"iterations": 2, "sigma_luminance": 2.0}):
        D.assert_close(D.cpu(*x, **kw), D.restate(*x, **kw), what=f"{name} {kw}")


@pytest.mark.parametrize("h,w", [(1, 1), (1, 13), (13, 1), (2, 3), (7, 5), (3, 31)])
@pytest.mark.parametrize("iterations", [1, 5, 10])
def test_edge_sizes_and_images_smaller_than_the_step(h, w, iterations):
    x = D.random_inputs(h, w, 100 + h * 7 + w, miss_frac=0.2)
    D.assert_close(D.cpu(*x, iterations=iterations), D.restate(*x, iterations=iterations), what=f"{h}x{w}")


def test_one_pixel_and_all_miss_images_pass_the_colour_through():
    x = list(D.random_inputs(1, 1, 9, miss_frac=0.0))
    x[2][:] = 0.5  # albedo that divides and multiplies back exactly
    assert D.cpu(*x).tobytes() == x[0].tobytes()  # only the centre tap: c' = c
    y = list(D.random_inputs(12, 10, 10))
    y[4][:] = D.INF
    y[2][:] = 0.0  # a miss: albedo 0, so a = 1
    assert D.cpu(*y).tobytes() == y[0].tobytes()


def test_misses_do_not_leak_into_hits():
    """A tap on a miss pixel has weight 0: changing the colour of every miss leaves every hit's result alone."""
    x = list(D.random_inputs(20, 24, 11, miss_frac=0.3))
    a = D.cpu(*x)
    miss = x[4] >= D.INF
    x[0] = x[0].copy()
    x[0][miss] = 1e3
    b = D.cpu(*x)
    assert np.array_equal(a[~miss], b[~miss])
    assert (b[miss] != a[miss]).any()


def test_defaults_are_the_zero_fields():
    x = D.random_inputs(16, 16, 12)
    assert D.cpu(*x).tobytes() == D.cpu(*x, iterations=0, sigma_normal=0, sigma_depth=0.0, sigma_luminance=0.0).tobytes()
    assert D.cpu(*x).tobytes() != D.cpu(*x, iterations=4).tobytes()


def test_building_blocks():
    L = D.lib()
    for d2 in (1, 2, 4, 5, 8):
        assert np.float32(L.denoise_cpu_radius(d2)) == np.sqrt(np.float32(d2))  # correctly rounded
    for b in (0.99, 0.5, 0.9999, 1.0, 0.0):
        assert np.float32(L.denoise_cpu_powi(b, 128)).tobytes() == _squarings(np.float32(b), 7).tobytes()
        for e in (1, 3, 100, 256):
            assert abs(L.denoise_cpu_powi(b, e) - b ** e) <= 1e-5 * max(b ** e, 1e-30) + 1e-38
    for v in (0.0, -1e-3, -1.0, -20.0, -86.0):
        assert abs(L.denoise_cpu_expf_neg(v) - np.exp(v)) <= 2e-7 * np.exp(v)


def _squarings(b, n):
    for _ in range(n):
        b = np.float32(b * b)
    return b


def test_cpu_build_refuses_what_trt_denoise_refuses():
    x = [D._f32(a) for a in D.random_inputs(4, 4, 13)]
    out = np.empty((4, 4, 3), np.float32)
    ptrs = [a.ctypes.data_as(D.fp) for a in x] + [out.ctypes.data_as(D.fp)]
    for p in (D.params(iterations=11), D.params(iterations=-1), D.params(sigma_normal=257), D.params(sigma_normal=-1),
              D.params(sigma_depth=-1.0), D.params(sigma_luminance=float("nan")), D.params(flags=1)):
        assert D.lib().denoise_cpu(C.byref(p), 4, 4, *ptrs) == 1


# ---- the C ABI and the Python layer -------------------------------------------------------------------------------------------------

def _entry_args(w=4, h=4):
    bufs = [np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32),
            np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)]
    return bufs, [b.ctypes.data_as(D.fp) for b in bufs]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_denoise_entries_check_their_arguments_before_the_device():
    lib = _abi.load_hip()
    keep, ptrs = _entry_args()
    good = D.params()

    def host(p, w, h, bufs):
        return lib.trt_denoise(0, p, w, h, *bufs, None)

    def dev(p, w, h, bufs):
        return lib.trt_denoise_device(0, p, w, h, *[C.cast(b, C.c_void_p) if b else None for b in bufs], None, None)

    for call in (host, dev):
        for i in range(6):
            bufs = list(ptrs)
            bufs[i] = None
            assert call(C.byref(good), 4, 4, bufs) == 1 and b"null buffer" in lib.trt_last_error()
        assert call(C.byref(good), 0, 4, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(good), 4, -3, ptrs) == 1
        assert call(C.byref(good), 1 << 15, (1 << 13) + 1, ptrs) == 1 and b"2^28" in lib.trt_last_error()
        for p, msg in ((D.params(iterations=11), b"iterations"), (D.params(iterations=-2), b"iterations"), (D.params(sigma_normal=300), b"sigma_normal"),
                       (D.params(sigma_normal=-5), b"sigma_normal"), (D.params(sigma_depth=-0.5), b"sigmas"), (D.params(sigma_luminance=float("nan")), b"sigmas"),
                       (D.params(flags=2), b"flags")):
            assert call(C.byref(p), 4, 4, ptrs) == 1 and msg in lib.trt_last_error(), msg
    if not _gpu_present():
        # valid arguments reach the device check: no gfx950 here
        assert host(C.byref(good), 4, 4, ptrs) == 4
        assert host(None, 4, 4, ptrs) == 4  # NULL params = every default
        assert lib.trt_denoise(7, C.byref(good), 4, 4, *ptrs, None) == 4


def test_python_denoise_checks_shapes_and_parameters():
    x = D.random_inputs(6, 5, 14)
    with pytest.raises(T.TrtError, match="color"):
        T.denoise(x[0][..., :2], *x[1:])
    with pytest.raises(T.TrtError, match="variance"):
        T.denoise(x[0], x[1][:, :4], *x[2:])
    with pytest.raises(T.TrtError, match="normal"):
        T.denoise(x[0], x[1], x[2], x[3][:5], x[4])
    with pytest.raises(T.TrtError, match="depth"):
        T.denoise(*x[:4], x[4][None])
    with pytest.raises(T.TrtError, match="iterations"):
        T.denoise(*x, iterations=11)
    with pytest.raises(T.TrtError, match="sigma_normal"):
        T.denoise(*x, sigma_normal=-1)
    with pytest.raises(T.TrtError, match="sigmas"):
        T.denoise(*x, sigma_luminance=-1)
    with pytest.raises(T.TrtError, match="denoise_into"):
        T.denoise_into(x[0], *x[1:], out=None)


def test_denoise_symbols_are_declared_exported_and_mirrored():
    hip = C.CDLL(os.path.join(_abi.LIB_DIR, "libtrt_hip.so"))
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    for n in ("trt_denoise", "trt_denoise_device"):
        assert hasattr(hip, n) and n in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + n + r"\(", text)
    assert re.search(r"TRT_K_DENOISE = 6\b", text) and T.TRT_K_DENOISE == _abi.TRT_K_DENOISE == 6 < _abi.TRT_MAX_KERNELS
    assert "denoise" not in _abi.KERNEL_NAMES and len(_abi.KERNEL_NAMES) == 6  # bench.py reads KERNEL_NAMES[-1]
    assert re.search(r"#define TRT_ABI_VERSION 5\b", text)
    sizes = (C.c_int64 * 12)()
    assert _abi.load_host().trth_abi_sizes(sizes) == 0
    assert sizes[10] == C.sizeof(_abi.DenoiseParams) == 20


def test_mean_luminance_variance_from_moments():
    rng = np.random.default_rng(15)
    spp, n = 8, 50
    L = rng.gamma(2.0, 0.3, size=(spp, n, 3))
    v = L / spp
    got = T.mean_luminance_variance(v.sum(0), (v * v).sum(0), spp)
    want = (L.var(axis=0, ddof=1) / spp) @ (D.LUMA ** 2)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    assert got.dtype == np.float32 and (T.mean_luminance_variance(np.ones((3, 3)), np.ones((3, 3)) / 4, 4) == 0).all()


def _tinyrt(*extra):
    exe = os.path.join(_abi.LIB_DIR, "tinyrt")
    d = os.path.join(ROOT, "scenes", "back")
    cmd = [exe, d, os.path.join(d, "back.mtl"), os.path.join(d, "back.xml"), os.path.join(d, "back.obj"), *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,msg", [
    (["--gpus", "2"], "--gpus or --devices"),
    (["--devices", "0"], "--gpus or --devices"),
    (["--devices", "0,0"], "--gpus or --devices"),
    (["--every", "4"], "--every or --checkpoint"),
    (["--checkpoint", "x.acc"], "--every or --checkpoint"),
])
def test_tinyrt_refuses_denoise_with_tiling_and_progressive_options(extra, msg, tmp_path):
    r = _tinyrt("16", "--denoise", str(tmp_path / "d.png"), *extra)
    assert r.returncode == 2 and msg in r.stderr, r.stderr
    assert not (tmp_path / "d.png").exists()


def test_tinyrt_refuses_denoise_of_one_sample(tmp_path):
    r = _tinyrt("1", "--denoise", str(tmp_path / "d.png"))
    assert r.returncode == 2 and "spp >= 2" in r.stderr
    r = _tinyrt("4", "--denoise")
    assert r.returncode == 2 and "needs a value" in r.stderr
