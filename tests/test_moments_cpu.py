"""trt_reproject_moments without a GPU: the CPU build of the kernels' per-pixel code (tests/moments) gives trt_reproject's and
trt_reproject_motion's colour path bit for bit; it agrees with the float64 restatement of the contract (tests/moments_ref.py); the temporal
and the spatial estimate give the variance that was put in; edges stop the spatial estimate; identical frames have no variance; an isolated
pixel falls back on v = M1^2; images smaller than the window; the C entries' argument checks in their order, the Python wrappers and the
ABI mirror; hostile values under the host sanitizers (a stand-alone driver)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import moments_ref as MV
import motion_ref as M
import reproject_ref as R
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [0, R.FIXED]
H, W = 37, 53
# Tolerance, as tests/test_reproject_cpu.py derives it for the same chain of operations: |got - want| <= RTOL (|want| + max |want| of the
# channel), RTOL = 5e-5.  The variance is a difference m2 - m1^2 of two numbers of the size of m2: its fp32 error is a few 2^-24 of m2,
# not of the difference, which is why the bound is taken against the channel's scale as well; stage B adds the weights' errors (128
# squarings' worth of 2^-24 on wn, about 1e-5), still inside the bound.
RTOL = 5e-5
MAX_EDGE_SHARE = 0.03
# the restatement's images: test_reproject_cpu.py's bound on a bilinear weight's error, W * 30 * 2^-24, holds RTOL up to W = 33
RH, RW = 24, 32
# chosen by the restatement alone: the first seed from 710 on whose edge share is under 3 % in every case of the test (710: 3.4 %, 711: 4.8 %,
# 712: 1.7 %)
SEED = 712


def _bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


def _points(kind, cam, cur, flags, seed):
    if kind == "camera":
        return None
    h, w = cur[3].shape
    return M.smooth_field_points(cam, w, h, cur[3], flags, seed) if kind == "field" else M.pixel_points(cam, w, h, cur[3], flags)


# ---- the colour path is trt_reproject's ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", GRIDS)
@pytest.mark.parametrize("kind", ["camera", "points", "field"])
def test_colour_path_has_the_bits_of_reproject_and_reproject_motion(kind, flags):
    cur, hist = MV.random_frames(H, W, 700)
    cam, pcam = R.nearby_cameras(W, H, 700)
    variance = np.full((H, W), 1e-3, np.float32)
    for prev, kw in ((pcam, {}), (cam, {}), (pcam, dict(alpha=0.05, depth_tolerance=0.12, normal_threshold=0.8, max_history=6.0))):
        P = _points(kind, cam, cur, flags, 700)
        got = MV.cpu(*cur, cam, prev, hist, prev_point=P, flags=flags, **kw)
        h4 = {k: hist[k] for k in R.HISTORY_KEYS}
        if P is None:
            want = R.cpu(cur[0], variance, *cur[1:], cam, prev, h4, flags=flags, **kw)
        else:
            want = M.cpu(cur[0], variance, *cur[1:], P, cam, prev, h4, flags=flags, **kw)
        used = (want["length"] > 1).mean()
        assert 0.2 < used < 0.98, used  # planted misses and NaN depths, failed taps: both outcomes
        assert _bits(got["cv"][..., :3], want["cv"][..., :3]) and _bits(got["length"], want["length"]) and _bits(got["color"], want["color"])
    # a first frame too
    got, want = MV.cpu(*cur, cam), R.cpu(cur[0], variance, *cur[1:], cam)
    assert _bits(got["cv"][..., :3], want["cv"][..., :3]) and _bits(got["length"], want["length"]) and _bits(got["color"], want["color"])


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def _compare(got, want, keys=MV.OUT_KEYS):
    edge = want["edge"]
    for k in keys:
        g, wn = got[k].astype(np.float64)[~edge], want[k][~edge]
        assert np.isfinite(g).all(), k
        scale = np.abs(wn).max(axis=0, initial=0.0)
        err = np.abs(g - wn) - RTOL * (np.abs(wn) + scale)
        assert (err <= 0).all(), (k, float(err.max()))


@pytest.mark.parametrize("flags", GRIDS)
@pytest.mark.parametrize("kind", ["camera", "field"])
def test_cpu_build_matches_the_float64_restatement(kind, flags):
    cur, hist = MV.random_frames(RH, RW, SEED)
    cam, pcam = R.nearby_cameras(RW, RH, SEED)
    P = _points(kind, cam, cur, flags, SEED)
    hit = cur[3] < R.INF
    for history, kw in ((hist, {}), (hist, dict(alpha=0.05, normal_threshold=0.8, max_history=6.0, min_frames=2, sigma_normal=32, sigma_depth=3.0)), (None, {})):
        got = MV.cpu(*cur, cam, pcam, history, prev_point=P, flags=flags, **kw)
        alone = MV.restate(*cur, cam, pcam, history, prev_point=P, flags=flags, **kw)
        want = MV.restate(*cur, cam, pcam, history, prev_point=P, flags=flags, stage_a=(got["mom"], got["length"]), **kw)
        share, share_alone = want["edge"][hit].mean(), alone["edge"][hit].mean()
        on_route = want["temporal"][hit].mean()
        print(f"{kind} flags {flags} {kw}: {int(hit.sum())} hit pixels, {on_route:.2f} on the temporal route, edge share {share:.3f} (the reference alone {share_alone:.3f})")
        assert share <= MAX_EDGE_SHARE and share_alone <= MAX_EDGE_SHARE
        if history is not None:
            assert 0.1 < on_route < 0.9  # both routes
        else:
            assert on_route == 0
        _compare(got, want)
        # stage A on its own against the reference alone (stage B's inputs there are the reference's own records)
        _compare(got, alone, keys=("color", "length", "mom"))
        both = ~alone["edge"] & alone["temporal"]
        g, wn = got["variance"].astype(np.float64)[both], alone["variance"][both]
        assert (np.abs(g - wn) <= RTOL * (np.abs(wn) + np.abs(alone["variance"][~alone["edge"]]).max())).all()
        # stage B's windows hold more than their centre: most spatial pixels estimate, not all
        spatial = hit & ~want["temporal"] & ~want["edge"]
        assert (got["cv"][..., 3][~hit] == 0).all() and (got["variance"][~hit] == 0).all()
        assert spatial.sum() > 50


# ---- estimates with a known answer ----------------------------------------------------------------------------------------------------

def _run_sequence(frames, cam, **kw):
    hist, outs = None, []
    for f in frames:
        out = MV.cpu(*f, cam, cam, hist, **kw)
        hist = MV.next_history(out, f[2], f[3])
        outs.append(out)
    return outs


def test_temporal_estimate_returns_the_variance_of_the_mean():
    """Five frames of l = 1 + 0.2 g on a flat plane, alpha = 0.2: the history is the running mean, s' = 1/5, every pixel on the temporal
    route, and the mean estimate is sigma^2 / 5 = 0.008 within 5 % (the standard error of the mean over 4096 pixels of an unbiased
    five-sample variance, relative sqrt(2 / 4) / 64 = 1.1 %)."""
    frames, cam = MV.flat_sequence(64, 64, 5, 11)
    out = _run_sequence(frames, cam, alpha=0.2)[-1]
    assert (out["length"] == 5).all()
    np.testing.assert_allclose(out["mom"][..., 2], 0.2, rtol=1e-6)
    mean = float(out["variance"].astype(np.float64).mean())
    print(f"temporal estimate: mean {mean:.6f}, expected {0.04 / 5:.6f}, ratio {mean / (0.04 / 5):.4f}")
    assert abs(mean - 0.04 / 5) <= 0.05 * (0.04 / 5)
    # the route: stage B changes nothing there — the variance is the pixel's own m2 - m1^2 over 1 - s, times s (the difference of two
    # numbers near 1 carries a few 2^-24 of absolute error in fp32, a quarter of which reaches the result)
    m = out["mom"].astype(np.float64)
    np.testing.assert_allclose(out["cv"][..., 3], np.maximum(m[..., 1] - m[..., 0] ** 2, 0) / (1 - m[..., 2]) * m[..., 2], rtol=1e-4, atol=1e-7)


def test_spatial_estimate_returns_the_variance_of_the_frame():
    """Frame 1 of the same sequence: no history, every pixel through stage B; an interior pixel's 49 taps weigh 1 each, W2 = 1/49, and the
    mean estimate over the 58 x 58 interior is sigma^2 = 0.04 within 10 % (overlapping windows: 3364 / 49 independent ones, 2.5 %)."""
    frames, cam = MV.flat_sequence(64, 64, 1, 11)
    out = _run_sequence(frames, cam)[0]
    assert (out["length"] == 1).all() and (out["mom"][..., 2] == 1).all()
    inner = out["variance"][3:-3, 3:-3].astype(np.float64)
    assert inner.shape == (58, 58)
    mean = float(inner.mean())
    print(f"spatial estimate: mean {mean:.5f}, expected 0.04, ratio {mean / 0.04:.4f}")
    assert abs(mean - 0.04) <= 0.1 * 0.04
    # one interior pixel by hand
    l = frames[0][0][..., 0].astype(np.float64)[10:17, 20:27]
    np.testing.assert_allclose(out["cv"][13, 23, 3], ((l * l).mean() - l.mean() ** 2) / (1 - 1 / 49), rtol=2e-4)


def test_edges_stop_the_spatial_estimate():
    h, w = 24, 32
    l = np.where(np.arange(w) < w // 2, 1.0, 10.0)[None, :].repeat(h, 0)
    normal = np.zeros((h, w, 3), np.float32)
    normal[:, : w // 2, 2] = 1.0
    normal[:, w // 2:, 0] = 1.0
    color = R._f32(np.repeat(l[..., None], 3, axis=2))
    frame = (color, np.ones((h, w, 3), np.float32), normal, np.full((h, w), 5.0, np.float32))
    out = MV.cpu(*frame, R.plane_camera(0.0, 0.0, w, h))
    assert (out["variance"] <= 1e-5 * l * l).all(), float((out["variance"] / (l * l)).max())
    # what the normal weight is for: without it the seam columns would mix 1 and 10
    out = MV.cpu(color, frame[1], np.broadcast_to(np.float32([0, 0, 1]), (h, w, 3)), frame[3], R.plane_camera(0.0, 0.0, w, h))
    assert out["variance"][:, w // 2 - 1: w // 2 + 1].min() > 10.0


def test_identical_frames_have_no_variance():
    frames, cam = MV.flat_sequence(16, 20, 1, 5)
    out = _run_sequence([frames[0]] * 8, cam)[-1]
    l = frames[0][0][..., 0].astype(np.float64)
    assert (out["length"] == 8).all()
    assert (out["variance"] <= 1e-5 * l * l).all() and (out["cv"][..., 3] <= 1e-5 * l * l).all()


def test_isolated_pixel_takes_its_own_value_as_its_deviation():
    h, w = 9, 11
    depth = np.full((h, w), R.INF, np.float32)
    depth[4, 5] = 7.0
    depth[0, 0] = 3.0  # a corner: its window is mostly outside the image
    normal = np.zeros((h, w, 3), np.float32)
    normal[4, 5] = normal[0, 0] = (0.0, 0.6, 0.8)
    color = np.full((h, w, 3), 0.6, np.float32)
    albedo = np.full((h, w, 3), 0.5, np.float32)
    out = MV.cpu(color, albedo, normal, depth, R.plane_camera(0.0, 0.0, w, h))
    for y, x in ((4, 5), (0, 0)):
        m1 = np.float32(out["mom"][y, x, 0])
        assert out["cv"][y, x, 3] == m1 * m1 and abs(m1 - 1.2) < 1e-6
        np.testing.assert_allclose(out["variance"][y, x], float(m1) ** 2 * 0.25, rtol=1e-6)
    miss = depth >= R.INF
    assert (out["variance"][miss] == 0).all() and (out["cv"][..., 3][miss] == 0).all() and (out["length"] == 1).all()


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 7)])
def test_images_smaller_than_the_window(h, w):
    frames, cam = MV.flat_sequence(h, w, 6, 3)
    outs = _run_sequence(frames, cam)
    for k, out in enumerate(outs):
        assert all(np.isfinite(out[key]).all() for key in MV.OUT_KEYS) and (out["length"] == k + 1).all()
        want = MV.restate(*frames[k], cam, cam, None if k == 0 else MV.next_history(outs[k - 1], frames[k][2], frames[k][3]))
        assert want["temporal"].all() == (k + 1 >= 4)
        ok = ~want["edge"]
        np.testing.assert_allclose(out["variance"][ok], want["variance"][ok], rtol=1e-3, atol=1e-7)
    # the first frame of a 1 x 1 image is an isolated pixel
    if h * w == 1:
        assert outs[0]["cv"][0, 0, 3] == outs[0]["mom"][0, 0, 0] ** 2


# ---- robustness, under the host sanitizers ------------------------------------------------------------------------------------------

def test_hostile_values_finish_under_the_host_sanitizers(tmp_path):
    """NaN and infinite depths, cameras, points and mom records (a negative s, s > 1) through both stages at 1 x 1, 5 x 7 and 33 x 17: a
    stand-alone program (tests/moments/moments_san.cpp with the CPU build compiled in) under AddressSanitizer and UBSan."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "moments_san")
    cmd = [cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
           "-ffp-contract=off", "-march=x86-64-v3", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyraytracing_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "moments", "moments_cpu.cpp"), os.path.join(ROOT, "tests", "moments", "moments_san.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    # the inherited environment, unchanged but for the sanitizers' own options; the runtimes are linked statically into this stand-alone
    # program, and the link-order check is off so that it also starts where the environment preloads some other library
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the C ABI and the Python layer -------------------------------------------------------------------------------------------------

# color, albedo, normal, depth, prev_point | prev_cv, prev_len, prev_normal, prev_depth, prev_mom | out_color, out_variance, out_cv, out_len, out_mom
SHAPES = [3, 3, 3, 1, 3, 4, 1, 3, 1, 4, 3, 1, 4, 1, 4]
REQUIRED, HISTORY = (0, 1, 2, 3, 10, 11, 12, 13, 14), (5, 6, 7, 8, 9)


def _entry_args(w=4, h=4):
    bufs = [np.zeros((h, w, c), np.float32) for c in SHAPES]
    return bufs, [b.ctypes.data_as(R.fp) for b in bufs]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_moments_entries_check_their_arguments_in_order_before_the_device():
    lib = _abi.load_hip()
    keep, ptrs = _entry_args()
    cam = R.plane_camera(0.0, 0.0, 4, 4)
    good = MV.params(cam)

    def host(p, w, h, bufs):
        return lib.trt_reproject_moments(0, p, w, h, *bufs, None)

    def dev(p, w, h, bufs):
        return lib.trt_reproject_moments_device(0, p, w, h, *[C.cast(b, C.c_void_p) if b else None for b in bufs], None, None)

    def cpu(p, w, h, bufs):
        return MV.lib().reproject_moments_cpu(p, w, h, *bufs)

    nan = float("nan")
    # the order: each case is wrong in the named way AND in every later way; the named message must come
    bad_later = dict(alpha=2.0, min_frames=300, sigma_normal=-1, sigma_depth=-1.0)
    for call in (host, dev):
        assert call(None, 0, 0, [None] * 15) == 1 and b"null params" in lib.trt_last_error()
        for i in REQUIRED:
            bufs = list(ptrs)
            bufs[i], bufs[5] = None, None  # and a partial history
            assert call(C.byref(MV.params(cam, **bad_later)), 0, 4, bufs) == 1 and b"null buffer" in lib.trt_last_error()
        for missing in ((5,), (6,), (7,), (8,), (9,), (5, 6), (6, 7, 8, 9), (5, 9), (5, 6, 7, 8)):
            bufs = list(ptrs)
            for i in missing:
                bufs[i] = None
            assert call(C.byref(MV.params(cam, **bad_later)), 0, 4, bufs) == 1 and b"partial history" in lib.trt_last_error()
        assert call(C.byref(MV.params(cam, **bad_later)), 0, 4, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(good), 4, -3, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(MV.params(cam, **bad_later)), 1 << 15, (1 << 13) + 1, ptrs) == 1 and b"2^28" in lib.trt_last_error()
        later = dict(min_frames=300, sigma_normal=-1, sigma_depth=-1.0)
        for kw, msg in ((dict(alpha=-0.1), b"alpha"), (dict(alpha=nan), b"alpha"), (dict(depth_tolerance=-1.0), b"depth_tolerance"),
                        (dict(normal_threshold=1.01), b"normal_threshold"), (dict(max_history=0.5), b"max_history"), (dict(flags=1), b"flags"),
                        (dict(flags=R.FIXED | 2), b"flags")):
            assert call(C.byref(MV.params(cam, **dict(later, **kw))), 4, 4, ptrs) == 1 and msg in lib.trt_last_error(), kw
        # trt_reproject's own order among its fields
        assert call(C.byref(MV.params(cam, alpha=2.0, flags=1)), 4, 4, ptrs) == 1 and b"alpha" in lib.trt_last_error()
        assert call(C.byref(MV.params(cam, max_history=0.5, flags=1)), 4, 4, ptrs) == 1 and b"max_history" in lib.trt_last_error()
        # then the new fields, in theirs
        for kw, msg in ((dict(min_frames=-1, sigma_normal=-1, sigma_depth=-1.0), b"min_frames"), (dict(min_frames=256), b"min_frames"),
                        (dict(sigma_normal=-1, sigma_depth=-1.0), b"sigma_normal"), (dict(sigma_normal=257, sigma_depth=nan), b"sigma_normal"),
                        (dict(sigma_depth=-1.0), b"sigma_depth"), (dict(sigma_depth=nan), b"sigma_depth")):
            assert call(C.byref(MV.params(cam, **kw)), 4, 4, ptrs) == 1 and msg in lib.trt_last_error(), kw
    # 16-byte records: the device entry refuses a cv or a mom that is not aligned
    for i in (5, 9, 12, 14):
        off = list(ptrs)
        off[i] = C.cast(C.c_void_p(keep[i].ctypes.data + 4), R.fp)
        assert dev(C.byref(good), 4, 3, off) == 1 and b"aligned" in lib.trt_last_error(), i
        assert dev(C.byref(MV.params(cam, sigma_depth=-1.0)), 4, 3, off) == 1 and b"sigma_depth" in lib.trt_last_error()
    if not _gpu_present():
        # valid arguments reach the device check: no gfx950 here.  prev_point is optional, the history all or none
        for bufs in (ptrs, ptrs[:4] + [None] + ptrs[5:], ptrs[:5] + [None] * 5 + ptrs[10:], ptrs[:4] + [None] * 6 + ptrs[10:]):
            for p in (good, MV.params(cam, alpha=1.0, max_history=1.0, flags=R.FIXED, min_frames=255, sigma_normal=256, sigma_depth=0.0)):
                for call in (host, dev):
                    assert call(C.byref(p), 4, 4, bufs) == 4
    # the CPU build refuses the same arguments and takes the same ones
    assert cpu(C.byref(MV.params(cam, min_frames=256)), 4, 4, ptrs) == 1
    assert cpu(C.byref(good), 4, 4, ptrs[:5] + [None] + ptrs[6:]) == 1
    assert cpu(C.byref(good), 4, 4, ptrs) == 0 and cpu(C.byref(good), 4, 4, ptrs[:4] + [None] * 6 + ptrs[10:]) == 0


def test_defaults_are_filled_in():
    cam = R.plane_camera(0.0, 0.0, 4, 4)
    out = (C.c_float * 4)()
    assert MV.lib().moments_cpu_defaults(C.byref(MV.params(cam, min_frames=0, sigma_normal=0, sigma_depth=0.0, alpha=0.0)), out) == 0
    assert list(out) == [4.0, 128.0, 1.0, np.float32(0.2)]
    assert MV.lib().moments_cpu_defaults(C.byref(MV.params(cam, min_frames=7, sigma_normal=3, sigma_depth=2.5, alpha=0.5)), out) == 0
    assert list(out) == [7.0, 3.0, 2.5, 0.5]
    # zeros and the written-out defaults are the same call
    cur, hist = MV.random_frames(12, 10, 3)
    a = MV.cpu(*cur, cam, cam, hist, min_frames=0, sigma_normal=0, sigma_depth=0.0, alpha=0.0, depth_tolerance=0.0, normal_threshold=0.0, max_history=0.0)
    b = MV.cpu(*cur, cam, cam, hist)
    assert all(_bits(a[k], b[k]) for k in MV.OUT_KEYS)


def test_python_layer_checks_shapes_and_parameters():
    cur, hist = MV.random_frames(6, 5, 14)
    cam = R.plane_camera(0.0, 0.0, 5, 6)
    with pytest.raises(T.TrtError, match="color"):
        T.reproject_moments(cur[0][..., :2], *cur[1:], cam)
    with pytest.raises(T.TrtError, match="albedo"):
        T.reproject_moments(cur[0], cur[1][:, :4], *cur[2:], cam)
    with pytest.raises(T.TrtError, match="depth"):
        T.reproject_moments(*cur[:3], cur[3][None], cam)
    with pytest.raises(T.TrtError, match="prev_point"):
        T.reproject_moments(*cur, cam, prev_point=cur[0][:3])
    with pytest.raises(T.TrtError, match="history"):
        T.reproject_moments(*cur, cam, history={k: hist[k] for k in R.HISTORY_KEYS})  # reproject()'s history lacks mom
    with pytest.raises(T.TrtError, match="history mom"):
        T.reproject_moments(*cur, cam, history=dict(hist, mom=hist["mom"][..., :3]))
    with pytest.raises(T.TrtError, match="min_frames"):
        T.reproject_moments(*cur, cam, history=hist, min_frames=1000)
    with pytest.raises(T.TrtError, match="sigma_depth"):
        T.reproject_moments(*cur, cam, sigma_depth=-2.0)
    with pytest.raises(T.TrtError, match="alpha"):
        T.reproject_moments(*cur, cam, alpha=1.5)
    with pytest.raises(T.TrtError, match="reproject_moments_into"):
        T.reproject_moments_into(*cur, cam, None, None, None, None, None, None)
    # the accumulator: "samples" is the default and keeps its floor of two samples; "moments" takes one
    one = T.make_params(16, 12, 1, 1)
    with pytest.raises(T.TrtError, match="spp must be >= 2"):
        T.TemporalAccumulator(None, one)
    with pytest.raises(T.TrtError, match="spp must be >= 2"):
        T.TemporalAccumulator(None, one, variance="samples")
    with pytest.raises(T.TrtError, match="variance"):
        T.TemporalAccumulator(None, one, variance="history")
    with pytest.raises(T.TrtError, match="whole image"):
        T.TemporalAccumulator(None, T.make_params(16, 12, 1, 1, tile=(0, 0, 8, 12)), variance="moments")
    with pytest.raises(T.TrtError, match="interleave"):
        T.TemporalAccumulator(None, T.make_params(16, 12, 1, 1, rows=(2, 3, 1)), variance="moments")
    acc = T.TemporalAccumulator(None, one, variance="moments", min_frames=3, sigma_depth=2.0, iterations=3)
    assert acc.variance == "moments" and acc.moments_kw == {"min_frames": 3, "sigma_depth": 2.0} and acc.denoise_kw == {"sigma_depth": 2.0, "iterations": 3}
    assert T.TemporalAccumulator(None, T.make_params(16, 12, 2, 1)).variance == "samples"


def test_moments_symbols_are_declared_exported_and_mirrored():
    hip = C.CDLL(os.path.join(_abi.LIB_DIR, "libtrt_hip.so"))
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    for n in ("trt_reproject_moments", "trt_reproject_moments_device"):
        assert hasattr(hip, n) and n in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + n + r"\(", text)
    assert C.sizeof(_abi.MomentsParams) == C.sizeof(_abi.ReprojectParams) + 12
    fields = re.search(r"typedef struct trt_moments_params \{(.*?)\} trt_moments_params;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields)) == [f[0] for f in _abi.MomentsParams._fields_]
    for k in ("reproject_moments", "reproject_moments_into"):
        assert hasattr(T, k)
