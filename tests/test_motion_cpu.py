"""trt_reproject_motion and trt_trace_points without a GPU: the ABI; the link to trt_reproject (the point that entry forms itself gives its
bits); the CPU build of the per-pixel code (tests/motion) against a float64 restatement (tests/motion_ref.py) on points displaced by a
smooth field; surfaces that move by whole pixels under a still camera; hostile points; the argument checks of the C entries and of the
Python layer; T.center_rays against step 3 in float64, and the points' independence of the direction's length."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import motion_ref as M
import reproject_ref as R
import test_reproject_cpu as TR
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [0, R.FIXED]
NEW = ("trt_trace_points", "trt_trace_points_device", "trt_reproject_motion", "trt_reproject_motion_device")


def _bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


def test_motion_symbols_are_declared_exported_and_mirrored():
    hip = C.CDLL(os.path.join(_abi.LIB_DIR, "libtrt_hip.so"))
    hip.trt_abi_version.restype = C.c_int
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    for n in NEW:
        assert hasattr(hip, n) and n in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + n + r"\(", text)
        assert getattr(_abi.load_hip(), n).argtypes
    assert re.search(r"#define TRT_ABI_VERSION 5\b", text) and _abi.TRT_ABI_VERSION == 5 and hip.trt_abi_version() == 5
    for k in ("center_rays", "reproject_motion", "reproject_motion_into"):
        assert hasattr(T, k)
    assert hasattr(T.Renderer, "trace_points") and hasattr(T.Renderer, "trace_points_into")


# ---- the link to trt_reproject ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", GRIDS)
@pytest.mark.parametrize("h,w", [(24, 32), (33, 17), (1, 13), (13, 1)])
def test_the_point_trt_reproject_forms_gives_its_bits(h, w, flags):
    """prev_point = cur.eye + (d / |d|) depth in fp32, trt_rp_project's order: trt_reproject_motion IS trt_reproject for cameras that differ.
    The link holds where z' = |prev_point - prev.eye| is finite in fp32, as it is here and wherever the cameras are less than 1.8e19 apart.
    The two sides differ on purpose beyond that: trt_rp_project lets an infinite z' through, and the tap test `|inf - zq| <= tol * inf' then
    passes; trt_rp_project_point refuses it, so that a hostile point of 1e38 has no history (test_hostile_points_give_no_history).  Neither
    side is to be `fixed' to match the other: trt_reproject's behaviour is pinned by its own tests, the motion entry's by the issue."""
    (cur, hist), (cam, pcam) = R.random_frames(h, w, 600 + h), R.nearby_cameras(w, h, 600 + w)
    assert bytes(cam) != bytes(pcam)
    P = M.pixel_points(cam, w, h, cur[4], flags)
    for kw in ({}, dict(alpha=0.05, depth_tolerance=0.12, normal_threshold=0.8, max_history=6.0)):
        want = R.cpu(*cur, cam, pcam, hist, flags=flags, **kw)
        got = M.cpu(*cur, P, cam, pcam, hist, flags=flags, **kw)
        for k in R.OUT_KEYS:
            assert _bits(got[k], want[k]), k
        if h * w >= 500 or flags:
            assert (want["length"] > 1).any()  # a history is used: the equality is not one of two pass-throughs
    none = M.cpu(*cur, P, cam, pcam, None, flags=flags)
    want = R.cpu(*cur, cam, pcam, None, flags=flags)
    assert all(_bits(none[k], want[k]) for k in R.OUT_KEYS)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
# test_reproject_cpu.py's rule and its reasoning: RTOL = 5e-5 off the edges, at most 5 % of the hit pixels on an edge.  The chain from v to
# (fx, fy) is the same one, shorter by the ten operations that form the point.
SIZES = [(24, 32), (33, 17), (1, 1), (1, 13), (13, 1)]
# chosen by the restatement alone: the first seed from 500 on whose edge share is within bounds, whose history is used by 20 .. 98 % of the
# hit pixels at 500 pixels or more and, on single-row images of the fixed grid, used at all (see _seed_ok)
SEEDS = {(1, 1, R.FIXED): 507}


def _case(h, w, flags, seed):
    (cur, hist), (cam, pcam) = R.random_frames(h, w, seed, miss_frac=0.1 if h * w > 1 else 0.0), R.nearby_cameras(w, h, seed)
    # the surface's previous place: the moved-camera point, displaced by up to 3 pixel footprints
    return cur, hist, cam, pcam, M.smooth_field_points(cam, w, h, cur[4], flags, seed, footprints=3.0)


def _seed_ok(h, w, flags, seed):
    """What the restatement alone says of a seed (no code under test): edge share and share of hit pixels with history, for both parameter sets."""
    cur, hist, cam, pcam, P = _case(h, w, flags, seed)
    hit = cur[4] < R.INF
    for kw in ({}, dict(alpha=0.05, depth_tolerance=0.12, normal_threshold=0.8, max_history=6.0)):
        want = M.restate(*cur, P, cam, pcam, hist, flags=flags, **kw)
        share = want["edge"][hit].mean() if hit.any() else 0.0
        used = (want["length"] > 1)[hit].mean() if hit.any() else 0.0
        if share > TR.MAX_EDGE_SHARE or (h * w >= 500 and not 0.2 < used < 0.98) or (h * w < 500 and flags and not used > 0):
            return False
    return True


@pytest.mark.parametrize("flags", GRIDS)
@pytest.mark.parametrize("h,w", SIZES)
def test_cpu_build_matches_the_float64_restatement(h, w, flags):
    seed = SEEDS.get((h, w, flags), 500)
    # the seed is the first from 500 on that the restatement accepts
    assert _seed_ok(h, w, flags, seed) and not any(_seed_ok(h, w, flags, k) for k in range(500, seed))
    cur, hist, cam, pcam, P = _case(h, w, flags, seed)
    for kw in ({}, dict(alpha=0.05, depth_tolerance=0.12, normal_threshold=0.8, max_history=6.0)):
        got = M.cpu(*cur, P, cam, pcam, hist, flags=flags, **kw)
        want = M.restate(*cur, P, cam, pcam, hist, flags=flags, **kw)
        hit = cur[4] < R.INF
        edge = want["edge"]
        share = edge[hit].mean() if hit.any() else 0.0
        used = (want["length"] > 1)[hit].mean() if hit.any() else 0.0
        print(f"{h}x{w} flags {flags} {kw}: {int(hit.sum())} hit pixels, {used:.2f} with history, {share:.3f} on an edge")
        assert share <= TR.MAX_EDGE_SHARE
        if h * w >= 500:
            assert 0.2 < used < 0.98  # the case exercises both outcomes
        elif flags:
            assert used > 0
        for k in R.OUT_KEYS:
            g, wn = got[k].astype(np.float64)[~edge], want[k][~edge]
            assert np.isfinite(g).all()
            scale = np.abs(wn).max(axis=0, initial=0.0)
            assert (np.abs(g - wn) <= TR.RTOL * (np.abs(wn) + scale)).all(), k
        none = ~edge & (want["length"] == 1)
        assert _bits(got["color"][none], cur[0][none]) and _bits(got["variance"][none], cur[1][none]) and (got["length"][none] == 1).all()
    # the displacement matters: the undisplaced points give another image
    same = M.cpu(*cur, M.pixel_points(cam, w, h, cur[4], flags), cam, pcam, hist, flags=flags)
    if h * w >= 500:
        assert not _bits(same["cv"], got["cv"])


@pytest.mark.parametrize("flags", GRIDS)
def test_the_two_restatements_agree_on_the_point_trt_reproject_forms(flags):
    """motion_ref.restate writes reproject_ref.restate's tap loop, edge flags and blend out again (that function takes no points and may
    not change).  So that the two cannot drift apart unnoticed: on the float64 point eye + depth d / |d| and differing cameras they must
    give the same results and the same edge flags."""
    h, w = 24, 32
    (cur, hist), (cam, pcam) = R.random_frames(h, w, 500), R.nearby_cameras(w, h, 500)
    eye, d = M.center_rays64(cam, w, h, flags)
    d = d.reshape(h, w, 3)
    z = cur[4].astype(np.float64)
    P = np.where((z < R.INF)[..., None], eye + z[..., None] * d / np.linalg.norm(d, axis=2, keepdims=True), np.nan)
    for kw in ({}, dict(alpha=0.05, depth_tolerance=0.12, normal_threshold=0.8, max_history=6.0)):
        a, b = M.restate(*cur, P, cam, pcam, hist, flags=flags, **kw), R.restate(*cur, cam, pcam, hist, flags=flags, **kw)
        assert (b["length"] > 1).any() and np.array_equal(a["edge"], b["edge"])
        for k in R.OUT_KEYS:
            np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=0.0, err_msg=k)


def test_point_projection_matches_the_restatement():
    w, h = 40, 30
    cam, pcam = R.nearby_cameras(w, h, 3)
    rng = np.random.default_rng(4)
    for flags in GRIDS:
        for prev in (pcam, cam):  # byte-identical cameras are no special case
            p = R.params(cam, prev, flags=flags)
            peye, pllc, phor, pver = R.camera_arrays(prev)
            for _ in range(6):
                P = rng.uniform(-3.0, 3.0, 3).astype(np.float32).astype(np.float64)
                k, a, b = np.linalg.solve(np.stack([pllc - peye, phor, pver], axis=1), P - peye)
                fx, fy = ((a / k) * w - 0.5, (h - 0.5) - (b / k) * h) if flags else ((a / k) * (w - 1), h - (b / k) * (h - 1))
                got = M.project_point(p, w, h, P)
                assert k > 0 and got is not None
                np.testing.assert_allclose(got, (fx, fy, np.linalg.norm(P - peye)), rtol=1e-5, atol=2e-4)


# ---- surfaces that move under a still camera ----------------------------------------------------------------------------------------------

def _own_points(cam, w, h, dist, flags):
    """The world points a plane_camera sees on the plane z = -dist, float64 [h, w, 3]."""
    eye, d = M.center_rays64(cam, w, h, flags)
    d = d.reshape(h, w, 3)
    return eye + d * (dist / -d[..., 2:3])


@pytest.mark.parametrize("flags", GRIDS)
@pytest.mark.parametrize("kx,ky", [(1, 0), (0, -2), (3, 2)])
def test_surface_moved_by_whole_pixels_shifts_a_ramp(kx, ky, flags):
    """A still camera on a fronto-parallel plane whose surface moved right by kx and up by ky pixel footprints since the history frame:
    prev_point = the pixel's own point - (kx px, ky py, 0).  What pixel (x, y) shows now, the previous frame showed kx columns further
    left and ky rows further DOWN (rows run top to bottom): a ramp stored in prev_cv comes out shifted by (kx, ky), from (x - kx, y + ky).
    The tolerance is test_camera_moved_by_whole_pixels_shifts_a_ramp's.  trt_reproject on the same frames, its cameras byte-identical,
    takes every pixel's history from the pixel itself."""
    w, h, dist = 28, 20, 4.0
    px, py = R.pixel_footprint(w, h, dist, flags)
    cam = R.plane_camera(0.3, -0.2, w, h)
    frame = TR._plane_frame(w, h, dist, flags)
    cv, length = TR._ramps(w, h)
    hist = {"cv": R._f32(cv), "length": R._f32(length), "normal": frame[3], "depth": frame[4]}
    P = (_own_points(cam, w, h, dist, flags) - np.array([kx * px, ky * py, 0.0])).astype(np.float32)
    got = M.cpu(*frame, P, cam, cam, hist, flags=flags, alpha=0.1, max_history=1e6)
    yy, xx = np.mgrid[0:h, 0:w]

    def expect(sx, sy):
        ch = np.stack([0.1 + 0.01 * sx + 0.02 * sy, 0.5 - 0.005 * sx + 0.01 * sy, 0.2 + 0.02 * sx - 0.004 * sy, 1e-3 + 1e-5 * sx + 2e-5 * sy], axis=2)
        n = 2.0 + 0.5 * sx + 0.25 * sy + 1.0
        al = np.maximum(0.1, 1.0 / n)
        c = frame[0].astype(np.float64) / 0.5
        return ch[..., :3] + al[..., None] * (c - ch[..., :3]), al ** 2 * (2e-3 / 0.5 ** 2) + (1 - al) ** 2 * ch[..., 3], n

    sx, sy = xx - kx, yy + ky
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    outside = (sx <= -1) | (sx >= w) | (sy <= -1) | (sy >= h)
    assert inside.sum() > w * h // 2 and outside.any()
    want_c, want_v, n = expect(sx, sy)
    np.testing.assert_allclose(got["length"][inside], n[inside], rtol=1e-4)
    np.testing.assert_allclose(got["cv"][..., :3][inside], want_c[inside], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(got["cv"][..., 3][inside], want_v[inside], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(got["color"][inside], (want_c * 0.5)[inside], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(got["variance"][inside], (want_v * 0.25)[inside], rtol=1e-4, atol=1e-8)
    assert (got["length"][outside] == 1).all()
    assert _bits(got["color"][outside], frame[0][outside]) and _bits(got["variance"][outside], frame[1][outside])
    # history length 2 wherever the source is inside the image, on a history of first frames
    two = M.cpu(*frame, P, cam, cam, dict(hist, length=np.ones((h, w), np.float32)), flags=flags)
    assert (two["length"][inside] == 2).all() and (two["length"][outside] == 1).all()
    # the same frames through trt_reproject come out unshifted
    still = R.cpu(*frame, cam, cam, hist, flags=flags, alpha=0.1, max_history=1e6)
    own_c, _, own_n = expect(xx, yy)
    np.testing.assert_allclose(still["length"], own_n, rtol=1e-6)
    np.testing.assert_allclose(still["cv"][..., :3], own_c, rtol=1e-5, atol=1e-6)
    assert not np.allclose(still["length"][inside], n[inside], rtol=1e-4)


@pytest.mark.parametrize("flags", GRIDS)
def test_still_camera_does_not_take_the_shortcut(flags):
    """Byte-identical cameras: trt_reproject reads each pixel's own history whatever its depth buffer says; trt_reproject_motion goes by
    the points.  With the pixel's own points it finds (nearly) the pixel itself — by arithmetic, so the depth it tests is |v|, not the
    depth buffer's value —, with points one footprint to the right the neighbour's history, and `cur` does not enter at all."""
    w, h, dist = 28, 20, 4.0
    px, _ = R.pixel_footprint(w, h, dist, flags)
    cam = R.plane_camera(0.3, -0.2, w, h)
    frame = TR._plane_frame(w, h, dist, flags)
    cv, length = TR._ramps(w, h)
    hist = {"cv": R._f32(cv), "length": R._f32(length), "normal": frame[3], "depth": frame[4]}
    own = _own_points(cam, w, h, dist, flags)
    p = R.params(cam, cam, flags=flags)
    for x, y in ((0, 0), (5, 7), (27, 19)):
        fx, fy, zp = M.project_point(p, w, h, own[y, x])
        assert abs(fx - x) < 1e-3 and abs(fy - y) < 1e-3 and abs(zp - frame[4][y, x]) < 1e-5 * zp
        fx1, _, _ = M.project_point(p, w, h, own[y, x] + [px, 0.0, 0.0])
        assert abs(fx1 - (x + 1)) < 1e-3
    a = M.cpu(*frame, own.astype(np.float32), cam, cam, hist, flags=flags, alpha=0.1, max_history=1e6)
    shortcut = R.cpu(*frame, cam, cam, hist, flags=flags, alpha=0.1, max_history=1e6)
    np.testing.assert_allclose(a["length"], shortcut["length"], rtol=1e-4)
    # a depth buffer that is wrong everywhere: the shortcut still passes its own pixel (z' = depth), the points do not lie
    far = list(frame)
    far[4] = frame[4] * np.float32(1.5)
    assert (R.cpu(*far, cam, cam, dict(hist, depth=far[4]), flags=flags)["length"] > 1).all()
    assert (M.cpu(*far, own.astype(np.float32), cam, cam, dict(hist, depth=far[4]), flags=flags)["length"] == 1).all()
    # cur is not used
    other = R.nearby_cameras(w, h, 9)[0]
    b = M.cpu(*frame, own.astype(np.float32), other, cam, hist, flags=flags, alpha=0.1, max_history=1e6)
    assert all(_bits(a[k], b[k]) for k in R.OUT_KEYS)


# ---- hostile points ----------------------------------------------------------------------------------------------------------------------

def test_hostile_points_give_no_history():
    w, h = 12, 9
    cur, hist = R.random_frames(h, w, 41, miss_frac=0.0)
    cam, pcam = R.nearby_cameras(w, h, 41)
    peye, pllc, phor, pver = R.camera_arrays(pcam)
    centre = pllc + 0.5 * phor + 0.5 * pver
    good = M.pixel_points(cam, w, h, cur[4], 0)
    nan, inf = float("nan"), float("inf")
    hostile = [np.full(3, nan), np.full(3, inf), np.full(3, -inf), np.full(3, 1e38), np.full(3, -1e38), np.array([nan, 0.0, 0.0]),
               np.array([0.0, inf, 0.0]), np.array([0.0, 0.0, 1e38]),
               peye - 5.0 * (centre - peye),  # behind the previous eye
               peye]  # on it
    bad_prev = _abi.Camera.from_buffer_copy(pcam)
    bad_prev.horizontal = _abi.c_float3(0.0, 0.0, 0.0)
    for flags in GRIDS:
        assert (M.cpu(*cur, M.pixel_points(cam, w, h, cur[4], flags), cam, pcam, hist, flags=flags)["length"] > 1).any()  # honest points do find it
        for v in hostile:
            P = np.broadcast_to(v.astype(np.float32), (h, w, 3))
            out = M.cpu(*cur, P, cam, pcam, hist, flags=flags)
            assert (out["length"] == 1).all() and _bits(out["color"], cur[0]) and _bits(out["variance"], cur[1]), v
            assert M.project_point(R.params(cam, pcam, flags=flags), w, h, v) is None
        # one hostile point among honest ones touches its own pixel only
        P = M.pixel_points(cam, w, h, cur[4], flags)
        base = M.cpu(*cur, P, cam, pcam, hist, flags=flags)
        y, x = np.argwhere(base["length"] > 1)[0]
        P2 = P.copy()
        P2[y, x] = nan
        out = M.cpu(*cur, P2, cam, pcam, hist, flags=flags)
        diff = out["length"] != base["length"]
        assert diff[y, x] and diff.sum() == 1 and out["length"][y, x] == 1
        # a degenerate previous camera: no history anywhere
        out = M.cpu(*cur, good, cam, bad_prev, hist, flags=flags)
        assert (out["length"] == 1).all() and _bits(out["color"], cur[0])


# ---- the C ABI and the Python layer -----------------------------------------------------------------------------------------------------

def _entry_args(w=4, h=4):
    shapes = [(h, w, 3), (h, w), (h, w, 3), (h, w, 3), (h, w), (h, w, 3), (h, w, 4), (h, w), (h, w, 3), (h, w), (h, w, 3), (h, w), (h, w, 4), (h, w)]
    bufs = [np.zeros(s, np.float32) for s in shapes]
    return bufs, [b.ctypes.data_as(R.fp) for b in bufs]


def test_reproject_motion_entries_check_their_arguments_before_the_device():
    lib = _abi.load_hip()
    keep, ptrs = _entry_args()
    cam = R.plane_camera(0.0, 0.0, 4, 4)
    good = R.params(cam)

    def host(p, w, h, bufs):
        return lib.trt_reproject_motion(0, p, w, h, *bufs, None)

    def dev(p, w, h, bufs):
        return lib.trt_reproject_motion_device(0, p, w, h, *[C.cast(b, C.c_void_p) if b else None for b in bufs], None, None)

    nan = float("nan")
    for call in (host, dev):
        no_point = list(ptrs)
        no_point[5] = None
        assert call(C.byref(good), 4, 4, no_point) == 1 and b"null buffer" in lib.trt_last_error()
        # then trt_reproject's list, in its order
        assert call(None, 4, 4, ptrs) == 1 and b"null params" in lib.trt_last_error()
        assert call(None, 4, 4, no_point) == 1 and b"null params" in lib.trt_last_error()
        for i in (0, 1, 2, 3, 4, 10, 11, 12, 13):
            bufs = list(ptrs)
            bufs[i] = None
            assert call(C.byref(good), 4, 4, bufs) == 1 and b"null buffer" in lib.trt_last_error()
        for missing in ((6,), (7,), (8,), (9,), (6, 7), (7, 8, 9), (6, 9)):
            bufs = list(ptrs)
            for i in missing:
                bufs[i] = None
            assert call(C.byref(good), 4, 4, bufs) == 1 and b"partial history" in lib.trt_last_error()
        bufs = list(ptrs)
        bufs[5], bufs[6] = None, None  # a null buffer comes before a partial history
        assert call(C.byref(good), 4, 4, bufs) == 1 and b"null buffer" in lib.trt_last_error()
        assert call(C.byref(good), 0, 4, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(good), 4, -3, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(good), 1 << 15, (1 << 13) + 1, ptrs) == 1 and b"2^28" in lib.trt_last_error()
        for kw, msg in ((dict(alpha=-0.1), b"alpha"), (dict(alpha=nan), b"alpha"), (dict(depth_tolerance=-1.0), b"depth_tolerance"),
                        (dict(normal_threshold=1.01), b"normal_threshold"), (dict(max_history=0.5), b"max_history"), (dict(flags=1), b"flags"),
                        (dict(flags=R.FIXED | 2), b"flags")):
            assert call(C.byref(R.params(cam, **kw)), 4, 4, ptrs) == 1 and msg in lib.trt_last_error(), kw
        assert call(C.byref(R.params(cam, alpha=2.0, flags=1)), 4, 4, ptrs) == 1 and b"alpha" in lib.trt_last_error()  # in trt_reproject's order
    off = list(ptrs)
    off[12] = C.cast(C.c_void_p(keep[12].ctypes.data + 4), R.fp)
    assert dev(C.byref(good), 4, 3, off) == 1 and b"aligned" in lib.trt_last_error()
    if not TR._gpu_present():
        no_hist = ptrs[:6] + [None] * 4 + ptrs[10:]
        for call in (host, dev):
            assert call(C.byref(good), 4, 4, ptrs) == 4  # valid arguments reach the device check: no gfx950 here
            assert call(C.byref(good), 4, 4, no_hist) == 4
    # the CPU build refuses the same arguments
    assert M.lib().reproject_motion_cpu(C.byref(good), 4, 4, *(ptrs[:5] + [None] + ptrs[6:])) == 1
    assert M.lib().reproject_motion_cpu(C.byref(R.params(cam, alpha=2.0)), 4, 4, *ptrs) == 1
    assert M.lib().reproject_motion_cpu(C.byref(good), 4, 4, *ptrs) == 0


def test_trace_points_entries_refuse_null_arguments():
    """Without a handle there is nothing to trace on: a null handle or array is TRT_EINVAL from both entries (the other checks need a
    handle: tests/test_gpu_motion.py)."""
    lib = _abi.load_hip()
    a = np.zeros((4, 3), np.float32)
    v = np.zeros((2, 3, 3), np.float32)
    p = a.ctypes.data_as(R.fp)
    assert lib.trt_trace_points(None, 4, p, p, v.ctypes.data_as(R.fp), 2, p, None) == 1 and b"null argument" in lib.trt_last_error()
    assert lib.trt_trace_points_device(None, 4, a.ctypes.data, a.ctypes.data, v.ctypes.data, 2, a.ctypes.data, None, None) == 1
    assert b"trt_trace_points_device: null argument" in lib.trt_last_error()


def test_python_motion_wrappers_check_shapes_and_dtypes():
    cur, hist = R.random_frames(6, 5, 14)
    cam = R.plane_camera(0.0, 0.0, 5, 6)
    P = np.zeros((6, 5, 3), np.float32)
    with pytest.raises(T.TrtError, match="color"):
        T.reproject_motion(cur[0][..., :2], *cur[1:], P, cam)
    with pytest.raises(T.TrtError, match="depth"):
        T.reproject_motion(*cur[:4], cur[4][None], P, cam)
    with pytest.raises(T.TrtError, match="prev_point"):
        T.reproject_motion(*cur, P[..., :2], cam)
    with pytest.raises(T.TrtError, match="prev_point"):
        T.reproject_motion(*cur, P[:5], cam)
    with pytest.raises(T.TrtError, match="prev_point"):
        T.reproject_motion(*cur, None, cam)
    with pytest.raises(T.TrtError, match="history cv"):
        T.reproject_motion(*cur, P, cam, history=dict(hist, cv=hist["cv"][..., :3]))
    with pytest.raises(T.TrtError, match="alpha"):
        T.reproject_motion(*cur, P, cam, history=hist, alpha=1.5)
    with pytest.raises(T.TrtError, match="reproject_motion_into"):
        T.reproject_motion_into(*cur, P, cam, None, None, None, None, None)
    r = T.Renderer.__new__(T.Renderer)  # no handle: the checks of the wrappers come before any call
    r._h = None
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(T.TrtError, match="tri_v_other"):
        r.trace_points(o, o, np.zeros((7, 3), np.float32))
    with pytest.raises(T.TrtError, match="length mismatch"):
        r.trace_points(o, o[:3], np.zeros((2, 3, 3), np.float32))
    with pytest.raises(T.TrtError, match="trace_points_into"):
        r.trace_points_into(o, o, np.zeros((2, 3, 3), np.float32), o)
    with pytest.raises(T.TrtError, match="width and height"):
        T.center_rays(cam, 0, 4)
    acc = T.TemporalAccumulator(None, T.make_params(16, 12, 4, 1))
    for bad in (np.zeros((10, 3), np.float32), np.zeros((10, 3, 2), np.float32), np.zeros((3, 3), np.float32)):
        with pytest.raises(T.TrtError, match="moved_from"):
            acc.frame(cam, moved_from=bad)
    assert acc.frame_index == 0


# ---- T.center_rays --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", GRIDS)
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (37, 53)])
def test_center_rays_are_step_3_in_fp32(h, w, flags):
    """dir = ((llc + horizontal s) + vertical t) - eye: three rounded operations behind a rounded product each, every intermediate no
    larger than a few times the largest camera component M; each rounding is at most half an ulp of that, so 4 ulp(M) bounds the chain."""
    for cam in (R.nearby_cameras(w, h, 7)[0], R.orbit_camera("back", 3.0, w, h)):
        org, d = T.center_rays(cam, w, h, flags)
        assert org.dtype == d.dtype == np.float32 and org.shape == d.shape == (h * w, 3)
        eye, want = M.center_rays64(cam, w, h, flags)
        assert _bits(org, np.broadcast_to(eye.astype(np.float32), (h * w, 3)))
        big = max(np.abs(a).max() for a in R.camera_arrays(cam))
        tol = 4 * np.spacing(np.float32(big))
        if (w == 1 or h == 1) and not flags:  # the reference's grid divides by W - 1 and H - 1: not a number on either side
            assert not np.isfinite(want).all() and (np.isfinite(d) == np.isfinite(want)).all()
        else:
            assert np.isfinite(d).all() and np.abs(d - want).max() <= tol


def test_points_do_not_depend_on_the_directions_length(scene_factory):
    """back's 53 x 37 centre rays through the oracle's closest hit and the CPU build of hitPoint, for dir and 2 dir: the same triangles,
    and points that differ by the rounding of (u, v) alone — a few ulp of the barycentrics times the triangle's size."""
    import oracle_lib as O
    w, h = 53, 37
    s = scene_factory("back", w, h)
    v = s.arrays()["tri_v"]
    cam = T.Camera.from_buffer_copy(s.flat.contents.camera)
    org, d = T.center_rays(cam, w, h, R.FIXED)
    t1, tri1, uv1 = O.trace(s.flat, org, d)
    t2, tri2, uv2 = O.trace(s.flat, org, (d * np.float32(2.0)).astype(np.float32))
    assert np.array_equal(tri1, tri2) and (tri1 >= 0).sum() > w * h // 3 and (tri1 < 0).any()
    p1, p2 = M.hit_points(v, tri1, uv1), M.hit_points(v, tri2, uv2)
    assert _bits(p1, M.hit_points_np(v, tri1, uv1)) and _bits(p2, M.hit_points_np(v, tri2, uv2))  # the CPU build is the formula, bit for bit
    hit = tri1 >= 0
    assert (p1[~hit].view(np.uint32) == M.NAN_BITS).all()
    size = np.abs(v).max()
    assert np.abs(p1[hit] - p2[hit]).max() <= 64 * np.spacing(np.float32(size))
    # and they lie on the rays: org + t dir, to 1e-4 relative
    on_ray = org[hit].astype(np.float64) + t1[hit, None].astype(np.float64) * d[hit].astype(np.float64)
    assert (np.linalg.norm(p1[hit] - on_ray, axis=1) <= 1e-4 * np.maximum(1.0, np.linalg.norm(on_ray, axis=1))).all()
