"""Motion vectors on the MI355X.  trt_trace_points gives, bit for bit, include/trt.h's formula on trt_trace_closest's (tri, u, v), on the
wave-uniform walk with 8-byte hit records and on both per-lane node kinds; its device entry gives the host entry's bits on a side stream
and writes nothing past its output.  trt_reproject_motion gives the bits of the CPU build of its per-pixel code (tests/motion) on random
frames of any size and on two rendered frames of back between which the inner object moved.  The history follows a surface that moved
under a still camera, where trt_reproject reads the history of whatever used to be at the pixel.  TemporalAccumulator.frame(moved_from=)
is the public pieces in a row, bit for bit, and an animated sequence keeps its history on the moving object."""
import ctypes as C
import re

import numpy as np
import pytest

import motion_ref as M
import raygen
import refit_ref as RR
import reproject_ref as R
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu

KEYS = ("color", "variance", "albedo", "normal", "depth")
W, H = 53, 37
# scene, the environment at trt_create, the node size its traversal reports, whether its hit records are the 8-byte ones
HANDLES = {"back": ({}, 64, "1"), "staircase": ({"TRT_NODE_KIND": "0"}, 128, "0"), "soup": ({"TRT_NODE_KIND": "1"}, 80, "0")}
_handles = {}


def _scene(name):
    return get_scene("soup", W, H, n=20000) if name == "soup" else get_scene(name, W, H)


@pytest.fixture(scope="module")
def handles():
    """Renderers of this module's own (geometry is never updated on them), created once: name -> (renderer, hit8 as trt_create reported it)."""
    yield _handles
    for r, _ in _handles.values():
        r.close()
    _handles.clear()


def _handle(name, handles, capfd, monkeypatch):
    if name not in handles:
        env = dict(HANDLES[name][0], TRT_DEBUG="1")
        capfd.readouterr()
        with monkeypatch.context() as m:
            for k in ("TRT_SLIM_WALK", "TRT_BIN_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND"):
                m.delenv(k, raising=False)
            for k, v in env.items():
                m.setenv(k, v)
            r = T.Renderer(_scene(name), 0)
        got = re.findall(r"trt_create: slim walk \d, 8-byte hit records (\d)", capfd.readouterr().err)
        assert len(got) == 1, got
        handles[name] = (r, got[0])
    return handles[name]


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _ray_sets(s):
    lo, hi = raygen.scene_bounds(s)
    o, d = raygen.random_rays(257, lo, hi, seed=21)
    sets = [(o[:n], d[:n]) for n in (1, 63, 64, 65, 257)]
    sets.append(T.center_rays(T.Camera.from_buffer_copy(s.flat.contents.camera), W, H, R.FIXED))
    return sets


# ---- trt_trace_points -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(HANDLES))
def test_trace_points_is_the_formula_on_trace_closest_hits(name, handles, capfd, monkeypatch):
    s = _scene(name)
    r, hit8 = _handle(name, handles, capfd, monkeypatch)
    env, node_bytes, want_hit8 = HANDLES[name]
    v_own = s.arrays()["tri_v"]
    hits = 0
    for o, d in _ray_sets(s):
        t, tri, uv, st = r.trace_closest(o, d, want_stats=True)
        assert st.inner_node_bytes == node_bytes and hit8 == want_hit8, (name, st.inner_node_bytes, hit8)  # which handle is which
        for v_other in (v_own, RR.smooth_displace(v_own)):
            got, pst = r.trace_points(o, d, v_other, want_stats=True)
            want = M.hit_points_np(v_other, tri, uv)
            assert got.dtype == np.float32 and _bits_equal(got, want), f"{name} n={len(o)}: {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())} points differ"
            assert (got[tri < 0].view(np.uint32) == M.NAN_BITS).all() and np.isfinite(got[tri >= 0]).all()
            assert _bits_equal(got, M.hit_points(v_other, tri, uv))  # and the CPU build of hitPoint
            # the stats are trt_trace_closest's
            assert pst.launches[1] == 1 and sum(pst.launches) == 1 and pst.inner_node_bytes == node_bytes and pst.redo_rays == st.redo_rays
            assert (list(pst.inner_visits), list(pst.tri_tests)) == (list(st.inner_visits), list(st.tri_tests))
        # on the scene's own vertices the point is the hit point
        hit = tri >= 0
        hits += int(hit.sum())
        own = r.trace_points(o, d, v_own)
        on_ray = o[hit].astype(np.float64) + t[hit, None].astype(np.float64) * d[hit].astype(np.float64)
        off = np.linalg.norm(own[hit] - on_ray, axis=1)
        assert (off <= 1e-4 * np.maximum(1.0, np.linalg.norm(own[hit], axis=1))).all(), f"{name}: {off.max()}"
    assert hits > W * H // 4
    # the points do not depend on the direction's length beyond the rounding of (u, v)
    o, d = _ray_sets(s)[-1]
    a, b = r.trace_points(o, d, v_own), r.trace_points(o, (d * np.float32(2.0)).astype(np.float32), v_own)
    both = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    assert (np.isfinite(a).all(axis=1) == np.isfinite(b).all(axis=1)).mean() > 0.99
    assert np.abs(a[both] - b[both]).max() <= 1e-4 * np.abs(v_own).max()


def test_trace_points_checks_its_arguments(handles, capfd, monkeypatch):
    r, _ = _handle("back", handles, capfd, monkeypatch)
    s = _scene("back")
    v = s.arrays()["tri_v"]
    o, d = _ray_sets(s)[2]
    with pytest.raises(T.TrtError, match="n_tris"):
        r.trace_points(o, d, v[:-1])
    with pytest.raises(T.TrtError, match="n_tris"):
        r.trace_points(o[:0], d[:0], v[:-1])  # the triangle count is checked before n == 0 is waved through
    assert r.trace_points(o[:0], d[:0], v).shape == (0, 3)
    lib, fp = r._lib, C.POINTER(C.c_float)
    out = np.empty_like(o)
    args = [o.ctypes.data_as(fp), d.ctypes.data_as(fp), v.ctypes.data_as(fp), len(v), out.ctypes.data_as(fp)]
    assert lib.trt_trace_points(r._h, 0x7FFF0001, *args, None) == 1 and b"too large" in lib.trt_last_error()
    for i in (0, 1, 2, 4):
        bad = list(args)
        bad[i] = None
        assert lib.trt_trace_points(r._h, len(o), *bad, None) == 1 and b"null argument" in lib.trt_last_error()


@pytest.mark.parametrize("name", ["back", "staircase"])
def test_trace_points_device_entry_matches_the_host_entry_on_a_side_stream(name, handles, capfd, monkeypatch):
    import torch
    s = _scene(name)
    r, _ = _handle(name, handles, capfd, monkeypatch)
    dev = torch.device("cuda", 0)
    v_other = RR.smooth_displace(s.arrays()["tri_v"])
    vt = torch.from_numpy(v_other).to(dev)
    side = torch.cuda.Stream(dev)
    sentinel = -12345.0
    for o, d in _ray_sets(s)[3:]:  # 65, 257 and the centre rays
        n = len(o)
        want = r.trace_points(o, d, v_other)
        ot, dt = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        big = torch.full((3 * n + 4096,), sentinel, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        for stream in (None, side):
            big.fill_(sentinel)
            torch.cuda.synchronize(dev)
            if stream is None:
                st = r.trace_points_into(ot, dt, vt, big[: 3 * n].view(n, 3))
            else:
                with torch.cuda.stream(side):
                    st = r.trace_points_into(ot, dt, vt, big[: 3 * n].view(n, 3), stream_ptr=side.cuda_stream)
            assert st.launches[1] == 1 and sum(st.launches) == 1
            got = big.cpu().numpy()
            assert _bits_equal(got[: 3 * n].reshape(n, 3), want) and (got[3 * n:] == sentinel).all()
        for t_, a_ in ((ot, o), (dt, d), (vt, v_other)):  # inputs untouched
            assert t_.cpu().numpy().tobytes() == a_.tobytes()


# ---- trt_reproject_motion against the CPU build -----------------------------------------------------------------------------------------

def _same_bits(cur, P, cam, pcam, hist, **kw):
    got = T.reproject_motion(*cur, P, cam, pcam, history=hist, **kw)
    want = M.cpu(*cur, P, cam, pcam, hist, **kw)
    for k in R.OUT_KEYS:
        same = got[k].view(np.uint32) == want[k].view(np.uint32)
        assert same.all(), f"{k}: {np.count_nonzero(~same)} values differ, first at {np.argwhere(~same)[0]} ({kw})"
    return got


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (29, 1), (16, 16), (17, 33), (64, 80)])
def test_reproject_motion_matches_the_cpu_build_bit_for_bit_on_any_size(h, w):
    cur, hist = R.random_frames(h, w, 2000 + 3 * h + w, miss_frac=0.15 if h * w > 1 else 0.0)
    cam, pcam = R.nearby_cameras(w, h, 2000 + h)
    for flags in (0, R.FIXED):
        P = M.smooth_field_points(cam, w, h, cur[4], flags, 2000 + w, footprints=3.0)
        _same_bits(cur, P, cam, pcam, None, flags=flags)
        got = _same_bits(cur, P, cam, pcam, hist, flags=flags)
        if flags and h * w >= 256:
            assert 0.2 < (got["length"] > 1).mean() < 0.98
        _same_bits(cur, P, cam, pcam, hist, flags=flags, alpha=0.05, depth_tolerance=0.03, normal_threshold=0.97, max_history=5.0)
        _same_bits(cur, P, cam, cam, hist, flags=flags)  # a still camera: no shortcut on either side
        _same_bits(cur, P, cam, pcam, hist, flags=flags, alpha=0.0, depth_tolerance=0.0, normal_threshold=0.0, max_history=0.0)  # zeros = the defaults
        # the link to trt_reproject holds on the GPU too
        link = T.reproject_motion(*cur, M.pixel_points(cam, w, h, cur[4], flags), cam, pcam, history=hist, flags=flags)
        plain = T.reproject(*cur, cam, pcam, history=hist, flags=flags)
        assert all(_bits_equal(link[k], plain[k]) for k in R.OUT_KEYS)


@pytest.fixture(scope="module")
def moved_back():
    """Two rendered 53 x 37 frames of back under its own, still camera, the inner object moved between them (refit_ref.move_inner_object) on
    a renderer and a scene of this fixture's own.  -> dict(cam, prev, cur: the denoiser's inputs of either frame, P: trace_points of the
    centre rays on the first frame's vertices, sel: the moved triangles, tri1: the second frame's centre hits)."""
    s = T.Scene.named("back", W, H)
    r = T.Renderer(s, 0)
    try:
        cam = T.Camera.from_buffer_copy(s.flat.contents.camera)
        v0 = s.arrays()["tri_v"]
        v1, sel = RR.move_inner_object(s)
        frames = []
        for i in range(2):
            if i:
                r.update_geometry(v1)
            d = r.render_camera_denoised(T.make_params(W, H, 8, T.SEED_BACK + i, flags=R.FIXED), cam)
            frames.append(tuple(d[k] for k in KEYS))
        org, dirs = T.center_rays(cam, W, H, R.FIXED)
        P = r.trace_points(org, dirs, v0).reshape(H, W, 3)
        tri1 = r.trace_closest(org, dirs)[1].reshape(H, W)
        yield dict(cam=cam, prev=frames[0], cur=frames[1], P=P, sel=sel, tri1=tri1)
    finally:
        r.close()
        s.close()


def test_reproject_motion_matches_the_cpu_build_on_rendered_frames_of_a_moved_object(moved_back):
    import torch
    m = moved_back
    cam, prev, cur, P = m["cam"], m["prev"], m["cur"], m["P"]
    first = T.reproject(*prev, cam)
    hist = {"cv": first["cv"], "length": first["length"], "normal": prev[3], "depth": prev[4]}
    got = _same_bits(cur, P, cam, cam, hist, flags=R.FIXED)
    _same_bits(cur, P, cam, cam, hist, flags=R.FIXED, alpha=0.05, depth_tolerance=0.03, normal_threshold=0.97, max_history=5.0)
    on_object = (m["tri1"] >= 0) & m["sel"][np.maximum(m["tri1"], 0)]
    hit = cur[4] < R.INF
    print(f"moved back: {int(hit.sum())} hit pixels, {(got['length'][hit] == 2).mean():.2f} found their history; on the moved object "
          f"{int(on_object.sum())} pixels, {(got['length'][on_object] == 2).mean():.2f}")
    assert on_object.sum() > 50 and (got["length"][hit] == 2).mean() > 0.5 and (got["length"][~hit] == 1).all()
    # the device entry: the same bits, nothing past the outputs, inputs untouched
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in cur] + [torch.from_numpy(P).to(dev)]
    hdev = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in hist.items()}
    sentinel = -12345.0
    sizes = {"color": H * W * 3, "variance": H * W, "cv": H * W * 4, "length": H * W}
    big = {k: torch.full((n + 4096,), sentinel, dtype=torch.float32, device=dev) for k, n in sizes.items()}
    outs = [big[k][: sizes[k]].view(got[k].shape) for k in R.OUT_KEYS]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    for history, expect in ((hdev, got), (None, T.reproject_motion(*cur, P, cam, cam, flags=R.FIXED))):
        with torch.cuda.stream(side):
            st = T.reproject_motion_into(*ins, cam, cam, *outs, history=history, flags=R.FIXED, stream_ptr=side.cuda_stream)
        assert st.launches[T.TRT_K_DENOISE] == 1 and sum(st.launches) == 1 and st.rays == 0
        for k in R.OUT_KEYS:
            g = big[k].cpu().numpy()
            assert g[: sizes[k]].tobytes() == expect[k].reshape(-1).tobytes(), k
            assert (g[sizes[k]:] == sentinel).all(), k
    for t_, a_ in list(zip(ins, list(cur) + [P])) + [(hdev[k], hist[k]) for k in hist]:
        assert t_.cpu().numpy().tobytes() == np.ascontiguousarray(a_).tobytes()


# ---- the history follows the surface ----------------------------------------------------------------------------------------------------

def test_history_follows_a_surface_that_moved_under_a_still_camera():
    """back at 64 x 48, its own camera.  Frame 0 on the scene's vertices; the inner object then moves 60 units along x — parallel to the
    image plane, 3.6 to 4 pixel footprints of 15 to 16.5 units at its depth of 1060 to 1320 — and frame 1 follows.  The history's colour
    is frame 0's own position buffer (the centre rays' hit points), its length 1000, the new frame's colour 0 on albedo 1 and alpha 1e-6:
    out_cv.rgb / (1 - 1 / N) is then the bilinear mean of the stored positions of the accepted taps, i.e. WHERE the history was read.
    A pixel qualifies when it found a history and the four taps around its float64-projected source lie on one triangle of frame 0; there
    the mean must lie within twice the largest distance between neighbouring stored positions of that 2 x 2 block from the pixel's
    previous point (a bound taken from frame 0's buffer alone).  Of the pixels whose centre ray hits the object in both frames at least half
    must qualify (on the CPU, with the oracle's hits and the CPU build: 85 of 146, largest error 0.005 of the bound).  The same frames through
    trt_reproject, whose cameras are byte-identical, read each pixel's own history: on the object that is 60 units off, outside the
    bound at every qualifying pixel — without trt_trace_points and trt_reproject_motion this test fails."""
    w, h = 64, 48
    s = T.Scene.named("back", w, h)
    r = T.Renderer(s, 0)
    try:
        v1, sel = M.moved_object(s, (60.0, 0.0, 0.0))
        lo, hi = raygen.scene_bounds(s)
        moved = v1[sel].reshape(-1, 3)
        assert (moved.min(0) > lo).all() and (moved.max(0) < hi).all()  # still inside the room
        res = M.follow_case(r.trace_closest, r.trace_points, r.update_geometry, T.reproject_motion, T.reproject, s, w, h, v1, sel, T.center_rays)
    finally:
        r.close()
        s.close()
    obj, q = res["object"], res["qualify"]
    on = q & obj
    print(f"object pixels {int(obj.sum())}, qualifying {int(on.sum())}; all qualifying pixels {int(q.sum())}; largest error / bound with motion "
          f"{(res['motion_err'][q] / res['tol'][q]).max():.4f}; trt_reproject outside the bound at {int((~(res['still_err'][on] <= res['tol'][on])).sum())} of them")
    assert obj.sum() > 100 and on.sum() >= 0.5 * obj.sum()
    assert q.sum() > 1000 and (res["motion_err"][q] <= res["tol"][q]).all()
    assert not (res["still_err"][on] <= res["tol"][on]).any()  # the contrast: no motion vectors, the wrong place (or no history at all)


# ---- TemporalAccumulator ----------------------------------------------------------------------------------------------------------------

def test_accumulator_with_moved_from_is_the_public_pieces_in_a_row():
    import torch
    W2, H2, spp, seed = 64, 48, 4, 4242
    s = T.Scene.named("back", W2, H2)
    r = T.Renderer(s, 0)
    try:
        cam = T.Camera.from_buffer_copy(s.flat.contents.camera)
        p = T.make_params(W2, H2, spp, seed, flags=R.FIXED)
        v = [s.arrays()["tri_v"]]
        for k in (1, 2, 3):
            v.append(M.moved_object(s, (20.0 * k, 0.0, -10.0 * k))[0])
        kw = dict(alpha=0.15, depth_tolerance=0.08)
        acc = T.TemporalAccumulator(r, p, iterations=3, **kw)
        other = T.TemporalAccumulator(r, p)  # a second accumulator on the same renderer, without motion: no interaction
        hist, lengths = None, []
        with pytest.raises(T.TrtError, match="triangles"):  # refused before anything is rendered
            acc.frame(cam, moved_from=v[0][:-1])
        assert acc.frame_index == 0
        for i in range(4):
            if i:
                r.update_geometry(v[i])
            before, _ = r.render(p)
            # frame 0: a first frame; 1: moved_from as numpy; 2: as a tensor on the device; 3: None, today's path
            mf = [None, v[0], torch.from_numpy(v[1]).to(torch.device("cuda", 0)), None][i]
            out = acc.frame(cam, moved_from=mf)
            other.frame(cam)
            after, _ = r.render(p)
            assert after.tobytes() == before.tobytes()  # renders before and after are untouched
            d = r.render_camera_denoised(T.make_params(W2, H2, spp, seed + i, flags=R.FIXED), cam)
            for k in KEYS:
                assert out[k].tobytes() == d[k].tobytes(), k
            ins = tuple(d[k] for k in KEYS)
            if mf is None:
                rp = T.reproject(*ins, cam, cam, history=hist, flags=R.FIXED, **kw)
            else:
                org, dirs = T.center_rays(cam, W2, H2, R.FIXED)
                P = r.trace_points(org, dirs, v[i - 1]).reshape(H2, W2, 3)
                rp = T.reproject_motion(*ins, P, cam, cam, history=hist, flags=R.FIXED, **kw)
            assert out["accumulated"].tobytes() == rp["color"].tobytes() and out["accumulated_variance"].tobytes() == rp["variance"].tobytes()
            assert out["history_length"].tobytes() == rp["length"].tobytes()
            den = T.denoise(rp["color"], rp["variance"], d["albedo"], d["normal"], d["depth"], iterations=3)
            assert out["denoised"].tobytes() == den.tobytes()
            assert out["stats"].launches[T.TRT_K_DENOISE] == 1 + 4 and out["stats"].rays == d["stats"].rays
            assert out["stats"].launches[1] == d["stats"].launches[1] + (0 if mf is None else 1)  # trace_points' one traversal
            hist = {"cv": rp["cv"], "length": rp["length"], "normal": d["normal"], "depth": d["depth"]}
            lengths.append(float(out["history_length"].max()))
        assert lengths == [1.0, 2.0, 3.0, 4.0] and acc.frame_index == 4 and other.frame_index == 4
        # a first frame has no history to look up: moved_from is checked and nothing is traced for it
        first = T.TemporalAccumulator(r, p).frame(cam, moved_from=v[2])
        d0 = r.render_camera_denoised(T.make_params(W2, H2, spp, seed, flags=R.FIXED), cam)
        assert first["accumulated"].tobytes() == d0["color"].tobytes() and (first["history_length"] == 1).all()
        assert first["stats"].launches[1] == d0["stats"].launches[1]
    finally:
        r.close()
        s.close()


# ---- an animated sequence ---------------------------------------------------------------------------------------------------------------

def _tonemapped(img):
    return np.clip(img.astype(np.float64), 0.0, 1.0) ** (1 / 2.2)


def test_an_animated_object_keeps_its_history():
    """back at 160 x 120, 4 spp, 6 frames under its own, still camera; the inner object moves 9.5 units along x per frame, 1.5 of its
    pixel footprints (6.2 to 6.6 units at its depth).  Interior pixels of the object: its pixels in the last frame (the centre ray hits one
    of its triangles) whose eight neighbours are its pixels too.  With moved_from more than half of them must have reached history length
    6, without it fewer.  (A length is a weighted mean of the taps' lengths divided by the sum of the weights, each a rounded fp32
    operation, so on taps that all hold 5 it may come out a few ulp of 6, 4.8e-7 each, off 6: the test counts lengths above 6 - 1e-3, a
    rounding tolerance.  One tap of length 4 at a hundredth of the weight already falls below it.)
    Printed: the tonemapped MSE against a 1024-spp render of the last state on the object's pixels and on the whole image, for the
    accumulated-and-denoised image with motion, without it (stale history), and for the last frame alone denoised.
    Measured: 1122 object pixels, 986 interior; at history length 6: 940 with moved_from, 583 without (those that lay on the object in
    all six frames, reading what used to be at the pixel; 961 and 583 lie above 5.5).  Tonemapped MSE with motion / stale / last frame alone: on the object 9.41e-4 /
    1.12e-3 / 1.94e-3, on the image 1.08e-3 / 1.11e-3 / 1.43e-3.  With motion the object is 2.06x and the image 1.33x closer to the converged
    render than one denoised frame, so `not worse than the last frame alone' is asserted on both; the stale history is only 1.19x worse
    than the tracked one on the object (an untextured face under smooth light: history from 1.5 pixels away is nearly right), and no
    ratio between those two is asserted."""
    W2, H2, spp, frames, step = 160, 120, 4, 6, 9.5
    s = T.Scene.named("back", W2, H2)
    r = T.Renderer(s, 0)
    try:
        cam = T.Camera.from_buffer_copy(s.flat.contents.camera)
        p = T.make_params(W2, H2, spp, T.SEED_BACK, flags=R.FIXED)
        vs = [s.arrays()["tri_v"]] + [M.moved_object(s, (step * k, 0.0, 0.0))[0] for k in range(1, frames)]
        sel = M.moved_object(s, (step, 0.0, 0.0))[1]
        with_motion, without = T.TemporalAccumulator(r, p), T.TemporalAccumulator(r, p)
        for k in range(frames):
            if k:
                r.update_geometry(vs[k])
            a = with_motion.frame(cam, moved_from=vs[k - 1] if k else None)
            b = without.frame(cam)
        single = r.render_camera_denoised(T.make_params(W2, H2, spp, T.SEED_BACK + frames - 1, flags=R.FIXED), cam)
        assert single["color"].tobytes() == a["color"].tobytes() == b["color"].tobytes()
        ref = r.render_camera(T.make_params(W2, H2, 1024, T.SEED_BACK + 0x1000, flags=R.FIXED), cam, samples_per_call=64)
        org, dirs = T.center_rays(cam, W2, H2, R.FIXED)
        tri = r.trace_closest(org, dirs)[1].reshape(H2, W2)
    finally:
        r.close()
        s.close()
    obj = (tri >= 0) & sel[np.maximum(tri, 0)]
    interior = obj.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior &= np.roll(np.roll(obj, dy, axis=0), dx, axis=1)
    full = frames - 1e-3
    n_motion, n_stale = int((a["history_length"][interior] > full).sum()), int((b["history_length"][interior] > full).sum())
    print(f"lengths above 5.5: {int((a['history_length'][interior] > 5.5).sum())} with moved_from, {int((b['history_length'][interior] > 5.5).sum())} without")
    print(f"object {int(obj.sum())} pixels, interior {int(interior.sum())}; at history length {frames}: {n_motion} with moved_from, {n_stale} without")
    mses = {}
    for what, m in (("object", obj), ("image", np.ones_like(obj))):
        mse = mses[what] = [np.mean((_tonemapped(x["denoised"])[m] - _tonemapped(ref)[m]) ** 2) for x in (a, b, single)]
        print(f"tonemapped MSE on the {what}: with motion {mse[0]:.4e}, stale history {mse[1]:.4e}, the last frame alone {mse[2]:.4e}")
    assert interior.sum() > 300 and np.isfinite(a["denoised"]).all()
    assert n_motion > 0.5 * interior.sum() and n_stale < n_motion
    assert mses["object"][0] <= mses["object"][2] and mses["image"][0] <= mses["image"][2]
