"""trt_reproject_moments on the MI355X: both kernels give the bits of the CPU build of their per-pixel code (tests/moments) in every
output, at sizes whose partial blocks and aprons cross every image border, on a first frame, a still camera's fifth frame, a moved camera
on both grids and the prev_point path, with misses and NaN depths on block corners, with stage B's LDS tile and without it, through the
host and the device entry; a block without a pixel for stage B returns early and its neighbours do not; the device entry refuses
misaligned records, counts two launches and allocates nothing; TemporalAccumulator(variance="moments") accumulates the default
accumulator's colours, runs at one sample per pixel, and its filter helps."""
import ctypes as C

import numpy as np
import pytest

import moments_ref as MV
import motion_ref as M
import reproject_ref as R
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd import _abi

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (37, 23), (53, 37)]  # (w, h)
OTHER = dict(alpha=0.05, depth_tolerance=0.12, normal_threshold=0.8, max_history=6.0, min_frames=2, sigma_normal=32, sigma_depth=3.0)


def _assert_bits(got, want, what):
    for k in MV.OUT_KEYS:
        g, w = np.ascontiguousarray(got[k]), want[k]
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), f"{what} {k}: {np.count_nonzero(~same)} values differ, first at {np.argwhere(~same)[0]}"


def _same_bits(cur, cam, pcam, hist, what, **kw):
    want = MV.cpu(*cur, cam, pcam, hist, **kw)
    _assert_bits(T.reproject_moments(*cur, cam, pcam, history=hist, **kw), want, what)
    return want


def _device(cur, cam, pcam, hist, prev_point=None, **kw):
    """The device entry on fresh tensors, on a side stream -> (dict of numpy outputs, Stats)."""
    import torch
    dev = torch.device("cuda", 0)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    h, w = cur[0].shape[:2]
    outs = {k: torch.full(v.shape, -12345.0, dtype=torch.float32, device=dev) for k, v in MV.empty_outputs(h, w).items()}
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        st = T.reproject_moments_into(*[to(a) for a in cur], cam, pcam, *[outs[k] for k in MV.OUT_KEYS],
                                      history=None if hist is None else {k: to(v) for k, v in hist.items()}, prev_point=to(prev_point),
                                      stream_ptr=side.cuda_stream, **kw)
    return {k: v.cpu().numpy() for k, v in outs.items()}, st


def _plant(cur, w, h):
    """Misses and NaN depths on the corners of the 16 x 16 blocks that lie in the image."""
    color, albedo, normal, depth = (a.copy() for a in cur)
    k = 0
    for y in (0, 15, 16, 31, h - 1):
        for x in (0, 15, 16, 31, 32, w - 1):
            if 0 <= y < h and 0 <= x < w and w * h > 1:
                depth[y, x] = np.nan if k % 2 else R.INF
                k += 1
    return color, albedo, normal, depth


@pytest.mark.parametrize("w,h", SIZES)
def test_kernels_match_the_cpu_build_bit_for_bit(w, h, monkeypatch):
    seed = 3000 + 3 * h + w
    cur, hist = MV.random_frames(h, w, seed, miss_frac=0.1 if h * w > 1 else 0.0)
    cur = _plant(cur, w, h)
    cam, pcam = R.nearby_cameras(w, h, seed)
    for lds in ("1", "0"):
        monkeypatch.setenv("TRT_MOMENTS_LDS", lds)
        what = f"{w}x{h} lds {lds}"
        first = _same_bits(cur, cam, None, None, what + " first frame")
        assert (first["length"] == 1).all()
        for flags in (0, R.FIXED):
            got = _same_bits(cur, cam, pcam, hist, f"{what} moved camera flags {flags}", flags=flags)
            if flags and w * h >= 256:
                assert 0.2 < (got["length"] > 1).mean() < 0.98
                hit = cur[3] < R.INF
                on_route = MV.restate(*cur, cam, pcam, hist, flags=flags)["temporal"][hit].mean()
                assert 0.1 < on_route < 0.9, on_route  # both routes in one image
            _same_bits(cur, cam, pcam, hist, f"{what} other parameters flags {flags}", flags=flags, **OTHER)
            P = M.smooth_field_points(cam, w, h, cur[3], flags, seed)
            _same_bits(cur, cam, pcam, hist, f"{what} prev_point flags {flags}", prev_point=P, flags=flags)
        # a still camera's frames 1 to 5 on a flat plane (after frame 4 every hit pixel is on the temporal route)
        frames, scam = MV.flat_sequence(h, w, 5, seed)
        hs = None
        for k, f in enumerate(frames):
            f = _plant(f, w, h) if k % 2 == 0 else f
            out = _same_bits(f, scam, scam, hs, f"{what} still frame {k + 1}")
            hs = MV.next_history(out, f[2], f[3])
        assert out["length"].max() == 5 or w * h == 1
    # the device entry: the host entry's bits
    monkeypatch.delenv("TRT_MOMENTS_LDS")
    for kw in (dict(hist=hist, flags=R.FIXED), dict(hist=None), dict(hist=hist, prev_point=M.smooth_field_points(cam, w, h, cur[3], 0, seed))):
        hst = kw.pop("hist")
        want = MV.cpu(*cur, cam, pcam, hst, **kw)
        got, st = _device(cur, cam, pcam, hst, **kw)
        _assert_bits(got, want, f"{w}x{h} device entry {sorted(kw)}")
        assert st.launches[T.TRT_K_DENOISE] == 2 and sum(st.launches) == 2 and st.rays == 0


def test_a_block_that_needs_no_spatial_estimate_returns_early(monkeypatch):
    """32 x 32 under a still camera: a history of length 8 (s = 0.2) everywhere except one 16 x 16 block, whose history is one frame long.
    Three blocks have no pixel for stage B and return after the vote; the fourth stages its tile, whose apron reaches into them."""
    w = h = 32
    frames, cam = MV.flat_sequence(h, w, 2, 77)
    first = MV.cpu(*frames[0], cam)
    hist = MV.next_history(first, frames[0][2], frames[0][3])
    hist["length"] = np.full((h, w), 8.0, np.float32)
    hist["mom"][..., 2] = 0.2
    hist["length"][0:16, 16:32] = 1.0
    hist["mom"][0:16, 16:32, 2] = 1.0
    want = MV.cpu(*frames[1], cam, cam, hist)
    ref = MV.restate(*frames[1], cam, cam, hist)
    assert not ref["temporal"][0:16, 16:32].any() and ref["temporal"][16:, :].all() and ref["temporal"][:, :16].all() and not ref["edge"].any()
    for lds in ("1", "0"):
        monkeypatch.setenv("TRT_MOMENTS_LDS", lds)
        _assert_bits(T.reproject_moments(*frames[1], cam, cam, history=hist), want, f"lds {lds}")
    monkeypatch.delenv("TRT_MOMENTS_LDS")
    got, _ = _device(frames[1], cam, cam, hist)
    _assert_bits(got, want, "device entry")


def test_device_entry_refuses_misaligned_records_counts_two_launches_and_allocates_nothing():
    import torch
    w, h = 40, 24
    cur, hist = MV.random_frames(h, w, 91)
    cam, pcam = R.nearby_cameras(w, h, 91)
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(a).to(dev) for a in cur]
    hdev = {k: torch.from_numpy(v).to(dev) for k, v in hist.items()}
    outs = {k: torch.empty(v.shape, dtype=torch.float32, device=dev) for k, v in MV.empty_outputs(h, w).items()}
    lib = _abi.load_hip()
    p = MV.params(cam, pcam)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    base = [ptr(t) for t in ins] + [None] + [ptr(hdev[k]) for k in MV.HISTORY_KEYS] + [ptr(outs[k]) for k in MV.OUT_KEYS]
    spare = torch.empty(h * w * 4 + 4, dtype=torch.float32, device=dev)
    for i in (5, 9, 12, 14):  # prev_cv, prev_mom, out_cv, out_mom
        bad = list(base)
        bad[i] = ptr(spare, 4)
        assert lib.trt_reproject_moments_device(0, C.byref(p), w, h, *bad, None, None) == 1 and b"aligned" in lib.trt_last_error(), i
    args = (*ins, cam, pcam, *[outs[k] for k in MV.OUT_KEYS])
    T.reproject_moments_into(*args, history=hdev)  # the first call loads the code objects
    torch.cuda.synchronize(dev)
    free_before, _ = torch.cuda.mem_get_info(dev)  # hipMemGetInfo
    st = T.reproject_moments_into(*args, history=hdev)
    free_after, _ = torch.cuda.mem_get_info(dev)
    assert free_after == free_before, (free_before, free_after)
    assert st.launches[T.TRT_K_DENOISE] == 2 and sum(st.launches) == 2 and st.rays == 0
    assert st.kernel_ms[T.TRT_K_DENOISE] > 0 and st.render_ms >= st.kernel_ms[T.TRT_K_DENOISE]
    _assert_bits({k: v.cpu().numpy() for k, v in outs.items()}, MV.cpu(*cur, cam, pcam, hist), "device entry")
    _, hst = T.reproject_moments(*cur, cam, pcam, history=hist, want_stats=True)
    assert hst.launches[T.TRT_K_DENOISE] == 2 and sum(hst.launches) == 2


# ---- TemporalAccumulator(variance="moments") -----------------------------------------------------------------------------------------

W, H = 160, 120


def _tonemapped(img):
    return np.clip(img.astype(np.float64), 0.0, 1.0) ** (1 / 2.2)


def test_moments_accumulator_accumulates_the_default_accumulators_colours(renderer_factory):
    r = renderer_factory(get_scene("back", W, H))
    p = T.make_params(W, H, 2, T.SEED_BACK)
    a, b = T.TemporalAccumulator(r, p), T.TemporalAccumulator(r, p, variance="moments")
    for k in range(4):
        cam = R.orbit_camera("back", float(k), W, H)
        oa, ob = a.frame(cam), b.frame(cam)
        assert ob["variance"] is None and set(oa) == set(ob)
        for key in ("color", "albedo", "normal", "depth", "accumulated", "history_length"):
            assert oa[key].tobytes() == ob[key].tobytes(), (k, key)
        assert np.isfinite(ob["denoised"]).all() and np.isfinite(ob["accumulated_variance"]).all()
        assert ob["stats"].launches[T.TRT_K_DENOISE] == 2 + 6
    assert round(float(oa["history_length"].max())) == 4  # a weighted mean over resampled taps plus one: 4 to rounding


def test_one_sample_per_pixel_frames_denoise(renderer_factory):
    """back at 160 x 120, 1 spp, 8 frames of a 1-degree-per-frame orbit, against a 1024-spp render of the last camera: the filter, driven by
    the estimated variance, must not be worse than the accumulated image it starts from.  Recorded, not asserted: the ratio
    of the two MSEs, the default accumulator at 2 spp over the last 4 of those cameras (the same 8 samples per pixel), and the share of hit
    pixels on the temporal route at frame 8."""
    r = renderer_factory(get_scene("back", W, H))
    acc = T.TemporalAccumulator(r, T.make_params(W, H, 1, T.SEED_BACK), variance="moments")
    for k in range(8):
        cam = R.orbit_camera("back", float(k), W, H)
        out = acc.frame(cam)
        assert all(np.isfinite(v).all() for key, v in out.items() if key not in ("stats", "variance", "depth")), k
    two = T.TemporalAccumulator(r, T.make_params(W, H, 2, T.SEED_BACK + 100))
    for k in range(4, 8):
        out2 = two.frame(R.orbit_camera("back", float(k), W, H))
    ref = _tonemapped(r.render_camera(T.make_params(W, H, 1024, T.SEED_BACK + 0x1000), cam, samples_per_call=64))
    mse = lambda img: float(np.mean((_tonemapped(img) - ref) ** 2))  # noqa: E731
    mse_acc, mse_den, mse_two = mse(out["accumulated"]), mse(out["denoised"]), mse(out2["denoised"])
    hit = out["depth"] < R.INF
    mom = acc._history["mom"].cpu().numpy()
    route = hit & (out["history_length"] >= 4) & (1.0 - mom[..., 2] >= MV.MIN_DOF)
    print(f"back 160x120, 1 spp x 8 frames: tonemapped MSE accumulated {mse_acc:.4e}, denoised {mse_den:.4e}, ratio {mse_acc / mse_den:.3f}; "
          f"default accumulator, 2 spp x 4 frames, denoised {mse_two:.4e}; {route.sum() / hit.sum():.3f} of {int(hit.sum())} hit pixels on the temporal route")
    assert mse_den <= mse_acc


def test_moments_accumulator_follows_moved_geometry_as_the_cpu_build_does():
    import torch
    w, h = 64, 48
    s = T.Scene.named("back", w, h)
    r = T.Renderer(s, 0)
    try:
        cam = T.Camera.from_buffer_copy(s.flat.contents.camera)
        v0 = s.arrays()["tri_v"]
        v1 = M.moved_object(s, (20.0, 0.0, -10.0))[0]
        acc = T.TemporalAccumulator(r, T.make_params(w, h, 1, 4242, flags=R.FIXED), variance="moments", alpha=0.15)
        acc.frame(cam)
        hist = {k: v.cpu().numpy() for k, v in acc._history.items()}
        dev = torch.device("cuda", 0)
        r.update_geometry_from(torch.from_numpy(v1).to(dev))
        out = acc.frame(cam, moved_from=torch.from_numpy(v0).to(dev))
        org, dirs = T.center_rays(cam, w, h, R.FIXED)
        P = r.trace_points(org, dirs, v0).reshape(h, w, 3)
        want = MV.cpu(out["color"], out["albedo"], out["normal"], out["depth"], cam, cam, hist, prev_point=P, flags=R.FIXED, alpha=0.15)
        got = {"color": out["accumulated"], "variance": out["accumulated_variance"], "length": out["history_length"],
               "cv": acc._history["cv"].cpu().numpy(), "mom": acc._history["mom"].cpu().numpy()}
        _assert_bits(got, want, "moved_from")
        assert (out["history_length"] == 2).mean() > 0.3 and np.isfinite(out["denoised"]).all()
        assert out["stats"].launches[T.TRT_K_DENOISE] == 2 + 6
    finally:
        r.close()
        s.close()
