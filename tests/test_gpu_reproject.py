"""trt_reproject on the MI355X: the kernel gives the bits of the CPU build of its per-pixel code (tests/reproject) on two real frames of
back, veach-mis and staircase from an orbiting camera and on random frames of sizes that are no multiple of the 16 x 16 block, on both
pixel grids, with and without history; the device entry gives the host entry's bits on a side stream, writes nothing past its outputs and
leaves its inputs alone; TemporalAccumulator is render_camera_denoised's buffers -> reproject -> denoise, bit for bit, and changes no
render; after 8 frames of an orbit its image is closer to the converged one than the single denoised frame; a still camera accumulates
the mean of its frames wherever a pixel's feature buffers hold still, on one wall and on a shipped view."""
import numpy as np
import pytest

import reproject_ref as R
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu

SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}
KEYS = ("color", "variance", "albedo", "normal", "depth")
OTHER = dict(alpha=0.05, depth_tolerance=0.03, normal_threshold=0.97, max_history=5.0)
_frames = {}


def _same_bits(cur, cam, pcam, hist, **kw):
    got = T.reproject(*cur, cam, pcam, history=hist, **kw)
    want = R.cpu(*cur, cam, pcam, hist, **kw)
    for k in R.OUT_KEYS:
        g, w = got[k], want[k]
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), f"{k}: {np.count_nonzero(~same)} values differ, first at {np.argwhere(~same)[0]} ({kw})"
    return got


def _two_frames(renderer_factory, name, flags, w=53, h=37, spp=8):
    """Two frames of a scene, the camera orbited by 2 degrees and the seed changed between them: ((camera, buffers), (camera, buffers))."""
    k = (name, flags)
    if k not in _frames:
        r = renderer_factory(get_scene(name, w, h))
        out = []
        for i, deg in enumerate((0.0, 2.0)):
            cam = R.orbit_camera(name, deg, w, h)
            d = r.render_camera_denoised(T.make_params(w, h, spp, SEEDS[name] + i, flags=flags), cam)
            out.append((cam, tuple(d[key] for key in KEYS)))
        _frames[k] = out
    return _frames[k]


@pytest.mark.parametrize("flags", [0, R.FIXED])
@pytest.mark.parametrize("name", ["back", "veach-mis", "staircase"])
def test_gpu_matches_the_cpu_build_bit_for_bit_on_rendered_frames(renderer_factory, name, flags):
    (pcam, prev), (cam, cur) = _two_frames(renderer_factory, name, flags)
    first = _same_bits(prev, pcam, None, None, flags=flags)
    assert (first["length"] == 1).all() and first["color"].tobytes() == prev[0].tobytes()
    hist = {"cv": first["cv"], "length": first["length"], "normal": prev[3], "depth": prev[4]}
    second = _same_bits(cur, cam, pcam, hist, flags=flags)
    hit = cur[4] < R.INF
    share = (second["length"][hit] == 2).mean()
    print(f"{name} flags {flags}: {share:.2f} of {int(hit.sum())} hit pixels found their history")
    assert share > 0.5 and (second["length"][~hit] == 1).all()
    _same_bits(cur, cam, pcam, hist, flags=flags, **OTHER)
    # a third frame on the second's history, back at the first camera; and a still camera
    hist2 = {"cv": second["cv"], "length": second["length"], "normal": cur[3], "depth": cur[4]}
    third = _same_bits(prev, pcam, cam, hist2, flags=flags)
    assert third["length"].max() == 3
    still = _same_bits(cur, cam, cam, hist2, flags=flags)
    assert (still["length"][hit] == second["length"][hit] + 1).mean() > 0.95  # its own feature buffers pass their own tests


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (29, 1), (16, 16), (17, 33), (64, 80)])
def test_gpu_matches_the_cpu_build_bit_for_bit_on_any_size(h, w):
    cur, hist = R.random_frames(h, w, 2000 + 3 * h + w, miss_frac=0.15 if h * w > 1 else 0.0)
    cam, pcam = R.nearby_cameras(w, h, 2000 + h)
    for flags in (0, R.FIXED):
        _same_bits(cur, cam, pcam, None, flags=flags)
        got = _same_bits(cur, cam, pcam, hist, flags=flags)
        if flags and h * w >= 256:
            assert 0.2 < (got["length"] > 1).mean() < 0.98
        _same_bits(cur, cam, pcam, hist, flags=flags, **OTHER)
        _same_bits(cur, cam, cam, hist, flags=flags)
        _same_bits(cur, cam, pcam, hist, flags=flags, alpha=0.0, depth_tolerance=0.0, normal_threshold=0.0, max_history=0.0)  # zeros = the defaults


def test_device_entry_matches_the_host_entry_on_a_side_stream(renderer_factory):
    import torch
    (pcam, prev), (cam, cur) = _two_frames(renderer_factory, "staircase", 0)
    h, w = cur[0].shape[:2]
    first = T.reproject(*prev, pcam)
    hist = {"cv": first["cv"], "length": first["length"], "normal": prev[3], "depth": prev[4]}
    want, st = T.reproject(*cur, cam, pcam, history=hist, alpha=0.1, want_stats=True)
    assert st.launches[T.TRT_K_DENOISE] == 1 and sum(st.launches) == 1 and st.rays == 0
    assert st.kernel_ms[T.TRT_K_DENOISE] > 0 and st.render_ms >= st.kernel_ms[T.TRT_K_DENOISE]
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in cur]
    hdev = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in hist.items()}
    sentinel = -12345.0
    sizes = {"color": h * w * 3, "variance": h * w, "cv": h * w * 4, "length": h * w}
    big = {k: torch.full((n + 4096,), sentinel, dtype=torch.float32, device=dev) for k, n in sizes.items()}
    outs = [big[k][: sizes[k]].view(want[k].shape) for k in R.OUT_KEYS]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    for history, expect in ((hdev, want), (None, T.reproject(*cur, cam, pcam, alpha=0.1))):
        with torch.cuda.stream(side):
            st = T.reproject_into(*ins, cam, pcam, *outs, history=history, alpha=0.1, stream_ptr=side.cuda_stream)
        assert st.launches[T.TRT_K_DENOISE] == 1 and sum(st.launches) == 1
        for k in R.OUT_KEYS:
            got = big[k].cpu().numpy()
            assert got[: sizes[k]].tobytes() == expect[k].reshape(-1).tobytes(), k
            assert (got[sizes[k]:] == sentinel).all(), k
    for t, a in list(zip(ins, cur)) + [(hdev[k], hist[k]) for k in hist]:  # inputs untouched
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_accumulator_is_render_reproject_denoise_and_has_no_side_effects(renderer_factory):
    W, H, spp, seed = 64, 48, 4, 4242
    r = renderer_factory(get_scene("back", W, H))
    p = T.make_params(W, H, spp, seed)
    before, _ = r.render(p)
    aov_before = r.render_aov(p)
    cams = [R.orbit_camera("back", d, W, H) for d in (0.0, 1.5, 3.0)]
    kw = dict(alpha=0.15, depth_tolerance=0.08)
    acc = T.TemporalAccumulator(r, p, iterations=3, **kw)
    other = T.TemporalAccumulator(r, p)  # a second accumulator on the same renderer, interleaved: no interaction
    hist, pcam, lengths = None, None, []
    for i, cam in enumerate(cams):
        if i == 2:
            acc.reset()
            hist, pcam = None, None
        out = acc.frame(cam)
        other.frame(cams[0])
        d = r.render_camera_denoised(T.make_params(W, H, spp, seed + i), cam)
        for k in KEYS:
            assert out[k].tobytes() == d[k].tobytes(), k
        rp = T.reproject(*(d[k] for k in KEYS), cam, pcam, history=hist, **kw)
        assert out["accumulated"].tobytes() == rp["color"].tobytes() and out["accumulated_variance"].tobytes() == rp["variance"].tobytes()
        assert out["history_length"].tobytes() == rp["length"].tobytes()
        den = T.denoise(rp["color"], rp["variance"], d["albedo"], d["normal"], d["depth"], iterations=3)
        assert out["denoised"].tobytes() == den.tobytes()
        assert out["stats"].launches[T.TRT_K_DENOISE] == 1 + 4 and out["stats"].rays == d["stats"].rays
        hist, pcam = {"cv": rp["cv"], "length": rp["length"], "normal": d["normal"], "depth": d["depth"]}, cam
        lengths.append(float(out["history_length"].max()))
    assert lengths == [1.0, 2.0, 1.0] and acc.frame_index == 3  # reset(): the third frame is a first frame, with a seed of its own
    after, _ = r.render(p)
    assert after.tobytes() == before.tobytes()
    aov_after = r.render_aov(p)
    for k in ("albedo", "normal", "depth"):
        assert aov_after[k].tobytes() == aov_before[k].tobytes()


def _tonemapped(img):
    return np.clip(img.astype(np.float64), 0.0, 1.0) ** (1 / 2.2)


@pytest.mark.parametrize("name", ["staircase", "back"])
def test_accumulated_frames_are_closer_to_the_converged_image(renderer_factory, name):
    """160 x 120, 4 spp, 8 frames of an orbit of 1 degree per frame, against a 1024-spp render of the last camera; the baseline is the last
    frame alone, render_camera_denoised at 4 spp.  staircase must be strictly better, back (52 % hit pixels, a silhouette against the void,
    where partially missed pixels lose their history) not worse.  Measured tonemapped MSE, baseline / accumulated: staircase 7.87e-3 / 4.01e-3
    = 1.97x, back 1.47e-3 / 9.71e-4 = 1.51x (the accumulated image before the filter: 6.56e-3 and 1.65e-3).  Both ratios are below 2,
    so there is no second assertion at half the measured ratio."""
    W, H, spp, frames = 160, 120, 4, 8
    r = renderer_factory(get_scene(name, W, H))
    p = T.make_params(W, H, spp, SEEDS[name])
    acc = T.TemporalAccumulator(r, p)
    for k in range(frames):
        cam = R.orbit_camera(name, float(k), W, H)
        out = acc.frame(cam)
    base = r.render_camera_denoised(T.make_params(W, H, spp, SEEDS[name] + frames - 1), cam)
    assert base["color"].tobytes() == out["color"].tobytes()
    ref = r.render_camera(T.make_params(W, H, 1024, SEEDS[name] + 0x1000), cam, samples_per_call=64)
    assert np.isfinite(out["denoised"]).all()
    mse_base = np.mean((_tonemapped(base["denoised"]) - _tonemapped(ref)) ** 2)
    mse_acc = np.mean((_tonemapped(out["denoised"]) - _tonemapped(ref)) ** 2)
    mse_raw = np.mean((_tonemapped(out["accumulated"]) - _tonemapped(ref)) ** 2)
    hit = out["depth"] < R.INF
    print(f"{name}: tonemapped MSE, one denoised frame {mse_base:.4e}, accumulated {mse_raw:.4e}, accumulated and denoised {mse_acc:.4e}: "
          f"ratio {mse_base / mse_acc:.3f}; mean history length on hit pixels {out['history_length'][hit].mean():.2f}")
    if name == "staircase":
        assert mse_acc < mse_base
    else:
        assert mse_acc <= mse_base


class _SceneView:
    """The flat description of a scene (the arrays stay the scene's) with another camera as its own, for Renderer()."""

    def __init__(self, s, cam):
        import ctypes as C
        self._scene = s
        self._flat = T.SceneFlat.from_buffer_copy(s.flat.contents)
        self._flat.camera = cam
        self.flat = C.pointer(self._flat)


def _still_frames(r, cam, W, H, K):
    """K frames of a TemporalAccumulator under one camera, alpha = 1e-3 -> the frames' dicts."""
    acc = T.TemporalAccumulator(r, T.make_params(W, H, 4, 77), alpha=1e-3)
    return [acc.frame(cam) for _ in range(K)]


def _report(frames, sel, what):
    K, out = len(frames), frames[-1]
    mean = np.mean([f["color"].astype(np.float64) for f in frames], axis=0)
    err = np.abs(out["accumulated"] - mean) / np.maximum(np.abs(mean), 1e-6)
    print(f"{what}: {int(sel.sum())} pixels, history length {K} at {int((out['history_length'][sel] == K).sum())}, "
          f"accumulated off the mean by more than 1e-5 at {int((err[sel] > 1e-5).any(axis=1).sum())}")
    return mean


def test_still_camera_accumulates_the_mean_of_its_frames():
    """6 frames from the handle's own camera, alpha = 1e-3: the accumulated colour is the mean of the frames' colours to 1e-5 wherever the
    albedo is positive.
    The view.  The contract promises this where a pixel's feature buffers are the same in every frame: the buffers are means over the
    pixel's jittered samples of a seed that changes with the frame, so on a silhouette, a crease, a seam between materials or a texture the
    depth, normal or albedo of one pixel differs between frames under a still camera too, and the contract itself then has the pixel start
    over (the depth and normal tests) or remodulates it by another albedo than it was accumulated with (the next test pins that on back's
    own view; DESIGN.md 7.3 "Limits").  So the handle's camera here looks at the inside of one wall of back (one plane, one material, no
    texture; depths 89 .. 105, so the jitter moves a pixel's mean depth by far less than the tolerance): every pixel is inside a surface,
    and everything the still path can get wrong still shows — resampling (fx != x), a neighbour leaking in, the 1 / N schedule, the
    history swap, a stale or shared history.  The light of 4 spp differs from pixel to pixel and frame to frame by far more than 1e-5."""
    W, H, K = 64, 48, 6
    cam = T.look_at((278.0, 420.0, 470.0), (278.0, 420.0, 560.0), (0.0, 1.0, 0.0), 40.0, W, H)
    r = T.Renderer(_SceneView(get_scene("back", W, H), cam), 0)  # a handle whose own camera is `cam`
    try:
        frames = _still_frames(r, cam, W, H, K)
    finally:
        r.close()
    out = frames[-1]
    ok = np.all([(f["albedo"] > 0).all(axis=2) for f in frames], axis=0)
    mean = _report(frames, ok, "still camera, one wall")
    assert ok.all() and (out["history_length"] == K).all()
    assert np.abs(frames[0]["color"] - frames[1]["color"]).max() > 1e-2 and np.abs(np.diff(mean, axis=1)).max() > 1e-3  # frames and pixels differ
    np.testing.assert_allclose(out["accumulated"][ok], mean[ok], rtol=1e-5, atol=1e-7)


def test_still_camera_on_a_shipped_view_keeps_the_pixels_whose_features_hold_still(renderer_factory):
    """The same six frames on back's own view, which has silhouettes, creases and seams between materials.  A pixel is STABLE when its
    albedo has the same bits in every frame and every frame's depth and normal pass the contract's own tap test against the frame
    before (the test of trt_rp_tap_ok, restated here in fp32 in its operation order, at the defaults 0.1 and 0.9).  By the contract
    exactly those pixels keep their history through all frames and are demodulated by one albedo throughout: their history length is 6 and
    their accumulated colour is the mean of the frames to 1e-5.  Every other pixel may start over.  At 64 x 48 most pixels lie inside a
    surface: more than half of the pixels with a positive albedo must be stable (the bound the issue sets for real feature buffers after a
    small move, applied to no move at all).  Measured: 1412 pixels with albedo > 0 in every frame, 1185 of them stable, 1197 at history
    length 6, 227 off the mean of their frames by more than 1e-5."""
    W, H, K = 64, 48, 6
    s = get_scene("back", W, H)
    frames = _still_frames(renderer_factory(s), T.Camera.from_buffer_copy(s.flat.contents.camera), W, H, K)
    out = frames[-1]
    f32 = np.float32
    ok = np.all([(f["albedo"] > 0).all(axis=2) for f in frames], axis=0)
    stable = ok.copy()
    for prev, cur in zip(frames[:-1], frames[1:]):
        stable &= (cur["albedo"].view(np.uint32) == prev["albedo"].view(np.uint32)).all(axis=2)
        zp, zq, n_p, n_q = cur["depth"], prev["depth"], cur["normal"], prev["normal"]
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]  # noqa: E731
        dn = dot(n_p, n_q)
        stable &= (zq < f32(R.INF)) & (zp < f32(R.INF)) & (np.abs(zp - zq) <= f32(0.1) * zp)
        stable &= (dn > 0) & (dn * dn >= ((f32(0.9) * f32(0.9)) * dot(n_p, n_p)) * dot(n_q, n_q))
    mean = _report(frames, ok, "still camera, back's own view, albedo > 0")
    _report(frames, stable, "still camera, back's own view, stable")
    assert stable.sum() > 0.5 * ok.sum()
    assert (out["history_length"][stable] == K).all()
    np.testing.assert_allclose(out["accumulated"][stable], mean[stable], rtol=1e-5, atol=1e-7)
    assert (out["history_length"][ok] == K).sum() >= stable.sum()
