"""trt_despeckle on the MI355X: the kernel gives the bits of the CPU build of its per-pixel code (tests/despeckle) in all three outputs, at
the smallest sizes where it can go wrong (one pixel, less than a window, one block whose whole apron lies outside the image, partial blocks
whose aprons cross block and image borders) and on a rendered frame, at R = 1 and 2, through the host and the device entry, with and without
the optional buffers, with the LDS tile and (in a child process under TRT_DESPECKLE_LDS=0) without it; it counts one launch; and
TemporalAccumulator(despeckle=...) is the chain despeckle -> reproject_moments -> denoise called by hand."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as DN
import despeckle_ref as D
import reproject_ref as R
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd import _abi

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (3, 3), (16, 16), (17, 16), (33, 19)]  # (w, h)


def _plant(depth):
    """Misses and NaN depths on the corners of the 16 x 16 blocks that lie in the image."""
    h, w = depth.shape
    depth = depth.copy()
    k = 0
    for y in (0, 15, 16, h - 1):
        for x in (0, 15, 16, 31, 32, w - 1):
            if 0 <= y < h and 0 <= x < w and w * h > 9:
                depth[y, x] = np.nan if k % 2 else DN.INF
                k += 1
    return depth


def _planted_cases():
    """The cases of tests/test_despeckle_cpu.py: a spike in a field, two adjacent spikes, a NaN and an infinite centre, NaN neighbours and
    misses, a hit among misses with two and with three hit neighbours, a flat image of an arbitrary value."""
    out = {}
    color, albedo, depth, variance = D.field(9, 9)
    color[4, 4] = 1e4
    out["spike"] = (color, variance, albedo, depth)
    color = color.copy()
    color[4, 5] = 1e4
    out["two spikes"] = (color, variance, albedo, depth)
    color, albedo, depth, variance = D.field(7, 7, 0.5, 0.25)
    color[3, 3, 0], color[1, 5], variance[3, 3] = np.nan, np.inf, np.nan
    out["nan centre"] = (color, variance, albedo, depth)
    color, albedo, depth, variance = D.field(9, 9, 0.5, 0.5)
    color[4, 4], color[3, 3], color[4, 5, 2], color[5, 4] = 300.0, np.nan, np.inf, 7.0
    depth[5, 4], depth[3, 5] = DN.INF, np.nan
    out["nan neighbours and misses"] = (color, variance, albedo, depth)
    color, albedo, depth, variance = D.field(7, 7)
    depth[:] = DN.INF
    depth[3, 3] = depth[3, 4] = depth[2, 2] = 4.0
    color[3, 3] = 50.0
    out["two taps"] = (color, variance, albedo, depth)
    depth = depth.copy()
    depth[4, 3] = 4.0
    out["three taps"] = (color, variance, albedo, depth)
    color, albedo, depth, variance = D.field(20, 18, 0.37, 0.61)
    out["flat"] = (color, variance, albedo, depth)
    return out


def _random_cases():
    out = {}
    for w, h in SIZES:
        (color, variance, albedo, _, depth), _, _ = D.spiked_inputs(h, w, 4000 + 3 * h + w, spikes=max(1, w * h // 40), nans=min(3, w * h // 9))
        out[f"{w}x{h}"] = (color, variance, albedo, _plant(depth))
    return out


def _rendered_case():
    """staircase at 64 x 48 and one sample per pixel with its render_aov buffers, rendered here; the variance is made up (l^2 / 4)."""
    w, h = 64, 48
    r = T.Renderer(get_scene("staircase", w, h), 0)
    try:
        p = T.make_params(w, h, 1, T.SEED_STAIRCASE)
        color, _ = r.render(p)
        aov = r.render_aov(p)
    finally:
        r.close()
    lum = color.astype(np.float64) @ DN.LUMA
    return {"staircase 64x48 1 spp": (color, (0.25 * lum * lum).astype(np.float32), aov["albedo"], aov["depth"])}


def _host(color, variance, albedo, depth, want_scale, radius):
    """trt_despeckle itself, so that out_scale can be left out -> (outputs, Stats)."""
    h, w = depth.shape
    out = {"color": np.full((h, w, 3), -12345.0, np.float32), "variance": None if variance is None else np.full((h, w), -12345.0, np.float32),
           "scale": np.full((h, w), -12345.0, np.float32) if want_scale else None}
    st = T.Stats()
    p = D.params(radius=radius)
    ptr = lambda a: None if a is None else a.ctypes.data_as(D.fp)  # noqa: E731
    rc = _abi.load_hip().trt_despeckle(0, C.byref(p), w, h, ptr(color), ptr(variance), ptr(albedo), ptr(depth), *[ptr(out[k]) for k in D.OUT_KEYS], C.byref(st))
    assert rc == 0, _abi.load_hip().trt_last_error()
    return out, st


def _device(color, variance, albedo, depth, want_scale, radius):
    """The device entry on fresh tensors, on a side stream -> (outputs, Stats)."""
    import torch
    dev = torch.device("cuda", 0)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    h, w = depth.shape
    new = lambda *shape: torch.full(shape, -12345.0, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"color": new(h, w, 3), "variance": None if variance is None else new(h, w), "scale": new(h, w) if want_scale else None}
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        st = T.despeckle_into(to(color), to(albedo), to(depth), out["color"], variance=to(variance), out_variance=out["variance"], out_scale=out["scale"],
                              radius=radius, stream_ptr=side.cuda_stream)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}, st


def _assert_bits(got, want, what):
    for k in D.OUT_KEYS:
        if want[k] is None:
            assert got[k] is None
            continue
        g, w = np.ascontiguousarray(got[k]), want[k]
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), f"{what} {k}: {np.count_nonzero(~same)} values differ, first at {np.argwhere(~same)[0]}"


def run_cases(cases):
    """Every case at R = 1 and 2, through both entries, with and without variance and out_scale, against the CPU build.  -> calls made."""
    calls = 0
    for name, (color, variance, albedo, depth) in cases.items():
        for radius in (1, 2):
            for optional in (True, False):
                var = variance if optional else None
                want = D.cpu(color, albedo, depth, var, want_scale=optional, radius=radius)
                for entry in (_host, _device):
                    got, st = entry(color, var, albedo, depth, optional, radius)
                    _assert_bits(got, want, f"{name} R {radius} {entry.__name__} optional buffers {optional}")
                    assert st.launches[T.TRT_K_DENOISE] == 1 and sum(st.launches) == 1 and st.rays == 0
                    calls += 1
    return calls


GROUPS = {"sizes": _random_cases, "planted": _planted_cases, "rendered": _rendered_case}


def all_cases():
    return {k: v for make in GROUPS.values() for k, v in make().items()}


@pytest.mark.parametrize("group", ["sizes", "planted"])
def test_kernel_matches_the_cpu_build_bit_for_bit_with_the_lds_tile(group, monkeypatch):
    monkeypatch.delenv("TRT_DESPECKLE_LDS", raising=False)
    cases = GROUPS[group]()
    assert run_cases(cases) == 8 * len(cases)
    if group == "sizes":  # the cases do what they are there for: pixels clamped, replaced and left alone in one image
        w = D.cpu(*[cases["33x19"][i] for i in (0, 2, 3, 1)])
        assert ((w["scale"] < 1) & (w["scale"] > 0)).any() and (w["scale"] == 0).any() and (w["scale"] == 1).any()


def test_kernel_matches_the_cpu_build_on_a_rendered_frame(monkeypatch):
    monkeypatch.delenv("TRT_DESPECKLE_LDS", raising=False)
    cases = _rendered_case()
    assert run_cases(cases) == 8
    frame = cases["staircase 64x48 1 spp"]
    s = D.cpu(frame[0], frame[2], frame[3])["scale"]
    assert 20 < (s != 1).sum() < 0.2 * s.size, int((s != 1).sum())  # a 1-spp frame has its fireflies
    # the wrapper: the same outputs by name, and Stats on request
    out, st = T.despeckle(frame[0], frame[2], frame[3], variance=frame[1], radius=2, want_stats=True)
    _assert_bits(out, D.cpu(frame[0], frame[2], frame[3], frame[1], radius=2), "T.despeckle")
    assert st.launches[T.TRT_K_DENOISE] == 1 and st.kernel_ms[T.TRT_K_DENOISE] > 0 and st.render_ms >= st.kernel_ms[T.TRT_K_DENOISE]
    assert T.despeckle(frame[0], frame[2], frame[3])["variance"] is None


CHILD = """
import os, sys
sys.path[:0] = [{tests!r}, {root!r}]
assert os.environ["TRT_DESPECKLE_LDS"] == "0"
import test_gpu_despeckle as G
cases = G.all_cases()
print("ok", G.run_cases(cases), len(cases))
"""


def test_kernel_matches_the_cpu_build_bit_for_bit_without_the_lds_tile():
    """The same cases in a child process whose environment sends the taps to global memory (the library reads TRT_DESPECKLE_LDS per call)."""
    code = CHILD.format(tests=TESTS, root=os.path.dirname(TESTS))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TRT_DESPECKLE_LDS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n_calls, n_cases = (int(x) for x in r.stdout.split()[-2:])
    assert r.stdout.split()[-3] == "ok" and n_calls == 8 * n_cases and n_cases == len(SIZES) + 7 + 1


def test_device_entry_allocates_nothing():
    import torch
    w, h = 40, 24
    (color, variance, albedo, _, depth), _, _ = D.spiked_inputs(h, w, 91)
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(a).to(dev) for a in (color, albedo, depth)]
    var = torch.from_numpy(variance).to(dev)
    outs = [torch.empty_like(ins[0]), torch.empty_like(var), torch.empty_like(var)]
    T.despeckle_into(*ins, outs[0], variance=var, out_variance=outs[1], out_scale=outs[2])  # the first call loads the code objects
    torch.cuda.synchronize(dev)
    free_before, _ = torch.cuda.mem_get_info(dev)
    st = T.despeckle_into(*ins, outs[0], variance=var, out_variance=outs[1], out_scale=outs[2])
    free_after, _ = torch.cuda.mem_get_info(dev)
    assert free_after == free_before, (free_before, free_after)
    assert st.launches[T.TRT_K_DENOISE] == 1 and sum(st.launches) == 1
    _assert_bits(dict(zip(D.OUT_KEYS, (o.cpu().numpy() for o in outs))), D.cpu(color, albedo, depth, variance), "device entry")
    with pytest.raises(T.TrtError, match="out_variance"):
        T.despeckle_into(*ins, outs[0], variance=var, out_variance=outs[1][:3])
    with pytest.raises(T.TrtError, match="both or neither"):
        T.despeckle_into(*ins, outs[0], variance=var)


# ---- TemporalAccumulator(despeckle=...) ------------------------------------------------------------------------------------------------

W, H = 32, 24


def test_accumulator_with_the_clamp_is_the_chain_called_by_hand(renderer_factory):
    r = renderer_factory(get_scene("back", W, H))
    p = T.make_params(W, H, 1, T.SEED_BACK)
    for arg, kw in ((True, {}), ({"radius": 2, "sigma": 2.0}, {"radius": 2, "sigma": 2.0})):
        acc = T.TemporalAccumulator(r, p, variance="moments", despeckle=arg)
        hist, prev = None, None
        for k in range(3):
            cam = R.orbit_camera("back", float(k), W, H)
            out = acc.frame(cam)
            assert out["stats"].launches[T.TRT_K_DENOISE] == 2 + 6 + 1 and out["variance"] is None
            ds = T.despeckle(out["color"], out["albedo"], out["depth"], **kw)
            assert out["despeckle_scale"].tobytes() == ds["scale"].tobytes() == D.cpu(out["color"], out["albedo"], out["depth"], **kw)["scale"].tobytes()
            rp = T.reproject_moments(ds["color"], out["albedo"], out["normal"], out["depth"], cam, prev, history=hist)
            den = T.denoise(rp["color"], rp["variance"], out["albedo"], out["normal"], out["depth"])
            for key, want in (("accumulated", rp["color"]), ("accumulated_variance", rp["variance"]), ("history_length", rp["length"]), ("denoised", den)):
                assert out[key].tobytes() == want.tobytes(), (k, key)
            hist = {"cv": rp["cv"], "length": rp["length"], "normal": out["normal"], "depth": out["depth"], "mom": rp["mom"]}
            prev = cam
        assert (out["history_length"] > 1).any()


def test_accumulator_without_the_clamp_is_unchanged(renderer_factory):
    r = renderer_factory(get_scene("back", W, H))
    p = T.make_params(W, H, 1, T.SEED_BACK)
    a, b = T.TemporalAccumulator(r, p, variance="moments"), T.TemporalAccumulator(r, p, variance="moments", despeckle=None)
    for k in range(3):
        cam = R.orbit_camera("back", float(k), W, H)
        oa, ob = a.frame(cam), b.frame(cam)
        assert set(oa) == set(ob) and "despeckle_scale" not in oa
        for key in oa:
            if key not in ("stats", "variance"):
                assert oa[key].tobytes() == ob[key].tobytes(), (k, key)
        assert list(oa["stats"].launches) == list(ob["stats"].launches) and oa["stats"].launches[T.TRT_K_DENOISE] == 2 + 6
    # with variance="samples" the frame's variance is clamped with its colour
    two = T.TemporalAccumulator(r, T.make_params(W, H, 2, T.SEED_BACK), despeckle=True)
    out = two.frame(cam)
    ds = T.despeckle(out["color"], out["albedo"], out["depth"], variance=out["variance"])
    rp = T.reproject(ds["color"], ds["variance"], out["albedo"], out["normal"], out["depth"], cam)
    assert out["accumulated"].tobytes() == rp["color"].tobytes() and out["accumulated_variance"].tobytes() == rp["variance"].tobytes()
    assert out["stats"].launches[T.TRT_K_DENOISE] == 1 + 6 + 1 and out["despeckle_scale"].tobytes() == ds["scale"].tobytes()
