"""The adaptive-sampling policy (tinyraytracing_amd/adaptive.py, Renderer.render_adaptive) against a fake renderer whose per-pixel
moments are known in closed form, and the ABI of trt_render_pixels (no GPU needed)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import tinyraytracing_amd as T
from tinyraytracing_amd import _abi, adaptive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakePixels:
    """Pixel q's sample s has the grey value v = base[q] * (1 + amp[q] * (-1)^s).  Over an even count n the mean is base and the
    unbiased variance base^2 amp^2 n / (n - 1), so with luminance weights summing to 1 the relative error is amp / sqrt(n - 1).
    Records every call as (pixels, s0, s1)."""

    def __init__(self, base, amp):
        self.base, self.amp, self.calls = np.asarray(base, float), np.asarray(amp, float), []
        self.done = np.zeros(len(base), np.int64)  # samples each pixel has received so far

    def __call__(self, pixels, s0, s1, sums, sumsq):
        pixels = np.asarray(pixels)
        self.calls.append((pixels.copy(), s0, s1))
        assert (self.done[pixels] == s0).all(), "a pixel's samples must stay the prefix [0, n_q) of its stream"
        sums, sumsq = sums.copy(), sumsq.copy()
        for s in range(s0, s1):
            v = self.base[pixels] * (1.0 + self.amp[pixels] * (-1.0) ** s)
            sums += v[:, None]
            sumsq += (v * v)[:, None]
        self.done[pixels] = s1
        return sums, sumsq


def expected_count(amp, rel, min_spp, max_spp, batch):
    n = min_spp
    while n < max_spp and amp / math.sqrt(n - 1) > rel:
        n = min(n + batch, max_spp)
    return n


def run_policy(fake, k, rel, min_spp, max_spp, batch):
    return adaptive.run(fake, np.arange(k), np.zeros((k, 3)), np.zeros((k, 3)), np.zeros(k, np.int64), rel, min_spp, max_spp, batch)


def test_thresholds_give_the_closed_form_counts():
    amps = np.array([0.0, 0.05, 0.3, 0.5, 0.8, 1.0, 1.5, 3.0, 10.0])
    fake = FakePixels(np.full(amps.size, 2.5), amps)
    sums, sumsq, counts, err, rounds = run_policy(fake, amps.size, 0.25, 4, 64, 4)
    want = [expected_count(a, 0.25, 4, 64, 4) for a in amps]
    assert counts.tolist() == want
    assert want[0] == 4 and want[-1] == 64 and len(set(want)) >= 5
    np.testing.assert_allclose(err, amps / np.sqrt(counts - 1.0), rtol=1e-12, atol=1e-15)
    assert ((err <= 0.25) | (counts == 64)).all()
    np.testing.assert_allclose(sums, 2.5 * counts[:, None] * np.ones((1, 3)), rtol=1e-14)
    # one call per round; every round renders the same range for all of its pixels, and only those still above the threshold
    assert rounds == len(fake.calls) == 1 + (64 - 4) // 4
    assert fake.calls[0][1:] == (0, 4) and len(fake.calls[0][0]) == amps.size
    for i, (pix, s0, s1) in enumerate(fake.calls[1:]):
        assert (s0, s1) == (4 + 4 * i, 8 + 4 * i)
        assert sorted(pix.tolist()) == [q for q in range(amps.size) if want[q] > s0]


def test_zero_mean_zero_variance_is_converged_and_zero_mean_with_variance_is_not():
    fake = FakePixels([0.0, 0.0, 1.0], [0.0, 0.7, 0.0])
    _, _, counts, err, _ = run_policy(fake, 3, 0.01, 4, 32, 4)
    assert counts.tolist() == [4, 4, 4] and err.tolist() == [0.0, 0.0, 0.0]
    # a mean of 0 with a variance above 0 cannot come from radiance, but must not count as converged
    e = adaptive.relative_error(np.array([[0.0, 0.0, 0.0]]), np.array([[1.0, 1.0, 1.0]]), np.array([4]))
    assert np.isinf(e[0])


def test_max_spp_stops_and_clips_the_last_batch():
    fake = FakePixels(np.ones(4), [0.0, 0.2, 5.0, 50.0])
    _, _, counts, _, rounds = run_policy(fake, 4, 0.1, 4, 10, 4)
    assert counts.tolist() == [4, expected_count(0.2, 0.1, 4, 10, 4), 10, 10]
    assert [c[1:] for c in fake.calls] == [(0, 4), (4, 8), (8, 10)] and rounds == 3
    # min_spp == max_spp: one round only
    fake = FakePixels(np.ones(2), [9.0, 9.0])
    _, _, counts, _, rounds = run_policy(fake, 2, 0.1, 6, 6, 4)
    assert counts.tolist() == [6, 6] and rounds == 1


def test_colour_error_is_over_luminance():
    """A pixel noisy in blue only has a luminance error weighted by 0.0722."""
    n = 4
    sums = np.array([[4.0, 4.0, 4.0]])
    sq = np.array([[4.0, 4.0, 4.0 * (1 + 0.5 ** 2)]])  # blue: mean 1, unbiased variance 0.25 * 4 / 3
    sd_b = math.sqrt(0.25 * 4 / 3)
    want = adaptive.LUMA[2] * sd_b / math.sqrt(n) / 1.0
    assert adaptive.relative_error(sums, sq, np.array([n]))[0] == pytest.approx(want, rel=1e-12)


def test_bad_policy_arguments():
    fake = FakePixels([1.0], [0.0])
    for args in [(0.0, 4, 8, 4), (0.1, 1, 8, 4), (0.1, 8, 4, 4), (0.1, 4, 8, 0)]:
        with pytest.raises(ValueError):
            run_policy(fake, 1, *args)


def test_torch_tensors_take_the_same_decisions():
    torch = pytest.importorskip("torch")
    amps = np.array([0.0, 0.3, 0.9, 2.0, 7.0])

    def torch_render(fake):
        def f(pix, s0, s1, su, sq):
            a, b = fake(pix.numpy(), s0, s1, su.numpy(), sq.numpy())
            return torch.from_numpy(a), torch.from_numpy(b)
        return f

    fake_np, fake_t = FakePixels(np.ones(5), amps), FakePixels(np.ones(5), amps)
    _, _, c_np, e_np, r_np = run_policy(fake_np, 5, 0.2, 4, 40, 6)
    k = 5
    out = adaptive.run(torch_render(fake_t), torch.arange(k), torch.zeros((k, 3), dtype=torch.float64), torch.zeros((k, 3), dtype=torch.float64),
                       torch.zeros(k, dtype=torch.int64), 0.2, 4, 40, 6)
    assert out[2].tolist() == c_np.tolist() and out[4] == r_np
    assert np.array_equal(out[3].numpy(), e_np)


def test_render_adaptive_image_counts_and_stats_with_a_fake_renderer():
    """Renderer.render_adaptive over a tile: the pixel list it builds, the image sum * spp / n_q, and the summed statistics."""
    W, H = 12, 9
    p = T.make_params(W, H, 16, 1, tile=(2, 1, 10, 8))
    rng = np.random.default_rng(0)
    base, amp = rng.uniform(0.0, 2.0, W * H), rng.uniform(0.0, 2.0, W * H)
    base[: W * 3] = 0.0  # three black rows
    fake = FakePixels(base, amp)
    r = T.Renderer.__new__(T.Renderer)

    def render_pixels(params, pixels, s0, s1, sums, sumsq):
        su, sq = fake(pixels.astype(np.int64), s0, s1, sums, sumsq)
        st = T.Stats()
        st.rays_camera = len(pixels) * (s1 - s0)
        st.passes, st.max_bounces = 1, s1
        return su, sq, st

    r.render_pixels = render_pixels
    res = r.render_adaptive(p, 0.3, 4, 24, 4)
    ys, xs = np.arange(1, 8), np.arange(2, 10)
    assert res.image.shape == (7, 8, 3) and res.counts.shape == (7, 8) and res.error.shape == (7, 8)
    assert {q for call in fake.calls for q in call[0].tolist()} == set((ys[:, None] * W + xs[None, :]).reshape(-1).tolist())
    q = (ys[:, None] * W + xs[None, :])
    want_n = np.vectorize(lambda a, b: 4 if b == 0.0 else expected_count(a, 0.3, 4, 24, 4))(amp[q], base[q])
    assert (res.counts == want_n).all()
    assert (res.counts[:2] == 4).all()  # rows 1 and 2 of the tile are black
    # image = sum * spp / n_q with sums of the fake's raw values (even counts): the mean, base, times spp
    np.testing.assert_allclose(res.image[..., 1], base[q] * 16, rtol=1e-12, atol=1e-12)
    assert res.stats.rays_camera == int(res.counts.sum()) and res.stats.passes == res.rounds and res.stats.max_bounces == 24


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_version_5_in_header_and_mirror():
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    assert int(re.search(r"#define TRT_ABI_VERSION (\d+)", text).group(1)) == _abi.TRT_ABI_VERSION == 5
    assert _abi.load_hip().trt_abi_version() == 5


def test_render_pixels_signatures():
    assert {"trt_render_pixels", "trt_render_pixels_device"} <= set(_abi.HIP_SYMBOLS)
    lib = _abi.load_hip()
    assert lib.trt_render_pixels.argtypes == [C.c_void_p, C.POINTER(_abi.Params), C.c_uint32, C.POINTER(C.c_uint32), C.c_int32, C.c_int32,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_abi.Stats)]
    assert lib.trt_render_pixels_device.argtypes == [C.c_void_p, C.POINTER(_abi.Params), C.c_uint32, C.c_void_p, C.c_int32, C.c_int32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_abi.Stats)]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trt.h")).read(), flags=re.S)
    decl = re.search(r"int trt_render_pixels\((.*?)\);", text, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["h", "p", "n_pixels", "pixels", "sample_begin", "sample_end", "sum_host", "sumsq_host", "stats"]


def test_render_pixels_argument_checks_need_no_device():
    """The refusals that come before any device work: null pointers, bad ranges, the path-id range, a null handle."""
    lib = _abi.load_hip()
    p = T.make_params(16, 16, 4, 0)
    st = _abi.Stats()
    assert lib.trt_render_pixels(None, C.byref(p), 4, None, 0, 4, None, None, C.byref(st)) == 1
    assert b"null" in lib.trt_last_error()
