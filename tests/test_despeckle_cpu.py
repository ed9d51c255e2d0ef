"""trt_despeckle without a GPU: the CPU build of the kernel's per-pixel code (tests/despeckle) agrees with the float64 restatement of the
contract (tests/despeckle_ref.py) on random frames with planted fireflies and on oracle frames; the exact properties of the contract, bit
for bit; what the clamp does to the filtered image's distance from a converged render (the figures DESIGN.md quotes); the C entries' argument
checks in their order, the Python wrappers and the ABI mirror; hostile values under the host sanitizers (a stand-alone driver)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as DN
import despeckle_ref as D
import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = [1, 2]
SCENES = ["back", "staircase", "veach-mis"]


def _bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


def _untouched(out, color, variance):
    return _bits(out["color"], color) and _bits(out["variance"], variance) and (out["scale"] == 1.0).all()


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def _against_restatement(color, variance, albedo, depth, what, **kw):
    got = D.cpu(color, albedo, depth, variance, **kw)
    want = D.restate(color, albedo, depth, variance, **kw)
    hit = want["hit"]
    share = float(want["edge"][hit].mean())
    print(f"{what} {kw}: {int(hit.sum())} hit pixels, {int(want['clamped'].sum())} clamped, {int(want['replaced'].sum())} replaced, "
          f"{int(want['edge'].sum())} within rounding of T (share {share:.4f})")
    D.compare(got, want, color, what)
    return want, share


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("seed,h,w", [(1, 37, 53), (2, 24, 32)])
def test_cpu_build_matches_the_float64_restatement_on_random_frames(seed, h, w, radius):
    (color, variance, albedo, _, depth), spikes, bad = D.spiked_inputs(h, w, seed)
    for sigma in (3.0, 1.5):
        want, share = _against_restatement(color, variance, albedo, depth, f"random {seed}", radius=radius, sigma=sigma)
        assert share <= D.MAX_EDGE_SHARE  # the restatement alone: how many pixels it excuses
        assert all(want["replaced"][y, x] or want["edge"][y, x] for y, x in bad if want["hit"][y, x] and radius == 2)
        # the planted fireflies are clamped wherever they stand alone in their window
        assert sum(bool(want["clamped"][y, x]) for y, x in spikes) >= len(spikes) // 2
        assert 0 < want["clamped"].sum() < 0.2 * want["hit"].sum()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", SCENES)
def test_cpu_build_matches_the_float64_restatement_on_oracle_frames(name, radius):
    color, variance, albedo, _, depth = D.oracle_frame(name, 4, None)
    want, _ = _against_restatement(color, variance, albedo, depth, name, radius=radius)
    assert want["clamped"].sum() > 0 and not want["replaced"].any()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", SCENES)
def test_restatement_excuses_at_most_half_a_percent_of_an_oracle_frame(name, radius):
    """The cap on the pixels whose decision is left open, on the restatement alone: 0 of 2102 (back) and 0 of 3072 (staircase, veach-mis) hit
    pixels at either radius.  The pixels inside a directly seen emitter, where the pixel and all its taps carry one value and l_p = m = T is a
    tie (84 and 48 pixels of staircase at R = 1 and 2, 34 and 10 of veach-mis), are not among them because the contract decides a flat window by
    comparison (step 6); summed and divided in fp32 they would be open, and more than the cap allows."""
    color, variance, albedo, _, depth = D.oracle_frame(name, 4, None)
    want = D.restate(color, albedo, depth, variance, radius=radius)
    flagged, hits = int(want["edge"].sum()), int(want["hit"].sum())
    print(f"{name} R = {radius}: {flagged} of {hits} hit pixels within rounding of T ({100 * flagged / hits:.2f} %), {int(want['flat'].sum())} in flat windows")
    assert flagged <= D.MAX_EDGE_SHARE * hits


# ---- exact properties ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", RADII)
def test_constant_image_is_untouched(radius):
    for value, albedo in ((1.0, 1.0), (0.37, 0.61), (0.75, 0.5), (3.1, 0.25), (0.0, 0.5), (1.0, 0.0)):
        color, alb, depth, variance = D.field(11, 13, value, albedo)
        assert _untouched(D.cpu(color, alb, depth, variance, radius=radius), color, variance)


@pytest.mark.parametrize("radius", RADII)
def test_flat_windows_of_any_value_are_untouched(radius):
    """400 tiles of 7 x 7 pixels, each of one random value: l_p = m = T in exact arithmetic.  Summed and divided in fp32, m falls an ulp or two
    short of l_p for about 1 % (R = 1) and 4 % (R = 2) of the values; the contract decides a flat window by comparison, and every tile's centre
    keeps its bits."""
    rng = np.random.default_rng(radius)
    lum = rng.uniform(0.01, 20.0, size=(16, 25)).astype(np.float32).repeat(7, 0).repeat(7, 1)
    color = np.repeat(lum[..., None], 3, axis=2) * np.float32([1.0, 0.5, 0.25])
    albedo = np.full(color.shape, 0.5, np.float32)
    depth, variance = np.full(lum.shape, 2.0, np.float32), np.full(lum.shape, 0.1, np.float32)
    out = D.cpu(color, albedo, depth, variance, radius=radius)
    assert (out["scale"][3::7, 3::7] == 1.0).all() and _bits(out["color"][3::7, 3::7], color[3::7, 3::7])
    assert D.restate(color, albedo, depth, variance, radius=radius)["flat"][3::7, 3::7].all()


@pytest.mark.parametrize("radius", RADII)
def test_one_spike_comes_down_to_the_field(radius):
    color, albedo, depth, variance = D.field(9, 9)
    color[4, 4] = 1e4
    keep = [x.copy() for x in (color, albedo, depth, variance)]
    out = D.cpu(color, albedo, depth, variance, radius=radius)
    s = np.float32(1e-4)
    assert (out["color"][4, 4] == 1.0).all() and out["scale"][4, 4] == s
    assert out["variance"][4, 4] == (np.float32(0.25) * s) * s
    others = np.ones((9, 9), bool)
    others[4, 4] = False
    assert _bits(out["color"][others], color[others]) and _bits(out["variance"][others], variance[others]) and (out["scale"][others] == 1.0).all()
    # inputs are not modified
    assert all(_bits(a, b) for a, b in zip(keep, (color, albedo, depth, variance)))
    # the optional buffers change nothing else
    assert _bits(D.cpu(color, albedo, depth, radius=radius)["color"], out["color"])
    assert _bits(D.cpu(color, albedo, depth, variance, want_scale=False, radius=radius)["variance"], out["variance"])


def test_two_adjacent_spikes():
    """Each of two adjacent fireflies is one bright tap of the other's window.  At R = 2 that is f = 1 / 24 < 0.1 and both are reduced; at
    R = 1 it is f = 1 / 8 > 0.1, the rule that protects one-pixel lines protects them too, and both stay (include/trt.h says so)."""
    color, albedo, depth, variance = D.field(9, 9)
    color[4, 4] = color[4, 5] = 1e4
    out = D.cpu(color, albedo, depth, variance, radius=2)
    assert (out["scale"][4, 4:6] < 1.0).all() and (out["scale"][4, 4:6] > 0.0).all() and (out["color"][4, 4:6] < 1e4).all()
    assert _bits(out["color"][4, 4], out["color"][4, 5]) and (out["scale"] != 1.0).sum() == 2
    assert _untouched(D.cpu(color, albedo, depth, variance, radius=1), color, variance)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", ["edge", "corner", "line_h", "line_v"])
def test_edges_corners_and_lines_are_untouched_at_contrast_100(shape, radius):
    h, w = 15, 17
    lum = np.ones((h, w), np.float32)
    if shape == "edge":
        lum[:, 8:] = 100.0
    elif shape == "corner":
        lum[6:, 7:] = 100.0  # a bright quadrant: its corner pixel (6, 7) has 3 of 8 (8 of 24) bright taps
    elif shape == "line_h":
        lum[7, :] = 100.0
    else:
        lum[:, 8] = 100.0
    # grey 0.5 and 50 over an albedo of 0.5: the luminances are 1 and 100 bit for bit, every sum of the window is exact, and the constant
    # stretches on either side of the feature are no rounding ties
    color = np.repeat(lum[..., None], 3, axis=2) * np.float32(0.5)
    albedo = np.full((h, w, 3), 0.5, np.float32)
    depth, variance = np.full((h, w), 3.0, np.float32), np.full((h, w), 0.5, np.float32)
    assert _untouched(D.cpu(color, albedo, depth, variance, radius=radius), color, variance)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_inf_centre_pixels_are_replaced_by_the_mean(bad, radius):
    color, albedo, depth, variance = D.field(7, 7, 0.5, 0.25)
    albedo[3, 3] = (0.5, 0.0, 0.125)  # a black channel demodulates by 1
    for channels in ((0,), (0, 1, 2)):
        c = color.copy()
        c[3, 3, list(channels)] = bad
        out = D.cpu(c, albedo, depth, variance, radius=radius)
        m = np.float32(out["color"][3, 3, 1])  # m * 1
        assert m == np.float32(D.restate(c, albedo, depth, radius=radius)["mean"][3, 3]) and abs(m - 2.0) < 1e-6
        assert (out["color"][3, 3] == m * np.float32([0.5, 1.0, 0.125])).all() and out["scale"][3, 3] == 0.0 and out["variance"][3, 3] == variance[3, 3]
        assert (out["scale"].ravel() == 1.0).sum() == 48 and np.isfinite(out["color"]).all()  # the neighbours do not count it, and stay
    # a variance that is not a number goes to 0 with the replaced pixel, and only there
    c, v = color.copy(), variance.copy()
    c[3, 3, 1] = bad
    v[3, 3] = v[0, 0] = np.nan
    out = D.cpu(c, albedo, depth, v, radius=radius)
    assert out["variance"][3, 3] == 0.0 and np.isnan(out["variance"][0, 0]) and out["scale"][0, 0] == 1.0


@pytest.mark.parametrize("radius", RADII)
def test_nan_neighbours_and_misses_do_not_count(radius):
    """A spike among neighbours of which some are NaN, infinite or misses: the result is the one of the same image with those pixels turned
    into misses, and T is formed from the others alone."""
    color, albedo, depth, variance = D.field(9, 9, 0.5, 0.5)
    color[4, 4] = 300.0
    a, b = color.copy(), depth.copy()
    a[3, 3], a[4, 5, 2], a[5, 4] = np.nan, np.inf, 7.0
    b[5, 4] = DN.INF           # a miss with a bright colour
    b[3, 5] = np.nan            # a NaN depth is a miss
    out = D.cpu(a, albedo, b, variance, radius=radius)
    assert (out["color"][4, 4] == 0.5).all() and out["scale"][4, 4] == np.float32(1.0) / np.float32(600.0)  # T = 1, l_p = 300 / 0.5
    assert _bits(out["color"][5, 4], a[5, 4]) and _bits(out["color"][3, 5], a[3, 5]) and out["scale"][5, 4] == 1.0 and out["scale"][3, 5] == 1.0
    # the two pixels that are not numbers are replaced by the mean of THEIR counting taps, the spike among them
    want = D.restate(a, albedo, b, variance, radius=radius)
    for y, x in ((3, 3), (4, 5)):
        assert out["scale"][y, x] == 0.0 and want["replaced"][y, x]
        np.testing.assert_allclose(out["color"][y, x], want["mean"][y, x] * 0.5, rtol=D.RTOL)


def test_fewer_than_three_taps_pass_through():
    for bad in (50.0, np.nan, np.inf):
        for h, w in ((1, 1), (1, 2)):  # a 1 x 1 and a 2 x 1 image: no pixel has three taps, at either radius
            color, albedo, depth, variance = D.field(h, w)
            color[0, 0] = bad
            for radius in RADII:
                assert _untouched(D.cpu(color, albedo, depth, variance, radius=radius), color, variance)
        # a hit among misses, with two hit neighbours
        color, albedo, depth, variance = D.field(7, 7)
        depth[:] = DN.INF
        depth[3, 3] = depth[3, 4] = depth[2, 2] = 4.0
        color[3, 3] = bad
        for radius in RADII:
            assert _untouched(D.cpu(color, albedo, depth, variance, radius=radius), color, variance)
        # a third neighbour, and the pixel is dealt with
        depth[4, 3] = 4.0
        assert D.cpu(color, albedo, depth, variance, radius=1)["scale"][3, 3] != 1.0
    # 1 x 3 at R = 1 has two taps at most, at R = 2 too; 1 x 4 at R = 2 has three for the inner pixels
    color, albedo, depth, variance = D.field(1, 4)
    color[0, 1] = 1e3
    assert _untouched(D.cpu(color, albedo, depth, variance, radius=1), color, variance)
    assert D.cpu(color, albedo, depth, variance, radius=2)["scale"][0, 1] < 1.0


def test_defaults_are_filled_in():
    out = (C.c_float * 2)()
    assert D.lib().despeckle_cpu_defaults(C.byref(D.params(0, 0.0)), out) == 0 and list(out) == [1.0, 3.0]
    assert D.lib().despeckle_cpu_defaults(None, out) == 0 and list(out) == [1.0, 3.0]
    assert D.lib().despeckle_cpu_defaults(C.byref(D.params(2, 1.5)), out) == 0 and list(out) == [2.0, 1.5]
    (color, variance, albedo, _, depth), _, _ = D.spiked_inputs(12, 10, 3)
    a, b = D.cpu(color, albedo, depth, variance, radius=0, sigma=0.0), D.cpu(color, albedo, depth, variance)
    assert all(_bits(a[k], b[k]) for k in D.OUT_KEYS)


# ---- quality -------------------------------------------------------------------------------------------------------------------------

def _quality(name):
    """Per case of D.QUALITY_CASES: (MSE filtered, MSE clamped then filtered, clamped pixels, hit pixels, mean after / before the clamp of the
    filtered image), at R = 1 and sigma 3, the filter = the CPU build of trt_denoise, against the 512-spp oracle render."""
    ref = D.converged(name)
    rows = []
    for spp, seed in D.QUALITY_CASES:
        color, variance, albedo, normal, depth = D.oracle_frame(name, spp, seed)
        plain = DN.cpu(color, variance, albedo, normal, depth)
        ds = D.cpu(color, albedo, depth, variance, radius=1, sigma=3.0)
        clamped = DN.cpu(ds["color"], ds["variance"], albedo, normal, depth)
        assert np.isfinite(plain).all() and np.isfinite(clamped).all()
        rows.append((D.tonemapped_mse(plain, ref), D.tonemapped_mse(clamped, ref), int((ds["scale"] != 1.0).sum()), int((depth < DN.INF).sum()),
                     float(clamped.astype(np.float64).mean() / plain.astype(np.float64).mean())))
    for (spp, seed), (a, b, n, hits, e) in zip(D.QUALITY_CASES, rows):
        print(f"{name} spp {spp} seed {seed}: filtered {a:.5f}, clamped then filtered {b:.5f} (ratio {b / a:.3f}), {n} of {hits} pixels clamped, "
              f"mean after the filter {100 * (e - 1):+.1f} %")
    return rows


def test_quality_staircase_gets_closer_to_the_converged_image():
    """Measured with the CPU build: ratios 0.795 / 0.713 / 0.617, 168 / 173 / 213 of 3072 pixels clamped, mean -3.5 / -4.5 / -8.6 %."""
    for a, b, *_ in _quality("staircase"):
        assert b <= 0.9 * a


def test_quality_back_is_neutral():
    """Measured with the CPU build: ratios 0.997 / 0.995 / 0.986, 77 / 69 / 111 of 2102 / 2095 / 2102 hit pixels clamped, mean -0.4 / -0.6 / -1.4 %."""
    for a, b, *_ in _quality("back"):
        assert b <= 1.01 * a


def test_quality_veach_mis_is_finite():
    """Small emitters and their highlights are clamped with the fireflies: nothing is asserted but finiteness, the figures are printed
    (measured with the CPU build: ratios 1.003 / 1.030 / 1.011, 80 / 101 / 99 of 3072 pixels clamped, mean -2.8 / -7.8 / -7.2 %)."""
    _quality("veach-mis")


# ---- robustness, under the host sanitizers ------------------------------------------------------------------------------------------

def test_hostile_values_finish_under_the_host_sanitizers(tmp_path):
    """NaN, infinite and negative colours, zero and negative albedos and NaN depths at 1 x 1, 1 x 40 and 17 x 3: a stand-alone program
    (tests/despeckle/despeckle_san.cpp with the CPU build compiled in) under AddressSanitizer and UBSan."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "despeckle_san")
    cmd = [cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
           "-ffp-contract=off", "-march=x86-64-v3", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyraytracing_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "despeckle", "despeckle_cpu.cpp"), os.path.join(ROOT, "tests", "despeckle", "despeckle_san.cpp")]
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

# color, variance, albedo, depth | out_color, out_variance, out_scale
SHAPES = [3, 1, 3, 1, 3, 1, 1]
REQUIRED = (0, 2, 3, 4)


def _entry_args(w=4, h=4):
    bufs = [np.zeros((h, w, c), np.float32) for c in SHAPES]
    return bufs, [b.ctypes.data_as(D.fp) for b in bufs]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_despeckle_entries_check_their_arguments_in_order_before_the_device():
    lib = _abi.load_hip()
    keep, ptrs = _entry_args()

    def host(p, w, h, bufs):
        return lib.trt_despeckle(0, p, w, h, *bufs, None)

    def dev(p, w, h, bufs):
        return lib.trt_despeckle_device(0, p, w, h, *[C.cast(b, C.c_void_p) if b else None for b in bufs], None, None)

    def cpu(p, w, h, bufs):
        return D.lib().despeckle_cpu(p, w, h, *bufs)

    nan = float("nan")
    good = D.params()
    # the order: each case is wrong in the named way AND in every later way; the named message must come
    worst = D.params(radius=3, sigma=-1.0, flags=1)
    for call in (host, dev):
        for i in REQUIRED:
            bufs = list(ptrs)
            bufs[i], bufs[1] = None, None  # and a variance without its output
            assert call(C.byref(worst), 0, 1 << 30, bufs) == 1 and b"null buffer" in lib.trt_last_error(), i
        for i in (1, 5):
            bufs = list(ptrs)
            bufs[i] = None
            assert call(C.byref(worst), 0, 1 << 30, bufs) == 1 and b"both or neither" in lib.trt_last_error(), i
        assert call(C.byref(worst), 0, 1 << 30, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(good), 4, -3, ptrs) == 1 and b">= 1" in lib.trt_last_error()
        assert call(C.byref(worst), 1 << 15, (1 << 13) + 1, ptrs) == 1 and b"2^28" in lib.trt_last_error()
        for radius in (3, -1, 1 << 20):
            assert call(C.byref(D.params(radius=radius, sigma=-1.0, flags=1)), 4, 4, ptrs) == 1 and b"radius" in lib.trt_last_error()
        for sigma in (-1.0, -1e-30, nan, float("-inf")):
            assert call(C.byref(D.params(sigma=sigma, flags=1)), 4, 4, ptrs) == 1 and b"sigma" in lib.trt_last_error()
        for flags in (1, 16, 1 << 31):
            assert call(C.byref(D.params(flags=flags)), 4, 4, ptrs) == 1 and b"flags" in lib.trt_last_error()
    if not _gpu_present():
        # valid arguments reach the device check: no gfx950 here.  The variance pair and out_scale are optional, params may be null
        for bufs in (ptrs, [ptrs[0], None] + ptrs[2:5] + [None, ptrs[6]], ptrs[:6] + [None], [ptrs[0], None] + ptrs[2:5] + [None, None]):
            for p in (C.byref(good), None, C.byref(D.params(0, 0.0)), C.byref(D.params(2, float("inf")))):
                for call in (host, dev):
                    assert call(p, 4, 4, bufs) == 4
    # the CPU build refuses the same arguments and takes the same ones
    assert cpu(C.byref(D.params(radius=3)), 4, 4, ptrs) == 1 and cpu(C.byref(good), 4, 4, ptrs[:5] + [None, ptrs[6]]) == 1
    assert cpu(C.byref(good), 4, 4, [None] + ptrs[1:]) == 1 and cpu(C.byref(D.params(sigma=nan)), 4, 4, ptrs) == 1
    assert cpu(C.byref(good), 4, 4, ptrs) == 0 and cpu(None, 4, 4, [ptrs[0], None] + ptrs[2:5] + [None, None]) == 0
    del keep


def test_python_layer_checks_shapes_and_parameters():
    (color, variance, albedo, _, depth), _, _ = D.spiked_inputs(6, 5, 14)
    with pytest.raises(T.TrtError, match="color"):
        T.despeckle(color[..., :2], albedo, depth)
    with pytest.raises(T.TrtError, match="albedo"):
        T.despeckle(color, albedo[:, :4], depth)
    with pytest.raises(T.TrtError, match="albedo"):
        T.despeckle(color, None, depth)
    with pytest.raises(T.TrtError, match="depth"):
        T.despeckle(color, albedo, depth[None])
    with pytest.raises(T.TrtError, match="variance"):
        T.despeckle(color, albedo, depth, variance=variance[:3])
    with pytest.raises(T.TrtError, match="radius"):
        T.despeckle(color, albedo, depth, radius=3)
    with pytest.raises(T.TrtError, match="sigma"):
        T.despeckle(color, albedo, depth, variance=variance, sigma=-2.0)
    with pytest.raises(T.TrtError, match="despeckle_into"):
        T.despeckle_into(color, albedo, depth, None)  # numpy arrays are not device tensors
    if not _gpu_present():
        with pytest.raises(T.TrtError, match=r"trt_despeckle failed \(4\)"):
            T.despeckle(color, albedo, depth, variance=variance)
    # the accumulator's argument: off by default, True or a dict of radius / sigma, an unknown key refused
    one = T.make_params(16, 12, 1, 1)
    assert T.TemporalAccumulator(None, one, variance="moments").despeckle_kw is None
    assert T.TemporalAccumulator(None, one, variance="moments", despeckle=True).despeckle_kw == {}
    assert T.TemporalAccumulator(None, one, variance="moments", despeckle={"radius": 2, "sigma": 2.5}).despeckle_kw == {"radius": 2, "sigma": 2.5}
    with pytest.raises(T.TrtError, match="unknown despeckle key sigm"):
        T.TemporalAccumulator(None, one, variance="moments", despeckle={"sigm": 2.0})
    with pytest.raises(T.TrtError, match="despeckle must be"):
        T.TemporalAccumulator(None, one, variance="moments", despeckle=3)


def test_despeckle_symbols_are_declared_exported_and_mirrored():
    hip = C.CDLL(os.path.join(_abi.LIB_DIR, "libtrt_hip.so"))
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    for n in ("trt_despeckle", "trt_despeckle_device"):
        assert hasattr(hip, n) and n in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + n + r"\(", text)
        assert getattr(_abi.load_hip(), n).argtypes is not None
    assert len(_abi.load_hip().trt_despeckle.argtypes) == 12 and len(_abi.load_hip().trt_despeckle_device.argtypes) == 13
    assert C.sizeof(_abi.DespeckleParams) == 12
    fields = re.search(r"typedef struct trt_despeckle_params \{(.*?)\} trt_despeckle_params;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields)) == [f[0] for f in _abi.DespeckleParams._fields_]
    assert re.search(r"#define TRT_DS_MIN_TAPS 3\b", text)
    for k in ("despeckle", "despeckle_into"):
        assert hasattr(T, k)
    import inspect
    assert inspect.signature(T.TemporalAccumulator.__init__).parameters["despeckle"].default is None
    # what must not move
    assert _abi.TRT_ABI_VERSION == 5 and len(_abi.KERNEL_NAMES) == 6 and re.search(r"#define TRT_MAX_KERNELS 8\b", text)
