"""TRT_FLAG_ONE_LIGHT without a GPU: lightPick (csrc/trt_path.h, through the CPU build tests/onelight) against a float64 restatement of the
contract of include/trt.h; the statistical criterion the device test uses, shown to accept the estimator, to accept the reference against
itself and to reject an estimator that forgets the division by the probability; the flag's value in the header and the ABI mirror; the
stand-alone program under the host sanitizers.  (TRT_EINVAL for the flag without TRT_FLAG_FIXED_NEE needs a handle, and a handle needs a
device: tests/test_gpu_one_light.py checks it.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hostsim_lib as HS
import onelight_lib as OL
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LS = (2, 9, 65, 300)
U_EDGE = np.array([0.0, 1.0 - 2.0 ** -24, 2.0 ** -24, 0.5], np.float32)


def _tables():
    """(name, area [L], radiance [L, 3]) — the planted tables at every L, then random ones."""
    rng = np.random.default_rng(0x11A7)
    for L in LS:
        ones = np.ones((L, 3), np.float32)
        one = np.zeros(L, np.float32)
        one[L // 2] = 3.0
        yield f"one positive weight among zeros, L={L}", one, ones
        yield f"equal weights, L={L}", np.full(L, 0.75, np.float32), ones
        yield f"weights spanning 2^40, L={L}", (2.0 ** np.linspace(-20, 20, L)).astype(np.float32), ones
        yield f"weights spanning 2^40 downwards, L={L}", (2.0 ** np.linspace(20, -20, L)).astype(np.float32), ones
        yield f"all zero, L={L}", np.zeros(L, np.float32), ones
        for k in range(6):
            area = rng.uniform(0.01, 10.0, L).astype(np.float32)
            rad = rng.uniform(0.0, 40.0, (L, 3)).astype(np.float32)
            area[rng.random(L) < 0.2] = 0.0          # lights without area
            rad[rng.random(L) < 0.1] = 0.0           # black lights
            yield f"random {k}, L={L}", area, rad


def test_light_pick_against_the_float64_restatement():
    rng = np.random.default_rng(0xF64)
    cases = near = wrong = 0
    for name, area, rad in _tables():
        u = np.concatenate([U_EDGE, (rng.integers(0, 1 << 24, 2000) / np.float32(1 << 24)).astype(np.float32)])
        w = OL.weights(area, rad)
        cdf = OL.cdf32(w)
        for table in (True, False):
            got = OL.pick(area, rad, u, table=table)
            assert got["cdf"].tobytes() == cdf.tobytes(), name
            assert (got["draws"] == 1).all(), name
            assert (got["index"] < len(area)).all(), name
            if not (cdf[-1] > 0 and np.isfinite(cdf[-1])):
                assert not got["sampled"].any(), name  # the draw is spent, no light is sampled
                continue
            assert got["sampled"].all(), name
            idx = got["index"].astype(np.int64)
            assert (w[idx] > 0).all(), f"{name}: a light of weight zero was picked"
            want, margin = OL.pick_f64(w, cdf, u)
            differ = idx != want
            # r = u * cdf[-1] is rounded to fp32 on the device: where it lies within 4 ulp of a table entry the pick may be the neighbour's
            assert not (differ & (margin > 4.0)).any(), f"{name}: {int((differ & (margin > 4.0)).sum())} picks differ away from every table entry"
            cases += len(u)
            near += int((margin <= 4.0).sum())
            wrong += int(differ.sum())
            # inv_p * w_l / cdf[-1] within 2 ulp of 1
            ratio = got["inv_p"].astype(np.float64) * w[idx].astype(np.float64) / float(cdf[-1])
            assert np.abs(ratio - 1.0).max() <= 2.0 * 2.0 ** -23, f"{name}: inv_p off by {np.abs(ratio - 1.0).max() / 2.0 ** -23:.2f} ulp"
            want_inv = (np.float32(cdf[-1]) / w[idx]).astype(np.float32)  # one fp32 division
            assert got["inv_p"].tobytes() == want_inv.tobytes(), name
    print(f"{cases} picks, {near} within 4 ulp of a table entry, {wrong} of those differ from the float64 search")
    assert wrong <= 0.01 * cases


def test_fewer_than_two_lights_spend_no_draw():
    for L in (0, 1):
        got = OL.pick(np.full(L, 2.0, np.float32), np.ones((L, 3), np.float32), U_EDGE)
        assert (got["draws"] == 0).all() and (got["index"] == 0).all()
        assert got["sampled"].all() == (L == 1) and got["sampled"].any() == (L == 1)
        assert (got["inv_p"] == 1.0).all()


def test_hostile_weights_are_zero():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    area = np.array([nan, -1.0, 0.0, inf, 2.0, 2.0, 2.0, 2.0, 1.0], np.float32)
    rad = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [nan, 1, 1], [-5, 0, 0], [inf, 0, 0], [0, 0, 0], [1, 2, 3]], np.float32)
    w = OL.weights(area, rad)
    assert (w[:-1] == 0).all() and w[-1] > 0
    got = OL.pick(area, rad, np.linspace(0, 1, 101, endpoint=False).astype(np.float32))
    assert got["sampled"].all() and (got["index"] == 8).all() and (got["inv_p"] == 1.0).all()


# ---- the statistical criterion ---------------------------------------------------------------------------------------------------------
N = 8
SEED_A, SEED_B, SEED_C = 0x0A11CE, 0x0B0B00, 0x0C0FFE
CRITERION_SCENES = [("lamps", {"n": 8}), ("staircase", {})]


def _criterion_scene(name, kw):
    s = get_scene(name, 24, 16, **kw)
    return s, T.make_params(24, 16, 1, 0, flags=OL.FLAGS)


@pytest.mark.parametrize("name,kw", CRITERION_SCENES, ids=[c[0] for c in CRITERION_SCENES])
def test_all_lights_mode_of_the_cpu_build_is_hostsim_render(name, kw):
    """What the criterion's reference rests on: mode ALL_LIGHTS of the CPU build is hostsim_render with TRT_FLAG_FIXED_NEE, bit for bit; and a scene
    of one light renders the same with the flag (no draw is taken)."""
    s, _ = _criterion_scene(name, kw)
    p = T.make_params(24, 16, 2, SEED_A, flags=T.TRT_FLAG_FIXED_NEE)
    ref, ref_rays = HS.render(s.flat, p)
    got, rays = OL.render(s.flat, p, OL.ALL_LIGHTS)
    assert got.tobytes() == ref.tobytes() and rays == ref_rays
    one, one_rays = OL.render(s.flat, T.make_params(24, 16, 2, SEED_A, flags=OL.FLAGS))
    assert one.tobytes() != ref.tobytes() and one_rays[1] < ref_rays[1]
    back = get_scene("back", 24, 16)
    a, ra = OL.render(back.flat, T.make_params(24, 16, 2, SEED_A, flags=OL.FLAGS))
    b, rb = HS.render(back.flat, p)
    assert a.tobytes() == b.tobytes() and ra == rb


@pytest.mark.parametrize("name,kw", CRITERION_SCENES, ids=[c[0] for c in CRITERION_SCENES])
def test_criterion_accepts_the_estimator_and_the_reference_and_rejects_the_mutant(name, kw):
    """N = 8 one-sample renders per image at 24 x 16: the smallest power of two at which (a), (b) and (c) all hold on both scenes.  Measured with
    the CPU build, as (share of hit pixels with |z| > 4, image-wide z) for (a) one-light against all-lights, (b) all-lights against all-lights with
    another seed, (c) the estimator without the division by the probability against all-lights:
        lamps n = 8 (246 hit pixels)   N = 2: (a) 0.055, 0.22  (b) 0.054, 0.19  (c) 0.160, 3.74    - (a) and (b) fail: two samples give no variance
                                       N = 4: (a) 0.012, 0.36  (b) 0.004, 1.07  (c) 0.120, 5.30    - (a) fails
                                       N = 8: (a) 0.000, 1.14  (b) 0.000, 1.12  (c) 0.193, 6.48
                                    N = 1024: (a) 0.008, 2.64  (b) 0.000, 0.07  (c) 0.882, 90.95
        staircase (384 hit pixels)     N = 2: (a) 0.078, 0.29  (b) 0.044, 0.02  (c) 0.109, 10.23
                                       N = 4: (a) 0.031, 0.16  (b) 0.003, 1.04  (c) 0.050, 14.45
                                       N = 8: (a) 0.005, 0.89  (b) 0.000, 1.17  (c) 0.034, 18.41
                                    N = 1024: (a) 0.000, 0.90  (b) 0.000, 1.02  (c) 0.893, 60.76
    (every power of two from 8 to 1024 passes all three on both scenes)."""
    s, p = _criterion_scene(name, kw)

    def image(seed, mode):
        q = T.make_params(24, 16, 1, seed, flags=OL.FLAGS)
        return OL.moments_of(OL.render_seeds(s.flat, q, N, mode))

    ref_a, ref_b = image(SEED_A, OL.ALL_LIGHTS), image(SEED_B, OL.ALL_LIGHTS)
    one, mutant = image(SEED_C, OL.FEATURE), image(SEED_C, OL.MUTANT_NO_WEIGHT)
    a = OL.criterion(*one, *ref_a)
    b = OL.criterion(*ref_a, *ref_b)
    c = OL.criterion(*mutant, *ref_a)
    print(f"{name} N={N}: (a) one-light vs all-lights {a}, (b) all-lights vs all-lights {b}, (c) mutant vs all-lights {c}")
    assert a[2] > 100
    assert OL.passes(a[0], a[1]), f"(a) one-light against all-lights: {a}"
    assert OL.passes(b[0], b[1]), f"(b) all-lights against itself: {b}"
    assert not OL.passes(c[0], c[1]), f"(c) the mutant passes: {c}"


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------

def test_flag_value_in_header_and_abi_mirror():
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    m = re.search(r"#define\s+TRT_FLAG_ONE_LIGHT\s+(\d+)u", text)
    assert m and int(m.group(1)) == 128 == _abi.TRT_FLAG_ONE_LIGHT == T.TRT_FLAG_ONE_LIGHT
    others = [int(x) for x in re.findall(r"#define\s+TRT_FLAG_(?!ONE_LIGHT)\w+\s+(\d+)u", text)]
    assert all(o & 128 == 0 for o in others)
    assert re.search(r"#define\s+TRT_ABI_VERSION\s+5\b", text)


def test_stand_alone_program_finishes_under_the_host_sanitizers(tmp_path):
    """tests/onelight/onelight_san.cpp with the CPU build compiled in, under AddressSanitizer and UBSan: `lamps` with 8 lamps at 16 x 9 x 2 spp in
    all three modes, then lightPick over hostile tables (NaN, negative, zero and infinite areas and radiances; 0, 1, 2 and 300 lights; u = 0 and
    1 - 2^-24; with and without the selection table): every index stays inside [0, L)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "onelight_san")
    libdir = os.path.join(ROOT, "tinyraytracing_amd", "lib")
    cmd = [cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
           "-ffp-contract=off", "-march=x86-64-v3", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyraytracing_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "onelight", "onelight_cpu.cpp"), os.path.join(ROOT, "tests", "onelight", "onelight_san.cpp"),
           "-L" + libdir, "-ltrt_host", "-Wl,-rpath," + libdir]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    # the inherited environment, unchanged but for the sanitizers' own options; the runtimes are linked statically into this stand-alone
    # program, and the link-order check is off so that it also starts where the environment preloads some other library
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe, os.path.join(ROOT, "scenes", "back")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
