"""TRT_FLAG_NEAR_LIGHTS without a GPU: buildLightTree (csrc/trt_lighttree.h) and lightPickNear (csrc/trt_path.h), through the CPU build tests/nearlights,
against the restatement of the contract of include/trt.h in tests/nearlights_lib.py; hostile light tables; the statistical criterion of the one-light
tests, shown to accept the estimator, to accept the reference against itself and to reject two estimators with a wrong inv_p; the variance the descent
buys on a corridor of lamps; the flag's value in the header and the ABI mirror; the stand-alone program under the host sanitizers.  (TRT_EINVAL for the
flag without TRT_FLAG_ONE_LIGHT needs a handle, and a handle needs a device: tests/test_gpu_near_lights.py checks it.)"""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import near_cases as NC
import nearlights_lib as NL
import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23


TABLES = list(NL.shared_tables())


@pytest.mark.parametrize("name,t", TABLES, ids=[x[0] for x in TABLES])
def test_tree_invariants_and_the_restatement(name, t):
    nodes, root, M = NL.tree(t)
    w = NL.weights(t.area, t.radiance)
    want = [x[0] for x in NL.tree_lights(t)]
    assert M == len(want) and len(nodes) == max(M, 1) - 1
    assert M >= 2 and root == 0, name
    depth = NL.depth_of(nodes, root)  # (asserts that no light sits in two leaves)
    assert sorted(depth) == want, "every tree light in exactly one leaf, no other light in the tree"
    assert all(w[l] > 0 for l in depth), "a light of weight zero is in the tree"
    assert max(depth.values()) <= math.ceil(math.log2(M)), f"depth {max(depth.values())} for {M} tree lights"
    # child weights are the fp32 sums, boxes contain their lights' vertices: by the restatement's nodes bit for bit, and directly
    ref_nodes, ref_root, ref_M = NL.build(t)
    assert (ref_root, ref_M) == (root, M)
    assert nodes.tobytes() == ref_nodes.tobytes(), f"{name}: {int((nodes != ref_nodes).sum())} nodes differ from the restatement"

    def lights_under(ref):
        if ref & NL.LEAF:
            return [ref & ~NL.LEAF]
        return lights_under(int(nodes["child0"][ref])) + lights_under(int(nodes["child1"][ref]))

    for i in range(len(nodes)):
        for c in ("0", "1"):
            under = lights_under(int(nodes["child" + c][i]))
            v = np.concatenate([t.verts[int(t.tri_first[l]):int(t.tri_first[l]) + int(t.tri_count[l])].reshape(-1, 3) for l in under])
            assert (v >= nodes["lo" + c][i]).all() and (v <= nodes["hi" + c][i]).all()
            assert (v.min(axis=0) == nodes["lo" + c][i]).all() and (v.max(axis=0) == nodes["hi" + c][i]).all(), "the box is not the exact one"
            total = float(w[under].astype(np.float64).sum())
            assert abs(float(nodes["w" + c][i]) - total) <= len(under) * ULP * total


def _points(t, rng, m=600):
    """Random points inside and far outside the lights' bounds, the light centres themselves, points at 1e30."""
    v = t.verts.reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    inside = rng.uniform(lo - 1.0, hi + 1.0, (m, 3))
    outside = rng.uniform(-1.0, 1.0, (m // 4, 3)) * 1.0e4
    centres = np.array([x[3] for x in NL.tree_lights(t)])
    far = np.array([[1e30, 0, 0], [0, -1e30, 0], [1e30, 1e30, 1e30], [-1e30, 1e30, 0]])
    return np.concatenate([inside, outside, centres, far]).astype(np.float32)


@pytest.mark.parametrize("name,t", TABLES, ids=[x[0] for x in TABLES])
def test_descent_against_the_restatement(name, t):
    rng = np.random.default_rng(0xDE5C)
    nodes, root, M = NL.tree(t)
    depth = NL.depth_of(nodes, root)
    P = _points(t, rng)
    m = len(P)
    cases = near = wrong = 0
    for kind in ("random", "zero", "last", "stream"):
        U = {"random": (rng.integers(0, 1 << 24, (m, NL.MAX_DEPTH)) / np.float32(1 << 24)).astype(np.float32),
             "zero": np.zeros((m, NL.MAX_DEPTH), np.float32), "last": np.full((m, NL.MAX_DEPTH), 1.0 - 2.0 ** -24, np.float32), "stream": None}[kind]
        got = NL.pick(t, P, U)
        assert (got["index"] < t.n).all() and got["sampled"].all(), f"{name} {kind}"
        idx = got["index"].astype(np.int64)
        assert all(int(l) in depth for l in idx), f"{name} {kind}: a light outside the tree was picked"
        assert (got["draws"] == np.array([depth[int(l)] for l in idx])).all(), f"{name} {kind}: the draws are not the depth of the leaf"
        want = NL.descend(nodes, root, P, got["u"])
        differ = idx != want["index"]
        # r = u * s is rounded to fp32 in the build: within 4 ulp of imp0 the pick may be the sibling's
        assert not (differ & (want["margin"] > 4.0)).any(), f"{name} {kind}: {int((differ & (want['margin'] > 4.0)).sum())} picks differ away from every decision"
        cases += m
        near += int((want["margin"] <= 4.0).sum())
        wrong += int(differ.sum())
        same = ~differ
        assert got["inv_p"][same].tobytes() == want["inv_p32"][same].tobytes(), f"{name} {kind}: inv_p is not the fp32 product of the contract"
        off = np.abs(got["inv_p"][same].astype(np.float64) * want["prob"][same] - 1.0)
        assert (off <= got["draws"][same] * 2.0 * ULP).all(), f"{name} {kind}: inv_p * probability off by {off.max() / ULP:.2f} ulp"
    print(f"{name}: {cases} picks, {near} within 4 ulp of a decision, {wrong} of those differ from the float64 decision")
    assert wrong <= 0.01 * cases
    prob = NL.probabilities(nodes, root, t.n, P[::7])
    assert np.abs(prob.sum(axis=1) - 1.0).max() <= 1e-5
    tree = np.zeros(t.n, bool)
    tree[list(depth)] = True
    assert (prob[:, ~tree] == 0).all()
    assert (prob[:, tree] > 0).all(), "a tree light without probability"


def test_hostile_tables_never_enter_the_tree():
    t = NL.hostile_tables()
    nodes, root, M = NL.tree(t)
    depth = NL.depth_of(nodes, root)
    assert sorted(depth) == [11, 12, 13] == [x[0] for x in NL.tree_lights(t)] and M == 3
    rng = np.random.default_rng(3)
    got = NL.pick(t, rng.uniform(-50, 50, (500, 3)))
    assert got["sampled"].all() and set(got["index"].tolist()) == {11, 12, 13}
    assert np.isfinite(nodes.view(np.float32).reshape(-1, 16)[:, :14]).all()


def test_no_tree_light_and_one_tree_light_take_no_draw():
    P = np.random.default_rng(4).uniform(-5, 5, (64, 3))
    none = NL.Tables.quads(np.zeros(5), np.ones((5, 3)), np.zeros((5, 3)), 1.0)
    assert NL.tree(none)[1:] == (NL.NONE, 0) == NL.build(none)[1:]
    got = NL.pick(none, P)
    assert not got["sampled"].any() and (got["draws"] == 0).all() and (got["index"] == 0).all()
    area = np.zeros(5, np.float32)
    area[3] = 2.0
    one = NL.Tables.quads(area, np.ones((5, 3)), np.zeros((5, 3)), 1.0)
    assert NL.tree(one)[1:] == (NL.LEAF | 3, 1) == NL.build(one)[1:]
    got = NL.pick(one, P)
    assert got["sampled"].all() and (got["draws"] == 0).all() and (got["index"] == 3).all() and (got["inv_p"] == 1.0).all()
    for L in (0, 1):  # fewer than two lights: the flag does nothing
        few = NL.Tables.quads(np.full(L, 2.0), np.ones((L, 3)), np.zeros((L, 3)), 1.0)
        got = NL.pick(few, P)
        assert (got["draws"] == 0).all() and (got["index"] == 0).all() and (got["inv_p"] == 1.0).all() and got["sampled"].all() == (L == 1) == bool(got["sampled"].any())


# ---- the statistical criterion ---------------------------------------------------------------------------------------------------------
N = 8            # lamps, staircase: the N of tests/test_one_light_cpu.py
N_CORRIDOR = 64  # corridor(16): the smallest power of two at which both mutants fail there (docstring below)
SEED_A, SEED_B, SEED_C = 0x0A11CE, 0x0B0B00, 0x0C0FFE
CRITERION_SCENES = {"lamps": N, "staircase": N, "corridor": N_CORRIDOR}


def criterion_scene(name):
    return NC.corridor(16, 24, 16) if name == "corridor" else get_scene(name, 24, 16, **({"n": 8} if name == "lamps" else {}))


def _moments(s, seed, mode, n):
    return NL.moments_of(NL.render_seeds(s.flat, T.make_params(24, 16, 1, seed, flags=NL.FLAGS), n, mode))


def test_modes_of_the_cpu_build_are_the_one_light_build_and_hostsim():
    """What the criterion's reference and the variance comparison rest on: the modes ALL_LIGHTS and ONE_LIGHT of this CPU build are those of
    tests/onelight's, bit for bit."""
    import onelight_lib as OL
    for name in CRITERION_SCENES:
        s = criterion_scene(name)
        p = T.make_params(24, 16, 2, SEED_A, flags=NL.FLAGS)
        for mine, theirs in ((NL.ALL_LIGHTS, OL.ALL_LIGHTS), (NL.ONE_LIGHT, OL.FEATURE)):
            a, ra = NL.render(s.flat, p, mine)
            b, rb = OL.render(s.flat, p, theirs)
            assert a.tobytes() == b.tobytes() and ra == rb, name
        near, _ = NL.render(s.flat, p, NL.NEAR)
        assert near.tobytes() != b.tobytes(), name
    back = get_scene("back", 24, 16)
    a, ra = NL.render(back.flat, p, NL.NEAR)
    b, rb = NL.render(back.flat, p, NL.ALL_LIGHTS)
    assert a.tobytes() == b.tobytes() and ra == rb  # one light: the flag does nothing


_verdicts = {}


@pytest.mark.parametrize("name", list(CRITERION_SCENES))
def test_criterion_accepts_the_estimator_and_the_reference(name):
    """One-sample renders at 24 x 16, as (share of hit pixels with |z| > 4, image-wide z) for (a) NEAR against all-lights, (b) all-lights against all-lights
    with another seed, (c1) inv_p forced to 1 against all-lights, (c2) inv_p = TRT_FLAG_ONE_LIGHT's cdf / w on the tree's pick against all-lights.
    Measured with the CPU build (F = fails the criterion):
        lamps n = 8 (244 hit pixels)   N =  8: (a) 0.000, 1.66  (b) 0.000, 1.12  (c1) 0.168,  9.19 F  (c2) 0.000, 0.59
                                       N = 16: (a) 0.000, 2.86  (b) 0.000, 1.06  (c1) 0.332, 12.72 F  (c2) 0.000, 0.47
                                       N = 32: (a) 0.004, 1.98  (b) 0.000, 1.50  (c1) 0.520, 12.07 F  (c2) 0.004, 2.08
        staircase (384 hit pixels)     N =  8: (a) 0.000, 0.79  (b) 0.000, 1.17  (c1) 0.005,  7.41 F  (c2) 0.003,  6.51 F
                                       N = 16: (a) 0.000, 0.76  (b) 0.000, 1.35  (c1) 0.000, 11.41 F  (c2) 0.003,  9.08 F
                                       N = 32: (a) 0.000, 0.07  (b) 0.000, 0.54  (c1) 0.013, 15.10 F  (c2) 0.005, 10.80 F
        corridor(16) (45 hit pixels)   N =  8: (a) 0.000, 0.72  (b) 0.000, 1.39  (c1) 0.000, 0.51    (c2) 0.000, 3.11
                                       N = 16: (a) 0.000, 0.03  (b) 0.000, 2.18  (c1) 0.000, 0.37    (c2) 0.000, 4.52 F
                                       N = 32: (a) 0.000, 0.74  (b) 0.000, 2.09  (c1) 0.000, 1.33    (c2) 0.000, 6.19 F
                                       N = 64: (a) 0.000, 0.36  (b) 0.000, 1.53  (c1) 0.022, 1.20 F  (c2) 0.000, 9.50 F
    N = 8 separates (c1) on lamps and on staircase and (c2) on staircase.  On the corridor it separates neither: the floor is a strip of 45 pixels, and
    under a lamp the descent reaches that lamp with probability about 0.75, so that forgetting the division costs a quarter of the light.  There
    N = 64 is the smallest power of two at which both mutants fail.  (On lamps n = 8 the power-weighted mutant does not fail: the room's one large
    light dominates both weightings.)"""
    s, n = criterion_scene(name), CRITERION_SCENES[name]
    ref_a, ref_b = _moments(s, SEED_A, NL.ALL_LIGHTS, n), _moments(s, SEED_B, NL.ALL_LIGHTS, n)
    near = _moments(s, SEED_C, NL.NEAR, n)
    c1, c2 = _moments(s, SEED_C, NL.MUTANT_NO_WEIGHT, n), _moments(s, SEED_C, NL.MUTANT_POWER_WEIGHT, n)
    a, b = NL.criterion(*near, *ref_a), NL.criterion(*ref_a, *ref_b)
    m1, m2 = NL.criterion(*c1, *ref_a), NL.criterion(*c2, *ref_a)
    print(f"{name} N={n}: (a) near vs all-lights {a}, (b) all-lights vs all-lights {b}, (c1) inv_p = 1 {m1}, (c2) inv_p by power {m2}")
    assert a[2] >= (40 if name == "corridor" else 100)
    assert NL.passes(a[0], a[1]), f"(a) near against all-lights: {a}"
    assert NL.passes(b[0], b[1]), f"(b) all-lights against itself: {b}"
    _verdicts[name] = (NL.passes(m1[0], m1[1]), NL.passes(m2[0], m2[1]))
    if name == "corridor":
        assert not NL.passes(m1[0], m1[1]), f"(c1) the mutant without the division passes on the corridor: {m1}"
        assert not NL.passes(m2[0], m2[1]), f"(c2) the mutant weighted by power passes on the corridor: {m2}"


def test_each_mutant_fails_on_some_scene():
    for name in CRITERION_SCENES:
        if name not in _verdicts:
            test_criterion_accepts_the_estimator_and_the_reference(name)
    for k, what in enumerate(("inv_p forced to 1", "inv_p = cdf / w of TRT_FLAG_ONE_LIGHT")):
        assert not all(v[k] for v in _verdicts.values()), f"the mutant '{what}' passes the criterion on every scene: {_verdicts}"


# ---- it helps ----------------------------------------------------------------------------------------------------------------------------

def _variance(s, mode):
    lum = NL.render_seeds(s.flat, T.make_params(32, 8, 1, 0x5EED, flags=NL.FLAGS), 64, mode).astype(np.float64) @ NL.LUMA
    return float(lum.var(axis=0, ddof=1).sum())


def test_the_descent_lowers_the_variance_on_the_corridor():
    """corridor(16) at 32 x 8, 64 one-sample renders with fixed seeds: the per-pixel variance of the luminance, summed over the image, with NEAR against
    ONE_LIGHT from the same CPU build.  Measured: NEAR 256.94, ONE_LIGHT 282.72, all lights 255.54 — ratio NEAR / ONE_LIGHT 0.909.  Most of every figure
    is not the light selection's (a pixel is two units of floor wide and sees lit and unlit floor and, now and then, a lamp itself: all-lights has
    it too); what the selection adds on top of all-lights falls from 27.2 to 1.4, a ratio of 0.05.
    The same ratio NEAR / ONE_LIGHT where position says little, printed and not asserted: lamps n = 16: 2.18, staircase: 2.38 — there the descent by
    distance alone is worse than power alone at equal samples (the near lamp may face away or be hidden, and the large light is under-sampled)."""
    s = NC.corridor(16, 32, 8)
    near, one, every = _variance(s, NL.NEAR), _variance(s, NL.ONE_LIGHT), _variance(s, NL.ALL_LIGHTS)
    print(f"corridor(16): variance near {near:.2f}, one-light {one:.2f}, all lights {every:.2f}; near / one-light {near / one:.3f}; over all-lights {(near - every) / (one - every):.3f}")
    for name, kw in (("lamps", {"n": 16}), ("staircase", {})):
        o = get_scene(name, 32, 8, **kw)
        print(f"{name} {kw}: near / one-light {_variance(o, NL.NEAR) / _variance(o, NL.ONE_LIGHT):.3f}")
    assert near < one
    # under the centre of lamp k that lamp carries about 300 times its neighbour's contribution; power alone reaches it with probability 1 / 16, the
    # descent with 0.76 at the ends of the corridor and 0.51 in its middle (the top levels of the tree see only the centres of their halves)
    t = NL.tables_of(s.flat)
    nodes, root, _ = NL.tree(t)
    prob = NL.probabilities(nodes, root, t.n, np.array([[4.0 * k + 2.0, 0.0, 0.0] for k in range(16)], np.float32))
    print("probability of the lamp overhead, lamp 0 to 15:", np.round(np.diag(prob), 3))
    assert (prob.argmax(axis=1) == np.arange(16)).all() and (np.diag(prob) > 0.5).all()


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------

def test_flag_value_in_header_and_abi_mirror():
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    m = re.search(r"#define\s+TRT_FLAG_NEAR_LIGHTS\s+(\d+)u", text)
    assert m and int(m.group(1)) == 256 == _abi.TRT_FLAG_NEAR_LIGHTS == T.TRT_FLAG_NEAR_LIGHTS
    others = [int(x) for x in re.findall(r"#define\s+TRT_FLAG_(?!NEAR_LIGHTS)\w+\s+(\d+)u", text)]
    assert others and all(o & 256 == 0 for o in others)
    assert re.search(r"#define\s+TRT_ABI_VERSION\s+5\b", text)


def test_stand_alone_program_finishes_under_the_host_sanitizers(tmp_path):
    """tests/nearlights/nearlights_san.cpp with the CPU build compiled in, under AddressSanitizer and UBSan: corridor(3) at 16 x 9 x 2 spp in all five
    modes, the tree and the descent over the scene's tables before and after an update that moves the lamps, and over hostile tables."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "nearlights_san")
    libdir = os.path.join(ROOT, "tinyraytracing_amd", "lib")
    cmd = [cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
           "-ffp-contract=off", "-march=x86-64-v3", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyraytracing_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "nearlights", "nearlights_cpu.cpp"), os.path.join(ROOT, "tests", "nearlights", "nearlights_san.cpp"),
           "-L" + libdir, "-ltrt_host", "-Wl,-rpath," + libdir]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    scene_dir = tmp_path / "scene"
    scene_dir.mkdir()
    NC.write_case(str(scene_dir), "corridor3", 16, 9)
    # the inherited environment, unchanged but for the sanitizers' own options; the runtimes are linked statically into this stand-alone
    # program, and the link-order check is off so that it also starts where the environment preloads some other library
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe, str(scene_dir), "corridor3"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
