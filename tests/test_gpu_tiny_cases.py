"""The corpus of tests/tiny_cases.py through every route of the wave-uniform walk, the route asserted, bits equal to the CPU oracle — MI355X only.

The four walks (trt_kernels.h: uniformWalkImpl with flushPending, k_tail's uniformWalk, traceQueueBinned, fusedWalk in k_shade's FUSE flavour) each
restate the visit set, the candidate order, the leaf-floor rule and the tie fold; the other GPU files render them on the Cornell box, which has no two
triangles at one distance and never more than two candidates per lane.  Here every case is a scene on which one of those rules DECIDES the picture
(tests/test_tiny_cases_cpu.py asserts that on the oracle alone), rendered on one handle per route:

    default                          fused bounce 0, then k_tail
    TRT_TAIL_N=64                    fused bounce 0, then the binned queue walk and k_shade on 8-byte records for the later bounces
    TRT_FUSE_PRIMARY=0               the two-kernel bounce 0
    TRT_BIN_WALK=0 (TRT_TAIL_N=64)   the unbinned queue walk (a render reaches the queue kernels only with a short tail)
    TRT_SLIM_WALK=0                  the classic wave-uniform kernels; once more with TRT_TAIL_N=64 for their queue walk
    TRT_TRACE_IMPL=3                 the per-lane driver

Which route a handle takes is read from the TRT_DEBUG lines of trt_create and trt_render and from the launch counts of a TRT_FLAG_TIMING render, and
asserted before anything is compared.  Then two handles answer a ray batch (the case's pixel-centre rays and 4096 rays aimed at the tied triangles, a
third of them with a zero direction component): the queue kernels' rewalk of parked rays on ties, which no render reaches.
"""
import re

import numpy as np
import pytest

import oracle_lib as O
import tiny_cases as TC
import tinyraytracing_amd as T

pytestmark = pytest.mark.gpu

SEED = 0x71E5
ORACLE_FIELDS = ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "max_bounces")
K_CLOSEST, K_SHADE, K_TAIL = (T.KERNEL_NAMES.index(k) for k in ("trace_closest", "shade", "tail"))
DEFAULT_TAIL_N = 131072

# name -> (environment, what trt_create must report: slim walk, 8-byte records, binned walk, fused primary, tail_n; the per-lane driver?)
HANDLES = {
    "default": ({}, (1, 1, 1, 1, DEFAULT_TAIL_N), False),
    "queue": ({"TRT_TAIL_N": "64"}, (1, 1, 1, 1, 64), False),
    "two-kernel": ({"TRT_FUSE_PRIMARY": "0"}, (1, 1, 1, 0, DEFAULT_TAIL_N), False),
    "unbinned": ({"TRT_BIN_WALK": "0", "TRT_TAIL_N": "64"}, (1, 1, 0, 1, 64), False),
    "classic": ({"TRT_SLIM_WALK": "0"}, (0, 0, 0, 0, DEFAULT_TAIL_N), False),
    "classic-queue": ({"TRT_SLIM_WALK": "0", "TRT_TAIL_N": "64"}, (0, 0, 0, 0, 64), False),
    "per-lane": ({"TRT_TRACE_IMPL": "3"}, (0, 0, 0, 0, DEFAULT_TAIL_N), True),
}
ENV_KEYS = ("TRT_TAIL_N", "TRT_FUSE_PRIMARY", "TRT_BIN_WALK", "TRT_SLIM_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def handle(s, env, want, per_lane, capfd, monkeypatch):
    """A Renderer created under `env`; the route trt_create reports is asserted here"""
    capfd.readouterr()
    with monkeypatch.context() as m:
        for k in ENV_KEYS:
            m.delenv(k, raising=False)
        m.setenv("TRT_DEBUG", "1")
        for k, v in env.items():
            m.setenv(k, v)
        r = T.Renderer(s, 0)
    err = capfd.readouterr().err
    got = re.findall(r"trt_create: slim walk (\d), 8-byte hit records (\d), binned walk (\d)\ntrt_create: fused primary (\d)", err)
    tail = re.findall(r"trt_create: refill_min \d+ tail_n (\d+)", err)
    assert len(got) == 1 and len(tail) == 1, err
    assert tuple(int(x) for x in got[0]) + (int(tail[0]),) == want, (got, tail, want)
    # the 8-wide tree is built for the per-lane drivers only (trt_create: trace_impl != 0): its line tells the per-lane handle from the classic one
    assert ("trt_create: oct tree" in err) == per_lane, err
    return r


def render(r, p, fused, capfd):
    capfd.readouterr()
    img, st = r.render(p)
    got = [int(x) for x in re.findall(r"trt_render: fused primary (\d)", capfd.readouterr().err)]
    assert got == [1 if fused else 0], got
    return img, st


_oracle = {}


def oracle(case, s, flags):
    """The oracle's render of a case, computed once per flag word"""
    key = (case.name, flags & ~T.TRT_FLAG_TIMING)
    if key not in _oracle:
        _oracle[key] = O.render(s.flat, T.make_params(case.w, case.h, case.spp, SEED, flags=key[1]))
    return _oracle[key]


def check_render(case, s, r, flags, fused, capfd, what):
    p = T.make_params(case.w, case.h, case.spp, SEED, flags=flags)
    img, st = render(r, p, fused, capfd)
    ref, ost = oracle(case, s, flags)
    bad = int((bits(img) != bits(ref)).any(axis=2).sum())
    assert bad == 0, f"{what}, flags {flags}: {bad} pixels differ from the oracle, max abs diff {float(np.abs(img - ref).max())}"
    assert [getattr(st, f) for f in ORACLE_FIELDS] == [getattr(ost, f) for f in ORACLE_FIELDS], (what, flags)
    return st, ost


def check_batch(case, s, r, what):
    org, dirs = TC.centre_rays(s, case.w, case.h)
    a_org, a_dirs = TC.aimed_rays(s)
    assert len(a_org) == 4096 and int((a_dirs == 0).any(axis=1).sum()) >= 4096 // 3
    org, dirs = np.concatenate([org, a_org]), np.concatenate([dirs, a_dirs])
    key = (case.name, "batch")
    if key not in _oracle:
        _oracle[key] = O.trace(s.flat, org, dirs)
    t0, tri0, uv0 = _oracle[key]
    t, tri, uv = r.trace_closest(org, dirs)
    assert np.array_equal(tri, tri0), f"{what}: {int((tri != tri0).sum())} of {len(tri)} rays end on another triangle than the oracle's"
    assert np.array_equal(bits(t), bits(t0)) and np.array_equal(bits(uv), bits(uv0)), what
    return tri0


QUALIFY = [c for c in TC.CASES if c.qualifies]
BEYOND = [c for c in TC.CASES if not c.qualifies]


@pytest.mark.parametrize("case", QUALIFY, ids=[c.name for c in QUALIFY])
def test_every_route_renders_the_oracles_image(case, tmp_path, capfd, monkeypatch):
    s = case.make(tmp_path)
    redo = {}
    # paths that go on after bounce 0 (the oracle's indirect rays of a render cut at depth 2, same random numbers): the queue the tail threshold is compared with
    after_bounce_0 = O.render(s.flat, T.make_params(case.w, case.h, case.spp, SEED, max_depth=2))[1].rays_indirect
    assert after_bounce_0 > 64 or case.kind == "camera-away", after_bounce_0
    for name, (env, want, per_lane) in HANDLES.items():
        r = handle(s, env, want, per_lane, capfd, monkeypatch)
        try:
            fused, short_tail = bool(want[3]), want[4] == 64
            for flags in (0, T.TRT_FLAG_FIXED_NEE):
                st, ost = check_render(case, s, r, flags, fused, capfd, name)
                redo.setdefault(flags, {})[name] = st.redo_rays
            # the kernels that ran: one closest-hit launch per bounce, except for a fused bounce 0, which is booked under `shade`; k_tail ends a pass whose queue
            # is at most tail_n long, so with the default it follows bounce 0 at once and no queue kernel runs, and with tail_n = 64 the queue kernels do
            st, ost = check_render(case, s, r, T.TRT_FLAG_TIMING, fused, capfd, name)
            launches = list(st.launches)
            assert st.passes == 1 and launches[K_CLOSEST] == launches[K_SHADE] - (1 if fused else 0), (name, launches)
            if not short_tail:
                assert launches[K_SHADE] == 1 and launches[K_TAIL] == (1 if after_bounce_0 else 0), (name, launches)
            elif after_bounce_0 > 64:
                assert launches[K_SHADE] >= 2, (name, launches)
            # counters (a counting render keeps the two kernels on every handle)
            st, ost = check_render(case, s, r, T.TRT_FLAG_COUNT, False, capfd, name)
            if not per_lane:  # (the per-lane drivers cull by distance: a subset of the reference's visit set)
                assert list(st.inner_visits) == list(ost.inner_visits) and list(st.tri_tests) == list(ost.tri_tests), name
                redo.setdefault(T.TRT_FLAG_COUNT, {})[name] = st.redo_rays
            if name in ("default", "classic"):
                tri0 = check_batch(case, s, r, name)
                if case.kind != "camera-away":
                    assert int((tri0 >= 0).sum()) >= 1024  # the aimed rays do meet the triangles
        finally:
            r.close()
    for flags, by_handle in redo.items():
        uniform = {k: v for k, v in by_handle.items() if k != "per-lane"}
        assert len(set(uniform.values())) == 1, (flags, uniform)  # rays with a zero direction component: the same count on every wave-uniform route


@pytest.mark.parametrize("case", BEYOND, ids=[c.name for c in BEYOND])
def test_one_beyond_the_limits_leaves_the_route(case, tmp_path, capfd, monkeypatch):
    """33 nodes, 65 triangles: trt_create refuses the wave-uniform walk and everything built on it; the per-lane route gives the oracle's image"""
    s = case.make(tmp_path)
    r = handle(s, {}, (0, 0, 0, 0, DEFAULT_TAIL_N), True, capfd, monkeypatch)
    try:
        for flags in (0, T.TRT_FLAG_FIXED_NEE, T.TRT_FLAG_COUNT):
            check_render(case, s, r, flags, False, capfd, "default")
        check_batch(case, s, r, "default")
    finally:
        r.close()
