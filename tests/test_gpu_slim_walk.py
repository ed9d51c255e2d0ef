"""The slim kernels of the wave-uniform walk (trt_kernels.h WalkUniformFlags / WalkUniformHit8: 8-byte hit records, (u, v) formed in k_shade,
the triangles' flag words read from LDS) against the kernels TRT_SLIM_WALK=0 keeps — MI355X only.

Every render, pixel list and ray batch must come out bit-identical with the switch on and off, and equal to the CPU oracle.  Which
kernels ran is read from the TRT_DEBUG line of trt_create and asserted first.
"""
import re

import numpy as np
import pytest

import oracle_lib as O
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu


def renderer(s, slim, capfd, monkeypatch, env=None):
    env = dict(env or {}, TRT_DEBUG="1")
    if not slim:
        env["TRT_SLIM_WALK"] = "0"
    capfd.readouterr()
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        r = T.Renderer(s, 0)
    got = re.findall(r"trt_create: slim walk (\d), 8-byte hit records (\d)", capfd.readouterr().err)
    assert got == ([("1", "1")] if slim else [("0", "0")]), got
    return r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


STAT_FIELDS = ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "max_bounces", "redo_rays")


def stats_of(st, count):
    out = [getattr(st, f) for f in STAT_FIELDS]
    if count:
        out += list(st.inner_visits) + list(st.tri_tests)
    return out


def render_both(s, p, capfd, monkeypatch, env=None):
    out = []
    for slim in (True, False):
        r = renderer(s, slim, capfd, monkeypatch, env)
        try:
            out.append(r.render(p))
        finally:
            r.close()
    return out


LAMPS_MANY = 9  # the back box and 9 lamps: 59 triangles, 10 lights
CASES = [  # (scene, n added lamps, w, h, spp, flags, env)
    ("back", None, 128, 128, 16, 0, {}),
    ("back", None, 96, 64, 16, T.TRT_FLAG_FIXED_NEE, {}),
    ("back", None, 96, 64, 16, T.TRT_FLAG_OVERLAP, {}),
    ("back", None, 96, 64, 8, T.TRT_FLAG_COUNT, {}),
    ("back", None, 96, 64, 8, 0, {"TRT_TAIL_N": "40000"}),      # k_tail takes the paths over after the first bounces
    ("back", None, 96, 64, 8, T.TRT_FLAG_COUNT, {"TRT_TAIL_N": "0"}),
    ("lamps", 2, 64, 36, 8, 0, {}),                            # 3 lights: k_shade SHADE_FEW
    ("lamps", LAMPS_MANY, 64, 36, 8, T.TRT_FLAG_FIXED_NEE, {}),  # > 8 lights: SHADE_MANY
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}{c[1] or ''}-{c[2]}x{c[3]}x{c[4]}-f{c[5]}-{'-'.join(c[6].values()) or 'tail'}" for c in CASES])
def test_render_slim_equals_classic_and_oracle(case, capfd, monkeypatch):
    name, lamps, w, h, spp, flags, env = case
    s = get_scene(name, w, h, n=lamps) if lamps else get_scene(name, w, h)
    assert s.info["n_triangles"] <= 64
    p = T.make_params(w, h, spp, 0x51A + spp, flags=flags)
    (img_s, st_s), (img_c, st_c) = render_both(s, p, capfd, monkeypatch, env)
    assert np.array_equal(bits(img_s), bits(img_c)), "slim and classic kernels differ"
    count = bool(flags & T.TRT_FLAG_COUNT)
    assert stats_of(st_s, count) == stats_of(st_c, count)
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(bits(img_s), bits(ref)), f"max abs diff to the oracle {float(np.abs(img_s - ref).max())}"
    assert (st_s.rays_camera, st_s.rays_shadow, st_s.rays_indirect, st_s.shaded_hits, st_s.max_bounces) == \
        (ost.rays_camera, ost.rays_shadow, ost.rays_indirect, ost.shaded_hits, ost.max_bounces)


def test_pixel_list_slim_equals_classic(capfd, monkeypatch):
    s = get_scene("back", 64, 36)
    p = T.make_params(64, 36, 8, T.SEED_BACK)
    rng = np.random.default_rng(7)
    pixels = rng.integers(0, 64 * 36, 3000).astype(np.uint32)
    out = []
    for slim in (True, False):
        r = renderer(s, slim, capfd, monkeypatch)
        try:
            su, sq, st = r.render_pixels(p, pixels, 0, 8)
        finally:
            r.close()
        out.append((su, sq, stats_of(st, False)))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    assert out[0][2] == out[1][2]


@pytest.mark.parametrize("per_axis", [64, 300_000])
def test_ray_batch_with_zero_direction_components(per_axis, capfd, monkeypatch):
    """Axis-aligned rays are parked and walked again with the literal slab test (rewalk); with 300 000 per axis a wave meets more than the
    128 its list holds and goes over its share once more.  Both write the 8-byte records that k_hit_uv widens for the batch."""
    s = get_scene("back", 64, 36)
    org, dirs = SU.axis_rays(s, per_axis)
    t0, tri0, uv0 = O.trace(s.flat, org, dirs)
    got = []
    for slim in (True, False):
        r = renderer(s, slim, capfd, monkeypatch)
        try:
            got.append(r.trace_closest(org, dirs, want_stats=True))
        finally:
            r.close()
    (t1, tri1, uv1, st1), (t2, tri2, uv2, st2) = got
    assert st1.redo_rays == st2.redo_rays == 6 * per_axis
    for t, tri, uv in ((t1, tri1, uv1), (t2, tri2, uv2)):
        assert np.array_equal(tri, tri0) and np.array_equal(bits(t), bits(t0)) and np.array_equal(bits(uv), bits(uv0))
