"""Camera rays that provably miss the scene are not formed, walked or resolved (trt_cull.h; k_shade's fused bounce 0 and k_resolve_tile) —
MI355X only.  Nothing may change: on a one-light scene (the Cornell box seen from 1200 away, a third of the frame) and on a scene with three
lights (veach-mis from 85 away, likewise), at 97 x 41 x 4 spp, the default handle, TRT_CULL_PRIMARY=0, TRT_FUSE_PRIMARY=0 and TRT_TAIL_N=64
return one image and one set of counters, the oracle's.  What the bound decided is read from the TRT_DEBUG line first and held to the CPU
build of the same function (tests/cull_ref.py).  Then: a tile whose left edge lies in the culled strip, interleaved stripes of rows, two
passes in flight, a counting render, sums left behind by an earlier render in the slots of culled paths, and a refitted handle."""
import re

import numpy as np
import pytest

import cull_ref as CR
import oracle_lib as O
import tinyraytracing_amd as T
from conftest import get_scene
from test_gpu_fused_primary import BYTES_PER_PATH, ORACLE_FIELDS, STAT_FIELDS, WithCamera, bits

pytestmark = pytest.mark.gpu

W, H, SPP = 97, 41, 4
CAMERAS = {
    "back": lambda: T.look_at((278, 273, -1200), (278, 273, 0), (0, 1, 0), 39.3077, W, H),
    "veach-mis": lambda: T.look_at((90, 20, 0), (5, 8, 0), (0, 1, 0), 30, W, H),
}
HANDLES = ({}, {"TRT_CULL_PRIMARY": "0"}, {"TRT_FUSE_PRIMARY": "0"}, {"TRT_TAIL_N": "64"})


def framed(name, scene=None):
    return WithCamera(scene or get_scene(name, W, H), CAMERAS[name]())


def root_boxes(s):
    n = s.flat.contents.nodes[0]
    return np.array(list(n.lo0) + list(n.hi0) + list(n.lo1) + list(n.hi1), np.float32)


def expected_line(s, p):
    b = CR.bound(s.flat.contents.camera, p.width, p.height, bool(p.flags & T.TRT_FLAG_FIXED_PIXELS), root_boxes(s))
    assert b["active"] and 0.5 < CR.culled_mask(b, p.width, p.height).mean() < 0.8, b
    return "columns [%d, %d] rows [%d, %d] band rows [%d, %d] band columns [%d, %d]" % (b["rect"] + b["rows"] + b["cols"])


def make(s, env, capfd, monkeypatch):
    capfd.readouterr()
    with monkeypatch.context() as m:
        m.setenv("TRT_DEBUG", "1")
        for k, v in env.items():
            m.setenv(k, v)
        r = T.Renderer(s, 0)
    got = re.findall(r"trt_create: cull primary (\d)", capfd.readouterr().err)
    assert got == [env.get("TRT_CULL_PRIMARY", "1")], got
    return r


def cull_lines(capfd):
    return re.findall(r"trt_render: cull primary (.*)", capfd.readouterr().err)


def stats_of(st, fields=STAT_FIELDS):
    return [getattr(st, f) for f in fields]


@pytest.mark.parametrize("name", ["back", "veach-mis"])
def test_handles_agree_with_each_other_and_the_oracle(name, capfd, monkeypatch):
    s = framed(name)
    p = T.make_params(W, H, SPP, 0xC011)
    line = expected_line(s, p)
    ref, ost = O.render(s.flat, p)
    assert (ref.reshape(-1, 3).max(axis=1) == 0).mean() > 0.5  # the framing: most of the frame sees nothing
    first = None
    for env in HANDLES:
        r = make(s, env, capfd, monkeypatch)
        try:
            img, st = r.render(p)
            assert cull_lines(capfd) == (["off: TRT_CULL_PRIMARY=0"] if "TRT_CULL_PRIMARY" in env else [line]), env
        finally:
            r.close()
        assert np.array_equal(bits(img), bits(ref)), (env, float(np.abs(img - ref).max()))
        assert stats_of(st, ORACLE_FIELDS) == stats_of(ost, ORACLE_FIELDS), env
        first = first or stats_of(st)
        assert stats_of(st) == first, env
    assert st.rays_camera == W * H * SPP


def test_tiles_stripes_overlap_count_and_stale_sums(capfd, monkeypatch):
    s = framed("back")
    line = expected_line(s, T.make_params(W, H, SPP, 1))
    j_lo = int(re.match(r"columns \[(\d+),", line).group(1))
    assert j_lo > 8
    r, r_off = make(s, {}, capfd, monkeypatch), make(s, {"TRT_CULL_PRIMARY": "0"}, capfd, monkeypatch)
    try:
        # a tile inside the box first: every slot of the pass memory it uses holds the sum of a path that hit something
        p_in = T.make_params(W, H, SPP, 0x57A1E, tile=(j_lo + 4, 8, j_lo + 28, 32))
        img, _ = r.render(p_in)
        assert np.array_equal(bits(img), bits(O.render(s.flat, p_in)[0])) and (img.reshape(-1, 3).max(axis=1) > 0).mean() > 0.5
        cases = {
            "whole frame, over the sums the tile left behind": T.make_params(W, H, SPP, 0x57A1E),
            "left edge in the culled strip": T.make_params(W, H, SPP, 0x71E, tile=(j_lo - 5, 3, W - 2, H - 1)),
            "stripes of 8 rows": T.make_params(W, H, SPP, 0x57, rows=(8, 2, 1)),
            "two passes in flight": T.make_params(W, H, SPP, 0x0E, flags=T.TRT_FLAG_OVERLAP, mem_budget=2 * W * H * BYTES_PER_PATH),
        }
        for what, p in cases.items():
            capfd.readouterr()
            img, st = r.render(p)
            assert cull_lines(capfd) == [line], what
            ref, ost = O.render(s.flat, p)
            assert np.array_equal(bits(img), bits(ref)), (what, float(np.abs(img - ref).max()))
            assert stats_of(st, ORACLE_FIELDS) == stats_of(ost, ORACLE_FIELDS), what
            img_off, st_off = r_off.render(p)
            assert np.array_equal(bits(img), bits(img_off)) and stats_of(st) == stats_of(st_off), what
        assert st.passes > 1
        # a counting render culls nothing: the root visit of every camera ray is counted, as without the switch and as the oracle counts it
        pc = T.make_params(W, H, SPP, 0xC0, flags=T.TRT_FLAG_COUNT)
        capfd.readouterr()
        img, st = r.render(pc)
        assert cull_lines(capfd) == ["off: counting render"]
        img_off, st_off = r_off.render(pc)
        ref, ost = O.render(s.flat, pc)
        assert np.array_equal(bits(img), bits(ref)) and np.array_equal(bits(img), bits(img_off))
        assert list(st.inner_visits) == list(st_off.inner_visits) == list(ost.inner_visits)
        assert list(st.tri_tests) == list(st_off.tri_tests) == list(ost.tri_tests)
        assert stats_of(st) == stats_of(st_off)
    finally:
        r.close()
        r_off.close()


def test_refitted_handle_culls_by_the_moved_boxes(capfd, monkeypatch):
    """trt_update_geometry reads the refitted root node back: after the box has moved 400 to the side the rectangle has moved with it, and
    the image is a fresh handle's and the oracle's."""
    scene = T.Scene.named("back", W, H)
    try:
        p = T.make_params(W, H, SPP, 0x2EF17)
        s = framed("back", scene)
        before = expected_line(s, p)
        r = make(s, {}, capfd, monkeypatch)
        try:
            img0, _ = r.render(p)
            assert cull_lines(capfd) == [before]
            v = scene.arrays()["tri_v"]
            v[..., 0] += np.float32(400.0)
            scene.set_vertices(v)
            moved = framed("back", scene)
            after = expected_line(moved, p)
            assert after != before
            r.update_geometry(scene)
            img1, st1 = r.render(p)
            assert cull_lines(capfd) == [after]
        finally:
            r.close()
        fresh = make(moved, {}, capfd, monkeypatch)
        try:
            img2, st2 = fresh.render(p)
        finally:
            fresh.close()
        ref, ost = O.render(moved.flat, p)
        assert np.array_equal(bits(img1), bits(img2)) and np.array_equal(bits(img1), bits(ref))
        assert stats_of(st1) == stats_of(st2) and stats_of(st1, ORACLE_FIELDS) == stats_of(ost, ORACLE_FIELDS)
        assert not np.array_equal(bits(img0), bits(img1))
    finally:
        scene.close()
