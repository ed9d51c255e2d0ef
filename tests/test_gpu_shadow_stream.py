"""The shadow walks of bounce b on a side stream, beside closest hits and k_shade of bounce b + 1 (trt_api.hip renderCore)
— MI355X only.  No kernel differs, so nothing may change: every case is rendered on a default handle and on a TRT_SHADOW_STREAM=0
handle (one stream, the order of old), and images, ray counts and the integers of trt_stats are bit-equal between the two and equal to
the oracle's.  Which route a call took is read from its TRT_DEBUG line first.  The schedule the default handle enqueued (TRT_DEBUG_SCHEDULE=1:
one line per operation, with streams, events and the element ranges read and written) goes through tests/sched_graph.py: every two
operations that conflict are ordered, the additions into Lacc follow bounce and light order.  All handles run with TRT_TAIL_N=64, so a
pass is queue bounces nearly to its end."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import scene_util as SU
import sched_graph as G
import tiny_cases as TC
import tinyraytracing_amd as T
from conftest import get_scene
from test_gpu_fused_primary import ORACLE_FIELDS, bits

pytestmark = pytest.mark.gpu

ENV = {"TRT_DEBUG": "1", "TRT_DEBUG_SCHEDULE": "1", "TRT_TAIL_N": "64"}


def make(s, capfd, monkeypatch, env=None):
    e = dict(ENV, **(env or {}))
    capfd.readouterr()
    with monkeypatch.context() as m:
        for k, v in e.items():
            m.setenv(k, v)
        r = T.Renderer(s, 0)
    got = re.findall(r"trt_create: shadow stream (\d)", capfd.readouterr().err)
    assert got == [e.get("TRT_SHADOW_STREAM", "1")], got
    return r


def look(capfd, entry="trt_render"):
    """(route lines, operations) of the calls since the last look: a route is 'on' or 'off: <reason>'"""
    err = capfd.readouterr().err
    return re.findall(entry + r": shadow stream (on|off: .*)", err), G.parse(err)


def ints(st, fields=None):
    """every integer of trt_stats (the times are the only other fields), or the named ones"""
    if fields is not None:
        return [int(getattr(st, f)) for f in fields]
    out = []
    for name, _ in st._fields_:
        v = getattr(st, name)
        if isinstance(v, float) or name == "kernel_ms":
            continue
        out += [int(x) for x in v] if hasattr(v, "__len__") else [int(v)]
    return out


def pair(s, capfd, monkeypatch, env=None):
    return make(s, capfd, monkeypatch, env), make(s, capfd, monkeypatch, dict(env or {}, TRT_SHADOW_STREAM="0"))


def check_trace(ops, side):
    G.assert_ordered(ops)
    streams = {o.stream for o in ops if o.op == "shadow"}
    assert streams == ({"side"} if side else {"slot0"}) or not streams, streams
    if not side:
        assert not any(e.startswith("shad") for o in ops for e in o.waits + [o.record or ""])


def both(s, p, capfd, monkeypatch, want="on", env=None, oracle=True):
    """p on a default handle and on a one-stream handle -> (image, Stats, operations) of the first; everything compared"""
    r, r_off = pair(s, capfd, monkeypatch, env)
    try:
        img, st = r.render(p)
        routes, ops = look(capfd)
        assert routes == [want], routes
        check_trace(ops, want == "on")
        img_off, st_off = r_off.render(p)
        routes, ops_off = look(capfd)
        assert routes == ["off: TRT_SHADOW_STREAM=0"], routes
        check_trace(ops_off, False)
    finally:
        r.close()
        r_off.close()
    assert np.array_equal(bits(img), bits(img_off)) and ints(st) == ints(st_off)
    assert [(o.op, o.pass_, o.bounce, o.light) for o in ops] == [(o.op, o.pass_, o.bounce, o.light) for o in ops_off]  # the same launches
    if oracle:
        ref, ost = O.render(s.flat, p)
        assert np.array_equal(bits(img), bits(ref)), float(np.abs(img - ref).max())
        assert ints(st, ORACLE_FIELDS) == [int(getattr(ost, f)) for f in ORACLE_FIELDS]
    return img, st, ops


def shade_waits(ops, ps=0):
    """per queue bounce b >= 1 of pass ps: does k_shade wait for the shadow walk of bounce b - 1?"""
    return [("shadow%d" % ((o.bounce - 1) & 1)) in o.waits for o in G.find(ops, "shade", ps) if o.bounce >= 1]


# ---- tiny scenes of this file: a room, a floor under lamps
def room_tris(open_front=False):
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, 0.0, 3.0, -2.0, 7.0
    q = lambda m, a, b, c, d, n: [(m, (a, b, c), n), (m, (a, c, d), n)]
    t = q("white", (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), (0, 1, 0))       # floor
    t += q("white", (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1), (0, -1, 0))    # ceiling
    t += q("red", (x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1), (1, 0, 0))
    t += q("green", (x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), (-1, 0, 0))
    t += q("white", (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (0, 0, 1))     # back
    if not open_front:
        t += q("blue", (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (0, 0, -1))  # behind the camera
    t += q("lamp", (-1.0, 2.9, 0.5), (1.0, 2.9, 0.5), (1.0, 2.9, 2.5), (-1.0, 2.9, 2.5), (0, -1, 0))
    return t


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("shadow_stream")


@pytest.fixture(scope="module")
def closed_room(tmp):
    s = TC.build(tmp, "room", room_tris(), 2, w=40, h=30, fovy=60.0, eye=(0, 1.5, 6), lookat=(0, 1.4, 0))
    yield s
    s.close()


def lamps_scene(tmp, name, mats, lights, mtl):
    tris = list(TC.FLOOR)
    for k, m in enumerate(mats):
        x = -2.0 + 2.0 * k
        tris += [(m, ((x - 0.5, 3.0, 0.5), (x + 0.5, 3.0, 0.5), (x + 0.5, 3.0, 1.5)), (0, -1, 0))]
    tris += [("pane", ((-1.0, 0.1, 2.0), (1.0, 0.1, 2.0), (0.0, 1.8, 2.0)), (0, 0, 1))]
    d = os.path.join(str(tmp), name)
    os.makedirs(d, exist_ok=True)
    SU.write_scene(d, name, TC.obj_text(tris), mtl, lights=lights, w=36, h=24, fovy=40.0, eye=TC.EYE, lookat=TC.LOOKAT)
    return SU.load(d, name, leaf_num=2)


MTL_LAMPS = "".join(f"newmtl {n}\nKd {kd}\nKs 0 0 0\nNs 1\nNi 1\n" for n, kd in (("white", "0.7 0.7 0.7"), ("lamp0", "0 0 0"), ("lamp1", "0 0 0"), ("lamp2", "0 0 0")))
PANE_PLAIN = "newmtl pane\nKd 0.2 0.5 0.8\nKs 0 0 0\nNs 1\nNi 1\n"
PANE_GLASS = "newmtl pane\nKd 0.5 0.5 0.5\nKs 0 0 0\nTr 0.8 1 0.95\nNs 1\nNi 1.5\n"


@pytest.fixture(scope="module")
def three_lights(tmp):
    s = lamps_scene(tmp, "three", ("lamp0", "lamp1", "lamp2"), [("lamp0", (20, 16, 12)), ("lamp1", (4, 16, 20)), ("lamp2", (12, 20, 6))], MTL_LAMPS + PANE_PLAIN)
    yield s
    s.close()


@pytest.fixture(scope="module")
def glass(tmp):
    s = lamps_scene(tmp, "glass", ("lamp0",), [("lamp0", (20, 16, 12))], MTL_LAMPS + PANE_GLASS)
    yield s
    s.close()


# ---- the cases
def test_back_uses_both_ends_from_bounce_0(capfd, monkeypatch):
    w, h, spp = 96, 54, 8
    img, st, ops = both(get_scene("back", w, h), T.make_params(w, h, spp, 0x5AD0), capfd, monkeypatch)
    waits = shade_waits(ops)
    assert len(waits) >= 8 and not any(waits), waits                          # free from bounce 0: 40 % of the frame sees nothing
    N = w * h * spp
    at = [[iv for iv in o.writes if iv[0] == "shadow0"][0] for o in G.find(ops, "shade", 0)]
    assert at[0][1] == 0 and at[1][2] == N and at[1][1] > 0 and at[2][1] == 0  # even bounces upward from 0, odd ones up to N
    assert all(iv[2] <= N for iv in at)
    assert len(G.find(ops, "shadow")) >= 8 and len(G.find(ops, "tail")) == 1 and st.rays_shadow > 0


def test_closed_room_waits_first_and_runs_free_later(closed_room, capfd, monkeypatch):
    p = T.make_params(40, 30, 8, 0xC105ED)
    img, st, ops = both(closed_room, p, capfd, monkeypatch)
    sh0, shade1 = G.find(ops, "shadow", 0, 0)[0], G.find(ops, "shade", 0, 1)[0]
    n_s0 = [iv for iv in sh0.reads if iv[0] == "shadow0"][0][2]
    n_active1 = [iv for iv in shade1.reads if iv[0] == "hit"][0][2]
    assert n_s0 + n_active1 > 40 * 30 * 8                                      # every camera ray hits a wall: the two ends meet
    waits = shade_waits(ops)
    first_free = waits.index(False)
    assert first_free >= 1 and all(waits[:first_free]) and not any(waits[first_free:]) and len(waits) - first_free >= 4, waits


def test_glass_is_serial(glass, capfd, monkeypatch):
    assert glass.info["n_lights"] == 1
    img, st, ops = both(glass, T.make_params(36, 24, 8, 0x61A55), capfd, monkeypatch, want="off: a material with Ni > 1 (k_shade adds to Lacc)")
    assert st.rays_shadow > 0 and st.rays_indirect > 0


def test_three_lights_take_the_side_stream(three_lights, capfd, monkeypatch):
    assert three_lights.info["n_lights"] == 3
    img, st, ops = both(three_lights, T.make_params(36, 24, 8, 0x3117), capfd, monkeypatch)
    assert {o.light for o in G.find(ops, "shadow")} == {0, 1, 2}


def test_veach_mis_walks_per_lane_and_is_serial(capfd, monkeypatch):
    w, h = 64, 36
    both(get_scene("veach-mis", w, h), T.make_params(w, h, 4, 0x7EAC), capfd, monkeypatch, want="off: per-lane walk (shared redo list and spill area)")


def test_three_passes_by_mem_budget(capfd, monkeypatch):
    w, h, spp = 48, 30, 6
    p = T.make_params(w, h, spp, 0x3A55, mem_budget=2 * w * h * (132 + 48))
    img, st, ops = both(get_scene("back", w, h), p, capfd, monkeypatch)
    assert st.passes == 3
    reach = G.before(ops)
    for ps in (1, 2):  # the pass's first operations lie behind every shadow walk of the pass before
        first = [o for o in ops if o.pass_ == ps and o.stream == "slot0"][0]
        walks = G.find(ops, "shadow", ps - 1)
        assert walks and all((reach[first.index] >> o.index) & 1 for o in walks)
    resolves = G.find(ops, "resolve")
    assert len(resolves) == 3 and all(any(e.startswith("shadow") for e in o.waits) or G.find(ops, "tail", o.pass_) for o in resolves)


@pytest.mark.parametrize("flag,why", [("TRT_FLAG_OVERLAP", "two passes in flight"), ("TRT_FLAG_TIMING", "TRT_FLAG_TIMING"), ("TRT_FLAG_COUNT", "counting render")])
def test_flags_that_keep_one_stream(flag, why, capfd, monkeypatch):
    w, h, spp = 48, 30, 4
    budget = 2 * 2 * w * h * (132 + 48) if flag == "TRT_FLAG_OVERLAP" else 0
    s = get_scene("back", w, h)
    p = T.make_params(w, h, spp, 0xF1A6, flags=getattr(T, flag), mem_budget=budget)
    r, r_off = pair(s, capfd, monkeypatch)
    try:
        img, st = r.render(p)
        routes, ops = look(capfd)
        assert routes == ["off: " + why]
        assert {o.stream for o in G.find(ops, "shadow")} <= {"slot0", "slot1"}
        if flag != "TRT_FLAG_OVERLAP":
            G.assert_ordered(ops)
        img_off, st_off = r_off.render(p)
    finally:
        r.close()
        r_off.close()
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(bits(img), bits(img_off)) and np.array_equal(bits(img), bits(ref))
    assert ints(st) == ints(st_off) and ints(st, ORACLE_FIELDS) == [int(getattr(ost, f)) for f in ORACLE_FIELDS]
    if flag == "TRT_FLAG_COUNT":
        assert list(st.inner_visits) == list(st_off.inner_visits) == list(ost.inner_visits) and list(st.tri_tests) == list(st_off.tri_tests) == list(ost.tri_tests)
    if flag == "TRT_FLAG_OVERLAP":
        assert st.passes >= 2


def test_samples_pixel_list_and_rays(capfd, monkeypatch):
    """render_samples onto a caller's sums (two calls), a pixel list and caller-supplied rays: all on the side stream, all the oracle's image"""
    w, h, spp = 48, 30, 4
    s = get_scene("back", w, h)
    p = T.make_params(w, h, spp, 0x11575)
    ref, _ = O.render(s.flat, p)
    pix = np.arange(w * h, dtype=np.uint32)
    org, dirs = T.camera_rays(s.flat.contents.camera, p, pix, 0, spp)
    got = []
    for r in pair(s, capfd, monkeypatch):
        try:
            side = len(got) == 0
            want = ["on"] if side else ["off: TRT_SHADOW_STREAM=0"]
            _, acc, st_a = r.render_samples(p, 0, 1)
            routes, ops = look(capfd)
            assert routes == want
            check_trace(ops, side)
            img, acc, st_b = r.render_samples(p, 1, spp, accum=acc)
            routes, ops = look(capfd)
            assert routes == want
            check_trace(ops, side)
            sums, sumsq, st_p = r.render_pixels(p, pix[::-1].copy(), 0, spp)
            routes, ops = look(capfd, "trt_render_pixels")
            assert routes == want
            check_trace(ops, side)
            rsums, _, st_r = r.render_rays(p, org, dirs)
            routes, ops = look(capfd, "trt_render_rays")
            assert routes == want
            check_trace(ops, side)
            got.append((img, acc, sums, sumsq, rsums, ints(st_a) + ints(st_b) + ints(st_p) + ints(st_r)))
        finally:
            r.close()
    a, b = got
    for x, y in zip(a, b):
        assert (np.array_equal(bits(x), bits(y)) if isinstance(x, np.ndarray) else x == y)
    assert np.array_equal(bits(a[0]), bits(ref))
    assert np.array_equal(bits(a[2][::-1].astype(np.float32).reshape(h, w, 3)), bits(ref))
    assert np.array_equal(bits(a[4].astype(np.float32).reshape(h, w, 3)), bits(ref))


def test_render_into_on_a_stream_of_the_callers(capfd, monkeypatch):
    import torch
    w, h, spp = 48, 30, 4
    s = get_scene("back", w, h)
    p = T.make_params(w, h, spp, 0x57EA)
    ref, ost = O.render(s.flat, p)
    out = []
    for r in pair(s, capfd, monkeypatch):
        try:
            stream = torch.cuda.Stream()
            t = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            st = r.render_into(p, t, stream.cuda_stream)
            routes, ops = look(capfd)
            assert routes == (["on"] if not out else ["off: TRT_SHADOW_STREAM=0"])
            check_trace(ops, not out)
            out.append((t.cpu().numpy(), ints(st)))
        finally:
            r.close()
    assert np.array_equal(bits(out[0][0]), bits(ref)) and np.array_equal(bits(out[0][0]), bits(out[1][0])) and out[0][1] == out[1][1]


def test_injected_failure_drains_the_side_stream(capfd, monkeypatch):
    """TRT_TEST_FAIL_AT_BOUNCE=2: the call fails with bounce 2's kernels and the shadow walks of bounce 1 in flight; the next render on the
    handle writes the same arena from its first kernel on, and is the oracle's"""
    w, h, spp = 96, 54, 8
    s = get_scene("back", w, h)
    p = T.make_params(w, h, spp, 0xFA11)
    r = make(s, capfd, monkeypatch, {"TRT_TEST_FAIL_AT_BOUNCE": "2"})
    try:
        with pytest.raises(T.TrtError, match="injected failure"):
            r.render(p)
        routes, ops = look(capfd)
        assert routes == ["on"] and G.find(ops, "shadow", 0, 1) and not G.find(ops, "shadow", 0, 2)
        img, st = r.render(p)
        routes, ops = look(capfd)
        assert routes == ["on"]
        check_trace(ops, True)
    finally:
        r.close()
    ref, ost = O.render(s.flat, p)
    assert np.array_equal(bits(img), bits(ref))
    assert ints(st, ORACLE_FIELDS) == [int(getattr(ost, f)) for f in ORACLE_FIELDS]
