"""The WORK of an updated handle on the MI355X.  tests/test_gpu_refit.py compares every output of an updated handle with a fresh one's; a box that an update
left too large changes no output, only the number of nodes visited and triangles tested.  The counters of TRT_FLAG_COUNT and of the ray queries' stats
(inner_visits[0..1], tri_tests[0..1], redo_rays) are exact functions of the stored boxes, so here they are held, with exact equality, to

  (a) a handle that was never updated, after a round trip S0 -> S1 -> S0 (S1: an object at half its size; light 0 far out);
  (b) a handle that went S0 -> S2 directly, after S0 -> S1 -> S2 — once more with the second handle updated from device memory on a side stream;
  (c) hostsim's reference of "created on S0, then updated" (hostsim_lib.refit_trace_counts: the per-node functions of csrc/trt_refit.h in the loops of
      tests/refit/refit_loops.h, the per-lane walkers of trt_path.h / trt_oct.h), per-ray counts summed, records compared too — after the batch has shown
      that a FRESH handle of the moved scene does different work, so two equal collapses are not what is being compared;
  (d) the oracle's counters of a TRT_FLAG_COUNT render of the moved scene, on the wave-uniform walk of back (the caller's BVH2, inner_node_bytes == 64);
  (e) hostsim's continuation on the 4-wide nodes after boxes past 2^40 ended the 8-wide ones.

tests/test_refit_work_cpu.py shows on hostsim that each batch is moved by the driver fault it is here to catch (a level no launch covers, parents before
children, light boxes that only grow) and holds the reference to the oracle.  Scenes, moves and rays: tests/refit_work_cases.py.

Left out, and why.  wave_steps and lane_census count wave-level iterations: they depend on which rays share a wave (traceGrid, the slices, the refill
condition — tests/test_gpu_schedule_invariance.py only bounds them), and hostsim walks one ray at a time.  The plane filter (f): planeMaybe() is read by
k_trace_fix, which is compiled without counters, and by k_tail's per-lane walk, whose rays no caller aims; a stale filter (a superset) sends more rays to the
literal walk, which returns the same hits — no counter a test can steer moves, so the state is unobservable by design.  On back the premise of
(c) cannot hold for the shrink and smooth moves: its tree has four BVH2 nodes and one collapse (hostsim: equal work at every amplitude from 12 to 400), so
those rows assert that equality instead and the cube at three times its size ('grow'), where a fresh handle does differ, is added.  In (c) work is compared
on the rays without a zero direction component (the others go to k_trace_fix), records on all of them."""
import numpy as np
import pytest

import hostsim_lib as H
import oracle_lib as O
import refit_work_cases as RC
import tinyraytracing_amd as T

pytestmark = pytest.mark.gpu
ENV_KEYS = ("TRT_SLIM_WALK", "TRT_BIN_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND", "TRT_TAIL_N")
NO_TAIL = {"TRT_TAIL_N": "0"}  # every bounce through the queue kernels (k_tail walks its paths itself)

# row -> (scene, environment at trt_create, inner_node_bytes, hostsim's node kind or None for the wave-uniform walk of the BVH2)
ROWS = {
    "back-default": ("back", {}, 64, None),
    "back-slim0": ("back", {"TRT_SLIM_WALK": "0"}, 64, None),
    "back-bin0": ("back", {"TRT_BIN_WALK": "0"}, 64, None),
    "back-per-lane-4": ("back", dict(NO_TAIL, TRT_TRACE_IMPL="3", TRT_NODE_KIND="0"), 128, 0),
    "back-per-lane-8": ("back", dict(NO_TAIL, TRT_TRACE_IMPL="3", TRT_NODE_KIND="1"), 80, 1),
}
# the 4-wide walk with its stack in LDS is back-per-lane-4's (stack need 4); the large scenes need 26 / 46 / 28 entries, past the 16 of LDS: the spilled stack
for _name in RC.LARGE:
    ROWS[f"{_name}-wide4"] = (_name, dict(NO_TAIL, TRT_NODE_KIND="0"), 128, 0)
    ROWS[f"{_name}-oct8"] = (_name, dict(NO_TAIL, TRT_NODE_KIND="1"), 80, 1)
HOSTSIM_ROWS = [k for k, v in ROWS.items() if v[3] is not None]
UNIFORM_ROWS = [k for k, v in ROWS.items() if v[3] is None]
SAME_COLLAPSE = {("back", "shrink"), ("back", "smooth")}  # (c): a fresh handle of these does A's work (module docstring)


def renderer(scene, env, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return T.Renderer(scene, 0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def counters(st):
    return (st.inner_visits[0], st.inner_visits[1], st.tri_tests[0], st.tri_tests[1], st.redo_rays)


def all_work(r, name, node_bytes):
    """The counters of every entry point on the scene's batch: the four ray queries and a counting render in parity mode and with TRT_FLAG_FIXED_NEE."""
    o, d, _ = RC.rays(name)
    t_max = RC.bounds(name)
    out = {}
    st = r.trace_closest(o, d, want_stats=True)[3]
    assert st.inner_node_bytes == node_bytes
    out["closest"] = counters(st)
    out["closest-bounded"] = counters(r.trace_closest(o, d, want_stats=True, t_max=t_max)[3])
    out["occluded"] = counters(r.trace_occluded(o, d, want_stats=True)[1])
    out["occluded-bounded"] = counters(r.trace_occluded(o, d, t_max=t_max, want_stats=True)[1])
    for key, flags in (("render", 0), ("render-nee", T.TRT_FLAG_FIXED_NEE)):
        img, st = r.render(T.make_params(RC.W, RC.H, RC.SPP, RC.SEEDS[name], flags=flags | T.TRT_FLAG_COUNT))
        out[key] = counters(st) + (st.rays_camera, st.rays_shadow, st.rays_indirect)
        assert st.inner_visits[0] > 0 and st.inner_visits[1] > 0
        if node_bytes != 64:
            assert st.launches[T.KERNEL_NAMES.index("tail")] == 0
    assert out["closest"][0] > 0 and out["occluded"][1] > 0
    return out


def update(r, name, move):
    r.update_geometry(RC.scene(name, move))


@pytest.mark.parametrize("row", list(ROWS))
def test_a_round_trip_leaves_the_work_of_a_handle_that_was_never_updated(row, monkeypatch):
    name, env, node_bytes, _ = ROWS[row]
    never = renderer(RC.scene(name), env, monkeypatch)
    try:
        want = all_work(never, name, node_bytes)
    finally:
        never.close()
    for mid in ("shrink", "light"):
        A = renderer(RC.scene(name), env, monkeypatch)
        try:
            update(A, name, mid)
            away = counters(A.trace_closest(*RC.rays(name)[:2], want_stats=True)[3])
            update(A, name, "S0")
            got = all_work(A, name, node_bytes)
        finally:
            A.close()
        print(f"{row} S0 -> {mid} -> S0: closest at S0 {want['closest']}, at {mid} {away}; renders {want['render']} {want['render-nee']}")
        assert away != want["closest"], f"{row}: the {mid} move changes nothing the batch sees"
        assert got == want, f"{row}: after S0 -> {mid} -> S0 " + "; ".join(f"{k}: {got[k]} against {want[k]}" for k in got if got[k] != want[k])


@pytest.mark.parametrize("row", list(ROWS))
def test_the_path_to_a_vertex_set_does_not_change_the_work(row, monkeypatch):
    name, env, node_bytes, _ = ROWS[row]
    A, A2 = renderer(RC.scene(name), env, monkeypatch), renderer(RC.scene(name), env, monkeypatch)
    try:
        update(A, name, "shrink")
        update(A, name, "smooth")
        update(A2, name, "smooth")
        got, want = all_work(A, name, node_bytes), all_work(A2, name, node_bytes)
    finally:
        A.close()
        A2.close()
    assert got == want, f"{row}: S0 -> shrink -> smooth against S0 -> smooth " + "; ".join(f"{k}: {got[k]} against {want[k]}" for k in got if got[k] != want[k])


def test_the_device_entry_on_a_side_stream_leaves_the_same_work(monkeypatch):
    import torch
    name, env, node_bytes, _ = ROWS["staircase-oct8"]
    dev = torch.device("cuda", 0)
    A, A2 = renderer(RC.scene(name), env, monkeypatch), renderer(RC.scene(name), env, monkeypatch)
    try:
        update(A, name, "shrink")
        update(A, name, "smooth")
        moved = RC.scene(name, "smooth")
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            v = torch.from_numpy(moved.arrays()["tri_v"]).to(dev)
            vn = torch.from_numpy(moved.arrays()["tri_vn"]).to(dev)
        side.synchronize()
        A2.update_geometry_from(v, tri_vn=vn, lights_from=moved, stream_ptr=side.cuda_stream)
        got, want = all_work(A, name, node_bytes), all_work(A2, name, node_bytes)
    finally:
        A.close()
        A2.close()
    assert got == want, "; ".join(f"{k}: {got[k]} against {want[k]}" for k in got if got[k] != want[k])


C_CASES = [(row, move) for row in HOSTSIM_ROWS for move in ("shrink", "smooth") + (("grow",) if ROWS[row][0] == "back" else ())]


@pytest.mark.parametrize("row,move", C_CASES, ids=[f"{r}-{m}" for r, m in C_CASES])
def test_work_and_records_after_a_move_are_the_references(row, move, monkeypatch):
    name, env, node_bytes, nk = ROWS[row]
    o, d, plain = RC.rays(name)
    po, pd = o[plain], d[plain]
    moved = RC.scene(name, move)
    A, B = renderer(RC.scene(name), env, monkeypatch), renderer(moved, env, monkeypatch)
    try:
        update(A, name, move)
        sa, sb = A.trace_closest(po, pd, want_stats=True)[3], B.trace_closest(po, pd, want_stats=True)[3]
        assert sa.inner_node_bytes == sb.inner_node_bytes == node_bytes
        # before anything else: is this a batch on which a fresh handle does other work?
        print(f"{row} {move}: updated {counters(sa)}, fresh {counters(sb)}")
        if (name, move) in SAME_COLLAPSE:
            assert counters(sa) == counters(sb), f"{row} {move}: a fresh handle now differs — take the pair out of SAME_COLLAPSE"
        else:
            assert counters(sa) != counters(sb), f"{row} {move}: a fresh handle does the same work, so the comparison below would prove nothing about the update"
        so = A.trace_occluded(po, pd, want_stats=True)[1]
        rec = A.trace_closest(o, d)
        occ = A.trace_occluded(o, d)
    finally:
        A.close()
        B.close()
    v = [RC.vertices(name, move)]
    ref = H.refit_trace_counts(RC.scene(name).flat, v, moved.flat, nk, o, d)
    ref_any = H.refit_trace_counts(RC.scene(name).flat, v, moved.flat, nk, o, d, any=True)
    assert ref.kind == ref_any.kind == nk
    print(f"{row} {move}: closest {(sa.inner_visits[0], sa.tri_tests[0])} hostsim {ref.sums()}; occluded {(so.inner_visits[1], so.tri_tests[1])} hostsim {ref_any.sums()}")
    assert (sa.inner_visits[0], sa.tri_tests[0]) == ref.sums(), f"{row} {move}: closest-hit work against the sum of the reference's per-ray counts"
    assert (sa.inner_visits[1], sa.tri_tests[1]) == (0, 0)
    assert (so.inner_visits[1], so.tri_tests[1]) == ref_any.sums(), f"{row} {move}: any-hit work against the sum of the reference's per-ray counts"
    assert rec[1].tobytes() == ref.tri.tobytes() and rec[0].tobytes() == ref.t.tobytes() and rec[2].tobytes() == ref.uv.tobytes(), f"{row} {move}: records"
    assert np.array_equal(occ, ref_any.tri >= 0) and (ref.tri >= 0).sum() > 10000


@pytest.mark.parametrize("row", UNIFORM_ROWS)
def test_the_bvh2_route_does_the_oracles_work_on_the_moved_scene(row, monkeypatch):
    name, env, node_bytes, _ = ROWS[row]
    A = renderer(RC.scene(name), env, monkeypatch)
    try:
        for move in ("shrink", "grow", "S0"):
            update(A, name, move)
            for flags in (0, T.TRT_FLAG_FIXED_NEE):
                p = T.make_params(RC.W, RC.H, RC.SPP, RC.SEEDS[name], flags=flags | T.TRT_FLAG_COUNT)
                img, st = A.render(p)
                ref, ost = O.render(RC.scene(name, move).flat, p)
                assert st.inner_node_bytes == 64
                print(f"{row} {move} flags {flags}: {list(st.inner_visits)} {list(st.tri_tests)} oracle {list(ost.inner_visits)} {list(ost.tri_tests)}")
                assert list(st.inner_visits) == list(ost.inner_visits) and list(st.tri_tests) == list(ost.tri_tests), (row, move, flags)
                assert img.tobytes() == ref.tobytes() and st.inner_visits[0] > 0 and st.inner_visits[1] > 0
    finally:
        A.close()


def test_after_the_fallback_the_4_wide_nodes_do_the_references_work(monkeypatch):
    """test_gpu_refit.py's test_boxes_past_2_to_the_40, counters this time: the 4-wide nodes were refitted through every update without being walked."""
    name = "blob"
    o, d, plain = RC.rays(name)
    po, pd = o[plain], d[plain]
    s0 = RC.scene(name)
    v0, smooth = RC.vertices(name, "S0"), RC.vertices(name, "smooth")
    scaled = RC.load(name)
    scaled.set_vertices(v0 * np.float32(2.0 ** 33))
    A = renderer(s0, {"TRT_NODE_KIND": "1"}, monkeypatch)
    try:
        update(A, name, "smooth")
        st = A.trace_closest(po, pd, want_stats=True)[3]
        ref = H.refit_trace_counts(s0.flat, [smooth], RC.scene(name, "smooth").flat, 1, po, pd)
        assert st.inner_node_bytes == 80 and (st.inner_visits[0], st.tri_tests[0]) == ref.sums()
        A.update_geometry(scaled)
        A.update_geometry(s0)
        st = A.trace_closest(po, pd, want_stats=True)[3]
        so = A.trace_occluded(po, pd, want_stats=True)[1]
        rec = A.trace_closest(o, d)
    finally:
        A.close()
        scaled.close()
    seq = [smooth, v0 * np.float32(2.0 ** 33), v0]
    assert H.refit_trace_counts(s0.flat, seq, s0.flat, 1, o, d).rc == H.NO_LONGER_OCT
    ref = H.refit_trace_counts(s0.flat, seq, s0.flat, 1, o, d, go_on=True)
    ref_any = H.refit_trace_counts(s0.flat, seq, s0.flat, 1, o, d, any=True, go_on=True)
    assert ref.kind == 0 and st.inner_node_bytes == 128
    print(f"after the fallback: closest {(st.inner_visits[0], st.tri_tests[0])} hostsim {ref.sums()}; occluded {(so.inner_visits[1], so.tri_tests[1])} hostsim {ref_any.sums()}")
    assert (st.inner_visits[0], st.tri_tests[0]) == ref.sums()
    assert (so.inner_visits[1], so.tri_tests[1]) == ref_any.sums()
    assert rec[1].tobytes() == ref.tri.tobytes() and rec[0].tobytes() == ref.t.tobytes() and rec[2].tobytes() == ref.uv.tobytes()
