"""The traversal work of an updated handle, without a GPU: hostsim_refit_trace_counts (tests/hostsim/hostsim.cpp) builds a HostScene on S0, refits it in
place through a list of vertex sets with the per-node functions of csrc/trt_refit.h (the loops: tests/refit/refit_loops.h) and returns the records and
the per-ray (node visits, triangle tests) of its ray queries.  This file holds that reference to what is already proven — an empty list gives
hostsim_trace_counts' numbers, a round trip gives them back, S0 -> S1 -> S2 equals S0 -> S2, the records are the oracle's on the moved scene, a tree
whose 8-wide nodes stop qualifying goes on as the 4-wide tree would — and then shows that every batch tests/test_gpu_refit_work.py uses is SENSITIVE:
altered copies of the loops (refitloops::Order, and light boxes that only grow) change its summed counters, so a driver with that fault could not pass there.

Sensitivity, summed (node visits, triangle tests) of the closest-hit walk over the plain rays of refit_work_cases.rays (56 192 of 56 480; printed by
test_every_batch_is_moved_by_the_altered_loops with -s; any-hit figures likewise):

                          (c) S0 -> shrink: update / skips deepest / shallowest first       (a) S0 -> shrink -> S0: update / shallowest first
    back      4-wide     57905 452903  /  63264 493948  /  63264 452903            63264 493403  /  57905 456043
    back      8-wide     58035 457610  /  63423 499040  /  63423 457610            63423 498490  /  58035 461885
    veach-mis 4-wide     72698  64730  /  72998  64733  /  79464  63093            78219  72133  /  78940  64287
    veach-mis 8-wide     60154  66527  /  60275  66530  /  64861  64978            64406  74211  /  63073  65357
    staircase 4-wide    123690  54152  / 126343  54137  / 208209  47664           191518  87340  / 243746  74405
    staircase 8-wide     90982  57426  /  91364  57426  / 135725  50890           131239  96541  / 245659  84720
    blob      4-wide    346758 108697  / 351655 108711  / 460022  89754           390154 134870  / 439258 100168
    blob      8-wide    214539 117090  / 228154 117307  / 293332  93298           264388 155103  / 301096 108905

A skipped deepest level cannot show in (a) or (b): its nodes keep the boxes of S0, which a round trip returns to and which both paths of (b) share.
It shows in (c), on every batch.  Parents refitted before their children show in (a), (b) and (c).  Light boxes that are never reset show on the
parity-mode shadow rays of the render after light 0 went far out and came back: staircase 8-wide (855216, 845347) after the update against
(888030, 869600) with the boxes united, blob 8-wide (157197, 201796) against (172024, 211948) (test_light_boxes_that_only_grow_cost_shadow_rays_work prints them)."""
import numpy as np
import pytest

import hostsim_lib as H
import oracle_lib as O
import query_ref as Q
import refit_work_cases as RC
import tinyraytracing_amd as T

SCENES = ("back", "veach-mis", "staircase", "blob")
CASES = [(name, nk) for name in SCENES for nk in (0, 1)]
IDS = [f"{name}-{'8-wide' if nk else '4-wide'}" for name, nk in CASES]
_work = {}


def work(name, moves, nk, any=False, bounded=False, alter=H.ALTER_NONE, go_on=False):
    """The handle created on S0 of `name` on node kind nk, updated through `moves`, asked the batch of refit_work_cases.rays (cached)."""
    key = (name, tuple(moves), nk, any, bounded, alter, go_on)
    if key not in _work:
        o, d, _ = RC.rays(name)
        after = RC.scene(name, moves[-1]).flat if moves else None
        bound = Q.bound(RC.bounds(name), len(o)) if bounded else None
        _work[key] = H.refit_trace_counts(RC.scene(name).flat, [RC.vertices(name, m) for m in moves], after, nk, o, d, any=any, bound=bound, alter=alter, go_on=go_on)
    return _work[key]


def same_work(a, b):
    return np.array_equal(a.visits, b.visits) and np.array_equal(a.tests, b.tests)


def same_records(a, b):
    return a.t.tobytes() == b.t.tobytes() and a.tri.tobytes() == b.tri.tobytes() and a.uv.tobytes() == b.uv.tobytes()


def plain_sums(name, w):
    plain = RC.rays(name)[2]
    assert not w.visits[~plain].any() and not w.tests[~plain].any()
    return w.sums()


@pytest.mark.parametrize("name,nk", CASES, ids=IDS)
def test_without_an_update_the_entry_gives_trace_counts_numbers_and_the_oracles_records(name, nk):
    o, d, plain = RC.rays(name)
    flat = RC.scene(name).flat
    assert H.compressible(flat)
    w = work(name, (), nk)
    assert w.rc == 0 and w.kind == nk
    v, t = H.trace_counts(flat, nk, o[plain], d[plain])
    assert np.array_equal(w.visits[plain], v) and np.array_equal(w.tests[plain], t)
    assert not w.visits[~plain].any() and not w.tests[~plain].any()
    t0, tri0, uv0 = O.trace(flat, o, d)[:3]
    assert np.array_equal(w.tri, tri0) and w.t.tobytes() == t0.tobytes() and w.uv.tobytes() == uv0.tobytes()
    assert (tri0 >= 0).sum() > 10000


@pytest.mark.parametrize("name,nk", CASES, ids=IDS)
def test_a_round_trip_gives_the_work_and_the_records_back(name, nk):
    for mid in ("shrink", "smooth", "light"):
        for any in (False, True):
            base, back = work(name, (), nk, any), work(name, (mid, "S0"), nk, any)
            assert back.kind == nk and same_work(base, back) and same_records(base, back), (mid, any)
    assert not same_work(work(name, (), nk), work(name, ("shrink",), nk)), "the shrink move changes nothing the rays see"


@pytest.mark.parametrize("name,nk", CASES, ids=IDS)
def test_the_path_to_a_vertex_set_does_not_matter(name, nk):
    for path, direct in ((("shrink", "smooth"), ("smooth",)), (("light", "shrink"), ("shrink",))):
        for any, bounded in ((False, False), (True, False), (False, True), (True, True)):
            a, b = work(name, path, nk, any, bounded), work(name, direct, nk, any, bounded)
            assert same_work(a, b) and same_records(a, b), (path, any, bounded)


@pytest.mark.parametrize("name,nk", CASES, ids=IDS)
def test_records_after_a_move_are_the_oracles_on_the_moved_scene(name, nk):
    o, d, _ = RC.rays(name)
    t_max = RC.bounds(name)
    for move in ("shrink", "smooth", "light") + (("grow",) if name == "back" else ()):
        ref = O.trace(RC.scene(name, move).flat, o, d)[:3]
        w = work(name, (move,), nk)
        assert w.kind == nk
        assert np.array_equal(w.tri, ref[1]) and w.t.tobytes() == ref[0].tobytes() and w.uv.tobytes() == ref[2].tobytes(), move
        assert np.array_equal(work(name, (move,), nk, any=True).tri >= 0, ref[1] >= 0), move
        if move == "shrink":
            want = Q.closest(ref, t_max)
            w = work(name, (move,), nk, bounded=True)
            assert np.array_equal(w.tri, want[1]) and w.t.tobytes() == want[0].tobytes() and w.uv.tobytes() == want[2].tobytes()
            assert np.array_equal(work(name, (move,), nk, any=True, bounded=True).tri >= 0, Q.occluded(ref, t_max))


@pytest.mark.parametrize("name,nk", CASES, ids=IDS)
def test_every_batch_is_moved_by_the_altered_loops(name, nk):
    """(a) the round trip, (b) path independence and (c) absolute work of tests/test_gpu_refit_work.py, each run on the altered copies of the loops: the
    check must tell the altered driver from the right one.  Exact inequality of the summed counters; the figures are printed."""
    SKIP, EARLY = H.ALTER_SKIP_DEEPEST, H.ALTER_SHALLOWEST_FIRST
    tag = f"{name} {'8-wide' if nk else '4-wide'}"
    for any in (False, True):
        walk = "any-hit" if any else "closest"
        base = plain_sums(name, work(name, (), nk, any))
        # (c): against the reference after one move, both faults, both moves
        for move in ("shrink", "smooth"):
            right = plain_sums(name, work(name, (move,), nk, any))
            skipped, early = (plain_sums(name, work(name, (move,), nk, any, alter=a)) for a in (SKIP, EARLY))
            print(f"{tag} {walk} (c) S0 -> {move}: update {right}, skips the deepest level {skipped}, shallowest first {early}")
            assert skipped != right and early != right, (tag, walk, move)
        # (a): back at S0 a parent still holds its children's boxes of S1
        early = plain_sums(name, work(name, ("shrink", "S0"), nk, any, alter=EARLY))
        print(f"{tag} {walk} (a) S0 -> shrink -> S0: update {base}, shallowest first {early}")
        assert early != base, (tag, walk)
        # (b): the two paths end on different trees
        via, direct = (plain_sums(name, work(name, p, nk, any, alter=EARLY)) for p in (("shrink", "smooth"), ("smooth",)))
        print(f"{tag} {walk} (b) shallowest first: S0 -> shrink -> smooth {via}, S0 -> smooth {direct}")
        assert via != direct, (tag, walk)


def shadow_batch(name):
    """The parity-mode shadow rays the render of test_gpu_refit_work.py draws for light 0 on S0."""
    p = T.make_params(RC.W, RC.H, RC.SPP, RC.SEEDS[name])
    o, d, light = H.shadow_rays(RC.scene(name).flat, p)
    keep = light == 0
    assert keep.sum() > 5000
    return o[keep], d[keep]


@pytest.mark.parametrize("name", ["staircase", "blob"])  # (veach-mis: its lights hang free above the plates — the same work with the box united, 272150 visits either way)
def test_light_boxes_that_only_grow_cost_shadow_rays_work(name):
    """The render of (a) with light 0 far out and back: on the 8-wide nodes a parity-mode shadow ray is ended by its light's box (LightBox, trt_oct.h), so a box
    that kept the far position lets every shadow ray walk on.  The same rays, walked as the render walks them."""
    o, d = shadow_batch(name)
    flat = RC.scene(name).flat
    vs = [RC.vertices(name, "light"), RC.vertices(name, "S0")]
    base = H.refit_trace_counts(flat, [], None, 1, o, d, light=0)
    back = H.refit_trace_counts(flat, vs, flat, 1, o, d, light=0)
    grown = H.refit_trace_counts(flat, vs, flat, 1, o, d, light=0, alter=H.ALTER_LIGHT_UNION)
    assert base.kind == back.kind == grown.kind == 1
    print(f"{name} 8-wide, {len(o)} shadow rays of light 0, S0 -> light far out -> S0: update {back.sums()}, light boxes kept and united {grown.sums()}")
    assert same_work(base, back) and same_records(base, back)
    assert grown.sums() != base.sums()
    # the closest-hit walk does not read the light boxes: the same fault leaves the ray batch's work alone, which is why (a) uses the render for it
    o, d, _ = RC.rays(name)
    assert same_work(work(name, (), 1), H.refit_trace_counts(flat, vs, flat, 1, o, d, alter=H.ALTER_LIGHT_UNION))


def test_a_tree_that_leaves_the_8_wide_nodes_goes_on_as_the_4_wide_tree():
    """test_gpu_refit.py's test_boxes_past_2_to_the_40 on the reference: a moderate update keeps the 8-wide nodes; boxes that reach 2^40 end them (the entry says so),
    and with go_on the scene walks the 4-wide nodes it refitted all along — back at the original size with the work and the records of a 4-wide handle of S0."""
    name = "blob"
    o, d, _ = RC.rays(name)
    flat = RC.scene(name).flat
    v0, smooth = RC.vertices(name, "S0"), RC.vertices(name, "smooth")
    assert work(name, ("smooth",), 1).kind == 1
    seq = [smooth, v0 * np.float32(2.0 ** 33), v0]
    assert H.refit_trace_counts(flat, seq, flat, 1, o, d).rc == H.NO_LONGER_OCT
    w = H.refit_trace_counts(flat, seq, flat, 1, o, d, go_on=True)
    assert w.rc == 0 and w.kind == 0
    want = work(name, (), 0)
    assert same_work(w, want) and same_records(w, want)
    assert not same_work(w, work(name, (), 1))
