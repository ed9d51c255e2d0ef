"""Every ray of a batch gets its record written, on every traversal driver, for hostile rays on foreign trees.

The ray queries stage their records in a buffer of the handle that is reused from call to call and never cleared, so a ray the traversal
never stores would return the previous call's record for its index.  Before every batch under test a DECOY batch of the same size runs on
the same handle: rays aimed at triangles, each of which hits (the oracle says so), whose records differ from the expected answer of the
batch under test at every index.  A second, different decoy repeats the check.  An unwritten record then shows up as the decoy's.  The
device entries (trace_*_into) write into the very tensors the decoy filled.  Byte outputs are checked raw: 0 or 1, nothing else."""
import ctypes as C

import numpy as np
import pytest

import hostsim_lib as H
import oracle_lib as O
import query_ref as Q
import raygen
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene
from sched_cases import parked_per_wave

pytestmark = pytest.mark.gpu

_scenes = {}


def scene_of(name):
    if name not in _scenes:
        if name == "non-nesting":
            s = T.Scene.named("staircase", 64, 36)
            assert SU.shrink_some_boxes(s, 60) > 0
        elif name == "non-nesting-soup":  # deep: 4-wide nodes with the stack spilled beyond LDS
            s = T.Scene.named("soup", 64, 36, n=60000)
            assert SU.shrink_some_boxes(s, 3000, seed=7, amount=0.45) > 0
            # traversalOf() takes the spill row when the collapse's stack_need + 1 exceeds the 16 LDS levels (hostsim: the same collapse)
            assert H.tree_hashes(s.flat, 1)[4] >> 32 > 16
        elif name == "reversed":
            s = T.Scene.named("staircase", 64, 36)
            assert SU.renumber_nodes_reversed(s) > 0
        elif name == "lbvh":
            s = T.Scene.named("staircase", 64, 36, builder="lbvh")
        elif name == "reference-tree":
            s = SU.load_with_reference_tree("veach-mis", 64, 36)
        else:
            s = get_scene(name, 64, 36)
        _scenes[name] = s
    return _scenes[name]


def hostile_rays(s):
    """The families of tests/test_hostsim_hostile_rays.py, in one batch."""
    sets = [raygen.non_finite_rays(s, 3000), raygen.adversarial_rays(s, 3000), raygen.grazing_rays(s.flat, 1500), SU.axis_rays(s, 48),
            raygen.zero_direction_rays(s, 2400)]
    return np.concatenate([o for o, _ in sets]), np.concatenate([d for _, d in sets])


def centroid_rays(flat, n, seed):
    """n rays that each hit something, with the oracle's records: from 0.05 .. 2 units in front of a random triangle, aimed at its centroid."""
    f = flat.contents
    tv = np.ctypeslib.as_array(C.cast(f.tri_v, C.POINTER(C.c_float)), (f.n_tris * 9,)).reshape(f.n_tris, 3, 3).astype(np.float64)
    rng = np.random.default_rng(seed)
    m = max(2 * n, 4096)
    ti = rng.integers(0, f.n_tris, m)
    P = tv[ti].mean(1)
    N = np.cross(tv[ti, 1] - tv[ti, 0], tv[ti, 2] - tv[ti, 0])
    N /= np.linalg.norm(N, axis=1, keepdims=True) + 1e-300
    N *= rng.choice([-1.0, 1.0], (m, 1))
    o = (P + N * rng.uniform(0.05, 2.0, (m, 1))).astype(np.float32)
    d = (-N).astype(np.float32)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(d).sum(1) > 0)
    o, d = o[ok], d[ok]
    t, tri, uv = O.trace(flat, o, d)
    hit = tri >= 0
    assert hit.sum() >= 2, "no decoy ray hits"
    o, d, t, tri, uv = o[hit], d[hit], t[hit], tri[hit], uv[hit]
    return o, d, (t, tri, uv)


def records_equal(a, b):
    """per ray: the records (t, tri, uv) agree bit for bit"""
    return (a[1] == b[1]) & (a[0].view(np.uint32) == b[0].view(np.uint32)) & (a[2].view(np.uint32) == b[2].view(np.uint32)).all(1)


def decoy(flat, wants, seed):
    """A decoy batch for the expected records `wants` (one or more tuples of n records): rays that hit, whose records differ from each of
    them at every index."""
    wants = wants if isinstance(wants, list) else [wants]
    n = len(wants[0][0])
    o, d, rec = centroid_rays(flat, n, seed)
    pool = len(o)
    idx = np.arange(n) % pool
    for _ in range(4):  # move an index whose decoy record happens to be the expected one to the next decoy ray
        same = np.zeros(n, bool)
        for w in wants:
            same |= records_equal(tuple(x[idx] for x in rec), w)
        if not same.any():
            break
        idx[same] = (idx[same] + 1) % pool
    out = tuple(x[idx] for x in rec)
    for w in wants:
        assert not records_equal(out, w).any(), "the decoy cannot be told from the expected records"
    assert (out[1] >= 0).all()
    return o[idx], d[idx], out


def renderer_with(s, env, monkeypatch):
    for k in ("TRT_SLIM_WALK", "TRT_BIN_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND", "TRT_TRACE_FILLB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = T.Renderer(s, 0)
    for k in env:
        monkeypatch.delenv(k)
    return r


def bits_equal(got, want):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(got, want))


def check_host_entries(r, s, o, d, ref, tag, decoys=None, unbounded=False):
    """The host entries on the batch (o, d), each after a decoy batch.  decoys: two (o, d, records) batches of the same size to use instead of
    fresh ones; unbounded: trace_occluded without t_max is checked as well.  -> redo_rays of the batch."""
    n = len(o)
    tm = Q.bounds_for(ref[0])
    want_b = Q.closest(ref, tm)
    want_occ = Q.occluded(ref, tm)
    if decoys is None:
        decoys = [decoy(s.flat, [ref, want_b], 101), decoy(s.flat, [ref, want_b], 202)]
    redo = None
    for k, (do, dd, drec) in enumerate(decoys):
        assert not records_equal(drec, ref).any() and not records_equal(drec, want_b).any(), tag
        # the decoy's own records come back right: it really did fill the staging buffer
        assert bits_equal(r.trace_closest(do, dd), drec), f"{tag}: decoy {k}"
        t, tri, uv, st = r.trace_closest(o, d, want_stats=True)
        assert bits_equal((t, tri, uv), ref), f"{tag}: trace_closest after decoy {k}: {int((~records_equal((t, tri, uv), ref)).sum())} records differ"
        assert redo in (None, st.redo_rays), f"{tag}: redo_rays {redo}, then {st.redo_rays} on the same batch"
        redo = st.redo_rays
        assert bits_equal(r.trace_closest(do, dd, t_max=np.full(n, 1e30, np.float32)), drec), f"{tag}: decoy {k}"
        got = r.trace_closest(o, d, t_max=tm)
        assert bits_equal(got, want_b), f"{tag}: trace_closest(t_max=) after decoy {k}: {int((~records_equal(got, want_b)).sum())} records differ"
    # occlusion: decoy 0 leaves a 1 at every index (all its rays hit), decoy 1 a 0 (the same rays bounded below TRT_T_MIN); between them every
    # expected byte is contradicted at some point
    do, dd, _ = decoys[0]
    bounds = [(tm, want_occ)] + ([(None, Q.occluded(ref, None))] if unbounded else [])
    for k, (dm, want_dec) in enumerate(((None, np.ones(n, bool)), (np.zeros(n, np.float32), np.zeros(n, bool)))):
        for bound, want in bounds:
            got = r.trace_occluded(do, dd, t_max=dm)
            assert np.array_equal(got.view(np.uint8), want_dec.view(np.uint8)), f"{tag}: occlusion decoy {k}"
            got = r.trace_occluded(o, d, t_max=bound)
            raw = got.view(np.uint8)
            assert raw.max() <= 1, f"{tag}: occlusion bytes other than 0 / 1 after decoy {k}"
            assert np.array_equal(raw.astype(bool), want), \
                f"{tag}: {int((raw.astype(bool) != want).sum())} occlusions differ after decoy {k} (bounded: {bound is not None})"
    return redo


def check_device_entries(r, s, o, d, ref, tag, decoys=None):
    """The device entries, which write into the very tensors the decoy filled.  decoys: as for check_host_entries."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(o)
    tm = Q.bounds_for(ref[0])
    want_b = Q.closest(ref, tm)
    want_occ = Q.occluded(ref, tm)
    og, dg, tg = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (o, d, tm))
    t = torch.empty(n, dtype=torch.float32, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    if decoys is None:
        decoys = [decoy(s.flat, [ref, want_b], seed) for seed in (303, 404)]
    for k, (do, dd, drec) in enumerate(decoys):
        assert not records_equal(drec, ref).any(), tag
        dog, ddg = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (do, dd))
        for bound, want in ((None, ref), (tg, want_b)):
            r.trace_closest_into(dog, ddg, t, tri, uv)
            got = (t.cpu().numpy(), tri.cpu().numpy(), uv.cpu().numpy())
            assert bits_equal(got, drec), f"{tag}: device decoy {k}"
            r.trace_closest_into(og, dg, t, tri, uv, t_max=bound)
            got = (t.cpu().numpy(), tri.cpu().numpy(), uv.cpu().numpy())
            assert bits_equal(got, want), f"{tag}: trace_closest_into (bound {bound is not None}) after decoy {k}"
        for dm, want_dec in ((None, 1), (torch.zeros(n, dtype=torch.float32, device=dev), 0)):
            r.trace_occluded_into(dog, ddg, occ, t_max=dm)
            assert (occ.cpu().numpy() == want_dec).all(), f"{tag}: device occlusion decoy {k}"
            r.trace_occluded_into(og, dg, occ, t_max=tg)
            raw = occ.cpu().numpy()
            assert raw.max() <= 1 and np.array_equal(raw.astype(bool), want_occ), f"{tag}: trace_occluded_into after decoy {k}"


# scene -> the environments at trt_create that put it on each driver row of traversalOf() (trt_api.hip): the wave-uniform walk with and
# without the slim walk and the binned walk, 4-wide nodes (depth <= 16 on `back`, with the stack spilled beyond LDS on the deeper trees) and
# the 8-wide quantised nodes (a tree whose boxes do not nest is walked on the 4-wide ones whatever TRT_NODE_KIND says)
UNIFORM = [{}, {"TRT_SLIM_WALK": "0"}, {"TRT_BIN_WALK": "0"}, {"TRT_SLIM_WALK": "0", "TRT_BIN_WALK": "0"}]
PERSISTENT = [{"TRT_NODE_KIND": "0"}, {"TRT_NODE_KIND": "1"}]
CASES = ([("back", e) for e in UNIFORM] + [("back", {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"})]
         + [(n, e) for n in ("veach-mis", "staircase", "lbvh", "reference-tree") for e in PERSISTENT]
         + [(n, PERSISTENT[0]) for n in ("non-nesting", "non-nesting-soup", "reversed")])
IDS = [f"{n}-{'-'.join(f'{k}={v}' for k, v in e.items()) or 'default'}" for n, e in CASES]


@pytest.mark.parametrize("name,env", CASES, ids=IDS)
def test_every_record_is_written_after_a_decoy(name, env, monkeypatch):
    s = scene_of(name)
    o, d = hostile_rays(s)
    ref = O.trace(s.flat, o, d)
    r = renderer_with(s, env, monkeypatch)
    try:
        # the driver row: wave-uniform walk (64-B BVH2 nodes), 4-wide (128 B) or 8-wide quantised nodes (80 B; a tree whose boxes do not nest
        # gets no 8-wide collapse)
        bytes_want = 64 if "TRT_TRACE_IMPL" not in env and name == "back" else (80 if env.get("TRT_NODE_KIND") == "1" else 128)
        assert r.trace_closest(o[:64], d[:64], want_stats=True)[3].inner_node_bytes == bytes_want
        check_host_entries(r, s, o, d, ref, f"{name} {env}")
        check_device_entries(r, s, o, d, ref, f"{name} {env}")
    finally:
        r.close()


# (name, environment at trt_create, n): the default grid of 300 000 rays gives every wave one batch, i.e. at most 64 parked rays (the
# 128-entry list); TRT_TRACE_FILLB=8 shrinks the grid to 296 blocks, and every wave parks 192 or 256: more than the list holds, so it walks
# its share of the queue a second time
PARKING = [("binned-list", {}, 0), ("binned-overflow", {"TRT_TRACE_FILLB": "8"}, 8),
           ("uniform-list", {"TRT_BIN_WALK": "0"}, 0), ("uniform-overflow", {"TRT_BIN_WALK": "0", "TRT_TRACE_FILLB": "8"}, 8),
           ("uniform-no-slim-overflow", {"TRT_SLIM_WALK": "0", "TRT_TRACE_FILLB": "8"}, 8)]


@pytest.mark.parametrize("case,env,fillb", PARKING, ids=[c for c, _, _ in PARKING])
def test_zero_directions_park_and_come_back(case, env, fillb, monkeypatch):
    """300 000 rays with the zero vector as direction on the wave-uniform walk: every ray is parked, and walked again from the wave's list or,
    past 128 per wave, from a second pass over the wave's share of the queue.  Every ray's record is written and is the oracle's (a miss)."""
    s = scene_of("back")
    n = 300000
    per_wave = parked_per_wave(n, fillb or 2048)
    if case.endswith("overflow"):
        assert per_wave.min() > 128, per_wave.min()
    else:
        assert per_wave.max() <= 128, per_wave.max()
    o, d = raygen.zero_direction_rays(s, n, seed=17)
    ref = O.trace(s.flat, o, d)
    assert (ref[1] < 0).all()
    r = renderer_with(s, env, monkeypatch)
    try:
        tm = np.full(n, 1e30, np.float32)
        for k, seed in enumerate((505, 606)):
            do, dd, drec = decoy(s.flat, ref, seed)
            assert bits_equal(r.trace_closest(do, dd), drec), f"{case}: decoy {k}"
            t, tri, uv, st = r.trace_closest(o, d, want_stats=True)
            assert bits_equal((t, tri, uv), ref), f"{case}: {int((tri != ref[1]).sum())} records differ after decoy {k}"
            assert st.redo_rays == n, (case, st.redo_rays)
            assert bits_equal(r.trace_closest(do, dd, t_max=tm), drec), f"{case}: decoy {k}"
            assert bits_equal(r.trace_closest(o, d, t_max=tm), Q.closest(ref, tm)), f"{case}: bounded, after decoy {k}"
            assert np.array_equal(r.trace_occluded(do, dd).view(np.uint8), np.ones(n, np.uint8)), f"{case}: occlusion decoy {k}"
            raw = r.trace_occluded(o, d, t_max=tm).view(np.uint8)
            assert raw.max() <= 1 and not raw.any(), f"{case}: {int(raw.astype(bool).sum())} zero-direction rays occluded after decoy {k}"
    finally:
        r.close()
