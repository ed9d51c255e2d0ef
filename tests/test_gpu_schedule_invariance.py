"""What a traversal launch computes does not depend on how its rays are dealt out — MI355X only.

Which lane walks which ray, and when its record is stored, is decided by trt_handle::traceGrid, by the slice arithmetic and the refill
condition of the persistent kernels, and by their choice between a node step and a leaf step (trt_kernels.h).  The knobs trt_create reads
for them (tests/sched_cases.py) are "scheduling only"; this file holds them to it.  For every driver row of traversalOf(), every knob set
and every batch size at which a slice is empty, holds one ray, is exactly one refill batch or one more (sched_cases.edge_sizes):

  - every entry point of the ray queries returns the oracle's records bit for bit, each after a decoy batch of the same size
    (test_gpu_records_written.py has the technique), for a prefix of one ray pool and for a rotated window of it, so that the same ray
    lands on other lanes and slices;
  - the work done per ray is the same: the node visits and triangle tests of the batch equal those of a default-knob handle on the same
    batch and, on the persistent drivers, the sum of hostsim's per-ray counts.  A ray walked twice, dropped or restarted shows there even
    when its record is right;
  - small renders with the tail kernel off, which put every queue length from thousands down to one through k_trace_closest, k_trace_shadow
    and the shade queues, equal the oracle's image and ray counts, with the same traversal counters under every knob set.

Every assertion is exact equality.  Under the default grid a slice exceeds 64 rays only past 524 288 rays, so the batch in which every
wave's slice holds 65 is long there (532 480 rays; 2 129 920 under TRT_TRACE_RPW=64) and repeats the pool; the tests that run it take
0.5 to 2 s each on an MI355X, the others less."""
import numpy as np
import pytest

import aov_ref
import hostsim_lib as H
import oracle_lib as O
import raygen
import sched_cases as SC
import tinyraytracing_amd as T
from conftest import get_scene
from test_gpu_records_written import centroid_rays, check_device_entries, check_host_entries, decoy

pytestmark = pytest.mark.gpu

POOL = SC.LONG_N
ROTATE = 7777          # start of the rotated window: 7777 % 64 = 33, so every ray changes lane as well as slice
ENV_KEYS = ("TRT_SLIM_WALK", "TRT_BIN_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND", "TRT_TRACE_FILLB", "TRT_TRACE_MAXB", "TRT_TRACE_RPW", "TRT_REFILL_MIN",
            "TRT_SCHED_W", "TRT_LEAF_LOOP", "TRT_TAIL_N", "TRT_SLOTS", "TRT_SHADOW_STOP")


def renderer_with(s, env, monkeypatch):
    """A Renderer created under exactly `env` (read at trt_create)."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return T.Renderer(s, 0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


# ---------------------------------------------------------------------------------------------------------------- ray queries
# driver -> scene, the environment that puts it on that row of traversalOf(), the bytes of the nodes it walks, hostsim's node kind (None:
# the wave-uniform walk, which hostsim does not restate)
DRIVERS = {
    "wide4": ("staircase", {"TRT_NODE_KIND": "0"}, 128, 0),
    "wide4-spill": ("soup", {"TRT_NODE_KIND": "0"}, 128, 0),
    "oct8": ("veach-mis", {"TRT_NODE_KIND": "1"}, 80, 1),
    "per-lane-tiny": ("back", {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, 128, 0),
}
for _sw in SC.SWITCHES:  # the wave-uniform walk: every kernel combination is a driver of its own
    DRIVERS["uniform" + "".join(f"-{k[4:]}={v}" for k, v in _sw.items())] = ("back", dict(_sw), 64, None)

QUERY_CASES = [(d, e) for d in ("wide4", "wide4-spill", "per-lane-tiny") for e in SC.PERSISTENT_KNOBS]
QUERY_CASES += [("oct8", e) for e in SC.PERSISTENT_KNOBS] + [("oct8", {"TRT_LEAF_LOOP": "1"}), ("oct8", {"TRT_LEAF_LOOP": "24"})]
QUERY_CASES += [(d, g) for d in DRIVERS if d.startswith("uniform") for g in SC.UNIFORM_GRIDS]
QUERY_IDS = [f"{d}-{SC.knob_id(e)}" for d, e in QUERY_CASES]

_scenes, _pools, _decoys, _baselines = {}, {}, {}, {}


def scene_of(name):
    if name not in _scenes:
        if name == "soup":  # deep: 4-wide nodes with the stack spilled beyond LDS, as test_gpu_records_written.py's, with boxes that nest
            s = T.Scene.named("soup", 64, 36, n=60000)
            assert H.tree_hashes(s.flat, 1)[4] >> 32 > 16
        else:
            s = get_scene(name, 64, 36)
        _scenes[name] = s
    return _scenes[name]


class Pool:
    """POOL rays of one scene whose walks end at very different times, interleaved lane by lane: rays that miss the root box at once, rays
    aimed at a triangle's centroid from close by, long diagonals through the scene; every hundredth one has a zero direction component.
    With the oracle's records, and hostsim's per-ray work on both node kinds where the tree has them."""

    def __init__(self, name):
        s = scene_of(name)
        self.scene = s
        lo, hi = raygen.scene_bounds(s)
        ext = np.maximum(hi - lo, np.float32(1e-3))
        rng = np.random.default_rng(4242)
        k = np.arange(POOL)
        co, cd, _ = centroid_rays(s.flat, POOL, 909)
        ro, rd = raygen.random_rays(POOL, lo - 5, hi + 5, seed=77)
        away = rng.random((POOL, 3)) + 0.05
        mo = (hi + ext * (0.1 + rng.random((POOL, 3)))).astype(np.float32)           # beyond the far corner of the scene's box ...
        md = (away / np.linalg.norm(away, axis=1, keepdims=True)).astype(np.float32)  # ... and leaving
        o = np.where((k % 3 == 0)[:, None], mo, np.where((k % 3 == 1)[:, None], co[k % len(co)], ro))
        d = np.where((k % 3 == 0)[:, None], md, np.where((k % 3 == 1)[:, None], cd[k % len(cd)], rd))
        hostile = k % 100 == 50
        ao, ad = raygen.adversarial_rays(s, POOL, seed=31)
        o[hostile], d[hostile] = ao[hostile], ad[hostile]
        self.o, self.d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        # rays of raySpecial() (trt_path.h: a reciprocal direction component that is not finite): the hostile ones, and the rays aimed at an
        # axis-aligned triangle along its normal
        self.zero = (np.abs(self.d) < np.float32(1e-30)).any(1)
        assert self.zero[hostile].all() and hostile.sum() == POOL // 100
        self.ref = O.trace(s.flat, self.o, self.d)
        miss = self.ref[1][(k % 3 == 0) & ~hostile]
        assert (miss < 0).all() and (self.ref[1] >= 0).sum() > POOL // 4
        # the comparison of work runs on the pool without them: they may take the redo path, which is counted elsewhere
        self.plain = np.nonzero(~self.zero)[0]
        assert len(self.plain) > POOL // 2 and ((self.plain % 3 == 1).sum() > POOL // 100)
        self.counts = {}

    def window(self, n, start, plain=False):
        """Indices into the pool of a batch of n rays from `start` on, wrapping around (a batch longer than the pool repeats it)."""
        m = len(self.plain) if plain else POOL
        idx = (start + np.arange(n)) % m
        return self.plain[idx] if plain else idx

    def rays(self, idx):
        return self.o[idx], self.d[idx]

    def records(self, idx):
        return tuple(x[idx] for x in self.ref)

    def hostsim_counts(self, nk):
        """Per ray of the pool: (node visits, triangle tests) of hostsim's per-lane closest-hit walk on node kind nk."""
        if nk not in self.counts:
            v, t = H.trace_counts(self.scene.flat, nk, self.o[self.plain], self.d[self.plain])
            old = H.set_node_kind(nk)  # the same numbers as H.trace's totals, which test_trace_matches_oracle_on_incoherent_rays compares
            try:
                _, _, _, total = H.trace(self.scene.flat, self.o[self.plain], self.d[self.plain])
            finally:
                H.set_node_kind(old)
            assert [int(v.sum()), int(t.sum())] == total
            full = np.zeros((POOL, 2), np.int64)
            full[self.plain, 0], full[self.plain, 1] = v, t
            self.counts[nk] = full
        return self.counts[nk]


def pool_of(name):
    if name not in _pools:
        _pools[name] = Pool(name)
    return _pools[name]


def decoy_for(pool, name, start, seed):
    """A decoy for every batch that starts at `start`: POOL rays that hit, whose records differ from the pool's at every index of the
    window.  Batch i of a longer batch repeats the pool, and so may its decoy."""
    key = (name, start, seed)
    if key not in _decoys:
        _decoys[key] = decoy(pool.scene.flat, [pool.records(pool.window(POOL, start))], seed)
    return _decoys[key]


def cut(dec, n):
    idx = np.arange(n) % POOL
    do, dd, drec = dec
    return do[idx], dd[idx], tuple(x[idx] for x in drec)


def work_of(r, o, d):
    """The traversal counters of one closest-hit and one occlusion launch over the batch."""
    sc = r.trace_closest(o, d, want_stats=True)[3]
    so = r.trace_occluded(o, d, want_stats=True)[1]
    return sc, so


def baseline_work(driver, monkeypatch, pool, n, start):
    """(node visits, triangle tests) of the closest-hit and of the occlusion launch of a handle of this driver with no knob set, per batch."""
    if driver not in _baselines:
        _baselines[driver] = (renderer_with(pool.scene, DRIVERS[driver][1], monkeypatch), {})
    r, seen = _baselines[driver]
    if (n, start) not in seen:
        sc, so = work_of(r, *pool.rays(pool.window(n, start, plain=True)))
        seen[(n, start)] = (sc.inner_visits[0], sc.tri_tests[0], so.inner_visits[1], so.tri_tests[1])
    return seen[(n, start)]


def baseline_redo(driver, monkeypatch, pool, n, start):
    baseline_work(driver, monkeypatch, pool, 1, 0)
    r, seen = _baselines[driver]
    if ("redo", n, start) not in seen:
        seen[("redo", n, start)] = r.trace_closest(*pool.rays(pool.window(n, start)), want_stats=True)[3].redo_rays
    return seen[("redo", n, start)]


@pytest.fixture(scope="module", autouse=True)
def _close_baselines():
    yield
    for r, _ in _baselines.values():
        r.close()
    _baselines.clear()


@pytest.mark.parametrize("driver,knobs", QUERY_CASES, ids=QUERY_IDS)
def test_ray_queries_do_not_depend_on_the_schedule(driver, knobs, monkeypatch):
    name, base, node_bytes, nk = DRIVERS[driver]
    pool = pool_of(name)
    s = pool.scene
    small_grid = knobs.get("TRT_TRACE_MAXB") == "8"
    r = renderer_with(s, dict(base, **knobs), monkeypatch)
    try:
        assert r.trace_closest(pool.o[:64], pool.d[:64], want_stats=True)[3].inner_node_bytes == node_bytes
        for n, labels in SC.edge_sizes(knobs):
            for start in (0, ROTATE):
                tag = f"{driver} {SC.knob_id(knobs)} n={n} ({'/'.join(labels)}) from {start}"
                idx = pool.window(n, start)
                o, d = pool.rays(idx)
                ref = pool.records(idx)
                redo = check_host_entries(r, s, o, d, ref, tag, decoys=[cut(decoy_for(pool, name, start, seed), n) for seed in (101, 202)], unbounded=True)
                assert redo == baseline_redo(driver, monkeypatch, pool, n, start), f"{tag}: redo_rays"
                if small_grid:
                    check_device_entries(r, s, o, d, ref, tag, decoys=[cut(decoy_for(pool, name, start, seed), n) for seed in (303, 404)])
                # ---- work accounting, on the pool without the zero-component rays
                pidx = pool.window(n, start, plain=True)
                sc, so = work_of(r, *pool.rays(pidx))
                got = (sc.inner_visits[0], sc.tri_tests[0], so.inner_visits[1], so.tri_tests[1])
                assert got == baseline_work(driver, monkeypatch, pool, n, start), f"{tag}: (node visits, triangle tests) closest, occluded"
                if nk is not None:
                    per_ray = pool.hostsim_counts(nk)[pidx]
                    assert got[:2] == (int(per_ray[:, 0].sum()), int(per_ray[:, 1].sum())), f"{tag}: hostsim's per-ray steps"
                    for st, kind in ((sc, 0), (so, 1)):
                        assert st.wave_steps[0] > 0 and st.inner_visits[kind] <= 64 * st.wave_steps[0], f"{tag}: more node visits than 64 per wave step"
                        c = st.lane_census
                        assert c[0] + c[1] + c[2] <= 64 * c[3], f"{tag}: lane census"
                        assert (c[3] > 0) == (node_bytes == 80), f"{tag}: the census is the oct driver's"
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- renders
RENDERS = {"veach-mis": (48, 27, 4, 0x5EED0002, {}), "staircase": (48, 27, 4, T.SEED_STAIRCASE, {}), "back": (32, 32, 8, T.SEED_BACK, {"TRT_TRACE_IMPL": "3"})}
NO_TAIL = {"TRT_TAIL_N": "0"}
RENDER_KNOBS = [dict(NO_TAIL, **e) for e in SC.PERSISTENT_KNOBS] + [dict(NO_TAIL, TRT_SHADOW_STOP="0"), dict(NO_TAIL, TRT_SLOTS="1"), {}]
RENDER_CASES = [(n, e) for n in RENDERS for e in RENDER_KNOBS]
RENDER_IDS = [f"{n}-{SC.knob_id({k: v for k, v in e.items() if k != 'TRT_TAIL_N'})}{'' if e else '-tail'}" for n, e in RENDER_CASES]
MODES = (0, T.TRT_FLAG_FIXED_NEE)  # parity mode, and the any-hit shadow walk
_oracle_renders, _render_baselines = {}, {}


def oracle_render(name, mode):
    if (name, mode) not in _oracle_renders:
        w, h, spp, seed, _ = RENDERS[name]
        _oracle_renders[(name, mode)] = O.render(get_scene(name, w, h).flat, T.make_params(w, h, spp, seed, flags=mode))
    return _oracle_renders[(name, mode)]


def counters(st):
    return (st.inner_visits[0], st.tri_tests[0], st.inner_visits[1], st.tri_tests[1])


def render_baseline(name, mode, monkeypatch):
    """The traversal counters of a no-tail render on a handle with no knob set."""
    if (name, mode) not in _render_baselines:
        w, h, spp, seed, base = RENDERS[name]
        r = renderer_with(get_scene(name, w, h), dict(base, **NO_TAIL), monkeypatch)
        try:
            _, st = r.render(T.make_params(w, h, spp, seed, flags=mode | T.TRT_FLAG_COUNT))
        finally:
            r.close()
        _render_baselines[(name, mode)] = counters(st)
    return _render_baselines[(name, mode)]


@pytest.mark.parametrize("name,env", RENDER_CASES, ids=RENDER_IDS)
def test_renders_do_not_depend_on_the_schedule(name, env, monkeypatch):
    w, h, spp, seed, base = RENDERS[name]
    s = get_scene(name, w, h)
    tail = T.KERNEL_NAMES.index("tail")
    extra, budget, passes = 0, 0, 1
    if "TRT_SLOTS" in env:
        # one slot vetoes TRT_FLAG_OVERLAP, and the budget holds `chunk` samples of every pixel: 8 spp in three passes of 3, 3, 2; 4 spp cannot
        # be split into three equal-sized passes (2 + 2 or 1 + 1 + 1 + 1), so it takes four
        chunk = 3 if spp == 8 else 1
        extra, budget, passes = T.TRT_FLAG_OVERLAP, w * h * chunk * (132 + 48 * s.info["n_lights"]), (spp + chunk - 1) // chunk
        assert passes >= 3
    r = renderer_with(s, dict(base, **env), monkeypatch)
    try:
        for mode in MODES:
            ref, ost = oracle_render(name, mode)
            for count in (0, T.TRT_FLAG_COUNT):
                tag = f"{name} {env} flags {mode | count | extra}"
                img, st = r.render(T.make_params(w, h, spp, seed, flags=mode | count | extra, mem_budget=budget))
                bad = img.view(np.uint32) != ref.view(np.uint32)
                assert not bad.any(), f"{tag}: {int(bad.any(-1).sum())} pixels differ from the oracle's"
                assert (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits, st.max_bounces) == \
                    (ost.rays_camera, ost.rays_shadow, ost.rays_indirect, ost.shaded_hits, ost.max_bounces), tag
                assert st.passes == passes, tag
                assert st.inner_node_bytes != 64, f"{tag}: not on a persistent driver"
                if not env:
                    assert st.launches[tail] >= 1, f"{tag}: the default hand-over point leaves these passes' later bounces to k_tail"
                    continue  # k_tail walks its paths itself: its steps are not the queue kernels'
                assert st.launches[tail] == 0, tag
                if not count:
                    continue
                got, want = counters(st), render_baseline(name, mode, monkeypatch)
                if "TRT_SHADOW_STOP" in env and mode == 0 and st.inner_node_bytes == 80:
                    # not a scheduling knob for the work of parity-mode shadow rays on the oct driver: with all of space as every light's box no
                    # shadow ray ends early (LightBox), so each walks the same steps and then goes on.  What holds exactly: the same switch
                    # on a small grid with single-lane refills does the same work
                    assert got[:2] == want[:2] and got[2] >= want[2] and got[3] >= want[3], f"{tag}: {got} against {want}"
                    twin = renderer_with(s, dict(base, **env, TRT_TRACE_MAXB="8", TRT_REFILL_MIN="1"), monkeypatch)
                    try:
                        img2, st2 = twin.render(T.make_params(w, h, spp, seed, flags=mode | count))
                    finally:
                        twin.close()
                    assert np.array_equal(img2.view(np.uint32), ref.view(np.uint32)) and counters(st2) == got, f"{tag}: {counters(st2)} on the small grid against {got}"
                else:
                    assert got == want, f"{tag}: (node visits, triangle tests) of closest-hit and shadow rays"
                assert 0 < got[0] and 0 < got[2] and got[0] + got[2] <= 64 * st.wave_steps[0], f"{tag}: more node visits than 64 per wave step"
                c = st.lane_census
                assert c[0] + c[1] + c[2] <= 64 * c[3] and (c[3] > 0) == (st.inner_node_bytes == 80), f"{tag}: lane census"
    finally:
        r.close()


def test_pixel_lists_and_feature_buffers_on_a_small_grid_with_single_lane_refills(monkeypatch):
    """trt_render_pixels and trt_render_aov under TRT_TRACE_MAXB=8, TRT_REFILL_MIN=1 with the tail kernel off: 32 waves whatever the queue
    length, every finished lane refilled at once."""
    name = "staircase"
    w, h, spp, seed, base = RENDERS[name]
    s = get_scene(name, w, h)
    p = T.make_params(w, h, spp, seed)
    rng = np.random.default_rng(37)
    pixels = rng.integers(0, w * h, 30).astype(np.uint32)
    pixels = np.concatenate([pixels, pixels[:5], pixels[:2]])  # 37 entries; five pixels twice, two of them three times
    rng.shuffle(pixels)
    assert len(pixels) == 37 and len(np.unique(pixels)) < 37
    r = renderer_with(s, dict(base, **NO_TAIL, TRT_TRACE_MAXB="8", TRT_REFILL_MIN="1"), monkeypatch)
    try:
        _, acc, _ = r.render_samples(p, 0, spp)
        sums, sumsq, st = r.render_pixels(p, pixels, 0, spp)
        aov = r.render_aov(p)
    finally:
        r.close()
    assert st.launches[T.KERNEL_NAMES.index("tail")] == 0 and st.rays_camera == 37 * spp
    want = acc.reshape(-1, 3)[pixels]
    assert np.array_equal(sums.view(np.uint64), want.view(np.uint64)), "render_pixels' sums against render_samples' of the same pixels"
    assert (sumsq >= 0).all()
    img, _ = oracle_render(name, 0)
    assert np.array_equal(want.astype(np.float32).view(np.uint32), img.reshape(-1, 3)[pixels].view(np.uint32))
    ref = aov_ref.render_aov(s, p)
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(aov[k].view(np.uint32), ref[k].view(np.uint32)), f"render_aov: {k}"
