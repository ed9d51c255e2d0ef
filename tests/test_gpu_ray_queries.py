"""The ray queries of include/trt.h on the MI355X: trt_trace_closest_range / trt_trace_occluded and their _device twins against query_ref.py
(the oracle's closest hit, clipped to each ray's bound), on every traversal driver a scene can be given, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import query_ref as Q
import raygen
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu
K_CLOSEST, K_SHADOW = 1, 3

# scene -> the environments at trt_create that put it on each driver row of traversalOf() (trt_api.hip): the wave-uniform walk with and without
# the slim walk / 8-byte hits, 4-wide nodes (depth <= 16, or with spill on the deep soup) and the 8-wide quantised nodes
UNIFORM = [{}, {"TRT_SLIM_WALK": "0"}, {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}]
PERSISTENT = [{"TRT_NODE_KIND": "0"}, {"TRT_NODE_KIND": "1"}]

_scenes = {}


def scene_of(name):
    if name not in _scenes:
        if name == "soup":
            _scenes[name] = get_scene("soup", 64, 36, n=200000)
        elif name == "lbvh":
            _scenes[name] = T.Scene.named("staircase", 64, 36, builder="lbvh")
        elif name == "reference-tree":
            _scenes[name] = SU.load_with_reference_tree("veach-mis", 64, 36)
        elif name == "non-nesting":
            s = T.Scene.named("staircase", 64, 36)
            SU.shrink_some_boxes(s, 60)
            _scenes[name] = s
        else:
            _scenes[name] = get_scene(name, 64, 36)
    return _scenes[name]


def ray_sets(s):
    lo, hi = raygen.scene_bounds(s)
    return {"random": raygen.random_rays(6000, lo, hi, seed=21),
            "primary": raygen.primary_rays(s, 64, 36),
            "adversarial": raygen.adversarial_rays(s, 3000),
            "non_finite": raygen.non_finite_rays(s, 2000),
            "grazing": raygen.grazing_rays(s.flat, 2000),
            "axis": SU.axis_rays(s, 48)}


_refs = {}


def reference(name, s):
    if name not in _refs:
        sets = ray_sets(s)
        _refs[name] = {k: (o, d, O.trace(s.flat, o, d)) for k, (o, d) in sets.items()}
    return _refs[name]


def renderer_with(s, env, monkeypatch):
    for k in ("TRT_SLIM_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = T.Renderer(s, 0)
    for k in env:
        monkeypatch.delenv(k)
    return r


def check_queries(r, refs, what):
    for set_name, (o, d, ref) in refs.items():
        tag = f"{what} / {set_name}"
        tm = Q.bounds_for(ref[0])
        t, tri, uv = r.trace_closest(o, d, t_max=tm)
        et, etri, euv = Q.closest(ref, tm)
        assert np.array_equal(tri, etri), f"{tag}: {int((tri != etri).sum())} tri differ"
        assert np.array_equal(t.view(np.uint32), et.view(np.uint32)) and np.array_equal(uv.view(np.uint32), euv.view(np.uint32)), tag
        occ = r.trace_occluded(o, d, t_max=tm)
        assert occ.dtype == np.bool_ and np.array_equal(occ, Q.occluded(ref, tm)), f"{tag}: {int((occ != Q.occluded(ref, tm)).sum())} occlusions differ"
        # no bound, and a bound of TRT_INF: trace_closest's bits, which are the oracle's
        base = r.trace_closest(o, d)
        for b in (None, np.full(len(o), Q.TRT_INF, np.float32)):
            got = r.trace_closest(o, d, t_max=b)
            for x, y, z in zip(got, base, ref):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(y.view(np.uint32), z.view(np.uint32)), tag
        assert np.array_equal(r.trace_occluded(o, d), ref[1] >= 0), tag


# (a tree whose boxes do not nest gets no 8-wide collapse: trt_create walks it on the 4-wide nodes whatever TRT_NODE_KIND says)
CASES = ([("back", e) for e in UNIFORM] + [(n, e) for n in ("veach-mis", "staircase", "soup", "lbvh", "reference-tree") for e in PERSISTENT]
         + [("non-nesting", PERSISTENT[0])])


@pytest.mark.parametrize("name,env", CASES, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in e.items()) or 'default'}" for n, e in CASES])
def test_queries_match_the_oracle_on_every_driver(name, env, monkeypatch):
    s = scene_of(name)
    refs = reference(name, s)
    r = renderer_with(s, env, monkeypatch)
    try:
        st = r.trace_closest(*refs["random"][:2], want_stats=True)[3]
        if "TRT_NODE_KIND" in env:
            assert st.inner_node_bytes == (80 if env["TRT_NODE_KIND"] == "1" else 128), st.inner_node_bytes
        else:
            assert st.inner_node_bytes == 64
        check_queries(r, refs, f"{name} {env}")
    finally:
        r.close()


def _torch():
    import torch
    return torch


@pytest.mark.parametrize("name", ["back", "veach-mis"])
def test_device_entries_equal_the_host_entries(name, renderer_factory):
    """trace_closest_into / trace_occluded_into on torch tensors: the host entries' bits, on the default stream and on a torch side stream,
    with and without uv, at n = 1, 63, 65, 4096 and 2^20 + 17."""
    torch = _torch()
    s = scene_of(name)
    r = renderer_factory(s)
    dev = torch.device("cuda", 0)
    lo, hi = raygen.scene_bounds(s)
    side = torch.cuda.Stream(dev)
    for n in (1, 63, 65, 4096, (1 << 20) + 17):
        o, d = raygen.random_rays(n, lo, hi, seed=n)
        base_t = r.trace_closest(o, d)[0]
        tm = Q.bounds_for(base_t, seed=n)
        want = r.trace_closest(o, d, t_max=tm)
        want_occ = r.trace_occluded(o, d, t_max=tm)
        want_none = r.trace_closest(o, d)
        og, dg, tg = (torch.from_numpy(x).to(dev) for x in (o, d, tm))
        side.wait_stream(torch.cuda.current_stream(dev))
        for stream in (None, side):
            ptr = 0 if stream is None else stream.cuda_stream
            with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream(dev)):
                for bound, exp in ((tg, want), (None, want_none)):
                    t = torch.empty(n, dtype=torch.float32, device=dev)
                    tri = torch.empty(n, dtype=torch.int32, device=dev)
                    uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
                    st = r.trace_closest_into(og, dg, t, tri, uv, t_max=bound, stream_ptr=ptr)
                    assert st.launches[K_CLOSEST] == 1
                    got = (t.cpu().numpy(), tri.cpu().numpy(), uv.cpu().numpy())
                    for x, y in zip(got, exp):
                        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, n, ptr)
                    t2 = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
                    tri2 = torch.full((n,), 7, dtype=torch.int32, device=dev)
                    r.trace_closest_into(og, dg, t2, tri2, None, t_max=bound, stream_ptr=ptr)  # uv not wanted
                    assert np.array_equal(t2.cpu().numpy().view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(tri2.cpu().numpy(), exp[1])
                for dtype in (torch.uint8, torch.bool):
                    occ = torch.full((n,), 3, dtype=torch.uint8, device=dev).to(dtype)
                    st = r.trace_occluded_into(og, dg, occ, t_max=tg, stream_ptr=ptr)
                    assert st.rays_shadow == n and st.launches[K_SHADOW] == 1
                    got = occ.cpu().numpy()
                    assert got.view(np.uint8).max() <= 1 and np.array_equal(got.astype(bool), want_occ), (name, n, ptr, dtype)
    with pytest.raises(T.TrtError):
        r.trace_occluded_into(og, dg, torch.empty(n, dtype=torch.float32, device=dev))
    with pytest.raises(T.TrtError):
        r.trace_closest_into(og, dg, torch.empty(n - 1, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("name", ["back", "staircase"])
def test_stats_of_the_queries(name, renderer_factory):
    s = scene_of(name)
    r = renderer_factory(s)
    lo, hi = raygen.scene_bounds(s)
    o, d = raygen.random_rays(20000, lo, hi, seed=3)
    occ, st = r.trace_occluded(o, d, want_stats=True)
    assert st.rays_shadow == len(o) and st.launches[K_SHADOW] >= 1 and st.inner_visits[1] > 0 and st.tri_tests[1] > 0
    assert st.launches[K_CLOSEST] == 0 and st.inner_visits[0] == 0
    _, _, _, sc = r.trace_closest(o, d, want_stats=True, t_max=np.full(len(o), 10.0, np.float32))
    assert sc.launches[K_CLOSEST] == 1 and sc.inner_visits[0] > 0 and sc.rays_shadow == 0
    # occlusion stops at the first leaf that yields a hit: never more node visits than the closest-hit walk of the same rays
    _, _, _, full = r.trace_closest(o, d, want_stats=True)
    assert st.inner_visits[1] <= full.inner_visits[0], (st.inner_visits[1], full.inner_visits[0])
    ao, ad = SU.axis_rays(s, 64)
    _, st_axis = r.trace_occluded(ao, ad, want_stats=True)
    _, _, _, sc_axis = r.trace_closest(ao, ad, want_stats=True, t_max=np.full(len(ao), 1e30, np.float32))
    assert st_axis.redo_rays > 0 and sc_axis.redo_rays > 0


def test_queries_leave_renders_and_trace_closest_alone(renderer_factory):
    """On one handle: a render and trace_closest before and after a round of the new queries give the same bits (the shared scratch buffers)."""
    s = scene_of("veach-mis")
    r = renderer_factory(s)
    p = T.make_params(64, 36, 2, 9)
    lo, hi = raygen.scene_bounds(s)
    o, d = raygen.random_rays(50000, lo, hi, seed=8)
    img0, _ = r.render(p)
    tr0 = r.trace_closest(o, d)
    o2, d2 = raygen.random_rays(300000, lo, hi, seed=9)
    r.trace_occluded(o2, d2, t_max=np.full(len(o2), 3.0, np.float32))
    r.trace_closest(o2, d2, t_max=np.full(len(o2), 3.0, np.float32))
    img1, _ = r.render(p)
    tr1 = r.trace_closest(o, d)
    assert np.array_equal(img0, img1)
    for x, y in zip(tr0, tr1):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
