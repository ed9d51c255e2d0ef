"""trt_update_geometry on the MI355X.  Handle A is created from the original scene and updated; handle B is created fresh from the scene
Scene.set_vertices left.  Every output element of every entry point is compared bit for bit, and B's render goes against the oracle, so the
chain ends at the reference's arithmetic."""
import numpy as np
import pytest

import oracle_lib as O
import raygen
import refit_ref as RR
import scene_util as SU
import tinyraytracing_amd as T

pytestmark = pytest.mark.gpu
W, H, SPP = 96, 64, 16
ENV_KEYS = ("TRT_SLIM_WALK", "TRT_BIN_WALK", "TRT_TRACE_IMPL", "TRT_NODE_KIND")


def renderer(scene, env, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = T.Renderer(scene, 0)
    for k in env:
        monkeypatch.delenv(k)
    return r


def rays_for(scene, n_random=200000):
    lo, hi = raygen.scene_bounds(scene)
    sets = [raygen.random_rays(n_random, lo, hi, seed=21), raygen.primary_rays(scene, W, H), SU.axis_rays(scene, 48)]
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


def outputs(r, scene, org, dirs, seed, renders=True):
    """Every output of every entry point, as a dict of arrays."""
    out = {}
    rng = np.random.default_rng(9)
    t_max = (rng.random(org.shape[0]) * 900.0).astype(np.float32)
    out["t"], out["tri"], out["uv"] = r.trace_closest(org, dirs)
    out["t_r"], out["tri_r"], out["uv_r"] = r.trace_closest(org, dirs, t_max=t_max)
    out["occ"] = r.trace_occluded(org, dirs)
    out["occ_r"] = r.trace_occluded(org, dirs, t_max=t_max)
    if renders:
        for name, flags in (("img", 0), ("img_nee", T.TRT_FLAG_FIXED_NEE)):
            p = T.make_params(W, H, SPP, seed, flags=flags)
            out[name], st = r.render(p)
            out[name + "_rays"] = np.array([st.rays_camera, st.rays_shadow, st.rays_indirect])
        aov = r.render_aov(T.make_params(W, H, SPP, seed))
        out.update({"aov_" + k: v for k, v in aov.items()})
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs between the updated and the fresh handle"


def check_case(scene, tri_v, monkeypatch, env=None, seed=T.SEED_BACK, lights=True, oracle=True, tri_vn=None, renders=True):
    """A = Renderer(scene) updated to tri_v; B = Renderer of the scene after set_vertices.  `scene` is moved in place."""
    env = env or {}
    A = renderer(scene, env, monkeypatch)
    scene.set_vertices(tri_v, tri_vn)
    if lights:
        A.update_geometry(scene)
    else:
        A.update_geometry(scene.arrays()["tri_v"], None if tri_vn is None else scene.arrays()["tri_vn"])
    B = renderer(scene, env, monkeypatch)
    org, dirs = rays_for(scene)
    oa, ob = outputs(A, scene, org, dirs, seed, renders), outputs(B, scene, org, dirs, seed, renders)
    assert_same(oa, ob, str(env))
    assert (oa["tri"] >= 0).sum() > 1000
    if oracle:
        p = T.make_params(W, H, SPP, seed)
        ref, ost = O.render(scene.flat, p)
        assert ob["img"].tobytes() == ref.tobytes(), "the fresh handle's render differs from the oracle"
        assert tuple(ob["img_rays"]) == (ost.rays_camera, ost.rays_shadow, ost.rays_indirect)
    return A, B, oa


BACK_ENVS = [{}, {"TRT_SLIM_WALK": "0"}, {"TRT_BIN_WALK": "0"}, {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}]


@pytest.mark.parametrize("env", BACK_ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_back_cube_translated_and_rotated(env, monkeypatch):
    s = T.Scene.named("back", W, H)
    v, sel = RR.move_inner_object(s)
    A, B, oa = check_case(s, v, monkeypatch, env)
    assert sel[oa["tri"][oa["tri"] >= 0]].any()


def test_back_light_lowered_with_tables(monkeypatch):
    s = T.Scene.named("back", W, H)
    v, sel = RR.move_material(s, "back:Light", delta=(0.0, -120.0, 0.0))
    check_case(s, v, monkeypatch)


def test_back_non_emissive_move_without_tables(monkeypatch):
    s = T.Scene.named("back", W, H)
    v, sel = RR.move_inner_object(s, delta=(-40.0, 0.0, 35.0), rotate_deg=-33.0)
    assert not np.isin(s.arrays()["tri_mat"][sel], [0]).any()  # material 0 is back:Light
    check_case(s, v, monkeypatch, lights=False)


@pytest.mark.parametrize("kind", ["0", "1"])
@pytest.mark.parametrize("name,n", [("blob", 20000), ("blob", 200000), ("soup", 100000), ("staircase", None)])
def test_deforming_scenes(name, n, kind, monkeypatch):
    s = T.Scene.named(name, W, H, n=n) if n else T.Scene.named(name, W, H)
    a = s.arrays()
    if name == "blob":
        v = RR.smooth_displace(a["tri_v"])
    elif name == "soup":
        v = RR.jitter(a["tri_v"])
    else:
        v, _ = RR.move_material(s, "Wood", delta=(0.3, 0.1, -0.2), rotate_deg=12.0)
    seed = {"blob": T.SEED_BLOB, "soup": T.SEED_SOUP, "staircase": T.SEED_STAIRCASE}[name]
    check_case(s, v, monkeypatch, {"TRT_NODE_KIND": kind}, seed=seed)


@pytest.mark.parametrize("tree", ["reference-leaf8", "lbvh", "renumbered", "shrunk"])
def test_foreign_trees(tree, monkeypatch):
    if tree == "reference-leaf8":
        s = SU.load_with_reference_tree("veach-mis", W, H)
    elif tree == "lbvh":
        s = T.Scene.named("staircase", W, H, builder="lbvh")
    else:
        s = T.Scene.named("staircase", W, H)
        if tree == "renumbered":
            assert SU.renumber_nodes_reversed(s) > 0
        else:
            assert SU.shrink_some_boxes(s, 60) > 0  # A's tree does not nest before the update, B's does
    check_case(s, RR.smooth_displace(s.arrays()["tri_v"], amp=0.8 if tree == "reference-leaf8" else 0.4), monkeypatch, seed=T.SEED_STAIRCASE)


def test_three_updates_the_last_back_to_the_original(monkeypatch):
    s = T.Scene.named("blob", W, H, n=20000)
    a = s.arrays()
    org, dirs = rays_for(s)
    never = renderer(s, {}, monkeypatch)
    want = outputs(never, s, org, dirs, T.SEED_BLOB)
    A = renderer(s, {}, monkeypatch)
    for v in (RR.smooth_displace(a["tri_v"]), RR.jitter(a["tri_v"]), a["tri_v"]):
        s.set_vertices(v, a["tri_vn"])
        A.update_geometry(s)
    assert_same(outputs(A, s, org, dirs, T.SEED_BLOB), want, "after three updates")


def test_every_triangle_collapsed_to_a_point(monkeypatch):
    """Degenerate triangles have no area: the light tables of such a scene hold NaN, which a handle that bisects its CDFs refuses (include/trt.h),
    so the tables stay and the ray queries — all that does not read them — are compared."""
    s = T.Scene.named("blob", W, H, n=20000)
    v = s.arrays()["tri_v"].copy()
    v[:, 1:, :] = v[:, :1, :]
    A = renderer(s, {}, monkeypatch)
    s.set_vertices(v)
    with pytest.raises(T.TrtError):
        A.update_geometry(s)
    A.update_geometry(v)
    B = renderer(s, {}, monkeypatch)
    org, dirs = rays_for(s, 50000)
    assert_same(outputs(A, s, org, dirs, 1, renders=False), outputs(B, s, org, dirs, 1, renders=False), "points")


def test_boxes_past_2_to_the_40(monkeypatch):
    s = T.Scene.named("blob", W, H, n=20000)
    a = s.arrays()
    lo, hi = raygen.scene_bounds(s)
    org, dirs = raygen.random_rays(100000, lo, hi, seed=4)
    A = renderer(s, {"TRT_NODE_KIND": "1"}, monkeypatch)
    assert A.trace_closest(org, dirs, want_stats=True)[3].inner_node_bytes == 80
    # a moderate update keeps the 8-wide nodes ...
    s.set_vertices(RR.smooth_displace(a["tri_v"]))
    A.update_geometry(s)
    assert A.trace_closest(org, dirs, want_stats=True)[3].inner_node_bytes == 80
    # ... boxes that reach 2^40 end them: A leaves the 8-wide nodes, and a fresh handle never gets them
    scale = np.float32(2.0 ** 33)
    s.set_vertices(a["tri_v"] * scale)
    A.update_geometry(s)
    B = renderer(s, {"TRT_NODE_KIND": "1"}, monkeypatch)
    org = org * scale
    ta, tb = A.trace_closest(org, dirs, want_stats=True), B.trace_closest(org, dirs, want_stats=True)
    for x, y in zip(ta[:3], tb[:3]):  # (at this size nothing is nearer than TRT_INF: the records agree as misses, the walks as node visits)
        assert x.tobytes() == y.tobytes()
    assert ta[3].inner_node_bytes == tb[3].inner_node_bytes == 128
    assert A.trace_occluded(org, dirs).tobytes() == B.trace_occluded(org, dirs).tobytes()
    # for good: back at the original size the handle stays on the exact nodes, with a fresh handle's results
    s.set_vertices(a["tri_v"], a["tri_vn"])
    A.update_geometry(s)
    B = renderer(s, {"TRT_NODE_KIND": "1"}, monkeypatch)
    org = org / scale
    ta, tb = A.trace_closest(org, dirs, want_stats=True), B.trace_closest(org, dirs, want_stats=True)
    for x, y in zip(ta[:3], tb[:3]):
        assert x.tobytes() == y.tobytes()
    assert (ta[1] >= 0).sum() > 1000
    assert (ta[3].inner_node_bytes, tb[3].inner_node_bytes) == (128, 80)


@pytest.mark.parametrize("name,n", [("blob", 200000), ("soup", 100000), ("staircase", None)])
def test_an_updated_handle_keeps_its_node_kind(name, n, monkeypatch):
    """On the 8-wide nodes an updated handle reports the node kind of trt_create; on the 4-wide nodes likewise.  (What it visits there:
    tests/test_gpu_refit_work.py.)"""
    for kind, node_bytes in (("1", 80), ("0", 128)):
        s = T.Scene.named(name, W, H, n=n) if n else T.Scene.named(name, W, H)
        v = RR.jitter(s.arrays()["tri_v"], amp=0.01 if name == "staircase" else 1.0)
        A = renderer(s, {"TRT_NODE_KIND": kind}, monkeypatch)
        s.set_vertices(v)
        A.update_geometry(s)
        lo, hi = raygen.scene_bounds(s)
        org, dirs = raygen.random_rays(50000, lo, hi, seed=8)
        assert A.trace_closest(org, dirs, want_stats=True)[3].inner_node_bytes == node_bytes


def test_host_and_device_entries_agree_and_bad_arguments_leave_the_handle_alone(monkeypatch):
    import torch
    s = T.Scene.named("staircase", W, H)
    a = s.arrays()
    org, dirs = rays_for(s, 50000)
    A = renderer(s, {}, monkeypatch)
    D = renderer(s, {}, monkeypatch)
    before = outputs(A, s, org, dirs, T.SEED_STAIRCASE)
    dev = torch.device("cuda", 0)
    good = torch.from_numpy(a["tri_v"]).to(dev)
    with pytest.raises(T.TrtError):
        D.update_geometry_from(torch.from_numpy(a["tri_v"]))              # a host tensor
    with pytest.raises(T.TrtError):
        D.update_geometry_from(good[:-1])                                  # n_tris differs
    with pytest.raises(T.TrtError):
        D.update_geometry_from(good.reshape(-1, 9))                        # wrong shape
    with pytest.raises(T.TrtError):
        D.update_geometry_from(good, tri_vn=good.to(torch.float64))        # wrong dtype
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = a["tri_v"].copy()
        bad[len(bad) // 2, 2, 1] = bad_value
        with pytest.raises(T.TrtError, match="NaN or infinite"):
            D.update_geometry_from(torch.from_numpy(bad).to(dev))
        with pytest.raises(T.TrtError, match="NaN or infinite"):
            D.update_geometry(bad)
    assert_same(outputs(D, s, org, dirs, T.SEED_STAIRCASE), before, "after refused updates")
    v, _ = RR.move_material(s, "Wood", delta=(0.3, 0.1, -0.2), rotate_deg=12.0)
    s.set_vertices(v)
    st_h = A.update_geometry(s, want_stats=True)
    st_d = D.update_geometry_from(torch.from_numpy(v).to(dev), tri_vn=torch.from_numpy(s.arrays()["tri_vn"]).to(dev), lights_from=s)
    assert_same(outputs(A, s, org, dirs, T.SEED_STAIRCASE), outputs(D, s, org, dirs, T.SEED_STAIRCASE), "host against device entry")
    for st in (st_h, st_d):
        assert st.launches[T.TRT_K_REFIT] > 0 and st.kernel_ms[T.TRT_K_REFIT] > 0 and st.render_ms >= st.kernel_ms[T.TRT_K_REFIT]
        assert st.rays == 0 and st.shaded_hits == 0 and sum(st.inner_visits) == 0 and sum(st.tri_tests) == 0 and st.redo_rays == 0
        assert all(st.launches[k] == 0 for k in range(7))


# launches[TRT_K_REFIT] of one update of `back` per wave driver and node kind: recorded on the GPU from the build of the commit before the update's host
# driver was split into stages (the vertex check, the triangle records, one launch per level of each tree the handle walks, the plane filter, the light boxes)
REFIT_LAUNCHES = [({"TRT_TRACE_IMPL": "0"}, 10), ({"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, 10), ({"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}, 13)]


@pytest.mark.parametrize("env,launches", REFIT_LAUNCHES, ids=lambda x: ",".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else str(x))
def test_an_update_reports_the_launches_it_made_and_nothing_else(env, launches, monkeypatch):
    """The bit-for-bit tests cannot see a launch that was added, dropped or moved out of the count: the count of each entry is a literal, the
    first update of a handle (which also numbers its trees: those launches are not the update's) reports what the later ones report."""
    import torch
    s = T.Scene.named("back", W, H)
    v, _ = RR.move_inner_object(s)
    A = renderer(s, env, monkeypatch)
    s.set_vertices(v)
    dv = torch.from_numpy(v).to(torch.device("cuda", 0))
    stats = [("host entry with light tables", A.update_geometry(s, want_stats=True)),
             ("device entry with light tables", A.update_geometry_from(dv, lights_from=s)),
             ("host entry without tables", A.update_geometry(v, want_stats=True))]
    for what, st in stats:
        print(f"{env} {what}: launches {list(st.launches)} kernel_ms {st.kernel_ms[T.TRT_K_REFIT]:.4f} render_ms {st.render_ms:.4f}")
    for what, st in stats:
        assert st.launches[T.TRT_K_REFIT] == launches, what
        assert all(st.launches[k] == 0 for k in range(len(st.launches)) if k != T.TRT_K_REFIT), what
        assert st.render_ms >= st.kernel_ms[T.TRT_K_REFIT] > 0, what
    A.close()
    s.close()


def _vertex_eye_scene_displaced(tmp_path):
    """test_hostsim_parity's vertex-eye scene with its one triangle elsewhere, loaded from a file of its own: no box of this tree — the box of the root's empty
    second leaf included, which an update leaves alone — has a plane of the fixture's."""
    obj = ("v 54434.95 57506.86 -161.27\nv 55692.92 56346.13 857.39\nv 56527.36 57846.1 -2700.01\n"
           "vn 0 0 1\nvt 0 0\nusemtl lamp\nf 1/1/1 2/1/1 3/1/1\n")
    SU.write_scene(tmp_path, "eye_moved", obj, SU.MTL_BASIC, lights=[("lamp", (4, 8, 9.5))], w=24, h=5, fovy=20.0, eye=(74036.484375, 79794.8046875, -4266.68115234375),
                   lookat=(72698.703125, 79148.5546875, -1440.929931640625))
    return SU.load(tmp_path, "eye_moved", leaf_num=15)


@pytest.mark.parametrize("impl,nk", [("0", "0"), ("3", "0"), ("3", "1")])
def test_an_update_rebuilds_the_plane_filter_for_the_new_planes(impl, nk, tmp_path, monkeypatch):
    """test_hostsim_parity's vertex-eye scene reached by an UPDATE: the handle is created with the triangle elsewhere and moved to the fixture's vertices.
    The rays' origin then sits on a vertex of the (unpadded at 7e4) leaf box, and the rays with a zero direction component find the triangle only through the
    literal slab test — which they get only if the filter of planeMaybe() knows the planes of the NEW boxes (k_refit_planes).  A filter left as trt_create made
    it clears those origins, the clean slab test runs, and the hits are lost.  Hits equal the oracle's on the scene set_vertices left, bit for bit."""
    from test_hostsim_parity import _vertex_eye_scene
    fixture = _vertex_eye_scene(tmp_path)
    f = fixture.flat.contents
    rng = np.random.default_rng(3)
    rays = [O.camera_ray(f.camera, 24, 5, 1, int(rng.integers(17, 22)), float(np.float32(rng.random())), float(np.float32(rng.random()))) for _ in range(20000)]
    org, dirs = np.array([r[0] for r in rays], np.float32), np.array([r[1] for r in rays], np.float32)
    v0, vn0 = fixture.arrays()["tri_v"].copy(), fixture.arrays()["tri_vn"].copy()
    s = _vertex_eye_scene_displaced(tmp_path)
    assert not np.isin(raygen.box_planes(s.flat), raygen.box_planes(fixture.flat)).any()
    A = renderer(s, {"TRT_TRACE_IMPL": impl, "TRT_NODE_KIND": nk}, monkeypatch)
    s.set_vertices(v0, vn0)
    A.update_geometry(s)
    t0, tri0, uv0 = O.trace(s.flat, org, dirs)
    assert (tri0[(dirs == 0).any(1)] >= 0).sum() > 50
    t1, tri1, uv1 = A.trace_closest(org, dirs)
    assert np.array_equal(tri0, tri1) and np.array_equal(t0, t1) and np.array_equal(uv0, uv1)
    A.close()
    s.close()
    fixture.close()
