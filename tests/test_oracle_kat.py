"""Known-answer tests that pin the CPU oracle (oracle/oracle.cpp).

The reference ships no tests or golden vectors for this path, so these
are analytic: each checks one restated function against a value derived by hand or in float64.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import raygen
import scene_util as SU
import tinyraytracing_amd as T
from conftest import ROOT, get_scene

TRI = [0, 0, 0, 1, 0, 0, 0, 1, 0]  # v0, v1, v2 in the plane z = 0


# ---------------------------------------------------------------- interactTriangle (bvh.cpp:177-209)
def test_triangle_hit_distance_and_barycentrics():
    hit, out = O.tri_test(TRI, [0.25, 0.5, 2.0], [0, 0, -1])
    assert hit and out[0] == 2.0 and out[1] == 0.25 and out[2] == 0.5
    hit, out = O.tri_test(TRI, [0.25, 0.5, -3.0], [0, 0, 1])   # back face hits too (r1 || r2, bvh.cpp:200)
    assert hit and out[0] == 3.0


def test_triangle_edge_and_vertex_points_miss():
    # strict inequalities (bvh.cpp:197-198): a point exactly on an edge or a vertex is a miss
    for p in ([0.5, 0.0], [0.0, 0.5], [0.5, 0.5], [0.0, 0.0], [1.0, 0.0]):
        hit, _ = O.tri_test(TRI, [p[0], p[1], 1.0], [0, 0, -1])
        assert not hit
    assert O.tri_test(TRI, [0.5, 1e-6, 1.0], [0, 0, -1])[0]


def test_triangle_t_min_and_behind():
    assert not O.tri_test(TRI, [0.2, 0.2, 0.0004], [0, 0, -1])[0]      # t < 0.0005 (bvh.cpp:189)
    assert O.tri_test(TRI, [0.2, 0.2, 0.0006], [0, 0, -1])[0]
    assert not O.tri_test(TRI, [0.2, 0.2, -1.0], [0, 0, -1])[0]        # behind the origin


def test_triangle_parallel_cut():
    # |N.d| < 1e-5 misses (bvh.cpp:185); N = (0,0,1)
    d = np.array([1.0, 0.0, -0.5e-5]); d /= np.linalg.norm(d)
    assert not O.tri_test(TRI, [-1.0, 0.2, 0.5e-5], d)[0]
    d = np.array([1.0, 0.0, -4e-5]); d /= np.linalg.norm(d)
    assert O.tri_test(TRI, [-1.0, 0.2, 1.2 * 4e-5], d)[0]
    # scale invariance of the cut: the same directions on a triangle 1000x larger
    big = [0, 0, 0, 1000, 0, 0, 0, 1000, 0]
    d = np.array([1.0, 0.0, -0.5e-5]); d /= np.linalg.norm(d)
    assert not O.tri_test(big, [-1.0, 200, 0.5e-5], d)[0]


def test_triangle_barycentrics_match_float64_least_squares():
    """findBaryCor (triangle.cpp:12-29) solves [v0 v1 v2; 1 1 1] b = [P; 1] in double."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        v = rng.uniform(-5, 5, (3, 3))
        w = rng.dirichlet([1, 1, 1])
        P = w @ v
        o = P + rng.normal(size=3) * 3
        d = P - o
        dist = np.linalg.norm(d); d /= dist
        hit, out = O.tri_test(v.reshape(-1), o, d)
        if not hit:
            continue
        A = np.vstack([v.T.astype(np.float32).astype(np.float64), np.ones(3)])
        Ph = o.astype(np.float32).astype(np.float64) + d.astype(np.float32).astype(np.float64) * float(out[0])
        b = np.linalg.lstsq(A, np.append(Ph, 1.0), rcond=None)[0]
        assert abs(out[0] - dist) < 1e-4 * max(1.0, dist)
        assert np.allclose([1 - out[1] - out[2], out[1], out[2]], b, atol=5e-5)


# ---------------------------------------------------------------- interactAABB (bvh.cpp:231-245)
def test_aabb_cases():
    lo, hi = [0, 0, 0], [1, 1, 1]
    assert O.aabb(lo, hi, [-1, 0.5, 0.5], [1, 0, 0]) == 1.0            # entry distance
    assert O.aabb(lo, hi, [0.5, 0.5, 0.5], [1, 0, 0]) == 0.5           # origin inside -> exit distance
    assert O.aabb(lo, hi, [2, 0.5, 0.5], [1, 0, 0]) < 0                # box behind: t1 < 0 -> not > 0
    assert O.aabb(lo, hi, [-1, 2, 0.5], [1, 0, 0]) == -1.0             # misses the slab
    d = np.array([1, 1, 1]) / math.sqrt(3)
    assert abs(O.aabb(lo, hi, [-1, -1, -1], d) - math.sqrt(3)) < 1e-6


# ---------------------------------------------------------------- Sample (pathTracing.cpp:111-145)
def test_sample_frame_and_moments():
    rng = np.random.default_rng(9)
    axis = np.array([0.3, -0.5, 0.81]); axis /= np.linalg.norm(axis)
    u = rng.random((20000, 2)).astype(np.float32)
    dirs = np.array([O.sample(axis, 0, 1.0, float(a), float(b)) for a, b in u])
    assert np.allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-5)
    cos = dirs @ axis
    assert cos.min() >= -1e-6                                           # upper hemisphere
    assert abs(cos.mean() - 2 / 3) < 0.01                               # cosine-weighted: E[cos] = 2/3
    assert abs((cos ** 2).mean() - 0.5) < 0.01
    Ns = 50.0
    dirs = np.array([O.sample(axis, 1, Ns, float(a), float(b)) for a, b in u])
    cos = dirs @ axis
    assert abs(cos.mean() - (Ns + 1) / (Ns + 2)) < 5e-3                 # pdf ~ cos^Ns: E[cos] = (Ns+1)/(Ns+2)
    # phi is the FIRST draw: u_phi = 0 lies in the plane spanned by axis and `right`
    front = np.array([0.0, -axis[2], axis[1]]); front /= np.linalg.norm(front)   # |a.x| <= |a.y| branch
    d = O.sample(axis, 0, 1.0, 0.0, 0.5)
    assert abs(d @ front) < 1e-6
    assert abs(d @ axis - math.sqrt(0.5)) < 1e-6


def test_sample_branch_on_dominant_axis():
    a = np.array([0.9, 0.1, 0.42]); a /= np.linalg.norm(a)             # |a.x| > |a.y| -> front = normalize(a.z, 0, -a.x)
    front = np.array([a[2], 0, -a[0]]); front /= np.linalg.norm(front)
    d = O.sample(a, 0, 1.0, 0.25, 0.5)                                  # phi = pi/2 -> along front
    assert abs(d @ front - math.sqrt(0.5)) < 1e-6 and abs(d @ a - math.sqrt(0.5)) < 1e-6


# ---------------------------------------------------------------- glm::reflect / glm::refract
def test_reflect_refract_identities():
    n = np.array([0, 1, 0.0])
    i = np.array([1, -1, 0.0]) / math.sqrt(2)
    assert np.allclose(O.reflect(i, n), [1 / math.sqrt(2), 1 / math.sqrt(2), 0], atol=1e-7)
    t = O.refract(i, n, 1 / 1.5)
    sin_t = math.sin(math.pi / 4) / 1.5
    assert np.allclose(t, [sin_t, -math.sqrt(1 - sin_t ** 2), 0], atol=1e-6)
    assert np.allclose(np.linalg.norm(t), 1, atol=1e-6)
    # total internal reflection: glass -> air beyond the critical angle returns the zero vector
    g = np.array([math.sin(1.0), -math.cos(1.0), 0.0])
    assert np.array_equal(O.refract(g, n, 1.5), [0, 0, 0])
    assert np.allclose(O.refract([0, -1, 0], n, 1 / 1.5), [0, -1, 0], atol=1e-7)


def test_next_ray_fresnel_and_lobes():
    from tinyraytracing_amd._abi import Material
    fp = C.POINTER(C.c_float)
    def call(m, pn, inc, pixel):
        ctr = C.c_uint32(0)
        out = np.zeros(3, np.float32)
        pn = np.asarray(pn, np.float32); inc = np.asarray(inc, np.float32)
        ty = O.lib().oracle_next_ray(C.byref(m), pn.ctypes.data_as(fp), inc.ctypes.data_as(fp), 1, pixel, 0, C.byref(ctr), out.ctypes.data_as(fp))
        return ty, out, ctr.value
    glass = Material(); glass.Kd[:] = (0.5, 0.5, 0.5); glass.Tr[:] = (0.8, 1, 0.95); glass.Ns = 1; glass.Ni = 1.5
    pn, inc = [0, 1, 0], [0, -1, 0]
    types = [call(glass, pn, inc, k) for k in range(400)]
    n_tr = sum(1 for t, _, _ in types if t == 2)
    # normal incidence: F = ((1-1.5)/(1+1.5))^2 = 0.04 -> ~96 % refracted straight through
    assert 0.92 < n_tr / 400 < 0.99
    for t, d, c in types:
        if t == 2:
            assert np.allclose(d, [0, -1, 0], atol=1e-6) and c == 1          # Fresnel draw only
        else:
            assert t == 0 and c == 4 and d[1] > 0                            # falls through: lobe draw + phi + theta
    inside = [call(glass, pn, [math.sin(1.0), math.cos(1.0), 0.0], k) for k in range(200)]   # from inside, beyond the critical angle
    spec = [d for t, d, _ in inside if t == 1]
    assert spec and all(np.allclose(d, [math.sin(1.0), -math.cos(1.0), 0], atol=1e-6) for d in spec)   # TIR -> mirror, typed SPECULAR
    black = Material(); black.Ns = 1; black.Ni = 1
    t, d, c = call(black, pn, inc, 3)
    assert t == 3 and c == 1                                                 # Kd = Ks = 0 -> NaN weights -> INVALID (Q8)
    shiny = Material(); shiny.Kd[:] = (0.3, 0.2, 0.1); shiny.Ks[:] = (0.3, 0.2, 0.1); shiny.Ns = 200; shiny.Ni = 1
    kinds = [call(shiny, pn, [math.sqrt(0.5), -math.sqrt(0.5), 0], k)[0] for k in range(400)]
    assert 0.4 < kinds.count(0) / 400 < 0.6 and kinds.count(1) + kinds.count(0) == 400
    dull = Material(); dull.Kd[:] = (0.3, 0.2, 0.1); dull.Ks[:] = (0.3, 0.2, 0.1); dull.Ns = 1; dull.Ni = 1
    kinds = [call(dull, pn, inc, k)[0] for k in range(200)]
    assert kinds.count(3) > 60 and kinds.count(1) == 0                       # Ns <= 1: the specular half is INVALID


# ---------------------------------------------------------------- camera (main.cpp:88-95, camera.cpp:19-28)
def _camera_f32(cam, W, H, i, j, u1, u2):
    """main.cpp:88-95 + camera.cpp:19-28 emulated operation by operation in numpy float32/float64."""
    f = np.float32
    x = np.float64(j) / np.float64(W - 1.0) + (np.float64(f(u1)) - 0.5) / np.float64(W)
    y = np.float64(H - i) / np.float64(H - 1.0) + (np.float64(f(u2)) - 0.5) / np.float64(H)   # Q1: H - i
    s, t = f(x), f(y)
    llc = np.array(tuple(cam.lower_left_corner), f); hor = np.array(tuple(cam.horizontal), f)
    ver = np.array(tuple(cam.vertical), f); eye = np.array(tuple(cam.eye), f)
    d = ((llc + hor * s) + ver * t) - eye
    dd = f(f(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return d * (f(1.0) / np.sqrt(dd))


def test_camera_ray_quirks():
    s = get_scene("back", 1024, 1024)
    cam = s.flat.contents.camera
    for (i, j, u1, u2) in ((512, 0, 0.5, 0.5), (0, 10, 0.5, 0.5), (100, 100, 0.0, 0.5), (100, 100, 0.99999994, 0.25), (1023, 1023, 0.3, 0.9)):
        o, d = O.camera_ray(cam, 1024, 1024, i, j, u1, u2)
        assert np.allclose(o, [278, 273, -800])
        assert np.array_equal(d, _camera_f32(cam, 1024, 1024, i, j, u1, u2)), (i, j)
    # Q1: row 0 looks ABOVE the top edge of the viewport (t = H/(H-1) > 1); the usual H-1-i would give t = 1
    _, d_top = O.camera_ray(cam, 1024, 1024, 0, 512, 0.5, 0.5)
    ver_y = cam.vertical[1]
    assert d_top[1] / d_top[2] > 0.5 * ver_y * (1 + 0.5 / 1023)
    # Q2: the jitter spans one pixel in units of 1/W while the pixel pitch is 1/(W-1)
    _, d0 = O.camera_ray(cam, 64, 64, 32, 10, 0.0, 0.5)
    _, d1 = O.camera_ray(cam, 64, 64, 32, 11, 0.0, 0.5)
    _, dj = O.camera_ray(cam, 64, 64, 32, 10, 0.99999994, 0.5)
    pitch = d1[0] / d1[2] - d0[0] / d0[2]
    jit = dj[0] / dj[2] - d0[0] / d0[2]
    assert abs(jit / pitch - 63 / 64) < 1e-3


# ---------------------------------------------------------------- shared primitives (include/trt_prims.h)
def test_prims_accuracy_against_float64():
    L = O.lib()
    c = C.c_float(); s = C.c_float()
    worst = 0.0
    for u in np.linspace(0, 1, 4001, endpoint=False, dtype=np.float32):
        L.oracle_prims_sincos2pi(float(u), C.byref(c), C.byref(s))
        worst = max(worst, abs(c.value - math.cos(2 * math.pi * float(u))), abs(s.value - math.sin(2 * math.pi * float(u))))
    assert worst < 2.5e-7
    L.oracle_prims_sincos2pi(0.25, C.byref(c), C.byref(s)); assert (c.value, s.value) == (0.0, 1.0) or abs(c.value) < 1e-7
    rng = np.random.default_rng(1)
    for x, y in zip(rng.random(3000).astype(np.float32), np.exp(rng.uniform(-3, 7, 3000)).astype(np.float32)):
        got = L.oracle_prims_pow01(float(x), float(y))
        ref = float(x) ** float(y)
        assert abs(got - ref) <= 3e-6 * max(ref, 1e-30) * max(1.0, float(y)) + 1e-37, (x, y, got, ref)
    # at the exponents the shipped materials use (staircase Ns 1000 / 500 / 250 in the Phong lobe, 1 / (Ns + 1)
    # in its inverse CDF) the error does NOT grow with y: |y ln x| <= 87 wherever the result is not flushed, so the relative
    # error is bounded by 87 x the 1e-7 of the logarithm.  Measured <= 7.6e-6 over 40 000 bases per exponent.
    for y in (1000.0, 500.0, 250.0, 100.0, 1.0 / 1001.0, 1.0 / 501.0, 1.0 / 251.0):
        xs = np.concatenate([rng.random(4000), 1 - 10 ** rng.uniform(-6, 0, 4000)]).astype(np.float32)
        for x in xs[(xs > 0) & (xs < 1)]:
            got = L.oracle_prims_pow01(float(x), float(np.float32(y)))
            ref = float(x) ** float(np.float32(y))
            if ref > 1e-30:
                assert abs(got - ref) <= 1e-5 * ref, (x, y, got, ref)
    assert L.oracle_prims_pow01(0.37, 1.0) == np.float32(0.37)               # y == 1 exact
    assert L.oracle_prims_pow01(0.0, 5.0) == 0.0 and L.oracle_prims_pow01(1.0, 1000.0) == 1.0


def test_rng_stream_is_uniform_and_keyed():
    L = O.lib()
    u = np.array([L.oracle_prims_uniform(1, p, s, i) for p in range(40) for s in range(10) for i in range(25)])
    assert u.min() >= 0 and u.max() < 1
    assert abs(u.mean() - 0.5) < 0.01 and abs(u.var() - 1 / 12) < 0.005
    hist = np.histogram(u, bins=16, range=(0, 1))[0]
    assert hist.min() > 0.85 * len(u) / 16
    a = [L.oracle_prims_uniform(1, 7, 3, i) for i in range(8)]
    assert a == [L.oracle_prims_uniform(1, 7, 3, i) for i in range(8)]
    assert a != [L.oracle_prims_uniform(2, 7, 3, i) for i in range(8)]
    assert a != [L.oracle_prims_uniform(1, 8, 3, i) for i in range(8)] and a != [L.oracle_prims_uniform(1, 7, 4, i) for i in range(8)]
    # consecutive pixels/samples are uncorrelated in their first draw
    first = np.array([L.oracle_prims_uniform(5, p, 0, 0) for p in range(4000)])
    assert abs(np.corrcoef(first[:-1], first[1:])[0, 1]) < 0.05


# ---------------------------------------------------------------- traverseBVH (bvh.cpp:146-229)
@pytest.mark.parametrize("name,w,h", [("back", 64, 64), ("veach-mis", 64, 36), ("staircase", 64, 36)])
def test_traversal_equals_brute_force(name, w, h):
    s = get_scene(name, w, h)
    lo, hi = raygen.scene_bounds(s)
    o1, d1 = raygen.primary_rays(s, w, h, step=2)
    o2, d2 = raygen.random_rays(3000, lo, hi)
    org, dirs = np.vstack([o1, o2]), np.vstack([d1, d2])
    t, tri, uv = O.trace(s.flat, org, dirs, O.TRACE_REFERENCE)
    tb, trib, uvb = O.trace(s.flat, org, dirs, O.TRACE_BRUTE)
    assert np.array_equal(t, tb)
    same = tri == trib
    # equal-distance candidates in different leaves may resolve differently (bvh.cpp:168-174 vs index order)
    assert same.mean() > 0.999
    assert (tri >= 0).mean() > 0.3


def test_reference_builder_restatement_gives_same_hits():
    """oracle_build_bvh (bvh.cpp:16-144 incl. the Cost = INF fallback) vs the product builder."""
    s = get_scene("veach-mis", 64, 36)
    a = s.arrays()
    perm, nodes, n_nodes, depth = O.build_bvh(a["tri_v"], 8)
    assert sorted(perm.tolist()) == list(range(len(perm))) and 0 < n_nodes < 2 * len(perm)
    from tinyraytracing_amd._abi import SceneFlat
    f = s.flat.contents
    g = SceneFlat()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(SceneFlat))
    tv = np.ascontiguousarray(a["tri_v"][perm]); tvn = np.ascontiguousarray(a["tri_vn"][perm])
    tvt = np.ascontiguousarray(a["tri_vt"][perm]); tm = np.ascontiguousarray(a["tri_mat"][perm])
    fpt = C.POINTER(C.c_float)
    g.tri_v = tv.ctypes.data_as(fpt); g.tri_vn = tvn.ctypes.data_as(fpt); g.tri_vt = tvt.ctypes.data_as(fpt)
    g.tri_mat = tm.ctypes.data_as(C.POINTER(C.c_int32))
    g.nodes = nodes; g.n_nodes = n_nodes; g.bvh_depth = depth
    org, dirs = raygen.primary_rays(s, 64, 36)
    t0, tri0, _ = O.trace(s.flat, org, dirs)
    t1, tri1, _ = O.trace(C.pointer(g), org, dirs)
    assert np.array_equal(t0, t1)
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm), dtype=perm.dtype)
    hit = tri0 >= 0
    # same triangles (compare through the vertex data, the orders differ)
    assert np.array_equal(a["tri_v"][tri0[hit]], tv[tri1[hit]])


def test_emissive_wins_equal_distance(tmp_path):
    """bvh.cpp:168-172,219: of two coincident surfaces the emissive one is the hit, in either file order."""
    for order in ("lamp_first", "lamp_last"):
        lines, faces = ["vt 0 0", "vn 0 0 1"], []
        vb = 1
        q1 = SU.quad(-1, 1, -1, 1, 0, vb); vb = q1[2]
        q2 = SU.quad(-1, 1, -1, 1, 0, vb); vb = q2[2]
        mats = ("lamp", "white") if order == "lamp_first" else ("white", "lamp")
        obj = "\n".join(lines[:1] + lines[1:] + q1[0] + q2[0]) + "\n"
        obj += f"usemtl {mats[0]}\n" + "\n".join(x.format(n=1) for x in q1[1]) + f"\nusemtl {mats[1]}\n" + "\n".join(x.format(n=1) for x in q2[1]) + "\n"
        SU.write_scene(tmp_path, order, obj, SU.MTL_BASIC, lights=[("lamp", (5, 5, 5))])
        for leaf in (1, 8):
            s = SU.load(tmp_path, order, leaf_num=leaf)
            a = s.arrays()
            lamp_id = [k for k in range(s.info["n_materials"]) if s.material_name(k) == "lamp"][0]
            rng = np.random.default_rng(2)
            org = np.column_stack([rng.uniform(-0.9, 0.9, 300), rng.uniform(-0.9, 0.9, 300), np.full(300, 3.0)]).astype(np.float32)
            dirs = np.tile(np.array([0, 0, -1], np.float32), (300, 1))
            t, tri, _ = O.trace(s.flat, org, dirs)
            assert (tri >= 0).all() and np.all(t == 3.0)
            assert np.all(a["tri_mat"][tri] == lamp_id)


# ---------------------------------------------------------------- shade (pathTracing.cpp:3-102)
def test_iterative_equals_recursive_shade():
    for name, w, h, spp in (("back", 48, 48, 8), ("staircase", 48, 27, 4)):
        s = get_scene(name, w, h)
        p = T.make_params(w, h, spp, 123)
        a, sa = O.render(s.flat, p, mode=O.MODE_ITERATIVE)
        b, sb = O.render(s.flat, p, mode=O.MODE_RECURSIVE)
        assert (sa.rays_camera, sa.rays_shadow, sa.rays_indirect) == (sb.rays_camera, sb.rays_shadow, sb.rays_indirect)
        assert np.allclose(a, b, rtol=2e-5, atol=1e-6)


def test_direct_light_known_answer(tmp_path):
    """One diffuse floor point under a small square lamp, max_depth = 1: the pixel mean must equal the
    analytic NEE estimate E[radiance * cos_l * cos / d^2 * A * Kd/pi] (pathTracing.cpp:60-70)."""
    lines = ["vt 0 0", "vn 0 1 0", "vn 0 -1 0"]
    # floor y = 0 (normal +y), lamp y = 2 facing down, 0.2 x 0.2
    obj = "\n".join(lines) + "\n" + "v -50 0 -50\nv 50 0 -50\nv 50 0 50\nv -50 0 50\nv -0.1 2 -0.1\nv 0.1 2 -0.1\nv 0.1 2 0.1\nv -0.1 2 0.1\n"
    obj += "usemtl white\nf 1/1/1 3/1/1 2/1/1\nf 1/1/1 4/1/1 3/1/1\nusemtl lamp\nf 5/1/2 6/1/2 7/1/2\nf 5/1/2 7/1/2 8/1/2\n"
    SU.write_scene(tmp_path, "ka", obj, SU.MTL_BASIC, lights=[("lamp", (100, 100, 100))], w=16, h=16, fovy=0.5, eye=(3, 1, 0), lookat=(0, 0, 0))
    s = SU.load(tmp_path, "ka")
    p = T.make_params(16, 16, 256, 77, tile=(7, 7, 9, 9), max_depth=1)
    img, st = O.render(s.flat, p)
    # the camera looks at the origin from the side; tiny fov -> every sample hits ~ (0,0,0), straight under the lamp
    A = 0.04; d2 = 4.0
    expect = 100 * 1.0 * 1.0 / d2 * A * 0.7 / 3.1415926
    assert np.allclose(img.mean(axis=(0, 1)), expect, rtol=0.02)
    assert st.rays_indirect == 0 and st.rays_shadow == st.rays_camera


MTL_TWO_LAMPS = SU.MTL_BASIC + """newmtl lampB
Kd 0 0 0
Ks 0 0 0
Ns 1
Ni 1
"""


def _two_lamp_scene(tmp_path, blocker=False):
    """Floor y = 0; lamp (first light) 0.2 x 0.2 at y = 2 over the origin; lampB 2 x 2 at y = 2 centred on x = 3.
    `blocker`: a 1 x 1 white quad at y = 1 between the origin and the small lamp."""
    v = ["-50 0 -50", "50 0 -50", "50 0 50", "-50 0 50", "-0.1 2 -0.1", "0.1 2 -0.1", "0.1 2 0.1", "-0.1 2 0.1", "2 2 -1", "4 2 -1", "4 2 1", "2 2 1"]
    obj = "vt 0 0\nvn 0 1 0\nvn 0 -1 0\n" + "".join(f"v {x}\n" for x in v)
    obj += "usemtl white\nf 1/1/1 3/1/1 2/1/1\nf 1/1/1 4/1/1 3/1/1\nusemtl lamp\nf 5/1/2 6/1/2 7/1/2\nf 5/1/2 7/1/2 8/1/2\n"
    obj += "usemtl lampB\nf 9/1/2 10/1/2 11/1/2\nf 9/1/2 11/1/2 12/1/2\n"
    if blocker:
        obj += "v -0.5 1 -0.5\nv 0.5 1 -0.5\nv 0.5 1 0.5\nv -0.5 1 0.5\nusemtl white\nf 13/1/2 14/1/2 15/1/2\nf 13/1/2 15/1/2 16/1/2\n"
    SU.write_scene(tmp_path, "two", obj, MTL_TWO_LAMPS, lights=[("lamp", (100, 100, 100)), ("lampB", (10, 10, 10))], w=16, h=16, fovy=0.5, eye=(-3, 1, 0), lookat=(0, 0, 0))
    return SU.load(tmp_path, "two")


def test_fixed_nee_is_unbiased_where_the_quirks_are_not(tmp_path):
    """TRT_FLAG_FIXED_NEE (opt-out of Q3-Q5): with two lights of very different area the direct light at a floor
    point equals the area integral of radiance * cos * cos_l / d^2 * Kd/pi; parity mode draws every light's CDF
    with the first light's area (Q3) and is far off on the second one."""
    s = _two_lamp_scene(tmp_path)
    small = 100 * 0.04 / 4.0 * 0.7 / np.pi
    xs = (np.arange(400) + 0.5) / 400 * 2 + 2
    zs = (np.arange(400) + 0.5) / 400 * 2 - 1
    X, Z = np.meshgrid(xs, zs)
    big = 10 * (4.0 / (X * X + 4.0 + Z * Z) ** 2).mean() * 4.0 * 0.7 / np.pi
    p = T.make_params(16, 16, 1024, 5, tile=(7, 7, 9, 9), max_depth=1, flags=T.TRT_FLAG_FIXED_NEE)
    img, st = O.render(s.flat, p)
    assert np.allclose(img.mean(axis=(0, 1)), small + big, rtol=0.03)
    assert st.rays_shadow == 2 * st.rays_camera
    quirk, _ = O.render(s.flat, T.make_params(16, 16, 1024, 5, tile=(7, 7, 9, 9), max_depth=1))
    assert abs(quirk.mean() / (small + big) - 1) > 0.15


def test_fixed_nee_shadow_test_is_an_occlusion_test(tmp_path):
    """A quad between the floor point and the small lamp: the occlusion test removes exactly that lamp's light."""
    s = _two_lamp_scene(tmp_path, blocker=True)
    xs = (np.arange(400) + 0.5) / 400 * 2 + 2
    zs = (np.arange(400) + 0.5) / 400 * 2 - 1
    X, Z = np.meshgrid(xs, zs)
    big = 10 * (4.0 / (X * X + 4.0 + Z * Z) ** 2).mean() * 4.0 * 0.7 / np.pi
    img, _ = O.render(s.flat, T.make_params(16, 16, 1024, 5, tile=(7, 7, 9, 9), max_depth=1, flags=T.TRT_FLAG_FIXED_NEE))
    assert np.allclose(img.mean(axis=(0, 1)), big, rtol=0.03)


def test_image_statistics_against_reference_snapshots():
    """Loose pin: mean linear RGB of the reference's own 10-spp renders of test/back
    (image10.png 0.220/0.218/0.071, image10-0.png 0.237/0.243/0.098, 6.9 % black pixels), measured the
    same way: after the 8-bit gamma encode.  +-30 %."""
    s = get_scene("back", 256, 256)
    img, _ = O.render(s.flat, T.make_params(256, 256, 10, T.SEED_BACK))
    lin = (T.tonemap(img).astype(np.float64) / 255) ** 2.2
    mean = lin.reshape(-1, 3).mean(0)
    ref = np.array([(0.220 + 0.237) / 2, (0.218 + 0.243) / 2, (0.071 + 0.098) / 2])
    assert np.all(np.abs(mean / ref - 1) < 0.30), mean
    black = (lin.sum(-1) == 0).mean()
    assert abs(black - 0.069) < 0.01


def test_row_interleave_and_tiles_compose():
    s = get_scene("back", 40, 30)
    full, _ = O.render(s.flat, T.make_params(40, 30, 3, 9))
    parts = np.zeros_like(full)
    for r in range(3):
        p = T.make_params(40, 30, 3, 9, rows=(4, 3, r))
        out, _ = O.render(s.flat, p)
        parts[T.rows_selected(p)] = out
    assert np.array_equal(full, parts)
    tile, _ = O.render(s.flat, T.make_params(40, 30, 3, 9, tile=(5, 7, 22, 19)))
    assert np.array_equal(tile, full[7:19, 5:22])


def test_default_thread_count_honours_omp_num_threads():
    """threads <= 0 means OMP_NUM_THREADS when it is set (omp_get_max_threads), not every processor of the machine: a job given a
    share of a large host must not oversubscribe it.  A child process, because the OpenMP runtime reads the variable once."""
    machine = {os.cpu_count(), len(os.sched_getaffinity(0))}
    n = next(k for k in (3, 2, 5) if k not in machine)
    code = ("import oracle_lib as O, tinyraytracing_amd as T\n"
            "s = T.Scene.named('back', 16, 16)\n"
            "p = T.make_params(16, 16, 1, 7, tile=(4, 4, 6, 6))\n"
            "print(O.render(s.flat, p, threads=0)[1].threads, O.render_literal(s.flat, p, threads=0)[1].threads)\n")
    env = dict(os.environ, OMP_NUM_THREADS=str(n), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(n), str(n)], (out.stdout, n)
