"""The written arguments behind the traversal's bit parity, checked decision by decision on the CPU build of the device code (tests/hostsim):
the quantised-node superset claim (trt_oct.h, header (1)), the culling bound (trt_prims.h, trt_path.h above leafEntry), the light boxes (trt_oct.h above
LightBox) and the plane filter (trt_path.h planeMaybe).  Every property is exact — zero violations — and every test also asserts how many cases REACHED
its property (half of what the generators yield), so that a green result is not an empty one.  One negative control per checker shows it can fail."""
import numpy as np
import pytest

import hostsim_lib as H
import node_cases as NC
import oracle_lib as O
import raygen
import refit_ref as RR
import scene_util as SU
import tinyraytracing_amd as T

INF = np.float32(np.inf)
SCENES = ["staircase", "veach-mis", "blob", "soup"]
_cache = {}


def _scene(name):
    if name in ("blob", "soup"):
        return T.Scene.named(name, 64, 36, n=20000)
    if name.endswith("@ref8"):
        return SU.load_with_reference_tree(name[:-5], 64, 36)
    return T.Scene.named(name, 64, 36)


def _oct_tree(s):
    """The scene's 8-wide nodes as buildOct lays them out and the exact box octQuantise was fed for every slot."""
    from test_refit_cpu import _oct_case
    _, _, before, after, slot_box, _ = _oct_case(s, s.arrays()["tri_v"])
    assert RR.same_bits(before, after)
    return before.view(H.OCT_DT).copy(), slot_box.copy()


def scene_case(name):
    """Scene, rays and the oracle's hits, shared by the tests: raygen's adversarial, grazing and random rays, and rays aimed at corners, edges and faces of
    the exact boxes of random slots of the scene's oct tree (where it has one) or of random BVH2 boxes, twice: with node_cases' mix of directions, and with
    a direction component in the denormal range on every ray."""
    if name not in _cache:
        s = _scene(name)
        lo, hi = raygen.scene_bounds(s)
        sets = [raygen.adversarial_rays(s, 6000), raygen.grazing_rays(s.flat, 6000), raygen.random_rays(6000, lo, hi)]
        far = [np.zeros(len(x[0]), bool) for x in sets]
        tree = _oct_tree(s) if H.compressible(s.flat) else None
        rng = np.random.default_rng(17)
        if tree:
            onodes, slot_box = tree
            ni = rng.integers(0, len(onodes), 12000)
            used = onodes["meta"][ni] != 0
            boxes = slot_box[ni, (rng.random(used.shape) * used).argmax(1)]
        else:
            nodes = RR.nodes_of(s)
            ni = rng.integers(0, len(nodes), 12000)
            boxes = np.concatenate([nodes["lo0"][ni], nodes["hi0"][ni]], 1)
        # the second set: every direction with a component of 3.2e-39 .. 3.2e-38, so that planes a few units from the origin already overflow (small rooms)
        for seed, tiny in ((23, (1 / 3, -38.0, -30.0)), (29, (1.0, -38.5, -37.5))):
            o, d, f = NC.rays_at_boxes(boxes, seed=seed, tiny=tiny)
            sets.append((o, d))
            far.append(f)
        org, dirs = np.concatenate([x[0] for x in sets]), np.concatenate([x[1] for x in sets])
        t, tri, _ = O.trace(s.flat, org, dirs)
        _cache[name] = dict(scene=s, org=org, dirs=dirs, far=np.concatenate(far), t=t, tri=tri, tree=tree)
    return _cache[name]


# ---- a. quantised nodes ----------------------------------------------------------------------------------------------------------------------------------
def _synthetic():
    if "syn" not in _cache:
        blo, bhi, kind = NC.synthetic_nodes(4096)
        nodes, ok = H.oct_quantise_nodes(blo, bhi, kind)
        assert ok.all()
        slot_box = np.concatenate([blo, bhi], 2)
        rng = np.random.default_rng(5)
        node = np.repeat(np.arange(len(nodes)), 64).astype(np.uint32)
        used = kind[node] != 0
        org, dirs, far = NC.rays_at_boxes(slot_box[node, (rng.random(used.shape) * used).argmax(1)], seed=3)
        passes, entry = H.slot_ref(slot_box, node, org, dirs)
        idx, cull = NC.culls_for(passes, entry, used, np.full(len(node), INF), rng)
        _cache["syn"] = (nodes, slot_box, node[idx], org[idx], dirs[idx], cull, passes[idx], entry[idx], far[idx])
    return _cache["syn"]


def _floors(counts, floors):
    for k, v in floors.items():
        assert counts[k] >= v, f"only {counts[k]} cases of '{k}' reached the property (floor {v}): {counts}"


def test_superset_on_synthetic_nodes():
    """4 096 nodes from octQuantise (node_cases.synthetic_nodes: extents 2^-20 .. 2^34, frames up to 2^38 from 0, flat boxes, one slot, eight slots, the exponent
    byte at its floor) x 64 rays aimed at a slot's corners, edges and faces x culls (+inf; a passing slot's entry and the floats either side of it).
    Yield: 582 051 reference passes; 233 306 with a finite cull within one ulp of the entry; 143 606 on flat boxes; 59 944 with an overflowed
    product; 103 910 from origins 2^20 extents away.  Misses: 0."""
    nodes, slot_box, node, org, dirs, cull, passes, entry, far = _synthetic()
    assert ((nodes["ew"] & 0xFF) == 1).sum() > 500  # exponent bytes at the floor
    counts, text = NC.superset(nodes, slot_box, node, org, dirs, cull, H.oct_visit_cases(nodes, node, org, dirs, cull), passes, entry, far)
    print(counts)
    assert counts["misses"] == 0, text
    _floors(counts, dict(passes=291025, near_cull=116653, flat=71803, overflow=29972, far=51955))


def test_superset_control_far_bytes_moved_inward_by_one_miss():
    """The checker can fail: on a copy of the nodes whose box bytes are moved inward by one (lower bytes + 1, upper bytes - 1) octVisit misses reference passes."""
    nodes, slot_box, node, org, dirs, cull, passes, entry, far = _synthetic()
    bad = nodes.copy()
    bad["q"][:, :3] = np.where(bad["q"][:, :3] < 255, bad["q"][:, :3] + 1, 255)
    bad["q"][:, 3:] = np.where(bad["q"][:, 3:] > 0, bad["q"][:, 3:] - 1, 0)
    counts, _ = NC.superset(bad, slot_box, node, org, dirs, cull, H.oct_visit_cases(bad, node, org, dirs, cull), passes, entry, far)
    assert counts["misses"] > 1000, counts


@pytest.mark.parametrize("name", SCENES)
def test_superset_on_real_oct_trees(name):
    """The scene's own oct tree walked along the REFERENCE's descent (a child iff boxTest passes its exact box: hostsim_oct_descent), every reached node
    visited with culls +inf, trt_cull_bound(the oracle's hit), and a passing slot's entry with the floats either side of it.  The yield per scene is
    written beside OCT_FLOORS.  Flat boxes do not occur in these trees (the builders pad every leaf box by 0.001): that count is asserted on the
    synthetic nodes only.  Misses: 0."""
    c = scene_case(name)
    onodes, slot_box = c["tree"]
    alpha, nested, _ = H.scene_info(c["scene"].flat)
    assert nested
    node, ray = H.oct_descent(onodes, slot_box, c["org"], c["dirs"])
    org, dirs = c["org"][ray], c["dirs"][ray]
    passes, entry = H.slot_ref(slot_box, node, org, dirs)
    bound = np.where(c["tri"] >= 0, H.cull_bound(c["t"], alpha), INF).astype(np.float32)
    idx, cull = NC.culls_for(passes, entry, onodes["meta"][node] != 0, bound[ray], np.random.default_rng(9))
    node, org, dirs = node[idx], org[idx], dirs[idx]
    counts, text = NC.superset(onodes, slot_box, node, org, dirs, cull, H.oct_visit_cases(onodes, node, org, dirs, cull), passes[idx], entry[idx], c["far"][ray][idx])
    print(name, len(onodes), "nodes", counts)
    assert counts["misses"] == 0, text
    _floors(counts, OCT_FLOORS[name])


# half of the yield: reference passes / with the cull within one ulp of the entry / with an overflowed product / from 2^20 extents away, which is
# staircase 4251957 / 1420400 / 183712 / 569631; veach-mis 1566716 / 511605 / 57606 / 224513; blob 2416355 / 675912 / 770752 / 326112; soup 3125730 / 918482 / 1085492 / 396024
OCT_FLOORS = {"staircase": dict(passes=2125978, near_cull=710200, overflow=91856, far=284815),
              "veach-mis": dict(passes=783358, near_cull=255802, overflow=28803, far=112256),
              "blob": dict(passes=1208177, near_cull=337956, overflow=385376, far=163056),
              "soup": dict(passes=1562865, near_cull=459241, overflow=542746, far=198012)}


def test_zero_entries_carry_the_sign_gfx950_gives_them():
    """Box entries that are a zero through fminf / fmaxf of zeros of opposite sign: libm picks one by operand position, v_min_f32 / v_max_f32 order them.
    trt_fminf / trt_fmaxf (trt_prims.h) order the zeros on the host too: the CPU build returns gfx950's words for the recorded cases."""
    got = H.box_cases(NC.ZERO_SIGN_BOXES, NC.ZERO_SIGN_ORG, NC.ZERO_SIGN_DIR)
    assert np.array_equal(got, NC.ZERO_SIGN_WORDS), [[hex(int(x)) for x in r] for r in got]


# ---- b. the culling chain on the oracle's hits -------------------------------------------------------------------------------------------------------------
# half of the yield (rays, boxes): staircase 31465 / 531040, veach-mis 29222 / 369289, blob 29660 / 486048, soup 28584 / 399339, veach-mis@ref8 28435 / 315855
CHAIN_FLOORS = {"staircase": (15732, 265520), "veach-mis": (14611, 184644), "blob": (14830, 243024), "soup": (14292, 199669), "veach-mis@ref8": (14217, 157927)}


@pytest.mark.parametrize("name", SCENES + ["veach-mis@ref8"])
def test_culling_chain_on_the_oracles_hits(name):
    """For the oracle's hit (t, tri) of every ray of scene_case (misses and the rays traceClosest walks without culling left out), every box on tri's root
    path in the caller's BVH2 and in the 4-wide collapse: boxTest passes, entries do not decrease from the root down, NOT t < trt_leaf_floor(entry), NOT
    entry > trt_cull_bound(t).  Yield (rays, boxes) per scene: twice CHAIN_FLOORS."""
    c = scene_case(name)
    got = H.cull_chain(c["scene"].flat, c["org"], c["dirs"], c["t"], c["tri"])
    assert got is not None, "the boxes of this tree nest"
    counts, text = got
    print(name, counts)
    assert counts["bad"] == [0, 0, 0, 0], text
    lo_rays, lo_boxes = CHAIN_FLOORS[name]
    assert counts["rays"] >= lo_rays and counts["boxes"] >= lo_boxes, counts


def test_control_the_chain_checker_reports_hits_moved_in_front_of_their_boxes():
    """The checker can fail: with every t halved, hits lie in front of the boxes of their leaves and the chain reports 't < floor(entry)'."""
    c = scene_case("staircase")
    counts, text = H.cull_chain(c["scene"].flat, c["org"], c["dirs"], c["t"] * np.float32(0.5), c["tri"])
    assert counts["bad"][2] > 1000 and "t < floor(entry)" in text, counts


def test_culling_chain_is_not_claimed_for_a_tree_that_does_not_nest():
    s = T.Scene.named("staircase", 64, 36)
    assert SU.shrink_some_boxes(s, 60) > 0
    o, d = raygen.random_rays(100, *raygen.scene_bounds(s))
    t, tri, _ = O.trace(s.flat, o, d)
    assert H.cull_chain(s.flat, o, d, t, tri) is None
    s.close()


# ---- c. the pure float statement ---------------------------------------------------------------------------------------------------------------------------
def _float_triples(n=1 << 21, seed=4):
    """(b, alpha): b over every exponent, denormals and 0 included; alpha 0 (a quarter) or 2^-17 of a magnitude within 2^+-30 of b's."""
    rng = np.random.default_rng(seed)
    b = ((rng.integers(0, 255, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32)).view(np.float32).copy()
    b[::64] = 0.0
    b[1::64] = (rng.integers(1, 1 << 23, len(b[1::64])).astype(np.uint32)).view(np.float32)  # denormals
    mag = np.where(b > 0, b.astype(np.float64), 1.0) * np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-30, 31, n))
    with np.errstate(over="ignore", under="ignore"):
        alpha = (mag * 2.0 ** -17).astype(np.float32)
    alpha[rng.random(n) < 0.25] = 0.0
    alpha[~np.isfinite(alpha)] = 0.0
    return b, alpha


def _floor_above_bound_violations(b, alpha, bound):
    e = np.nextafter(bound, INF)
    ok = np.isfinite(bound)  # a bound of +inf never culls: nothing lies above it
    fl = H.leaf_floor(e, alpha)
    return int(ok.sum()), np.nonzero(ok & ~(fl > b))[0], e, fl


def test_the_floor_of_the_first_entry_above_the_cull_bound_is_above_b():
    """trt_prims.h: e > trt_cull_bound(b, alpha) implies trt_leaf_floor(e, alpha) > b — at the first float above the bound, so (the floor is monotone, below)
    at every one.  2 097 152 triples, 2 095 346 with a finite bound.  Violations: 0."""
    b, alpha = _float_triples()
    n, bad, e, fl = _floor_above_bound_violations(b, alpha, H.cull_bound(b, alpha))
    print(n, "finite bounds;", int((b == 0).sum()), "zeros,", int(((b > 0) & (b < 1.1754944e-38)).sum()), "denormals,", int((alpha == 0).sum()), "with alpha 0")
    assert len(bad) == 0, [(b[i], alpha[i], e[i], fl[i]) for i in bad[:8]]
    assert n >= 1047673 and (b == 0).sum() >= 16384 and ((b > 0) & (b < 1.1754944e-38)).sum() >= 16384 and (alpha == 0).sum() >= 262144


def test_control_a_cull_bound_without_its_factor_is_violated():
    """The checker can fail: with the bound b + 2 alpha — the factor 1 + 2^-14 left out — the floor of the next entry is not above b."""
    b, alpha = _float_triples(1 << 18)
    with np.errstate(over="ignore"):
        plain = (b + (alpha + alpha)).astype(np.float32)
    n, bad, _, _ = _floor_above_bound_violations(b, alpha, plain)
    assert len(bad) > n // 4, (len(bad), n)


def test_leaf_floor_is_monotone_in_the_entry():
    """trt_leaf_floor(e, alpha) does not decrease with e: over consecutive floats across 0 (denormals, -0, +0: where KNEG hands over to KPOS) at every
    exponent's alpha, and over random sorted entries of every exponent and both signs."""
    rng = np.random.default_rng(6)
    around0 = np.concatenate([-np.arange(4096, 0, -1, dtype=np.uint32).view(np.float32), np.array([-0.0, 0.0], np.float32), np.arange(1, 4097, dtype=np.uint32).view(np.float32)])
    n_pairs = 0
    for alpha in [np.float32(0)] + [np.float32(2.0 ** k) for k in range(-149, 128, 4)]:
        wide = ((rng.integers(0, 255, 20000).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, 20000).astype(np.uint32)).view(np.float32) * rng.choice([-1, 1], 20000).astype(np.float32)
        for e in (around0, np.sort(np.concatenate([wide, around0]))):
            fl = H.leaf_floor(e, alpha)
            ok = ~np.isnan(fl[1:]) & ~np.isnan(fl[:-1])
            assert not (fl[1:][ok] < fl[:-1][ok]).any(), (alpha, e[1:][ok][fl[1:][ok] < fl[:-1][ok]][:4])
            n_pairs += int(ok.sum())
    assert n_pairs >= 1000000


# ---- d. light boxes ------------------------------------------------------------------------------------------------------------------------------------
# (spp, half of the hits on each light): the yield is twice these.  staircase and veach-mis render enough samples for 10^4 hits on every light; the 24 added
# lamps of "lamps" are small and rarely the closest hit of their own shadow rays (39 .. 6 846 hits at 4 spp): 10^4 on the smallest would take a thousand samples
# per pixel, so that scene keeps 4 spp and its floors are what 4 spp yield.
LIGHT_FLOORS = {"staircase": (40, [72823, 24863, 6797, 77380, 71072, 5303]),
                "veach-mis": (6, [8090, 7686, 7396]),
                "lamps": (4, [2058, 465, 1426, 215, 189, 367, 1865, 154, 394, 612, 709, 118, 664, 20, 2940, 1572, 19, 127, 3423, 108, 711, 1120, 1024, 157, 360])}


@pytest.mark.parametrize("name", ["staircase", "veach-mis", "lamps"])
def test_a_hit_on_a_light_lies_in_that_lights_box(name):
    """Parity-mode shadow rays of a 64 x 36 render (the many-lights fixture: Scene.named("lamps")): where the oracle's closest hit carries the material of
    the light the ray was drawn for, the ray passes light_boxes[l] and NOT t < trt_leaf_floor(entry of that box).  Every light has its own floor of hits."""
    s = T.Scene.named("lamps", 64, 36, n=24) if name == "lamps" else T.Scene.named(name, 64, 36)
    seed = {"staircase": T.SEED_STAIRCASE, "veach-mis": T.SEED_BACK, "lamps": 0x11A7}[name]
    spp, floors = LIGHT_FLOORS[name]
    org, dirs, light = H.shadow_rays(s.flat, T.make_params(64, 36, spp, seed))
    alpha, _, boxes = H.scene_info(s.flat)
    f = s.flat.contents
    light_mat = np.array([f.lights[i].mat for i in range(f.n_lights)])
    t, tri, _ = O.trace(s.flat, org, dirs)
    on = (tri >= 0) & (s.arrays()["tri_mat"][np.maximum(tri, 0)] == light_mat[light])
    w = H.box_cases(boxes[light[on]], org[on], dirs[on])
    entry = w[:, 1].copy().view(np.float32)
    bad = ((w[:, 0] & 1) == 0) | (t[on] < H.leaf_floor(entry, alpha))
    per_light = np.bincount(light[on], minlength=f.n_lights)
    print(name, len(org), "shadow rays,", int(on.sum()), "hits on their light, per light", per_light.tolist())
    assert not bad.any(), [(light[on][i], org[on][i], dirs[on][i], t[on][i], entry[i], boxes[light[on][i]]) for i in np.nonzero(bad)[0][:8]]
    assert len(floors) == f.n_lights and (per_light >= np.array(floors)).all(), per_light.tolist()
    s.close()


# ---- e. the plane filter -----------------------------------------------------------------------------------------------------------------------------------
def _plane_queries(s):
    planes = raygen.box_planes(s.flat)
    axis = np.repeat(np.arange(3, dtype=np.int32), planes.shape[1])
    x = planes.reshape(-1).copy()
    zero = x == 0
    x[zero] = -x[zero]  # -0.0 asked for a +0.0 plane and the reverse
    return axis, x, int(zero.sum())


def _lbvh_scene(name):
    """A shipped scene with the tree of the GPU builder, from its restatement (lbvh_ref.build: node for node trt_build_lbvh's, test_gpu_lbvh_reference.py)."""
    import ctypes as C
    import os
    import lbvh_ref
    from tinyraytracing_amd._abi import BvhNode
    d = os.path.join(T.SCENES_DIR, name)
    s = T.Scene.load(os.path.join(d, name + ".xml"), os.path.join(d, name + ".obj"), os.path.join(d, name + ".mtl"), d, 64, 36)
    n = s.info["n_triangles"]
    v = np.empty(n * 9, np.float32)
    s._check(s._lib.trth_scene_vertices(s._h, v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
    raw, n_nodes, order, depth = lbvh_ref.build(v.reshape(n, 9), 2)
    nodes = (BvhNode * n_nodes).from_buffer_copy(raw)
    order = np.ascontiguousarray(order, np.uint32)
    s._check(s._lib.trth_scene_adopt_bvh(s._h, nodes, n_nodes, order.ctypes.data_as(C.POINTER(C.c_uint32)), depth))
    s._built = True
    return s


def _filter_trees():
    yield "staircase", T.Scene.named("staircase", 64, 36)
    yield "blob", T.Scene.named("blob", 64, 36, n=20000)
    yield "veach-mis@ref8", SU.load_with_reference_tree("veach-mis", 64, 36)
    yield "lbvh", _lbvh_scene("veach-mis")
    s = T.Scene.named("staircase", 64, 36)
    assert SU.renumber_nodes_reversed(s) > 0
    yield "renumbered", s
    s = T.Scene.named("veach-mis", 64, 36)
    s.set_vertices(RR.smooth_displace(s.arrays()["tri_v"], amp=0.4))
    yield "after set_vertices", s
    s = T.Scene.named("staircase", 64, 36)  # planes at +0.0 and -0.0 (the builders pad, so no shipped tree has one)
    for k in range(1, 9):
        s.flat.contents.nodes[k].lo0[k % 3] = 0.0 if k % 2 else -0.0
        s.flat.contents.nodes[k].hi1[(k + 1) % 3] = -0.0 if k % 2 else 0.0
    yield "zero planes", s


def test_the_plane_filter_never_answers_a_false_no():
    """planeMaybe on the filter planeFilterBuild makes is true for every lo and hi coordinate of every node (zeros asked with the other sign), on the loaders'
    trees, the reference's leaf-8 tree, an LBVH tree, a renumbered tree and a tree after Scene.set_vertices.  Printed only: the share of random coordinates
    that are no plane which the filter clears."""
    n_zero = n_all = 0
    for name, s in _filter_trees():
        bits, lg = H.plane_filter(s.flat)
        axis, x, nz = _plane_queries(s)
        maybe = H.plane_maybe(bits, lg, axis, x)
        assert maybe.all(), (name, [(int(axis[i]), x[i]) for i in np.nonzero(~maybe)[0][:8]])
        n_zero += nz
        n_all += len(x)
        rng = np.random.default_rng(2)
        lo, hi = raygen.scene_bounds(s)
        ra = rng.integers(0, 3, 200000).astype(np.int32)
        rx = (lo[ra] + (hi - lo)[ra] * rng.random(200000)).astype(np.float32)
        new = ~np.isin(rx, x)
        print(f"{name}: {len(x)} planes in 2^{lg} bits; clears {1.0 - H.plane_maybe(bits, lg, ra[new], rx[new]).mean():.3f} of {int(new.sum())} coordinates that are no plane")
        s.close()
    assert n_all >= 100000 and n_zero >= 4


def test_control_a_filter_with_one_word_cleared_answers_a_false_no():
    s = T.Scene.named("staircase", 64, 36)
    bits, lg = H.plane_filter(s.flat)
    axis, x, _ = _plane_queries(s)
    bad = bits.copy()
    bad[np.nonzero(bad)[0][0]] = 0
    assert not H.plane_maybe(bad, lg, axis, x).all()
    s.close()
