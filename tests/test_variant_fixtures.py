"""The fixtures of tests/test_gpu_variants.py, checked without a GPU: every scene lands in the k_shade<TABS, LIGHTS> cell it names
(expected_shade_tabs restates trt_create's rule), all 15 cells are reached, the caterpillar tree is 256 levels deep and walked alike by
the oracle and the hostsim, and the row-table, pixel-grid and light-count parameters sit exactly on the library's limits."""
import ctypes as C

import numpy as np
import pytest

import hostsim_lib as H
import oracle_lib as O
import scene_util as SU
import tinyraytracing_amd as T

TRT_EINVAL = 1


@pytest.mark.parametrize("cell", list(SU.SHADE_CELLS))
def test_fixture_lands_in_its_cell(cell, tmp_path):
    tabs, flavour, make = SU.SHADE_CELLS[cell]
    s = make(tmp_path)
    f = s.flat.contents
    assert SU.expected_shade_tabs(s) == tabs
    assert SU.shade_flavour(f.n_lights) == flavour
    cdf_bytes = 4 * f.n_light_tris
    table_bytes = ((96 * f.n_materials + 15) & ~15) + ((32 * f.n_lights + 15) & ~15)
    if "cdf_not_monotone" in cell:
        assert not SU.cdf_monotone(s) and table_bytes + cdf_bytes <= SU.SHADE_LDS_TABLE_BYTES  # the CDF would fit: its order alone drops it
    else:
        assert SU.cdf_monotone(s)
    if "cdf_too_large" in cell:
        assert table_bytes <= SU.SHADE_LDS_TABLE_BYTES < table_bytes + ((cdf_bytes + 15) & ~15)
    if tabs == 7:
        assert table_bytes + cdf_bytes + 80 * f.n_light_tris > SU.SHADE_LDS_TABLE_BYTES
    if "materials" in cell:
        assert f.n_materials > 256  # the materials alone exceed the budget


def test_all_fifteen_cells_reached():
    cells = {(tabs, flavour) for tabs, flavour, _ in SU.SHADE_CELLS.values()}
    assert cells == {(t, fl) for t in SU.SHADE_TABS for fl in ("one", "few", "many")}
    for fl in ("one", "few", "many"):  # TABS 3 both ways in every flavour
        assert {f"{fl}-3-cdf_too_large", f"{fl}-3-cdf_not_monotone"} <= set(SU.SHADE_CELLS)


@pytest.mark.parametrize("name,kw,tabs", [("back", {}, 31), ("soup", {"n": 1000}, 15), ("veach-mis", {}, 7), ("staircase", {}, 7),
                                          ("lamps", {"n": 8}, 31), ("lamps", {"n": 16}, 15), ("lamps", {"n": 64}, 7), ("lamps", {"n": 300}, 0)])
def test_expected_shade_tabs_on_the_shipped_scenes(name, kw, tabs):
    """The cells the suite covered before: the rule as restated puts them where the library does."""
    assert SU.expected_shade_tabs(T.Scene.named(name, 32, 18, **kw)) == tabs


def test_break_cdf_monotonicity_swaps_two_areas():
    s = T.Scene.named("back", 16, 16)
    f = s.flat.contents
    L = f.lights[0]
    before = [f.light_tris[k].cum_area for k in range(L.tri_first, L.tri_first + L.tri_count)]
    SU.break_cdf_monotonicity(s, 0)
    after = [f.light_tris[k].cum_area for k in range(L.tri_first, L.tri_first + L.tri_count)]
    assert after[:2] == before[1::-1] and after[2:] == before[2:]
    assert SU.expected_shade_tabs(s) == 3


# ---- the deepest tree

def test_caterpillar_256_levels_oracle_and_hostsim_agree():
    s = SU.caterpillar_scene(SU.MAX_BVH_DEPTH)
    f = s.flat.contents
    assert f.bvh_depth == SU.MAX_BVH_DEPTH and f.n_nodes == SU.MAX_BVH_DEPTH and f.n_tris == SU.MAX_BVH_DEPTH + 1
    for i in range(f.n_nodes):  # the chain: a leaf of triangle i, then node i + 1; boxes nested
        nd = f.nodes[i]
        assert nd.child0 == (0x80000000 | 1 << 27 | i)
        assert nd.child1 == (i + 1 if i + 1 < f.n_nodes else 0x80000000 | 1 << 27 | f.n_nodes)
        if i + 1 < f.n_nodes:
            kid = f.nodes[i + 1]
            for a in range(3):
                assert nd.lo1[a] <= min(kid.lo0[a], kid.lo1[a]) and nd.hi1[a] >= max(kid.hi0[a], kid.hi1[a])
    org, d = SU.axis_rays(s)
    t0, tri0, uv0 = O.trace(s.flat, org, d)
    assert (tri0 >= 0).sum() > len(tri0) // 4
    assert H.compressible(s.flat)
    for nk in (0, 1):
        old = H.set_node_kind(nk)
        try:
            t1, tri1, uv1, _ = H.trace(s.flat, org, d)
        finally:
            H.set_node_kind(old)
        assert np.array_equal(tri0, tri1) and np.array_equal(t0, t1) and np.array_equal(uv0, uv1), f"node kind {nk}"


def test_caterpillar_257_levels_refused_by_trt_create():
    """validateBvh runs before any device call: the refusal needs no GPU."""
    s = SU.caterpillar_scene(SU.MAX_BVH_DEPTH + 1)
    assert s.flat.contents.bvh_depth == SU.MAX_BVH_DEPTH + 1
    lib = T._abi.load_hip()
    h = C.c_void_p()
    assert lib.trt_create(s.flat, 0, C.byref(h)) == TRT_EINVAL and not h.value
    assert "deeper than 256 levels" in lib.trt_last_error().decode()


def test_65536_lights_refused_by_trt_create():
    flat, keep = SU.with_light_count(T.Scene.named("back", 16, 16), SU.MAX_SCENE_LIGHTS + 1)
    lib = T._abi.load_hip()
    h = C.c_void_p()
    assert lib.trt_create(C.byref(flat), 0, C.byref(h)) == TRT_EINVAL and not h.value
    msg = lib.trt_last_error().decode()
    assert "TRT_MAX_SCENE_LIGHTS" in msg and "65535" in msg
    del keep


# ---- the limits the GPU tests sit on

def rows_selected(p):
    """trt_rows_selected of the library (it makes no device call)."""
    return T._abi.load_hip().trt_rows_selected(C.byref(p))


@pytest.mark.parametrize("case", list(SU.ROW_CASES))
def test_row_cases_sit_on_the_limits(case):
    (name, kw), flavour, (w, h), tile, rows, want = SU.ROW_CASES[case]
    p = T.make_params(w, h, 2, 1, tile=tile, rows=rows)
    n = rows_selected(p)
    assert n == len(T.rows_selected(p))
    limit = SU.SHADE_ROWS_LDS[flavour]
    assert want == (n if n <= limit and h <= SU.GRID_MAX else 0)
    if want:
        assert n == limit  # exactly at the limit ...
    elif h <= SU.GRID_MAX:
        assert n == limit + 1  # ... or one past it
    else:
        assert n <= limit and tile[1] <= 65535 < tile[3] - 1  # rows off LDS for the height alone: the tile's rows straddle 16 bits
    if rows is not None:
        assert tile[3] - tile[1] > limit >= n  # a tile taller than the limit whose interleave selects no more than it


def test_row_cases_cover_every_flavour_both_sides():
    seen = {(fl, want > 0) for (_, fl, _, _, _, want) in SU.ROW_CASES.values()}
    assert seen == {(fl, b) for fl in ("one", "few", "many") for b in (True, False)}


@pytest.mark.parametrize("w,h", SU.GRID_SIZES)
def test_grid_cases_sit_on_the_limit(w, h):
    assert max(w, h) in (SU.GRID_MAX, SU.GRID_MAX + 1)
    x0, y0, x1, y1 = SU.grid_tile(w, h)
    assert (x0 > 49000 if w > h else y0 > 49000) and x1 <= w and y1 <= h and x1 - x0 == 24 and y1 - y0 == 12
    assert w * h <= 0xFFFFFFFF  # checkParams' bound
    assert rows_selected(T.make_params(w, h, 1, 1, tile=(x0, y0, x1, y1))) == 12


def test_light_counts_sit_on_the_limits():
    counts = SU.LIGHT_COUNTS
    assert {SU.shade_flavour(n) for n in counts} == {"few", "many"}
    assert SU.shade_flavour(2) == "few" and SU.shade_flavour(8) == "few" and SU.shade_flavour(9) == "many"
    assert SU.count_rows(13) == 16 < SU.count_rows(14)  # the counter-row layout changes between 13 and 14 lights
    assert [SU.publish_passes(n) for n in (511, 512, 1000)] == [1, 2, 2]  # k_publish_counts' block is capped at 1024 threads
    assert {2, 8, 9, 13, 14, 511, 512} <= set(counts)
