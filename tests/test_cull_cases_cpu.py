"""The preconditions of tests/cull_cases.py, without a GPU: every case has the status, the eight integers of TileDesc::cull and the culled share
that its entry states, every tile holds what its GPU test needs (culled and kept columns or rows on the right side of a table limit), and case
A's rays — the renderer's own, T.camera_rays — put zero direction components into band pixels outside the rectangle, in waves whose lane 0 is
culled.  These are conditions, not measurements: tests/test_gpu_primary_cull_edges.py can then never pass because a case degenerated."""
import numpy as np
import pytest

import cull_cases as CC
import cull_ref as CR
import tinyraytracing_amd as T

SHADE_CULL_COLS, SHADE_ROWS_LDS = 4096, 8192  # TRT_SHADE_CULL_COLS, shadeRowsLds(512) (trt_kernels.h)
FORMS = [(name, fixed) for name, c in CC.CASES.items() for fixed in (False, True) if c["v"][fixed] is not None]


@pytest.mark.parametrize("name,fixed", FORMS, ids=[f"{n}-{'fixed' if f else 'plain'}" for n, f in FORMS])
def test_status_bound_and_share(name, fixed):
    c = CC.CASES[name]
    s, p = CC.case(name, fixed)
    b = CC.bound_of(s, p)
    assert b["active"] == (c["status"] == CC.ACTIVE), b
    assert b["v"] == c["v"][fixed], b
    if not b["active"]:
        assert c["word"] in b["why"], b["why"]
        assert CC.debug_line(b) == "off: " + b["why"]
        return
    share = CR.culled_mask(b, p.width, p.height).mean()
    assert c["share"][0] <= share <= c["share"][1], share
    # what is culled is sound: the CPU build's sweep of every culled pixel under extreme and seeded jitters (tests/test_cull_cpu.py's)
    sw = CR.sweep(s.flat.contents.camera, p.width, p.height, fixed, CC.root_boxes(s), n_interior=8)
    assert sw["culled"] == int(round(share * p.width * p.height))
    for k in ("pass_clean", "pass_literal", "zero_component", "special"):
        assert sw[k] == 0, (k, sw)


@pytest.mark.parametrize("fixed", (False, True), ids=["plain", "fixed"])
def test_case_a_puts_zero_components_beside_culled_lanes(fixed):
    """Counts found (plain / fixed): 13 / 13 zero-component rays, 13 / 12 of them in pixels outside the rectangle (11 / 11 in column 48, the others in
    the band of rows); 5 / 5 waves with lane 0 culled; 1 / 1 with the ray at lane 0."""
    s, p = CC.case("bands", fixed)
    f = CC.facts(s, p)
    b = f["bound"]
    j_lo, j_hi, i_lo, i_hi = b["rect"]
    assert b["cols"][0] <= b["cols"][1] and (b["cols"][0] > j_hi or b["cols"][1] < j_lo), b  # the band of columns lies wholly outside the rectangle
    assert f["n_zero_outside"] >= 8, f["n_zero_outside"]  # in pixels that a band alone keeps
    for (y, x) in f["zero_pixels"]:
        assert b["cols"][0] <= x <= b["cols"][1] or b["rows"][0] <= y <= b["rows"][1], (y, x)
    assert f["zero_culled"] == 0
    assert f["waves_lane0_culled"] >= 2, f["waves_lane0_culled"]
    assert f["waves_zero_at_lane0"] >= 1, f["waves_zero_at_lane0"]
    assert f["n_waves"] == (p.width * p.height * p.spp + 63) // 64
    print(f"bands, {'fixed' if fixed else 'plain'}: {f['n_zero']} zero-component rays in {f['zero_pixels']}, {f['n_zero_outside']} outside the rectangle, {f['waves_lane0_culled']} waves with lane 0 culled, "
          f"{f['waves_zero_at_lane0']} with the ray at lane 0")


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_tiles_sit_on_the_right_side_of_the_table_limits(name):
    """A tile is culled in k_shade iff it has at most 4096 columns and at most 8192 table rows (renderCore); every tile holds culled and kept pixels,
    and culled ones on both sides of the kept ones."""
    routes = set()
    for tile, (_, want) in CC.CASES[name]["tiles"].items():
        s, p = CC.case(name, tile=tile)
        ys, xs = CC.tile_rows_cols(p)
        assert (CC.K_SHADE if xs.size <= SHADE_CULL_COLS and ys.size <= SHADE_ROWS_LDS else CC.RESOLVE) == want, tile
        routes.add(want)
        m = CC.tile_mask(CC.bound_of(s, p), p)
        line = m.any(axis=0) if name == "wide" else m.any(axis=1)  # per column / per row: holds a culled pixel
        kept = np.flatnonzero(~line)
        assert kept.size and line[:kept[0]].any() and line[kept[-1] + 1:].any(), tile
        assert m.mean() > 0.25, (tile, m.mean())
    assert routes == {CC.K_SHADE, CC.RESOLVE}
    sizes = {t: tuple(a.size for a in CC.tile_rows_cols(CC.case(name, tile=t)[1])) for t in CC.CASES[name]["tiles"]}
    if name == "wide":
        assert sorted(c for (_, c) in sizes.values()) == [4096, 4097, 4200]
        assert CC.case(name, tile="4096 wide at x0 = 100")[1].x0 == 100
    else:
        assert sorted(r for (r, _) in sizes.values()) == [4148, 8192, 8193, 8300]
        ys, _ = CC.tile_rows_cols(CC.case(name, tile="every other block of 8 rows")[1])
        assert ys.size < SHADE_ROWS_LDS < ys.max() and ys[0] != 0  # table rows are not image rows, and the image rows pass the table's size


def test_off_frame_keeps_only_the_bands():
    for fixed in (False, True):
        s, p = CC.case("off_frame", fixed)
        f = CC.facts(s, p)
        v = f["bound"]["v"]
        i, j = np.mgrid[0:p.height, 0:p.width]
        band = ((i >= v[4]) & (i < v[4] + v[5])) | ((j >= v[6]) & (j < v[6] + v[7]))
        assert v[5] > 0 and v[7] > 0 and np.array_equal(f["mask"], ~band)
        assert f["zero_culled"] == 0


def test_refit_positions():
    """The refit of the GPU file: with the box around case A's eye the bound is off because the eye is not in front of it; back at case A's place
    the vertices, and so the bound, are the first ones bit for bit."""
    w, h = CC.CASES["bands"]["size"]
    sc = CC.moved_back(w, h, CC.SHIFT_A)
    try:
        cam = CC.CASES["bands"]["camera"](w, h)
        v0 = sc.arrays()["tri_v"]
        b0 = CC.bound_of(CC.WithCamera(sc, cam), T.make_params(w, h, 1, 1))
        sc.set_vertices(CC.shifted_vertices(CC.SHIFT_AROUND_EYE))
        v1 = sc.arrays()["tri_v"]
        eye = np.array(list(cam.eye))
        assert (v1.reshape(-1, 3).min(axis=0) < eye).all() and (eye < v1.reshape(-1, 3).max(axis=0)).all()
        b1 = CC.bound_of(CC.WithCamera(sc, cam), T.make_params(w, h, 1, 1))
        assert not b1["active"] and "not in front" in b1["why"], b1
        sc.set_vertices(CC.shifted_vertices(CC.SHIFT_A))
        assert np.array_equal(sc.arrays()["tri_v"].view(np.uint32), v0.view(np.uint32))
        assert CC.bound_of(CC.WithCamera(sc, cam), T.make_params(w, h, 1, 1)) == b0 and b0["v"] == CC.CASES["bands"]["v"][0]
    finally:
        sc.close()
