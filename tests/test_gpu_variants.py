"""Every k_shade<TABS, LIGHTS> instantiation, the row table in LDS and in global memory, the pixel-grid fallback, the deepest tree the
library accepts and the light-count limits, each on the HIP path against the CPU oracle — MI355X only.

Every test reads which variant ran from the library's TRT_DEBUG lines (trt_create: k_shade tables ...; trt_render: k_shade ...,
rows in lds ..., grid_ok ...) and asserts it before it compares: a test that lands on another variant than the one it names fails.
Bar: bit-exact against the CPU oracle, ray counts equal, as in test_gpu_parity.py.  The fixtures are in scene_util.py; which cell
each lands in is checked without a GPU by test_variant_fixtures.py.
"""
import ctypes as C
import re
from dataclasses import dataclass

import numpy as np
import pytest

import oracle_lib as O
import scene_util as SU
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu
TOL = 0.0
TRT_EINVAL = 1


def assert_same_image(a, b, what=""):
    assert a.shape == b.shape, what
    assert np.isfinite(a).all(), what
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert d.max() <= TOL, f"{what}: max abs diff {d.max()} in {int((d.max(-1) > TOL).sum())} pixels"


def assert_same_counts(st, ost, what=""):
    got = (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits, st.max_bounces)
    want = (ost.rays_camera, ost.rays_shadow, ost.rays_indirect, ost.shaded_hits, ost.max_bounces)
    assert got == want, f"{what}: {got} != {want}"


@dataclass
class Variant:
    tabs: int          # k_shade<TABS>
    flavour: str       # k_shade<LIGHTS>: one / few / many
    rows_lds: int      # rows of the tile's row table kept in LDS (0: read from global memory)
    grid_ok: int       # the reciprocal pixel grid
    stack_need: int    # 4-wide traversal stack
    oct_levels: int    # levels of the oct tree (0: not built)


def parse_debug(err):
    tabs = re.findall(r"trt_create: k_shade tables (\d+) \(", err)
    render = re.findall(r"trt_render: k_shade (one|few|many), rows in lds (\d+), grid_ok (\d+)", err)
    stack = re.findall(r"trt_create: \d+ wide nodes, node kind \d, stack need (\d+)", err)
    octl = re.findall(r"trt_create: oct tree built \(.*\): \d+ nodes, (\d+) levels", err)
    assert len(tabs) == 1 and len(stack) == 1, f"expected one trt_create: k_shade tables line:\n{err}"
    assert len(render) <= 1, f"one trt_render line per render call:\n{err}"
    fl, rl, g = render[0] if render else ("", "-1", "-1")
    return Variant(int(tabs[0]), fl, int(rl), int(g), int(stack[0]), int(octl[0]) if octl else 0)


def render_variant(scene, p, capfd, monkeypatch, env=None):
    """A Renderer created with TRT_DEBUG (and `env`) set, one render, closed again: (image, stats, Variant)."""
    env = dict(env or {}, TRT_DEBUG="1")
    capfd.readouterr()
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        r = T.Renderer(scene, 0)
    try:
        img, st = r.render(p)
    finally:
        r.close()
    return img, st, parse_debug(capfd.readouterr().err)


def check_render(scene, p, capfd, monkeypatch, env, tabs, flavour, what, rows_lds=None, grid_ok=1):
    img, st, v = render_variant(scene, p, capfd, monkeypatch, env)
    assert (v.tabs, v.flavour) == (tabs, flavour), f"{what}: landed on k_shade<{v.tabs}, {v.flavour}>"
    assert v.tabs == SU.expected_shade_tabs(scene), f"{what}: the library and expected_shade_tabs disagree"
    assert v.grid_ok == grid_ok, what
    if rows_lds is not None:
        assert v.rows_lds == rows_lds, f"{what}: rows in lds {v.rows_lds}, wanted {rows_lds}"
    ref, ost = O.render(scene.flat, p)
    assert_same_image(img, ref, what)
    assert_same_counts(st, ost, what)
    assert st.rays_shadow > 0, what
    if env.get("TRT_TAIL_N") == "0":
        assert st.launches[T.KERNEL_NAMES.index("tail")] == 0, what
    return img, st, v


# ---- 1. the k_shade matrix: 5 table sets x 3 light flavours, natural scenes; TABS 3 both ways (CDF too large / not monotone)

@pytest.mark.parametrize("flags", [0, T.TRT_FLAG_FIXED_NEE], ids=["parity", "fixed_nee"])
@pytest.mark.parametrize("cell", list(SU.SHADE_CELLS))
def test_k_shade_cell_matches_oracle(cell, flags, tmp_path, capfd, monkeypatch):
    tabs, flavour, make = SU.SHADE_CELLS[cell]
    s = make(tmp_path)
    f = s.flat.contents
    p = T.make_params(s.info["width"], s.info["height"], 4 if f.n_lights <= 64 else 2, 0x5AD3 + tabs, flags=flags)
    check_render(s, p, capfd, monkeypatch, {"TRT_TAIL_N": "0"}, tabs, flavour, f"{cell} flags {flags}")


@pytest.mark.parametrize("cell", ["one-3-cdf_too_large", "few-0-materials", "many-7-lamps"])
def test_k_shade_flavour_with_default_tail(cell, tmp_path, capfd, monkeypatch):
    """The default tail_n: k_shade takes bounce 0 and k_tail the rest."""
    tabs, flavour, make = SU.SHADE_CELLS[cell]
    s = make(tmp_path)
    p = T.make_params(s.info["width"], s.info["height"], 4, 0x7A1, flags=T.TRT_FLAG_FIXED_NEE)
    _, st, _ = check_render(s, p, capfd, monkeypatch, {}, tabs, flavour, f"{cell}, default tail")
    assert st.launches[T.KERNEL_NAMES.index("tail")] >= 1


# ---- 2. the row table: in LDS up to shadeRowsLds(block) selected rows and an image height of 65536, else from global memory

@pytest.mark.parametrize("case", list(SU.ROW_CASES))
def test_row_table_lds_or_global(case, capfd, monkeypatch):
    (name, kw), flavour, (w, h), tile, rows, want = SU.ROW_CASES[case]
    s = get_scene(name, 64, 36, **kw)
    p = T.make_params(w, h, 2, 0x1207, tile=tile, rows=rows)
    n_rows = len(T.rows_selected(p))
    assert want in (0, n_rows)
    check_render(s, p, capfd, monkeypatch, {"TRT_TAIL_N": "0"}, SU.expected_shade_tabs(s), flavour, case, rows_lds=want,
                 grid_ok=int(h <= SU.GRID_MAX))


# ---- 3. the pixel grid: the proven reciprocals up to 65536 pixels a side, the fallback beyond; small tiles at the far edge

@pytest.mark.parametrize("flags", [0, T.TRT_FLAG_FIXED_PIXELS], ids=["jittered", "fixed_pixels"])
@pytest.mark.parametrize("w,h", SU.GRID_SIZES)
def test_pixel_grid_at_the_limit(w, h, flags, capfd, monkeypatch):
    s = get_scene("lamps", 64, 36, n=3)
    tile = SU.grid_tile(w, h)
    p = T.make_params(w, h, 4, 0x6A1D, tile=tile, flags=flags)
    ok = int(w <= SU.GRID_MAX and h <= SU.GRID_MAX)
    check_render(s, p, capfd, monkeypatch, {"TRT_TAIL_N": "0"}, 31, "few", f"{w}x{h}", rows_lds=12 if h <= SU.GRID_MAX else 0, grid_ok=ok)


# ---- 4. the deepest tree: a 256-level caterpillar on both node kinds (4-wide stack and oct levels beyond LDS, the BVH2 walk)

@pytest.fixture(scope="module")
def caterpillar():
    return SU.caterpillar_scene(SU.MAX_BVH_DEPTH)


@pytest.mark.parametrize("nk", ["0", "1"])
def test_caterpillar_trace_matches_oracle(nk, caterpillar, capfd, monkeypatch):
    s = caterpillar
    assert s.flat.contents.bvh_depth == SU.MAX_BVH_DEPTH
    capfd.readouterr()
    with monkeypatch.context() as m:
        m.setenv("TRT_DEBUG", "1")
        m.setenv("TRT_NODE_KIND", nk)
        r = T.Renderer(s, 0)
    try:
        org, d = SU.axis_rays(s)
        t1, tri1, uv1, st = r.trace_closest(org, d, want_stats=True)
    finally:
        r.close()
    v = parse_debug(capfd.readouterr().err)
    assert v.stack_need > 16  # beyond the LDS stack of the 4-wide kernels (TRT_LDS_STACK_MAX_LEVELS): the spill area is walked
    if nk == "1":
        assert v.oct_levels > 10 and st.inner_node_bytes == 80  # beyond OCT_LDS_LEVELS
    else:
        assert v.oct_levels == 0 and st.inner_node_bytes == 128
    t0, tri0, uv0 = O.trace(s.flat, org, d)
    assert (tri0 >= 0).sum() > len(tri0) // 4
    assert np.array_equal(tri0, tri1) and np.array_equal(t0, t1) and np.array_equal(uv0, uv1)


@pytest.mark.parametrize("nk", ["0", "1"])
def test_caterpillar_render_matches_oracle(nk, caterpillar, capfd, monkeypatch):
    p = T.make_params(48, 32, 4, 0xCA7)
    img, st, v = render_variant(caterpillar, p, capfd, monkeypatch, {"TRT_NODE_KIND": nk})
    assert v.flavour == "one" and v.stack_need > 16 and (v.oct_levels > 10) == (nk == "1")
    assert st.launches[T.KERNEL_NAMES.index("tail")] >= 1  # the default tail: k_tail walks the BVH2 for the raySpecial rays
    ref, ost = O.render(caterpillar.flat, p)
    assert_same_image(img, ref, f"caterpillar, node kind {nk}")
    assert_same_counts(st, ost, f"caterpillar, node kind {nk}")


def test_caterpillar_257_levels_refused():
    s = SU.caterpillar_scene(SU.MAX_BVH_DEPTH + 1)
    lib = T._abi.load_hip()
    h = C.c_void_p()
    assert lib.trt_create(s.flat, 0, C.byref(h)) == TRT_EINVAL and not h.value
    assert "deeper than 256 levels" in lib.trt_last_error().decode()


# ---- 5. light counts: the FEW ends, the counter-row layout, the publish loop, the bound and the refusal beyond it

@pytest.mark.parametrize("n_lights", SU.LIGHT_COUNTS)
def test_light_count_boundaries(n_lights, capfd, monkeypatch):
    small = n_lights <= 64
    s = get_scene("lamps", 64 if small else 32, 36 if small else 18, n=n_lights - 1)
    assert s.info["n_lights"] == n_lights
    p = T.make_params(64 if small else 32, 36 if small else 18, 4 if small else 2, 0x11C + n_lights)
    flavour = SU.shade_flavour(n_lights)
    check_render(s, p, capfd, monkeypatch, {"TRT_TAIL_N": "0"}, SU.expected_shade_tabs(s), flavour, f"{n_lights} lights")
    assert SU.publish_passes(n_lights) == (2 if n_lights >= 512 else 1)


def test_65535_lights_tiny_image(capfd, monkeypatch):
    """TRT_MAX_SCENE_LIGHTS lights, one pixel of the lit floor at 1 spp and one vertex (max_depth 1): one shadow launch and one
    k_trace_fix per light.  One pixel, because the oracle walks every box a shadow ray passes: among 65 534 lamps that is about half a
    millisecond per ray, some 30 s for this pixel's 29 000 shadow rays (a 2x2 tile through every bounce takes minutes).
    Measured on an MI355X: 25 s for this test, oracle included."""
    s = get_scene("lamps", 64, 36, n=SU.MAX_SCENE_LIGHTS - 1)
    assert s.info["n_lights"] == SU.MAX_SCENE_LIGHTS
    p = T.make_params(64, 36, 1, 0xFFFF, tile=(31, 17, 32, 18), max_depth=1)
    check_render(s, p, capfd, monkeypatch, {"TRT_TAIL_N": "0"}, SU.expected_shade_tabs(s), "many", "65535 lights")


def test_65536_lights_refused():
    flat, keep = SU.with_light_count(get_scene("back", 16, 16), SU.MAX_SCENE_LIGHTS + 1)
    lib = T._abi.load_hip()
    h = C.c_void_p()
    assert lib.trt_create(C.byref(flat), 0, C.byref(h)) == TRT_EINVAL and not h.value
    msg = lib.trt_last_error().decode()
    assert "TRT_MAX_SCENE_LIGHTS" in msg and "65535" in msg
    del keep
