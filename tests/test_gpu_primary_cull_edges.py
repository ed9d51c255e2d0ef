"""The camera-ray cull on the GPU where tests/test_gpu_primary_cull.py does not reach (trt_cull.h; k_shade's fused bounce 0, k_resolve_tile;
renderCore's choice between the two) — MI355X only.  The cases are tests/cull_cases.py's, and tests/test_cull_cases_cpu.py has held each to
what it states.  Every render is the oracle's bit for bit with the oracle's counters; the four handles of the existing file (default,
TRT_CULL_PRIMARY=0, TRT_FUSE_PRIMARY=0, TRT_TAIL_N=64) agree in every counter, redo_rays included; and the two TRT_DEBUG lines of every call
— the bound, and `trt_render: cull in k_shade N`, the route — are the CPU build's bound for the case and the route the case states.

The branches held here, and the fault each test would catch:
  1. the guard bands where they decide (test_bands; test_entries' -0.0): a k_shade that ignored bit 1 of s_colcls / s_rowcls would not walk
     the band pixels outside the rectangle and so count fewer redo_rays than the handles that do not cull; a resolve that ignored the bands
     would leave a caller's -0.0 in a band pixel
  2. fusedPrimaryHit's electing lane with culled lanes in the wave (test_bands): a wrong lane loses or doubles redo_rays
  3. the limits of s_colcls and s_rowcls (test_table_limits): 4096 / 4097 columns, x0 > 0, 8192 / 8193 rows, a row table that is not the identity
  4. the degenerate bounds (test_degenerate_bounds): everything outside, nothing outside, the off reasons a render can reach
  5. the other entries of the tile route (test_entries, test_refit_around_the_eye_and_back): render_samples onto a caller's sums, render_into on
     a side stream, TRT_FLAG_FIXED_PIXELS (test_bands, test_degenerate_bounds), a geometry update that turns culling off and on again"""
import re
from contextlib import contextmanager

import numpy as np
import pytest

import cull_cases as CC
import oracle_lib as O
import tinyraytracing_amd as T
from test_gpu_fused_primary import ORACLE_FIELDS, WithCamera, bits
from test_gpu_primary_cull import HANDLES, cull_lines, make, stats_of

pytestmark = pytest.mark.gpu

OFF_LINE = "off: TRT_CULL_PRIMARY=0"


class _Kept:
    """capfd for cull_lines(), which keeps what was read for the second line"""

    def __init__(self, capfd):
        self.capfd, self.err = capfd, ""

    def readouterr(self):
        r = self.capfd.readouterr()
        self.err = r.err
        return r


def lines(capfd):
    """-> (the bounds, the routes) of the tile renders since the last look"""
    k = _Kept(capfd)
    cull = cull_lines(k)
    return cull, [int(x) for x in re.findall(r"trt_render: cull in k_shade (\d)", k.err)]


@contextmanager
def handles(s, capfd, monkeypatch, envs=HANDLES):
    rs = []
    try:
        for env in envs:
            rs.append(make(s, env, capfd, monkeypatch))
        yield rs
    finally:
        for r in rs:
            r.close()


def expected(env, line, route):
    """The two lines of a handle created with env for a call whose bound prints `line` and whose tile takes `route` on a handle that culls and fuses"""
    if "TRT_CULL_PRIMARY" in env:
        return [OFF_LINE], [CC.RESOLVE]
    return [line], [CC.RESOLVE if "TRT_FUSE_PRIMARY" in env else route]


def held(rs, s, p, route, capfd, what, envs=HANDLES):
    """Renders p on every handle: the oracle's image and counters, one set of counters, the two lines.  -> (image, Stats, the bound)"""
    b = CC.bound_of(s, p)
    line = CC.debug_line(b)
    ref, ost = O.render(s.flat, p)
    first = None
    for env, r in zip(envs, rs):
        capfd.readouterr()
        img, st = r.render(p)
        assert lines(capfd) == expected(env, line, route), (what, env)
        assert np.array_equal(bits(img), bits(ref)), (what, env, float(np.abs(img - ref).max()))
        assert stats_of(st, ORACLE_FIELDS) == stats_of(ost, ORACLE_FIELDS), (what, env)
        first = first or stats_of(st)
        assert stats_of(st) == first, (what, env)
    assert st.rays_camera == len(T.rows_selected(p)) * (p.x1 - p.x0) * p.spp
    return img, st, b


@pytest.mark.parametrize("fixed", (False, True), ids=["plain", "fixed"])
def test_bands(fixed, capfd, monkeypatch):
    """Case A, both grid forms: the band of columns lies in the culled strip and holds every camera ray with d.x == 0 (13 zero-component rays
    at 16 spp, 5 waves with such a ray and a culled lane 0, 1 wave with the ray at lane 0: tests/cull_cases.py).
      - A k_shade that dropped the band test (bit 1 of the two classes, the `!= 1u`) would cull column 48 outside the rectangle.  Those pixels
        see nothing — the box is inside the rectangle — so the image could not tell; their zero-component rays would go uncounted, and redo_rays
        would fall below TRT_CULL_PRIMARY=0's and TRT_FUSE_PRIMARY=0's, which walk every camera ray.
      - An electing lane that is wrong when lane 0 is culled or absent loses the wave's redo_rays (no lane issues the atomic) or doubles them
        (two do) against the same two handles; at least the CPU count of zero-component camera rays must be there.
    A tile inside the rectangle is rendered first, with as many paths as the frame has (47 spp), so that the pass memory of the frame's culled
    paths holds what other paths left there: a k_shade that culled a pixel the resolve reads shows against the oracle as well."""
    s, p = CC.case("bands", fixed)
    f = CC.facts(s, p)
    b = f["bound"]
    assert f["n_zero_outside"] >= 8 and f["waves_lane0_culled"] >= 2 and f["waves_zero_at_lane0"] >= 1 and f["zero_culled"] == 0
    j_lo, j_hi, i_lo, i_hi = b["rect"]
    n_in, n_frame = (j_hi + 1 - j_lo) * (i_hi + 1 - i_lo), p.width * p.height * p.spp
    p_in = T.make_params(p.width, p.height, -(-n_frame // n_in), 0x57A1E, tile=(j_lo, i_lo, j_hi + 1, i_hi + 1), flags=p.flags)
    assert n_frame <= n_in * p_in.spp < 1.05 * n_frame  # no fewer paths than the frame has: the frame's pass lives in the memory this one filled
    with handles(s, capfd, monkeypatch) as rs:
        img, _, _ = held(rs, s, p_in, CC.K_SHADE, capfd, "the tile inside")
        assert (img.reshape(-1, 3).max(axis=1) > 0).mean() > 0.5
        img, st, _ = held(rs, s, p, CC.route("bands"), capfd, "the frame")
    assert st.redo_rays >= f["n_zero"], (st.redo_rays, f["n_zero"])
    lit = img.reshape(p.height, p.width, 3).max(axis=2) > 0
    assert lit.any() and not lit[f["mask"]].any()


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_table_limits(name, capfd, monkeypatch):
    """Case B at 2 spp: s_colcls has TRT_SHADE_CULL_COLS = 4096 entries and s_rowcls shadeRowsLds(512) = 8192; renderCore hands k_shade the bound
    only for tiles within both, and culls wider or taller ones in the resolve alone.
      wide   the 4200-wide frame and a 4097-wide tile: the resolve only; a 4096-wide tile at x0 = 100: k_shade, whose table is indexed by the
             tile's column and classed by the image's (x0 + column) — a kernel that mixed the two culls the box or keeps the strip
      tall   8300 and 8193 rows: the resolve only; 8192 rows at y0 = 50 and every other block of 8 rows of the whole image (4148 table rows whose
             image rows reach 8299): k_shade, whose table is indexed by the table's row and classed by the image's (td.rows[r])
    A route taken on the wrong side of a limit shows in the second line; a table read past its end or by the wrong index shows against the oracle."""
    s0, _ = CC.case(name)
    with handles(s0, capfd, monkeypatch) as rs:
        for tile in CC.CASES[name]["tiles"]:
            s, p = CC.case(name, tile=tile)
            img, st, b = held(rs, s, p, CC.route(name, tile), capfd, (name, tile))
            m = CC.tile_mask(b, p)
            lit = img.max(axis=2) > 0
            assert lit.any() and not lit[m].any() and 0.25 < m.mean() < 0.75, (name, tile)


@pytest.mark.parametrize("fixed", (False, True), ids=["plain", "fixed"])
def test_degenerate_bounds(fixed, capfd, monkeypatch):
    """Case C.  Everything outside (the boxes lie off the frame: v = [W, 0, H, 0, ...], only band pixels are walked): the image is +0.0 in every
    bit — the resolve leaves culled pixels alone, so this is the cleared sums' zero and the band pixels' +0.0 — nothing is shaded and every
    camera ray is counted, as without the switch: a kernel or a resolve that mishandled the empty rectangle (j_lo = W > j_hi) would walk or
    write something else.  Nothing outside (an active bound whose v[0:4] are zero): renderCore keeps the kernels it ran, k_shade does not
    cull.  Off, for the two reasons a render can reach (the eye inside the box, a slanted zero set): the line names the CPU build's reason
    and the images are the oracle's."""
    s, p = CC.case("off_frame", fixed)
    with handles(s, capfd, monkeypatch) as rs:
        img, st, b = held(rs, s, p, CC.route("off_frame"), capfd, "off frame")
    assert b["active"] and b["v"][:4] == [p.width, 0, p.height, 0]
    assert not bits(img).any() and st.shaded_hits == 0 and st.rays_camera == p.width * p.height * p.spp
    for name in ("nothing_outside", "eye_inside", "slanted"):
        if fixed and CC.CASES[name]["v"][1] is None:
            continue
        s, p = CC.case(name, fixed)
        with handles(s, capfd, monkeypatch) as rs:
            img, st, b = held(rs, s, p, CC.RESOLVE, capfd, name)
        assert b["active"] == (name == "nothing_outside") and b["v"][:4] == [0, 0, 0, 0]
        if not b["active"]:
            assert CC.CASES[name]["word"] in CC.debug_line(b)
        assert st.shaded_hits > 0 and (img.max(axis=2) > 0).any(), name


def test_entries(capfd, monkeypatch):
    """The other entries that take the tile route, on case A's scene at 4 spp, culling handle against TRT_CULL_PRIMARY=0.
      - render_samples over [0, 1), [1, 4) leaves one render's sums and image, the off handle's: k_resolve_tile adds onto the sums of earlier calls
      - onto a caller's accum with finite non-zero sums everywhere: a culled pixel keeps what it held, as adding +0.0 keeps it on the off handle
      - a caller's -0.0: kept in a culled pixel (the off handle returns +0.0, the one difference k_resolve_tile's comment admits, include/trt.h),
        turned into +0.0 in a band pixel outside the rectangle on both handles — a resolve that ignored the bands would leave it
      - render_into on a side stream: render's image, a sentinel behind the image untouched
      - render_pixels, render_adaptive and render_camera cull nothing and print neither line: the off handle's results"""
    import torch
    s, p = CC.case("bands", spp=4, seed=0xE47)
    b = CC.bound_of(s, p)
    line, route = CC.debug_line(b), CC.route("bands")
    mask = CC.tile_mask(b, p)
    shape = (p.height, p.width, 3)
    culled_px = tuple(np.argwhere(mask)[0])
    band_px = (0, b["cols"][0])  # in the band of columns, above the rectangle
    assert b["rect"][2] > 0 and not mask[band_px] and not (b["rect"][0] <= band_px[1] <= b["rect"][1])
    envs = HANDLES[:2]
    with handles(s, capfd, monkeypatch, envs) as (r, r_off):
        capfd.readouterr()
        whole, st = r.render(p)
        assert lines(capfd) == ([line], [route])
        assert np.array_equal(bits(whole), bits(O.render(s.flat, p)[0]))
        got = []
        for env, h in zip(envs, (r, r_off)):
            # from zeros, in two chunks
            capfd.readouterr()
            _, acc, st0 = h.render_samples(p, 0, 1)
            img, acc, st1 = h.render_samples(p, 1, 4, acc)
            want = expected(env, line, route)
            assert lines(capfd) == (want[0] * 2, want[1] * 2), env
            assert np.array_equal(bits(img), bits(whole)), env
            assert st0.rays_camera + st1.rays_camera == st.rays_camera and st0.shaded_hits + st1.shaded_hits == st.shaded_hits
            # onto sums of the caller's: k / 1024 + 1/4, exact in binary64 and nowhere zero
            mine = (np.arange(mask.size * 3, dtype=np.float64) / 1024.0 + 0.25).reshape(shape)
            img_m, acc_m, _ = h.render_samples(p, 0, 4, mine.copy())
            assert np.array_equal(bits(acc_m[mask]), bits(mine[mask])), env
            assert not np.array_equal(bits(acc_m[~mask]), bits(mine[~mask]))
            # a -0.0 in a culled pixel and in a band pixel outside the rectangle
            neg = np.zeros(shape, np.float64)
            neg[culled_px] = -0.0
            neg[band_px] = -0.0
            assert np.signbit(neg[culled_px]).all() and np.signbit(neg[band_px]).all()
            _, acc_n, _ = h.render_samples(p, 0, 4, neg)
            got.append((acc, acc_m, img_m, acc_n))
            assert not np.signbit(acc_n[band_px]).any() and not acc_n[band_px].any(), env
            assert np.signbit(acc_n[culled_px]).all() == ("TRT_CULL_PRIMARY" not in env) and not acc_n[culled_px].any(), env
        on, off = got
        for a, c in zip(on[:3], off[:3]):
            assert np.array_equal(bits(a), bits(c))
        differ = bits(on[3]) != bits(off[3])
        assert differ[culled_px].all() and int(differ.sum()) == 3  # the -0.0 of the one culled pixel and nothing else

        # the device entry on a side stream
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        n, sentinel = mask.size * 3, -7.0
        out = torch.full((n + 256,), sentinel, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        capfd.readouterr()
        r.render_into(p, out, stream_ptr=side.cuda_stream)
        assert lines(capfd) == ([line], [route])
        host = out.cpu().numpy()
        assert np.array_equal(bits(host[:n].reshape(shape)), bits(whole)) and (host[n:] == sentinel).all()

        # pixel lists and caller-supplied rays: no cull, no line
        pix = np.arange(mask.size, dtype=np.uint32)[::-1].copy()
        res = []
        for h in (r, r_off):
            capfd.readouterr()
            sums, sumsq, _ = h.render_pixels(p, pix, 0, p.spp)
            ad = h.render_adaptive(p, 0.3, 2, 6, 2)
            cam_img, cst = h.render_camera(p, s.flat.contents.camera, samples_per_call=2, want_stats=True)
            err = capfd.readouterr().err
            assert "trt_render_pixels: fused primary 0" in err and "trt_render_rays: fused primary 0" in err  # (the calls did print their own lines)
            assert "cull primary" not in err and "cull in k_shade" not in err
            res.append((sums, sumsq, ad.image, ad.counts, cam_img, stats_of(cst)))
        for a, c in zip(*res):
            assert np.array_equal(bits(a), bits(c)) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else np.array_equal(a, c)
        assert np.array_equal(bits(res[0][4]), bits(whole))  # render_camera's contract
        assert np.array_equal(bits(res[0][0][::-1].astype(np.float32).reshape(shape)), bits(whole))


def test_refit_around_the_eye_and_back(capfd, monkeypatch):
    """From case A's handle, trt_update_geometry to vertices that put the box around the eye: the bound comes from the root node the update reads
    back, so culling must switch off (`not in front`) — a handle that kept the first rectangle would cull the walls the eye now looks at — and
    the image is a fresh handle's and the oracle's.  Then back to case A's place: the first rectangle again and the first image's bits."""
    c = CC.CASES["bands"]
    w, h = c["size"]
    p = T.make_params(w, h, 4, 0x2EF17)
    cam = c["camera"](w, h)
    scene = CC.moved_back(w, h, CC.SHIFT_A)
    try:
        s = WithCamera(scene, cam)
        b0 = CC.bound_of(s, p)
        assert b0["active"] and b0["v"] == c["v"][0]
        with handles(s, capfd, monkeypatch, HANDLES[:1]) as (r,):
            capfd.readouterr()
            img0, st0 = r.render(p)
            assert lines(capfd) == ([CC.debug_line(b0)], [CC.K_SHADE])
            assert np.array_equal(bits(img0), bits(O.render(s.flat, p)[0]))

            scene.set_vertices(CC.shifted_vertices(CC.SHIFT_AROUND_EYE))
            around = WithCamera(scene, cam)
            b1 = CC.bound_of(around, p)
            assert not b1["active"] and "not in front" in b1["why"]
            r.update_geometry(scene)
            capfd.readouterr()
            img1, st1 = r.render(p)
            assert lines(capfd) == ([CC.debug_line(b1)], [CC.RESOLVE])
            ref1, ost1 = O.render(around.flat, p)
            assert np.array_equal(bits(img1), bits(ref1)) and stats_of(st1, ORACLE_FIELDS) == stats_of(ost1, ORACLE_FIELDS)
            assert (img1.max(axis=2) > 0).mean() > 0.5 and (img1[:, :b0["v"][0]].max(axis=2) > 0).any()  # the eye is in the room: what was culled is lit now
            with handles(around, capfd, monkeypatch, HANDLES[:1]) as (fresh,):
                capfd.readouterr()
                img2, st2 = fresh.render(p)
                assert lines(capfd) == ([CC.debug_line(b1)], [CC.RESOLVE])
            assert np.array_equal(bits(img1), bits(img2)) and stats_of(st1) == stats_of(st2)

            scene.set_vertices(CC.shifted_vertices(CC.SHIFT_A))
            r.update_geometry(scene)
            capfd.readouterr()
            img3, st3 = r.render(p)
            assert lines(capfd) == ([CC.debug_line(b0)], [CC.K_SHADE])
            assert np.array_equal(bits(img3), bits(img0)) and stats_of(st3) == stats_of(st0)
    finally:
        scene.close()
