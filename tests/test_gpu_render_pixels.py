"""trt_render_pixels / trt_render_pixels_device (pixel lists with per-pixel moments) and Renderer.render_adaptive — MI355X only.

Bars, all bit-exact:
  - a list of every pixel of a tile, in tile order, over [0, spp) from zeros leaves trt_render_samples' accum in `sum`, and
    (float)sum is trt_render's image: every scene kind, traversal kind, the tail both ways, two passes in flight, several passes;
  - sparse lists: sum and sumsq equal a float64 numpy restatement from the oracle's per-sample radiance (oracle_lib.debug_path);
  - resumption, sample ranges past spp, the device entry, the refusals, and the adaptive loop (tinyraytracing_amd/adaptive.py).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 8
SEEDS = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE, "lamps": T.SEED_LAMPS}


def scene(name):
    return get_scene("lamps", W, H, n=17) if name == "lamps" else get_scene(name, W, H)  # lamps: 18 lights (k_shade's SHADE_MANY)


def fresh_renderer(s, env, monkeypatch):
    """A Renderer created under `env` (read at trt_create)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return T.Renderer(s, 0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def tile_pixels(p):
    ys = np.asarray(T.rows_selected(p), np.int64)
    xs = np.arange(p.x0, p.x1, dtype=np.int64)
    return (ys[:, None] * p.width + xs[None, :]).reshape(-1).astype(np.uint32)


class OracleMoments:
    """sum / sumsq of v = (double)(L_s / (float)spp) per list entry, restated in float64 from the oracle's per-sample radiance."""

    def __init__(self, s, p):
        self.flat, self.p, self.cache = s.flat, p, {}

    def L(self, q, k):
        if (q, k) not in self.cache:
            path = O.debug_path(self.flat, self.p, int(q % self.p.width), int(q // self.p.width), k, max_vertices=4096)
            self.cache[(q, k)] = path[-1, 4:7].astype(np.float32)
        return self.cache[(q, k)]

    def moments(self, pixels, s0, s1, sums=None, sumsq=None):
        n = len(pixels)
        su = np.zeros((n, 3)) if sums is None else sums.copy()
        sq = np.zeros((n, 3)) if sumsq is None else sumsq.copy()
        spp = np.float32(self.p.spp)
        for i, q in enumerate(pixels):
            for k in range(s0, s1):
                v = (self.L(int(q), k) / spp).astype(np.float64)
                su[i] += v
                sq[i] += v * v
        return su, sq


def assert_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    bad = a.view(np.uint64 if a.dtype == np.float64 else np.uint32) != b.view(np.uint64 if b.dtype == np.float64 else np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}: {a[tuple(np.argwhere(bad)[0])]} != {b[tuple(np.argwhere(bad)[0])]}"


# ---- 1. every pixel of the tile, in tile order: the bits of trt_render_samples / trt_render -------------------------------------
# traversal kinds as the parity suite selects them: back is a tiny tree (wave-uniform walk by default; TRT_TRACE_IMPL=3 puts it on
# the per-lane driver), the others take 4-wide (TRT_NODE_KIND=0) or 8-wide oct nodes (1)
KINDS = {"default": {}, "wide4": {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "0"}, "oct8": {"TRT_TRACE_IMPL": "3", "TRT_NODE_KIND": "1"}}
RUNS = ["plain", "no_tail", "overlap", "passes"]


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ["back", "veach-mis", "staircase", "lamps"])
def test_full_tile_equals_render_samples(name, kind, run, monkeypatch):
    s = scene(name)
    env = dict(KINDS[kind])
    if run == "no_tail":
        env["TRT_TAIL_N"] = "0"
    flags, budget = 0, 0
    if run == "overlap":
        flags = T.TRT_FLAG_OVERLAP
    if run == "passes":
        budget = W * H * 3 * (132 + 48 * s.info["n_lights"])  # three samples of every pixel per pass
    p = T.make_params(W, H, SPP, SEEDS[name], flags=flags, mem_budget=budget)
    r = fresh_renderer(s, env, monkeypatch)
    try:
        img, acc, st_ref = r.render_samples(p, 0, SPP)
        img2, _ = r.render(p)
        sums, sumsq, st = r.render_pixels(p, tile_pixels(p), 0, SPP)
    finally:
        r.close()
    assert_bits(img, img2, "render_samples vs render")
    assert_bits(sums, acc.reshape(-1, 3), f"{name}/{kind}/{run}: sum vs trt_render_samples' accum")
    assert_bits(sums.astype(np.float32).reshape(H, W, 3), img, f"{name}/{kind}/{run}: (float)sum vs trt_render")
    assert (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits, st.max_bounces) == \
        (st_ref.rays_camera, st_ref.rays_shadow, st_ref.rays_indirect, st_ref.shaded_hits, st_ref.max_bounces)
    assert st.rows_rendered == 0 and st_ref.rows_rendered == H
    assert st.passes == st_ref.passes
    if run == "passes":
        assert st.passes == 3
    if run == "no_tail":
        assert st.launches[T._abi.KERNEL_NAMES.index("tail")] == 0


def test_sub_tile_with_row_interleave_equals_render_samples(renderer_factory):
    """Every pixel of an offset, interleaved tile: the tile fields of p select the list here, trt_render_pixels itself ignores them."""
    s = scene("veach-mis")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["veach-mis"], tile=(5, 3, 50, 31), rows=(2, 3, 1))
    _, acc, _ = r.render_samples(p, 0, SPP)
    sums, _, _ = r.render_pixels(p, tile_pixels(p), 0, SPP)
    assert_bits(sums, acc.reshape(-1, 3), "interleaved sub-tile")


# ---- 2. sparse lists against the oracle, per sample ----------------------------------------------------------------------------
def make_list(kind, rng):
    allpix = np.arange(W * H, dtype=np.uint32)
    if kind == "random":
        return rng.permutation(allpix)[:300]
    if kind == "duplicates":
        base = rng.choice(allpix, 40, replace=False)
        return rng.permutation(np.concatenate([base, base[:25], base[:7], base[:7]])).astype(np.uint32)
    if kind == "corners":
        return np.array([0, W - 1, (H - 1) * W, H * W - 1], np.uint32)
    if kind == "miss":  # back at 16:9: the columns beside the box see nothing
        xs = np.r_[0:4, W - 4:W]
        return (np.arange(0, H, 5)[:, None] * W + xs[None, :]).reshape(-1).astype(np.uint32)
    if kind == "single":
        return np.array([17 * W + 31], np.uint32)
    if kind == "long":  # longer than a k_shade block (512 threads), not a multiple of 64
        return rng.choice(allpix, 611, replace=True).astype(np.uint32)
    raise ValueError(kind)


LISTS = ["random", "duplicates", "corners", "miss", "single", "long"]
MODES = {"parity": (0, 0), "fixed_nee": (T.TRT_FLAG_FIXED_NEE, 0), "fixed_pixels": (T.TRT_FLAG_FIXED_PIXELS, 0),
         "ray_offset": (T.TRT_FLAG_RAY_OFFSET, 0), "specular_ks": (T.TRT_FLAG_SPECULAR_KS, 0), "max_depth": (0, 3)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("lst", LISTS)
def test_sparse_list_matches_oracle_back(lst, mode, renderer_factory):
    s = scene("back")
    flags, depth = MODES[mode]
    p = T.make_params(W, H, SPP, SEEDS["back"], flags=flags, max_depth=depth)
    pix = make_list(lst, np.random.default_rng(7))
    sums, sumsq, st = renderer_factory(s).render_pixels(p, pix, 0, 6)
    want_s, want_q = OracleMoments(s, p).moments(pix, 0, 6)
    assert_bits(sums, want_s, f"{lst}/{mode}: sum")
    assert_bits(sumsq, want_q, f"{lst}/{mode}: sumsq")
    assert st.rays_camera == len(pix) * 6 and st.rows_rendered == 0
    if lst == "miss":
        assert not sums.any() and not sumsq.any()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["veach-mis", "staircase", "lamps"])
def test_sparse_list_matches_oracle(name, mode, renderer_factory):
    s = scene(name)
    flags, depth = MODES[mode]
    p = T.make_params(W, H, SPP, SEEDS[name], flags=flags, max_depth=depth)
    pix = make_list("long" if name == "veach-mis" else "random", np.random.default_rng(11))
    sums, sumsq, _ = renderer_factory(s).render_pixels(p, pix, 0, 4)
    want_s, want_q = OracleMoments(s, p).moments(pix, 0, 4)
    assert_bits(sums, want_s, f"{name}/{mode}: sum")
    assert_bits(sumsq, want_q, f"{name}/{mode}: sumsq")


@pytest.mark.parametrize("kind", ["no_tail", "overlap_passes"])
def test_sparse_list_through_queue_kernels_and_passes(kind, monkeypatch):
    """The k_shade path for every bounce (no tail), and two passes in flight over a budget that forces several."""
    s = scene("veach-mis")
    env = {"TRT_TAIL_N": "0"} if kind == "no_tail" else {}
    pix = make_list("long", np.random.default_rng(3))
    budget = len(pix) * 2 * (132 + 48 * s.info["n_lights"]) if kind == "overlap_passes" else 0
    p = T.make_params(W, H, SPP, SEEDS["veach-mis"], flags=T.TRT_FLAG_OVERLAP if kind == "overlap_passes" else 0, mem_budget=budget)
    r = fresh_renderer(s, env, monkeypatch)
    try:
        sums, sumsq, st = r.render_pixels(p, pix, 0, 7)
    finally:
        r.close()
    want_s, want_q = OracleMoments(s, p).moments(pix, 0, 7)
    assert_bits(sums, want_s, kind)
    assert_bits(sumsq, want_q, kind)
    if kind == "overlap_passes":
        assert st.passes >= 4


# ---- 3. resumption and ranges past spp ----------------------------------------------------------------------------------------
def test_resumption_and_samples_past_spp(renderer_factory):
    s = scene("staircase")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["staircase"])
    pix = make_list("random", np.random.default_rng(5))
    a_s, a_q, _ = r.render_pixels(p, pix, 0, 8)
    b_s, b_q, _ = r.render_pixels(p, pix, 0, 3)
    b_s, b_q, _ = r.render_pixels(p, pix, 3, 8, b_s, b_q)
    assert_bits(b_s, a_s, "[0,3) + [3,8) vs [0,8): sum")
    assert_bits(b_q, a_q, "[0,3) + [3,8) vs [0,8): sumsq")
    want_s, want_q = OracleMoments(s, p).moments(pix, 8, 13, a_s, a_q)
    c_s, c_q, _ = r.render_pixels(p, pix, 8, 13, a_s.copy(), a_q.copy())  # p.spp = 8 only scales the terms (the sums are in/out)
    assert_bits(c_s, want_s, "past spp: sum")
    assert_bits(c_q, want_q, "past spp: sumsq")


# ---- 4. the device entry ------------------------------------------------------------------------------------------------------
def test_device_entry_matches_host_entry(renderer_factory):
    import torch
    s = scene("lamps")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["lamps"], flags=T.TRT_FLAG_OVERLAP)
    pix = make_list("long", np.random.default_rng(9))
    h_s, h_q, h_st = r.render_pixels(p, pix, 0, 5)
    dev = torch.device("cuda", 0)
    t_pix = torch.from_numpy(pix.astype(np.int32)).to(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):  # the entry runs on torch's current stream
        d_s, d_q, d_st = r.render_pixels(p, t_pix, 0, 5)
    assert d_s.device == dev and d_s.dtype == torch.float64
    assert_bits(d_s.cpu().numpy(), h_s, "device sum")
    assert_bits(d_q.cpu().numpy(), h_q, "device sumsq")
    assert (d_st.rays_camera, d_st.rays_shadow, d_st.rays_indirect) == (h_st.rays_camera, h_st.rays_shadow, h_st.rays_indirect)
    # in/out: resume on the device from the host's sums
    e_s, e_q, _ = r.render_pixels(p, t_pix, 5, 8, torch.from_numpy(h_s).to(dev), torch.from_numpy(h_q).to(dev))
    f_s, f_q, _ = r.render_pixels(p, pix, 0, 8)
    assert_bits(e_s.cpu().numpy(), f_s, "device resume sum")
    assert_bits(e_q.cpu().numpy(), f_q, "device resume sumsq")


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(renderer_factory):
    import torch
    s = scene("back")
    r = renderer_factory(s)
    lib = r._lib
    p = T.make_params(W, H, SPP, SEEDS["back"])
    pix = make_list("random", np.random.default_rng(1))[:50]
    su, sq = np.zeros((50, 3)), np.zeros((50, 3))
    u32 = C.POINTER(C.c_uint32)
    dp = C.POINTER(C.c_double)
    ok_pix = pix.ctypes.data_as(u32)
    st = T.Stats()

    def call(n, pixels, b, e, sums, sumsq, params=p):
        return lib.trt_render_pixels(r._h, C.byref(params), n, pixels, b, e, sums, sumsq, C.byref(st))

    bad_pix = pix.copy()
    bad_pix[17] = W * H
    refusals = {
        "null pixels": call(50, None, 0, 2, su.ctypes.data_as(dp), sq.ctypes.data_as(dp)),
        "null sums": call(50, ok_pix, 0, 2, None, sq.ctypes.data_as(dp)),
        "pixel >= width*height": call(50, bad_pix.ctypes.data_as(u32), 0, 2, su.ctypes.data_as(dp), sq.ctypes.data_as(dp)),
        "begin < 0": call(50, ok_pix, -1, 2, su.ctypes.data_as(dp), sq.ctypes.data_as(dp)),
        "begin > end": call(50, ok_pix, 3, 2, su.ctypes.data_as(dp), sq.ctypes.data_as(dp)),
        # checked before the list is read or any memory is sized by it
        "path-id range": call(0x7FFF0001, ok_pix, 0, 1, su.ctypes.data_as(dp), sq.ctypes.data_as(dp)),
    }
    for what, rc in refusals.items():
        assert rc == 1, f"{what}: returned {rc}, not TRT_EINVAL"
    assert not su.any() and not sq.any(), "a refused call wrote the sums"
    dev = torch.device("cuda", 0)
    t_bad = torch.from_numpy(bad_pix.astype(np.int32)).to(dev)
    with pytest.raises(T.TrtError, match=r"\(1\).*width \* height"):
        r.render_pixels(p, t_bad, 0, 2)
    # no-ops: nothing listed, or an empty range
    assert call(0, None, 0, 4, None, None) == 0
    assert call(50, ok_pix, 3, 3, su.ctypes.data_as(dp), sq.ctypes.data_as(dp)) == 0 and not su.any()
    # the budget cannot hold one sample of every entry
    tight = T.make_params(W, H, SPP, SEEDS["back"], mem_budget=49 * 180)
    assert call(50, ok_pix, 0, 2, su.ctypes.data_as(dp), sq.ctypes.data_as(dp), tight) == 3
    # still renders right
    sums, sumsq, _ = r.render_pixels(p, pix, 0, 4)
    want_s, want_q = OracleMoments(s, p).moments(pix, 0, 4)
    assert_bits(sums, want_s, "after refusals: sum")
    assert_bits(sumsq, want_q, "after refusals: sumsq")
    img, _ = r.render(p)
    ref, _ = O.render(s.flat, p)
    assert_bits(img, ref, "after refusals: trt_render")


def test_sumsq_may_be_null(renderer_factory):
    s = scene("back")
    r = renderer_factory(s)
    p = T.make_params(W, H, SPP, SEEDS["back"])
    pix = make_list("long", np.random.default_rng(2))
    want, _, _ = r.render_pixels(p, pix, 0, 3)
    su = np.zeros((len(pix), 3))
    st = T.Stats()
    rc = r._lib.trt_render_pixels(r._h, C.byref(p), len(pix), pix.ctypes.data_as(C.POINTER(C.c_uint32)), 0, 3,
                                  su.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(st))
    assert rc == 0
    assert_bits(su, want, "sum without sumsq")


# ---- 6. the adaptive loop -----------------------------------------------------------------------------------------------------
AW, AH, MIN_SPP, MAX_SPP, BATCH, REL = 320, 180, 4, 64, 12, 0.2


def test_render_adaptive_on_back():
    s = get_scene("back", AW, AH)
    r = T.Renderer(s, 0)
    try:
        p = T.make_params(AW, AH, MAX_SPP, SEEDS["back"])
        res = r.render_adaptive(p, REL, MIN_SPP, MAX_SPP, BATCH)
        n = res.counts
        assert n.shape == (AH, AW) and res.image.shape == (AH, AW, 3)
        assert n.min() == MIN_SPP and n.max() == MAX_SPP
        assert set(np.unique(n)) <= set(range(MIN_SPP, MAX_SPP, BATCH)) | {MAX_SPP}
        # the miss region (columns beside the box) stops at min_spp, with error 0
        miss = np.zeros((AH, AW), bool)
        miss[:, :60] = miss[:, 262:] = True
        assert (n[miss] == MIN_SPP).all() and (res.image[miss] == 0).all() and (res.error[miss] == 0).all()
        # stopped pixels are below the threshold, unless they ran into max_spp
        assert ((res.error <= REL) | (n == MAX_SPP)).all()
        assert (res.error[n < MAX_SPP] <= REL).all()
        # every pixel holds exactly the samples [0, n_q) of its stream: the bits of one call over that range
        flat_n, flat_img = n.reshape(-1), res.image.reshape(-1, 3)
        allpix = np.arange(AW * AH, dtype=np.uint32)
        for k in np.unique(flat_n):
            sel = np.nonzero(flat_n == k)[0]
            su, _, _ = r.render_pixels(p, allpix[sel], 0, int(k))
            assert_bits(flat_img[sel], su * float(p.spp) / flat_n[sel][:, None], f"pixels with {k} samples")
        # ... and the oracle's, on a sample of pixels of every count
        om = OracleMoments(s, p)
        rng = np.random.default_rng(4)
        for k in np.unique(flat_n):
            sel = rng.choice(np.nonzero(flat_n == k)[0], min(12, int((flat_n == k).sum())), replace=False)
            want, _ = om.moments(allpix[sel], 0, int(k))
            assert_bits(flat_img[sel], want * float(p.spp) / flat_n[sel][:, None], f"oracle, {k} samples")
        # far fewer rays than a fixed max_spp render
        _, st_fixed = r.render(p)
        assert res.stats.rays < 0.6 * st_fixed.rays, (res.stats.rays, st_fixed.rays)
        assert res.stats.rays_camera == int(n.sum())
        # the device loop: same selection, same bits
        dres = r.render_adaptive(p, REL, MIN_SPP, MAX_SPP, BATCH, on_device=True)
        assert dres.image.is_cuda and dres.rounds == res.rounds
        assert (dres.counts.cpu().numpy() == n).all()
        assert_bits(dres.image.cpu().numpy(), res.image, "on_device image")
        assert_bits(dres.error.cpu().numpy(), res.error, "on_device error")
    finally:
        r.close()
