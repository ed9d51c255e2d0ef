"""Full-size passes against the oracle — MI355X only.

The parity tests render small passes; the benchmark times passes of hundreds of millions of paths.  Past 2^28 paths a 16-B queue
record lies beyond 4 GiB, past 2^30 so does the 4-B redo list, and past 2^24 pixels the resolve loops go round more than once: an
offset computed in 32 bits anywhere there passes every small test.  Here every workload of bench.py renders as bench.py renders it,
and every size boundary is crossed under an explicit mem_budget whose pass plan the test asserts.  Bar: the one of
test_gpu_parity.py — bit-exact tiles of the full frame against the oracle (the four corners among them: grid-stride loops reach the
last pixels last), identical images and ray counts between one large pass and many small ones.

Every test owns its Renderer and closes it: DevBuf::ensure never shrinks, so a session renderer would keep 100+ GB.
"""
import contextlib
import math
import os
import sys

import numpy as np
import pytest

import bench
import oracle_lib as O
import raygen
import tinyraytracing_amd as T
from test_gpu_parity import assert_same_image

pytestmark = pytest.mark.gpu

P28, P24 = 1 << 28, 1 << 24
MARGIN = 8 << 30  # free device memory asked for beyond the arena: scene, output, staging, the torch tensors of a test
COUNTS = ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "max_bounces")


def _bench_command():
    """bench.py's own defaults (its headline workload), read from its parser rather than restated."""
    argv = sys.argv
    sys.argv = ["bench.py"]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


_A = _bench_command()
HEADLINE = (_A.scene, _A.width, _A.height, _A.spp, None)
W, H = _A.width, _A.height
WORKLOADS = [HEADLINE] + [(name, ew or W, eh or H, spp, tris) for name, spp, _steps, ew, eh, tris in bench.EXTRA]


def oracle_threads():
    return int(os.environ.get("OMP_NUM_THREADS") or 16)


def path_bytes(scene):
    """Arena bytes of one path (include/trt.h, mem_budget): two ray queues, the hit, Lacc and the redo index, 132 B, plus a 48-B shadow
    queue per light."""
    return 132 + 48 * scene.info["n_lights"]


def budget_for(scene, npix, chunk):
    """A mem_budget whose passes hold exactly `chunk` samples of every pixel."""
    return npix * chunk * path_bytes(scene)


def small_chunk(npix):
    """The most samples per pass that keep every pass at or below 2^24 paths."""
    return max(P24 // npix, 1)


def require_free(nbytes, what):
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < nbytes + MARGIN:
        pytest.skip(f"{what}: {free / 2**30:.1f} GiB free on the device, {(nbytes + MARGIN) / 2**30:.1f} GiB needed (arena + 8 GiB)")
    return free


def render_device(r, p):
    """What bench.py's step does: render_into a device tensor on torch's current stream.  -> (host image, Stats)"""
    import torch
    out = torch.empty((len(T.rows_selected(p)), p.x1 - p.x0, 3), dtype=torch.float32, device="cuda:0")
    st = r.render_into(p, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    img = out.cpu().numpy()
    del out
    return img, st


def last_lit_tile(scene, p):
    """Top-left corner of the 8x8 tile that ends at the last lit pixel, in raster order, of a 1-spp oracle render of every 8th row of
    the frame's last eighth.  A frame's corners may be black (back's camera sees past the box), and a loop that stops early leaves a
    black pixel black: this tile is where the last trips of the grid-stride loops have light to lose."""
    w, h = p.width, p.height
    probe = T.make_params(w, h, 1, p.seed, tile=(0, h - max(h // 8, 8), w, h), rows=(1, 8, 7), max_depth=p.max_depth, flags=p.flags)
    img, _ = O.render(scene.flat, probe, threads=oracle_threads())
    lit = img.max(-1) > 0
    assert lit.any(), "nothing lit in the last eighth of the frame"
    i = np.flatnonzero(lit.any(1))[-1]
    x, y = int(np.flatnonzero(lit[i])[-1]), T.rows_selected(probe)[i]
    return min(max(x - 7, 0), w - 8), min(max(y - 7, 0), h - 8)


def tile_corners(scene, p, n_random, seed):
    """Top-left corners of 8x8 tiles: the four corners of the frame, the last lit tile, then n_random placed by a fixed rng."""
    w, h = p.width, p.height
    rng = np.random.default_rng(seed)
    pos = [(0, 0), (w - 8, 0), (0, h - 8), (w - 8, h - 8), last_lit_tile(scene, p)]
    pos += [(int(x), int(y)) for x, y in zip(rng.integers(0, w - 7, n_random), rng.integers(0, h - 7, n_random))]
    return pos


def check_tiles(scene, img, p, what, n_random=5, seed=0):
    """8x8 tiles of the full-frame image `img` of params p against the oracle's render of just those tiles; every differing tile is
    reported."""
    bad = []
    for x0, y0 in tile_corners(scene, p, n_random, seed):
        pt = T.make_params(p.width, p.height, p.spp, p.seed, tile=(x0, y0, x0 + 8, y0 + 8), max_depth=p.max_depth, flags=p.flags)
        ref, _ = O.render(scene.flat, pt, threads=oracle_threads())
        try:
            assert_same_image(img[y0:y0 + 8, x0:x0 + 8], ref, f"tile {x0},{y0}")
        except AssertionError as e:
            bad.append(str(e).splitlines()[0])
    assert not bad, f"{what}: " + "; ".join(bad)


def counts(st):
    return tuple(getattr(st, f) for f in COUNTS)


def same_as_small_passes(r, scene, p, img, st, what):
    """The same frame in passes of at most 2^24 paths: identical image and ray counts."""
    npix = p.width * p.height
    chunk = small_chunk(npix)
    q = T.make_params(p.width, p.height, p.spp, p.seed, flags=p.flags, mem_budget=budget_for(scene, npix, chunk))
    small, st_small = render_device(r, q)
    assert st_small.passes == math.ceil(p.spp / chunk) and npix * math.ceil(p.spp / st_small.passes) <= P24, (what, st_small.passes)
    assert np.array_equal(img, small), f"{what}: the image differs from the one rendered in {st_small.passes} passes"
    assert counts(st) == counts(st_small), what


@contextlib.contextmanager
def own_renderer(name, w, h, n=None):
    """A scene and a Renderer of this test's own, both closed on the way out, and torch's cached blocks returned to the device."""
    import torch
    scene = T.Scene.named(name, w, h, n=n)
    r = T.Renderer(scene, 0)
    try:
        yield scene, r
    finally:
        r.close()
        scene.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ A: bench.py's workloads, as bench.py renders them
@pytest.mark.parametrize("name,w,h,spp,tris", WORKLOADS, ids=[f"{n}-{w}x{h}x{s}" for n, w, h, s, _ in WORKLOADS])
def test_bench_workload_full_frame(name, w, h, spp, tris):
    with own_renderer(name, w, h, n=tris) as (scene, r):
        npix = w * h
        free = require_free(budget_for(scene, npix, small_chunk(npix)), name)
        p = T.make_params(w, h, spp, bench.SEEDS[name])  # mem_budget 0: three quarters of what is free, as in bench.py
        img, st = render_device(r, p)
        print(f"{name} {w}x{h}x{spp}: default plan {st.passes} pass(es), {free / 2**30:.1f} GiB free before the render")
        assert st.rays_camera == npix * spp
        assert np.isfinite(img).all() and img.max() > 0
        check_tiles(scene, img, p, name)
        same_as_small_passes(r, scene, p, img, st, name)
        if (name, w, h, spp, tris) == HEADLINE:  # bench.py's with_pass_overlap
            po = T.make_params(w, h, spp, bench.SEEDS[name], flags=T.TRT_FLAG_OVERLAP)
            ov, st_ov = render_device(r, po)
            print(f"{name} with TRT_FLAG_OVERLAP: default plan {st_ov.passes} passes")
            assert np.array_equal(img, ov) and counts(st) == counts(st_ov)


# ------------------------------------------------------------------ B: the size boundaries, each under an asserted plan
def large_pass_frame(name, scene, r, spp, chunk, flags=0, n_random=5):
    """The frame of `scene` at spp samples in passes of `chunk` samples (an explicit budget): oracle tiles, then the same frame in
    small passes.  -> (params, image, Stats)"""
    w, h = scene.info["width"], scene.info["height"]
    npix = w * h
    b = budget_for(scene, npix, chunk)
    free = require_free(b, f"{name} {w}x{h}x{spp} in passes of {chunk} samples")
    p = T.make_params(w, h, spp, bench.SEEDS[name], flags=flags, mem_budget=b)
    img, st = render_device(r, p)
    print(f"{name} {w}x{h}x{spp} under a budget for {chunk} samples: {st.passes} pass(es), {free / 2**30:.1f} GiB free before the render")
    assert st.rays_camera == npix * spp
    check_tiles(scene, img, p, f"{name} {w}x{h}x{spp}", n_random=n_random, seed=spp)
    serial = T.make_params(w, h, spp, p.seed, flags=flags & ~T.TRT_FLAG_OVERLAP)
    same_as_small_passes(r, scene, serial, img, st, f"{name} {w}x{h}x{spp}")
    return p, img, st


def test_b1_headline_in_one_pass():
    """back 1920x1080 x 256 in ONE pass: 530 841 600 paths, every array of 16-B records past 8 GiB."""
    with own_renderer("back", 1920, 1080) as (scene, r):
        _, _, st = large_pass_frame("back", scene, r, 256, chunk=256)
    assert st.passes == 1 and 1920 * 1080 * 256 == 530_841_600 > P28


def test_b2_three_shadow_queues_past_4gib():
    """veach-mis (3 lights: three shadow queues of 16-B records, ShadowArena::queue(l)) at 1920x1080 x 260 under a budget for 130
    samples: 2 passes of 269 568 000 paths, so k_shade and k_trace_shadow write each of those arrays past 4 GiB."""
    with own_renderer("veach-mis", 1920, 1080) as (scene, r):
        assert scene.info["n_lights"] == 3
        _, _, st = large_pass_frame("veach-mis", scene, r, 260, chunk=130)
    assert st.passes == 2 and 1920 * 1080 * 130 == 269_568_000 > P28


def test_b3_two_slots_in_flight_past_2_28():
    """back 1920x1080 x 390 with TRT_FLAG_OVERLAP and a budget of 2 x 130 samples: 2 slots of 269 568 000 paths and 3 passes (the third
    reuses slot 0 after the ordered resolve).  Identical to the oracle's tiles, to small serial passes and to the serial render under
    the same budget (one slot: 2 passes of 195 samples)."""
    with own_renderer("back", 1920, 1080) as (scene, r):
        p, img, st = large_pass_frame("back", scene, r, 390, chunk=2 * 130, flags=T.TRT_FLAG_OVERLAP)
        assert st.passes == 3 and 1920 * 1080 * 130 == 269_568_000 > P28
        serial, st_serial = render_device(r, T.make_params(1920, 1080, 390, p.seed, mem_budget=p.mem_budget))
        assert st_serial.passes == 2
        assert np.array_equal(img, serial) and counts(st) == counts(st_serial)


def test_b4_trace_closest_past_2_28_rays():
    """trt_trace_closest on 1025 copies of 2^18 incoherent rays plus a partial copy (its last wave partial): 268 797 603 rays, every copy
    equal to the oracle's trace of the base batch, and the visit counts those of the copies added up."""
    with own_renderer("staircase", 64, 36) as (scene, r):
        n, copies, m = 1 << 18, 1025, 100_003
        total = n * copies + m
        assert n * copies > P28 and m % 64
        require_free(total * (3 * 16 + 2 * 12 + 4), "trace_closest batch")  # ra, rb, hit; the caller's org and dir; the redo list
        lo, hi = raygen.scene_bounds(scene)
        org, dirs = raygen.random_rays(n, lo - 5, hi + 5, seed=2024)
        t0, tri0, uv0 = O.trace(scene.flat, org, dirs)
        _, _, _, st_base = r.trace_closest(org, dirs, want_stats=True)
        _, _, _, st_part = r.trace_closest(org[:m], dirs[:m], want_stats=True)
        big_o = np.empty((total, 3), np.float32)
        big_d = np.empty((total, 3), np.float32)
        big_o[:n * copies].reshape(copies, n, 3)[:] = org
        big_d[:n * copies].reshape(copies, n, 3)[:] = dirs
        big_o[n * copies:] = org[:m]
        big_d[n * copies:] = dirs[:m]
        t, tri, uv, st = r.trace_closest(big_o, big_d, want_stats=True)
        del big_o, big_d
        k = n * copies
        assert (tri[:k].reshape(copies, n) == tri0).all()
        assert (t[:k].view(np.uint32).reshape(copies, n) == t0.view(np.uint32)).all()
        assert (uv[:k].view(np.uint64).reshape(copies, n) == uv0.view(np.uint64)[:, 0]).all()
        assert np.array_equal(tri[k:], tri0[:m])
        assert np.array_equal(t[k:].view(np.uint32), t0[:m].view(np.uint32))
        assert np.array_equal(uv[k:].view(np.uint64), uv0[:m].view(np.uint64))
        assert st.inner_visits[0] == st_base.inner_visits[0] * copies + st_part.inner_visits[0]
        assert st.tri_tests[0] == st_base.tri_tests[0] * copies + st_part.tri_tests[0]


def test_b5_render_pixels_device_past_2_28_entries():
    """trt_render_pixels_device on the whole 1920x1080 frame listed 130 times (269 568 000 entries), sample [0, 1) from zero sums: every
    copy bit-identical, copy 0 equal to render_samples' accumulator, sumsq == sum * sum (one sample: k_resolve_moments adds fl(v * v)
    to zero).  Then an entry of W * H in the last place: k_list_max's grid-stride loop must find it (TRT_EINVAL)."""
    import torch
    w, h, copies = 1920, 1080, 130
    with own_renderer("back", w, h) as (scene, r):
        npix = w * h
        n = npix * copies
        assert n > P28
        b = budget_for(scene, n, 1)
        require_free(b + 3 * n * 3 * 8 + n * 4, "render_pixels list")  # arena; sums, sumsq and sums * sums; the list
        p = T.make_params(w, h, 3, bench.SEEDS["back"], mem_budget=b)
        _, acc, _ = r.render_samples(p, 0, 1)
        pixels = torch.arange(npix, dtype=torch.int32, device="cuda:0").repeat(copies)
        sums, sumsq, st = r.render_pixels(p, pixels, 0, 1)
        torch.cuda.synchronize()
        assert st.passes == 1 and st.rays_camera == n
        bits = sums.view(torch.int64).view(copies, npix, 3)
        for c in range(1, copies):
            assert torch.equal(bits[c], bits[0]), f"copy {c} differs from copy 0"
        assert np.array_equal(sums[:npix].cpu().numpy().reshape(h, w, 3).view(np.uint64), acc.view(np.uint64))
        assert torch.equal(sumsq.view(torch.int64), (sums * sums).view(torch.int64))
        pixels[-1] = npix
        with pytest.raises(T.TrtError, match=r"failed \(1\).*width \* height"):
            r.render_pixels(p, pixels, 0, 1, sums, sumsq)
        del bits, pixels, sums, sumsq
        # the handle renders correctly afterwards: the last row of the frame
        last = torch.arange((h - 1) * w, npix, dtype=torch.int32, device="cuda:0")
        s2, _, _ = r.render_pixels(p, last, 0, 1)
        assert np.array_equal(s2.cpu().numpy().view(np.uint64), acc[h - 1].view(np.uint64))


def test_b6_resolve_loops_past_2_24_pixels():
    """back 8192x4096 x 2 (33 554 432 pixels) through render_into: k_resolve goes round its grid of 65 536 blocks twice and k_finalize
    six times (100 M floats).  Equal to the host render of the same frame and to the oracle's tiles, the bottom-right one among them."""
    w, h, spp = 8192, 4096, 2
    with own_renderer("back", w, h) as (scene, r):
        npix = w * h
        assert npix > P24 and npix * 3 > 4 * P24
        b = budget_for(scene, npix, spp)
        require_free(b + npix * 3 * (8 + 4 + 4), "8192x4096 frame")  # arena; sums, device output, the host render's staging
        p = T.make_params(w, h, spp, bench.SEEDS["back"], mem_budget=b)
        img, st = render_device(r, p)
        assert st.passes == 1 and st.rays_camera == npix * spp
        host, st_host = r.render(p)
        assert np.array_equal(img, host) and counts(st) == counts(st_host)
        check_tiles(scene, img, p, "back 8192x4096", n_random=3, seed=6)


def test_b7_largest_pass_past_2_30_paths():
    """back 2048x2048 x 260 in one pass: 1 090 519 040 paths (about 196 GB), so the 4-B redo list passes 4 GiB and the 16-B records
    16 GiB.  Runs only when the device has the arena plus 8 GiB free."""
    w, h, spp = 2048, 2048, 260
    with own_renderer("back", w, h) as (scene, r):
        _, _, st = large_pass_frame("back", scene, r, spp, chunk=spp, n_random=3)
    assert st.passes == 1 and w * h * spp == 1_090_519_040 > (1 << 30)
