"""Device groups whose ranks get unequal shares of the rows (trt_group_render*) — MI355X only, on one GPU named several times.

The group deals stripes of row_block rows to its ranks in turn, pads every rank's buffer to the largest share (pad_rows), skips ranks
that get no stripe and un-interleaves on the first device (k_uninterleave).  Here the shares differ, the last stripe is partial, ranks get
nothing, a tile ends inside a stripe, and one group renders a large frame, a small tile and the large frame again, so that the pad rows of
the small render still hold the large render's data.  Everything is compared bit for bit with one Renderer.render of the same
parameters, the summed ray counts included."""
import numpy as np
import pytest

import tinyraytracing_amd as T
from conftest import get_scene

pytestmark = pytest.mark.gpu

W, SPP, SEED = 53, 4, 0x5EED0002  # an odd row length


def params(h, tile=None, row_block=None):
    p = T.make_params(W, h, SPP, SEED, tile=tile)
    if row_block is not None:
        p.row_block = row_block  # the group's stripe height (a single render selects every row)
    return p


def shares(h, n, rb, y0=0, y1=None):
    """Rows of the tile each rank renders."""
    out = [0] * n
    for y in range(y0, h if y1 is None else y1):
        out[(y // rb) % n] += 1
    return out


_singles = {}


def single(scene_key, s, h, tile=None):
    """One Renderer.render of the tile: (image, Stats)."""
    key = (scene_key, h, tile)
    if key not in _singles:
        r = T.Renderer(s, 0)
        try:
            _singles[key] = r.render(params(h, tile))
        finally:
            r.close()
    return _singles[key]


def ray_counts(st):
    return (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits)


def assert_equals_single(img, gst, ref, st, rows, what):
    assert img.shape == ref.shape, what
    bad = img.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad.any(-1))[0].tolist()}"
    assert ray_counts(gst) == ray_counts(st), what
    assert gst.max_bounces == st.max_bounces and gst.rows_rendered == rows, what


# (H, ranks, row_block, tile, the shares this is about)
CASES = [
    (50, 3, 8, None, [18, 16, 16]),          # unequal shares; the last stripe has 2 rows and goes to rank 0
    (50, 4, 16, None, [16, 16, 16, 2]),      # rank 3 gets the 2-row stripe only
    (10, 4, 8, None, [8, 2, 0, 0]),          # ranks 2 and 3 get nothing
    (2, 2, 8, (0, 0, W, 1), [1, 0]),         # one row (an image has at least two: the tile is its first), rank 1 idle
    (50, 2, 4, (5, 8, 48, 45), [20, 17]),    # y0 on a stripe boundary of rank 0, y1 inside a stripe of rank 1
]


@pytest.mark.parametrize("h,n,rb,tile,want_shares", CASES, ids=[f"H{h}-n{n}-rb{rb}{'-tile' if t else ''}" for h, n, rb, t, _ in CASES])
def test_unequal_shares_equal_a_single_render(h, n, rb, tile, want_shares):
    y0, y1 = (tile[1], tile[3]) if tile else (0, h)
    assert shares(h, n, rb, y0, y1) == want_shares
    s = get_scene("veach-mis", W, h)
    ref, st = single("veach-mis", s, h, tile)
    g = T.GroupRenderer(s, [0] * n)
    try:
        for k in range(2):  # the second render reuses the group's buffers
            img, gst, gms = g.render(params(h, tile, rb))
            assert_equals_single(img, gst, ref, st, y1 - y0, f"H {h}, {n} ranks, stripes of {rb}, render {k}")
            assert gms >= 0.0
    finally:
        g.close()


def test_buffers_shrink_and_grow_on_one_group():
    """The full 50-row frame, a 10-row tile, the full frame again, through render and through render_into into a tensor filled with a
    sentinel and followed by guard floats that stay untouched."""
    import torch
    h, n, rb = 50, 3, 8
    s = get_scene("veach-mis", W, h)
    full, st_full = single("veach-mis", s, h)
    small_tile = (0, 0, W, 10)
    small, st_small = single("veach-mis", s, h, small_tile)
    assert shares(h, n, rb, 0, 10) == [8, 2, 0]
    g = T.GroupRenderer(s, [0] * n)
    try:
        for tile, ref, st in ((None, full, st_full), (small_tile, small, st_small), (None, full, st_full)):
            img, gst, _ = g.render(params(h, tile, rb))
            assert_equals_single(img, gst, ref, st, ref.shape[0], f"render, tile {tile}")
        sentinel, guard = -7.25, 64
        for tile, ref, st in ((None, full, st_full), (small_tile, small, st_small), (None, full, st_full)):
            need = ref.size
            out = torch.full((need + guard,), sentinel, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            gst, _ = g.render_into(params(h, tile, rb), out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[need:] == np.float32(sentinel)).all(), f"render_into, tile {tile}: floats behind the image were written"
            assert_equals_single(got[:need].reshape(ref.shape), gst, ref, st, ref.shape[0], f"render_into, tile {tile}")
    finally:
        g.close()


RCCL_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import tinyraytracing_amd as T
maps = lambda: open("/proc/self/maps").read()
assert "torch" not in sys.modules and "librccl" not in maps(), "librccl is mapped before any group exists"
s = T.Scene.named("veach-mis", {w}, 50)
p = T.make_params({w}, 50, {spp}, {seed})
r = T.Renderer(s, 0)
ref, st = r.render(p)
r.close()
assert "librccl" not in maps(), "a single renderer loaded librccl"
g = T.GroupRenderer(s, [0])
assert "librccl" in maps(), "the RCCL route was not taken: librccl is not loaded"
p.row_block = 8
for k in range(2):
    img, gst, _ = g.render(p)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), k
    assert (gst.rays_camera, gst.rays_shadow, gst.rays_indirect, gst.shaded_hits, gst.rows_rendered) == (st.rays_camera, st.rays_shadow, st.rays_indirect, st.shaded_hits, 50), k
g.close()
print("rccl route ok")
"""


def test_rccl_route_with_a_partial_last_stripe():
    """TRT_GROUP_FORCE_RCCL=1, one rank: ncclGather of a buffer whose last stripe has 2 rows.  In a process of its own, because this one
    has librccl mapped already once torch is imported: there the library appears exactly when the group is created."""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = RCCL_CHILD.format(root=os.path.dirname(tests), tests=tests, w=W, spp=SPP, seed=SEED)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TRT_GROUP_FORCE_RCCL="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "rccl route ok" in out.stdout, out.stdout + out.stderr


def test_many_lights_with_unequal_shares():
    """17 lights (k_shade's SHADE_MANY, shadow queues sized per rank by its own share) at 18 / 16 / 16 rows."""
    h, n, rb = 50, 3, 8
    s = get_scene("lamps", W, h, n=16)
    assert s.info["n_lights"] == 17
    ref, st = single("lamps", s, h)
    assert st.rays_shadow > 0
    g = T.GroupRenderer(s, [0] * n)
    try:
        img, gst, _ = g.render(params(h, None, rb))
        assert_equals_single(img, gst, ref, st, h, "17 lights, 3 ranks")
    finally:
        g.close()
