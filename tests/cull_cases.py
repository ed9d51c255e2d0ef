"""The cases that hold the camera-ray cull (trt_cull.h; k_shade's fused bounce 0, k_resolve_tile) on the GPU at its guard bands, at the limits
of its two LDS tables and at its degenerate bounds: plain data and helpers, no test.  Each case names its scene, size and camera and states,
before the bound is asked, the status the bound must have, the eight integers of TileDesc::cull it must give and, per tile, whether k_shade
culls in that call or the resolve alone.  tests/test_cull_cases_cpu.py holds every case to these statements without a GPU, so that
tests/test_gpu_primary_cull_edges.py cannot pass because a case degenerated.

  case(name, fixed, tile) -> (scene, params);   facts(scene, params) -> the bound (cull_ref.bound), the culled mask of the tile
  (cull_ref.culled_mask), and from the rays the renderer will trace (T.camera_rays): which paths have a zero direction component, and which
  of the fused kernel's 64-path waves (path i = s * npix + p, 64 consecutive i) hold such a ray next to culled paths."""
import numpy as np

import cull_ref as CR
import tinyraytracing_amd as T
from conftest import get_scene
from test_gpu_fused_primary import WithCamera
from test_gpu_primary_cull import root_boxes

ACTIVE, OFF = CR.ACTIVE, CR.OFF
FOVY = 39.3077                    # the shipped camera's
MIDDLE = (278.0, 273.0, 279.5)    # of the Cornell box, which spans [0, 556] x [0, 548.8] x [0, 559.2]
K_SHADE, RESOLVE = 1, 0           # the route of a call: k_shade skips the culled paths itself / k_resolve_tile alone skips their pixels
SHIFT_A = (4000.0, 0.0, 0.0)      # case A: the box moved to x in [4000, 4556]
SHIFT_AROUND_EYE = (3580.0, 0.0, -1500.0)  # the refit: the box spans [3580, 4136] x [0, 548.8] x [-1500, -940.8], case A's eye in its middle


def _orbit(yaw_deg, pitch_deg, dist):
    y, p = np.radians(yaw_deg), np.radians(pitch_deg)
    return tuple(np.array(MIDDLE) + np.array((dist * np.sin(y) * np.cos(p), dist * np.sin(p), -dist * np.cos(y) * np.cos(p))))


# name -> scene shift, (W, H), camera, spp, seed, status, the word an off reason must hold, TileDesc::cull per grid form (plain, fixed; None: not
# used in that form), the culled share of the frame it must stay within, tiles: name -> (make_params keywords, route)
CASES = {
    # A.  The eye looks down +z, 420 to the side of the box's middle: the band of columns (D_x = 0: the columns around s = 1/2) lies right of the
    # rectangle, in the culled strip.  At x = 3858 an ulp is 2^-12, a seventieth of a pixel's width in D_x, so one camera ray in seventy of column 48
    # has d.x == 0 exactly.  Found with seed 0xA014 at 16 spp (63 632 paths, 995 waves), plain / fixed grid: 13 / 13 rays with a zero component, 11 / 11
    # of them in column 48 (d.x) and 2 / 2 in the band of rows (d.y); 13 / 12 in pixels outside the rectangle, which a band alone keeps; 5 / 5 waves
    # hold one while lane 0 is culled; 1 / 1 wave holds one AT lane 0 with culled lanes behind it; none in a culled pixel.
    "bands": dict(shift=SHIFT_A, size=(97, 41), camera=lambda w, h: T.look_at((3858, 273, -1200), (3858, 273, 0), (0, 1, 0), FOVY, w, h), spp=16, seed=0xA014,
                  status=ACTIVE, word="", v=([6, 51, 3, 4, 20, 3, 47, 3], [5, 51, 2, 4, 19, 3, 47, 3]), share=(0.5, 0.7),
                  tiles={"frame": ({}, K_SHADE)}),
    # B.  4200 columns: more than TRT_SHADE_CULL_COLS = 4096 entries of s_colcls.  The box is columns [2016, 2183]; the band of rows takes four of the
    # six rows, so the share is 0.32.  Every tile holds culled columns on both sides of kept ones.
    "wide": dict(shift=None, size=(4200, 6), camera=lambda w, h: T.look_at((278, 273, -1200), (278, 273, 0), (0, 1, 0), 1.0, w, h), spp=2, seed=0xB1DE,
                 status=ACTIVE, word="", v=([2016, 2016, 0, 0, 2, 4, 2098, 4], None), share=(0.25, 0.4),
                 tiles={"frame": ({}, RESOLVE),  # 4200 wide
                        "4097 wide": (dict(tile=(50, 0, 4147, 6)), RESOLVE),
                        "4096 wide at x0 = 100": (dict(tile=(100, 0, 4196, 6)), K_SHADE)}),
    # B.  8300 rows: more than shadeRowsLds(512) = 8192 entries of s_rowcls.  An axis-parallel camera does not do (its band of columns covers all
    # eight columns: share 0), so the camera is turned — yawed 30 and pitched 20 degrees, 3000 from the box's middle, 30 degrees high — and every
    # component of its view direction stays away from zero over so narrow a frame: no band.  The box is rows [2127, 6592], share 0.46.
    "tall": dict(shift=None, size=(8, 8300), camera=lambda w, h: T.look_at(_orbit(30, 20, 3000), MIDDLE, (0, 1, 0), 30.0, w, h), spp=2, seed=0x7A11,
                 status=ACTIVE, word="", v=([0, 0, 2127, 1707, 0, 0, 0, 0], None), share=(0.25, 0.6),
                 tiles={"frame": ({}, RESOLVE),  # 8300 rows
                        "8193 rows": (dict(tile=(0, 50, 8, 8243)), RESOLVE),
                        "8192 rows": (dict(tile=(0, 50, 8, 8242)), K_SHADE),
                        # 4148 table rows of an image of 8300: table row r is image row 16 (r / 8) + 8 + r % 8, up to 8299
                        "every other block of 8 rows": (dict(rows=(8, 2, 1)), K_SHADE)}),
    # C.  The eye 3000 to the side: nothing of the box on the frame, everything is outside, only the bands are walked
    "off_frame": dict(shift=None, size=(97, 41), camera=lambda w, h: T.look_at((3278, 273, -1200), (3278, 273, 0), (0, 1, 0), FOVY, w, h), spp=4, seed=0xC0FF,
                      status=ACTIVE, word="", v=([97, 0, 41, 0, 20, 3, 47, 3], [97, 0, 41, 0, 19, 3, 47, 3]), share=(0.85, 0.95),
                      tiles={"frame": ({}, K_SHADE)}),
    # C.  The shipped camera on a square frame: the box fills it, the bound is active and nothing lies outside
    "nothing_outside": dict(shift=None, size=(41, 41), camera=None, spp=4, seed=0xC041,
                            status=ACTIVE, word="", v=([0, 0, 0, 0, 20, 3, 19, 3], None), share=(0.0, 0.0),
                            tiles={"frame": ({}, RESOLVE)}),
    # C.  The eye in the room, looking at the back wall
    "eye_inside": dict(shift=None, size=(97, 41), camera=lambda w, h: T.look_at((278, 273, 100), (278, 273, 500), (0, 1, 0), FOVY, w, h), spp=4, seed=0xC1D,
                       status=OFF, word="not in front", v=([0] * 8, [0] * 8), share=(0.0, 0.0),
                       tiles={"frame": ({}, RESOLVE)}),
    # C.  Yawed 30 and pitched 10 degrees at 70 degrees: the lines D_x = 0 and D_y = 0 cross the frame at a slant, through what would be culled
    "slanted": dict(shift=None, size=(97, 41), camera=lambda w, h: T.look_at(_orbit(30, 10, 3000), MIDDLE, (0, 1, 0), 70.0, w, h), spp=4, seed=0xC51,
                    status=OFF, word="slanted", v=([0] * 8, [0] * 8), share=(0.0, 0.0),
                    tiles={"frame": ({}, RESOLVE)}),
}

_moved = {}


def moved_back(w, h, shift):
    """A Scene of its own (not conftest's shared one): the shipped Cornell box with `shift` added to every vertex through Scene.set_vertices."""
    return T.Scene.named("back", w, h).set_vertices(shifted_vertices(shift))


def shifted_vertices(shift):
    """The shipped Cornell box's vertices plus `shift`, one fp32 addition each: the same bits whenever a scene is moved to `shift`, from wherever."""
    if "shipped" not in _moved:
        _moved["shipped"] = get_scene("back", 97, 41).arrays()["tri_v"]
    return _moved["shipped"] + np.array(shift, np.float32)


def scene_of(name):
    c = CASES[name]
    w, h = c["size"]
    if c["shift"] is None:
        base = get_scene("back", w, h)
    else:
        key = (w, h, c["shift"])
        if key not in _moved:
            _moved[key] = moved_back(w, h, c["shift"])
        base = _moved[key]
    return base if c["camera"] is None else WithCamera(base, c["camera"](w, h))


def case(name, fixed=False, tile="frame", **overrides):
    """-> (scene, params) of a case, on the plain or the fixed grid, for one of its tiles; `overrides` replace make_params keywords (spp, seed, ...)."""
    c = CASES[name]
    w, h = c["size"]
    kw = dict(c["tiles"][tile][0], flags=T.TRT_FLAG_FIXED_PIXELS if fixed else 0)
    spp, seed = overrides.pop("spp", c["spp"]), overrides.pop("seed", c["seed"])
    kw.update(overrides)
    return scene_of(name), T.make_params(w, h, spp, seed, **kw)


def route(name, tile="frame"):
    return CASES[name]["tiles"][tile][1]


def bound_of(s, p):
    return CR.bound(s.flat.contents.camera, p.width, p.height, bool(p.flags & T.TRT_FLAG_FIXED_PIXELS), root_boxes(s))


def debug_line(b):
    """What `trt_render: cull primary ` is followed by in the TRT_DEBUG output of a call whose bound is b"""
    if not b["active"]:
        return "off: " + b["why"]
    return "columns [%d, %d] rows [%d, %d] band rows [%d, %d] band columns [%d, %d]" % (b["rect"] + b["rows"] + b["cols"])


def tile_rows_cols(p):
    return np.asarray(T.rows_selected(p), np.int64), np.arange(p.x0, p.x1, dtype=np.int64)


def tile_mask(b, p):
    """cull_ref.culled_mask on the pixels of the tile of p, in tile order: bool [rows, tile_w]; all False for a bound that is off"""
    ys, xs = tile_rows_cols(p)
    if not b["active"]:
        return np.zeros((ys.size, xs.size), bool)
    return CR.culled_mask(b, p.width, p.height)[ys][:, xs]


def facts(s, p):
    """The bound of (s, p), the culled mask of its tile, and what the rays the renderer will trace (T.camera_rays: host code, the exact rays)
    say about k_shade's waves.  Path i = sample * npix + tile pixel; a wave is 64 consecutive i (the blocks are 512 wide and start at
    multiples of 512).
      zero [spp, npix]      the camera ray has a zero direction component (a ray of raySpecial: fusedPrimaryHit's vote, redo_rays)
      n_zero                their number
      zero_pixels           (y, x) of the image pixels that hold one
      zero_culled           how many of them lie in a culled pixel (must be 0)
      n_zero_outside        how many lie in a pixel outside the rectangle (kept by a band alone)
      waves_lane0_culled    waves that hold such a ray while lane 0 holds a culled path: the redo_rays atomic is not lane 0's to issue
      waves_zero_at_lane0   waves whose lane 0 holds such a ray and which have culled lanes behind it"""
    b = bound_of(s, p)
    mask = tile_mask(b, p)
    ys, xs = tile_rows_cols(p)
    pix = (ys[:, None] * p.width + xs[None, :]).reshape(-1)
    _, d = T.camera_rays(s.flat.contents.camera, p, pix.astype(np.uint32), 0, p.spp)
    zero = (d == 0).any(axis=-1)
    n = zero.size
    n_waves = (n + 63) // 64

    def waves(a):
        return np.concatenate([a.reshape(-1), np.zeros(n_waves * 64 - n, bool)]).reshape(n_waves, 64)

    zw, cw = waves(zero), waves(np.tile(mask.reshape(-1), p.spp))
    zp = np.unique(pix[zero.any(axis=0)])
    j_lo, j_hi, i_lo, i_hi = b["rect"] if b["active"] else (0, p.width - 1, 0, p.height - 1)
    outside = ((xs[None, :] < j_lo) | (xs[None, :] > j_hi) | (ys[:, None] < i_lo) | (ys[:, None] > i_hi)).reshape(-1)
    return {"bound": b, "mask": mask, "zero": zero, "n_zero": int(zero.sum()), "zero_pixels": [(int(q // p.width), int(q % p.width)) for q in zp],
            "zero_culled": int((zw & cw).sum()), "n_zero_outside": int((zero & outside[None, :]).sum()), "n_waves": n_waves,
            "waves_lane0_culled": int((zw.any(axis=1) & cw[:, 0]).sum()),
            "waves_zero_at_lane0": int((zw[:, 0] & cw[:, 1:].any(axis=1)).sum())}
