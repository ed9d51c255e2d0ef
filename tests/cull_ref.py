"""The camera-ray cull bound (tinyraytracing_amd/csrc/trt_cull.h) for the tests:
  - bound() / sweep(): the CPU build tests/cull/libcull_cpu.so (make cullcpu; part of `make all`), i.e. the host function itself and a sweep
    that forms the camera ray of every culled pixel under a set of jitter pairs with trt_path.h's cameraRay and holds it to boxTest and
    boxTestGlm;
  - analytic(): the projection written out again in numpy float64, independently of that code: the pixel rectangle that the sixteen corners
    of the two boxes span, widened by two pixels;
  - CAMERAS: the fixed corpus, each entry with the status the bound must report, stated before it is asked."""
import ctypes as C
import os

import numpy as np

import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cull", "libcull_cpu.so")
fp = C.POINTER(C.c_float)
_lib = None
SIZES = ((33, 25), (97, 41), (64, 2))
N_INTERIOR = 64
SEED = 0x5EED

# two boxes side by side that make up [-1, 1]^3: the root of every camera of the corpus but `back`'s
UNIT_BOXES = np.array([-1, -1, -1, 0, 1, 1, 0, -1, -1, 1, 1, 1], np.float32)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.cull_bound.argtypes = [C.POINTER(_abi.Camera), C.c_int, C.c_int, C.c_int, fp, C.c_uint32, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_char_p)]
        L.cull_sweep.argtypes = [C.POINTER(_abi.Camera), C.c_int, C.c_int, C.c_int, fp, C.c_uint32, C.c_double, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def bound(cam, w, h, fixed, boxes, n_nodes=1, margin=1.0):
    """-> dict(active, why, v = TileDesc::cull, rect = (j_lo, j_hi, i_lo, i_hi), rows = (lo, hi), cols = (lo, hi))"""
    boxes = np.ascontiguousarray(boxes, np.float32)
    out = (C.c_int32 * 16)()
    why = C.c_char_p()
    a = lib().cull_bound(C.byref(cam), w, h, int(fixed), boxes.ctypes.data_as(fp), n_nodes, margin, out, C.byref(why))
    o = list(out)
    return {"active": bool(a), "why": (why.value or b"").decode(), "v": o[:8], "rect": tuple(o[8:12]), "rows": tuple(o[12:14]), "cols": tuple(o[14:16])}


SWEEP_KEYS = ("culled", "rays", "pass_clean", "pass_literal", "zero_component", "special", "grid_forms_differ")


def sweep(cam, w, h, fixed, boxes, n_nodes=1, margin=1.0, n_interior=N_INTERIOR):
    boxes = np.ascontiguousarray(boxes, np.float32)
    cnt = (C.c_uint64 * 7)()
    lib().cull_sweep(C.byref(cam), w, h, int(fixed), boxes.ctypes.data_as(fp), n_nodes, margin, SEED, n_interior, cnt)
    return dict(zip(SWEEP_KEYS, [int(x) for x in cnt]))


def culled_mask(b, w, h):
    """The pixels TileDesc::cull = b["v"] culls, as pixelCulled (trt_path.h) decides it: bool [h, w]."""
    v = b["v"]
    i, j = np.mgrid[0:h, 0:w]
    out = (j < v[0]) | (j >= w - v[1]) | (i < v[2]) | (i >= h - v[3])
    band = ((i >= v[4]) & (i < v[4] + v[5])) | ((j >= v[6]) & (j < v[6] + v[7]))
    return out & ~band


def analytic(cam, w, h, fixed, boxes, frame=2):
    """The pixels outside the rectangle that the projections of the boxes' sixteen corners span, widened by `frame` pixels: bool [h, w].
    None where a corner does not project (not in front of the camera)."""
    f8 = np.float64
    eye, llc, hor, ver = (np.array(list(getattr(cam, k)), f8) for k in ("eye", "lower_left_corner", "horizontal", "vertical"))
    b = np.asarray(boxes, f8).reshape(2, 2, 3)
    st = []
    for box in b:
        for c in range(8):
            p = np.array([box[(c >> k) & 1, k] for k in range(3)])
            m = np.stack([hor, ver, -(p - eye)], axis=1)
            if abs(np.linalg.det(m)) < 1e-12:
                return None
            s, t, mu = np.linalg.solve(m, -(llc - eye))
            if mu <= 0:
                return None
            st.append((s, t))
    st = np.array(st)
    j = np.arange(w, dtype=f8)
    i = np.arange(h, dtype=f8)
    # pixel centres on cameraRay's grids
    sc = (j + 0.5) / w if fixed else j / (w - 1.0)
    tc = (h - 0.5 - i) / h if fixed else (h - i) / (h - 1.0)
    ps, pt = 1.0 / (w - 1.0), 1.0 / (h - 1.0)
    keep_c = (sc >= st[:, 0].min() - (frame + 0.5) * ps) & (sc <= st[:, 0].max() + (frame + 0.5) * ps)
    keep_r = (tc >= st[:, 1].min() - (frame + 0.5) * pt) & (tc <= st[:, 1].max() + (frame + 0.5) * pt)
    return ~(keep_r[:, None] & keep_c[None, :])


def back_case(w, h):
    """(camera, boxes) of the shipped Cornell box at w x h: its camera and the two child boxes of its root node."""
    sc = T.Scene.named("back", w, h)
    f = sc.flat.contents
    n = f.nodes[0]
    boxes = np.array(list(n.lo0) + list(n.hi0) + list(n.lo1) + list(n.hi1), np.float32)
    cam = _abi.Camera()
    for k in ("eye", "lower_left_corner", "horizontal", "vertical"):
        setattr(cam, k, _abi.c_float3(*list(getattr(f.camera, k))))
    sc.close()
    return cam, boxes


def _orbit(yaw_deg, pitch_deg, dist):
    y, p = np.radians(yaw_deg), np.radians(pitch_deg)
    return (dist * np.sin(y) * np.cos(p), dist * np.sin(p), -dist * np.cos(y) * np.cos(p))


ACTIVE, OFF = "active", "off"
# name -> (camera maker (w, h) -> Camera, boxes, status, the word the reason must hold when off).  The unit boxes make up [-1, 1]^3.
#   front          on the z axis, 12 away, 30 degrees: the box in the middle of the frame, D_x = 0 a band of columns, D_y = 0 a band of rows
#   rolled         the same rolled by 90 degrees: horizontal runs along y, vertical along x, so D_x = 0 is a band of rows and D_y = 0 one of columns
#   yawed_narrow   yawed 30 and pitched 10 degrees, 24 away, 12 degrees: every component of the view direction is far from zero over so narrow a
#                  frame (half angles 6 degrees and, at 97 x 41, 14), so no zero set reaches it
#   yawed_wide     the same at 70 degrees: the lines D_x = 0 and D_y = 0 cross the frame at a slant, through the culled area
#   inside         the eye in the box
#   near_plane     the eye on the plane z = -1 of the box, beside it: the corners of that face lie in the plane through the eye parallel to the image
#   side_plane     the eye on the plane x = 1 of the box, 12 in front of it: every corner in front, the rays along the plane are the band of columns
#   half_behind    the eye beside the box at its middle: half of it behind the camera
#   behind         the box behind the camera
#   covering       half a unit in front of the box at 30 degrees: at 33 x 25 the box fills the frame (active, nothing to cull)
#   corner         the box 40 away and the camera moved sideways and down (not turned: its zero sets stay bands), so that the box sits in the
#                  upper left corner of the frame
CAMERAS = {
    "front": (lambda w, h: T.look_at((0, 0, -12), (0, 0, 0), (0, 1, 0), 30, w, h), UNIT_BOXES, ACTIVE, ""),
    "rolled": (lambda w, h: T.look_at((0, 0, -12), (0, 0, 0), (1, 0, 0), 30, w, h), UNIT_BOXES, ACTIVE, ""),
    "yawed_narrow": (lambda w, h: T.look_at(_orbit(30, 10, 24), (0, 0, 0), (0, 1, 0), 12, w, h), UNIT_BOXES, ACTIVE, ""),
    "yawed_wide": (lambda w, h: T.look_at(_orbit(30, 10, 24), (0, 0, 0), (0, 1, 0), 70, w, h), UNIT_BOXES, OFF, "slanted"),
    "inside": (lambda w, h: T.look_at((0.25, 0.1, -0.5), (0.25, 0.1, 5), (0, 1, 0), 30, w, h), UNIT_BOXES, OFF, "front"),
    "near_plane": (lambda w, h: T.look_at((5, 0, -1), (5, 0, 5), (0, 1, 0), 30, w, h), UNIT_BOXES, OFF, "front"),
    "side_plane": (lambda w, h: T.look_at((1, 0, -12), (1, 0, 0), (0, 1, 0), 30, w, h), UNIT_BOXES, ACTIVE, ""),
    "half_behind": (lambda w, h: T.look_at((5, 0, 0), (5, 0, 5), (0, 1, 0), 30, w, h), UNIT_BOXES, OFF, "front"),
    "behind": (lambda w, h: T.look_at((0, 0, -12), (0, 0, -24), (0, 1, 0), 30, w, h), UNIT_BOXES, OFF, "front"),
    "covering": (lambda w, h: T.look_at((0, 0, -1.5), (0, 0, 0), (0, 1, 0), 30, w, h), UNIT_BOXES, ACTIVE, ""),
    "corner": (lambda w, h: T.look_at((9.5, -6.5, -40), (9.5, -6.5, 0), (0, 1, 0), 30, w, h), UNIT_BOXES, ACTIVE, ""),
}
