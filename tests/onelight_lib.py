"""ctypes binding of tests/onelight/libonelight_cpu.so — the CPU build of TRT_FLAG_ONE_LIGHT (tests/onelight/onelight_cpu.cpp) — the float64
restatement of lightPick's contract (include/trt.h), and the statistical criterion the one-light tests share."""
import ctypes as C
import os

import numpy as np

import tinyraytracing_amd as T
from tinyraytracing_amd._abi import Params, SceneFlat

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "onelight", "libonelight_cpu.so")
FEATURE, MUTANT_NO_WEIGHT, ALL_LIGHTS = 0, 1, 2  # `mutant` of onelight_render: the flag; inv_p forced to 1; every light (TRT_FLAG_FIXED_NEE's estimator)
FLAGS = T.TRT_FLAG_ONE_LIGHT | T.TRT_FLAG_FIXED_NEE
LUMA = np.array([0.2126, 0.7152, 0.0722])
_vp = C.c_void_p
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.onelight_render.restype = C.c_int
        L.onelight_render.argtypes = [C.POINTER(SceneFlat), C.POINTER(Params), _vp, C.POINTER(C.c_uint64), C.c_int]
        L.onelight_render_seeds.restype = C.c_int
        L.onelight_render_seeds.argtypes = [C.POINTER(SceneFlat), C.POINTER(Params), C.c_int, C.c_uint32, _vp]
        L.onelight_pick.restype = C.c_int
        L.onelight_pick.argtypes = [C.c_uint32, _vp, _vp, C.c_int, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]
        _lib = L
    return _lib


def _fixed(p):
    """p with TRT_FLAG_FIXED_NEE (the CPU build refuses anything else, as the library does) and without the bits a CPU render has no use for."""
    q = Params.from_buffer_copy(p)
    assert q.flags & T.TRT_FLAG_FIXED_NEE
    return q


def render(flat, p, mutant=FEATURE):
    """The tile of p -> (float32 image [rows, tile_w, 3], [camera, shadow, indirect] rays)."""
    q = _fixed(p)
    out = np.empty((len(T.rows_selected(q)), q.x1 - q.x0, 3), np.float32)
    rays = (C.c_uint64 * 3)()
    rc = lib().onelight_render(flat, C.byref(q), out.ctypes.data, rays, int(mutant))
    assert rc == 0, f"onelight_render returned {rc}"
    return out, [int(x) for x in rays]


def render_seeds(flat, p, n, mutant=FEATURE):
    """n one-sample renders with the seeds p.seed + 1 + k -> float32 [n, rows, tile_w, 3]."""
    q = _fixed(p)
    out = np.empty((n, len(T.rows_selected(q)), q.x1 - q.x0, 3), np.float32)
    rc = lib().onelight_render_seeds(flat, C.byref(q), int(mutant), int(n), out.ctypes.data)
    assert rc == 0, f"onelight_render_seeds returned {rc}"
    return out


def pick(area, radiance, u, table=True):
    """lightPick on n lights of (area, radiance [n, 3]) for each uniform of u -> dict(sampled bool [m], index uint32 [m], inv_p float32 [m],
    draws uint32 [m] (what lightPick took from a stream), cdf float32 [n] (the running sums of the selection table))."""
    area = np.ascontiguousarray(area, np.float32).reshape(-1)
    radiance = np.ascontiguousarray(radiance, np.float32).reshape(-1, 3)
    u = np.ascontiguousarray(u, np.float32).reshape(-1)
    n, m = len(area), len(u)
    assert radiance.shape[0] == n
    out = {"sampled": np.zeros(m, np.uint8), "index": np.zeros(m, np.uint32), "inv_p": np.zeros(m, np.float32), "draws": np.zeros(m, np.uint32),
           "cdf": np.zeros(max(n, 1), np.float32)}
    rc = lib().onelight_pick(n, area.ctypes.data, radiance.ctypes.data, 1 if table else 0, m, u.ctypes.data, out["sampled"].ctypes.data, out["index"].ctypes.data,
                             out["inv_p"].ctypes.data, out["draws"].ctypes.data, out["cdf"].ctypes.data)
    assert rc == 0, f"onelight_pick returned {rc} (3: lightPick and lightPickAt disagree on a stream's draw)"
    out["sampled"] = out["sampled"].astype(bool)
    out["cdf"] = out["cdf"][:n]
    return out


# ---- the contract of include/trt.h, restated ------------------------------------------------------------------------------------------

def weights(area, radiance):
    """w_l = area_l * lum(radiance_l) in fp32 (lum in trt_dn_lum's order), 0 unless area and luminance are both finite and > 0."""
    f = np.float32
    area = np.asarray(area, f).reshape(-1)
    rad = np.asarray(radiance, f).reshape(-1, 3)
    with np.errstate(all="ignore"):
        lum = (f(0.2126) * rad[:, 0] + f(0.7152) * rad[:, 1]) + f(0.0722) * rad[:, 2]
        ok = np.isfinite(area) & (area > 0) & np.isfinite(lum) & (lum > 0)
        return np.where(ok, area * lum, f(0)).astype(f)


def cdf32(w):
    """cdf_l = cdf_{l-1} + w_l, summed in fp32 in index order."""
    c, out = np.float32(0), np.zeros(len(w), np.float32)
    with np.errstate(all="ignore"):
        for l, x in enumerate(np.asarray(w, np.float32)):
            c = np.float32(c + x)
            out[l] = c
    return out


def pick_f64(w, cdf, u):
    """The search in float64 on the fp32 table: r = u * cdf[-1] exactly; the first l with r < cdf_l, else the last l with w_l > 0.
    -> (index [m], margin [m]: min |r - cdf_l| over l in fp32 ulps of r — how far r is from any decision)."""
    c = np.asarray(cdf, np.float64)
    r = np.asarray(u, np.float64) * c[-1]
    idx = np.searchsorted(c, r, side="right")
    last = int(np.flatnonzero(np.asarray(w) > 0)[-1])
    idx = np.where(idx >= len(c), last, idx)
    ulp = np.spacing(np.maximum(r, 1e-38).astype(np.float32)).astype(np.float64)  # of r as the device rounds it
    margin = np.abs(r[:, None] - c[None, :]).min(axis=1) / ulp
    return idx, margin


# ---- the statistical criterion -------------------------------------------------------------------------------------------------------
Z_PIXEL, PIXEL_SHARE, Z_IMAGE = 4.0, 0.01, 4.0


def moments_of(ones):
    """Per-pixel mean luminance and the variance of that mean from n one-sample renders [n, ..., 3], as tests/denoise_ref.py's oracle_inputs forms them."""
    lum = np.asarray(ones, np.float64) @ LUMA
    return lum.mean(axis=0), lum.var(axis=0, ddof=1) / lum.shape[0]


def criterion(m1, v1, m2, v2):
    """z = (m1 - m2) / sqrt(v1 + v2) per pixel over the pixels either image lit ("hit": a mean or a variance above 0).
    -> (share of hit pixels with |z| > 4, image-wide |sum(m1 - m2)| / sqrt(sum(v1 + v2)), hit pixels)."""
    m1, v1, m2, v2 = (np.asarray(a, np.float64).reshape(-1) for a in (m1, v1, m2, v2))
    hit = (m1 > 0) | (m2 > 0) | (v1 > 0) | (v2 > 0)
    d, v = (m1 - m2)[hit], (v1 + v2)[hit]
    with np.errstate(all="ignore"):
        z = np.where(v > 0, np.abs(d) / np.sqrt(v), np.where(d != 0, np.inf, 0.0))
    share = float((z > Z_PIXEL).mean()) if hit.any() else 0.0
    whole = float(abs(d.sum()) / np.sqrt(v.sum())) if v.sum() > 0 else (0.0 if d.sum() == 0 else np.inf)
    return share, whole, int(hit.sum())


def passes(share, whole):
    return share <= PIXEL_SHARE and whole <= Z_IMAGE
