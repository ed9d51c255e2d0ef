"""The a-trous filter of trt_denoise (include/trt.h) twice over, for the tests:
  - cpu(): the CPU build of the kernels' per-pixel code (tests/denoise/libdenoise_cpu.so from tinyraytracing_amd/csrc/trt_denoise.h), which
    the GPU must match bit for bit;
  - restate(): the contract of include/trt.h written out again in numpy float64, independently of that code, which the CPU build must
    match to about 1e-4 relative (fp32 against float64; products with reciprocals against quotients).
And small denoiser inputs made on the CPU: random guides, and oracle renders with tests/aov_ref.py feature buffers."""
import ctypes as C
import os

import numpy as np

import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise", "libdenoise_cpu.so")
fp = C.POINTER(C.c_float)
LUMA = np.array([0.2126, 0.7152, 0.0722])
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
INF = float(np.float32(T._abi.TRT_INF))
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        L.denoise_cpu.argtypes = [C.POINTER(_abi.DenoiseParams), C.c_int, C.c_int] + [fp] * 6
        L.denoise_cpu_expf_neg.restype = C.c_float
        L.denoise_cpu_expf_neg.argtypes = [C.c_float]
        L.denoise_cpu_radius.restype = C.c_float
        L.denoise_cpu_radius.argtypes = [C.c_int]
        L.denoise_cpu_powi.restype = C.c_float
        L.denoise_cpu_powi.argtypes = [C.c_float, C.c_int]
        _lib = L
    return _lib


def params(iterations=5, sigma_normal=128, sigma_depth=1.0, sigma_luminance=4.0, flags=0):
    p = _abi.DenoiseParams()
    p.iterations, p.sigma_normal, p.sigma_depth, p.sigma_luminance, p.flags = iterations, sigma_normal, sigma_depth, sigma_luminance, flags
    return p


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cpu(color, variance, albedo, normal, depth, **kw):
    """The CPU build: float32 [h, w, 3]."""
    bufs = [_f32(color), _f32(variance), _f32(albedo), _f32(normal), _f32(depth)]
    h, w = bufs[0].shape[:2]
    out = np.empty((h, w, 3), np.float32)
    p = params(**kw)
    rc = lib().denoise_cpu(C.byref(p), w, h, *[b.ctypes.data_as(fp) for b in bufs], out.ctypes.data_as(fp))
    assert rc == 0
    return out


def _shift(a, dx, dy):
    """b[y, x] = a[y + dy, x + dx] where that pixel is in the image, and the mask of those pixels."""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    m = np.zeros((h, w), bool)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[yd, xd] = a[ys, xs]
        m[yd, xd] = True
    return b, m


def restate(color, variance, albedo, normal, depth, iterations=5, sigma_normal=128, sigma_depth=1.0, sigma_luminance=4.0):
    """include/trt.h's contract in float64: -> [h, w, 3] float64."""
    color, albedo, normal = (np.asarray(x, np.float64) for x in (color, albedo, normal))
    variance, z = np.asarray(variance, np.float64), np.asarray(depth, np.float64)
    hit = z < INF
    # 1. demodulate
    a = np.where(albedo > 0, albedo, 1.0)
    c = color / a
    var = variance / np.maximum(a @ LUMA, 1e-6) ** 2
    # 2. depth gradient: per axis the smaller difference to a neighbour that is an in-image hit
    g = []
    for (dx0, dy0), (dx1, dy1) in (((-1, 0), (1, 0)), ((0, -1), (0, 1))):
        z0, m0 = _shift(z, dx0, dy0)
        z1, m1 = _shift(z, dx1, dy1)
        m0 &= _shift(hit, dx0, dy0)[0]
        m1 &= _shift(hit, dx1, dy1)[0]
        d0, d1 = np.abs(z0 - z), np.abs(z1 - z)
        g.append(np.where(m0 & m1, np.minimum(d0, d1), np.where(m0, d0, np.where(m1, d1, 0.0))))
    gz = np.maximum(g[0], g[1])
    # 3. levels
    for k in range(iterations):
        s = 2 ** k
        acc, ws = np.zeros_like(var), np.zeros_like(var)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v, m = _shift(var, dx, dy)
                kk = (0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25)
                acc += kk * v * m
                ws += kk * m
        sd = np.sqrt(acc / ws)
        lum = c @ LUMA
        sc, sv, sw = np.zeros_like(c), np.zeros_like(var), np.zeros_like(var)
        for j in range(5):
            for i in range(5):
                dx, dy = s * (i - 2), s * (j - 2)
                cq, m = _shift(c, dx, dy)
                vq, _ = _shift(var, dx, dy)
                if i == 2 and j == 2:
                    w = np.full(var.shape, 9 / 64)
                else:
                    nq, _ = _shift(normal, dx, dy)
                    zq, _ = _shift(z, dx, dy)
                    hq, _ = _shift(hit, dx, dy)
                    m = m & hq
                    with np.errstate(all="ignore"):
                        wn = np.maximum(0.0, np.sum(normal * nq, axis=2)) ** sigma_normal
                        dist = np.hypot(dx, dy)
                        wz = np.exp(-np.abs(z - zq) / (sigma_depth * gz * dist + 1e-3 * z))
                        wl = np.exp(-np.abs(lum - cq @ LUMA) / (sigma_luminance * sd + 1e-6))
                        w = np.where(m, H5[i] * H5[j] * wn * wz * wl, 0.0)
                sc += w[..., None] * cq
                sv += w * w * vq
                sw += w
        c = np.where(hit[..., None], sc / sw[..., None], c)
        var = np.where(hit, sv / (sw * sw), var)
    # 4. remodulate
    return c * a


def assert_close(got, want, rtol=1e-4, what=""):
    """|got - want| <= rtol |want| + rtol * 1e-3 max |want| everywhere (the absolute floor covers outputs that are nearly 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    floor = rtol * 1e-3 * max(float(np.abs(want).max()), 1e-30)
    err = np.abs(got - want) - (rtol * np.abs(want) + floor)
    bad = np.argwhere(err > 0)
    assert bad.size == 0, f"{what}: {len(bad)} values off, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def random_inputs(h, w, seed, miss_frac=0.1, planes=3):
    """Piecewise-smooth guides: a few planes with their own normal direction and depth slope, random misses, noisy colour on a smooth
    albedo-modulated signal, and a positive variance.  -> (color, variance, albedo, normal, depth) float32."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    label = (rng.integers(0, planes, (max(1, h // 4 + 1), max(1, w // 4 + 1))).repeat(4, 0).repeat(4, 1))[:h, :w]
    normal = np.zeros((h, w, 3))
    depth = np.zeros((h, w))
    for k in range(planes):
        n = rng.normal(size=3)
        n[2] = abs(n[2]) + 1.0
        n /= np.linalg.norm(n)
        sel = label == k
        length = rng.uniform(0.6, 1.0, size=(h, w))  # means of unit normals are shorter than 1
        normal[sel] = n * length[sel][:, None]
        depth[sel] = (rng.uniform(2, 50) + rng.uniform(-0.2, 0.2) * xx + rng.uniform(-0.2, 0.2) * yy)[sel]
    depth = np.maximum(depth, 0.5)
    miss = rng.random((h, w)) < miss_frac
    albedo = np.clip(0.5 + 0.3 * np.sin(xx / 3.0)[..., None] * rng.uniform(0.2, 1.0, 3) + 0.1 * rng.normal(size=(h, w, 3)), 0.0, 1.0)
    albedo[rng.random((h, w)) < 0.05] = 0.0  # black channels: demodulated by 1
    signal = 0.3 + 0.2 * np.cos(yy / 5.0)[..., None]
    color = np.maximum(signal * albedo + 0.05 * rng.normal(size=(h, w, 3)), 0.0)
    variance = rng.uniform(1e-4, 5e-3, size=(h, w))
    normal[miss] = 0.0
    albedo[miss] = 0.0
    depth[miss] = INF
    return tuple(np.ascontiguousarray(x, np.float32) for x in (color, variance, albedo, normal, depth))


def oracle_inputs(name, w, h, spp=4, aov_spp=2, seed=None):
    """Denoiser inputs of a shipped scene made on the CPU: the beauty = an oracle render at `spp`, the variance of its pixels' mean luminance
    from `spp` one-sample oracle renders with other seeds, the feature buffers from tests/aov_ref.py.  -> (color, variance, albedo, normal, depth)."""
    import aov_ref
    import oracle_lib as O
    from conftest import get_scene
    seeds = {"back": T.SEED_BACK, "veach-mis": 0x5EED0002, "staircase": T.SEED_STAIRCASE}
    seed = seeds[name] if seed is None else seed
    s = get_scene(name, w, h)
    color, _ = O.render(s.flat, T.make_params(w, h, spp, seed))
    ones = np.stack([O.render(s.flat, T.make_params(w, h, 1, seed + 1 + k))[0].astype(np.float64) @ LUMA for k in range(spp)])
    variance = ones.var(axis=0, ddof=1) / spp
    aov = aov_ref.render_aov(s, T.make_params(w, h, aov_spp, seed))
    return tuple(np.ascontiguousarray(x, np.float32) for x in (color, variance, aov["albedo"], aov["normal"], aov["depth"]))
