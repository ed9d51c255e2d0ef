"""The corpus of tools/shade_case_check (tests/test_shade_cases_cpu.py proves it, tests/test_gpu_shade_cases.py runs it on the GPU) and the layouts of its
case and result files (tools/shade_cases.h).  Everything is seeded numpy; nothing here needs a GPU.

Injecting draws.  A path's stream is (key, ctr) and draw i is mix32(mix32(k1 + i G) ^ k0) >> 8, G = 0x9E3779B9.  trt_mix32 is invertible (odd multipliers,
xor-shifts), so for a chosen k1, counter i and wanted 32-bit word w, k0 = mix32(k1 + i G) ^ mix32_inv(w) makes draw i exactly w >> 8 (key_for).  A second
draw can be fixed only by scanning k1; the keys such scans found are constants below (Q4_KEYS), so the search is not repeated.

The light pickers (sections pick, step, near) read light sets whose selection tables and trees are the CPU builds' own (onelight_lib, nearlights_lib): picker_sets,
picker_cases.  A uniform that puts r = u * total or u * s on a decision value is found by search in binary32 (steer)."""
import numpy as np

U32 = np.uint32
G = 0x9E3779B9
ULP = np.float32(2.0 ** -24)
ONE_M = np.float32(1.0 - 2.0 ** -24)
# the edge uniforms of the issue: 0, 2^-24, 0.25 -+ 2^-24, 0.5, 0.75, 1 - 2^-24
EDGE_U = np.array([0.0, 2.0 ** -24, 0.25 - 2.0 ** -24, 0.25, 0.25 + 2.0 ** -24, 0.5, 0.75, 1.0 - 2.0 ** -24], np.float32)
INV1 = pow(0x7feb352d, -1, 1 << 32)
INV2 = pow(0x846ca68b, -1, 1 << 32)


def mix32(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(U32)


def mix32_inv(y):
    y = np.asarray(y, np.uint64) & 0xFFFFFFFF
    y ^= y >> 16
    y = (y * INV2) & 0xFFFFFFFF
    y ^= y >> 15
    y ^= y >> 30
    y = (y * INV1) & 0xFFFFFFFF
    y ^= y >> 16
    return y.astype(U32)


def rng_u32(k0, k1, i):
    x = mix32(np.asarray(k1, np.uint64) + np.asarray(i, np.uint64) * G)
    return mix32(x ^ np.asarray(k0, U32))


def uniform(k0, k1, i):
    return ((rng_u32(k0, k1, i) >> 8).astype(np.float32) * ULP).astype(np.float32)


def key_for(k1, i, u, low=0):
    """k0 that makes draw i of the stream (k0, k1) the uniform u = m 2^-24 exactly (low: the eight bits below the mantissa, free)."""
    m = np.rint(np.asarray(u, np.float64) * 2.0 ** 24).astype(np.uint64)
    assert (m < 1 << 24).all() and (m.astype(np.float64) * 2.0 ** -24 == np.asarray(u, np.float64)).all(), "not a uniform the stream can produce"
    w = (m << 8) | np.asarray(low, np.uint64)
    return mix32(np.asarray(k1, np.uint64) + np.asarray(i, np.uint64) * G) ^ mix32_inv(w)


def find_q4_keys(count, tiny=2.0 ** -10, start=0):
    """Scan k1 for streams whose draw 1 is exactly 0 (by key_for) and whose draws 2 and 3 are both below `tiny`: what found Q4_KEYS."""
    out = []
    k1 = start
    while len(out) < count:
        ks = np.arange(k1, k1 + (1 << 22), dtype=np.uint64)
        k0 = key_for(ks, 1, np.zeros(len(ks)))
        ok = (uniform(k0, ks, 2) < tiny) & (uniform(k0, ks, 3) < tiny)
        out += [(int(a), int(b)) for a, b in zip(k0[ok], ks[ok].astype(U32))]
        k1 += 1 << 22
    return out[:count]


def make_key(seed, pixel, sample):
    """trt_rng_make_key."""
    def rot(x, r):
        return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & 0xFFFFFFFF
    a = mix32(np.asarray(seed, np.uint64) ^ 0x9E3779B9).astype(np.uint64)
    b = mix32(np.asarray(pixel, np.uint64) + 0x85EBCA6B).astype(np.uint64)
    c = mix32(np.asarray(sample, np.uint64) + 0xC2B2AE35).astype(np.uint64)
    return mix32(a ^ ((b + 0x27D4EB2F) & 0xFFFFFFFF) ^ rot(c, 1)), mix32(rot(a, 7) + b * 0x9E3779B1 + (c ^ 0x165667B1))


# (k0, k1) of streams whose draw 1 is exactly 0 and whose draws 2 and 3 lie below 2^-10 (find_q4_keys(16)): lightSample from ctr = 0 gets r1 = 0 and two tiny
# draws, i.e. an r / rs of Q4 with a tiny divisor.  (r1 = r2 = r3 = 0, the 0 / 0 of Q4, cannot be injected: three fixed draws are 72 bits of conditions on a
# 64-bit key — about 2^-8 keys with that property exist for all streams together — so no stream the renderer can run produces it.)
Q4_KEYS = [(4271726694, 720804), (1129576319, 862862), (4088478871, 4850451), (4021731157, 6474627), (965750348, 8100481), (780109090, 10334862),
           (745056784, 10886311), (230222002, 11494334), (2088730993, 12192403), (3801170436, 14109470), (2056023058, 15963223), (1146558461, 18932065),
           (2142629115, 20043908), (1974214056, 21047420), (494665626, 22392891), (2863071313, 22987036)]
# seeds for which draw 2 of the stream of (seed, pixel 0, sample 7) is exactly TRT_P_RR = 0.8f = 13421773 2^-24 (RR_AT: the path is killed) and the float below
# it (RR_BELOW: it survives); a bounce case reaches the key only through trt_rng_make_key, so these come from a scan of 2^28 seeds
RR_SAMPLE, RR_CTR = 7, 2
RR_AT = [7733993, 28678758, 53525624, 70167207, 72349451, 85430433, 103263577, 113831412, 159259041, 160058084, 164798158, 166101776, 172030054, 184477152, 188633613,
         188647380, 192789681, 224583847, 229502880, 236790709]
RR_BELOW = [269976, 15561620, 51986413, 62521703, 86941425, 117058463, 160493525, 164458841, 189563746, 207726458, 215459147, 221980636, 227300720, 237432257, 239511645,
            261229570]


def find_rr_seeds(m, limit=1 << 28):
    """Seeds below `limit` for which draw RR_CTR of the stream of (seed, pixel 0, sample RR_SAMPLE) is m 2^-24: what found RR_AT (m = 13421773) and RR_BELOW (m - 1)."""
    out = []
    for first in range(0, limit, 1 << 22):
        seed = np.arange(first, first + (1 << 22), dtype=np.uint64)
        k0, k1 = make_key(seed, 0, RR_SAMPLE)
        out += [int(x) for x in seed[(rng_u32(k0, k1, RR_CTR) >> 8) == m]]
    return out


# ---- records (tools/shade_cases.h, trt_path.h) ---------------------------------------------------------------------------------------------------------------
F3 = ("<f4", 3)
RAW_MAT_DT = np.dtype([("Kd", *F3), ("Ks", *F3), ("Tr", *F3), ("Ns", "<f4"), ("Ni", "<f4"), ("radiance", *F3), ("is_emissive", "<i4"), ("tex", "<i4")])
MAT_DT = np.dtype(RAW_MAT_DT.descr + [("Kd_pi", *F3), ("sel_kd", "<f4"), ("sel_kdks", "<f4"), ("rf0", "<f4"), ("Ni_inv", "<f4"), ("no_spec", "<i4")])
TEX_DT = np.dtype([("width", "<i4"), ("height", "<i4"), ("offset", "<u8")])
LIGHT_DT = np.dtype([("mat", "<i4"), ("radiance", *F3), ("area", "<f4"), ("tri_first", "<u4"), ("tri_count", "<u4"), ("pdf", "<f4")])
LTRI_DT = np.dtype([("v", "<f4", (3, 3)), ("vn", "<f4", (3, 3)), ("cum_area", "<f4"), ("pad", "<f4")])
TSHADE_DT = np.dtype([("vn", "<f4", 9), ("vt", "<f4", 6), ("mat", "<i4")])
TISECT_DT = np.dtype([("v0", *F3), ("e1", *F3), ("e2", *F3), ("tol", "<f4"), ("flags", "<u4"), ("pad", "<f4")])
PRIM_DT = np.dtype([("op", "<u4"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4")])
CAM_DT = np.dtype([("cam", "<f4", 12), ("W", "<i4"), ("H", "<i4"), ("i", "<i4"), ("j", "<i4"), ("u1", "<f4"), ("u2", "<f4"), ("mode", "<u4"), ("pad", "<u4")])
VERT_DT = np.dtype([("o", *F3), ("d", *F3), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("pad", "<u4", 3), ("ts", TSHADE_DT)])
LIGHTC_DT = np.dtype([("P", *F3), ("pn", *F3), ("wi", *F3), ("Kd", *F3), ("mat", "<u4"), ("li", "<u4"), ("k0", "<u4"), ("k1", "<u4"), ("ctr", "<u4"), ("flags", "<u4"),
                      ("light0_area", "<f4"), ("pad", "<u4")])
NEXT_DT = np.dtype([("pn", *F3), ("I", *F3), ("mat", "<u4"), ("k0", "<u4"), ("k1", "<u4"), ("ctr", "<u4"), ("pad", "<u4", 2)])
DIR_DT = np.dtype([("op", "<u4"), ("a", *F3), ("b", *F3), ("x", "<f4"), ("y", "<f4"), ("type", "<i4"), ("pad", "<u4", 2)])
BOUNCE_DT = np.dtype([("o", *F3), ("d", *F3), ("pid", "<u4"), ("meta", "<u4"), ("beta", *F3), ("bt_w", "<f4"), ("t", "<f4"), ("tri", "<i4"), ("u", "<f4"), ("v", "<f4"),
                      ("flags", "<u4"), ("max_depth", "<i4"), ("seed", "<u4"), ("s0", "<u4")])
SIZES = dict(mat=96, tex=16, light=32, ltri=80, tshade=64, tisect=48, prim=16, cam=80, vert=112, lightc=80, next=48, dir=48, bounce=80)
for _n, _d in dict(mat=MAT_DT, tex=TEX_DT, light=LIGHT_DT, ltri=LTRI_DT, tshade=TSHADE_DT, tisect=TISECT_DT, prim=PRIM_DT, cam=CAM_DT, vert=VERT_DT, lightc=LIGHTC_DT,
                   next=NEXT_DT, dir=DIR_DT, bounce=BOUNCE_DT).items():
    assert _d.itemsize == SIZES[_n], (_n, _d.itemsize)
# the light pickers: a light-tree node (trt_path.h LightNode), a light set, the three case records
NODE_DT = np.dtype([("lo0", *F3), ("hi0", *F3), ("lo1", *F3), ("hi1", *F3), ("w0", "<f4"), ("w1", "<f4"), ("child0", "<u4"), ("child1", "<u4")])
SET_DT = np.dtype([("light_first", "<u4"), ("n_lights", "<u4"), ("sel_first", "<u4"), ("node_first", "<u4"), ("n_nodes", "<u4"), ("root", "<u4"), ("pad", "<u4", 2)])
PICK_DT = np.dtype([("op", "<u4"), ("set", "<u4"), ("u", "<f4"), ("k0", "<u4"), ("k1", "<u4"), ("ctr", "<u4"), ("li", "<u4"), ("pad", "<u4")])
STEP_DT = np.dtype([("node", NODE_DT), ("P", *F3), ("u", "<f4"), ("inv_p", "<f4"), ("pad", "<u4", 3)])
NEAR_DT = np.dtype([("set", "<u4"), ("P", *F3), ("k0", "<u4"), ("k1", "<u4"), ("ctr", "<u4"), ("pad", "<u4")])
assert (NODE_DT.itemsize, SET_DT.itemsize, PICK_DT.itemsize, STEP_DT.itemsize, NEAR_DT.itemsize) == (64, 32, 32, 96, 32)
LEAF, NONE, NO_TABLE = 0x80000000, 0xFFFFFFFF, 0xFFFFFFFF
PICK_AT_TABLE, PICK_AT_SCAN, PICK_TABLE, PICK_SCAN, PICK_WEIGHT = range(5)
SECTIONS = ("prim", "cam", "vert", "light", "next", "dir", "bounce", "pick", "step", "near")
WORDS = dict(prim=4, cam=6, vert=9, light=9, next=8, dir=3, bounce=17, pick=4, step=2, near=4)
MAGIC, MAGIC_1 = 0x53434332, 0x53434331  # MAGIC_1: the layout from before the light pickers, still read
OP_SINCOS, OP_LOG, OP_EXP, OP_POW, OP_RNG, OP_SQRT, OP_DIV = range(7)
DIGEST_NS = np.array([1.5, 2.0, 10.0, 250.0, 500.0, 1000.0, 1.0e4, 1.0e6], np.float32)
DIGEST_CHUNK = 4096
# (name, first input: numerator of the uniform or bits of the float, chunks) of every digest stream, in the tool's order
DIGEST_STREAMS = ([("sincos2pi(u)", 0, 4096), ("sqrt(u)", 0, 4096), ("sqrt(1-u)", 0, 4096)] + [(f"pow01(u, 1/({ns}+1))", 0, 4096) for ns in DIGEST_NS] +
                  [(f"pow01(u, {ns})", 0, 4096) for ns in DIGEST_NS] +
                  [("logf on [2^-126, 2^-125)", 0x00800000, 2048), ("expf_neg on [-88, -86)", 0xC2AC0000, 64), ("sqrt on exponent fields 30..34", 30 << 23, 5 * 2048),
                   ("sqrt on exponent fields 252..255", 252 << 23, 4 * 2048), ("logf on (i + 1/2) 2^-20", 0, 256), ("expf_neg on -87 (i + 1/2) 2^-20", 0, 256),
                   ("sqrt on the bit patterns mix32(i)", 0, 256)] +
                  [(f"lightPickAt on the table of {n} lights", 0, 4096) for n in (2, 7, 64, 256)] + [(f"lightPickAt by scan of {n} lights", 0, 4096) for n in (2, 7)] +
                  [(f"lightNodeStep, {what}", 0, 4096) for what in ("ordinary importances", "a subnormal importance", "the fall-back by power", "two equal children")])
# (the tool's mode `digest` writes the first 26 streams, `digest-pickers` the ten of the pickers)
DIGEST_OLD_STREAMS = DIGEST_PICK0 = len(DIGEST_STREAMS) - 10
DIGEST_SCAN0, DIGEST_STEP0 = DIGEST_PICK0 + 4, DIGEST_PICK0 + 6
DIGEST_TOTAL = sum(s[2] for s in DIGEST_STREAMS)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(U32)


def pack_meta(ctr, typ, depth):
    return (np.asarray(ctr, U32) & U32(0xFFFF)) | ((np.asarray(typ, U32) & U32(3)) << U32(16)) | (np.asarray(depth, U32) << U32(20))


def unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cat(parts, dt):
    return np.concatenate([np.asarray(p, dt) for p in parts]) if parts else np.zeros(0, dt)


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------------------------
TEX_SIZES = [(1, 1), (1, 7), (7, 1), (3, 5), (256, 256)]  # width x height
M_DIFFUSE, M_GLOSSY, M_GLASS, M_TEX0 = 0, 1, 2, 3
M_EMISSIVE, M_NS1, M_NS1U, M_NS1000, M_NSBIG, M_DENSE = 8, 9, 10, 11, 12, 13
N_MAT = 14
# lights: 0 one triangle; 1 two, CDF 1/2, 1; 2: 33 triangles, CDF k/64 (ends at 33/64 of its area 1: a draw beyond picks nothing); 3 none; 4 normals that
# interpolate to zero; 5 three triangles of area 2.5; 6 a point at the origin (every sample is the origin: chosen distances and angles)
L_ONE, L_TWO, L_33, L_NONE, L_ZERO_N, L_THREE, L_POINT = range(7)


def tables(make_material_dev):
    """-> dict of the file's tables.  make_material_dev: hostsim_lib.make_material_dev (the derived fields are the library's own makeMaterialDev)."""
    rng = np.random.default_rng(7)
    raw = np.zeros(N_MAT, RAW_MAT_DT)
    raw["Ni"], raw["Ns"], raw["tex"] = 1.0, 10.0, -1
    raw["Kd"][M_DIFFUSE] = (0.7, 0.6, 0.5)
    raw["Kd"][M_GLOSSY], raw["Ks"][M_GLOSSY], raw["Ns"][M_GLOSSY] = 0.4, 0.3, 50.0
    raw["Kd"][M_GLASS], raw["Ks"][M_GLASS], raw["Tr"][M_GLASS], raw["Ns"][M_GLASS], raw["Ni"][M_GLASS] = 0.2, 0.2, 0.9, 100.0, 1.5
    for k in range(5):
        raw["Kd"][M_TEX0 + k], raw["tex"][M_TEX0 + k] = 0.5, k
    raw["radiance"][M_EMISSIVE], raw["is_emissive"][M_EMISSIVE] = (10.0, 8.0, 6.0), 1
    for m, ns in ((M_NS1, 1.0), (M_NS1U, np.nextafter(np.float32(1), np.float32(2))), (M_NS1000, 1000.0), (M_NSBIG, 3.0e38)):
        raw["Kd"][m], raw["Ks"][m], raw["Ns"][m] = (0.3, 0.4, 0.5), (0.5, 0.4, 0.3), ns
    raw["Kd"][M_DENSE], raw["Ks"][M_DENSE], raw["Tr"][M_DENSE], raw["Ns"][M_DENSE], raw["Ni"][M_DENSE] = 0.1, 0.3, 0.8, 20.0, 2.4
    mat = make_material_dev(raw).view(MAT_DT)
    assert mat["sel_kd"][M_DIFFUSE] == 1.0 and mat["no_spec"][M_DIFFUSE] == 1 and mat["no_spec"][M_GLOSSY] == 0
    # the lobe thresholds of these materials on values a draw can take exactly
    for m in (M_GLOSSY, M_NS1):
        mat["sel_kd"][m], mat["sel_kdks"][m] = 0.5, 0.75
    tex = np.zeros(len(TEX_SIZES), TEX_DT)
    off = 0
    for k, (w, h) in enumerate(TEX_SIZES):
        tex[k] = (w, h, off)
        off += (w * h * 3 + 15) // 16 * 16
    texbytes = rng.integers(0, 256, off, dtype=np.uint8)
    counts = [1, 2, 33, 0, 1, 3, 1]
    lights = np.zeros(len(counts), LIGHT_DT)
    ltri = np.zeros(sum(counts), LTRI_DT)
    first = 0
    for li, n in enumerate(counts):
        lights[li] = (M_EMISSIVE, (10.0, 8.0, 6.0), 2.5 if li == L_THREE else 1.0, first, n, 0.0)
        for k in range(n):
            c = np.array([rng.uniform(-1.5, 1.5), 5.0, rng.uniform(-1.5, 1.5)])
            ltri["v"][first + k] = c + rng.uniform(-0.5, 0.5, (3, 3)) * (1.0, 0.02, 1.0)
            ltri["vn"][first + k] = (0.0, -1.0, 0.0) + rng.uniform(-0.1, 0.1, (3, 3))
            ltri["cum_area"][first + k] = {L_ONE: 1.0, L_TWO: (k + 1) / 2, L_33: (k + 1) / 64, L_ZERO_N: 1.0, L_THREE: (0.75, 1.5, 2.5)[k % 3], L_POINT: 1.0}[li]
        if li == L_ZERO_N:
            ltri["vn"][first] = 0.0
        if li == L_POINT:
            ltri["v"][first], ltri["vn"][first] = 0.0, (0.0, -1.0, 0.0)
        first += n
    lights["pdf"] = np.float32(1.0) / lights["area"]
    # the triangles of the bounce cases: one per kind of material
    tri_mats = [M_DIFFUSE, M_GLOSSY, M_GLASS, M_TEX0 + 3, M_EMISSIVE, M_NS1, M_DENSE, M_TEX0 + 4]
    tshade, tisect = np.zeros(len(tri_mats), TSHADE_DT), np.zeros(len(tri_mats), TISECT_DT)
    for k, m in enumerate(tri_mats):
        n = unit(rng, 1)[0]
        tshade[k] = ((np.tile(n, 3) + rng.uniform(-0.05, 0.05, 9)).astype(np.float32), rng.uniform(-2, 2, 6).astype(np.float32), m)
        e1 = np.cross(n, unit(rng, 1)[0]).astype(np.float32)
        e2 = np.cross(n, e1).astype(np.float32)
        tisect[k] = (rng.uniform(-1, 1, 3), e1, e2, 1e-5, (m << 8) | (1 if m == M_EMISSIVE else 0), 0.0)
    return dict(mat=mat, tex=tex, texbytes=texbytes, light=lights, ltri=ltri, tshade=tshade, tisect=tisect)


# ---- the sections ----------------------------------------------------------------------------------------------------------------------------------------------
def prim_cases():
    """sincos2pi on the edge uniforms; logf on a stratified 2^17 of (0, 1] and the ends of its domain; expf_neg on a stratified 2^17 of [-87, 0], -88 and the
    flush boundary; pow01 at the flush boundary of either factor; the key and two draws of 2^16 (seed, pixel, sample); the sqrt family on 2^17 random bit patterns
    and the floats next to trt_exact_domain's ends; trt_div_by on the pixel-grid operands of the camera section's sizes.  (The exhaustive ranges of the issue —
    every float of [2^-126, 2^-125) for logf, of [-88, -86] for expf_neg, of the exponent fields within 2 of trt_exact_domain's ends for the square roots — and
    the 2^20-point sweeps are digest streams: 91 M inputs are not written to a file.)"""
    rng = np.random.default_rng(11)
    P = []

    def add(op, a, b=0, c=0):
        a = np.atleast_1d(a)
        r = np.zeros(len(a), PRIM_DT)
        r["op"], r["a"], r["b"], r["c"] = op, a, b, c
        P.append(r)
    add(OP_SINCOS, bits(EDGE_U))
    add(OP_SINCOS, bits((rng.integers(0, 1 << 24, 1 << 12) * 2.0 ** -24).astype(np.float32)))
    n = 1 << 17
    strat = ((np.arange(n) + rng.random(n)) / n)
    add(OP_LOG, bits(np.maximum(strat, 2.0 ** -126).astype(np.float32)))
    add(OP_LOG, bits(np.array([2.0 ** -126, np.nextafter(np.float32(2.0 ** -126), np.float32(1)), ONE_M, 1.0, 0.5, 0.70710677, 0.70710683, 0.7071067], np.float32)))
    add(OP_EXP, bits((-87.0 * strat).astype(np.float32)))
    edge = np.float32(-87.0)
    add(OP_EXP, bits(np.array([-88.0, -0.0, 0.0, -1e-45, -np.inf, np.nan] + [np.nextafter(edge, np.float32(s)) for s in (-100, 0)] + [edge, -87.3365, -87.33655, -86.99], np.float32)))
    # pow01: x at and around FLT_MIN (the `x > 1.17549435e-38f` cut), at and around 1; y log x at and around -87 (expf_neg's flush) for every Ns of the sweeps
    xs = np.array([0.0, 1e-45, 1.17549421e-38, 1.17549435e-38, 1.17549449e-38, ONE_M, 1.0, np.nextafter(np.float32(1), np.float32(2)), 0.5], np.float32)
    ys = np.concatenate([DIGEST_NS, (np.float32(1) / (DIGEST_NS + np.float32(1))).astype(np.float32), np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38, 1e-3], np.float32)])
    xx, yy = np.meshgrid(xs, ys)
    add(OP_POW, bits(xx.ravel()), bits(yy.ravel()))
    for ns in np.concatenate([DIGEST_NS, np.array([1.0000001, 3.0], np.float32)]):
        x0 = np.float32(np.exp(-87.0 / float(ns)))  # y log x = -87 here: 64 floats either side
        if not (1.2e-38 < x0 < 1.0):
            continue
        xb = (bits(np.array([x0]))[0].astype(np.int64) + np.arange(-64, 65)).astype(U32)
        add(OP_POW, xb, bits(np.full(len(xb), ns, np.float32)))
    m = 1 << 16
    add(OP_POW, bits(rng.random(m).astype(np.float32)), bits(rng.choice(ys, m).astype(np.float32)))
    add(OP_RNG, rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(U32), rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(U32), rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(U32))
    add(OP_RNG, np.array([0, 0xFFFFFFFF, 0, 1], U32), np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0], U32), np.array([0, 0xFFFFFFFF, 1, 0], U32))
    add(OP_SQRT, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32))
    ends = np.concatenate([(np.int64(e) << 23) + np.arange(-32, 33) for e in (0, 1, 32, 255)] + [np.array([0x80000000, 0x3F800000, 0x7F7FFFFF, 0x7FC00000, 0xFF800000])])
    add(OP_SQRT, ends.astype(U32))
    # trt_div_by: a an integer in [0, b] or u - 1/2 (m 2^-24), b = W - 1 or W of the camera section's sizes
    for b in (1, 2, 3, 1079, 1080, 1919, 1920, 65535, 65536):
        a = np.concatenate([np.unique(np.clip(np.concatenate([np.arange(0, 4), b - np.arange(0, 4), rng.integers(0, b + 1, 64)]), 0, b)).astype(np.float32),
                            (EDGE_U.astype(np.float64) - 0.5).astype(np.float32), (rng.integers(0, 1 << 24, 256) * 2.0 ** -24 - 0.5).astype(np.float32)])
        add(OP_DIV, bits(a), b)
    return cat(P, PRIM_DT)


CAM_SIZES = (1, 2, 3, 1080, 1920, 65536)


def cam_cases():
    """Pixel grids of W, H in CAM_SIZES: every corner pixel x the jitter draws 0 and 1 - 2^-24 x the three branches (fixed pixels; the grid reciprocals, where
    2 <= W, H; plain divisions), then random pixels with random and edge draws; a generic camera and one whose eye lies on the lower left corner (the direction of pixel (H, 0) with u = 1/2 cancels to 0)."""
    rng = np.random.default_rng(13)
    cams = np.array([[0.1, 1.2, 4.0, -1.3, 0.1, 2.0, 2.6, 0.0, 0.1, 0.0, 2.2, 0.05], [-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 2.0, 0.0, 0.0, 0.0, 2.0, 0.0]], np.float32)
    rows = []
    for W in CAM_SIZES:
        for H in CAM_SIZES:
            for mode in (0, 1, 2):
                if mode == 1 and (W < 2 or H < 2):
                    continue
                i = np.concatenate([np.repeat([0, H - 1, 0, H - 1, H], 4), rng.integers(0, H, 40)])
                j = np.concatenate([np.repeat([0, 0, W - 1, W - 1, 0], 4), rng.integers(0, W, 40)])
                u1 = np.concatenate([np.tile([0.0, 0.0, ONE_M, ONE_M], 5), rng.choice(EDGE_U, 20), (rng.integers(0, 1 << 24, 20) * 2.0 ** -24)]).astype(np.float32)
                u2 = np.concatenate([np.tile([0.0, ONE_M, 0.0, ONE_M], 5), rng.choice(EDGE_U, 20), (rng.integers(0, 1 << 24, 20) * 2.0 ** -24)]).astype(np.float32)
                for c in range(2):
                    r = np.zeros(len(i), CAM_DT)
                    r["cam"], r["W"], r["H"], r["i"], r["j"], r["u1"], r["u2"], r["mode"] = cams[c], W, H, i, j, u1, u2, mode
                    rows.append(r)
    # the eye on llc, the sample on llc: Q1's row H with u2 = 1/2 and column 0 with u1 = 1/2 give s = t = 0 in the parity branches
    r = np.zeros(3 * 36, CAM_DT)
    k = 0
    for W in CAM_SIZES:
        for H in CAM_SIZES:
            for mode in (1, 2, 0):
                if mode == 1 and (W < 2 or H < 2):
                    mode = 2
                r[k] = (cams[1], W, H, H if mode else H - 1, 0, 0.5 if mode else 0.0, 0.5 if mode else 0.0, mode, 0)
                k += 1
    rows.append(r)
    return cat(rows, CAM_DT)


def vert_cases(tb):
    """makeVertex.  With u = v = 0 the texture coordinate is (vt[0], vt[1]) exactly, so the first groups choose it: on texel boundaries k / width and the floats
    around them, on integers, negative, -eps (wraps to just below 1) and -2^-60 (wraps to 1.0: the upper clamp), 1e7 (fract 0), 1 - 2^-24, +-inf and NaN (the lower clamp
    on the CPU build: (int) of a NaN is the most negative int there, 0 on gfx950 — either way texel 0), for every texture; then random barycentrics, coordinates and normals, a zero
    normal and an untextured material among them."""
    rng = np.random.default_rng(17)
    rows = []
    special = np.array([0.0, -0.0, 1.0, 2.0, -1.0, -3.0, -1e-9, -2.0 ** -60, 1e7, -1e7, ONE_M, np.nextafter(np.float32(1), np.float32(2)), np.inf, -np.inf, np.nan, 0.5, 1e-45, -1e-45], np.float32)
    for k, (w, h) in enumerate(TEX_SIZES):
        edges = []
        for n in sorted({w, h}):
            base = (np.arange(0, n + 1) / n).astype(np.float32)
            for shift in (0.0, 1.0, -1.0, 5.0, 100.0):
                b = bits((base + np.float32(shift)).astype(np.float32)).astype(np.int64)
                edges.append(np.concatenate([(b + d).astype(U32).view(np.float32) for d in range(-3, 4)]))
        coords = np.unique(np.concatenate([special] + edges).view(U32)).view(np.float32)
        if len(coords) > 600:
            coords = np.concatenate([special, rng.choice(coords, 600 - len(special), replace=False)])
        cc, rr = np.meshgrid(coords, np.concatenate([special, rng.choice(coords, 12)]))
        r = np.zeros(cc.size, VERT_DT)
        r["ts"]["vt"][:, 0], r["ts"]["vt"][:, 1] = cc.ravel(), rr.ravel()
        r["ts"]["vn"][:, :3] = (0.0, 1.0, 0.0)
        r["ts"]["mat"] = M_TEX0 + k
        r["o"], r["d"], r["t"] = rng.uniform(-1, 1, (len(r), 3)), unit(rng, len(r)), rng.uniform(0.1, 10, len(r))
        rows.append(r)
    n = 60000
    r = np.zeros(n, VERT_DT)
    r["o"], r["d"], r["t"] = rng.uniform(-5, 5, (n, 3)), unit(rng, n), rng.uniform(0.001, 50, n)
    r["u"], r["v"] = rng.random(n), rng.random(n)
    flip = r["u"] + r["v"] > 1
    r["u"][flip], r["v"][flip] = 1 - r["u"][flip], 1 - r["v"][flip]
    edge = rng.random(n) < 0.1
    r["u"][edge] = rng.choice(np.array([0.0, 1.0, ONE_M, 2.0 ** -24], np.float32), edge.sum())
    r["v"][edge] = 0.0
    base = unit(rng, n)
    r["ts"]["vn"] = (np.tile(base, 3) + rng.uniform(-0.2, 0.2, (n, 9))).astype(np.float32)
    r["ts"]["vn"][rng.random(n) < 0.01] = 0.0
    r["ts"]["vt"] = rng.uniform(-3, 3, (n, 6)) * rng.choice([1.0, 1.0, 100.0], (n, 1))
    r["ts"]["mat"] = rng.choice([M_TEX0, M_TEX0 + 1, M_TEX0 + 2, M_TEX0 + 3, M_TEX0 + 4, M_TEX0 + 4, M_DIFFUSE], n)
    rows.append(r)
    return cat(rows, VERT_DT)


def _light_rows(n, rng):
    r = np.zeros(n, LIGHTC_DT)
    r["P"] = rng.uniform((-2, 0, -2), (2, 3, 2), (n, 3))
    r["pn"], r["wi"] = unit(rng, n), unit(rng, n)
    r["pn"][:, 1] = np.abs(r["pn"][:, 1]) * rng.choice([1.0, 1.0, 1.0, -1.0], n)
    r["Kd"] = rng.random((n, 3))
    r["k0"], r["k1"] = rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64)
    r["ctr"] = rng.integers(0, 64, n)
    r["flags"] = rng.integers(0, 4, n)
    r["light0_area"] = 1.0
    r["mat"] = rng.choice([M_DIFFUSE, M_GLOSSY, M_NS1, M_NS1U, M_NS1000, M_NSBIG, M_TEX0 + 3], n)
    return r


def light_cases(tb):
    """lightSample.  (A) random vertices, streams, materials and lights x parity / fixed x bisection / scan; (B) the CDF draw ON a cumulative area and one draw
    below it, for every triangle of the lights of 2 and 33 (the strict `<`), and beyond the last one; (C) Q4_KEYS: r1 = 0 with two tiny draws; (D) the point light at the
    origin: distances 0, 1e-20 (squares denormal), 1e19 and 2e19 (squares overflow), 1.001 |x' - x| and 0.999 |x' - x| on the floats around TRT_INF, cos_s = +0, -0 and
    +-one denormal, cos_alpha on random directions with pn = wi = wo (a rounding error either side of 1) and at denormal size, for Ns = 1, 1 + ulp, 1000, 3e38;
    (E) normals that interpolate to zero, the empty light."""
    rng = np.random.default_rng(19)
    rows = []
    n = 120000
    r = _light_rows(n, rng)
    r["li"] = rng.choice([L_ONE, L_TWO, L_33, L_33, L_NONE, L_ZERO_N, L_THREE, L_THREE], n)
    r["light0_area"] = rng.choice(np.array([1.0, 2.5, 0.5], np.float32), n)
    rows.append(r)
    # (B) light0_area = area = 1: rnd is the draw itself
    for li, cnt, den in ((L_TWO, 2, 2), (L_33, 33, 64)):
        cum = (np.arange(1, cnt + 1) / den).astype(np.float32)
        u = np.concatenate([cum[cum < 1], cum - ULP, np.array([0.0], np.float32)] + ([np.array([40 / 64, ONE_M], np.float32)] if li == L_33 else []))
        u = np.repeat(u, 16)
        r = _light_rows(len(u), rng)
        r["li"], r["flags"] = li, np.tile(np.arange(4), len(u) // 4)
        r["k0"] = key_for(r["k1"], r["ctr"], u)
        rows.append(r)
    # (C)
    r = _light_rows(len(Q4_KEYS) * 16, rng)
    r["k0"], r["k1"] = np.repeat(np.array(Q4_KEYS, np.uint64)[:, 0], 16), np.repeat(np.array(Q4_KEYS, np.uint64)[:, 1], 16)
    r["ctr"], r["flags"], r["li"] = 0, np.tile([0, 2], len(r) // 2), np.tile(np.repeat([L_ONE, L_THREE], 2), len(r) // 4)
    r["light0_area"] = np.where(r["li"] == L_THREE, 2.5, 1.0)
    rows.append(r)
    # (D)
    dirs = unit(rng, 4096)
    r = _light_rows(len(dirs), rng)
    r["li"], r["P"], r["pn"], r["wi"] = L_POINT, -dirs * rng.choice(np.array([1.0, 3.0, 0.37, 1e3], np.float32), (len(dirs), 1)), -dirs, -dirs
    r["mat"] = np.tile([M_GLOSSY, M_NS1, M_NS1U, M_NS1000, M_NSBIG, M_DIFFUSE, M_GLOSSY, M_NS1000], len(r) // 8)
    r["pn"], r["wi"] = dirs, dirs  # wo = normalize(0 - P) = dirs up to rounding: cos_alpha = dot(pn, normalize(wo)) lands either side of 1
    r["P"] = -dirs * rng.choice(np.array([1.0, 3.0, 0.37, 1e3], np.float32), (len(dirs), 1))
    rows.append(r)
    dist = np.concatenate([np.array([0.0, 1e-20, 1e19, 2e19, 1e-30, 3e-23], np.float32)] +
                          [(bits(np.array([np.float32(114514.0) / np.float32(f)]))[0].astype(np.int64) + np.arange(-12, 13)).astype(U32).view(np.float32) for f in (1.001, 0.999)])
    for pn in ([1.0, 0.0, 0.0], [-1.0, -0.0, -0.0], [1.0, 1e-45, 0.0], [1.0, -1e-45, 0.0], [0.0, 1.0, 0.0], [1.0, 1e-42, 0.0], [0.6, 0.8, 0.0]):
        for mats in ([M_GLOSSY, M_NS1, M_NS1U, M_NS1000], [M_NSBIG, M_DIFFUSE, M_TEX0 + 3, M_GLOSSY]):
            r = _light_rows(len(dist) * 4, rng)
            r["li"], r["mat"] = L_POINT, np.tile(mats, len(dist))
            r["P"] = np.repeat(dist, 4)[:, None] * np.array([0.0, -1.0, 0.0], np.float32)  # wo = (0, 1, 0)
            r["P"][:, 0], r["P"][:, 2] = 0.0, 0.0
            r["pn"], r["wi"] = np.array(pn, np.float32), np.array([0.0, 1.0, 0.0], np.float32)
            rows.append(r)
    for sc in (1.0, 1e-20, 1e19, 2e19):  # the same distances along a diagonal: three squares to add
        r = _light_rows(64, rng)
        r["li"], r["P"], r["pn"] = L_POINT, np.float32(sc) * np.array([-1.0, -1.0, -1.0], np.float32), unit(rng, 64)
        rows.append(r)
    # (E)
    r = _light_rows(512, rng)
    r["li"] = np.tile([L_ZERO_N, L_NONE], 256)
    rows.append(r)
    return cat(rows, LIGHTC_DT)


def fresnel_of(rf0, cos_in):
    """nextRayDecide's Schlick term, operation for operation in binary32."""
    rf0, cos_in = np.float32(rf0), np.asarray(cos_in, np.float32)
    x = np.float32(1) - np.abs(cos_in)
    x2 = x * x
    return rf0 + (np.float32(1) - rf0) * ((x2 * x2) * x)


def _next_rows(n, rng):
    r = np.zeros(n, NEXT_DT)
    r["pn"], r["I"] = unit(rng, n), unit(rng, n)
    r["k0"], r["k1"] = rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64)
    r["ctr"] = rng.integers(0, 64, n)
    return r


def next_cases(tb):
    """nextRayDecide + nextRayFinish.  (A) random normals, directions, streams over the diffuse, glossy, Ns = 1 and the two refracting materials; (B) Fresnel:
    pn = e_y and I = (sin, -+cos, 0) at grazing angles where the Schlick term lies in [1/2, 1) — a multiple of 2^-24, so the draw can equal it — with the draw on it
    and one ulp either side; (C) the lobe draw on sel_kd = 1/2 and sel_kdks = 3/4 and one ulp below each, for Ns = 50 and Ns = 1, and sel_kd == 1 (the draw is
    counted, not generated); (D) cos_in = +0, -0 and denormal on the refracting materials, with the largest draw; (E) edge uniforms as u_phi (the diffuse material: draw ctr + 1); (F) the specular lobe (lobe draw 5/8) around reflect(I, pn) with I within a denormal of the surface."""
    rng = np.random.default_rng(23)
    mat = tb["mat"]
    rows = []
    n = 120000
    r = _next_rows(n, rng)
    r["mat"] = rng.choice([M_DIFFUSE, M_GLOSSY, M_GLASS, M_GLASS, M_DENSE, M_DENSE, M_NS1], n)
    rows.append(r)
    for m in (M_GLASS, M_DENSE):
        c = np.concatenate([np.linspace(0.0, 0.12, 200), -np.linspace(0.0, 0.12, 200)]).astype(np.float32)
        f = fresnel_of(mat["rf0"][m], c)
        c, f = c[(f >= 0.5) & (f < ONE_M)], f[(f >= 0.5) & (f < ONE_M)]
        for d in (-1, 0, 1):
            r = _next_rows(len(c), rng)
            r["mat"], r["pn"] = m, (0.0, 1.0, 0.0)
            r["I"] = np.stack([np.sqrt(1 - c.astype(np.float64) ** 2), c, np.zeros(len(c))], 1)
            r["I"][:, 1] = c
            r["k0"] = key_for(r["k1"], r["ctr"], f + np.float32(d) * ULP)
            rows.append(r)
    for m in (M_GLOSSY, M_NS1):
        u = np.repeat(np.array([0.5 - 2.0 ** -24, 0.5, 0.75 - 2.0 ** -24, 0.75, 0.0, ONE_M], np.float32), 128)
        r = _next_rows(len(u), rng)
        r["mat"] = m
        r["k0"] = key_for(r["k1"], r["ctr"], u)
        rows.append(r)
    graze = np.tile(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-20, -1e-20, 1e-7, -1e-7], np.float32), 32)  # reflect(I, pn) as the specular lobe's axis at grazing incidence
    r = _next_rows(len(graze), rng)
    r["mat"], r["pn"] = M_GLOSSY, (0.0, 1.0, 0.0)
    r["I"][:, 1] = graze
    r["k0"] = key_for(r["k1"], r["ctr"], np.full(len(graze), 0.625))
    rows.append(r)
    r = _next_rows(len(EDGE_U) * 64, rng)
    r["mat"] = M_DIFFUSE
    r["k0"] = key_for(r["k1"], r["ctr"] + 1, np.repeat(EDGE_U, 64))
    rows.append(r)
    for I in ([1.0, 0.0, 0.0], [-1.0, -0.0, -1.0], [1.0, 1e-45, 0.0], [1.0, -1e-45, 0.0], [1.0, 1e-30, 0.0], [1.0, -1e-30, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]):
        for m in (M_GLASS, M_DENSE):
            r = _next_rows(32, rng)
            r["mat"], r["pn"], r["I"] = m, (0.0, 1.0, 0.0), np.array(I, np.float32)
            r["k0"] = key_for(r["k1"], r["ctr"], np.full(32, ONE_M))
            rows.append(r)
    return cat(rows, NEXT_DT)


def dir_cases():
    """sampleDir, refract and reflect on explicit arguments.  sampleDir: axes random, with |a.x| == |a.y|, +-e_y, the zero vector, a NaN component x both lobes x
    the Ns of the digest sweeps x EDGE_U^2 and random uniforms; refract: N = e_y, I = (sin, -cos, 0) with cos on the 129 floats around the critical angle of eta = 1.5,
    2.4, 1.33 (k within a few ulps of 0 on both sides), eta = 1 and its neighbours at grazing and normal incidence, random pairs; reflect: grazing and random."""
    rng = np.random.default_rng(29)
    rows = []
    axes = np.concatenate([unit(rng, 24), np.array([[0.5, 0.5, 0.70710677], [0.5, -0.5, 0.70710677], [-0.6, 0.6, 0.52915], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0],
                                                   [0.0, 0.0, 0.0], [np.nan, 0.5, 0.5], [0.3, np.nan, 0.1], [1.0, 0.0, 0.0], [-0.0, -0.0, -1.0]], np.float32)])
    uu = np.stack(np.meshgrid(EDGE_U, EDGE_U), -1).reshape(-1, 2)
    uu = np.concatenate([uu, (rng.integers(0, 1 << 24, (64, 2)) * 2.0 ** -24).astype(np.float32)])
    hostile = ~(np.abs(np.linalg.norm(axes.astype(np.float64), axis=1) - 1) < 1e-6)  # zero and NaN axes: outside the function's domain, every eighth pair of uniforms
    for typ, nss in ((0, DIGEST_NS[:1]), (1, DIGEST_NS)):
        for ns in nss:
            for ax, u2 in ((axes[~hostile], uu), (axes[hostile], uu[::8])):
                r = np.zeros(len(ax) * len(u2), DIR_DT)
                r["op"], r["type"], r["x"] = 0, typ, ns
                r["a"] = np.repeat(ax, len(u2), 0)
                r["y"], r["b"][:, 0] = np.tile(u2[:, 0], len(ax)), np.tile(u2[:, 1], len(ax))
                rows.append(r)
    n = 40000
    r = np.zeros(n, DIR_DT)
    r["op"], r["type"], r["x"], r["a"] = 0, rng.integers(0, 2, n), rng.choice(DIGEST_NS, n), unit(rng, n)
    r["y"], r["b"][:, 0] = rng.integers(0, 1 << 24, n) * 2.0 ** -24, rng.integers(0, 1 << 24, n) * 2.0 ** -24
    rows.append(r)
    for eta in (1.5, 2.4, 1.33, np.float32(1) / np.float32(1.5)):
        eta = np.float32(eta)
        cc = np.sqrt(max(0.0, 1.0 - 1.0 / float(eta) ** 2)) if eta > 1 else 0.5
        c = (bits(np.array([cc], np.float32))[0].astype(np.int64) + np.arange(-64, 65)).astype(U32).view(np.float32)
        for sgn in (1.0, -1.0):
            r = np.zeros(len(c), DIR_DT)
            r["op"], r["x"], r["b"] = 1, eta, (0.0, 1.0, 0.0)
            r["a"] = np.stack([np.sqrt(np.maximum(0.0, 1 - c.astype(np.float64) ** 2)), -sgn * c, np.zeros(len(c))], 1)
            r["a"][:, 1] = -sgn * c
            rows.append(r)
    one = np.float32(1)
    etas = np.array([one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), 1.0000002, 0.9999999], np.float32)
    cs = np.array([0.0, -0.0, 1e-45, 1e-20, 2.4e-4, 3.4e-4, 3.5e-4, 4.9e-4, 1.0, -1.0, ONE_M], np.float32)
    ee, cg = np.meshgrid(etas, cs)
    r = np.zeros(ee.size, DIR_DT)
    r["op"], r["x"], r["b"] = 1, ee.ravel(), (0.0, 1.0, 0.0)
    r["a"][:, 0], r["a"][:, 1] = np.sqrt(np.maximum(0, 1 - cg.ravel().astype(np.float64) ** 2)), -cg.ravel()
    rows.append(r)
    n = 20000
    r = np.zeros(n, DIR_DT)
    r["op"], r["a"], r["b"], r["x"] = 1, unit(rng, n), unit(rng, n), rng.choice(np.array([1.5, 1 / 1.5, 2.4, 1 / 2.4, 1.0], np.float32), n)
    rows.append(r)
    r = np.zeros(n // 2, DIR_DT)
    r["op"], r["a"], r["b"] = 2, unit(rng, n // 2), unit(rng, n // 2)
    g = np.arange(len(r)) % 4 == 0  # grazing: I almost in the plane of N = e_y
    r["b"][g] = (0.0, 1.0, 0.0)
    r["a"][g, 1] = rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-8, -1e-8, 1e-4], np.float32), g.sum())
    rows.append(r)
    return cat(rows, DIR_DT)


def bounce_cases(tb):
    """shadeBegin -> shadeNext on a queued ray record and its hit record, over the triangles of tables() (diffuse, glossy, glass, two textured, emissive, Ns = 1,
    dense glass) and misses, x depth 0, 1, 2, 5 x ray type x max_depth 0 (none), 1, 3, 6 x ray_offset x specular_ks; RR_AT / RR_BELOW put the roulette draw on 0.8 and on the
    float below it."""
    rng = np.random.default_rng(31)
    n = 100000
    n_tri = len(tb["tshade"])
    r = np.zeros(n, BOUNCE_DT)
    r["o"], r["d"], r["t"] = rng.uniform(-3, 3, (n, 3)), unit(rng, n), rng.uniform(0.01, 20, n)
    r["pid"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    r["meta"] = pack_meta(rng.integers(0, 200, n), rng.integers(0, 4, n), rng.choice([0, 1, 2, 5], n))
    r["beta"] = rng.random((n, 3))
    r["tri"] = rng.choice(np.concatenate([[-1], np.arange(n_tri), np.arange(n_tri)]), n)
    r["u"], r["v"] = rng.random(n) * 0.5, rng.random(n) * 0.5
    r["flags"], r["max_depth"] = rng.integers(0, 4, n), rng.choice([0, 0, 1, 3, 6], n)
    r["seed"], r["s0"] = rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 16, n)
    rows = [r]
    for seeds in (RR_AT, RR_BELOW):
        if not seeds:
            continue
        q = np.zeros(len(seeds) * 8, BOUNCE_DT)
        q[:] = r[:len(q)]
        q["seed"], q["s0"], q["pid"] = np.repeat(np.array(seeds, np.uint64), 8), RR_SAMPLE, 0
        q["meta"], q["max_depth"] = pack_meta(RR_CTR, 3, 0), 0
        q["tri"] = np.tile([0, 1, 2, 3, 5, 6, 7, 0], len(seeds))
        rows.append(q)
    return cat(rows, BOUNCE_DT)


# ---- the light pickers -------------------------------------------------------------------------------------------------------------------------------------------
class LightSets:
    """The pools of a case file's light sets.  A set's selection table is the CPU build's own lightSelTable (onelight_lib.pick), its tree the CPU build's
    buildLightTree (nearlights_lib.tree) or hand-made nodes; `info` keeps what the tests restate from."""

    def __init__(self):
        self.lights, self.sel, self.nodes, self.sets, self.info = [], [], [], [], []
        self.n_l = self.n_s = self.n_n = 0

    def add(self, name, area, radiance, nodes=None, root=NONE, built=True):
        import onelight_lib as OL
        area = np.ascontiguousarray(area, np.float32).reshape(-1)
        radiance = np.ascontiguousarray(radiance, np.float32).reshape(-1, 3)
        n = len(area)
        L = np.zeros(n, LIGHT_DT)
        L["radiance"], L["area"] = radiance, area
        cdf = OL.pick(area, radiance, np.zeros(1, np.float32))["cdf"]
        nodes = np.zeros(0, NODE_DT) if nodes is None else np.ascontiguousarray(nodes).view(NODE_DT).reshape(-1)
        rec = np.zeros(1, SET_DT)
        rec["light_first"], rec["n_lights"], rec["sel_first"], rec["node_first"], rec["n_nodes"], rec["root"] = self.n_l, n, self.n_s, self.n_n, len(nodes), root
        self.lights.append(L), self.sel.append(cdf), self.nodes.append(nodes), self.sets.append(rec)
        self.n_l, self.n_s, self.n_n = self.n_l + n, self.n_s + n, self.n_n + len(nodes)
        self.info.append(dict(name=name, n=n, area=area, radiance=radiance, w=OL.weights(area, radiance), cdf=cdf, nodes=nodes, root=int(root), built=built))
        return len(self.sets) - 1

    def add_tables(self, name, t):
        import nearlights_lib as NL
        if t.n == 0:
            return self.add(name, t.area, t.radiance)
        nodes, root, _ = NL.tree(t)
        return self.add(name, t.area, t.radiance, nodes, root)

    def pools(self):
        sel = cat(self.sel, np.float32)
        return dict(plights=cat(self.lights, LIGHT_DT), psel=np.concatenate([sel, np.zeros(-len(sel) % 4, np.float32)]), pnodes=cat(self.nodes, NODE_DT), sets=cat(self.sets, SET_DT))


def _chain(children_w, boxes):
    """Hand-made nodes in a chain: node k holds leaf k and node k + 1 (the last one leaves k and k + 1), with the given (w0, w1) and (lo0, hi0, lo1, hi1) per node."""
    n = np.zeros(len(children_w), NODE_DT)
    for k, ((w0, w1), (lo0, hi0, lo1, hi1)) in enumerate(zip(children_w, boxes)):
        last = k == len(n) - 1
        n[k] = (lo0, hi0, lo1, hi1, w0, w1, LEAF | k, LEAF | (k + 1) if last else k + 1)
    return n


BOX_A, BOX_B = ((-1, 2, -1), (1, 2.5, 1)), ((4, 2, 0), (5, 3, 1))
BOX_INVERTED = ((1, 2.5, 1), (-1, 2, -1))  # lo > hi: hi - centre is negative, r2 still a sum of squares
BOX_POINT = ((0.5, 1, 0.5), (0.5, 1, 0.5))
# what buildLightTree cannot produce: weights of 0, negative, NaN and infinity, inverted and empty boxes; three nodes per set
HAND_SETS = {
    "hand: zero and negative weights": ([(0.0, 2.0), (-1.0, -1.0), (3.0, 0.0)], [BOX_A + BOX_B, BOX_A + BOX_B, BOX_B + BOX_A]),
    "hand: NaN and infinite weights": ([(np.nan, 1.0), (np.inf, 1.0), (1.0, np.inf)], [BOX_A + BOX_B, BOX_B + BOX_A, BOX_A + BOX_B]),
    "hand: inverted and empty boxes": ([(2.0, 1.0), (1.0, 2.0), (-2.0, 3.0)], [BOX_INVERTED + BOX_B, BOX_POINT + BOX_INVERTED, BOX_A + BOX_POINT]),
    # a centre at infinity (0.5 lo + 0.5 hi = inf: hi - centre is inf - inf, r2 a NaN beside d2 = inf; with P at the same infinity d2 is inf - inf as well) and a
    # centre that is itself -inf + inf
    "hand: infinite box corners": ([(2.0, 1.0), (1.0, 2.0), (3.0, 1.5)], [((-1, 2, -1), (np.inf, 2.5, 1)) + BOX_B, BOX_A + ((-np.inf, -np.inf, 0), (4, 5, 1)),
                                                                        ((-np.inf, 2, -1), (np.inf, 2.5, 1)) + ((0, 0, 0), (np.inf, np.inf, np.inf))]),
    "hand: both weights zero, both negative": ([(0.0, 0.0), (-0.0, 1e-45), (-3.0, -1e-45)], [BOX_A + BOX_B, BOX_A + BOX_A, BOX_B + BOX_B]),
}
# the strata of P
P_INSIDE, P_CENTRE, P_1E4, P_1E19, P_1E20, P_1E30, P_INF, P_NAN = range(8)
P_FINITE = (P_INSIDE, P_CENTRE, P_1E4, P_1E19, P_1E20, P_1E30)
# the strata of u / of the stream: random; the three edge uniforms; steered onto a decision value, one float below it, one above it; any uniform of a pick case on the
# set `subnormal total`, whose table entries are a few subnormal steps apart (every r = u * total lies within 4 ulp of one: on a decision by construction, like the steered ones)
U_RANDOM, U_ZERO, U_ULP, U_LAST, U_AT, U_BELOW, U_ABOVE, U_SUBNORMAL = range(8)
U_EDGES = ((U_ZERO, np.float32(0)), (U_ULP, ULP), (U_LAST, ONE_M))


def picker_sets():
    """-> LightSets and the names of the sets with a special role."""
    import nearlights_lib as NL
    rng = np.random.default_rng(37)
    S = LightSets()
    for name, t in NL.shared_tables():
        S.add_tables(name, t)
    S.add_tables("hostile", NL.hostile_tables())
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257):
        S.add_tables(f"random, L={n}", NL.random_tables(n, 0xC0DE + n) if n else NL.Tables.quads(np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3)), 1.0))
    n = 1 << 16  # every leaf at depth 16
    S.add_tables("deep", NL.Tables.quads(rng.uniform(0.5, 2.0, n), np.ones((n, 3)), rng.uniform(-100.0, 100.0, (n, 3)), 0.1))
    S.add_tables("no tree light", NL.Tables.quads(np.zeros(5), np.ones((5, 3)), np.zeros((5, 3)), 1.0))
    one = np.zeros(5, np.float32)
    one[3] = 2.0
    S.add_tables("one tree light", NL.Tables.quads(one, np.ones((5, 3)), np.zeros((5, 3)), 1.0))
    n = 64
    along = np.stack([np.arange(n) * 3.0, np.full(n, 2.0), np.zeros(n)], 1)
    S.add_tables("weights from subnormal to 1e30", NL.Tables.quads(10.0 ** np.linspace(-44, 30, n), np.ones((n, 3)), along, 0.5))
    S.add_tables("total +inf", NL.Tables.quads(np.full(4, 3e38), np.ones((4, 3)), along[:4], 0.5))
    S.add_tables("subnormal total", NL.Tables.quads(np.array([3e-45, 0, 4e-45, 1e-44, 0, 0]), np.ones((6, 3)), along[:6], 0.5))
    S.add_tables("absorbed", NL.Tables.quads(np.array([1e-44, 1e30]), np.ones((2, 3)), along[:2], 0.5))
    S.add_tables("points", NL.Tables.quads(rng.uniform(0.5, 2.0, 8), np.ones((8, 3)), rng.uniform(-3.0, 3.0, (8, 3)), 0.0))
    S.add_tables("pair", NL.Tables.quads(np.array([1.0, 2.5]), np.ones((2, 3)), along[:2], 0.5))
    for name, (ws, boxes) in HAND_SETS.items():
        S.add(name, np.array([1.0, 2.0, 0.5, 4.0]), np.ones((4, 3)), _chain(ws, boxes), 0, built=False)
    return S


def step_parts(nd, P):
    """lightNodeStep's importances in binary32, one IEEE operation per operation of trt_path.h -> dict(raw0, raw1, raw_s: as computed; imp0, imp1, s: after the
    fall-back by power; fallback: 0 none, 1 a NaN importance, 2 s == 0, 3 s == inf, 4 a negative importance, 5 other)."""
    f = np.float32
    P = np.asarray(P, f).reshape(-1, 3)

    def child(lo, hi, w):
        c = f(0.5) * lo + f(0.5) * hi
        e, q = hi - c, P - c
        r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        d2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        return (w / np.fmax(d2, r2)).astype(f)
    with np.errstate(all="ignore"):
        raw0, raw1 = child(nd["lo0"], nd["hi0"], nd["w0"]), child(nd["lo1"], nd["hi1"], nd["w1"])
        raw_s = (raw0 + raw1).astype(f)
        ok = (raw0 >= 0) & (raw1 >= 0) & (raw_s > 0) & (raw_s < np.inf)
        nan = np.isnan(raw0) | np.isnan(raw1)
        neg = (raw0 < 0) | (raw1 < 0)
        fallback = np.where(ok, 0, np.where(nan, 1, np.where(neg, 4, np.where(raw_s == 0, 2, np.where(raw_s == np.inf, 3, 5)))))
        imp0, imp1 = np.where(ok, raw0, nd["w0"]).astype(f), np.where(ok, raw1, nd["w1"]).astype(f)
        s = np.where(ok, raw_s, (nd["w0"] + nd["w1"]).astype(f)).astype(f)
    return dict(raw0=raw0, raw1=raw1, raw_s=raw_s, imp0=imp0, imp1=imp1, s=s, fallback=fallback)


def step_f32(nd, P, u, inv_p):
    """lightNodeStep restated in binary32 -> dict(child, inv_p, r, first: before the flip, flipped) and step_parts' fields."""
    f = np.float32
    d = step_parts(nd, P)
    with np.errstate(all="ignore"):
        r = (np.asarray(u, f) * d["s"]).astype(f)
        first = r < d["imp0"]
        flipped = ~(np.where(first, d["imp0"], d["imp1"]) > 0)
        took = first ^ flipped
        d.update(r=r, first=first, flipped=flipped, child=np.where(took, nd["child0"], nd["child1"]).astype(U32),
                 inv_p=(np.asarray(inv_p, f) * (d["s"] / np.where(took, d["imp0"], d["imp1"])).astype(f)).astype(f))
    return d


def steer(target, scale):
    """Uniforms m 2^-24 whose binary32 product with `scale` is `target`, the float below it and the float above it -> [3, n] float32, NaN where none exists."""
    f = np.float32
    target, scale = np.asarray(target, f), np.asarray(scale, f)
    out = np.full((3, len(target)), np.nan, f)
    with np.errstate(all="ignore"):
        ok = (scale > 0) & np.isfinite(scale) & (target > 0) & (target <= scale)
        m0 = np.where(ok, np.rint(target.astype(np.float64) / np.where(ok, scale, 1).astype(np.float64) * 2.0 ** 24), 0).astype(np.int64)
        wants = (target, np.nextafter(target, f(-np.inf)), np.nextafter(target, f(np.inf)))
        for d in (0, -1, 1, -2, 2, -3, 3):
            m = m0 + d
            u = (m.astype(np.float64) * 2.0 ** -24).astype(f)
            r = (u * scale).astype(f)
            for k, want in enumerate(wants):
                hit = ok & (m >= 0) & (m < 1 << 24) & (r == want) & np.isnan(out[k])
                out[k][hit] = u[hit]
    return out


def set_points(info, rng, m):
    """m points of every stratum of P for a set -> (P [k, 3] float32, stratum [k])."""
    nd = info["nodes"]
    boxes = np.concatenate([nd["lo0"], nd["hi0"], nd["lo1"], nd["hi1"]]) if len(nd) else np.zeros((0, 3), np.float32)
    boxes = boxes[np.isfinite(boxes).all(1)]
    lo, hi = (boxes.min(0), boxes.max(0)) if len(boxes) else (np.full(3, -5.0), np.full(3, 5.0))
    inside = rng.uniform(lo - 1.0, hi + 1.0, (m, 3))
    if len(nd):  # the centres of the children's boxes: of single lights at the leaves (a point light's own position where the box is a point)
        k = rng.integers(0, len(nd), m)
        c = rng.integers(0, 2, m) == 0
        f = np.float32
        with np.errstate(invalid="ignore"):
            centre = np.where(c[:, None], f(0.5) * nd["lo0"][k] + f(0.5) * nd["hi0"][k], f(0.5) * nd["lo1"][k] + f(0.5) * nd["hi1"][k])
        centre = np.where(np.isfinite(centre).all(1)[:, None], centre, inside)  # (a hand-made box with a corner at infinity has no centre to stand on)
    else:
        centre = np.zeros((m, 3))
    parts, codes = [inside, centre], [P_INSIDE, P_CENTRE]
    axes = np.concatenate([np.eye(3), -np.eye(3), [[1, 1, 1], [-1, 1, 0]]])
    for code, sc in ((P_1E4, 1e4), (P_1E19, 1e19), (P_1E20, 1e20), (P_1E30, 1e30)):
        d = np.concatenate([axes, unit(rng, max(m // 4, 8) - len(axes))]) if m // 4 > len(axes) else axes
        parts.append(d * np.float32(sc)), codes.append(code)
    inf = np.inf
    at_inf = np.array([[inf, 0, 0], [-inf, 1, 2], [inf, inf, inf], [inf, -inf, 0], [0, inf, 0], [1, 2, -inf], [-inf, -inf, -inf], [0, 0, inf]])
    parts.append(np.tile(at_inf, (max(m // 32, 1), 1))), codes.append(P_INF)
    nan = inside[:max(m // 8, 8)].copy()
    nan[np.arange(len(nan)), rng.integers(0, 3, len(nan))] = np.nan
    parts.append(nan), codes.append(P_NAN)
    with np.errstate(all="ignore"):
        return np.concatenate(parts).astype(np.float32), np.concatenate([np.full(len(p), c) for p, c in zip(parts, codes)])


def picker_cases():
    """The sections pick, step and near -> (pools, {section: cases}, meta).  meta: `sets` (LightSets.info), per case of each section the stratum of its uniform
    (`pick_u`, `step_u`, `near_u`) and of its point (`step_p`, `near_p`), `step_set` / `step_node` (where a step case's node comes from)."""
    rng = np.random.default_rng(41)
    S = picker_sets()
    info = S.info
    by_name = {d["name"]: k for k, d in enumerate(info)}

    def keys(n):
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32), rng.integers(0, 64, n).astype(U32)

    # ---- pick: lightPickAt on the table and by scan (adjacent cases), lightPick keyed both ways, lightWeight of every light
    pick, pick_u = [], []
    for k, d in enumerate(info):
        n, cdf = d["n"], d["cdf"]
        many = d["name"] == "subnormal total"
        n_rand, n_steer = (64, 64) if n > 1000 else (3000 if many else 200, 100)
        us, codes = [np.array([u for _, u in U_EDGES], np.float32)], [np.array([c for c, _ in U_EDGES])]
        us.append((rng.integers(0, 1 << 24, n_rand) * 2.0 ** -24).astype(np.float32)), codes.append(np.full(n_rand, U_SUBNORMAL if many else U_RANDOM))
        if n >= 2:
            ls = np.arange(n) if n <= n_steer else np.sort(rng.choice(n, n_steer, replace=False))
            st = steer(cdf[ls], np.full(len(ls), cdf[-1], np.float32))
            for row, code in zip(st, (U_AT, U_BELOW, U_ABOVE)):
                us.append(row[~np.isnan(row)]), codes.append(np.full(int((~np.isnan(row)).sum()), code))
        u, code = np.concatenate(us), np.concatenate(codes)
        if n >= 2:
            r = np.zeros(2 * len(u), PICK_DT)
            r["op"], r["set"], r["u"] = np.tile([PICK_AT_TABLE, PICK_AT_SCAN], len(u)), k, np.repeat(u, 2)
            pick.append(r), pick_u.append(np.repeat(code, 2))
        keep = np.concatenate([np.arange(3), 3 + rng.choice(len(u) - 3, min(96, len(u) - 3), replace=False)])  # through the stream: the edges and a sample of the rest
        u, code = u[keep], code[keep]
        r = np.zeros(2 * len(u), PICK_DT)
        k1, ctr = keys(len(u))
        r["op"], r["set"] = np.tile([PICK_TABLE, PICK_SCAN], len(u)), k
        r["k1"], r["ctr"], r["k0"] = np.repeat(k1, 2), np.repeat(ctr, 2), np.repeat(key_for(k1, ctr, u), 2)
        pick.append(r), pick_u.append(np.repeat(code, 2))
        r = np.zeros(n, PICK_DT)
        r["op"], r["set"], r["li"] = PICK_WEIGHT, k, np.arange(n)
        pick.append(r), pick_u.append(np.full(n, U_RANDOM))

    # ---- step: lightNodeStep on nodes of every set x the strata of P x the strata of u
    step, step_u, step_p, step_set, step_node = [], [], [], [], []
    for k, d in enumerate(info):
        nd = d["nodes"]
        if not len(nd):
            continue
        P, pcode = set_points(d, rng, 160 if d["built"] else 480)
        node = rng.integers(0, len(nd), len(P))
        parts = step_parts(nd[node], P)
        st = steer(parts["imp0"], parts["s"])
        for code, u in list(U_EDGES) + [(U_RANDOM, None), (U_RANDOM, None), (U_AT, st[0]), (U_BELOW, st[1]), (U_ABOVE, st[2])]:
            if u is None:
                u = (rng.integers(0, 1 << 24, len(P)) * 2.0 ** -24).astype(np.float32)
            u = np.broadcast_to(np.asarray(u, np.float32), (len(P),))
            have = ~np.isnan(u)
            r = np.zeros(int(have.sum()), STEP_DT)
            r["node"], r["P"], r["u"] = nd[node[have]], P[have], u[have]
            r["inv_p"] = np.where(rng.random(len(r)) < 0.75, 1.0, rng.uniform(0.5, 1000.0, len(r)))
            step.append(r), step_u.append(np.full(len(r), code)), step_p.append(pcode[have]), step_set.append(np.full(len(r), k)), step_node.append(node[have])
    # subnormal importances: built nodes seen from about 1e19 (d2 about 1e38), the uniform random and at the top, where u * s rounds to s
    for name in ("weights from subnormal to 1e30", "random 0, L=300", "lamps n=64", "corridor(16)", "pair"):
        k = by_name[name]
        nd = info[k]["nodes"]
        m = 1500
        node = rng.integers(0, len(nd), m)
        P = (unit(rng, m) * rng.choice(np.array([3e18, 1e19, 1.7e19], np.float32), (m, 1))).astype(np.float32)
        for code, u in ((U_RANDOM, (rng.integers(0, 1 << 24, m) * 2.0 ** -24).astype(np.float32)), (U_LAST, np.full(m, ONE_M)), (U_RANDOM, (1.0 - rng.integers(1, 64, m) * 2.0 ** -24).astype(np.float32))):
            r = np.zeros(m, STEP_DT)
            r["node"], r["P"], r["u"], r["inv_p"] = nd[node], P, u, 1.0
            step.append(r), step_u.append(np.full(m, code)), step_p.append(np.full(m, P_1E19)), step_set.append(np.full(m, k)), step_node.append(node)

    # ---- near: lightPickNear on every set x the strata of P x streams: random, and keyed so that the first level's uniform is an edge or steered onto imp0
    near, near_u, near_p = [], [], []
    shallow = [k for k, d in enumerate(info) if len(d["nodes"]) == 1 and d["built"]]
    for k, d in enumerate(info):
        nd = d["nodes"]
        m = 1600 if d["name"] == "deep" else 560 if k in shallow else 64
        P, pcode = set_points(d, rng, m)
        st = np.full((3, len(P)), np.nan, np.float32)
        if len(nd) and not (d["root"] & LEAF):
            parts = step_parts(np.repeat(nd[d["root"]:d["root"] + 1], len(P)), P)
            st = steer(parts["imp0"], parts["s"])
        for code, u in [(U_RANDOM, None), (U_RANDOM, None)] + list(U_EDGES) + [(U_AT, st[0]), (U_BELOW, st[1]), (U_ABOVE, st[2])]:
            have = np.ones(len(P), bool) if u is None else ~np.isnan(np.broadcast_to(np.asarray(u, np.float32), (len(P),)))
            r = np.zeros(int(have.sum()), NEAR_DT)
            r["set"], r["P"] = k, P[have]
            r["k1"], r["ctr"] = keys(len(r))
            r["k0"] = keys(len(r))[0] if u is None else key_for(r["k1"], r["ctr"], np.broadcast_to(np.asarray(u, np.float32), (len(P),))[have])
            near.append(r), near_u.append(np.full(len(r), code)), near_p.append(pcode[have])
    near, near_u, near_p = cat(near, NEAR_DT), np.concatenate(near_u), np.concatenate(near_p)
    # every wave of 64 consecutive cases, the last and partial one too, holds descents of depth 16 (the deep set) and of depth 1 (sets of two tree lights): each
    # of the three kinds — deep, depth 1, neither — is spread evenly over the whole sequence (case i of n of a kind at (i + 1/2) / n, merged in that order)
    kinds = (np.flatnonzero(near["set"] == by_name["deep"]), np.flatnonzero(np.isin(near["set"], shallow)),
             np.flatnonzero((near["set"] != by_name["deep"]) & ~np.isin(near["set"], shallow)))
    kinds = [rng.permutation(k) for k in kinds]
    at = np.concatenate([(np.arange(len(k)) + 0.5) / len(k) for k in kinds])
    order = np.concatenate(kinds)[np.argsort(at, kind="stable")]
    meta = dict(sets=info, by_name=by_name, pick_u=np.concatenate(pick_u), step_u=np.concatenate(step_u), step_p=np.concatenate(step_p), step_set=np.concatenate(step_set),
                step_node=np.concatenate(step_node), near_u=near_u[order], near_p=near_p[order], shallow=shallow)
    return S.pools(), dict(pick=cat(pick, PICK_DT), step=cat(step, STEP_DT), near=near[order]), meta


def corpus(make_material_dev):
    """-> (tables, {section: cases})."""
    tb = tables(make_material_dev)
    cases = dict(prim=prim_cases(), cam=cam_cases(), vert=vert_cases(tb), light=light_cases(tb), next=next_cases(tb), dir=dir_cases(), bounce=bounce_cases(tb))
    pools, picker, meta = picker_cases()
    tb.update(pools)
    tb["meta"] = meta
    cases.update(picker)
    return tb, cases


# ---- the files -------------------------------------------------------------------------------------------------------------------------------------------------
def _bounce_records(b):
    out = np.zeros((len(b), 20), U32)
    f = out.view(np.float32)
    f[:, 0:3], f[:, 3], f[:, 4:6] = b["o"], b["d"][:, 0], b["d"][:, 1:3]
    out[:, 6], out[:, 7] = b["pid"], b["meta"]
    f[:, 8:11], f[:, 11] = b["beta"], b["bt_w"]
    f[:, 12], f[:, 14], f[:, 15] = b["t"], b["u"], b["v"]
    out[:, 13] = b["tri"].view(U32)
    out[:, 16], out[:, 17], out[:, 18], out[:, 19] = b["flags"], b["max_depth"].view(U32), b["seed"], b["s0"]
    return out


def case_bytes(tb, cases):
    """The case file (tools/shade_cases.h) as bytes -> (bytes, {section: count})."""
    n = {s: len(cases.get(s, ())) for s in SECTIONS}
    pools = dict(no_pools(), **{k: tb[k] for k in ("plights", "psel", "pnodes", "sets") if k in tb})
    assert len(pools["psel"]) % 4 == 0
    head = np.array([MAGIC] + [n[s] for s in SECTIONS[:7]] + [len(tb["mat"]), len(tb["tex"]), len(tb["texbytes"]), len(tb["light"]), len(tb["ltri"]), len(tb["tshade"]), 0, 0] +
                    [n[s] for s in SECTIONS[7:]] + [len(pools["plights"]), len(pools["psel"]), len(pools["pnodes"]), len(pools["sets"]), 0], "<u4")
    assert len(tb["tshade"]) == len(tb["tisect"]) and len(tb["texbytes"]) % 16 == 0
    parts = [head, tb["mat"], tb["tex"], tb["light"], tb["ltri"], tb["tshade"], tb["tisect"]]
    for s in SECTIONS:
        if s == "pick":
            parts += [pools["plights"], pools["psel"], pools["pnodes"], pools["sets"]]
        c = cases.get(s)
        if c is not None and len(c):
            parts.append(_bounce_records(c) if s == "bounce" else c)
    parts.append(tb["texbytes"])
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts), n


def split_words(words, n):
    """The result file's words -> {section: [count, words per case]}."""
    out, at = {}, 0
    assert len(words) == sum(n[s] * WORDS[s] for s in SECTIONS), (len(words), n)
    for s in SECTIONS:
        out[s] = words[at:at + n[s] * WORDS[s]].reshape(n[s], WORDS[s])
        at += n[s] * WORDS[s]
    return out


def digest_of(words, index):
    """The digest the tool forms of a chunk's output words: the wrapping 64-bit sum of mix32(word + index)."""
    return int(mix32(np.asarray(words, np.uint64) + np.asarray(index, np.uint64)).astype(np.uint64).sum(dtype=np.uint64))


def no_pools():
    return dict(plights=np.zeros(0, LIGHT_DT), psel=np.zeros(0, np.float32), pnodes=np.zeros(0, NODE_DT), sets=np.zeros(0, SET_DT))


def no_tables():
    """The tables of a file that holds primitive cases only."""
    return dict(mat=np.zeros(0, MAT_DT), tex=np.zeros(0, TEX_DT), texbytes=np.zeros(0, np.uint8), light=np.zeros(0, LIGHT_DT), ltri=np.zeros(0, LTRI_DT),
                tshade=np.zeros(0, TSHADE_DT), tisect=np.zeros(0, TISECT_DT))


def digest_sets():
    """The tables and nodes of the pickers' digest streams (tools/shade_cases.h digestPoolsFill) -> (LightSets of the four tables, the four nodes, their points)."""
    S = LightSets()
    for k, n in enumerate((2, 7, 64, 256)):
        l = np.arange(n)
        m = mix32(0x5E700000 + 256 * k + l).astype(np.int64)
        e = np.full(n, -20) if k < 2 else (m & 31) - 28
        area = np.ldexp(((m >> 9) + 1).astype(np.float64), e).astype(np.float32)  # exact
        area[np.isin(l, [2, 3, 6]) if k == 1 else (l % 5 == 0) if k == 3 else np.zeros(n, bool)] = 0
        S.add(f"digest table {k}", area, np.tile(np.array([0.5, 2.0, 1.0], np.float32), (n, 1)))
    nodes = np.zeros(4, NODE_DT)
    nodes[:] = (BOX_A[0], BOX_A[1], BOX_B[0], BOX_B[1], 3.0, 1.5, LEAF | 0, LEAF | 1)
    P = np.tile(np.array([0.25, 0.0, 0.125], np.float32), (4, 1))
    nodes["w0"][1], nodes["w1"][1], P[1, 0] = 4.0, 0.25, 1e19
    P[2, 0] = 1e20
    nodes["lo1"][3], nodes["hi1"][3], nodes["w1"][3] = nodes["lo0"][3], nodes["hi0"][3], 3.0
    return S, nodes, P


def digest_chunk_cases(stream, chunk):
    """The inputs of one digest chunk as explicit cases -> (tables, section, cases); digest_chunk_want turns their words into the digest."""
    first = DIGEST_STREAMS[stream][1]
    m = first + chunk * DIGEST_CHUNK + np.arange(DIGEST_CHUNK, dtype=np.uint64)
    u = (m.astype(np.float64) * 2.0 ** -24).astype(np.float32)
    if stream >= DIGEST_OLD_STREAMS:
        S, nodes, P = digest_sets()
        tb = dict(no_tables(), **S.pools())
        if stream >= DIGEST_STEP0:
            c = np.zeros(len(m), STEP_DT)
            c["node"], c["P"], c["u"], c["inv_p"] = nodes[stream - DIGEST_STEP0], P[stream - DIGEST_STEP0], u, 1.0
            return tb, "step", c
        c = np.zeros(len(m), PICK_DT)
        scan = stream >= DIGEST_SCAN0
        c["op"], c["set"], c["u"] = PICK_AT_SCAN if scan else PICK_AT_TABLE, stream - (DIGEST_SCAN0 if scan else DIGEST_PICK0), u
        return tb, "pick", c
    c = np.zeros(len(m), PRIM_DT)
    if stream == 0:
        c["op"], c["a"] = OP_SINCOS, bits(u)
    elif stream in (1, 2):
        c["op"], c["a"] = OP_SQRT, bits(u if stream == 1 else np.float32(1) - u)
    elif stream < 19:
        k = stream - 3
        e = np.float32(1) / (DIGEST_NS[k] + np.float32(1)) if k < 8 else DIGEST_NS[k - 8]
        c["op"], c["a"], c["b"] = OP_POW, bits(u), bits(np.full(len(m), e, np.float32))
    elif stream in (19, 20):
        c["op"], c["a"] = (OP_LOG, OP_EXP)[stream - 19], m
    elif stream in (21, 22):
        c["op"], c["a"] = OP_SQRT, m
    else:
        strat = ((m.astype(np.float64) + 0.5) * 2.0 ** -20).astype(np.float32)
        x = (strat, np.float32(-87.0) * strat, mix32(m).view(np.float32))[stream - 23]
        c["op"], c["a"] = (OP_LOG, OP_EXP, OP_SQRT)[stream - 23], bits(x)
    return no_tables(), "prim", c


def digest_chunk_want(stream, chunk, w):
    """The digest of a chunk from the words [4096, words per case] of its explicit cases."""
    m = DIGEST_STREAMS[stream][1] + chunk * DIGEST_CHUNK + np.arange(DIGEST_CHUNK, dtype=np.uint64)
    if stream >= DIGEST_STEP0:
        return digest_of(w.ravel(), np.stack([2 * m, 2 * m + 1], 1).ravel())
    if stream >= DIGEST_OLD_STREAMS:  # the index with the returned bool in bit 31; the bits of inv_p
        return digest_of(np.stack([w[:, 1] | (w[:, 0] << 31), w[:, 2]], 1).ravel(), np.stack([2 * m, 2 * m + 1], 1).ravel())
    if stream == 0:
        return digest_of(w[:, :2].ravel(), np.stack([2 * m, 2 * m + 1], 1).ravel())
    if stream in (21, 22, 25):
        return digest_of(w[:, :3].ravel(), np.stack([3 * m, 3 * m + 1, 3 * m + 2], 1).ravel())
    return digest_of(w[:, 0], m)
