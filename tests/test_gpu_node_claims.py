"""octVisit, innerStep and the box tests as gfx950 compiles them (tools/node_visit_check, one thread per case) against the CPU build of the same functions
(tests/hostsim): every output word equal — the first check of innerStep's packed two-wide slab arithmetic, which only the device build has, against
boxTest — and the superset property of trt_oct.h's header (1) on the GPU's own words."""
import os
import subprocess

import numpy as np
import pytest

import hostsim_lib as H
import node_cases as NC
import raygen
import refit_ref as RR
import tinyraytracing_amd as T

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
HOSTILE = np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0, -0.0], np.float32)


def _hostile_rays(org, dirs, rng):
    """Every 8th ray gets a zero direction component (every 16th with its origin left where it is: on a plane if the generator put it there), every 64th the
    zero vector in one of its eight sign patterns, every 128th a NaN or an infinity in the direction."""
    org, dirs = org.copy(), dirs.copy()
    k = np.arange(len(org))
    z = k % 8 == 3
    dirs[z, rng.integers(0, 3, z.sum())] = np.where(rng.random(z.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    zv = np.nonzero(k % 64 == 5)[0]
    for a in range(3):
        dirs[zv, a] = np.where((zv // 64 >> a) & 1, np.float32(-0.0), np.float32(0.0))
    h = k % 128 == 9
    dirs[h, rng.integers(0, 3, h.sum())] = HOSTILE[rng.integers(0, 3, h.sum())]
    return org, dirs


def build_cases():
    """(oct nodes, slot boxes, oct cases, reference of the oct cases, 4-wide nodes, innerStep cases, box cases): sizes in the test's docstring."""
    from test_refit_cpu import _oct_case, _wide_case
    rng = np.random.default_rng(41)
    s = T.Scene.named("staircase", 64, 36)
    # (i) synthetic oct nodes x 64 rays, then staircase's oct nodes x 64 rays (48 aimed at a slot's box, 16 of raygen.adversarial_rays)
    blo, bhi, kind = NC.synthetic_nodes(4096)
    syn, ok = H.oct_quantise_nodes(blo, bhi, kind)
    assert ok.all()
    _, _, before, after, real_box, _ = _oct_case(s, s.arrays()["tri_v"])
    assert RR.same_bits(before, after)
    real = before.view(H.OCT_DT)
    onodes = np.concatenate([syn, real])
    slot_box = np.concatenate([np.concatenate([blo, bhi], 2), real_box])
    node = np.concatenate([np.repeat(np.arange(len(syn)), 64), np.repeat(len(syn) + np.arange(len(real)), 64)]).astype(np.uint32)
    used = onodes["meta"][node] != 0
    org, dirs, far = NC.rays_at_boxes(slot_box[node, (rng.random(used.shape) * used).argmax(1)], seed=43)
    adv = np.nonzero((node >= len(syn)) & (np.arange(len(node)) % 4 == 1))[0]
    org[adv], dirs[adv] = raygen.adversarial_rays(s, len(adv))
    far[adv] = False
    passes, entry = H.slot_ref(slot_box, node, org, dirs)
    with np.errstate(divide="ignore"):
        passes[~np.isfinite(np.float32(1) / dirs).all(1)] = False  # traceClosestOct sends no ray of raySpecial() to these nodes: nothing is claimed for them
    idx, cull = NC.culls_for(passes, entry, used, np.full(len(node), INF), rng)
    keep = np.ones(len(idx), bool)
    keep[len(node):2 * len(node)] = False  # culls_for's second group (the bound of a hit) is +inf again here
    idx, cull = idx[keep], cull[keep]
    oct_cases = (node[idx], org[idx], dirs[idx], cull)
    oct_ref = (passes[idx], entry[idx], far[idx])
    # (ii) staircase's 4-wide nodes, and a copy with NaN / +-inf planes, x 64 rays: aimed at a child's box, adversarial, zero vectors, hostile directions
    _, _, wide, _ = _wide_case(s, s.arrays()["tri_v"])
    poisoned = wide.copy()
    hit = rng.random(poisoned["box"].shape) < 0.05
    poisoned["box"][hit] = HOSTILE[rng.integers(0, 3, hit.sum())]
    wnodes = np.concatenate([wide, poisoned])
    wn = np.repeat(np.arange(len(wnodes)), 32 if len(wnodes) > 8192 else 64).astype(np.uint32)
    child = rng.integers(0, 4, len(wn))
    cbox = wnodes["box"][wn, :, child]
    cbox = np.where(np.isfinite(cbox), cbox, np.float32(1.0))
    worg, wdir, _ = NC.rays_at_boxes(cbox, seed=47)
    worg, wdir = _hostile_rays(worg, wdir, rng)
    w_inf = H.inner_step_cases(wnodes, wn, worg, wdir, np.full(len(wn), INF))
    ebits = H.box_cases(cbox, worg, wdir)[:, 1].copy().view(np.float32)
    wcull = np.where(np.arange(len(wn)) % 3 == 0, INF, np.where(np.arange(len(wn)) % 3 == 1, ebits, np.nextafter(ebits, -INF))).astype(np.float32)
    assert (w_inf[:, 2] == 3).sum() > 100 and (w_inf[:, 1] == 0).sum() > 100  # four children passed; none passed
    inner_cases = (wn, worg, wdir, wcull)
    # (iii) 262 144 box cases and two recorded ones: the boxes above and staircase's BVH2 boxes, poisoned ones among them, with the same kinds of rays
    nodes2 = RR.nodes_of(s)
    pool = np.concatenate([slot_box[onodes["meta"] != 0], np.concatenate([nodes2["lo0"], nodes2["hi0"]], 1), np.concatenate([nodes2["lo1"], nodes2["hi1"]], 1)])
    box = pool[rng.integers(0, len(pool), 262144)].copy()
    borg, bdir, _ = NC.rays_at_boxes(box, seed=53)
    borg, bdir = _hostile_rays(borg, bdir, rng)
    bad = rng.random(box.shape) < 0.01
    box[bad] = HOSTILE[rng.integers(0, 3, bad.sum())]
    s.close()
    box, borg, bdir = np.concatenate([box, NC.ZERO_SIGN_BOXES]), np.concatenate([borg, NC.ZERO_SIGN_ORG]), np.concatenate([bdir, NC.ZERO_SIGN_DIR])  # recorded: the last two
    return onodes, slot_box, oct_cases, oct_ref, wnodes, inner_cases, (box, borg, bdir)


def _differences(name, gpu, cpu, cases):
    bad = np.nonzero((gpu != cpu).any(1))[0]
    text = "; ".join(f"case {i}: gpu {[hex(int(x)) for x in gpu[i]]} cpu {[hex(int(x)) for x in cpu[i]]} " + " ".join(repr(c[i]) for c in cases) for i in bad[:6])
    print(f"{name}: {len(gpu)} cases, {len(bad)} differ")
    return len(bad), text


def test_gfx950_makes_the_cpu_builds_decisions_and_visits_a_superset(tmp_path):
    """One run of tools/node_visit_check (1 187 614 octVisit, 433 728 innerStep and 262 146 box cases) over 4 096 synthetic oct nodes and staircase's own, each x 64 rays x the culls +inf / a passing slot's entry / the
    floats either side of it; staircase's 4-wide nodes and a copy with NaN and infinite planes x 64 rays (zero direction components on box planes, the zero
    vector with its +inf entries, NaN and infinite directions); 262 144 box cases of the same kinds.  Every word equals the CPU build's, and the superset
    property (node_cases.superset) holds on the GPU's words of the oct cases.
    The last two box cases are node_cases.ZERO_SIGN_*: zero entries whose sign libm's fminf / fmaxf would get wrong (trt_prims.h, trt_fminf)."""
    exe = os.path.join(T.REPO_ROOT, "tools", "node_visit_check")
    assert os.path.exists(exe), "tools/node_visit_check is not built (make nodecheck)"
    onodes, slot_box, oct_cases, oct_ref, wnodes, inner_cases, box_cases = build_cases()
    case_file, result_file = str(tmp_path / "cases.bin"), str(tmp_path / "result.bin")
    sizes = NC.write_case_file(case_file, onodes, oct_cases, wnodes, inner_cases, *box_cases)
    r = subprocess.run([exe, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    g_oct, g_inner, g_box = NC.read_result_file(result_file, *sizes)
    diffs = [_differences("octVisit", g_oct, H.oct_visit_cases(onodes, *oct_cases), oct_cases),
             _differences("innerStep", g_inner, H.inner_step_cases(wnodes, *inner_cases), inner_cases),
             _differences("boxTest / boxTestGlm", g_box, H.box_cases(*box_cases), box_cases)]
    assert np.array_equal(g_box[-2:], NC.ZERO_SIGN_WORDS), g_box[-2:]
    counts, text = NC.superset(onodes, slot_box, *oct_cases, g_oct, *oct_ref)
    print(counts)
    assert [d[0] for d in diffs] == [0, 0, 0], "\n".join(d[1] for d in diffs)
    assert counts["misses"] == 0, text
    # half of what build_cases yields: 1 436 543 reference passes, 613 763 with a finite cull within one ulp of the entry, 106 883 on flat boxes, 45 276 with an
    # overflowed product, 240 934 from origins 2^20 extents away
    for k, v in dict(passes=718271, near_cull=306881, flat=53441, overflow=22638, far=120467).items():
        assert counts[k] >= v, (k, counts)
