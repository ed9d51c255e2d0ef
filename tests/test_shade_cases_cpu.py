"""The corpus of tests/shade_cases.py proves itself on the CPU build (tests/hostsim), without a GPU: (a) it reaches every branch it is meant to reach, counted on the
CPU build's words; (b) deliberately altered copies of seven functions (tests/hostsim/shade_mutants.cpp) change words of their sections; (c) the words agree with
float64 restatements in numpy of the continuous functions.  tests/test_gpu_shade_cases.py then holds gfx950's words to the same CPU build's."""
import os
import subprocess

import numpy as np
import pytest

import hostsim_lib as H
import nearlights_lib as NL
import onelight_lib as OL
import shade_cases as SC

F32 = np.float32
FLT_MIN = 2.0 ** -126


@pytest.fixture(scope="module")
def run():
    tb, cases = SC.corpus(H.make_material_dev)
    data, n = SC.case_bytes(tb, cases)
    n_words = sum(n[s] * SC.WORDS[s] for s in SC.SECTIONS)
    words = SC.split_words(H.shade_case_words(data, n_words), n)
    for w in words.values():
        w.setflags(write=False)
    return dict(tb=tb, cases=cases, data=data, n=n, n_words=n_words, words=words)


def f32(w):
    return np.ascontiguousarray(w, np.uint32).view(F32)


def _atleast(counts, floor=100):
    print(counts)
    low = {k: v for k, v in counts.items() if v < floor}
    assert not low, f"reached fewer than {floor} times: {low}"


# ---- (a) coverage --------------------------------------------------------------------------------------------------------------------------------------------
def test_next_ray_cases_reach_every_plan_and_both_refraction_outcomes(run):
    c, w = run["cases"]["next"], run["words"]["next"]
    mat = run["tb"]["mat"]
    kind, typ, after = w[:, 0], w[:, 3], w[:, 7]
    counts = {f"kind {k}": int((kind == k).sum()) for k in range(4)}
    counts["TIR -> reflect"] = int(((kind == 1) & (typ == 1)).sum())
    counts["transmission"] = int(((kind == 1) & (typ == 2)).sum())
    counts["sel_kd == 1: the lobe draw counted, not generated"] = int(((c["mat"] == SC.M_DIFFUSE) & (kind == 2) & (after == c["ctr"] + 3)).sum())
    draw = SC.uniform(c["k0"], c["k1"], c["ctr"])
    # Fresnel: the draw on the Schlick term and one ulp either side (pn = e_y: cos_in is I.y exactly)
    glass = np.isin(c["mat"], [SC.M_GLASS, SC.M_DENSE]) & (c["pn"] == (0.0, 1.0, 0.0)).all(1) & (c["I"][:, 2] == 0)
    f = SC.fresnel_of(mat["rf0"][c["mat"]], c["I"][:, 1])
    on, above, below = glass & (draw == f), glass & (draw == f + SC.ULP) & (f >= 0.5), glass & (draw == f - SC.ULP) & (f >= 0.5)
    counts.update({"draw == fresnel": int(on.sum()), "draw == fresnel + ulp": int(above.sum()), "draw == fresnel - ulp": int(below.sum())})
    assert (kind[on] != 1).all() and (kind[below] != 1).all() and (kind[above] == 1).all()  # `fresnel < draw`, strictly
    # the lobe draw on the thresholds 1/2 and 3/4 of the glossy materials
    for m, name, ns_gt_1 in ((SC.M_GLOSSY, "Ns 50", True), (SC.M_NS1, "Ns 1", False)):
        g = c["mat"] == m
        for p, want in ((F32(0.5) - SC.ULP, 2), (F32(0.5), 3 if ns_gt_1 else 0), (F32(0.75) - SC.ULP, 3 if ns_gt_1 else 0), (F32(0.75), 0)):
            sel = g & (draw == p)
            counts[f"{name}: lobe draw {float(p)!r}"] = int(sel.sum())
            assert (kind[sel] == want).all(), (name, p, want, np.unique(kind[sel]))
    _atleast(counts)


def test_camera_cases_take_all_three_branches_on_every_grid(run):
    c, w = run["cases"]["cam"], run["words"]["cam"]
    counts = {f"mode {m}": int((c["mode"] == m).sum()) for m in range(3)}
    corner = ((c["i"] == 0) | (c["i"] == c["H"] - 1)) & ((c["j"] == 0) | (c["j"] == c["W"] - 1))
    for s in SC.CAM_SIZES:
        counts[f"corner pixels of W = {s}"] = int((corner & (c["W"] == s)).sum())
        counts[f"corner pixels of H = {s}"] = int((corner & (c["H"] == s)).sum())
    counts["jitter 0"] = int(((c["u1"] == 0) | (c["u2"] == 0)).sum())
    counts["jitter 1 - 2^-24"] = int(((c["u1"] == SC.ONE_M) | (c["u2"] == SC.ONE_M)).sum())
    _atleast(counts)
    d = f32(w[:, 3:6])
    cancelled = np.isnan(d).all(1) & (c["cam"][:, :3] == c["cam"][:, 3:6]).all(1)
    assert cancelled.sum() >= 36, cancelled.sum()  # the eye on llc, the sample on llc: normalize(0) — once per grid and more


def test_light_cases_reach_both_picks_every_exit_and_the_phong_switch(run):
    c, w = run["cases"]["light"], run["words"]["light"]
    mat, lights = run["tb"]["mat"], run["tb"]["light"]
    emit, after = w[:, 0], w[:, 8]
    picked = after == c["ctr"] + 4
    counts = {"pick by bisection": int((picked & (c["flags"] & 2 != 0)).sum()), "pick by scan": int((picked & (c["flags"] & 2 == 0)).sum()),
              "pick >= tri_count": int(((after == c["ctr"] + 1) & (lights["tri_count"][c["li"]] > 0)).sum()),
              "empty light": int(((after == c["ctr"] + 1) & (lights["tri_count"][c["li"]] == 0)).sum()),
              "cos_s rejected": int((picked & (emit == 0)).sum()),
              "no_spec on": int(((emit == 1) & (mat["no_spec"][c["mat"]] == 1)).sum()), "no_spec off": int(((emit == 1) & (mat["no_spec"][c["mat"]] == 0)).sum()),
              "fixed": int((picked & (c["flags"] & 1 != 0)).sum()), "parity": int((picked & (c["flags"] & 1 == 0)).sum()),
              "t_max capped at TRT_INF": int(((emit == 1) & (f32(w[:, 7]) == F32(114514.0))).sum()),
              "NaN contribution": int(((emit == 1) & np.isnan(f32(w[:, 4:7])).any(1)).sum())}
    for n in (1, 2, 33):
        counts[f"tri_count {n}"] = int((picked & (lights["tri_count"][c["li"]] == n)).sum())
    # the CDF draw ON a cumulative area (rnd = the draw: area 1): the strict `<` picks the NEXT triangle, the float below picks this one
    draw = SC.uniform(c["k0"], c["k1"], c["ctr"])
    unit_area = (c["light0_area"] == 1) & np.isin(c["li"], [SC.L_TWO, SC.L_33])
    den = np.where(c["li"] == SC.L_TWO, 2, 64)
    on = unit_area & (draw * den == np.floor(draw * den)) & (draw > 0)
    counts["rnd on a cumulative area"] = int(on.sum())
    counts["rnd one float below a cumulative area"] = int((unit_area & ((draw + SC.ULP) * den == np.floor((draw + SC.ULP) * den))).sum())
    _atleast(counts)
    q4 = np.zeros(len(c), bool)
    for k0, k1 in SC.Q4_KEYS:
        q4 |= (c["k0"] == k0) & (c["k1"] == k1) & (c["ctr"] == 0)
    assert (SC.uniform(c["k0"][q4], c["k1"][q4], 1) == 0).all() and (SC.uniform(c["k0"][q4], c["k1"][q4], 2) < 2.0 ** -10).all()
    _atleast({"Q4: r1 = 0 and two tiny draws, sampled": int((q4 & picked & (c["flags"] & 1 == 0)).sum())}, 10)


def _texel_raw(coord, size):
    """(int)(fract(coord) * size) before the clamps, in binary64 as makeVertex forms it; NaN where the coordinate is not finite."""
    with np.errstate(invalid="ignore"):
        x = coord.astype(np.float64)
        return (x - np.floor(x)) * size


def test_vertex_cases_reach_the_four_texel_clamps_and_the_wrap(run):
    c = run["cases"]["vert"]
    mat, tex = run["tb"]["mat"], run["tb"]["tex"]
    t = mat["tex"][c["ts"]["mat"]]
    exact = (t >= 0) & (c["u"] == 0) & (c["v"] == 0)  # the coordinate is (vt[0], vt[1]) exactly
    col, row = c["ts"]["vt"][:, 0], c["ts"]["vt"][:, 1]
    rc, rr = _texel_raw(col, tex["width"][t]), _texel_raw(row, tex["height"][t])
    counts = {"column clamped from above": int((exact & (rc >= tex["width"][t])).sum()), "row clamped from above": int((exact & (rr >= tex["height"][t])).sum()),
              "column clamped from below (not finite)": int((exact & np.isnan(rc)).sum()), "row clamped from below (not finite)": int((exact & np.isnan(rr)).sum()),
              "a negative coordinate wrapped": int((exact & (col < 0) & np.isfinite(col) & (rc > 0) & (rc < tex["width"][t])).sum()),
              "a coordinate on a texel boundary": int((exact & (rc == np.floor(rc)) & (rc > 0)).sum()),
              "fract is 0 at 1e7": int((exact & (np.abs(col) == 1e7)).sum()), "untextured": int((t < 0).sum()), "NaN normal": int(np.isnan(f32(run["words"]["vert"][:, 3:6])).any(1).sum())}
    for k, (w, h) in enumerate(SC.TEX_SIZES):
        counts[f"texture {w} x {h}"] = int((t == k).sum())
    _atleast(counts)
    # a coordinate that is not finite gives texel 0 (the clamps: (int) of a NaN is negative on the CPU build, 0 on gfx950)
    bad = exact & ~(np.isfinite(col) & np.isfinite(row))
    kd = f32(run["words"]["vert"][:, 6:9])
    nan_both = exact & ~np.isfinite(col) & ~np.isfinite(row)
    first = run["tb"]["texbytes"][tex["offset"][t[nan_both]].astype(np.int64)[:, None] + np.arange(3)].astype(F32) / F32(255)
    assert bad.sum() >= 100 and np.array_equal(kd[nan_both], first)


def test_bounce_cases_reach_roulette_depth_emission_and_both_offset_sides(run):
    c, w, tb = run["cases"]["bounce"], run["words"]["bounce"], run["tb"]
    emit, flags = w[:, 0], w[:, 13]
    had_hit, shade_ok, add_l = flags & 1 != 0, flags & 2 != 0, flags & 4 != 0
    depth, ctr = c["meta"] >> 20, c["meta"] & 0xFFFF
    last = (c["max_depth"] > 0) & (depth + 1 >= c["max_depth"])
    pl = c["pid"] % 256  # the tile is 64 x 4 with rows 0..3: the pixel index is the path's index in the tile
    k0, k1 = SC.make_key(c["seed"], pl, c["s0"].astype(np.uint64) + c["pid"] // 256)
    rr = SC.uniform(k0, k1, ctr)
    killed = shade_ok & ~last & ~(rr < F32(0.8))
    assert (emit[killed] == 0).all() and (emit[last] == 0).all()
    emissive = had_hit & (tb["tshade"]["mat"][np.maximum(c["tri"], 0)] == SC.M_EMISSIVE)
    counts = {"miss": int((~had_hit).sum()), "RR kill": int(killed.sum()), "RR survived, no lobe": int((shade_ok & ~last & (rr < F32(0.8)) & (emit == 0)).sum()),
              "last depth": int((shade_ok & last).sum()), "emissive hit kept": int((emissive & add_l).sum()), "emissive hit dropped": int((emissive & ~add_l).sum()),
              "extension ray": int((emit == 1).sum()), "specular_ks": int(((emit == 1) & (c["flags"] & 2 != 0)).sum())}
    for t in range(3):
        counts[f"ray type {t}"] = int(((emit == 1) & ((w[:, 8] >> 16) & 3 == t)).sum())
    # which side of the surface the offset origin lies on (TRT_FLAG_RAY_OFFSET): against the geometric normal e1 x e2
    off = (emit == 1) & (c["flags"] & 1 != 0)
    P = c["o"] + c["d"] * c["t"][:, None]  # binary32, a product and a sum per component: makeVertex's P exactly
    ng = np.cross(tb["tisect"]["e1"].astype(np.float64), tb["tisect"]["e2"].astype(np.float64))[np.maximum(c["tri"], 0)]
    side = np.einsum("ij,ij->i", f32(w[:, 1:4]).astype(np.float64) - P.astype(np.float64), ng)
    counts["offset origin on the normal's side"] = int((off & (side > 0)).sum())
    counts["offset origin on the other side"] = int((off & (side < 0)).sum())
    assert np.array_equal(f32(w[:, 1:4])[(emit == 1) & ~off], P[(emit == 1) & ~off])  # Q6: the hit point itself
    _atleast(counts)
    at = np.isin(c["seed"], SC.RR_AT) & (c["s0"] == SC.RR_SAMPLE) & (c["pid"] == 0) & (ctr == SC.RR_CTR)
    below = np.isin(c["seed"], SC.RR_BELOW) & (c["s0"] == SC.RR_SAMPLE) & (c["pid"] == 0) & (ctr == SC.RR_CTR)
    assert (rr[at] == F32(0.8)).all() and (rr[below] == np.nextafter(F32(0.8), F32(0))).all()
    assert (emit[at] == 0).all()  # `draw < 0.8`, strictly
    _atleast({"RR draw on 0.8: killed": int((at & shade_ok).sum()), "RR draw one float below 0.8: an extension ray": int((below & (emit == 1)).sum())}, 10)


def test_direction_cases_put_k_on_both_sides_of_zero(run):
    c, w = run["cases"]["dir"], run["words"]["dir"]
    r = c["op"] == 1
    I, N, eta = c["a"], c["b"], c["x"]
    dn = (N[:, 0] * I[:, 0] + N[:, 1] * I[:, 1]) + N[:, 2] * I[:, 2]  # binary32, glm's order
    k = F32(1) - eta * eta * (F32(1) - dn * dn)
    zero = (w == 0).all(1) | (w == 0x80000000).all(1)
    tiny = r & (np.abs(k) <= F32(64 * 2.0 ** -24))
    counts = {"k a few ulps below 0": int((tiny & (k < 0)).sum()), "k a few ulps above 0": int((tiny & (k > 0)).sum()), "k == 0": int((r & (k == 0)).sum()),
              "total internal reflection": int((r & (k < 0)).sum()), "refracted": int((r & (k > 0)).sum()),
              "sampleDir |a.x| == |a.y|": int(((c["op"] == 0) & (np.abs(c["a"][:, 0]) == np.abs(c["a"][:, 1]))).sum()),
              "sampleDir NaN axis": int(((c["op"] == 0) & np.isnan(c["a"]).any(1)).sum()), "reflect": int((c["op"] == 2).sum())}
    for u in SC.EDGE_U:
        counts[f"sampleDir u_phi = {float(u)!r}"] = int(((c["op"] == 0) & (c["y"] == u)).sum())
        counts[f"sampleDir u_theta = {float(u)!r}"] = int(((c["op"] == 0) & (c["b"][:, 0] == u)).sum())
    assert zero[r & (k < 0)].all() and not zero[r & (k >= 0) & (I != 0).any(1)].any()  # `k < 0`, strictly: k == 0 still refracts
    _atleast(counts, 5)
    _atleast({k_: v for k_, v in counts.items() if k_ != "k == 0"})


# ---- the light pickers: coverage, the words restated in binary32, table against scan, the float64 restatements ---------------------------------------------------
def _same_words(got, want_bits):
    """got words == expected words, any NaN being the one canonical NaN."""
    return got == np.where(np.isnan(f32(want_bits)), np.uint32(0x7FC00000), np.asarray(want_bits, np.uint32))


def _pick_at(d, u):
    """lightPickAt restated in binary32 on the set's table -> (ok, li, inv_p, r, idx: the search's result before the fall-back)."""
    cdf, w, n = d["cdf"], d["w"], d["n"]
    total = cdf[-1]
    u = np.asarray(u, F32)
    if not (total > 0 and total < np.inf):
        z = np.zeros(len(u), np.int64)
        return np.zeros(len(u), bool), z, np.ones(len(u), F32), np.zeros(len(u), F32), z
    with np.errstate(all="ignore"):
        r = (u * total).astype(F32)
        idx = np.searchsorted(cdf, r, side="right")
        li = np.where(idx >= n, np.flatnonzero(w > 0)[-1], idx)
        return np.ones(len(u), bool), li, (total / w[li]).astype(F32), r, idx


def test_pick_cases_reach_every_exit_of_lightPickAt_and_match_its_restatement(run):
    """Every pick case's words are those of lightPickAt / lightPick / lightWeight restated in binary32 on the CPU build's own table (the steered strata among them: r on a
    table entry picks the next light of positive weight, one float below it the entry's own); the table form and the scan form give identical words; each exit is taken."""
    c, w, meta = run["cases"]["pick"], run["words"]["pick"], run["tb"]["meta"]
    at, stream, weight = c["op"] < 2, (c["op"] == SC.PICK_TABLE) | (c["op"] == SC.PICK_SCAN), c["op"] == SC.PICK_WEIGHT
    counts = {k: 0 for k in ("total not positive", "total not finite", "pick by bisection", "pick by scan", "the pick >= n fall-back", "a pick behind a zero-weight plateau",
                             "r on the value of a plateau", "r on a table entry", "r one float below a table entry", "r one float above a table entry",
                             "lightPick, fewer than two lights", "lightPick, one draw", "weight zero", "weight positive", "weight subnormal")}
    for k, d in enumerate(meta["sets"]):
        n, cdf, wt = d["n"], d["cdf"], d["w"]
        for kind, sel in (("at", at & (c["set"] == k)), ("stream", stream & (c["set"] == k))):
            if not sel.any():
                continue
            u = c["u"][sel] if kind == "at" else SC.uniform(c["k0"][sel], c["k1"][sel], c["ctr"][sel])
            got = w[sel]
            if n < 2:
                assert (got[:, 0] == (n == 1)).all() and (got[:, 1] == 0).all() and (f32(got[:, 2]) == 1).all() and (got[:, 3] == c["ctr"][sel]).all(), d["name"]
                counts["lightPick, fewer than two lights"] += int(sel.sum())
                continue
            ok, li, ip, r, idx = _pick_at(d, u)
            assert (got[:, 0] == ok).all() and (got[:, 1] == np.where(ok, li, 0)).all() and _same_words(got[:, 2], SC.bits(np.where(ok, ip, 1))).all(), d["name"]
            if kind == "stream":
                assert (got[:, 3] == c["ctr"][sel] + 1).all()
                counts["lightPick, one draw"] += int(sel.sum())
                continue
            assert (got[:, 3] == c["ctr"][sel]).all()
            if not ok.any():
                counts["total not positive" if not cdf[-1] > 0 else "total not finite"] += int(sel.sum())
                continue
            assert (wt[li] > 0).all(), f"{d['name']}: a light of weight zero was picked"
            counts["pick by bisection"] += int((c["op"][sel] == SC.PICK_AT_TABLE).sum())
            counts["pick by scan"] += int((c["op"][sel] == SC.PICK_AT_SCAN).sum())
            counts["the pick >= n fall-back"] += int((idx >= n).sum())
            behind = (li >= 1) & (wt[np.maximum(li, 1) - 1] == 0) & (idx < n)
            counts["a pick behind a zero-weight plateau"] += int(behind.sum())
            counts["r on the value of a plateau"] += int((behind & (r == cdf[np.maximum(li, 1) - 1])).sum())
            code = meta["pick_u"][sel]
            on = np.isin(r, cdf)
            counts["r on a table entry"] += int((on & (code == SC.U_AT)).sum())
            counts["r one float below a table entry"] += int((np.isin(np.nextafter(r, F32(np.inf)), cdf) & (code == SC.U_BELOW)).sum())
            counts["r one float above a table entry"] += int((np.isin(np.nextafter(r, F32(-np.inf)), cdf) & (code == SC.U_ABOVE)).sum())
            assert (on == (code == SC.U_AT))[np.isin(code, [SC.U_AT])].all()
            assert (cdf[np.minimum(li, n - 1)][on & (idx < n)] > r[on & (idx < n)]).all()  # the strict `<`: r on cdf_l never picks l
        sel = weight & (c["set"] == k)
        assert np.array_equal(w[sel][:, 2], SC.bits(wt)) and np.array_equal(w[sel][:, 1], np.arange(n)), d["name"]
        counts["weight zero"] += int((wt == 0).sum())
        counts["weight positive"] += int((wt > 0).sum())
        counts["weight subnormal"] += int(((wt > 0) & (wt < FLT_MIN)).sum())
    _atleast({k_: v for k_, v in counts.items() if k_ != "weight subnormal"})
    _atleast({"weight subnormal": counts["weight subnormal"]}, 5)
    # table against scan: adjacent cases, the same set and uniform (or stream)
    for a, b in ((SC.PICK_AT_TABLE, SC.PICK_AT_SCAN), (SC.PICK_TABLE, SC.PICK_SCAN)):
        i = np.flatnonzero(c["op"] == a)
        assert (c["op"][i + 1] == b).all() and all(np.array_equal(c[f][i], c[f][i + 1]) for f in ("set", "u", "k0", "k1", "ctr"))
        assert np.array_equal(w[i], w[i + 1]), f"{int((w[i] != w[i + 1]).any(1).sum())} cases differ between the table and the scan"


def test_pick_cases_agree_with_the_float64_search(run):
    """OL.pick_f64 (r = u cdf_{L-1} exact) on the strata that are not steered onto a table entry: a pick may differ only within 4 ulp of an entry, in at most 1 % of a
    stratum's cases, and inv_p is the one binary32 division cdf_{L-1} / w where it agrees (tests/test_one_light_cpu.py's rule).  The steered strata sit on a decision
    by construction and are held to their expected words by the test above."""
    c, w, meta = run["cases"]["pick"], run["words"]["pick"], run["tb"]["meta"]
    tally = {code: [0, 0, 0] for code in (SC.U_RANDOM, SC.U_ZERO, SC.U_ULP, SC.U_LAST)}
    for k, d in enumerate(meta["sets"]):
        cdf = d["cdf"]
        if d["n"] < 2 or not (cdf[-1] > 0 and cdf[-1] < np.inf):
            continue
        for code in tally:
            sel = (c["op"] < 2) & (c["set"] == k) & (meta["pick_u"] == code)
            if not sel.any():
                continue
            want, margin = OL.pick_f64(d["w"], cdf, c["u"][sel])
            differ = w[sel][:, 1] != want
            assert not (differ & (margin > 4.0)).any(), d["name"]
            same = ~differ
            with np.errstate(over="ignore"):  # (a subnormal weight under a large total: inv_p is +inf on either side)
                assert np.array_equal(w[sel][same, 2], SC.bits((cdf[-1] / d["w"][want[same]]).astype(F32))), d["name"]
            tally[code][0] += int(sel.sum()); tally[code][1] += int((margin <= 4.0).sum()); tally[code][2] += int(differ.sum())
    print({code: t for code, t in tally.items()})
    for code, (cases, near, wrong) in tally.items():  # (an edge uniform is one case per set and form)
        assert cases >= (100 if code == SC.U_RANDOM else 50) and wrong <= 0.01 * cases, (code, cases, near, wrong)


def _step_f64(nd, P, u):
    """One level of NL.descend: r = u s in float64 against the binary32 importances -> (takes child 0, the binary32 factor s / imp, |r - imp0| in ulps of r)."""
    imp0, imp1, s = NL.importances(nd, P)
    with np.errstate(all="ignore"):
        r = u.astype(np.float64) * s.astype(np.float64)
        first = r < imp0
        first = np.where(np.where(first, imp0, imp1) > 0, first, ~first)
        ulp = np.spacing(np.maximum(r, 1e-38).astype(F32)).astype(np.float64)
        return first, (s / np.where(first, imp0, imp1).astype(F32)).astype(F32), np.abs(r - imp0) / ulp


def test_step_cases_reach_every_branch_of_lightNodeStep_and_match_its_restatements(run):
    """Every step case's words are lightNodeStep restated in binary32 (SC.step_f32: the hand-made nodes, the points at infinity and with a NaN among them); each branch is
    taken, counted on that restatement, which the words confirm; on nodes buildLightTree made and finite points the float64 decision of NL.descend agrees but within 4 ulp
    of imp0, in at most 1 % of the cases of each stratum that is not steered onto imp0, with inv_p bit for bit where it agrees."""
    c, w, meta = run["cases"]["step"], run["words"]["step"], run["tb"]["meta"]
    S = SC.step_f32(c["node"], c["P"], c["u"], c["inv_p"])
    assert np.array_equal(w[:, 0], S["child"]), int((w[:, 0] != S["child"]).sum())
    assert _same_words(w[:, 1], SC.bits(S["inv_p"])).all()
    built = np.array([d["built"] for d in meta["sets"]])[meta["step_set"]]

    def subnormal(x):
        with np.errstate(invalid="ignore"):
            return (np.abs(x) > 0) & (np.abs(x) < FLT_MIN)
    fb = S["fallback"]
    counts = {"importance as computed": int((fb == 0).sum()), "by power: a NaN importance": int((fb == 1).sum()), "by power: s == 0": int((fb == 2).sum()),
              "by power: s == inf": int((fb == 3).sum()), "by power: a negative importance": int((fb == 4).sum()), "the flip": int(S["flipped"].sum()),
              "the flip on a built node": int((S["flipped"] & built).sum()), "r == imp0": int((S["r"] == S["imp0"]).sum()),
              "r one float below imp0": int((np.nextafter(S["r"], F32(np.inf)) == S["imp0"]).sum()), "r one float above imp0": int((np.nextafter(S["r"], F32(-np.inf)) == S["imp0"]).sum()),
              "a subnormal importance": int(((fb == 0) & (subnormal(S["imp0"]) | subnormal(S["imp1"]))).sum()), "a subnormal s": int(((fb == 0) & subnormal(S["s"])).sum()),
              "a subnormal r": int(((fb == 0) & subnormal(S["r"])).sum()), "a hand-made node": int((~built).sum()), "child 0": int((w[:, 0] == c["node"]["child0"]).sum()),
              "child 1": int((w[:, 0] == c["node"]["child1"]).sum()), "inv_p not finite": int((~np.isfinite(f32(w[:, 1]))).sum())}
    for p in range(8):
        counts[f"P stratum {p}"] = int((meta["step_p"] == p).sum())
    assert (fb != 5).all()  # every fall-back has one of the four causes
    # a NaN importance without a NaN in the inputs: on the hand-made nodes whose box corners are infinite the centre is infinite (or -inf + inf), so that hi - centre, and
    # with P at the same infinity P - centre, is inf - inf
    corners = meta["step_set"] == meta["by_name"]["hand: infinite box corners"]
    with np.errstate(invalid="ignore"):
        clean = ~np.isnan(c["P"]).any(1)
        counts["a NaN importance by inf - inf"] = int((corners & clean & (np.isnan(S["raw0"]) | np.isnan(S["raw1"]))).sum())
        counts["an infinite centre beside a finite point"] = int((corners & np.isfinite(c["P"]).all(1)).sum())
    steered = {SC.U_AT: S["r"] == S["imp0"], SC.U_BELOW: np.nextafter(S["r"], F32(np.inf)) == S["imp0"], SC.U_ABOVE: np.nextafter(S["r"], F32(-np.inf)) == S["imp0"]}
    for code, hit in steered.items():
        assert hit[meta["step_u"] == code].all()
    at = (meta["step_u"] == SC.U_AT) & ~S["flipped"]
    assert (w[at, 0] == c["node"]["child1"][at]).all()  # `r < imp0`, strictly
    _atleast(counts)
    tally = {}
    for code in (SC.U_RANDOM, SC.U_ZERO, SC.U_ULP, SC.U_LAST):
        sel = built & np.isin(meta["step_p"], SC.P_FINITE) & (meta["step_u"] == code)
        first, factor, margin = _step_f64(c["node"][sel], c["P"][sel], c["u"][sel])
        differ = (w[sel, 0] == c["node"]["child0"][sel]) != first
        same_child = c["node"]["child0"][sel] == c["node"]["child1"][sel]
        differ &= ~same_child
        assert not (differ & (margin > 4.0)).any(), code
        with np.errstate(all="ignore"):
            want = (c["inv_p"][sel] * factor).astype(F32)
        assert _same_words(w[sel, 1][~differ], SC.bits(want[~differ])).all(), code
        tally[code] = (int(sel.sum()), int((margin <= 4.0).sum()), int(differ.sum()))
        assert sel.sum() >= 100 and differ.sum() <= 0.01 * sel.sum(), tally
    print(tally)


def _descend_f32(d, P, k0, k1, ctr):
    """lightPickNear restated in binary32 over SC.step_f32 -> (ok, li, inv_p, draws)."""
    m = len(P)
    if d["n"] < 2:
        return np.full(m, d["n"] == 1), np.zeros(m, np.uint32), np.ones(m, F32), np.zeros(m, np.uint32)
    if d["root"] == SC.NONE:
        return np.zeros(m, bool), np.zeros(m, np.uint32), np.ones(m, F32), np.zeros(m, np.uint32)
    ref, ip, draws = np.full(m, d["root"], np.uint32), np.ones(m, F32), np.zeros(m, np.uint32)
    while True:
        act = np.flatnonzero((ref & SC.LEAF) == 0)
        if not len(act):
            break
        S = SC.step_f32(d["nodes"][ref[act]], P[act], SC.uniform(k0[act], k1[act], ctr[act] + draws[act]), ip[act])
        ref[act], ip[act] = S["child"], S["inv_p"]
        draws[act] += 1
    ok = np.isfinite(ip)
    return ok, ref & ~np.uint32(SC.LEAF), np.where(ok, ip, F32(1)), draws


def test_near_cases_reach_every_exit_of_lightPickNear_and_match_its_restatements(run):
    """Every near case's words are lightPickNear restated in binary32 (hand-made nodes, infinite and NaN points among them); each exit is taken; every wave of 64 consecutive
    cases, the last one too, mixes descents of depth 1 and of depth 16; on built trees and finite points NL.descend agrees by tests/test_near_lights_cpu.py's rule.
    The exit for an inv_p that is not finite is reached on built trees: in the set `absorbed` (weights 1e-44 and 1e30 under one node) the first child is taken with
    s / imp0 = +inf whenever the keyed uniform 0 makes r = 0 < imp0, and in the set `total +inf` the weights of a node sum to +inf, so that s / imp is inf / inf."""
    c, w, meta = run["cases"]["near"], run["words"]["near"], run["tb"]["meta"]
    draws = w[:, 3] - c["ctr"]
    counts = {k: 0 for k in ("fewer than two lights", "TRT_LIGHT_NONE", "a leaf root", "a full-depth descent", "inv_p not finite", "inv_p not finite on a built tree",
                             "hand-made nodes", "a descent of depth 1")}
    for p in range(8):
        counts[f"P stratum {p}"] = int((meta["near_p"] == p).sum())
    for u in range(7):
        counts[f"stream stratum {u}"] = int((meta["near_u"] == u).sum())
    tally = {code: [0, 0, 0] for code in (SC.U_RANDOM, SC.U_ZERO, SC.U_ULP, SC.U_LAST)}
    for k, d in enumerate(meta["sets"]):
        sel = c["set"] == k
        ok, li, ip, n_draws = _descend_f32(d, c["P"][sel], c["k0"][sel], c["k1"][sel], c["ctr"][sel])
        got = w[sel]
        assert (got[:, 0] == ok).all() and (got[:, 1] == li).all() and _same_words(got[:, 2], SC.bits(ip)).all() and (draws[sel] == n_draws).all(), d["name"]
        assert (li < max(d["n"], 1)).all()
        inner = d["n"] >= 2 and d["root"] != SC.NONE and not d["root"] & SC.LEAF
        counts["fewer than two lights"] += int(sel.sum()) if d["n"] < 2 else 0
        counts["TRT_LIGHT_NONE"] += int(sel.sum()) if d["n"] >= 2 and d["root"] == SC.NONE else 0
        counts["a leaf root"] += int(sel.sum()) if d["n"] >= 2 and d["root"] != SC.NONE and d["root"] & SC.LEAF else 0
        counts["a full-depth descent"] += int((n_draws == 16).sum())
        counts["a descent of depth 1"] += int((n_draws == 1).sum())
        counts["inv_p not finite"] += int((~ok).sum()) if inner else 0
        counts["inv_p not finite on a built tree"] += int((~ok).sum()) if inner and d["built"] else 0
        counts["hand-made nodes"] += 0 if d["built"] else int(sel.sum())
        if not (inner and d["built"]):
            continue
        # the float64 descent
        U = np.stack([SC.uniform(c["k0"][sel], c["k1"][sel], c["ctr"][sel] + j) for j in range(NL.MAX_DEPTH)], 1)
        finite = np.isin(meta["near_p"][sel], SC.P_FINITE)
        want = NL.descend(d["nodes"].view(NL.NODE), d["root"], c["P"][sel][finite], U[finite])
        g_li, g_ip, g_ok = got[finite, 1], got[finite, 2], got[finite, 0] == 1
        differ = g_li != want["index"]
        assert not (differ & (want["margin"] > 4.0)).any(), d["name"]
        same = ~differ
        assert (g_ok[same] == np.isfinite(want["inv_p32"][same])).all(), d["name"]
        assert _same_words(g_ip[same & g_ok], SC.bits(want["inv_p32"][same & g_ok])).all(), d["name"]
        for code in tally:
            t = meta["near_u"][sel][finite] == code
            tally[code][0] += int(t.sum()); tally[code][1] += int((want["margin"][t] <= 4.0).sum()); tally[code][2] += int(differ[t].sum())
    _atleast(counts)
    print(tally)
    for code, (cases, near, wrong) in tally.items():
        assert cases >= 100 and wrong <= 0.01 * cases, (code, cases, near, wrong)
    waves = [draws[i:i + 64] for i in range(0, len(c), 64)]  # every wave, the last and partial one too
    assert min((wv == 16).sum() for wv in waves) >= 4 and min((wv == 1).sum() for wv in waves) >= 4, "a wave without descents of depth 1 and of depth 16"


# ---- (b) sensitivity ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant,section,what", [(1, "light", "`rnd <= cum` in the CDF pick"), (2, "dir", "`k <= 0` in refract"), (3, "vert", "the texel column taken in fp32"),
                                                 (4, "pick", "`r <= light_sel[mid]` in lightPickAt's bisection"), (5, "step", "`r <= imp0` in lightNodeStep"),
                                                 (6, "step", "lightNodeStep without the flip"), (7, "step", "lightChildImportance with d2 alone")])
def test_an_altered_function_changes_words_of_its_section(run, mutant, section, what):
    control = SC.split_words(H.shade_case_words(run["data"], run["n_words"], mutant=0), run["n"])
    for s in SC.SECTIONS:
        assert np.array_equal(control[s], run["words"][s]), s  # the mutants' library runs the headers' own functions to the same words
    words = SC.split_words(H.shade_case_words(run["data"], run["n_words"], mutant=mutant), run["n"])
    changed = {s: int((words[s] != run["words"][s]).any(1).sum()) for s in SC.SECTIONS}
    print(what, changed)
    assert changed[section] > 0, what
    assert all(v == 0 for s, v in changed.items() if s != section), changed


def _tool_refuses(tmp_path, data, why):
    """tools/shade_case_check itself on the file: exit code 2 with the rule's message and no result file — parse runs before the device is touched, so this needs no GPU."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "shade_case_check")
    assert os.path.exists(exe), "tools/shade_case_check is not built (make shadecheck)"
    case_file, result_file = str(tmp_path / "bad.bin"), str(tmp_path / "bad.out")
    with open(case_file, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, case_file, result_file], capture_output=True, text=True, timeout=60)
    return r.returncode == 2 and why in r.stderr and not os.path.exists(result_file)


def test_a_file_with_an_index_out_of_range_is_refused(run, tmp_path):
    tb = run["tb"]
    small = {s: run["cases"][s][:8].copy() for s in SC.SECTIONS}

    def refused(tb2=tb, **changed):
        data, n = SC.case_bytes(tb2, dict(small, **changed))
        return H.shade_case_words(data, sum(n[s] * SC.WORDS[s] for s in SC.SECTIONS)) is None
    assert not refused()

    def edit(section, field, value, sub=None):
        c = small[section].copy()
        (c[sub] if sub else c)[field][3] = value
        return {section: c}
    assert refused(**edit("light", "mat", len(tb["mat"])))
    assert refused(**edit("light", "li", len(tb["light"])))
    assert refused(**edit("next", "mat", len(tb["mat"])))
    assert refused(**edit("vert", "mat", len(tb["mat"]), sub="ts")) and refused(**edit("vert", "mat", -1, sub="ts"))
    assert refused(**edit("bounce", "tri", len(tb["tshade"])))
    assert refused(**edit("prim", "op", 7)) and refused(**edit("dir", "op", 3)) and refused(**edit("cam", "mode", 3))
    c = small["cam"].copy()
    c["mode"][0], c["W"][0] = 1, 1
    assert refused(cam=c)
    for table, field, value in (("mat", "tex", len(tb["tex"])), ("tex", "offset", len(tb["texbytes"]) - 2), ("tex", "width", 0), ("tex", "height", 1 << 20),
                                ("light", "tri_count", len(tb["ltri"]) + 1), ("light", "tri_first", 0xFFFFFFFF), ("tshade", "mat", len(tb["mat"]))):
        t = tb[table].copy()
        t[field][-1] = value
        assert refused(dict(tb, **{table: t})), (table, field)
    data, n = SC.case_bytes(tb, small)
    assert H.shade_case_words(data[:-16], sum(n[s] * SC.WORDS[s] for s in SC.SECTIONS)) is None
    # the layout from before the light pickers (its magic, the first 64 B of the header, no pools) is read as a file without picker cases: the same words
    seven = {s: small[s] for s in SC.SECTIONS[:7]}
    data, n = SC.case_bytes(dict(tb, **SC.no_pools()), seven)
    n_words = sum(n[s] * SC.WORDS[s] for s in SC.SECTIONS)
    before = np.array([SC.MAGIC_1], "<u4").tobytes() + data[4:64] + data[96:]
    assert np.array_equal(H.shade_case_words(before, n_words), H.shade_case_words(data, n_words))
    assert H.shade_case_words(before[:-16], n_words) is None and H.shade_case_words(before[:60], n_words) is None
    # the light sets: one file per rule.  Set `k`: corridor(16), fifteen nodes in pre-order, node 0 holds two inner references
    k = tb["meta"]["by_name"]["corridor(16)"]
    st = tb["sets"][k]
    assert st["n_nodes"] == 15 and not (tb["pnodes"]["child0"][st["node_first"]] | tb["pnodes"]["child1"][st["node_first"]]) & SC.LEAF
    for field, value, why in (("light_first", len(tb["plights"]), "lights leave the pool"), ("n_lights", len(tb["plights"]) + 1, "lights leave the pool"),
                              ("sel_first", len(tb["psel"]), "selection table leaves the pool"), ("node_first", len(tb["pnodes"]), "nodes leave the pool"),
                              ("n_nodes", len(tb["pnodes"]) + 1, "nodes leave the pool"), ("root", 15, "root is outside the set's nodes"),
                              ("root", SC.LEAF | 16, "root names a light outside the set")):
        sets = tb["sets"].copy()
        sets[field][k] = value
        assert refused(dict(tb, sets=sets)), field
        assert _tool_refuses(tmp_path, SC.case_bytes(dict(tb, sets=sets), small)[0], why), field
    sets = tb["sets"].copy()
    sets["sel_first"][small["pick"]["set"][0]] = SC.NO_TABLE  # a set without a table is sound, a case that asks for its table is not
    assert small["pick"]["op"][0] == SC.PICK_AT_TABLE and refused(dict(tb, sets=sets)) and not refused(dict(tb, sets=sets), pick=small["pick"][1:2])
    leaf_at = int(np.flatnonzero(tb["pnodes"]["child0"][st["node_first"]:st["node_first"] + 15] & SC.LEAF)[0])
    for node, value, why in ((leaf_at, SC.LEAF | 16, "a leaf reference names a light outside its set"), (leaf_at, SC.NONE, "a leaf reference names a light outside its set"),
                             (3, 3, "an inner reference is not greater than the index of the node that holds it"),
                             (3, 1, "an inner reference is not greater than the index of the node that holds it"), (0, 15, "an inner reference is outside the set's nodes")):
        nodes = tb["pnodes"].copy()
        nodes["child0"][st["node_first"] + node] = value
        assert refused(dict(tb, pnodes=nodes)), (node, value)
        assert _tool_refuses(tmp_path, SC.case_bytes(dict(tb, pnodes=nodes), small)[0], why), (node, value)
    assert not _tool_refuses(tmp_path, b"", "a leaf reference")  # (the helper can tell: an empty file is refused for another reason)
    assert refused(**edit("pick", "op", 5)) and refused(**edit("pick", "set", len(tb["sets"]))) and refused(**edit("near", "set", len(tb["sets"])))
    one = tb["meta"]["by_name"]["random, L=1"]
    c = small["pick"].copy()
    c["op"][0], c["set"][0] = SC.PICK_AT_SCAN, one  # lightPickAt is for two or more lights
    assert refused(pick=c)
    c["op"][0], c["li"][0] = SC.PICK_WEIGHT, 1
    assert refused(pick=c)
    c["li"][0] = 0
    assert not refused(pick=c)


def test_a_digest_is_the_sum_over_its_chunks_explicit_words():
    """The digests are what the explicit cases compute: chunk 0x123 of sincos2pi, of pow01(u, 1/(250+1)), chunk 5 of the logf range, ..., and chunks of every stream of the
    light pickers, from the words of the primitive, pick and step sections."""
    starts = np.cumsum([0] + [s[2] for s in SC.DIGEST_STREAMS])
    assert len(SC.DIGEST_STREAMS) == 36 and SC.DIGEST_STEP0 + 4 == 36
    for stream, chunk in ((0, 0x123), (6, 4095), (19, 5), (22, 8191), (25, 7), (2, 0), (21, 17), (26, 0x123), (27, 4095), (28, 0), (29, 2048), (30, 7), (31, 4095), (32, 0),
                          (33, 4095), (34, 2048), (35, 2048)):
        tb, section, c = SC.digest_chunk_cases(stream, chunk)
        data, n = SC.case_bytes(tb, {section: c})
        w = H.shade_case_words(data, SC.WORDS[section] * len(c)).reshape(-1, SC.WORDS[section])
        assert int(H.shade_digests(int(starts[stream]) + chunk, 1)[0]) == SC.digest_chunk_want(stream, chunk, w), (stream, chunk)


# ---- (c) float64 restatements ---------------------------------------------------------------------------------------------------------------------------------
def _prim_words(c):
    data, _ = SC.case_bytes(SC.no_tables(), dict(prim=c))
    return H.shade_case_words(data, 4 * len(c)).reshape(-1, 4)


def test_sincos2pi_of_every_uniform_against_float64():
    """All 2^24 uniforms the stream can produce: |error| below the project's bound of 2.5e-7 (tests/test_oracle_kat.py), for the cosine and the sine."""
    worst = 0.0
    for block in range(16):
        m = np.arange(block << 20, (block + 1) << 20, dtype=np.uint64)
        c = np.zeros(len(m), SC.PRIM_DT)
        c["op"], c["a"] = SC.OP_SINCOS, SC.bits((m.astype(np.float64) * 2.0 ** -24).astype(F32))
        w = f32(_prim_words(c)[:, :2]).astype(np.float64)
        a = 2.0 * np.pi * (m.astype(np.float64) * 2.0 ** -24)
        worst = max(worst, float(np.abs(w[:, 0] - np.cos(a)).max()), float(np.abs(w[:, 1] - np.sin(a)).max()))
    print(f"sincos2pi: max abs error over 2^24 uniforms {worst:.3e}")
    assert worst < 2.5e-7


# The maxima below are measured on the CPU build (deterministic: a fixed sequence of IEEE operations) over the corpus' primitive cases, rounded up to two significant digits;
# include/trt_prims.h states them beside the functions.
LOGF_MAX_REL = 7.8e-8  # measured 7.790e-08
EXPF_MAX_REL = 8.0e-8  # measured 7.982e-08, x > -86.5
POW01_MAX_REL_PER_EXPONENT = 1.4e-7  # measured 1.340e-07: relative error divided by max(1, |y log x|), y log x > -86.5


def test_logf_expf_and_pow01_of_the_corpus_against_float64(run):
    """Relative error against float64 over the corpus.  trt_expf_neg flushes to 0 at x <= -87 although e^x is still normal down to -87.34, and trt_pow01 does so through
    it: inputs within 0.5 of that threshold (x, or y log x, in [-87.5, -86.5]) are skipped, inputs further below must give exactly 0; pow01's other two exits (x <= FLT_MIN,
    x >= 1) are exact by definition and checked as such.  The skipped share stays below 2 %."""
    c, w = run["cases"]["prim"], run["words"]["prim"]
    with np.errstate(invalid="ignore"):  # the words of the other operations are not numbers
        got = f32(w[:, 0]).astype(np.float64)
        a, b = f32(c["a"]).astype(np.float64), f32(c["b"]).astype(np.float64)
    # logf: positive normal floats
    s = (c["op"] == SC.OP_LOG)
    ref = np.log(a[s])
    rel = np.abs(got[s] - ref) / np.where(ref == 0, 1.0, np.abs(ref))
    log_max = float(rel.max())
    # expf_neg: x <= 0
    s = (c["op"] == SC.OP_EXP) & ~np.isnan(a)
    near = s & (a >= -87.5) & (a <= -86.5)
    flush = s & (a < -87.5)
    assert (got[flush] == 0).all()
    keep = s & ~near & ~flush
    exp_max = float((np.abs(got[keep] - np.exp(a[keep])) / np.exp(a[keep])).max())
    exp_skipped = near.sum() / s.sum()
    # pow01: x in [0, 1], y > 0
    s = (c["op"] == SC.OP_POW) & (a >= 0) & (a <= 1)
    assert np.array_equal(got[s & (b == 1)], a[s & (b == 1)])  # y == 1 is exact
    s &= b != 1
    assert (got[s & (a <= FLT_MIN)] == 0).all() and (got[s & (a >= 1)] == 1).all()
    inner = s & (a > FLT_MIN) & (a < 1)
    with np.errstate(divide="ignore"):
        e = b * np.log(np.where(inner, a, 0.5))
    near = inner & (e >= -87.5) & (e <= -86.5)
    flush = inner & (e < -87.5)
    assert (got[flush] == 0).all()
    keep = inner & ~near & ~flush
    # the error of the exponent y log x enters e^(y log x) relatively: the bound is per unit of max(1, |y log x|)
    rel = np.abs(got[keep] - np.exp(e[keep])) / np.exp(e[keep]) / np.maximum(1.0, np.abs(e[keep]))
    pow_max = float(rel.max())
    pow_skipped = near.sum() / s.sum()
    print(f"max relative error: logf {log_max:.3e} over {int((c['op'] == SC.OP_LOG).sum())}, expf_neg {exp_max:.3e} (skipped {exp_skipped:.2%}), "
          f"pow01 {pow_max:.3e} per max(1, |y log x|) over {int(keep.sum())} (skipped {pow_skipped:.2%})")
    assert exp_skipped <= 0.02 and pow_skipped <= 0.02
    assert log_max <= LOGF_MAX_REL and exp_max <= EXPF_MAX_REL and pow_max <= POW01_MAX_REL_PER_EXPONENT


def test_sample_dir_is_a_unit_vector_at_the_sampled_angle_to_its_axis(run):
    """sampleDir(a, ...) for a unit axis: |result| = 1 and result . a = cos(theta), theta the sampled polar angle: sqrt(1 - u) for the diffuse lobe, u^(1/(Ns+1)) for the
    specular one.  Bounds: about ten binary32 roundings of O(1) quantities (the basis, the combination, two normalisations) — 1e-6 — plus, for the specular lobe, pow01's error
    bound above times max(1, |log(u) / (Ns + 1)|).  Axes that are not unit vectors (zero, NaN: outside the function's domain) are skipped."""
    c, w = run["cases"]["dir"], run["words"]["dir"]
    s = c["op"] == 0
    a = c["a"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        unit = s & (np.abs(np.linalg.norm(a, axis=1) - 1) < 1e-6)
    u = c["b"][:, 0].astype(np.float64)
    spec = c["type"] == 1
    keep = unit
    skipped = 1 - keep.sum() / s.sum()
    out = f32(w).astype(np.float64)
    assert np.abs(np.linalg.norm(out[keep], axis=1) - 1).max() < 1e-6
    with np.errstate(divide="ignore"):
        cos_t = np.where(spec, np.where(u > 0, np.exp(np.log(np.maximum(u, 1e-300)) / (c["x"].astype(np.float64) + 1)), 0.0), np.sqrt(1 - u))
    got = np.einsum("ij,ij->i", out, a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-30))
    with np.errstate(divide="ignore"):
        expo = np.where(u > 0, np.abs(np.log(np.maximum(u, 1e-300)) / (c["x"].astype(np.float64) + 1)), 0.0)
    tol = np.where(spec, 1e-6 + POW01_MAX_REL_PER_EXPONENT * np.maximum(1.0, expo), 1e-6)
    err = np.abs(got - cos_t)[keep]
    print(f"sampleDir: {int(keep.sum())} cases, max |cos error| diffuse {err[~spec[keep]].max():.3e}, specular {err[spec[keep]].max():.3e}, skipped {skipped:.2%}")
    assert (err <= tol[keep]).all(), float(err.max())
    assert skipped <= 0.02


def test_refract_obeys_snells_law(run):
    """refract(I, N, eta) for unit I and N: zero exactly when k = 1 - eta^2 sin^2(theta_i) < 0; otherwise a unit vector whose component across N is eta times I's
    (sin theta_t = eta sin theta_i) and whose component along N points against N (glm's convention: N faces the incoming ray).  Cases with |k| < 1e-6 in float64 (rounding decides the branch there) are skipped."""
    c, w = run["cases"]["dir"], run["words"]["dir"]
    s = c["op"] == 1
    I, N, eta = c["a"].astype(np.float64), c["b"].astype(np.float64), c["x"].astype(np.float64)
    unit = s & (np.abs(np.linalg.norm(I, axis=1) - 1) < 1e-6) & (np.abs(np.linalg.norm(N, axis=1) - 1) < 1e-6)
    dn = np.einsum("ij,ij->i", I, N)
    k = 1 - eta * eta * (1 - dn * dn)
    keep = unit & (np.abs(k) >= 1e-6)
    skipped = 1 - keep.sum() / s.sum()
    T = f32(w).astype(np.float64)
    tir = keep & (k < 0)
    assert (T[tir] == 0).all() and tir.sum() > 1000
    through = keep & (k > 0)
    assert np.abs(np.linalg.norm(T[through], axis=1) - 1).max() < 1e-6 * max(1.0, float(eta[through].max()))
    across = np.cross(T, N) - eta[:, None] * np.cross(I, N)
    assert np.abs(across[through]).max() < 1e-6 * max(1.0, float(eta[through].max()))
    assert (np.einsum("ij,ij->i", T, N)[through] < 0).all()
    print(f"refract: {int(through.sum())} refracted, {int(tir.sum())} reflected, skipped {skipped:.2%}")
    assert skipped <= 0.02
