"""The shading functions of trt_path.h (cameraRay, makeVertex, lightSample, nextRayDecide / nextRayFinish, sampleDir, refract / reflect, shadeBegin -> shadeNext), the
light pickers (lightWeight, lightPickAt / lightPick, lightNodeStep, lightPickNear) and the primitives of trt_prims.h / trt_exact.h under them as gfx950 compiles them (tools/shade_case_check, one thread per case) against the CPU build of the same
functions (tests/hostsim): every output word of the corpus of tests/shade_cases.py equal, and every digest of the exhaustive sweeps equal.  What the corpus covers and
that it can tell an altered function from the real one is tests/test_shade_cases_cpu.py's business."""
import os
import subprocess

import numpy as np
import pytest

import hostsim_lib as H
import shade_cases as SC
import tinyraytracing_amd as T

pytestmark = pytest.mark.gpu
EXE = os.path.join(T.REPO_ROOT, "tools", "shade_case_check")


def _run(args):
    assert os.path.exists(EXE), "tools/shade_case_check is not built (make shadecheck)"
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _inputs(c):
    return " ".join(f"{k}={c[k]!r}" for k in c.dtype.names if not k.startswith("pad"))


def _differences(name, gpu, cpu, cases):
    bad = np.nonzero((gpu != cpu).any(1))[0]
    text = "; ".join(f"{name} case {i}: gpu {[hex(int(x)) for x in gpu[i]]} cpu {[hex(int(x)) for x in cpu[i]]} {_inputs(cases[i])}" for i in bad[:6])
    print(f"{name}: {len(gpu)} cases, {len(bad)} differ")
    return len(bad), text


def test_gfx950_computes_the_cpu_builds_words_case_by_case(tmp_path):
    """One run of tools/shade_case_check over the corpus (532 957 primitive, 11 748 camera, 104 940 vertex, 129 424 light, 125 204 next-ray, 108 383 direction, 100 288
    bounce, 102 188 pick, 187 441 step and 140 281 near cases): every word equals the CPU build's.  A failure names the first six differing cases of each section with their
    inputs and both sides' words.  The table form and the scan form of lightPickAt / lightPick (adjacent pick cases) agree on the device's own words as well."""
    tb, cases = SC.corpus(H.make_material_dev)
    data, n = SC.case_bytes(tb, cases)
    case_file, result_file = str(tmp_path / "cases.bin"), str(tmp_path / "result.bin")
    with open(case_file, "wb") as f:
        f.write(data)
    print(_run([case_file, result_file]).strip())
    n_words = sum(n[s] * SC.WORDS[s] for s in SC.SECTIONS)
    gpu = SC.split_words(np.fromfile(result_file, "<u4"), n)
    cpu = SC.split_words(H.shade_case_words(data, n_words), n)
    diffs = [_differences(s, gpu[s], cpu[s], cases[s]) for s in SC.SECTIONS]
    assert [d[0] for d in diffs] == [0] * len(SC.SECTIONS), "\n".join(d[1] for d in diffs if d[0])
    table = np.flatnonzero(np.isin(cases["pick"]["op"], [SC.PICK_AT_TABLE, SC.PICK_TABLE]))
    assert len(table) > 10000 and (cases["pick"]["op"][table + 1] == cases["pick"]["op"][table] + 1).all()
    assert np.array_equal(gpu["pick"][table], gpu["pick"][table + 1]), "the table and the scan form of the pick differ on the device"


def test_gfx950_computes_the_cpu_builds_digests_of_the_exhaustive_sweeps(tmp_path):
    """One run in each digest mode: all 2^24 uniforms through sincos2pi, sqrt(u), sqrt(1 - u), pow01(u, 1 / (Ns + 1)) and pow01(u, Ns) for the eight Ns; every float of
    [2^-126, 2^-125) through logf, of [-88, -86) through expf_neg, of the exponent fields 30..34 and 252..255 through the square roots; three 2^20-point sweeps; all 2^24 uniforms through lightPickAt on four
    tables (two of them by scan as well) and through lightNodeStep on four (node, point) pairs.  Every
    digest of 4096 inputs equals the CPU build's; a chunk that differs is run again as explicit cases, so that the message names its first differing input."""
    gpu = []
    for mode in ("digest", "digest-pickers"):
        result_file = str(tmp_path / f"{mode}.bin")
        print(_run([mode, result_file]).strip())
        gpu.append(np.fromfile(result_file, "<u8"))
    gpu = np.concatenate(gpu)
    cpu = H.shade_digests()
    assert len(gpu) == len(cpu) == SC.DIGEST_TOTAL
    bad = np.nonzero(gpu != cpu)[0]
    print(f"{len(cpu)} digests, {len(bad)} differ")
    if not len(bad):
        return
    starts = np.cumsum([0] + [s[2] for s in SC.DIGEST_STREAMS])
    text = []
    for i in bad[:3]:
        stream = int(np.searchsorted(starts, i, "right") - 1)
        tb, section, c = SC.digest_chunk_cases(stream, int(i - starts[stream]))
        data, n = SC.case_bytes(tb, {section: c})
        case_file, out_file = str(tmp_path / f"chunk{i}.bin"), str(tmp_path / f"chunk{i}.out")
        with open(case_file, "wb") as f:
            f.write(data)
        _run([case_file, out_file])
        g = np.fromfile(out_file, "<u4").reshape(-1, SC.WORDS[section])
        h = H.shade_case_words(data, SC.WORDS[section] * len(c)).reshape(-1, SC.WORDS[section])
        text.append(f"{SC.DIGEST_STREAMS[stream][0]}, chunk {int(i - starts[stream])}: " + _differences("digest chunk", g, h, c)[1])
    raise AssertionError(f"{len(bad)} of {len(cpu)} digests differ: " + "\n".join(text))
