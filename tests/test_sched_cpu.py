"""The host side of the shadow walks' side stream, without a GPU: the placement of a bounce's shadow records at the two ends of the
queues (tinyraytracing_amd/csrc/trt_sched.h, built for the CPU: tests/sched/sched_cpu.cpp) swept over every small size, its edges, the
function under the host sanitizers (a stand-alone program), and the checker of the schedule trace (tests/sched_graph.py) on hand-written
traces: a correct one, and one with each ordering of DESIGN.md §4.3's table taken out, which it has to reject."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import sched_graph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def place(N, parity, prev_at, prev_n, cap):
    """shadowPlace over arrays of cases -> (at, wait)"""
    global _LIB
    if _LIB is None:
        path = os.path.join(ROOT, "tests", "sched", "libsched_cpu.so")
        if not os.path.exists(path):
            subprocess.run(["make", "schedcpu"], cwd=ROOT, check=True, capture_output=True)
        _LIB = ctypes.CDLL(path)
        u64p, u32p, u8p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        _LIB.sched_place.argtypes = [ctypes.c_uint64, u64p, u32p, u64p, u64p, u64p, u64p, u8p]
        _LIB.sched_place.restype = None
    a = [np.ascontiguousarray(np.broadcast_to(x, np.broadcast(N, parity, prev_at, prev_n, cap).shape).ravel(), dtype=t)
         for x, t in ((N, np.uint64), (parity, np.uint32), (prev_at, np.uint64), (prev_n, np.uint64), (cap, np.uint64))]
    at, wait = np.zeros(len(a[0]), np.uint64), np.zeros(len(a[0]), np.uint8)
    ptr = lambda x, t: x.ctypes.data_as(ctypes.POINTER(t))
    _LIB.sched_place(len(at), ptr(a[0], ctypes.c_uint64), ptr(a[1], ctypes.c_uint32), ptr(a[2], ctypes.c_uint64), ptr(a[3], ctypes.c_uint64), ptr(a[4], ctypes.c_uint64),
                     ptr(at, ctypes.c_uint64), ptr(wait, ctypes.c_uint8))
    return at.astype(np.int64), wait.astype(bool)


def test_every_small_size_both_parities():
    """N = 1..64, every n_s and n_active in 0..N, both parities.  The interval being read is where the bounce before was placed: at the
    other end, for the fewest records that bounce can have had room for (n_s, and max(n_s, n_active): a queue never grows) and the most (N)."""
    rows = []
    for N in range(1, 65):
        n_s, n_active = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
        for parity in (0, 1):
            for cap_prev in (n_s, np.maximum(n_s, n_active), np.full_like(n_s, N)):
                rows.append(np.stack([np.full_like(n_s, N), np.full_like(n_s, parity), n_s, n_active, cap_prev], -1).reshape(-1, 5))
    N, parity, n_s, n_active, cap_prev = np.concatenate(rows).T
    prev_at, prev_wait = place(N, parity ^ 1, 0, 0, cap_prev)  # the bounce before, with nothing being read: its own place
    assert not prev_wait.any()
    assert np.array_equal(prev_at, np.where(parity == 1, 0, N - cap_prev))
    at, wait = place(N, parity, prev_at, n_s, n_active)
    assert (at >= 0).all() and (at + n_active <= N).all()                   # n_active records inside [0, N)
    assert np.array_equal(at, np.where(parity == 1, N - n_active, 0))          # ... at the bounce's own end
    disjoint = (n_s == 0) | (n_active == 0) | (at + n_active <= prev_at) | (prev_at + n_s <= at)
    assert np.array_equal(~wait, disjoint)
    assert wait.any() and (~wait).any()
    # the records of the bounce before packed against their end (it had room for exactly n_s): free exactly up to n_s + n_active == N
    packed = cap_prev == n_s
    full = packed & (n_s > 0) & (n_active > 0)
    assert np.array_equal(wait[full], (n_s + n_active > N)[full])
    # an even bounce before writes upward from 0 whatever room it had: likewise
    low = (parity == 1) & (n_s > 0) & (n_active > 0)
    assert np.array_equal(wait[low], (n_s + n_active > N)[low])


@pytest.mark.parametrize("N", [1, 2, 63, 64, 1000, 0x7FFF0000, 2 ** 40])
def test_edges(N):
    for n_s in sorted({1, N // 3, N // 2, N - 1, N} - {0}):
        for parity in (0, 1):
            prev_at = 0 if parity == 1 else N - n_s
            fits = N - n_s
            at, wait = place(N, parity, prev_at, n_s, fits)          # n_s + n_active == N
            assert not wait[0] and at[0] == (N - fits if parity else 0)
            if fits + 1 <= N:
                at, wait = place(N, parity, prev_at, n_s, fits + 1)  # N + 1
                assert wait[0] and at[0] == (N - fits - 1 if parity else 0)
    assert not place(N, 0, 0, N, 0)[1][0] and not place(N, 1, 0, 0, N)[1][0]  # nothing to write, nothing being read


def test_placement_under_the_host_sanitizers(tmp_path):
    """tests/sched/sched_san.cpp with the CPU build compiled in, under AddressSanitizer and UBSan: a stand-alone program."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "sched_san")
    cmd = [cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
           "-I" + os.path.join(ROOT, "tinyraytracing_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sched", "sched_cpu.cpp"),
           os.path.join(ROOT, "tests", "sched", "sched_san.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the checker on hand-written traces.  One light, passes of 100 paths.  Pass 0: four bounces whose records never meet the interval
# being read (30 + 60 <= 100, ...), then k_tail.  Pass 1: bounce 1 (70 paths) has to wait for the walk of bounce 0 (60 records); then the
# queue is empty and the resolve follows the last walk.
P = 100
LACC = ("Lacc", 0, P)


def bounce(ps, b, n, at, n_s, waits=(), fused=False):
    """closest, k_shade and publish of bounce b over n paths on slot0, then the bounce's shadow walk of n_s records on the side stream"""
    cur, e = b & 1, str(b & 1)
    out = []
    if not fused:
        out.append(dict(op="closest", pass_=ps, bounce=b, light=-1, stream="slot0", reads=[("Q%d" % cur, 0, n)], writes=[("hit", 0, n)]))
    out.append(dict(op="shade", pass_=ps, bounce=b, light=-1, stream="slot0", waits=list(waits), record="shade" + e,
                    reads=([] if fused else [("hit", 0, n), ("Q%d" % cur, 0, n)]),
                    writes=[("Q%d" % (cur ^ 1), 0, n), ("shadow0", at, at + n), ("d_counts", b, b + 1)] + ([LACC] if b == 0 else [])))
    out.append(dict(op="publish", pass_=ps, bounce=b, light=-1, stream="slot0", reads=[("d_counts", b, b + 2)]))
    if n_s:
        out.append(dict(op="shadow", pass_=ps, bounce=b, light=0, stream="side", waits=["shade" + e], record="shadow" + e, reads=[("shadow0", at, at + n_s), LACC], writes=[LACC]))
    return out


def good_trace(tail=True):
    t = [dict(op="clear", pass_=0, bounce=-1, light=-1, stream="call", record="begin", writes=[("stats", 0, 1), ("sum", 0, 10)]),
         dict(op="memset", pass_=0, bounce=-1, light=-1, stream="slot0", waits=["begin"], writes=[("d_counts", 0, 4096)])]
    t += bounce(0, 0, 100, 0, 30, fused=True)
    t += bounce(0, 1, 60, 40, 25)                      # [40, 100) beside the walk over [0, 30)
    t += bounce(0, 2, 35, 0, 20, waits=["shadow0"])    # [0, 35) beside the walk over [40, 65); bounce 0's walk read [0, 30)
    t += bounce(0, 3, 30, 70, 10, waits=["shadow1"])
    if tail:
        t.append(dict(op="tail", pass_=0, bounce=4, light=-1, stream="slot0", waits=["shadow1"], reads=[("Q0", 0, 12), LACC], writes=[LACC]))
    t.append(dict(op="resolve", pass_=0, bounce=-1, light=-1, stream="slot0", waits=[] if tail else ["shadow1"], record="resolved", reads=[LACC, ("sum", 0, 10)], writes=[("sum", 0, 10)]))
    t.append(dict(op="memset", pass_=1, bounce=-1, light=-1, stream="slot0", writes=[("d_counts", 0, 4096)]))
    t += bounce(1, 0, 100, 0, 60, fused=True)
    t += bounce(1, 1, 70, 30, 40, waits=["shadow0"])   # [30, 100) meets [0, 60)
    t.append(dict(op="resolve", pass_=1, bounce=-1, light=-1, stream="slot0", waits=["resolved", "shadow1"], record="resolved", reads=[LACC, ("sum", 0, 10)], writes=[("sum", 0, 10)]))
    t.append(dict(op="finalize", pass_=0, bounce=-1, light=-1, stream="call", waits=["resolved"], reads=[("sum", 0, 10), ("stats", 0, 1)]))
    return t


def ops_of(trace):
    return G.parse("\n".join(G.format_op(d["op"], d["pass_"], d["bounce"], d["light"], d["stream"], d.get("waits", ()), d.get("record"), d.get("reads", ()), d.get("writes", ()))
                             for d in trace))


def pick(trace, op, ps, b):
    (d,) = [d for d in trace if d["op"] == op and d["pass_"] == ps and d["bounce"] == b]
    return d


def violations(trace):
    ops = ops_of(trace)
    return [(kind, (ops[i].op, ops[i].pass_, ops[i].bounce), (ops[j].op, ops[j].pass_, ops[j].bounce)) for (kind, i, j, _) in G.check(ops)]


@pytest.mark.parametrize("tail", [True, False])
def test_checker_accepts_the_correct_traces(tail):
    ops = ops_of(good_trace(tail))
    assert G.check(ops) == []
    G.assert_ordered(ops)
    reach = G.before(ops)
    sh0, shade1 = G.find(ops, "shadow", 0, 0)[0], G.find(ops, "shade", 0, 1)[0]
    assert not (reach[shade1.index] >> sh0.index) & 1 and not (reach[sh0.index] >> shade1.index) & 1  # the pair the side stream is for: free to overlap


def test_parse_round_trip():
    line = G.format_op("shadow", 2, 7, 1, "side", ["shade1"], "shadow1", [("shadow1", 5, 9), ("Lacc", 0, 64)], [("Lacc", 0, 64)])
    (o,) = G.parse("noise\n" + line + "\ntrt_render: k_shade one\n")
    assert (o.op, o.pass_, o.bounce, o.light, o.stream, o.waits, o.record) == ("shadow", 2, 7, 1, "side", ["shade1"], "shadow1")
    assert o.reads == [("shadow1", 5, 9), ("Lacc", 0, 64)] and o.writes == [("Lacc", 0, 64)]


def test_checker_rejects_each_missing_edge():
    # shadow(b) after shade(b)
    t = good_trace()
    pick(t, "shadow", 0, 1)["waits"] = []
    assert ("race", ("shade", 0, 1), ("shadow", 0, 1)) in violations(t)
    # shadow(b) after shadow(b - 1): the order of the additions into Lacc (a walk on a stream of its own)
    t = good_trace()
    pick(t, "shadow", 0, 2)["stream"] = "side2"
    v = violations(t)
    assert ("lacc", ("shadow", 0, 1), ("shadow", 0, 2)) in v and ("race", ("shadow", 0, 1), ("shadow", 0, 2)) in v
    # ... and enqueued in another order
    t = good_trace()
    i, j = t.index(pick(t, "shadow", 0, 1)), t.index(pick(t, "shadow", 0, 2))
    t[i]["bounce"], t[j]["bounce"] = 2, 1
    assert any(k == "lacc" for (k, _, _) in violations(t))
    # k_tail after every shadow launch
    t = good_trace()
    pick(t, "tail", 0, 4)["waits"] = []
    assert ("race", ("shadow", 0, 3), ("tail", 0, 4)) in violations(t)
    # the resolve after every shadow launch (a pass whose queue ran empty: no k_tail before it)
    t = good_trace()
    pick(t, "resolve", 1, -1)["waits"] = ["resolved"]
    assert ("race", ("shadow", 1, 1), ("resolve", 1, -1)) in violations(t)
    # the next pass's bounce 0 after every shadow launch of the pass before (which ended without k_tail)
    t = good_trace(tail=False)
    assert violations(t) == []
    pick(t, "resolve", 0, -1)["waits"] = []
    v = violations(t)
    assert ("race", ("shadow", 0, 3), ("shade", 1, 0)) in v and ("race", ("shadow", 0, 2), ("shade", 1, 0)) in v
    # shade(b + 1) against the interval shadow(b) reads, where the two meet
    t = good_trace()
    pick(t, "shade", 1, 1)["waits"] = []
    assert violations(t) == [("race", ("shadow", 1, 0), ("shade", 1, 1))]
    # shade(b + 1) against the interval shadow(b - 1) read: its own end
    t = good_trace()
    pick(t, "shade", 0, 2)["waits"] = []
    assert violations(t) == [("race", ("shadow", 0, 0), ("shade", 0, 2))]
    # a walk that reads past what the placement allowed for
    t = good_trace()
    pick(t, "shade", 0, 1)["writes"][1] = ("shadow0", 25, 85)
    assert ("race", ("shadow", 0, 0), ("shade", 0, 1)) in violations(t)
