"""The schedule of a render call, read from the `trt_sched:` lines the pass loop prints under TRT_DEBUG with TRT_DEBUG_SCHEDULE=1
(tinyraytracing_amd/csrc/trt_api.hip SchedTrace), as a graph: one node per enqueued operation; an edge from every operation to the next
one on its stream, and from the operation an event was last recorded behind to every operation whose stream was told to wait for that
event (the record in force when the wait was issued, which is the one latest in the trace: the lines come in the order of the host's
calls).  check() returns what the happens-before relation of that graph leaves open:

  * two operations that touch overlapping element ranges of one buffer, at least one of them writing, and are not ordered;
  * the operations of one pass that write Lacc not following each other in bounce order and, within a bounce, light order (k_shade
    before the bounce's shadow walks), each ordered behind the one before — the order of the fp32 additions into a path's sum.

Buffers belong to a pass slot (the stream slotN of the pass; `side` serves slot0, the only slot of a call that uses it), except the
per-pixel sums and the counters of the call, which every slot shares."""
import re
from collections import namedtuple

Op = namedtuple("Op", "index op pass_ bounce light stream waits record reads writes line")
SHARED = ("sum", "stats")
_LINE = re.compile(r"trt_sched: op=(\w+) pass=(\d+) bounce=(-?\d+) light=(-?\d+) stream=(\w+) wait=(\S+) record=(\S+) read=(\S+) write=(\S+)")
_IV = re.compile(r"(\w+)\[(\d+),(\d+)\)")


def _intervals(text):
    if text == "-":
        return []
    got = [(m.group(1), int(m.group(2)), int(m.group(3))) for m in _IV.finditer(text)]
    assert got and _IV.sub("", text).strip(",") == "", text
    return got


def parse(text):
    ops = []
    for line in text.splitlines():
        if "trt_sched:" not in line:
            continue
        m = _LINE.search(line)
        assert m, line
        waits = [] if m.group(6) == "-" else m.group(6).split(",")
        record = None if m.group(7) == "-" else m.group(7)
        ops.append(Op(len(ops), m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5), waits, record,
                      _intervals(m.group(8)), _intervals(m.group(9)), line.strip()))
    return ops


def format_op(op, pass_, bounce, light, stream, waits=(), record=None, reads=(), writes=()):
    """A trace line from its fields, for hand-written traces: reads / writes are (buffer, lo, hi)."""
    iv = lambda l: ",".join("%s[%d,%d)" % t for t in l) or "-"
    return "trt_sched: op=%s pass=%d bounce=%d light=%d stream=%s wait=%s record=%s read=%s write=%s" % (
        op, pass_, bounce, light, stream, ",".join(waits) or "-", record or "-", iv(reads), iv(writes))


def before(ops):
    """before[j]: bit i set = operation i happens before operation j."""
    last_on, recorded, reach = {}, {}, []
    for o in ops:
        preds = []
        if o.stream in last_on:
            preds.append(last_on[o.stream])
        preds += [recorded[e] for e in o.waits if e in recorded]  # a wait for an event never recorded is no wait
        r = 0
        for p in preds:
            r |= reach[p] | (1 << p)
        reach.append(r)
        last_on[o.stream] = o.index
        if o.record:
            recorded[o.record] = o.index
    return reach


def _slot(o):
    return o.stream if o.stream.startswith("slot") else "slot0"


def _touches(o):
    for write, l in ((False, o.reads), (True, o.writes)):
        for (buf, lo, hi) in l:
            if hi > lo:
                yield (buf if buf in SHARED else (_slot(o), buf)), lo, hi, write


def lacc_key(o):
    # within a bounce: k_shade (light -1), then the lights; k_rays_pack (bounce -1) first; k_tail carries the bounce it starts at, past every walk
    return (o.bounce, o.light)


def check(ops):
    """-> list of (kind, i, j, what): kind 'race' (conflicting, unordered) or 'lacc' (Lacc writers out of order / unordered)."""
    reach = before(ops)
    bad = []
    by_buf = {}
    for o in ops:
        for key, lo, hi, write in _touches(o):
            by_buf.setdefault(key, []).append((o.index, lo, hi, write))
    for key, uses in by_buf.items():
        for a in range(len(uses)):
            i, lo_i, hi_i, w_i = uses[a]
            for b in range(a + 1, len(uses)):
                j, lo_j, hi_j, w_j = uses[b]
                if i == j or not (w_i or w_j) or hi_i <= lo_j or hi_j <= lo_i:
                    continue
                if not (reach[j] >> i) & 1:
                    bad.append(("race", i, j, "%s [%d,%d) / [%d,%d)" % (key if isinstance(key, str) else key[1], lo_i, hi_i, lo_j, hi_j)))
    passes = {}
    for o in ops:
        if any(buf == "Lacc" and hi > lo for (buf, lo, hi) in o.writes):
            passes.setdefault((_slot(o), o.pass_), []).append(o)
    for writers in passes.values():
        for prev, nxt in zip(writers, writers[1:]):
            if not lacc_key(prev) < lacc_key(nxt):
                bad.append(("lacc", prev.index, nxt.index, "enqueued out of bounce / light order"))
            elif not (reach[nxt.index] >> prev.index) & 1:
                bad.append(("lacc", prev.index, nxt.index, "not ordered"))
    return sorted(set(bad))


def assert_ordered(ops):
    bad = check(ops)
    assert not bad, "\n".join("%s: %s\n    %s\n    %s" % (k, what, ops[i].line, ops[j].line) for (k, i, j, what) in bad[:8])


def find(ops, op, pass_=None, bounce=None, light=None):
    return [o for o in ops if o.op == op and (pass_ is None or o.pass_ == pass_) and (bounce is None or o.bounce == bounce) and (light is None or o.light == light)]
