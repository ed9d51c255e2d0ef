#!/usr/bin/env python3
"""How much of the shadow walks ran beside which other kernel, from the kernel trace of one `rocprofv3 --kernel-trace` run
(<name>_kernel_trace.csv): per kernel family the sum of its launches' durations and the time at least one of them was running, and for the
shadow walks of the timed renders (k_trace_shadow<false, ...>) the milliseconds that lay inside a launch of k_shade, inside a closest-hit
launch, inside both, and beside nothing.  Intervals are the trace's begin and end timestamps; no counters are involved.

    python tools/stream_overlap.py new_kernel_trace.csv [parent_kernel_trace.csv]
"""
import csv
import re
import sys

FAMILIES = (("shadow", r"k_trace_shadow<false"), ("closest", r"k_trace_closest(_binned)?<false"), ("shade_queue", r"k_shade<.*true, false>"),
            ("shade_bounce0", r"k_shade<.*true, true>"), ("tail", r"k_tail<false"), ("resolve", r"k_resolve"))


def load(path):
    fam = {name: [] for name, _ in FAMILIES}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name, pat in FAMILIES:
                if re.search(pat, row["Kernel_Name"]):
                    fam[name].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
                    break
    return fam


def union(iv):
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def length(iv):
    return sum(b - a for a, b in iv)


def intersect(x, y):
    out, i, j = [], 0, 0
    while i < len(x) and j < len(y):
        a, b = max(x[i][0], y[j][0]), min(x[i][1], y[j][1])
        if a < b:
            out.append([a, b])
        if x[i][1] < y[j][1]:
            i += 1
        else:
            j += 1
    return out


def report(path):
    fam = load(path)
    ms = lambda ns: ns / 1e6
    print(path)
    for name, _ in FAMILIES:
        iv = fam[name]
        print("  %-14s launches %4d   sum of durations %9.3f ms   time covered %9.3f ms" % (name, len(iv), ms(length(iv)), ms(length(union(iv)))))
    sh, shade, closest = union(fam["shadow"]), union(fam["shade_queue"] + fam["shade_bounce0"]), union(fam["closest"])
    in_shade, in_closest = intersect(sh, shade), intersect(sh, closest)
    in_both = intersect(in_shade, closest)
    alone = length(sh) - length(in_shade) - length(in_closest) + length(in_both)
    print("  shadow walks: %.3f ms covered; inside k_shade %.3f ms, inside closest-hit launches %.3f ms, inside both %.3f ms, beside neither %.3f ms"
          % (ms(length(sh)), ms(length(in_shade)), ms(length(in_closest)), ms(length(in_both)), ms(alone)))
    everything = union([iv for name, _ in FAMILIES for iv in fam[name]])
    print("  all of these kernels together cover %.3f ms" % ms(length(everything)))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for p in sys.argv[1:]:
        report(p)
