#!/usr/bin/env python3
"""Kernel-by-kernel ISA comparison of two builds of trt_api.hip's device code (profiles/pixels_cost_1080p.txt, "ISA").

Every kernel of the OLD code object must have the same instructions (branch labels and symbol names aside) and the same
resources (VGPRs, SGPRs, LDS, kernarg bytes, scratch, spills) in the NEW one.  Symbol names that a change of template parameters
renames are mapped with --rename OLD_REGEX=NEW (applied to the demangled old names; repeatable).

    hipcc <HIPFLAGS of the Makefile> --cuda-device-only -c -o old.co tinyraytracing_amd/csrc/trt_api.hip   # at the parent commit
    hipcc <HIPFLAGS of the Makefile> --cuda-device-only -c -o new.co tinyraytracing_amd/csrc/trt_api.hip
    python3 tools/isa_diff.py old.co new.co [--rename ...]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
KEYS = ["vgpr_count", "sgpr_count", "group_segment_fixed_size", "kernarg_segment_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"]


def unbundle(co, tmp):
    targets = subprocess.run([f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={co}"], capture_output=True, text=True, check=True).stdout
    target = next(t for t in targets.split() if "gfx950" in t)
    elf = os.path.join(tmp, os.path.basename(co) + ".elf")
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={co}", f"--targets={target}", f"--output={elf}"], check=True)
    return elf


def functions(elf):
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", elf], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.strip() == "...":
            continue  # objdump's mark for the zero padding up to the next function's alignment: no instruction, and it moves with the layout
        elif cur and line.strip():
            ins = re.sub(r"^[0-9a-f]+:\s*", "", line.split("//")[0].strip())
            out[cur].append(re.sub(r"<[^>]+>", "<L>", ins))
    return out


def resources(elf):
    text = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", elf], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = tuple((re.search(r"\." + k + r":\s+(\S+)", blk) or [None, None])[1] for k in KEYS)
    return out


def demangle(names):
    names = list(names)
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], help="OLD_REGEX=REPLACEMENT on demangled old names")
    ap.add_argument("--drop", action="append", default=[], help="OLD_REGEX=REPLACEMENT on demangled new names (e.g. a new defaulted argument)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        eo, en = unbundle(a.old, tmp), unbundle(a.new, tmp)
        fo, fn, ro, rn = functions(eo), functions(en), resources(eo), resources(en)
    do, dn = demangle(fo), demangle(fn)

    def sub(rules, s):
        for r in rules:
            pat, rep = r.split("=", 1)
            s = re.sub(pat, rep, s)
        return s

    by_name = {sub(a.drop, dn[k]): k for k in fn}
    bad = 0
    matched = set()
    for k in fo:
        want = sub(a.rename, do[k])
        nk = by_name.get(want)
        if nk is None:
            print("MISSING ", do[k])
            bad += 1
            continue
        matched.add(nk)
        if fo[k] != fn[nk] or ro.get(k) != rn.get(nk):
            print("CHANGED ", do[k], f"({len(fo[k])} -> {len(fn[nk])} instructions, resources {ro.get(k)} -> {rn.get(nk)})")
            bad += 1
    print(f"{len(fo) - bad} of {len(fo)} kernels of the old build identical in the new one ({sum(len(v) for v in fo.values())} instructions); "
          f"{len(fn) - len(matched)} new kernels:")
    for k in sorted(set(fn) - matched, key=lambda k: dn[k]):
        print("  +", dn[k].split("(")[0])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
