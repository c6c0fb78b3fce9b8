#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python scripts/isa_diff.py OLD_TREE NEW_TREE unit.hip [unit.hip ...] [--keep DIR]

Each named unit of sessionsimilaritysearch_amd/csrc is compiled in both trees with
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S
split by kernel symbol, stripped of comments and blank lines, and its basic-block labels (.LBB<function>_<block>) are
renumbered in order of appearance.  Per unit it prints "N kernels, M identical", then for each kernel that differs the
demangled name, the instruction counts and, from the kernel's own metadata lines, VGPRs, SGPR spills and scratch bytes.
The exit status is 1 if any kernel differs (2: a unit did not compile).  Text only: no instruction is looked for.

A tree is any directory holding sessionsimilaritysearch_amd/csrc and include, e.g.
    mkdir /tmp/old && git archive HEAD~1 sessionsimilaritysearch_amd/csrc include | tar -x -C /tmp/old
--keep DIR leaves the .s files in DIR/old and DIR/new and reuses a DIR/old/<unit>.s that is already there (the old tree
of a refactor does not change; scan.hip alone takes minutes to compile).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("sessionsimilaritysearch_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
META = (("vgprs", ".vgpr_count:"), ("sgpr_spills", ".sgpr_spill_count:"), ("scratch", ".private_segment_fixed_size:"))


def compile_unit(tree, unit, out, reuse):
    if reuse and os.path.exists(out):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(os.path.abspath(tree), CSRC, unit)
    subprocess.run([hipcc, *FLAGS, src, "-o", out], check=True, cwd=os.path.dirname(src))
    return out


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels_of(path):
    """{symbol: (normalised body lines, {metadata key: value})} of every kernel of one .s file."""
    text = open(path).read()
    meta = {}
    # amdhsa.kernels metadata: one "- .agpr_count:" ... ".name: sym" ... block per kernel
    for block in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):])[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if name:
            meta[name.group(1)] = {k: (re.search(re.escape(key) + r"\s*(\d+)", block) or [None, "?"])[1] for k, key in META}
    out = {}
    for sym in meta:
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), text, re.M | re.S)
        labels, body = {}, []
        for line in m.group(0).splitlines()[1:-1]:
            line = line.split(";")[0].strip()
            if line:
                body.append(line)
        for line in body:
            lm = re.match(r"(\.LBB\d+_\d+):", line)
            if lm:
                labels[lm.group(1)] = ".L%d" % len(labels)
        body = [re.sub(r"\.LBB\d+_\d+", lambda g: labels.get(g.group(0), g.group(0)), line) for line in body]
        out[sym] = (body, meta[sym])
    return out


def n_instr(body):
    return sum(1 for line in body if not line.startswith(".") and not line.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("units", nargs="+")
    ap.add_argument("--keep", metavar="DIR")
    args = ap.parse_args()
    tmp = None if args.keep else tempfile.TemporaryDirectory()
    root = args.keep or tmp.name
    jobs = {}
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        for side, tree in (("old", args.old_tree), ("new", args.new_tree)):
            os.makedirs(os.path.join(root, side), exist_ok=True)
            for unit in args.units:
                out = os.path.join(root, side, os.path.splitext(unit)[0] + ".s")
                jobs[side, unit] = pool.submit(compile_unit, tree, unit, out, bool(args.keep) and side == "old")
    differ = 0
    for unit in args.units:
        try:
            old, new = kernels_of(jobs["old", unit].result()), kernels_of(jobs["new", unit].result())
        except subprocess.CalledProcessError as e:
            print("%s: did not compile (%s)" % (unit, e))
            return 2
        names = sorted(set(old) | set(new))
        same = [s for s in names if s in old and s in new and old[s][0] == new[s][0]]
        print("%s: %d kernels, %d identical" % (unit, len(names), len(same)))
        pretty = demangle(names)
        for s in names:
            if s in same:
                continue
            differ += 1
            print("  " + pretty[s])
            for side, ks in (("old", old), ("new", new)):
                if s not in ks:
                    print("    %s: absent" % side)
                    continue
                body, meta = ks[s]
                print("    %s: %d instructions, %s" % (side, n_instr(body), ", ".join("%s %s" % (k, meta[k]) for k, _ in META)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
