#!/usr/bin/env python3
"""Compare the kernels of two sets of `make asm` outputs, symbol by symbol.

    tools/kernel_isa_diff.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...]

A refactor that moves kernels between translation units, or folds copies of device code into one function, is proved
free when every kernel compiles to the instructions it compiled to before.  For each kernel symbol (a function with an
.amdhsa_kernel block) of either set this prints one line: identical, or what differs, of
  - the instruction text: comments and assembler directives dropped, the function index inside local labels
    (.LBB<n>_<m>) normalised since kernels change position;
  - the .amdhsa_ sizes: next free VGPR / SGPR, private segment, group segment.
It only hashes and compares text: it knows no instruction names.  Exit status: 1 if the sets of symbols differ, else 0
(differing kernels are reported, not judged: the caller knows which ones may differ).
"""
import argparse
import collections
import hashlib
import re
import sys

SIZES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_")


def kernels(paths):
    """symbol -> (instruction lines, sizes) for every kernel of the files."""
    bodies, sizes = {}, {}
    for path in paths:
        body = cur = None  # lines of the function being read; the .amdhsa_kernel block being read
        for raw in open(path, encoding="utf-8", errors="replace"):
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                body = bodies.setdefault(m.group(1), [])
                continue
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur, body = sizes.setdefault(m.group(1), {}), None
                continue
            if line == ".end_amdhsa_kernel":
                cur = None
            elif cur is not None:
                m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", line)
                if m and m.group(1) in SIZES:
                    cur[m.group(1)] = m.group(2)
            elif body is not None:
                if line.startswith(".") and not line.endswith(":"):  # a directive (a local label ends with ':')
                    if line.startswith((".section", ".size")):
                        body = None
                    continue
                body.append(LOCAL_LABEL.sub(r".L\1_", line))
    return {s: (bodies.get(s, []), sizes[s]) for s in sizes}


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--old", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--new", nargs="+", required=True, metavar="FILE.s")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    n_same = 0
    for sym in sorted(set(old) & set(new)):
        (ob, osz), (nb, nsz) = old[sym], new[sym]
        what = []
        if ob != nb:
            same_set = collections.Counter(ob) == collections.Counter(nb)
            what.append(f"instructions differ ({len(ob)} -> {len(nb)} lines, {digest(ob)} -> {digest(nb)}; "
                        f"{'the same lines in another order' if same_set else 'other lines'})")
        for k in SIZES:
            if osz.get(k) != nsz.get(k):
                what.append(f"{k} {osz.get(k)} -> {nsz.get(k)}")
        if ob != nb and not any(osz.get(k) != nsz.get(k) for k in SIZES):
            what.append("sizes equal: " + " ".join(f"{k} {nsz.get(k)}" for k in SIZES))
        n_same += not (ob != nb or osz != nsz)
        print(f"{sym}: " + ("identical" if not what else "; ".join(what)))
    for sym in sorted(set(old) - set(new)):
        print(f"{sym}: only in --old")
    for sym in sorted(set(new) - set(old)):
        print(f"{sym}: only in --new")
    print(f"# {len(old)} kernels before, {len(new)} after, {n_same} identical")
    return 1 if set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
