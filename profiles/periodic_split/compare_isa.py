#!/usr/bin/env python3
"""Compares the gfx950 ISA listings of two builds kernel by kernel: compare_isa.py PARENT_LIB_DIR BRANCH_LIB_DIR

A kernel = a line `_ZN4jinc...kernel...:` up to the next `.Lfunc_end`.  Compared per symbol: the instruction text (comment lines and
trailing comments dropped; the per-function index of local labels .LBB<n>_, .Lfunc_end<n>, .Ltmp<n> normalised, since it counts the
functions of the unit) and the symbol's `.amdhsa_kernel ... .end_amdhsa_kernel` block (registers, LDS, scratch, occupancy).  The
parent's kernel_periodic-gfx950.s is held against the union of the branch's kernel_periodic*-gfx950.s; every other listing against
the listing of the same name.  Prints a summary; exit status 1 when anything differs.
"""
import glob
import os
import re
import sys

KERNEL = re.compile(r"^(_ZN4jinc\S*kernel\S*):")
LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")


def normal(line):
    line = line.split(";", 1)[0].rstrip()  # (no string operands in these listings: a ';' starts a comment)
    return LABEL.sub(lambda m: "." + m.group(1) + "N", line)


def kernels_of(path):
    """{symbol: (instruction lines, descriptor lines)} of one listing."""
    code, desc, cur, body, block = {}, {}, None, None, None
    for raw in open(path):
        if block is not None:  # inside .amdhsa_kernel ... .end_amdhsa_kernel
            if raw.strip().startswith(".end_amdhsa_kernel"):
                block = None
            else:
                block.append(normal(raw).strip())
            continue
        if raw.strip().startswith(".amdhsa_kernel "):
            block = desc.setdefault(raw.split()[1], [])
            assert not block, f"two descriptors of {raw.split()[1]} in {path}"
            block.append("")
            continue
        m = KERNEL.match(raw)
        if m and cur is None:
            cur, body = m.group(1), []
        elif cur is not None and raw.startswith(".Lfunc_end"):
            assert cur not in code, f"{cur} twice in {path}"
            code[cur], cur = body, None
        elif cur is not None and normal(raw).strip():
            body.append(normal(raw))
    return {k: (v, desc.get(k)) for k, v in code.items()}


def main(parent, branch):
    bad = 0
    name = lambda p: os.path.basename(p)
    pfiles = {name(p): p for p in glob.glob(os.path.join(parent, "*-gfx950.s"))}
    bfiles = {name(p): p for p in glob.glob(os.path.join(branch, "*-gfx950.s"))}
    split = sorted(n for n in bfiles if n.startswith("kernel_periodic"))
    print(f"parent listings: {len(pfiles)}, branch listings: {len(bfiles)}; periodic units of the branch: {', '.join(split)}")

    want = kernels_of(pfiles["kernel_periodic-gfx950.s"])
    got, where = {}, {}
    for n in split:
        ks = kernels_of(bfiles[n])
        print(f"  {n}: {len(ks)} kernels, {sum(len(c) for c, _ in ks.values())} instruction lines")
        for k, v in ks.items():
            if k in got:
                print(f"EMITTED TWICE: {k} in {where[k]} and {n}")
                bad += 1
            got[k], where[k] = v, n
    missing, new = sorted(set(want) - set(got)), sorted(set(got) - set(want))
    print(f"kernel symbols: parent {len(want)}, branch {len(got)}, missing {len(missing)}, new {len(new)}")
    for k in missing + new:
        print(("MISSING: " if k in want else "NEW: ") + k)
    bad += len(missing) + len(new)
    code_diff = [k for k in want if k in got and want[k][0] != got[k][0]]
    desc_diff = [k for k in want if k in got and (want[k][1] is None or want[k][1] != got[k][1])]
    print(f"instruction text differs: {len(code_diff)} of {len(want)}; .amdhsa_kernel block differs: {len(desc_diff)} of {len(want)}")
    for k in sorted(set(code_diff + desc_diff)):
        print(f"DIFFERENT: {k} ({where[k]})")
    bad += len(code_diff) + len(desc_diff)

    others = sorted(n for n in set(pfiles) | set(bfiles) if not n.startswith("kernel_periodic"))
    changed = []
    for n in others:
        if n not in pfiles or n not in bfiles:
            changed.append(n + " (on one side only)")
        elif open(pfiles[n]).read() != open(bfiles[n]).read():  # byte for byte
            changed.append(n)
    print(f"other listings: {len(others)}, changed: {len(changed)}")
    for n in changed:
        print("CHANGED: " + n)
    bad += len(changed)
    print("IDENTICAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
