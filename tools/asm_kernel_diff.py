#!/usr/bin/env python3
"""Which kernels of two gfx950 assembly listings of the same source (make asm) differ.

    python tools/asm_kernel_diff.py [--rename OLD=NEW ...] before/rt_kernels.s after/rt_kernels.s

Each kernel's instructions are compared with the label numbers (.LBBn_m) and the
__hip_cuid_ symbol normalised, so that a change to one kernel does not show in the others.
Prints one line per kernel that differs or exists on one side only, with its static
instruction counts by unit (VALU, SALU, LDS, VMEM/SMEM, branches), then the number of
identical kernels.  --rename OLD=NEW (repeatable) replaces the substring OLD of the mangled
names of the "before" listing by NEW, for kernels whose template or function parameters changed.
"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", s)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if not s or s.startswith((";", ".")) and not s.startswith(".LBB"):
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s.split(";")[0].strip())
        s = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", s)
        if s:
            body.append(s)
    return out


def counts(body):
    c = {"valu": 0, "salu": 0, "lds": 0, "mem": 0, "branch": 0}
    for s in body:
        op = s.split()[0]
        if op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_", "s_load", "s_buffer_load")):
            c["mem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


def main():
    args, renames = sys.argv[1:], []
    while args and args[0] == "--rename":
        renames.append(args[1].split("=", 1))
        args = args[2:]
    a, b = kernels(args[0]), kernels(args[1])
    for old, new in renames:
        a = {k.replace(old, new): v for k, v in a.items()}
    same = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}: only in {'after' if k in b else 'before'}")
        elif a[k] == b[k]:
            same += 1
        else:
            print(f"{k}: before {counts(a[k])} after {counts(b[k])}")
    print(f"{same} kernels identical")


if __name__ == "__main__":
    main()
