#!/usr/bin/env python3
"""Static instruction-class counts per kernel from a gfx950 assembly file.

  hipcc <the Makefile's flags for qnet32.o> -S --cuda-device-only q-learning_amd/csrc/qnet32.hip -o qnet32.s
  python3 scripts/valu_count.py qnet32.s [kernel-name-substring ...]

Per kernel: MFMA instructions, other vector ALU instructions (v_* that are not v_mfma*), their ratio, LDS, vector memory,
scalar ALU and branch instructions, and the VGPR count of the kernel's metadata.  With --blocks, the same per basic block
(label), so a hot loop's body can be read off.  The counts are static (program text), not executed counts: a loop body
counts once.
"""
import re
import sys
from collections import OrderedDict

CLASSES = ("mfma", "valu", "lds", "vmem", "salu", "branch")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return None


def parse(path):
    kernels = OrderedDict()
    cur = None
    block = None
    vgprs = {}
    func = re.compile(r"^(_Z\w+):")
    label = re.compile(r"^(\.LBB\w+):")
    inst = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
    for line in open(path):
        m = func.match(line)
        if m:
            cur = kernels.setdefault(m.group(1), OrderedDict())
            block = cur.setdefault("entry", dict.fromkeys(CLASSES, 0))
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = label.match(line)
        if m:
            block = cur.setdefault(m.group(1), dict.fromkeys(CLASSES, 0))
            continue
        m = inst.match(line)
        if m:
            c = classify(m.group(1))
            if c:
                block[c] += 1
    name = None
    for line in open(path):
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.vgpr_count:\s+(\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
    return kernels, vgprs


def row(label, c, extra=""):
    ratio = c["valu"] / c["mfma"] if c["mfma"] else float("nan")
    return "%-28s mfma %5d  other-valu %5d  (%5.2f / mfma)  lds %4d  vmem %4d  salu %5d  branch %4d%s" % (
        label, c["mfma"], c["valu"], ratio, c["lds"], c["vmem"], c["salu"], c["branch"], extra)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    blocks = "--blocks" in sys.argv
    if not args:
        sys.exit(__doc__)
    kernels, vgprs = parse(args[0])
    for name, bl in kernels.items():
        if args[1:] and not any(s in name for s in args[1:]):
            continue
        tot = dict.fromkeys(CLASSES, 0)
        for c in bl.values():
            for k in CLASSES:
                tot[k] += c[k]
        print(name)
        print(row("  total", tot, "  vgprs %s" % vgprs.get(name, "?")))
        if blocks:
            for lab, c in bl.items():
                if c["mfma"] or c["valu"] >= 8:
                    print(row("    " + lab, c))


if __name__ == "__main__":
    main()
