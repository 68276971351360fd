#!/usr/bin/env python3
"""Instruction counts of k_flushw's band loops from the compiler's assembly.

    make asm            (hipcc --save-temps: lpg_kernels-hip-amdgcn-amd-amdhsa-gfx950.s)
    python3 tools/flushw_asm_stats.py FILE.s [KMAX NB LB WPB]      (default 96 2 1 8)

Prints the kernel's register and scratch figures and, for every stretch of
code between two s_barrier that holds the band's MFMAs, the instruction mix:
the stretch ending at the full-band loop's barrier is one band of that loop.
"""
from __future__ import annotations

import collections
import re
import sys


def kernel_text(lines, tag):
    name = None
    for ln in lines:
        m = re.match(r"^(_ZN3lpg8k_flushw\w+):", ln)
        if m and tag in m.group(1):
            name = m.group(1)
            break
    if name is None:
        raise SystemExit(f"no k_flushw instantiation matching {tag}")
    i0 = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for ln in lines[i1:i1 + 400]:
        m = re.match(r"^\s*[;.]\s*(\.?\w[\w .]*?):?\s+(\d+)\s*$", ln)
        if m and m.group(1) in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "NumSgprs", "LDSByteSize"):
            meta.setdefault(m.group(1), int(m.group(2)))
    return name, lines[i0 + 1:i1], meta


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith(("global_load", "buffer_load", "flat_load")):
        return "vmem_load"
    if op.startswith(("global_store", "buffer_store", "flat_store")):
        return "vmem_store"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64")):
        return "valu_int_mul"
    if re.match(r"v_cmpx?_\w+_[iu]64", op):
        return "valu_cmp64"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path = sys.argv[1]
    k = sys.argv[2:6] if len(sys.argv) >= 6 else ["96", "2", "1", "8"]
    tag = "".join(f"Li{v}E" for v in k)
    lines = open(path).read().split("\n")
    name, body, meta = kernel_text(lines, tag)
    print(name)
    print("  " + "  ".join(f"{a} {b}" for a, b in sorted(meta.items())))
    ins = []                                   # (op, operands) and ("label", name)
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            ins.append(("label", t[:-1]))
        elif not t.startswith("."):
            ins.append((t.split()[0], t))
    where = {x[1]: i for i, x in enumerate(ins) if x[0] == "label"}
    for i, (op, t) in enumerate(ins):
        if not (op.startswith("s_cbranch") or op == "s_branch"):
            continue
        j = where.get(t.split()[-1])
        if j is None or j > i:
            continue                           # forward branch
        loop = [x for x in ins[j:i + 1] if x[0] != "label"]
        ops = [x[0] for x in loop]
        if ops.count("s_barrier") != 1 or not any(o.startswith("v_mfma") for o in ops):
            continue                           # not a band loop (the item loop holds several barriers)
        c = collections.Counter(classify(o) for o in ops if o != "s_barrier")
        tot = sum(c.values())
        print(f"  band loop {t.split()[-1]}: {tot} instructions per band, {tot - c['mfma']} not MFMA")
        print("    " + "  ".join(f"{a} {b}" for a, b in sorted(c.items())))


if __name__ == "__main__":
    main()
