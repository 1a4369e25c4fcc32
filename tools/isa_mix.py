#!/usr/bin/env python3
"""Instruction mix of a kernel's MFMA loops, from the gfx950 assembly of one translation unit of csrc/ (no GPU needed):

    python tools/isa_mix.py kernels_syrk_uv.hip syrk_uv16c_kernel            # compile with the Makefile's flags, then report
    python tools/isa_mix.py --asm unit.s kernels_syrk_uv.hip syrk_uv16c_kernel   # report on an assembly file made earlier
    python tools/isa_mix.py --markdown ...                                   # the table as markdown rows

For every basic block of the named kernel that holds MFMAs it prints the instruction counts by class -- MFMA, vector ALU, vector
memory, LDS, s_waitcnt, other scalar -- and the instructions per MFMA.  A wave alone on its SIMD pays an issue turn for EVERY
instruction of its stream, so in such a loop the instructions per MFMA are the time.  A basic block begins at a
label or behind a branch and ends with a branch.  Instructions are classified by prefix and opcode family only (`v_mfma` /
`v_smfmac`; `v_`; `global_` / `flat_` / `buffer_` / `scratch_`; `ds_`; `s_waitcnt`; `s_`); `private` counts the vector-memory
instructions that address the private segment (`scratch_`, or `buffer_` through the scratch descriptor s[0:3])."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_isa import ROOT, demangle, kernels_of, make_flags  # noqa: E402

CLASSES = ("mfma", "valu", "vmem", "lds", "waitcnt", "salu")
TITLES = {"mfma": "MFMA", "valu": "vector ALU", "vmem": "vector memory", "lds": "LDS", "waitcnt": "s_waitcnt", "salu": "other scalar"}


def classify(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_", "tbuffer_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_"):
        return "salu"
    raise ValueError("instruction of no known class: %s" % op)


def is_private(op, operands):
    return op.startswith("scratch_") or (op.startswith("buffer_") and re.search(r"\bs\[0:3\]", operands) is not None)


def blocks_of(code):
    """[(label or None, [(opcode, operands), ...]), ...] of a kernel's instruction lines (kernel_isa.kernels_of): a block begins at a
    label or behind a branch"""
    out, label, cur = [], None, []
    for line in code:
        tok = line.strip()
        if tok.endswith(":"):
            if cur:
                out.append((label, cur))
            label, cur = tok[:-1], []
            continue
        if tok.startswith("."):
            continue
        op, _, rest = tok.partition(" ")
        cur.append((op, rest))
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
            out.append((label, cur))
            label, cur = None, []
    if cur:
        out.append((label, cur))
    return out


def mix_of(block):
    """class counts, opcode histogram and private-segment accesses of one block"""
    count = collections.Counter({c: 0 for c in CLASSES})
    ops = collections.Counter()
    private = 0
    for op, rest in block:
        count[classify(op)] += 1
        ops[op] += 1
        private += is_private(op, rest)
    return {"count": dict(count), "ops": dict(ops), "private": private, "total": len(block),
            "per_mfma": len(block) / count["mfma"] if count["mfma"] else None}


def assembly(csrc, unit):
    """the unit compiled device-only to gfx950 assembly with the Makefile's flags"""
    hipcc, flags = make_flags(csrc)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", os.path.basename(unit), "-o", out], cwd=csrc, check=True,
                       stderr=subprocess.DEVNULL)
        return open(out).read()


def report(asm, kernel):
    """{"kernel": demangled name, "info": {VGPR, AGPR, LDS, scratch}, "blocks": [{"label", "count", "ops", ...}]}: the blocks of the one
    kernel whose name (without namespace, template and parameter lists) is `kernel` that hold MFMAs, in program order"""
    kernels = kernels_of(asm)
    dem = demangle(sorted(kernels))
    base = lambda d: re.sub(r"[<(].*", "", re.sub(r"^\w+\s+", "", d.strip())).split("::")[-1]
    hits = [n for n in kernels if base(dem[n]) == kernel or n == kernel]
    if len(hits) != 1:
        raise SystemExit("%d kernels named %s (have: %s)" % (len(hits), kernel, ", ".join(sorted({base(d) for d in dem.values()}))))
    _, code, info = kernels[hits[0]]
    blocks = []
    for k, (label, block) in enumerate(blocks_of(code)):
        m = mix_of(block)
        if m["count"]["mfma"]:
            m["label"] = label or "(behind a branch, block %d)" % k
            blocks.append(m)
    return {"kernel": dem[hits[0]], "info": {k: int(v) for k, v in info.items()}, "blocks": blocks}


def hottest(rep):
    """the block with the most MFMAs"""
    return max(rep["blocks"], key=lambda b: b["count"]["mfma"])


def table(rep, markdown=False):
    head = ["block"] + [TITLES[c] for c in CLASSES] + ["private", "total", "per MFMA"]
    rows = [[b["label"]] + [str(b["count"][c]) for c in CLASSES] + [str(b["private"]), str(b["total"]), "%.2f" % b["per_mfma"]]
            for b in rep["blocks"]]
    if markdown:
        return "\n".join(["| " + " | ".join(head) + " |", "|" + "---|" * len(head)] + ["| " + " | ".join(r) + " |" for r in rows])
    width = [max(len(r[k]) for r in [head] + rows) for k in range(len(head))]
    return "\n".join("  ".join(c.ljust(w) if k == 0 else c.rjust(w) for k, (c, w) in enumerate(zip(r, width))) for r in [head] + rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("unit", help="a *.hip file of the source directory")
    ap.add_argument("kernel", help="kernel name without namespace and parameter list")
    ap.add_argument("--csrc", default=os.path.join(ROOT, "snprelate_amd", "csrc"), help="source directory (default: this tree's)")
    ap.add_argument("--asm", help="an assembly file of the unit made earlier (nothing is compiled)")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--ops", action="store_true", help="the opcode histogram of the block with the most MFMAs as well")
    a = ap.parse_args()
    rep = report(open(a.asm).read() if a.asm else assembly(a.csrc, a.unit), a.kernel)
    info = rep["info"]
    print("%s%s: %s VGPR, %s AGPR, %s bytes of LDS, %s bytes of scratch" % ("`" if a.markdown else "", rep["kernel"].split("(")[0] +
                                                                         ("`" if a.markdown else ""), info.get("VGPR", "?"),
                                                                         info.get("AGPR", "?"), info.get("LDS", "?"), info.get("scratch", "?")))
    if a.markdown:
        print()
    print(table(rep, a.markdown))
    if a.ops:
        hot = hottest(rep)
        print("\nblock %s, by opcode:" % hot["label"])
        for op, n in sorted(hot["ops"].items(), key=lambda t: (-t[1], t[0])):
            print("%6d  %s%s%s" % (n, "`" if a.markdown else "", op, "`" if a.markdown else ""))


if __name__ == "__main__":
    main()
