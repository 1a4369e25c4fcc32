#!/usr/bin/env python3
"""The gfx950 code of every kernel of csrc/, one normalised text file per kernel, so that two source trees compare with `diff -r`:

    python tools/kernel_isa.py --all OUT_NEW                 # every translation unit of snprelate_amd/csrc
    python tools/kernel_isa.py kernels_syrk_uv.hip OUT_NEW   # one (or several) of them
    diff -r OUT_OLD OUT_NEW                                  # OUT_OLD: the same tool, copied into tools/ of another checkout

A translation unit is compiled device-only to assembly with the Makefile's flags plus `--offload-device-only -S`.  A kernel's file
(demangled name, made file-safe) holds its `.amdhsa_*` block (registers, LDS, scratch) and its instruction stream with everything
removed that changes when a kernel only moves to another file: comments, `.file` / `.ident` / section / debug lines, and the function
index k of the local labels `.LBB<k>_<n>`.  `--table` prints VGPR / AGPR / LDS / scratch per kernel as markdown rows.

    python tools/kernel_isa.py --compare OUT_OLD OUT_NEW     # the class of every kernel, from two such directories

identical: the files are equal.  reordered: the `.amdhsa_*` block is equal (registers, LDS, scratch) and the instruction stream has
the same number of every mnemonic -- only order, register numbers and label numbers differ.  differs: anything else.
The tool compares; it does not look for any instruction."""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = (".file", ".ident", ".section", ".text", ".loc", ".cfi_", ".size", ".type", ".globl", ".protected", ".weak", ".hidden", ".set",
        ".addrsig", ".amdgcn_target", ".amdgpu_metadata", ".end_amdgpu_metadata")
INFO = {"NumVgprs": "VGPR", "NumAgprs": "AGPR", "LDSByteSize": "LDS", "ScratchSize": "scratch"}


def make_flags(csrc):
    """HIPCC and CXXFLAGS as csrc/Makefile sets them ($(ARCH) expanded; the environment overrides `?=` as make does)"""
    var = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"(\w+)\s*\?=\s*(.*)", line)
        if m:
            var[m.group(1)] = os.environ.get(m.group(1), m.group(2).strip())
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    return expand(var["HIPCC"]), expand(var["CXXFLAGS"]).split()


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def file_name(dem):
    """`void ns::kernel<2, true>(unsigned int const*, ...)` -> `ns__kernel_2_true_`: without return type and parameter list"""
    s = dem.strip()
    if s.endswith(")"):                            # cut the parameter list: the bracket that matches the last one
        depth = 0
        for k in range(len(s) - 1, -1, -1):
            depth += (s[k] == ")") - (s[k] == "(")
            if depth == 0:
                s = s[:k]
                break
    s = re.sub(r"^(void|int)\s+", "", s)
    return re.sub(r"[^A-Za-z0-9_.-]+", "_", s.replace("::", "__"))


def kernels_of(asm):
    """{mangled name: (amdhsa lines, instruction lines, info)} of one assembly text"""
    lines = asm.split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res, cur, in_hsa, last = {}, None, None, None
    for raw in lines:
        m = re.match(r";\s*(\w+):\s*(\d+)", raw)
        if m and m.group(1) in INFO and last:
            res[last][2].setdefault(INFO[m.group(1)], m.group(2))
        line = raw.split(";", 1)[0].rstrip()
        tok = line.strip()
        if not tok:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", tok)
        if m:
            in_hsa = m.group(1)
            res.setdefault(in_hsa, ([], [], {}))
        if in_hsa:
            res[in_hsa][0].append(tok)
            if tok == ".end_amdhsa_kernel":
                in_hsa = None
            continue
        m = re.match(r"([A-Za-z_$][\w$.]*):$", tok)
        if m and m.group(1) in names:
            cur = last = m.group(1)
            res.setdefault(cur, ([], [], {}))
            tmp = {}
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", tok):
            cur = None
            continue
        if tok.startswith(DROP):
            continue
        tok = re.sub(r"\.(LBB|LJTI)\d+_(\d+)", r".\1_\2", tok)
        tok = re.sub(r"\.Ltmp\d+", lambda t: tmp.setdefault(t.group(0), ".Ltmp_%d" % len(tmp)), tok)
        res[cur][1].append(tok if tok.endswith(":") else "\t" + re.sub(r"\s+", " ", tok))
    return res


def compile_unit(args):
    hipcc, flags, src = args
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", os.path.basename(src), "-o", out], cwd=os.path.dirname(src),
                       check=True, stderr=subprocess.DEVNULL)
        return src, kernels_of(open(out).read())


def split_kernel_file(path):
    """(amdhsa lines, mnemonic histogram) of one kernel file written by main()"""
    lines = open(path).read().split("\n")[1:]
    end = lines.index(".end_amdhsa_kernel") + 1 if ".end_amdhsa_kernel" in lines else 0
    code = [ln.split() for ln in lines[end:] if ln.startswith("\t") and not ln.lstrip().startswith(".")]
    return lines[:end], collections.Counter(t[0] for t in code if t)


def compare(old, new):
    """print `class<TAB>kernel` for every kernel file of the two directories; returns the number of kernels that differ"""
    names = lambda d: {f for f in os.listdir(d) if f.endswith(".txt")}
    a, b = names(old), names(new)
    count = collections.Counter()
    for f in sorted(a | b):
        if f not in a or f not in b:
            cls = "only in " + (old if f in a else new)
        elif open(os.path.join(old, f)).read() == open(os.path.join(new, f)).read():
            cls = "identical"
        else:
            cls = "reordered" if split_kernel_file(os.path.join(old, f)) == split_kernel_file(os.path.join(new, f)) else "differs"
        count[cls] += 1
        print("%s\t%s" % (cls, f[:-4]))
    print(", ".join("%d %s" % (n, c) for c, n in sorted(count.items())), file=sys.stderr)
    return sum(n for c, n in count.items() if c not in ("identical", "reordered"))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], epilog="or: --compare OLD_DIR NEW_DIR")
    ap.add_argument("--all", action="store_true", help="every *.hip of the source directory")
    ap.add_argument("--csrc", default=os.path.join(ROOT, "snprelate_amd", "csrc"), help="source directory (default: this tree's)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--table", action="store_true", help="print `| kernel | file | VGPR | AGPR | LDS | scratch |` rows")
    ap.add_argument("paths", nargs="+", metavar="UNIT... OUTDIR")
    a = ap.parse_args()
    outdir, units = a.paths[-1], a.paths[:-1]
    if a.all == bool(units):
        ap.error("give either --all or the translation units, then the output directory")
    srcs = sorted(glob.glob(os.path.join(a.csrc, "*.hip"))) if a.all else [os.path.join(a.csrc, os.path.basename(u)) for u in units]
    hipcc, flags = make_flags(a.csrc)
    os.makedirs(outdir, exist_ok=True)
    rows = []
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for src, kernels in pool.map(compile_unit, [(hipcc, flags, s) for s in srcs]):
            dem = demangle(sorted(kernels))
            for name, (hsa, code, info) in sorted(kernels.items()):
                path = os.path.join(outdir, file_name(dem[name]) + ".txt")
                if os.path.exists(path) and path in [r[0] for r in rows]:
                    sys.exit("two kernels map to %s" % path)
                with open(path, "w") as f:
                    f.write("\n".join(["# " + dem[name]] + hsa + code) + "\n")
                rows.append((path, "| `%s` | `%s` | %s |" % (os.path.basename(path)[:-4], os.path.basename(src),
                                                           " | ".join(info.get(k, "?") for k in INFO.values()))))
    if a.table:
        print("\n".join(r[1] for r in sorted(rows)))
    print("%d kernels of %d translation units -> %s" % (len(rows), len(srcs), outdir), file=sys.stderr)


if __name__ == "__main__":
    main()
