"""Plain-Python restatements of the reference's text converters, loop for loop: gnrConvGDS2PED and gnrConvGDS2EIGEN
(src/SNPRelate.cpp:685-767, :828-859), gnrParsePED with CReadLine::GetCell (src/ConvToGDS.cpp:123-179, :1175-1361), and the side
files the R wrappers write or read around them (R/Conversion.R:26-124, :132-302, :695-785).  No numpy in the loops, no package
code: the tests compare the package with these."""
import numpy as np


# ---- out -------------------------------------------------------------------------------------------------------------------------
def ped_text(sample_ids, alleles, geno, fmt):
    """gnrConvGDS2PED.  geno: [sample][snp] of 0 / 1 / 2 / 3; fmt 1 "A/G/C/T" (alleles: the snp.allele strings), 2 "A/B", 3 "1/2"."""
    out = []
    for i, sid in enumerate(sample_ids):
        line = "0\t" + str(sid) + "\t0\t0\t0\t-9"
        for j, g in enumerate(geno[i]):
            g = int(g)
            if fmt == 1:
                s = str(alleles[j])
                k = 0
                s1 = s2 = ""
                while k < len(s) and s[k] != "/":
                    s1 += s[k]
                    k += 1
                if k < len(s) and s[k] == "/":
                    k += 1
                while k < len(s) and s[k] != "/":
                    s2 += s[k]
                    k += 1
                if not s1:
                    s1 = "0"
                if not s2:
                    s2 = "0"
                if g == 0:
                    line += "\t" + s2 + " " + s2
                elif g == 1:
                    line += "\t" + s1 + " " + s2
                elif g == 2:
                    line += "\t" + s1 + " " + s1
                else:
                    line += "\t0 0"
            elif fmt == 2:
                line += "\t" + ("B B" if g == 0 else "A B" if g == 1 else "A A" if g == 2 else "0 0")
            else:
                line += "\t" + ("2 2" if g == 0 else "1 2" if g == 1 else "1 1" if g == 2 else "0 0")
        out.append(line + "\n")
    return "".join(out).encode("latin1")


def eigen_text(geno):
    """gnrConvGDS2EIGEN.  geno: [snp][sample]."""
    return "".join("".join(str(int(g)) if g <= 2 else "9" for g in row) + "\n" for row in geno).encode("latin1")


def map_text(chrom, rs, pos):
    """the .map file of snpgdsGDS2PED (R/Conversion.R:98-107)"""
    sub = {"23": "X", "25": "Y", "24": "XY", "26": "MT"}
    return "".join("%s\t%s\t0\t%d\n" % (sub.get(str(c), str(c)), r, p) for c, r, p in zip(chrom, rs, pos))


def snp_text(snp_id, chrom, pos):
    return "".join("%s\t%s\t0\t%d\n" % (i, c, p) for i, c, p in zip(snp_id, chrom, pos))


def ind_text(sample_id, sex):
    return "".join("%s\t%s\tcontrol\n" % (i, s) for i, s in zip(sample_id, sex))


# ---- in --------------------------------------------------------------------------------------------------------------------------
class PedError(ValueError):
    def __init__(self, message, line, column, cell):
        ValueError.__init__(self, message)
        self.message, self.line, self.column, self.cell = message, line, column, cell


class ReadLine:
    """CReadLine with SplitBySpaceTab over the lines of a text (readLines: '\\n' or '\\r\\n' ends a line, a last line needs none)"""

    def __init__(self, text):
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        self.lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
        self.next, self.cur, self.p, self.line_no, self.column_no = 0, None, 0, 0, 0

    def if_end(self):
        return self.next >= len(self.lines)

    def get_cell(self, last_column):
        if self.cur is None:
            if self.if_end():
                raise ValueError("It is the end.")
            self.cur = self.lines[self.next] + b"\0"
            self.next += 1
            self.line_no += 1
            self.p, self.column_no = 0, 0
        s, p = self.cur, self.p
        b = p
        while s[p] != 9 and s[p] != 32 and s[p] != 0:
            p += 1
        e = p
        self.column_no += 1
        if b == e and s[p] == 0:
            raise ValueError("fewer columns than what expected.")
        if last_column:
            while s[p] == 32:
                p += 1
            if s[p] != 0:
                raise ValueError("more columns than what expected.")
            self.cur = None
        else:
            if s[p] == 9:
                p += 1
            elif s[p] == 32:
                while s[p] == 32:
                    p += 1
            self.p = p
        if e > b + 1:
            if (s[b] == 0x22 and s[e - 1] == 0x22) or (s[b] == 0x27 and s[e - 1] == 0x27):
                b, e = b + 1, e - 1
        return s[b:e]


def parse_ped(text, n_snp, ii=None):
    """gnrParsePED over the bytes of a .ped file.  ii: the 0-based SNP order of the MAP file (None: identity).  Returns a dict:
    sample_id, family, father, mother, sex, phenotype (lists of str), allele_file (snp.allele in FILE order, as the reference
    appends it), allele (the same permuted by ii, as the package stores it) and geno [sample][snp] in the order ii.
    Raises PedError with the line, column and cell COREARRAY_TRY_END would report."""
    ii = list(range(n_snp)) if ii is None else [int(x) for x in ii]
    cell = b""
    rl = ReadLine(text)
    try:
        lists = [dict() for _ in range(n_snp)]
        while not rl.if_end():
            for _ in range(6):
                cell = rl.get_cell(False)
            for i in range(2 * n_snp):
                cell = rl.get_cell(i >= 2 * n_snp - 1)
                if cell != b"0":
                    lists[i >> 1][cell] = lists[i >> 1].get(cell, 0) + 1
        ref, alt = [], []
        for i in range(n_snp):
            nmax, smax = 0, b"0"
            for k in sorted(lists[i]):
                if nmax < lists[i][k]:
                    nmax, smax = lists[i][k], k
            ref.append(smax)
            s = b",".join(k for k in sorted(lists[i]) if k != smax)
            alt.append(s if s else b"0")
        allele_file = [(r + b"/" + a).decode("latin1") for r, a in zip(ref, alt)]

        rl = ReadLine(text)
        out = dict(sample_id=[], family=[], father=[], mother=[], sex=[], phenotype=[], geno=[])
        while not rl.if_end():
            for name in ("family", "sample_id", "father", "mother", "sex", "phenotype"):
                cell = rl.get_cell(False)
                v = cell.decode("latin1")
                if name == "sex":
                    v = "M" if v == "1" else "F" if v == "2" else v
                out[name].append(v)
            g = []
            for i in range(n_snp):
                missing, x = False, 0
                cell = rl.get_cell(False)
                if cell != b"0":
                    x += 1 if cell == ref[i] else 0
                else:
                    missing = True
                cell = rl.get_cell(i >= n_snp - 1)
                if cell != b"0":
                    x += 1 if cell == ref[i] else 0
                else:
                    missing = True
                g.append(3 if missing else x)
            out["geno"].append([g[k] for k in ii])
    except ValueError as e:
        if isinstance(e, PedError):
            raise
        raise PedError(str(e), rl.line_no, rl.column_no, cell)
    out["allele_file"] = allele_file
    out["allele"] = [allele_file[k] for k in ii]
    out["geno"] = np.array(out["geno"], np.uint8).reshape(len(out["sample_id"]), n_snp)
    return out


def map_order(chrom, pos):
    """ii of snpgdsPED2GDS (R/Conversion.R:164-170) for the MAP columns V1 (str tokens) and V4 (int), 0-based, and the
    chromosome column after `map$V1[is.na(map$V1)] <- 0`.  "NA" is NA.  Numeric column: order(V1, V4); else
    order(as.integer(V1), V1, V4) with the labels compared as bytes.  NA sorts last, ties keep the file's order."""
    def num(x):
        try:
            return float(x)
        except ValueError:
            return None
    vals = [None if c == "NA" else num(c) for c in chrom]
    numeric = all(c == "NA" or v is not None for c, v in zip(chrom, vals))
    n = len(chrom)
    if numeric:
        key = [(vals[i] is None, 0.0 if vals[i] is None else vals[i], pos[i]) for i in range(n)]
        ii = sorted(range(n), key=lambda i: key[i])
        col = [0 if vals[i] is None else (int(vals[i]) if vals[i] == int(vals[i]) else vals[i]) for i in ii]
        return ii, col
    code = [None if v is None else int(v) for v in vals]
    key = [(code[i] is None, 0 if code[i] is None else code[i], chrom[i] == "NA", chrom[i].encode("latin1"), pos[i]) for i in range(n)]
    ii = sorted(range(n), key=lambda i: key[i])
    return ii, ["0" if chrom[i] == "NA" else chrom[i] for i in ii]
