"""An independent restatement of the reference's VCF parser (gnrParseVCF4, src/ConvToGDS.cpp:667-997, with CReadLine::GetCell,
getInt32 and getFloat) in plain Python on str: no numpy in the parsing, no code shared with snprelate_amd/vcf.py.  It reads a whole
file's text line by line and cell by cell, as slowly as the reference does, and is what the GPU rows are compared with."""
import math
import re
import struct

_INT = re.compile(r"[ \t\n\v\f\r]*([+-]?[0-9]+)")
_FLT = re.compile(r"[ \t\n\v\f\r]*([+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)")
_WS = " \t\n\v\f\r"


class RefError(Exception):
    """what the reference raises: its message, the file's 1-based line and the column counter at the throw (0: none)"""

    def __init__(self, message, line=0, column=0):
        Exception.__init__(self, message)
        self.message, self.line, self.column = message, line, column


def _short(s):
    return s if len(s) <= 16 else s[:16] + "..."


def cell_code(cell, num_allele, ref_index=0):
    """dosage code of one sample cell after GetCell: the loop of lines 917-986"""
    gt = cell.split(":", 1)[0].split("\0", 1)[0].lstrip(_WS)
    dosage = 0
    while gt:
        m = _INT.match(gt)
        if m is None:
            if gt[0] != ".":
                raise RefError('Invalid integer conversion "%s".' % _short(gt))
            val, rest = -1, gt
        else:
            v = max(-2 ** 63, min(2 ** 63 - 1, int(m.group(1))))
            val = struct.unpack("<i", struct.pack("<q", v)[:4])[0]                # the long goes into an int
            if val < 0:
                raise RefError('Genotype code should be non-negative "%s".' % _short(gt))
            if val >= num_allele:
                raise RefError('Genotype code is out of range "%s".' % _short(gt))
            rest = gt[m.end():]
        cut = re.search(r"[|/]", rest)
        gt = rest[cut.end():] if cut else ""
        if dosage >= 0:
            dosage = -1 if val < 0 else dosage + (1 if val == ref_index else 0)
    return 3 if dosage < 0 else min(dosage, 2)


class _Line:
    """GetCell on one line, tabs only"""

    def __init__(self, text):
        self.rest, self.column = text, 0

    def cell(self, last=False):
        self.column += 1
        if self.rest == "":               # at the end of the line, behind the last cell or behind a trailing tab
            raise RefError("fewer columns than what expected.", 0, self.column)
        head, tab, self.rest = self.rest.partition("\t")
        if last and tab:
            raise RefError("more columns than what expected.", 0, self.column)
        if len(head) > 1 and head[0] == head[-1] and head[0] in "\"'":
            head = head[1:-1]
        return head


def line_codes(cells_text, n_samp, num_allele, ref_index=0):
    """codes of the n_samp sample cells of a line (the text from its first sample cell); RefError.column is counted from 9"""
    ln = _Line(cells_text)
    ln.column = 9
    out = []
    for j in range(n_samp):
        try:
            c = ln.cell(last=(j == n_samp - 1))
            out.append(cell_code(c, num_allele, ref_index))
        except RefError as e:
            raise RefError(e.message, 0, ln.column)
    return out


def pack_row(codes):
    """2-bit codes, four per byte, LSB first, the unused codes of the last byte 3"""
    c = list(codes) + [3] * (-len(codes) % 4)
    return bytes(c[i] | c[i + 1] << 2 | c[i + 2] << 4 | c[i + 3] << 6 for i in range(0, len(c), 4))


def _int32(s):
    p = s.lstrip(_WS)
    m = _INT.match(p)
    if m is None:
        if p[:1] != ".":
            raise RefError('Invalid integer conversion "%s".' % _short(p))
        return -2 ** 31
    if not -2 ** 31 <= int(m.group(1)) <= 2 ** 31 - 1:
        raise RefError('Invalid integer conversion "%s".' % _short(p))
    tail = p[m.end():].lstrip(_WS)
    if tail:
        raise RefError('Invalid integer conversion "%s".' % _short(tail))
    return int(m.group(1))


def _float32(s):
    p = s.lstrip(_WS)
    m = _FLT.match(p)
    if m is None:
        if p[:1] != ".":
            raise RefError('Invalid float conversion "%s".' % _short(p))
        return math.nan
    tail = p[m.end():].lstrip(_WS)
    if tail:
        raise RefError('Invalid float conversion "%s".' % _short(tail))
    return struct.unpack("<f", struct.pack("<f", float(m.group(1))))[0]


def parse_vcf(text, method="biallelic.only", ref_allele=None, prefixes=("chr",), first_id=1, first_line=0):
    """text: a whole VCF file (str).  dict of sample_id, snp_id, chrom, pos, rs, allele, qual, filter (lists), geno (list of code
    lists), next_id, lines: the nodes snpgdsVCF2GDS writes, and the counters a following file starts from."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [s[:-1] if s.endswith("\r") else s for s in lines]
    k = 0
    while k < len(lines) and not lines[k].startswith("#CHROM"):
        k += 1
    if k >= len(lines):
        raise RefError("Error VCF format: invalid sample id!")
    samp = lines[k].split("\t")[9:]
    n = len(samp)
    out = dict(sample_id=samp, snp_id=[], chrom=[], pos=[], rs=[], allele=[], qual=[], filter=[], geno=[])
    vid, gidx = first_id, first_line
    for no in range(k + 1, len(lines)):
        ln = _Line(lines[no])
        try:
            gidx += 1
            chrom, pos, rs, ref, alt = [ln.cell() for _ in range(5)]
            if method == "biallelic.only" and not (len(ref) == 1 and ref in "ACGTacgt" and len(alt) == 1 and alt in "ACGTacgt"):
                for i in range(n + 4, 0, -1):
                    ln.cell(last=(i <= 1))
                continue
            num_allele = 1
            if alt != ".":
                num_allele += len([a for a in alt.split(",")]) - (1 if alt.endswith(",") or alt == "" else 0)
            for pre in prefixes:
                if chrom[:len(pre)].upper() == pre.upper():
                    chrom = chrom[len(pre):]
                    break
            position = _int32(pos)
            ref_index, allele = 0, ref + "/" + alt
            if ref_allele is not None:
                if gidx - 1 >= len(ref_allele):
                    raise RefError("'ref.allele' has fewer alleles than what expected.", 0, -1)
                want = ref_allele[gidx - 1]
                if want is not None:
                    al = [ref] + [a for a in alt.split(",")]
                    if al[-1] == "" and len(al) > 1:
                        al.pop()
                    if want in al:
                        ref_index = al.index(want)
                        allele = want + "/" + ",".join(al[:ref_index] + al[ref_index + 1:])
                    else:
                        ref_index, allele = -1, want + "/" + ref + "," + alt
            qual = _float32(ln.cell())
            filt = ln.cell()
            ln.cell()
            ln.cell()
            codes = []
            for j in range(n):
                codes.append(cell_code(ln.cell(last=(j == n - 1)), num_allele, ref_index))
        except RefError as e:
            raise RefError(e.message, no + 1, 0 if e.column == -1 else ln.column)
        out["snp_id"].append(vid)
        vid += 1
        out["chrom"].append(chrom)
        out["pos"].append(position)
        out["rs"].append("" if rs == "." else rs)
        out["allele"].append(allele)
        out["qual"].append(qual)
        out["filter"].append("" if filt == "." else filt)
        out["geno"].append(codes)
    out["next_id"], out["lines"] = vid, gidx
    return out
