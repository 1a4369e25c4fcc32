"""VCF text as a genotype source: what ``snpgdsVCF2GDS`` + ``snpgdsOpen`` give in the reference, without the GDS file in between.

The division of work follows the text.  A data line is nine short fixed columns and then one cell per sample; at 100 000 samples
the cells are 0.4 to 1.5 MB of a line and the fixed columns a few dozen bytes.  So

* the host reads the file (plain or ``.gz``) in chunks of whole lines into page-locked buffers, finds the lines and their fixed
  columns (``snpgpu_vcf_index``, C++), and builds the per-variant metadata as ``gnrParseVCF4`` does (src/ConvToGDS.cpp:753-904):
  the ``method`` filter, ``num_allele``, ids, chromosome, position, ``REF/ALT`` with the ``ref.allele`` rewriting, QUAL, FILTER;
* the device reduces the sample cells of the kept lines to SNPGPU_GENO_PACKED2 rows (``snpgpu_vcf_genotypes``), the chunk's own
  bytes being its input;
* a line the kernel flags (an allele position that ``strtol`` would read differently, an allele index out of range, a wrong
  number of cells) is parsed again here by :func:`host_cells`, which follows the reference's loop character for character and
  either yields the row (patched on the device) or raises the reference's message with ``FILE:``, ``LINE:``, ``COLUMN:``.

There is no CPU fallback for the cells: without a device :meth:`VcfReader.blocks` fails with ``SnpGpuError``.
"""
import os
import re

import numpy as np

from .gds import pack_2bit_rows
from . import textio
from .textio import Cells, VcfFormatError, open_binary

NA_INTEGER = -2147483648
_SPACE = b" \t\n\v\f\r"
_FLOAT = re.compile(rb"[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf(?:inity)?|nan)", re.I)
_BIALLELIC = frozenset(b"ACGTacgt"[i:i + 1] for i in range(8))


def _short(p):
    p = p.decode("latin1")
    return p if len(p) <= 16 else p[:16] + "..."


def _skip(s, i=0):
    while i < len(s) and s[i] in _SPACE:
        i += 1
    return i


def _strtol(s, i):
    """strtol(s + i, &end, 10) on bytes: (value as a C long, end); end == i when there is no conversion"""
    j = _skip(s, i)
    neg = False
    if j < len(s) and s[j] in b"+-":
        neg = s[j] == 0x2D
        j += 1
    k = j
    while k < len(s) and 0x30 <= s[k] <= 0x39:
        k += 1
    if k == j:
        return 0, i
    v = int(s[j:k])
    v = -v if neg else v
    return max(-(1 << 63), min((1 << 63) - 1, v)), k


def get_int32(txt):
    """getInt32 (src/ConvToGDS.cpp:467-503) with RaiseError"""
    p = _skip(txt)
    val, end = _strtol(txt, p)
    if end == p:
        if txt[p:p + 1] != b".":
            raise VcfFormatError("Invalid integer conversion \"%s\"." % _short(txt[p:]))
        return NA_INTEGER
    if val < -(1 << 31) or val > (1 << 31) - 1:
        raise VcfFormatError("Invalid integer conversion \"%s\"." % _short(txt[p:]))
    q = _skip(txt, end)
    if q < len(txt):
        raise VcfFormatError("Invalid integer conversion \"%s\"." % _short(txt[q:]))
    return val


def get_float(txt):
    """getFloat (src/ConvToGDS.cpp:506-532) with RaiseError: strtof of the text, NaN for '.'"""
    p = _skip(txt)
    m = _FLOAT.match(txt, p)
    if not m:
        if txt[p:p + 1] != b".":
            raise VcfFormatError("Invalid float conversion \"%s\"." % _short(txt[p:]))
        return np.float32("nan")
    q = _skip(txt, m.end())
    if q < len(txt):
        raise VcfFormatError("Invalid float conversion \"%s\"." % _short(txt[q:]))
    with np.errstate(over="ignore"):
        return np.float32(float(m.group().decode("latin1")))


def gt_code(cell, num_allele, ref_index):
    """the dosage code of one sample cell (src/ConvToGDS.cpp:917-986): 0 / 1 / 2 copies of allele ref_index, 3 = missing"""
    c = cell.find(b":")
    v = cell if c < 0 else cell[:c]
    z = v.find(b"\0")
    if z >= 0:
        v = v[:z]
    p = _skip(v)
    dosage = 0
    while p < len(v):
        val, end = _strtol(v, p)
        if end == p:
            if v[p:p + 1] != b".":
                raise VcfFormatError("Invalid integer conversion \"%s\"." % _short(v[p:]))
            val = -1
        else:
            val = ((val + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)                  # int val = strtol(...)
            if val < 0:
                raise VcfFormatError("Genotype code should be non-negative \"%s\"." % _short(v[p:]))
            if val >= num_allele:
                raise VcfFormatError("Genotype code is out of range \"%s\"." % _short(v[p:]))
            p = end
        while p < len(v) and v[p] not in b"|/":
            p += 1
        if p < len(v):
            p += 1
        if dosage >= 0:
            dosage = (dosage + (val == ref_index)) if val >= 0 else -1
    return 3 if dosage < 0 else min(dosage, 2)


def host_cells(line, n_samp, num_allele, ref_index, pos=0, column=9, cell=b""):
    """the n_samp sample cells of `line` (bytes without the line end) from offset `pos`, as the reference reads them: uint8 codes,
    or VcfFormatError with the column and cell the reference would report"""
    rl = Cells(line, pos, column, cell)
    out = np.empty(n_samp, np.uint8)
    for j in range(n_samp):
        c = rl.get(j >= n_samp - 1)
        try:
            out[j] = gt_code(c, num_allele, ref_index)
        except VcfFormatError as e:
            raise VcfFormatError(e.message, rl.column, rl.cell)
    return out


def allele_text(ref, alt, want):
    """snp.allele and ref_allele_index of one line (src/ConvToGDS.cpp:826-887).  want None: REF/ALT, index 0.  Else the allele
    `want` moves to the front; when the line does not have it, it is put in front of all and the index is -1."""
    if want is None:
        return ref + "/" + alt, 0
    alleles = [ref] + [a for a in alt.split(",")]
    if alleles[-1] == "" and len(alleles) > 1:
        alleles.pop()                                                           # a trailing comma adds no allele (s != p)
    if want in alleles:
        i = alleles.index(want)
        rest = alleles[:i] + alleles[i + 1:]
        return want + "/" + ",".join(rest), i
    return want + "/" + ref + "," + alt, -1


def read_header(f):
    """consume the lines of a binary file object up to and including #CHROM: (sample ids, lines consumed)"""
    n = 0
    while True:
        s = f.readline()
        if not s:
            raise ValueError("Error VCF format: invalid sample id!")
        n += 1
        if s[:6] == b"#CHROM":
            t = s.rstrip(b"\r\n").decode("latin1").split("\t")
            return t[9:], n


def sample_ids(fn):
    with open_binary(fn) as f:
        return read_header(f)[0]


def _chunk_bytes():
    return int(os.environ.get("SNPGPU_VCF_CHUNK_BYTES", 64 << 20))


class VcfReader:
    """One VCF file read once, front to back.  sample_id comes from the header at construction; the per-variant nodes (snp_id,
    snp_rs_id, snp_chromosome, snp_position, snp_allele, snp_annot) grow as :meth:`blocks` (or :meth:`chunks`) goes through the file
    and are numpy arrays after it.  snp_id_start / line_start carry the counters of gnrParseVCF4 from one file to the next: ids
    count kept variants, ref_allele is indexed by all data lines."""

    METHODS = ("biallelic.only", "copy.num.of.ref")

    def __init__(self, vcf_fn, method="biallelic.only", ref_allele=None, ignore_chr_prefix="chr", snp_id_start=1, line_start=0,
                 chunk_bytes=None):
        if method not in self.METHODS:
            raise ValueError("'method' should be one of \"biallelic.only\", \"copy.num.of.ref\"")
        self.path, self.method = str(vcf_fn), method
        self.ref_allele = None if ref_allele is None else list(ref_allele)
        self.prefixes = [ignore_chr_prefix] if isinstance(ignore_chr_prefix, str) else list(ignore_chr_prefix or [])
        self.chunk_bytes = int(chunk_bytes) if chunk_bytes else _chunk_bytes()
        self._f = open_binary(self.path)
        try:
            ids, self._header_lines = read_header(self._f)
        except Exception:
            self._f.close()
            raise
        if len(ids) <= 0:
            self._f.close()
            raise ValueError("No sample in the VCF file!")
        self.sample_id = np.array(ids)
        self.n_samp = len(ids)
        self.next_snp_id, self.lines_seen = int(snp_id_start), int(line_start)
        self._file_line = self._header_lines
        self._nodes = dict(snp_id=[], chrom=[], pos=[], rs=[], allele=[], qual=[], filt=[])
        self.n_snp = 0
        self._done = False

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    # ---- errors as COREARRAY_TRY_END formats them ----
    def _raise(self, e, file_line):
        if e.column > 0:
            raise ValueError("%s\nFILE: %s\nLINE: %d, COLUMN: %d, %s\n" % (e.message, self.path, file_line, e.column,
                                                                         e.cell.decode("latin1")))
        raise ValueError("%s\nFILE: %s\nLINE: %d\n" % (e.message, self.path, file_line))

    # ---- the fixed columns of a chunk's lines ----
    def _scan(self, buf, n_bytes, final):
        """index buf[:n_bytes] and build the metadata of its lines: (kept dict, consumed).  kept: cell_begin, line_end, num_allele,
        ref_index, file_line per kept line."""
        from . import _lib
        col, end, used = _lib.vcf_index(buf, n_bytes, final, line_base=self._file_line)
        n_samp, nodes = self.n_samp, self._nodes
        biallelic = self.method == "biallelic.only"
        kept = dict(cell_begin=[], line_end=[], num_allele=[], ref_index=[], file_line=[])
        for i in range(len(col)):
            c, e = col[i], int(end[i])
            self._file_line += 1
            self.lines_seen += 1
            f = bytes(buf[int(c[0]):int(c[9])]).split(b"\t")[:9]                # only the fixed columns are copied out of the chunk
            f = [x[1:-1] if len(x) > 1 and x[0] == x[-1] and x[0] in b"\"'" else x for x in f]
            ref, alt = f[3], f[4]
            try:
                if biallelic and not (ref in _BIALLELIC and alt in _BIALLELIC):
                    # the reference still walks the line's cells: a wrong number of them is an error on a skipped line too
                    n_tab = int(np.count_nonzero(buf[int(c[9]):e] == 9))
                    if n_tab + 1 != n_samp or int(c[9]) == e or buf[e - 1] == 9:
                        rl = Cells(bytes(buf[int(c[0]):e]), int(c[5]) - int(c[0]), 5, f[4])
                        for k in range(n_samp + 4, 0, -1):
                            rl.get(k <= 1)
                    continue
                # one more allele per comma-separated piece of ALT; a trailing comma adds none (the loop stops at the NUL)
                num_allele = 1 if alt in (b".", b"") else 2 + alt.count(b",") - alt.endswith(b",")
                chrom = f[0].decode("latin1")
                for pre in self.prefixes:
                    if chrom[:len(pre)].upper() == pre.upper():                # StrCaseCmp: chrom starts with the prefix
                        chrom = chrom[len(pre):]
                        break
                try:
                    pos = get_int32(f[1])
                except VcfFormatError as err:
                    raise VcfFormatError(err.message, 5, f[1])
                want = None
                if self.ref_allele is not None:
                    if self.lines_seen - 1 >= len(self.ref_allele):
                        raise VcfFormatError("'ref.allele' has fewer alleles than what expected.")
                    want = self.ref_allele[self.lines_seen - 1]
                allele, ref_index = allele_text(ref.decode("latin1"), alt.decode("latin1"), want)
                try:
                    qual = get_float(f[5])
                except VcfFormatError as err:
                    raise VcfFormatError(err.message, 6, f[5])
            except VcfFormatError as err:
                self._raise(err, self._file_line)
            nodes["snp_id"].append(self.next_snp_id)
            self.next_snp_id += 1
            nodes["chrom"].append(chrom)
            nodes["pos"].append(pos)
            nodes["rs"].append("" if f[2] == b"." else f[2].decode("latin1"))
            nodes["allele"].append(allele)
            nodes["qual"].append(qual)
            nodes["filt"].append("" if f[6] == b"." else f[6].decode("latin1"))
            kept["cell_begin"].append(int(c[9]))
            kept["line_end"].append(e)
            kept["num_allele"].append(num_allele)
            kept["ref_index"].append(ref_index)
            kept["file_line"].append(self._file_line)
        self.n_snp = len(nodes["snp_id"])
        out = {k: np.array(v, np.int32 if k in ("num_allele", "ref_index") else np.int64) for k, v in kept.items()}
        return out, used

    def chunks(self, buffers=None):
        """(buffer, n_bytes, kept) per chunk of whole lines; buffers: two uint8 arrays of one size to read into (page-locked ones
        for the device path), default two numpy arrays of chunk_bytes."""
        if self._done:
            raise ValueError("a VcfReader goes through its file once")
        if buffers is None:
            buffers = [np.empty(self.chunk_bytes, np.uint8) for _ in range(2)]
        try:
            for buf, n, _final, kept in textio.chunks(self._f, buffers, self._scan, self.path, "SNPGPU_VCF_CHUNK_BYTES"):
                yield buf, n, kept
        finally:
            self._done = True
            self.close()
            self._finish()

    def _finish(self):
        d = self._nodes
        self.snp_id = np.array(d["snp_id"], np.int32)
        self.snp_chromosome = np.array(d["chrom"], dtype=str) if d["chrom"] else np.empty(0, dtype="<U1")
        self.snp_position = np.array(d["pos"], np.int32)
        self.snp_rs_id = np.array(d["rs"], dtype=str) if d["rs"] else np.empty(0, dtype="<U1")
        self.snp_allele = np.array(d["allele"], dtype=str) if d["allele"] else np.empty(0, dtype="<U1")
        self.snp_annot = {"qual": np.array(d["qual"], np.float32),
                          "filter": np.array(d["filt"], dtype=str) if d["filt"] else np.empty(0, dtype="<U1")}
        self.n_snp = len(self.snp_id)

    # ---- the device path ----
    def blocks(self, block_snps, device=0):
        """(snp_begin, n_snp, rows) in one pass over the file: rows is a torch uint8 tensor [n_snp][ceil(n_samp / 4)] on `device`,
        SNPGPU_GENO_PACKED2, valid until the next block is asked for; snp_begin counts this file's kept variants from 0.  A block
        holds at most block_snps variants and never spans two chunks of the file.  The calls are synchronous."""
        from . import _lib
        block_snps = int(block_snps)
        if block_snps < 1:
            raise ValueError("block_snps should be positive")
        if _lib.device_count() < 1:
            raise _lib.SnpGpuError("VcfReader.blocks: no HIP device (the VCF genotype parser has no CPU fallback)")
        import torch
        rb = (self.n_samp + 3) // 4
        pinned = [_lib.PinnedBuffer((self.chunk_bytes,)) for _ in range(2)]
        dev = [torch.empty((block_snps, rb), dtype=torch.uint8, device="cuda:%d" % int(device)) for _ in range(2)]
        turn, done = 0, 0
        try:
            for buf, n, kept in self.chunks([p.array for p in pinned]):
                ptr = pinned[0].ptr if buf is pinned[0].array else pinned[1].ptr
                for lo in range(0, len(kept["cell_begin"]), block_snps):
                    sl = slice(lo, min(lo + block_snps, len(kept["cell_begin"])))
                    m = sl.stop - sl.start
                    rows = dev[turn & 1][:m]
                    turn += 1
                    flags, _cells = _lib.vcf_genotypes(ptr, kept["cell_begin"][sl], kept["line_end"][sl], kept["num_allele"][sl],
                                                       kept["ref_index"][sl], self.n_samp, int(rows.data_ptr()), n_bytes=n,
                                                       text_mem=_lib.HOST_PINNED, device=device)
                    for i in np.flatnonzero(flags):
                        k = lo + int(i)
                        line = bytes(buf[int(kept["cell_begin"][k]):int(kept["line_end"][k])])
                        try:
                            codes = host_cells(line, self.n_samp, int(kept["num_allele"][k]), int(kept["ref_index"][k]))
                        except VcfFormatError as err:
                            self._raise(err, int(kept["file_line"][k]))
                        rows[int(i)].copy_(torch.from_numpy(pack_2bit_rows(codes[None, :])[0]))
                    if len(flags) and flags.any():
                        torch.cuda.synchronize(int(device))
                    yield done, m, rows
                    done += m
        finally:
            for p in pinned:
                p.free()
