"""PLINK text PED/MAP as a genotype source: what ``snpgdsPED2GDS`` + ``snpgdsOpen`` give in the reference, without the GDS file in
between.

The division of work follows the text.  A .ped line is six short columns and then two allele tokens per SNP, so

* the host reads the MAP file and orders its SNPs as R/Conversion.R:164-170 does (:func:`read_map`), reads the .ped file (plain or
  ``.gz``) in chunks of whole lines into page-locked buffers, finds the lines and reads the six leading columns of each with
  ``textio.Cells`` -- the restatement of ``CReadLine::GetCell`` (src/ConvToGDS.cpp:123-179) splitting by space and tab;
* the device turns the rest of every line into allele tokens (``snpgpu_ped_tokens``), counts them per SNP
  (``snpgpu_ped_census``) and, once the host has picked every SNP's reference allele as src/ConvToGDS.cpp:1238-1270 does, codes
  them into 2-bit sample rows (``snpgpu_ped_codes``) -- two sweeps over the text, as the reference reads the file twice; a file
  of one chunk stays on the device between them;
* a line the kernel flags (an allele of several bytes such as an indel, a quoted token, an empty token, a wrong number of
  tokens) is read again here by :func:`host_tokens`, which follows the reference's loop character for character: its tokens
  join the census through per-SNP dictionaries and its row is patched, or the reference's message is raised with ``FILE:``,
  ``LINE:``, ``COLUMN:``.

There is no CPU fallback for the tokens: without a device :meth:`PedReader.run` fails with ``SnpGpuError``.

Two deviations from the reference, both stated in DESIGN section 26.  The MAP order compares chromosome labels as bytes where
R's ``order`` collates by locale.  And ``snp_allele`` is permuted by the MAP order like the genotypes, rs ids and positions:
gnrParsePED appends it in file order (src/ConvToGDS.cpp:1272-1276 against :1353-1355), so that with an unsorted MAP the
reference's alleles belong to other SNPs; for a sorted MAP nothing differs.
"""
import functools

import numpy as np

from . import textio
from .gds import pack_2bit_rows
from .textio import Cells, VcfFormatError, c_string, last_cell, open_binary, stage_bytes


# ---- the MAP file ------------------------------------------------------------------------------------------------------------------
def _number(x):
    try:
        return float(x)
    except ValueError:
        return None


def map_order(chrom, pos):
    """ii of snpgdsPED2GDS (R/Conversion.R:164-170), 0-based, and the chromosome column after `map$V1[is.na(map$V1)] <- 0`, for
    the MAP columns V1 (text) and V4 (int).  "NA" is NA.  A numeric V1: order(V1, V4), the column as int32; else
    order(as.integer(V1), V1, V4) with the labels compared as bytes (R collates by locale: the one deviation of the order), the
    column as text.  NA sorts last; the sort is stable."""
    n = len(chrom)
    vals = [None if c == "NA" else _number(c) for c in chrom]
    pos = np.asarray(pos, np.int64)
    if all(c == "NA" or v is not None for c, v in zip(chrom, vals)):
        na = np.array([v is None for v in vals], bool)
        val = np.array([0.0 if v is None else v for v in vals], np.float64)
        ii = np.lexsort((pos, val, na)) if n else np.zeros(0, np.int64)
        return ii, np.where(na, 0, val).astype(np.int32)[ii]
    code = [None if v is None or v != v or abs(v) >= 2.0 ** 31 else int(v) for v in vals]
    key = [(code[i] is None, 0 if code[i] is None else code[i], chrom[i] == "NA", chrom[i].encode("latin1"), int(pos[i])) for i in range(n)]
    ii = np.array(sorted(range(n), key=key.__getitem__), np.int64)
    return ii, np.array(["0" if chrom[i] == "NA" else chrom[i] for i in ii], dtype=str)


def read_map(map_fn):
    """the MAP file as read.table reads it (whitespace-separated, at least four columns; empty lines skipped) in the order ii:
    dict(ii, snp_chromosome, snp_rs_id, snp_position)"""
    chrom, rs, pos = [], [], []
    with open_binary(map_fn) as f:
        for k, raw in enumerate(f):
            t = raw.decode("latin1").split()
            if not t:
                continue
            if len(t) < 4:
                raise ValueError("'%s', line %d: a MAP file has four columns (chromosome, id, genetic distance, position)" % (map_fn, k + 1))
            try:
                pos.append(int(t[3]))
            except ValueError:
                raise ValueError("'%s', line %d: the position \"%s\" is not an integer" % (map_fn, k + 1, t[3]))
            chrom.append(t[0])
            rs.append(t[1])
    if not chrom:
        raise ValueError("'%s' has no SNP" % map_fn)
    ii, col = map_order(chrom, pos)
    return dict(ii=ii, snp_chromosome=col, snp_rs_id=np.array(rs, dtype=str)[ii], snp_position=np.array(pos, np.int64)[ii].astype(np.int32))


# ---- a line on the host --------------------------------------------------------------------------------------------------------------
def host_head(line):
    """the six leading cells of a .ped line and the offset of the seventh, as GetCell reads them"""
    rl = Cells(line, space=True)
    return [rl.get(False) for _ in range(6)], rl.p


def host_tokens(line, n_snp):
    """the 2 n_snp allele cells of a whole .ped line (bytes without the line end) as the reference reads them, or VcfFormatError
    with the column and cell it would report"""
    rl = Cells(c_string(line), space=True)
    for _ in range(6):
        rl.get(False)
    return [rl.get(k >= 2 * n_snp - 1) for k in range(2 * n_snp)]


def pick_alleles(counts):
    """(ref, alt) of one SNP from {cell: count} as src/ConvToGDS.cpp:1238-1270: the largest count, ties to the smaller string; the
    others ascending, comma-separated; b"0" for an empty side"""
    nmax, smax = 0, b"0"
    keys = sorted(counts)
    for k in keys:
        if nmax < counts[k]:
            nmax, smax = counts[k], k
    alt = b",".join(k for k in keys if k != smax)
    return smax, (alt if alt else b"0")


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
class PedReader:
    """The two sweeps over one .ped file.  After :meth:`run`: sample_id, sample_annot columns (family, father, mother, sex,
    phenotype), snp_allele in FILE order and `rows`, a torch uint8 tensor [n_samp][ceil(n_snp / 4)] of SNPGPU_GENO_PACKED2 sample
    rows in FILE order of the SNPs on `device`.  flagged_lines counts what the kernel left to the host, windows the text windows
    of one sweep."""

    def __init__(self, ped_fn, n_snp, device=0, chunk_bytes=None):
        self.path, self.n_snp, self.device = str(ped_fn), int(n_snp), int(device)
        self.chunk_bytes = int(chunk_bytes) if chunk_bytes else stage_bytes()
        self.flagged_lines, self.windows = 0, 0
        self._tail = b""                                   # the last cell of the line in front of the current chunk

    def _raise(self, e, file_line):
        raise ValueError("%s\nFILE: %s\nLINE: %d, COLUMN: %d, %s\n" % (e.message, self.path, file_line, e.column, e.cell.decode("latin1")))

    def _chunks(self, heads):
        """(device text, n_bytes, cell_begin, line_end, first file line, pending error) per chunk of whole lines; with `heads` the
        six leading cells of every line are appended to it.  A line whose leading columns fail ends its chunk: the lines in
        front of it are still yielded, so that an earlier line's error is raised first."""
        import torch
        from . import _lib
        size = self.chunk_bytes
        pinned = [_lib.PinnedBuffer((size,)) for _ in range(2)]
        dev = torch.empty(size, dtype=torch.uint8, device="cuda:%d" % self.device)
        lines = functools.partial(textio.split_lines, strip_cr=True)
        file_line = 0
        try:
            with open_binary(self.path) as f:
                for buf, n, _final, begin, end in textio.chunks(f, [p.array for p in pinned], lines, self.path, "SNPGPU_TEXT_STAGE_BYTES"):
                    cell_begin, cells, err = textio.leading_columns(buf, begin, end, host_head, self._tail)
                    m = len(cell_begin)
                    if heads is not None:
                        heads.extend(cells)
                    if m:
                        dev[:n].copy_(torch.from_numpy(buf[:n]))
                        torch.cuda.synchronize(self.device)
                        yield dev, n, cell_begin, end[:m], file_line, buf
                    if err is not None:
                        self._raise(err, file_line + m + 1)
                    file_line += m
                    self._tail = last_cell(bytes(buf[int(begin[-1]):int(end[-1])]))
        finally:
            for p in pinned:
                p.free()

    def run(self):
        import torch
        from . import _lib
        from .text import device_visible
        if not device_visible():
            raise _lib.SnpGpuError("snpgdsOpenPED: no HIP device (the PED tokeniser has no CPU fallback)")
        M, rb, dv = self.n_snp, (self.n_snp + 3) // 4, "cuda:%d" % self.device
        table = torch.zeros((M, _lib.PED_ALLELES), dtype=torch.int32, device=dv)
        extra = {}                                         # SNP -> {cell: count} of the lines the host settled
        heads, n_lines, kept = [], 0, None
        tokens = None

        def tokenise(text, n, cb, le):
            nonlocal tokens
            if tokens is None or tokens.numel() < len(cb) * 2 * M:
                tokens = torch.empty(len(cb) * 2 * M, dtype=torch.uint8, device=dv)
            return _lib.ped_tokens(int(text.data_ptr()), n, cb, le, M, int(tokens.data_ptr()), device=self.device)[0]

        def settle(buf, cb, le, i, first_line):
            # the whole line again, from its first byte: the head is short, and the reference's column numbers count from it
            b = int(cb[i])
            while b > 0 and buf[b - 1] != 10:
                b -= 1
            try:
                return host_tokens(bytes(buf[b:int(le[i])]), M)
            except VcfFormatError as err:
                self._raise(err, first_line + i + 1)

        # ---- sweep 1: the census --------------------------------------------------------------------------------------------------
        for text, n, cb, le, first_line, buf in self._chunks(heads):
            flags = tokenise(text, n, cb, le)
            for i in np.flatnonzero(flags):
                for k, cell in enumerate(settle(buf, cb, le, int(i), first_line)):
                    if cell != b"0":
                        d = extra.setdefault(k >> 1, {})
                        d[cell] = d.get(cell, 0) + 1
            self.flagged_lines += int(np.count_nonzero(flags))
            _lib.ped_census(int(tokens.data_ptr()), flags, M, int(table.data_ptr()), device=self.device)
            n_lines += len(cb)
            self.windows += 1
            # a file of one chunk: its tokens stay on the device for the second sweep (the page-locked buffer does not)
            kept = (cb, le, first_line, buf[:n].copy() if flags.any() else None, flags) if self.windows == 1 and n < self.chunk_bytes else None
        if n_lines == 0:
            raise ValueError("'%s' has no sample" % self.path)

        # ---- the reference alleles (src/ConvToGDS.cpp:1238-1270) ----------------------------------------------------------------------
        cnt = table.cpu().numpy().view(np.uint32)
        ref = (np.argmax(cnt, 1) + 0x21).astype(np.uint8)                        # the first maximum: ties to the smaller byte
        ref[cnt.max(1) == 0] = 0x30
        n_alleles = np.count_nonzero(cnt, 1)
        allele, ref_cells = [None] * M, [None] * M
        for j in range(M):
            if j in extra or n_alleles[j] > 2:
                d = {bytes([0x21 + int(c)]): int(cnt[j, c]) for c in np.flatnonzero(cnt[j])}
                for k, v in extra.get(j, {}).items():
                    d[k] = d.get(k, 0) + v
                r, a = pick_alleles(d)
                ref[j] = r[0] if len(r) == 1 else 0
            else:
                r = bytes([ref[j]])
                a = b"0" if n_alleles[j] < 2 else bytes([0x21 + int(c) for c in np.flatnonzero(cnt[j]) if 0x21 + c != ref[j]])
            allele[j], ref_cells[j] = (r + b"/" + a).decode("latin1"), r

        # ---- sweep 2: the codes -----------------------------------------------------------------------------------------------------
        rows = torch.empty((n_lines, rb), dtype=torch.uint8, device=dv)
        done = 0

        def code(cb, le, first_line, buf, flags):
            nonlocal done
            m = len(cb)
            _lib.ped_codes(int(tokens.data_ptr()), m, M, ref, int(rows[done:done + m].data_ptr()), device=self.device)
            for i in np.flatnonzero(flags):
                cells = settle(buf, cb, le, int(i), first_line)
                g = np.empty(M, np.uint8)
                for j in range(M):
                    t1, t2 = cells[2 * j], cells[2 * j + 1]
                    g[j] = 3 if (t1 == b"0" or t2 == b"0") else (t1 == ref_cells[j]) + (t2 == ref_cells[j])
                rows[done + int(i)].copy_(torch.from_numpy(pack_2bit_rows(g[None, :])[0]))
            done += m

        if kept is not None:
            code(*kept)
        else:
            for text, n, cb, le, first_line, buf in self._chunks(None):
                code(cb, le, first_line, buf, tokenise(text, n, cb, le))
        torch.cuda.synchronize(self.device)

        def col(k, f=lambda v: v):
            return np.array([f(h[k].decode("latin1")) for h in heads], dtype=str)
        self.sample_id = col(1)
        self.sample_annot = dict(family=col(0), father=col(2), mother=col(3), sex=col(4, lambda v: "M" if v == "1" else "F" if v == "2" else v),
                                 phenotype=col(5))
        self.snp_allele = np.array(allele, dtype=str)
        self.rows, self.n_samp = rows, n_lines
        return self
