"""PLINK text PED/MAP as a genotype source: what ``snpgdsPED2GDS`` + ``snpgdsOpen`` give in the reference, without the GDS file in
between.

The division of work follows the text.  A .ped line is six short columns and then two allele tokens per SNP, so

* the host reads the MAP file and orders its SNPs as R/Conversion.R:164-170 does (:func:`read_map`), reads the .ped file (plain or
  ``.gz``) in chunks of whole lines into page-locked buffers, finds the lines and reads the six leading columns of each with
  ``vcf._Cells`` -- the restatement of ``CReadLine::GetCell`` (src/ConvToGDS.cpp:123-179) splitting by space and tab;
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
import os

import numpy as np

from .gds import pack_2bit_rows
from .vcf import VcfFormatError, _Cells, open_binary

_HEAD = 1024           # bytes of a line looked at for its six leading columns before the whole line is taken


def stage_bytes():
    return max(1, int(os.environ.get("SNPGPU_TEXT_STAGE_BYTES", 256 << 20)))


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
def _c_string(line):
    z = line.find(b"\0")
    return line if z < 0 else line[:z]


def host_head(line):
    """the six leading cells of a .ped line and the offset of the seventh, as GetCell reads them"""
    rl = _Cells(line, space=True)
    return [rl.get(False) for _ in range(6)], rl.p


def host_tokens(line, n_snp):
    """the 2 n_snp allele cells of a whole .ped line (bytes without the line end) as the reference reads them, or VcfFormatError
    with the column and cell it would report"""
    rl = _Cells(_c_string(line), space=True)
    for _ in range(6):
        rl.get(False)
    return [rl.get(k >= 2 * n_snp - 1) for k in range(2 * n_snp)]


def last_cell(line):
    """the last cell of a line that was read without an error: what the reference's `cell` variable still holds when the first
    cell of the next line fails"""
    s = _c_string(line).rstrip(b" ")
    c = s[max(s.rfind(b"\t"), s.rfind(b" ")) + 1:]
    return c[1:-1] if len(c) > 1 and c[0] == c[-1] and c[0] in b"\"'" else c


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

    def _lines(self, buf, n, final):
        """the whole lines of buf[:n]: (begin, end) arrays without the line ends, and the bytes consumed"""
        nl = np.flatnonzero(buf[:n] == 10)
        begin = np.concatenate(([0], nl + 1)).astype(np.int64)
        end = nl.astype(np.int64)
        used = int(nl[-1]) + 1 if len(nl) else 0
        if final and used < n:
            end = np.concatenate((end, [n]))
            used = n
        else:
            begin = begin[:len(end)]
        cr = (end > begin) & (buf[np.maximum(end - 1, 0)] == 13)
        return begin, end - cr, used

    @staticmethod
    def _head(buf, b, e):
        """the six leading cells of the line buf[b:e] and the offset of the seventh: from the line's first _HEAD bytes when they
        hold them, else from the whole line"""
        head = bytes(buf[b:min(e, b + _HEAD)])
        if e - b > _HEAD or b"\0" in head:
            if b"\0" not in head:
                try:
                    cells, p = host_head(head)
                    if p < len(head):
                        return cells, p
                except VcfFormatError:
                    pass
            head = _c_string(bytes(buf[b:e]))
        return host_head(head)

    def _chunks(self, heads):
        """(device text, n_bytes, cell_begin, line_end, first file line, pending error) per chunk of whole lines; with `heads` the
        six leading cells of every line are appended to it.  A line whose leading columns fail ends its chunk: the lines in
        front of it are still yielded, so that an earlier line's error is raised first."""
        import torch
        from . import _lib
        size = self.chunk_bytes
        pinned = [_lib.PinnedBuffer((size,)) for _ in range(2)]
        dev = torch.empty(size, dtype=torch.uint8, device="cuda:%d" % self.device)
        turn, left, file_line = 0, 0, 0
        try:
            with open_binary(self.path) as f:
                while True:
                    buf = pinned[turn].array
                    n = left
                    while n < size:
                        got = f.readinto(memoryview(buf)[n:size])
                        if not got:
                            break
                        n += got
                    final = n < size
                    if n == 0:
                        break
                    begin, end, used = self._lines(buf, n, final)
                    if used == 0:
                        raise ValueError("'%s': a line longer than the %d bytes of a chunk (SNPGPU_TEXT_STAGE_BYTES)" % (self.path, size))
                    cell_begin, pending = np.empty(len(begin), np.int64), None
                    for i in range(len(begin)):
                        b, e = int(begin[i]), int(end[i])
                        try:
                            cells, p = self._head(buf, b, e)
                        except VcfFormatError as err:
                            if err.column == 1:            # no cell of this line was read: `cell` is the line before's last one
                                err.cell = last_cell(bytes(buf[int(begin[i - 1]):int(end[i - 1])])) if i else self._tail
                            pending = (err, file_line + i + 1)
                            begin, end, cell_begin = begin[:i], end[:i], cell_begin[:i]
                            break
                        cell_begin[i] = b + p
                        if heads is not None:
                            heads.append(cells)
                    if len(begin):
                        dev[:n].copy_(torch.from_numpy(buf[:n]))
                        torch.cuda.synchronize(self.device)
                        yield dev, n, cell_begin, end, file_line, buf
                    if pending is not None:
                        self._raise(*pending)
                    file_line += len(begin)
                    self._tail = last_cell(bytes(buf[int(begin[-1]):int(end[-1])]))
                    left = n - used
                    if left:
                        pinned[1 - turn].array[:left] = buf[used:n]
                    turn = 1 - turn
                    if final:
                        break
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
