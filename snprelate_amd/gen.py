"""Oxford GEN + sample files as a genotype source: what ``snpgdsGEN2GDS`` + ``snpgdsOpen`` give in the reference, without the GDS
file in between.

The division of work follows the text.  A .gen line is five short columns and then three decimal numbers per sample, about 1.8 MB
of a line at 100 000 samples.  So

* the host reads the sample file (:func:`read_sample`), reads a .gen file (plain or ``.gz``) in chunks of whole lines into
  page-locked buffers, finds the lines and reads the five leading columns of each with ``textio.Cells`` -- the restatement of
  ``CReadLine::GetCell`` (src/ConvToGDS.cpp:123-179) splitting by space and tab -- and ``vcf.get_int32`` for the position;
* the device reads the numbers of the rest of every line, rounds each once to single precision as ``strtof`` does and calls
  every sample through the tree of gnrParseGEN (src/ConvToGDS.cpp:1134-1145): ``snpgpu_gen_genotypes``, the chunk's own bytes
  being its input;
* a line the kernel flags (an exponent, a sign, ``inf``, ``nan``, a quote, a ``\\r``, ``.`` alone, more digits than fp64 holds
  exactly, an empty cell, a wrong number of cells) is read again by ``snpgpu_gen_line_host``, which follows the reference's loop
  character for character with the C library's ``strtof``: its row is patched, or the reference's message is raised with
  ``FILE:``, ``LINE:``, ``COLUMN:``.

There is no CPU fallback for the calls: without a device :meth:`GenReader.blocks` fails with ``SnpGpuError``.
"""
import functools

import numpy as np

from . import textio
from .gds import pack_2bit_rows
from .textio import Cells, VcfFormatError, c_string, last_cell, open_binary, stage_bytes
from .vcf import get_int32

VERSIONS = (">=2.0", "<=1.1.5")


# ---- the sample file -------------------------------------------------------------------------------------------------------------
def _fields(raw):
    t = raw.decode("latin1").split()
    return [x[1:-1] if len(x) > 1 and x[0] == x[-1] and x[0] in "\"'" else x for x in t]


def read_sample(sample_fn, version=">=2.0"):
    """the sample file as R/Conversion.R:849-858 reads it: a header line, with version ">=2.0" one line of column types that is
    skipped, then one line per sample; whitespace-separated, empty lines skipped.  (sample_id, {column name: text per sample})
    with sample_id the first column."""
    if version not in VERSIONS:
        raise ValueError("'arg' should be one of \">=2.0\", \"<=1.1.5\"")
    with open_binary(sample_fn) as f:
        lines = [t for t in (_fields(raw) for raw in f) if t]
    if not lines:
        raise ValueError("'%s' has no header line" % sample_fn)
    names, data = lines[0], lines[(2 if version == ">=2.0" else 1):]
    if not data:
        raise ValueError("'%s' has no sample" % sample_fn)
    for k, t in enumerate(data):
        if len(t) != len(names):
            raise ValueError("'%s': sample %d has %d columns, the header has %d" % (sample_fn, k + 1, len(t), len(names)))
    cols = {name: np.array([t[j] for t in data], dtype=str) for j, name in enumerate(names)}
    return np.array([t[0] for t in data], dtype=str), cols


# ---- a line on the host ------------------------------------------------------------------------------------------------------------
def host_head(line):
    """the five leading cells of a .gen line (SNP id, rs id, position, allele A, allele B) with the position through getInt32, and
    the offset of the sixth, as gnrParseGEN reads them (src/ConvToGDS.cpp:1094-1110); VcfFormatError carries the column and what
    the reference's `cell` variable holds there: the alleles are read into variables of their own, so from column 4 to the first
    probability it is still the position."""
    rl = Cells(line, space=True)
    snp, rs, pos = rl.get(False), rl.get(False), rl.get(False)
    try:
        position = get_int32(pos)
    except VcfFormatError as err:
        raise VcfFormatError(err.message, 3, pos)
    try:
        a, b = rl.get(False), rl.get(False)
    except VcfFormatError as err:
        raise VcfFormatError(err.message, err.column, pos)
    return (snp, rs, position, a, b), rl.p


def error_cell(line, column, message, tail=b""):
    """what the reference's `cell` variable holds when reading cell `column` (1-based, of the whole line) fails with `message`:
    the cell itself for a conversion, else the last cell read into it -- the position up to column 6, the last cell of the line
    in front (`tail`) at column 1"""
    rl = Cells(c_string(line), space=True)
    cells = []
    try:
        for _ in range(column):
            cells.append(rl.get(False))
    except VcfFormatError:
        pass
    if message.startswith("Invalid") and len(cells) >= column:
        return cells[column - 1]
    prev = min(column - 1, len(cells))
    if prev == 0:
        return tail
    return cells[2] if 3 <= prev <= 5 else cells[prev - 1]


def pack_row(codes):
    """one PACKED2 row as snpgpu_gen_genotypes writes it: the unused codes of the last byte are 0"""
    row = pack_2bit_rows(codes[None, :])[0]
    if len(codes) & 3:
        row[-1] &= (1 << (2 * (len(codes) & 3))) - 1
    return row


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
class GenReader:
    """One .gen file read once, front to back.  The per-variant nodes (snp_id: column 1 as text, snp_rs_id, snp_position,
    snp_allele "A/B") grow as :meth:`blocks` goes through the file and are numpy arrays after it.  flagged_lines counts what the
    kernel left to the host, windows the chunks of text."""

    def __init__(self, gen_fn, n_samp, call_threshold=0.9, chunk_bytes=None):
        self.path, self.n_samp, self.call_threshold = str(gen_fn), int(n_samp), float(call_threshold)
        if self.n_samp < 1:
            raise ValueError("n_samp should be positive")
        self.chunk_bytes = int(chunk_bytes) if chunk_bytes else stage_bytes()
        self.flagged_lines, self.windows, self.n_snp = 0, 0, 0
        self._nodes = dict(snp=[], rs=[], pos=[], allele=[])
        self._tail = b""                                   # the last cell of the line in front of the current one
        self._done = False

    def _raise(self, message, column, cell, file_line):
        raise ValueError("%s\nFILE: %s\nLINE: %d, COLUMN: %d, %s\n" % (message, self.path, file_line, column, cell.decode("latin1")))

    def _finish(self):
        d = self._nodes
        text = lambda v: np.array(v, dtype=str) if v else np.empty(0, dtype="<U1")          # noqa: E731
        self.snp_id, self.snp_rs_id, self.snp_allele = text(d["snp"]), text(d["rs"]), text(d["allele"])
        self.snp_position = np.array(d["pos"], np.int32)
        self.n_snp = len(self.snp_id)

    def blocks(self, block_snps, device=0):
        """(snp_begin, n_snp, rows) in one pass over the file: rows is a torch uint8 tensor [n_snp][ceil(n_samp / 4)] on `device`,
        SNPGPU_GENO_PACKED2 with padding codes 0, valid until the next block is asked for.  A block holds at most block_snps
        lines and never spans two chunks of the file.  The calls are synchronous."""
        from . import _lib
        block_snps = int(block_snps)
        if block_snps < 1:
            raise ValueError("block_snps should be positive")
        if self._done:
            raise ValueError("a GenReader goes through its file once")
        if _lib.device_count() < 1:
            raise _lib.SnpGpuError("GenReader.blocks: no HIP device (the GEN genotype caller has no CPU fallback)")
        import torch
        size, N, rb = self.chunk_bytes, self.n_samp, (self.n_samp + 3) // 4
        pinned = [_lib.PinnedBuffer((size,)) for _ in range(2)]
        dev = [None, None]
        blk, file_line, done, nodes = 0, 0, 0, self._nodes
        lines = functools.partial(textio.split_lines, strip_cr=False)           # a '\r' stays: the reference's isspace skips it
        try:
            with open_binary(self.path) as f:
                for buf, n, _final, begin, end in textio.chunks(f, [p.array for p in pinned], lines, self.path, "SNPGPU_TEXT_STAGE_BYTES"):
                    ptr = pinned[0].ptr if buf is pinned[0].array else pinned[1].ptr
                    # ---- the leading columns; a line that fails there ends the chunk, the lines in front of it are still called --------
                    cell_begin, heads, err = textio.leading_columns(buf, begin, end, host_head, self._tail)
                    n_lines = len(cell_begin)
                    for cells in heads:
                        nodes["snp"].append(cells[0].decode("latin1"))
                        nodes["rs"].append(cells[1].decode("latin1"))
                        nodes["pos"].append(cells[2])
                        nodes["allele"].append((cells[3] + b"/" + cells[4]).decode("latin1"))
                    # ---- the probabilities: blocks of lines on the device ------------------------------------------------------------------
                    for lo in range(0, n_lines, block_snps):
                        hi = min(lo + block_snps, n_lines)
                        m = hi - lo
                        if dev[blk & 1] is None or dev[blk & 1].shape[0] < m:
                            dev[blk & 1] = torch.empty((m, rb), dtype=torch.uint8, device="cuda:%d" % int(device))
                        rows = dev[blk & 1][:m]
                        blk += 1
                        flags, _cells = _lib.gen_genotypes(ptr, cell_begin[lo:hi], end[lo:hi], N, self.call_threshold,
                                                           int(rows.data_ptr()), n_bytes=n, text_mem=_lib.HOST_PINNED, device=device)
                        for i in np.flatnonzero(flags):
                            k = lo + int(i)
                            b, e = int(begin[k]), int(end[k])
                            codes, column, message = _lib.gen_line_host(c_string(bytes(buf[int(cell_begin[k]):e])), N, self.call_threshold)
                            if codes is None:
                                line = bytes(buf[b:e])
                                tail = last_cell(bytes(buf[int(begin[k - 1]):int(end[k - 1])])) if k else self._tail
                                self._raise(message, column + 5, error_cell(line, column + 5, message, tail), file_line + k + 1)
                            rows[int(i)].copy_(torch.from_numpy(pack_row(codes)))
                        if flags.any():
                            self.flagged_lines += int(np.count_nonzero(flags))
                            torch.cuda.synchronize(int(device))
                        self.n_snp = done + m
                        yield done, m, rows
                        done += m
                    if err is not None:
                        self._raise(err.message, err.column, err.cell, file_line + n_lines + 1)
                    self.windows += 1
                    file_line += n_lines
                    self._tail = last_cell(bytes(buf[int(begin[-1]):int(end[-1])]))
        finally:
            self._done = True
            for p in pinned:
                p.free()
            self._finish()
