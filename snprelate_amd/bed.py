"""PLINK binary PED files (.bed / .bim / .fam) as genotype sources and as output.

A ``.bed`` file is a 3-byte header ``6C 1B mode`` and then the 2-bit matrix this package already moves on the device: 4
genotypes per byte, LSB first, every row starting on a byte, the unused codes of a row's last byte zero.  ``mode`` 1 is
SNP-major (``n_snp`` rows of ``ceil(n_samp / 4)`` bytes), ``mode`` 0 individual-major (``n_samp`` rows of ``ceil(n_snp / 4)``
bytes).  Its codes are 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2 where the GDS genotype node (and
SNPGPU_GENO_PACKED2) counts A alleles: BED -> GDS is {2, 3, 1, 0} (src/ConvToGDS.cpp:585), GDS -> BED {3, 2, 0, 1}
(src/SNPRelate.cpp:801).

* :func:`read_fam`, :func:`read_bim` -- the two text files, ``.gz`` through gzip as the reference's connections do;
* :class:`BedStream` -- a :class:`~snprelate_amd.gds.GenoStream` over a ``.bed`` file with the metadata ``snpgdsBED2GDS`` would
  have stored (R/Conversion.R:479-653), so that every ``snpgds*`` function takes it as it takes an opened GDS file.  ``blocks()``
  recodes on the host with numpy; ``select_blocks()`` hands the file's own bytes to the device (``snpgpu_geno_convert``);
* :func:`encode_bed` -- GDS codes to the bytes of a ``.bed`` body with numpy, for ``snpgdsGDS2BED`` without a device.
"""
import gzip
import os
import re
import warnings

import numpy as np

from .gds import GenoStream, gather_segments, pack_2bit_rows

MAGIC = b"\x6c\x1b"
BED_TO_GDS = np.array([2, 3, 1, 0], np.uint8)
GDS_TO_BED = np.array([3, 2, 0, 1], np.uint8)


def _byte_table(code_table):
    """the map of one code applied to the four codes of every byte value"""
    b = np.arange(256, dtype=np.uint16)
    out = np.zeros(256, np.uint16)
    for k in range(4):
        out |= code_table[(b >> (2 * k)) & 3].astype(np.uint16) << (2 * k)
    return out.astype(np.uint8)


_BED_TO_GDS_BYTE = _byte_table(BED_TO_GDS)


def default_option(autosome_start=1, autosome_end=22, **chromosome_code):
    """snpgdsOption() without a file (R/AllUtilities.R:1910-1990): the autosome range and the chromosome codes, by default
    X, XY, Y, M = MT = autosome_end + 1 ... + 4"""
    e = int(autosome_end)
    code = dict(chromosome_code) if chromosome_code else {"X": e + 1, "XY": e + 2, "Y": e + 3, "M": e + 4, "MT": e + 4}
    return {"autosome_start": int(autosome_start), "autosome_end": e, "chromosome_code": code}


def _open_text(fn):
    return gzip.open(fn, "rt", encoding="latin1") if str(fn).lower().endswith(".gz") else open(fn, "r", encoding="latin1")


def _read_columns(fn, names):
    """the whitespace-separated columns of a text file as lists of strings (read.table(header=FALSE, comment.char=""))"""
    cols = [[] for _ in names]
    with _open_text(fn) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if len(t) != len(names):
                raise ValueError("'%s', line %d: %d columns where %d are expected (%s)" % (fn, ln, len(t), len(names), ", ".join(names)))
            for c, v in zip(cols, t):
                c.append(v)
    return dict(zip(names, cols))


def _type_convert(x):
    """a text column as read.table types it: integers when every entry is one, else numbers, else strings"""
    for t in (np.int64, np.float64):
        try:
            return np.array(x, dtype=object).astype(t)
        except (ValueError, OverflowError):
            pass
    return np.array(x, dtype=str)


def read_fam(fn):
    """dict of the six columns FamilyID, InvID, PatID, MatID, Sex, Pheno of a .fam file, typed as read.table would"""
    d = _read_columns(fn, ("FamilyID", "InvID", "PatID", "MatID", "Sex", "Pheno"))
    return {k: _type_convert(v) for k, v in d.items()}


def read_bim(fn):
    """dict of the six columns chr (always text), snp_id, map, pos, allele1, allele2 of a .bim file"""
    d = _read_columns(fn, ("chr", "snp_id", "map", "pos", "allele1", "allele2"))
    out = {k: _type_convert(v) for k, v in d.items()}
    out["chr"] = np.array(d["chr"], dtype=str)
    out["allele1"], out["allele2"] = np.array(d["allele1"], dtype=str), np.array(d["allele2"], dtype=str)
    return out


def chrom_numeric(chrom):
    """the leading integer of every chromosome label as strtol reads it (gnrChromParse, src/SNPRelate.cpp:982-1032) and whether
    there is one"""
    val = np.zeros(len(chrom), np.int64)
    ok = np.zeros(len(chrom), bool)
    for i, s in enumerate(chrom):
        m = re.match(r"\s*[+-]?\d+", str(s))
        if m:
            val[i], ok[i] = int(m.group()), True
    return val, ok


def _inflate_cap():
    return int(os.environ.get("SNPGPU_GDS_INFLATE_MAX", 8 << 30))


class BedStream(GenoStream):
    """A PLINK .bed / .bim / .fam triple opened for reading: what snpgdsBED2GDS + snpgdsOpen give in the reference, without the
    GDS file in between.  The genotypes stay in the file: a plain .bed is memory-mapped, a .bed.gz is inflated once into host
    memory (refused above SNPGPU_GDS_INFLATE_MAX bytes, default 8 GiB).  Blocks come out as SNPGPU_GENO_PACKED2 rows, the A1
    allele counted as the GDS file of snpgdsBED2GDS would count it."""

    def __init__(self, bed_fn, fam_fn, bim_fn, family=False, option=None, cvt_chr="int", cvt_snpid="auto"):
        if cvt_chr not in ("int", "char"):
            raise ValueError("'cvt.chr' should be one of \"int\", \"char\"")
        if cvt_snpid not in ("auto", "int"):
            raise ValueError("'cvt.snpid' should be one of \"auto\", \"int\"")
        fam, bim = read_fam(fam_fn), read_bim(bim_fn)
        n, L = len(fam["InvID"]), len(bim["snp_id"])
        if n < 1 or L < 1:
            raise ValueError("'%s' / '%s': no sample or no SNP" % (fam_fn, bim_fn))
        self.path, self.fam_fn, self.bim_fn = str(bed_fn), str(fam_fn), str(bim_fn)
        self.n_samp, self.n_snp = n, L

        sample_id = fam["InvID"]
        if len(np.unique(sample_id)) != n:
            sample_id = np.array(["%s-%s" % (a, b) for a, b in zip(fam["FamilyID"], fam["InvID"])])
            if len(np.unique(sample_id)) != n:
                raise ValueError("IDs in PLINK BED are not unique!")
        self.sample_id = sample_id
        self.snp_rs_id = None
        if cvt_snpid == "auto" and len(np.unique(bim["snp_id"])) == L:
            self.snp_id = bim["snp_id"]
        else:
            self.snp_id, self.snp_rs_id = np.arange(1, L + 1, dtype=np.int32), bim["snp_id"]
        self.snp_position = np.asarray(bim["pos"]).astype(np.int32)
        self.snp_allele = np.array(["%s/%s" % (a, b) for a, b in zip(bim["allele1"], bim["allele2"])])

        if cvt_chr == "int":
            opt = default_option() if option is None else option
            label = bim["chr"].astype(object)
            for name, code in opt["chromosome_code"].items():
                label[bim["chr"] == name] = str(code)
            chrom = np.zeros(L, np.int32)
            bad = False
            for i, s in enumerate(label):
                try:
                    chrom[i] = int(s)
                except ValueError:
                    bad = True
            if bad:
                warnings.warn("Please use cvt.chr=\"char\" for non-numeric chromosome codes, otherwise non-numeric codes are replaced "
                              "by zero.")
            self.snp_chromosome = chrom
            self.autosome_start, self.autosome_end = int(opt["autosome_start"]), int(opt["autosome_end"])
            self.chromosome_code = dict(opt["chromosome_code"])
        else:
            if option is not None:
                raise ValueError("'option' should be NULL when 'cvt.chr=\"char\"'.")
            self.snp_chromosome = bim["chr"]
            # autosome_only=True keeps the labels that parse (chrom_numeric) into 1 ... 22
            self.autosome_start, self.autosome_end = 1, 22
            self.chromosome_code = {}

        sex = np.array(["M" if s == 1 else "F" if s == 2 else "" for s in
                        (fam["Sex"] if fam["Sex"].dtype.kind in "if" else np.zeros(n))])
        annot = {"sex": sex, "phenotype": fam["Pheno"]}
        if family:
            annot = {"family": fam["FamilyID"], "father": fam["PatID"], "mother": fam["MatID"], **annot}
        self.sample_annot = annot

        self._gz = self.path.lower().endswith(".gz")
        head = self._read_head()
        if head[:2] != MAGIC:
            raise ValueError("'%s' is not a PLINK BED file (magic number %s, not 6c 1b)" % (self.path, head[:2].hex(" ") or "missing"))
        if len(head) < 3 or head[2] not in (0, 1):
            raise ValueError("'%s': invalid mode byte %s (0: individual-major, 1: SNP-major)"
                             % (self.path, "missing" if len(head) < 3 else "%d" % head[2]))
        self.mode = int(head[2])
        self.sample_order = self.mode == 1
        rows, cols = (L, n) if self.mode == 1 else (n, L)
        self._rows, self._row_bytes = rows, (cols + 3) // 4
        need = 3 + rows * self._row_bytes
        have = self._length_of(need)
        if have != need:
            raise ValueError("'%s' holds %s bytes where %d %s of %d genotypes need 3 + %d x %d = %d (%d samples in '%s', %d SNPs in '%s')"
                             % (self.path, "more than %d" % need if have > need and self._gz else "%d" % have, rows,
                                "SNPs" if self.mode == 1 else "samples", cols, rows, self._row_bytes, need, n, self.fam_fn, L, self.bim_fn))

    # ---- the file's bytes ----
    def _read_head(self):
        with (gzip.open(self.path, "rb") if self._gz else open(self.path, "rb")) as f:
            return f.read(3)

    def _length_of(self, need):
        if not self._gz:
            return os.path.getsize(self.path)
        if need > _inflate_cap():
            raise ValueError("'%s': a compressed .bed of %d bytes does not fit the in-memory budget of %d bytes "
                             "(SNPGPU_GDS_INFLATE_MAX)" % (self.path, need, _inflate_cap()))
        with gzip.open(self.path, "rb") as f:
            d = f.read(need + 1)                                       # one byte more shows a file that is too long
        if len(d) == need:
            self._inflated = np.frombuffer(d, np.uint8)[3:]
        return len(d)

    def _body(self):
        """the rows after the header, uint8 [rows x row bytes]: a memory map, or the inflated copy of a .gz"""
        if self._gz:
            return self._inflated
        return np.memmap(self.path, dtype=np.uint8, mode="r", offset=3, shape=(self._rows * self._row_bytes,))

    # ---- the host path ----
    def blocks(self, block_snps, buffers=None, snp_begin=0, snp_end=None):
        snp_end = self.n_snp if snp_end is None else min(int(snp_end), self.n_snp)
        n, rb, body = self.n_samp, (self.n_samp + 3) // 4, self._body()
        pad = (0xFF << (2 * (n % 4))) & 0xFF if n % 4 else 0
        by_sample = body.reshape(self._rows, self._row_bytes) if self.mode == 0 else None
        turn = 0
        for lo in range(snp_begin, snp_end, block_snps):
            hi = min(lo + block_snps, snp_end)
            if self.mode == 1:
                rows = _BED_TO_GDS_BYTE[np.asarray(body[lo * rb:hi * rb])].reshape(hi - lo, rb)
                if pad:
                    rows[:, -1] |= pad
            else:
                # every sample's bytes of the block's SNP range (as _blocks_snp_order: a strided read over the sample rows)
                b0 = lo >> 2
                seg = np.asarray(by_sample[:, b0:(hi + 3) >> 2])
                codes = np.stack([(seg >> (2 * k)) & 3 for k in range(4)], 2).reshape(n, -1)[:, lo - 4 * b0:][:, :hi - lo]
                rows = pack_2bit_rows(np.ascontiguousarray(BED_TO_GDS[codes].T))
            if buffers is not None:
                out = np.asarray(buffers[turn % len(buffers)]).reshape(-1)[:(hi - lo) * rb].reshape(hi - lo, rb)
                out[:] = rows
                rows = out
                turn += 1
            yield lo, hi - lo, rows

    # ---- the device path ----
    def select_blocks(self, block_snps, samp_index=None, snp_begin=0, snp_end=None, device=0, to="device"):
        """GenoStream.select_blocks for a .bed file: the file's own bytes go to the device and come back recoded
        (snpgpu_geno_convert, BED -> GDS) as SNPGPU_GENO_PACKED2 rows of the selected samples.  Mode 1: the block's byte range.
        Mode 0: the selected samples' segments of the block's SNP range, gathered into a page-locked buffer with a bit phase per
        row.  The file is never read or copied as a whole."""
        from . import _lib
        if to not in ("device", "host"):
            raise ValueError("'to' should be \"device\" or \"host\"")
        block_snps = int(block_snps)
        if block_snps < 1:
            raise ValueError("block_snps should be positive")
        n, L = self.n_samp, self.n_snp
        snp_begin = int(snp_begin)
        snp_end = L if snp_end is None else min(int(snp_end), L)
        samp = None
        if samp_index is not None:
            samp = np.ascontiguousarray(samp_index, dtype=np.int32).reshape(-1)
            if samp.size == 0 or samp.min() < 0 or samp.max() >= n:
                raise ValueError("samp_index should hold positions 0 ... n_samp - 1 of the file's samples")
        n_out = n if samp is None else samp.size
        rb = (n_out + 3) // 4
        bmax = max(1, min(block_snps, snp_end - snp_begin))
        dev_bufs = pinned = None
        if to == "device":
            import torch
            dev_bufs = [torch.empty((bmax, rb), dtype=torch.uint8, device="cuda:%d" % int(device)) for _ in range(2)]

        def out_of(turn, m):
            if dev_bufs is None:
                return np.empty((m, rb), np.uint8), None
            t = dev_bufs[turn & 1][:m]
            return int(t.data_ptr()), t

        body, frb = self._body(), self._row_bytes
        try:
            if self.mode == 1:
                for turn, lo in enumerate(range(snp_begin, snp_end, block_snps)):
                    hi = min(lo + block_snps, snp_end)
                    out, t = out_of(turn, hi - lo)
                    _lib.geno_convert(np.asarray(body[lo * frb:hi * frb]), 0, hi - lo, n, src_code=_lib.CODE_BED, row_stride_bits=8 * frb,
                                      samp_index=samp, out=out, device=device)
                    yield lo, hi - lo, (out if t is None else t)
            else:
                rows = np.arange(n, dtype=np.int64) if samp is None else samp.astype(np.int64)
                w = min(len(body), (2 * bmax + 6 + 7) >> 3)                     # bytes of a segment at the worst phase
                pinned = _lib.PinnedBuffer((n_out * w,))
                for turn, lo in enumerate(range(snp_begin, snp_end, block_snps)):
                    hi = min(lo + block_snps, snp_end)
                    bit = 8 * rows * frb + 2 * lo
                    start = np.minimum(bit >> 3, len(body) - w)                 # a window at the end of the file is moved back
                    stage = pinned.array[:n_out * w].reshape(n_out, w)
                    gather_segments(body, start, w, stage)
                    row_bit = 8 * w * np.arange(n_out, dtype=np.int64) + (bit - 8 * start)
                    out, t = out_of(turn, hi - lo)
                    _lib.geno_convert(pinned.ptr, 1, n_out, hi - lo, src_code=_lib.CODE_BED, row_bit=row_bit, n_bytes=n_out * w,
                                      mem=_lib.HOST_PINNED, out=out, device=device)
                    yield lo, hi - lo, (out if t is None else t)
        finally:
            if pinned is not None:
                pinned.free()


def encode_bed(geno, individual_major=False):
    """GDS codes uint8 [n_snp][n_samp] (0 / 1 / 2 A alleles, 3 missing) as the rows of a .bed body: uint8 [n_snp][ceil(n_samp / 4)],
    or for individual_major [n_samp][ceil(n_snp / 4)]; the unused codes of a row's last byte are 0"""
    g = GDS_TO_BED[np.minimum(np.asarray(geno, np.uint8), 3)]
    if individual_major:
        g = g.T
    R, C = g.shape
    full = np.zeros((R, 4 * ((C + 3) // 4)), np.uint8)
    full[:, :C] = g
    full = full.reshape(R, -1, 4)
    return (full[:, :, 0] | (full[:, :, 1] << 2) | (full[:, :, 2] << 4) | (full[:, :, 3] << 6)).astype(np.uint8)
