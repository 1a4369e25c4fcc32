"""Putting data sets together: snpgdsSNPList, snpgdsSNPListIntersect, snpgdsCombineGeno and snpgdsAlleleSwitch.

Which SNPs two data sets share and which of them count the other allele is host work -- strings and a hash join over allele
names, strand complements and allele frequencies (snpgdsSNPListIntersect -> gnrAlleleStrand, src/SNPRelate.cpp:866-978).  Moving
the genotypes is device work: ``snpgpu_geno_merge`` places every file's selected rectangle at its column offset of the merged 2-bit
rows and re-codes the flagged rows, two bits per genotype all the way.  The merged rows come back to host memory window by window
(SNPGPU_MERGE_STAGE_BYTES of them at a time).  There is no CPU fallback: without a device the two genotype-moving functions fail
with ``SnpGpuError``.
"""
import os

import numpy as np

from . import _lib
from .gds import GenoFile, GenoStream

NA_INTEGER = -2 ** 31

_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
_CATEGORIES = ("no flip", "flip", "no flip on different strand", "flip on different strand", "no flip / ambiguous strand",
               "flip / ambiguous strand", "no flip / different and ambiguous strand", "flip / different and ambiguous strand")


class SNPList(dict):
    """what snpgdsSNPList returns (the reference's "snpgdsSNPListClass" data frame): snp_id, chromosome, position, allele, afreq"""


def snp_list(gdsobj, afreq):
    for node, name in ((gdsobj.snp_position, "snp.position"), (gdsobj.snp_allele, "snp.allele")):
        if node is None:
            raise ValueError("No such GDS node \"%s\"!" % name)
    return SNPList(snp_id=np.asarray(gdsobj.snp_id), chromosome=np.asarray(gdsobj.snp_chromosome), position=np.asarray(gdsobj.snp_position),
                   allele=np.asarray(gdsobj.snp_allele), afreq=np.asarray(afreq, np.float64))


# ---- gnrAlleleStrand -----------------------------------------------------------------------------------------------------------
def split_allele(txt):
    """the two alleles of "A/B" as gnrAlleleStrand reads them: split at the first '/', else at the first ',', upper-cased; no
    separator leaves the second one empty"""
    txt = str(txt)
    p = txt.find("/")
    if p < 0:
        p = txt.find(",")
    if p < 0:
        return txt.upper(), ""
    return txt[:p].upper(), txt[p + 1:].upper()


def _minor_side(f):
    return 0 if f <= 0.5 else 1                        # a NaN frequency is side 1


def allele_strand(allele1, allele2, afreq1, afreq2, same_strand=False):
    """int32 per SNP: bit 1 = allele2 counts the other allele (flip), bit 2 = it is on the other strand, bit 4 = the names cannot
    tell the strand (A/T, C/G) and the flip was decided by which side of 0.5 the two frequencies lie; NA_INTEGER = mismatch"""
    out = np.full(len(allele1), NA_INTEGER, np.int32)
    for i in range(len(allele1)):
        r1, r2 = split_allele(allele1[i])
        d1, d2 = split_allele(allele2[i])
        flag, by_freq = None, False
        if same_strand:
            if r1 == d1 and r2 == d2:
                flag = 0
            elif r1 == d2 and r2 == d1:
                flag = 1
        else:
            if r1 == d1 and r2 == d2:
                by_freq = d2 in _COMPLEMENT and r1 == _COMPLEMENT[d2]
                flag = 0
            elif r1 == d2 and r2 == d1:
                by_freq = d1 in _COMPLEMENT and r1 == _COMPLEMENT[d1]
                flag = 1
            elif all(x in _COMPLEMENT for x in (r1, r2, d1, d2)):
                if r1 == _COMPLEMENT[d1] and r2 == _COMPLEMENT[d2]:
                    by_freq = r1 == d2
                    flag = 2
                elif r1 == _COMPLEMENT[d2] and r2 == _COMPLEMENT[d1]:
                    by_freq = r1 == d1
                    flag = 3
            if by_freq and flag is not None:
                flag = (1 if _minor_side(afreq1[i]) != _minor_side(afreq2[i]) else 0) | (flag & ~1) | 4
        if flag is not None:
            out[i] = flag
    return out


# ---- snpgdsSNPListIntersect ----------------------------------------------------------------------------------------------------
def _keys(lst, method):
    if method == "position":
        return ["%s:%s" % (c, p) for c, p in zip(lst["chromosome"], lst["position"])]
    return ["%s:%s:%s:%s" % (s, c, p, a) for s, c, p, a in zip(lst["snp_id"], lst["chromosome"], lst["position"], lst["allele"])]


def snp_list_intersect(lists, method="position", na_rm=True, same_strand=False):
    """R/AllUtilities.R:667-736: dict idx1 ... idxK (0-based positions of the common SNPs in every list: the order of list 1,
    duplicates dropped, the first occurrence in each list) and, for method "position", flag2 ... flagK (allele_strand against list 1)"""
    for x in lists:
        if not isinstance(x, SNPList):
            raise TypeError("All objects should be 'snpgdsSNPListClass'.")
    if method not in ("position", "exact"):
        raise ValueError("'arg' should be one of \"position\", \"exact\"")
    for v, name in ((na_rm, "na.rm"), (same_strand, "same.strand")):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    keys = [_keys(x, method) for x in lists]
    first = []
    for k in keys:
        d = {}
        for i, key in enumerate(k):
            d.setdefault(key, i)
        first.append(d)
    common = [key for key in first[0] if all(key in d for d in first[1:])]          # dicts keep the order of insertion
    rv = {}
    for i, d in enumerate(first):
        rv["idx%d" % (i + 1)] = np.array([d[key] for key in common], np.int32)
    if method == "position":
        ii = rv["idx1"]
        al1, af1 = lists[0]["allele"][ii], lists[0]["afreq"][ii]
        for i in range(1, len(lists)):
            ii = rv["idx%d" % (i + 1)]
            rv["flag%d" % (i + 1)] = allele_strand(al1, lists[i]["allele"][ii], af1, lists[i]["afreq"][ii], bool(same_strand))
        if na_rm:
            keep = np.ones(len(common), bool)
            for i in range(1, len(lists)):
                keep &= rv["flag%d" % (i + 1)] != NA_INTEGER
            if not keep.all():
                rv = {k: v[keep] for k, v in rv.items()}
    return rv


# ---- the genotypes ---------------------------------------------------------------------------------------------------------------
def stage_bytes():
    return max(1, int(os.environ.get("SNPGPU_MERGE_STAGE_BYTES", 256 << 20)))


def need_device(what):
    try:
        ok = _lib.device_count() > 0
    except _lib.SnpGpuError:
        ok = False
    if not ok:
        raise _lib.SnpGpuError("%s: no HIP device (merging genotypes has no CPU fallback)" % what)


def merged_rows(sources, n_snp_out, device=0):
    """uint8 [n_snp_out][ceil(N / 4)] in host memory from snpgpu_geno_merge.  sources: per part (packed rows uint8 [n_snp][ceil(n /
    4)], n, samp_index | None, snp_index | None, flip | None).  A window of output rows is merged on the device and copied back;
    of every source only the span of rows the window names goes along."""
    import torch
    N = sum(n if samp is None else len(samp) for _, n, samp, _, _ in sources)
    rb = (N + 3) // 4
    out = np.empty((n_snp_out, rb), np.uint8)
    per = max(1, min(n_snp_out, stage_bytes() // rb))
    dev = torch.empty((per, rb), dtype=torch.uint8, device="cuda:%d" % int(device))
    for k0 in range(0, n_snp_out, per):
        k1 = min(k0 + per, n_snp_out)
        parts = []
        for packed, n, samp, snp, flip in sources:
            if snp is None:
                lo, hi, idx = k0, k1, None
            else:
                w = np.asarray(snp[k0:k1], np.int64)
                lo, hi = int(w.min()), int(w.max()) + 1
                idx = (w - lo).astype(np.int32)
            parts.append(_lib.merge_part(packed[lo:hi], 0, hi - lo, n, row_stride_bits=8 * ((n + 3) // 4), samp_index=samp, snp_index=idx,
                                         flip=None if flip is None else flip[k0:k1]))
        _lib.geno_merge(parts, int(dev.data_ptr()), n_snp_out=k1 - k0, device=device)
        out[k0:k1] = dev[:k1 - k0].cpu().numpy()
    return out


def _match(want, have):
    """R's match(): the first position of every entry of `want` in `have`"""
    d = {}
    for i, x in enumerate(have):
        d.setdefault(x, i)
    return np.array([d[x] for x in want], np.int32)


def _concat(arrays):
    arrays = [np.asarray(a) for a in arrays]
    if len({a.dtype.kind in "USO" for a in arrays}) > 1:
        arrays = [a.astype(str) for a in arrays]
    return np.concatenate(arrays)


def combine_common_samples(files, samp_id, device=0):
    """branch 1 of snpgdsCombineGeno (R/AllUtilities.R:1336-1436): the SNPs of all files one after the other, over the samples
    they share"""
    for f in files:
        if f.snp_position is None or f.snp_allele is None:
            raise ValueError("No such GDS node \"%s\"!" % ("snp.position" if f.snp_position is None else "snp.allele"))
    rows = []
    for f in files:
        ii = _match(samp_id, f.sample_id)
        rows.append(merged_rows([(f.packed, f.n_samp, ii, None, None)], f.n_snp, device))
    n_snp = sum(f.n_snp for f in files)
    out = GenoFile(packed=np.concatenate(rows, 0), n_samp=len(samp_id), sample_id=np.asarray(samp_id),
                   snp_id=np.arange(1, n_snp + 1, dtype=np.int32), snp_chromosome=_concat([f.snp_chromosome for f in files]),
                   snp_position=np.concatenate([f.snp_position for f in files]), snp_allele=_concat([f.snp_allele for f in files]))
    if getattr(files[0], "snp_rs_id", None) is not None:
        out.snp_rs_id = np.concatenate([np.asarray(f.snp_rs_id).astype(str) if getattr(f, "snp_rs_id", None) is not None
                                        else np.full(f.n_snp, "") for f in files])
    return out


def combine_common_snps(files, lists, snp, device=0):
    """branch 2 of snpgdsCombineGeno (R/AllUtilities.R:1482-1556): the samples of all files side by side over the common SNPs `snp`
    (snp_list_intersect), every file's flagged rows re-coded to file 1's allele.  The strand and ambiguity bits of a flag leave the
    genotypes alone, as in the reference."""
    idx1 = snp["idx1"]
    sources = []
    for i, f in enumerate(files):
        flag = snp.get("flag%d" % (i + 1))
        flip = None if flag is None else ((flag != NA_INTEGER) & ((flag & 1) != 0)).astype(np.uint8)
        sources.append((f.packed, f.n_samp, None, snp["idx%d" % (i + 1)], flip))
    packed = merged_rows(sources, len(idx1), device)
    f1 = files[0]
    annot = {}
    for name in f1.sample_annot:
        if all(name in f.sample_annot for f in files):
            annot[name] = _concat([f.sample_annot[name] for f in files])
    out = GenoFile(packed=packed, n_samp=sum(f.n_samp for f in files), sample_id=_concat([f.sample_id for f in files]),
                   snp_id=lists[0]["snp_id"][idx1], snp_chromosome=lists[0]["chromosome"][idx1], snp_position=lists[0]["position"][idx1],
                   snp_allele=lists[0]["allele"][idx1], sample_annot=annot)
    if getattr(f1, "snp_rs_id", None) is not None:
        out.snp_rs_id = np.asarray(f1.snp_rs_id)[idx1]
    return out


def print_flags(i, x):
    """the reference's lines for file i (1-based, i >= 2).  Its counts are sums of the masked bit VALUES (R/AllUtilities.R:1463-1465):
    the second figure is four times the number of ambiguous loci, and is printed as the reference prints it."""
    ok = x != NA_INTEGER
    print("    file %d: %d allele flips, %d ambiguous locus/loci" % (i, int((x[ok] & 1).sum()), int((x[ok] & 4).sum())))
    counts = [int((x == v).sum()) for v in range(8)] + [int((~ok).sum())]
    for name, y in zip(_CATEGORIES + ("mismatch",), counts):
        if y > 0:
            print("        [%s]: %d" % (name, y))


# ---- snpgdsAlleleSwitch ----------------------------------------------------------------------------------------------------------
def switch_flags(snp_allele, a_allele):
    """gnrStrandSwitch's decision (src/SNPRelate.cpp:428-452): snp.allele split at the first '/' only, compared as it is; int32 0 =
    A is the given allele, 1 = B is (the alleles are exchanged), NA_INTEGER otherwise or for a None entry.  Returns (flags, the new
    snp.allele)."""
    flags = np.full(len(snp_allele), NA_INTEGER, np.int32)
    new = []
    for i, (val, want) in enumerate(zip(snp_allele, a_allele)):
        val = str(val)
        if want is not None and not (isinstance(want, float) and want != want):
            p = val.find("/")
            a, b = (val, "") if p < 0 else (val[:p], val[p + 1:])
            if a == str(want):
                flags[i] = 0
            elif b == str(want):
                flags[i] = 1
        new.append(b + "/" + a if flags[i] == 1 else val)
    return flags, np.array(new)


def allele_switch(gdsobj, a_allele, verbose=True, device=0):
    if not isinstance(gdsobj, (GenoFile, GenoStream)):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    if isinstance(a_allele, str) or not all(x is None or isinstance(x, (str, np.str_, float)) for x in a_allele):
        raise TypeError("is.character(A.allele) is not TRUE")
    if gdsobj.snp_allele is None:
        raise ValueError("There is no allelic information in the GDS file (no 'snp.allele' variable).")
    if len(gdsobj.snp_allele) != len(a_allele):
        raise ValueError("The length of 'A.allele' should correspond to 'snp.allele' in the GDS file.")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    if not isinstance(gdsobj, GenoFile):
        raise ValueError("The GDS file should allow writing.")
    need_device("snpgdsAlleleSwitch")
    flags, new = switch_flags(gdsobj.snp_allele, a_allele)
    gdsobj.packed = merged_rows([(gdsobj.packed, gdsobj.n_samp, None, None, (flags == 1).astype(np.uint8))], gdsobj.n_snp, device)
    gdsobj.snp_allele = new
    if verbose:
        print("Strand-switching at %d SNP locus/loci." % int((flags == 1).sum()))
        print("Unable to determine switching at %d SNP locus/loci." % int((flags == NA_INTEGER).sum()))
    return flags
