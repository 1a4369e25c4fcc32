"""numpy restatements for the merging of data sets, one byte per genotype and written from the semantics, not from the package:
snpgpu_geno_merge (include/snpgpu.h section 1o: unpack the bits of every part, select, flip, concatenate, pack with padding 3 --
the source layouts are those of geno_select_ref), the allele-strand rules of gnrAlleleStrand, snpgdsSNPListIntersect, the two
branches of snpgdsCombineGeno and the decision of snpgdsAlleleSwitch."""
import numpy as np

import geno_select_ref as S

NA = -2 ** 31


def unpack_ref(rows, n):
    """rows [L][ceil(n / 4)] -> codes [L][n]"""
    bits = np.unpackbits(np.ascontiguousarray(rows, dtype=np.uint8), axis=1, bitorder="little")
    return (bits[:, 0:2 * n:2] | (bits[:, 1:2 * n:2] << 1)).astype(np.uint8)


def flip_codes(g):
    """0 / 1 / 2 / 3 -> 2 / 1 / 0 / 3"""
    return np.array([2, 1, 0, 3], np.uint8)[g]


def merge_codes(parts):
    """parts: dicts with data, kw (the description of geno_select_ref.make_stream), samp_index, snp_index, flip.  Codes [L][N]."""
    cols = []
    for p in parts:
        kw = p["kw"]
        n_samp = kw["n_rows"] if kw["major"] else kw["n_cols"]
        g = unpack_ref(S.ref_of(p["data"], kw, p.get("samp_index"), p.get("snp_index")),
                       n_samp if p.get("samp_index") is None else len(p["samp_index"]))
        if p.get("flip") is not None:
            f = np.asarray(p["flip"]) != 0
            g = np.where(f[:, None], flip_codes(g), g)
        cols.append(g)
    return np.concatenate(cols, axis=1)


def merge_ref(parts):
    return S.pack_ref(merge_codes(parts))


# ---- gnrAlleleStrand ---------------------------------------------------------------------------------------------------------------
PAIR = {"A": "T", "T": "A", "C": "G", "G": "C"}


def two_alleles(text):
    cut = text.index("/") if "/" in text else (text.index(",") if "," in text else None)
    if cut is None:
        return text.upper(), ""
    return text[:cut].upper(), text[cut + 1:].upper()


def side(freq):
    return 0 if freq <= 0.5 else 1


def strand_flag(a1, a2, f1, f2, same_strand):
    """the flag of one SNP: file 1 has alleles a1 with frequency f1, the other file a2 with f2; None = mismatch"""
    r, d = two_alleles(a1), two_alleles(a2)
    if same_strand:
        return 0 if r == d else 1 if r == d[::-1] else None
    acgt = lambda x: x in PAIR                                  # noqa: E731
    flag, freq = None, False
    if r == d:
        flag, freq = 0, acgt(d[1]) and r[0] == PAIR[d[1]]
    elif r == d[::-1]:
        flag, freq = 1, acgt(d[0]) and r[0] == PAIR[d[0]]
    elif all(acgt(x) for x in r + d):
        if r == (PAIR[d[0]], PAIR[d[1]]):
            flag, freq = 2, r[0] == d[1]
        elif r == (PAIR[d[1]], PAIR[d[0]]):
            flag, freq = 3, r[0] == d[0]
    if flag is not None and freq:
        flag = (flag & 2) | 4 | (1 if side(f1) != side(f2) else 0)
    return flag


def strand_flags(al1, al2, af1, af2, same_strand=False):
    out = [strand_flag(a, b, f, g, same_strand) for a, b, f, g in zip(al1, al2, af1, af2)]
    return np.array([NA if x is None else x for x in out], np.int32)


# ---- snpgdsSNPListIntersect ----------------------------------------------------------------------------------------------------
def intersect_ref(lists, method="position", na_rm=True, same_strand=False):
    """lists: dicts with snp_id, chromosome, position, allele, afreq.  idx 0-based."""
    def key(l, i):
        k = "%s:%s" % (l["chromosome"][i], l["position"][i])
        return k if method == "position" else "%s:%s:%s" % (l["snp_id"][i], k, l["allele"][i])
    keys = [[key(l, i) for i in range(len(l["snp_id"]))] for l in lists]
    others, seen, common = [set(ks) for ks in keys[1:]], set(), []
    for k in keys[0]:
        if k not in seen and all(k in other for other in others):
            common.append(k)
        seen.add(k)
    rv = {"idx%d" % (i + 1): np.array([ks.index(k) for k in common], np.int32) for i, ks in enumerate(keys)}
    if method == "position":
        i1 = rv["idx1"]
        for i in range(1, len(lists)):
            ii = rv["idx%d" % (i + 1)]
            rv["flag%d" % (i + 1)] = strand_flags(np.asarray(lists[0]["allele"])[i1], np.asarray(lists[i]["allele"])[ii],
                                                  np.asarray(lists[0]["afreq"])[i1], np.asarray(lists[i]["afreq"])[ii], same_strand)
        if na_rm:
            keep = np.ones(len(common), bool)
            for i in range(1, len(lists)):
                keep &= rv["flag%d" % (i + 1)] != NA
            rv = {k: v[keep] for k, v in rv.items()}
    return rv


def allele_freq(g):
    """the frequency of the A allele per SNP of codes [L][n] (3 = missing), NaN without a called genotype"""
    ok = g < 3
    n = ok.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, (g * ok).sum(1) / (2.0 * n), np.nan)


# ---- snpgdsCombineGeno at a byte per genotype ----------------------------------------------------------------------------------
def combine_snps_ref(genos, snp):
    """branch 2: genos[i] codes [L_i][n_i]; snp from intersect_ref.  Codes [common][sum n_i]: file i's rows idx_i, 2 - g where bit 1
    of its flag is set, missing stays missing."""
    cols = []
    for i, g in enumerate(genos):
        x = g[snp["idx%d" % (i + 1)]]
        if i:
            f = snp["flag%d" % (i + 1)]
            x = np.where(((f != NA) & ((f & 1) == 1))[:, None], flip_codes(x), x)
        cols.append(x)
    return np.concatenate(cols, axis=1)


def combine_samples_ref(genos, sample_ids):
    """branch 1: the SNPs of every file one after the other over the samples common to all, in file 1's order"""
    common = [s for s in dict.fromkeys(sample_ids[0]) if all(s in ids for ids in sample_ids[1:])]
    rows = [g[:, [list(ids).index(s) for s in common]] for g, ids in zip(genos, sample_ids)]
    return common, np.concatenate(rows, axis=0)


def switch_ref(alleles, a_allele):
    """(flags, new alleles) of snpgdsAlleleSwitch"""
    flags, new = [], []
    for al, want in zip(alleles, a_allele):
        a, _, b = al.partition("/")
        f = NA if want is None else 0 if a == want else 1 if b == want else NA
        flags.append(f)
        new.append(b + "/" + a if f == 1 else al)
    return np.array(flags, np.int32), new
