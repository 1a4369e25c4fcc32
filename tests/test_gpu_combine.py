"""snpgdsCombineGeno and snpgdsAlleleSwitch on the hapmap fixture: the data set split into objects that are put together again,
against the fixture's own genotypes and against the restatements of tests/geno_merge_ref.py at one byte per genotype."""
import os

import numpy as np
import pytest

import geno_merge_ref as R
from conftest import GOLDEN
from snprelate_amd import api
from snprelate_amd.gds import GenoFile, unpack_2bit_rows

pytestmark = pytest.mark.gpu

NA = R.NA
SNPS = np.arange(3500, 5500)                        # holds the fixture's one duplicated position (SNPs 4644 and 4645)
_CACHE = {}


def _hapmap():
    if not _CACHE:
        h = api.snpgdsOpen(os.path.join(GOLDEN, "hapmap_geno.gds"))
        _CACHE.update(h=h, codes=unpack_2bit_rows(h.packed, h.n_samp))
    return _CACHE["h"], _CACHE["codes"]


def _sub(samp, snp):
    """the samples `samp` and the SNPs `snp` (positions) of the fixture as an in-memory object of its own"""
    h, codes = _hapmap()
    samp, snp = np.asarray(samp), np.asarray(snp)
    g = GenoFile(genotype=codes[snp][:, samp], sample_id=h.sample_id[samp], snp_id=h.snp_id[snp], snp_chromosome=h.snp_chromosome[snp],
                 snp_position=h.snp_position[snp], snp_allele=h.snp_allele[snp], sample_annot={k: v[samp] for k, v in h.sample_annot.items()})
    g.snp_rs_id = h.snp_rs_id[snp]
    return g


def _codes(g):
    return unpack_2bit_rows(g.packed, g.n_samp)


def _lists(objs):
    return [dict(snp_id=o.snp_id, chromosome=o.snp_chromosome, position=o.snp_position, allele=o.snp_allele, afreq=R.allele_freq(_codes(o)))
            for o in objs]


def _two():
    """the first 140 samples with all of SNPS, and the other 139 with a permuted subset that leaves the duplicated position out"""
    rng = np.random.default_rng(1)
    pick = rng.permutation(SNPS[(SNPS != 4644) & (SNPS != 4645)])[:1300]
    return _sub(np.arange(140), SNPS), _sub(np.arange(140, 279), pick), pick


def test_switch_then_combine_reproduces_the_fixture(capsys):
    h, codes = _hapmap()
    a, b, pick = _two()
    before, alleles = b.packed.copy(), list(b.snp_allele)
    # a third of the SNPs are asked for their B allele, a few for neither (or nothing), the rest for their A allele
    want = []
    for i, al in enumerate(alleles):
        x, y = al.split("/")
        want.append(y if i % 3 == 0 else None if i % 50 == 1 else "N" if i % 50 == 2 else x)
    flags = api.snpgdsAlleleSwitch(b, want, verbose=True)
    rf, rn = R.switch_ref(alleles, want)
    out = capsys.readouterr().out
    assert flags.dtype == np.int32 and np.array_equal(flags, rf) and list(b.snp_allele) == rn
    assert (flags == 1).sum() == (1300 + 2) // 3 and (flags == NA).sum() == 35
    assert "Strand-switching at 434 SNP locus/loci.\n" in out and "Unable to determine switching at 35 SNP locus/loci.\n" in out
    sw = flags == 1
    assert all(n == al.split("/")[1] + "/" + al.split("/")[0] for n, al in zip(np.asarray(rn)[sw], np.asarray(alleles)[sw]))
    assert np.array_equal(_codes(b), np.where(sw[:, None], R.flip_codes(codes[pick][:, 140:]), codes[pick][:, 140:]))
    assert np.array_equal(b.packed[~sw], before[~sw]) and not np.array_equal(b.packed[sw], before[sw])

    # the switched object and the first one, put together: the fixture's genotypes at the common SNPs, in file 1's order
    m = api.snpgdsCombineGeno([a, b], same_strand=True, verbose=False)
    common = SNPS[np.isin(SNPS, pick)]
    assert m.n_samp == 279 and list(m.sample_id) == list(h.sample_id) and np.array_equal(m.snp_id, h.snp_id[common])
    assert np.array_equal(_codes(m), codes[common])
    assert list(m.snp_allele) == list(h.snp_allele[common]) and np.array_equal(m.snp_position, h.snp_position[common])
    assert list(m.snp_rs_id) == list(h.snp_rs_id[common]) and list(m.sample_annot["pop.group"]) == list(h.sample_annot["pop.group"])
    assert m.packed.shape == (len(common), 70) and (m.packed[:, -1] >> 6 == 3).all()                      # 279 samples: one padding code

    # the same pair counts as the fixture itself over those SNPs
    x = api.snpgdsIBSNum(m, verbose=False)
    y = api.snpgdsIBSNum(h, snp_id=h.snp_id[common], verbose=False)
    assert np.array_equal(x["snp_id"], y["snp_id"])
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(x[k], y[k])

    # switching back with the first alleles restores the bytes and the names
    back = api.snpgdsAlleleSwitch(b, [al.split("/")[0] for al in alleles], verbose=False)
    assert np.array_equal(back == 1, sw) and np.array_equal(b.packed, before) and list(b.snp_allele) == alleles


def test_combine_without_same_strand_equals_the_restatement(capsys):
    a, b, pick = _two()
    al = np.array(b.snp_allele)
    # file 2 names an eighth of its SNPs on the other strand, an eighth the other way round, an eighth both, a few with another allele
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for i in range(len(al)):
        x, y = al[i].split("/")
        if i % 8 == 1:
            al[i] = comp[x] + "/" + comp[y]
        elif i % 8 == 2:
            al[i] = y + "/" + x
        elif i % 8 == 3:
            al[i] = comp[y] + "/" + comp[x]
        elif i % 97 == 0:
            al[i] = x + "/N"
    b.snp_allele = al
    want = R.intersect_ref(_lists([a, b]), "position", True, False)
    lists = [api.snpgdsSNPList(o) for o in (a, b)]
    assert all(np.allclose(l["afreq"], r["afreq"], rtol=0, atol=1e-15, equal_nan=True) for l, r in zip(lists, _lists([a, b])))
    got = api.snpgdsSNPListIntersect(*lists, verbose=False)
    assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert set(np.unique(want["flag2"]).tolist()) >= {0, 1, 2, 3, 4, 5} and len(want["idx1"]) < 1300      # mismatches dropped
    m = api.snpgdsCombineGeno([a, b], verbose=True)
    out = capsys.readouterr().out
    assert np.array_equal(_codes(m), R.combine_snps_ref([_codes(a), _codes(b)], want))
    assert np.array_equal(m.snp_id, a.snp_id[want["idx1"]]) and list(m.snp_allele) == list(a.snp_allele[want["idx1"]])
    f = want["flag2"]
    assert "Concatenating samples (mapping to the first GDS file) ...\n" in out
    assert "    file 2: %d allele flips, %d ambiguous locus/loci\n" % ((f & 1).sum(), (f & 4).sum()) in out
    assert "        [flip on different strand]: %d\n" % (f == 3).sum() in out and "[mismatch]" not in out       # (dropped before)


def test_three_files_one_of_them_a_bed_stream():
    h, codes = _hapmap()
    bed = api.snpgdsOpenBED(*[os.path.join(GOLDEN, "plinkhapmap.%s.gz" % e) for e in ("bed", "fam", "bim")], verbose=False)
    rest = np.flatnonzero(~np.isin(h.sample_id, bed.sample_id))          # the BED file's 60 samples are the fixture's
    assert len(rest) == 219
    allsnp = np.arange(h.n_snp)
    a, c = _sub(rest[:100], allsnp), _sub(rest[100:], allsnp[::-1])
    objs = [a, bed, c]
    want = R.intersect_ref(_lists(objs), "position", True, False)
    assert 0 < len(want["idx1"]) <= 129 and (want["flag2"] & 1).any()
    m = api.snpgdsCombineGeno(objs, verbose=False)
    assert m.n_samp == 279 and list(m.sample_id) == list(a.sample_id) + list(bed.sample_id) + list(c.sample_id)
    assert np.array_equal(_codes(m), R.combine_snps_ref([_codes(o) for o in objs], want))
    assert sorted(m.sample_annot) == ["sex"] and len(m.sample_annot["sex"]) == 279                         # the column all three have


def test_common_samples_concatenate_the_snps(capsys):
    h, codes = _hapmap()
    samp2 = np.random.default_rng(2).permutation(279)[:200]
    a, b = _sub(np.arange(20, 270), np.arange(0, 700)), _sub(samp2, np.arange(5000, 5333))
    b.snp_rs_id = None
    m = api.snpgdsCombineGeno([a, b], verbose=True)
    assert "Concatenating SNPs ...\n" in capsys.readouterr().out
    common, want = R.combine_samples_ref([_codes(a), _codes(b)], [list(a.sample_id), list(b.sample_id)])
    assert 0 < len(common) < 200 and list(m.sample_id) == common
    assert np.array_equal(_codes(m), want) and m.packed.shape == (1033, (len(common) + 3) // 4)
    assert np.array_equal(m.snp_id, np.arange(1, 1034)) and np.array_equal(m.snp_position, np.concatenate([a.snp_position, b.snp_position]))
    assert list(m.snp_allele) == list(a.snp_allele) + list(b.snp_allele) and list(m.snp_rs_id) == list(a.snp_rs_id) + [""] * 333


def test_refusals():
    a, b = _sub(np.arange(10), np.arange(0, 50)), _sub(np.arange(10, 30), np.arange(50, 90))
    with pytest.raises(ValueError, match="There is no common SNP."):
        api.snpgdsCombineGeno([a, b], verbose=False)
    with pytest.raises(ValueError, match="length\\(gds.fn\\) >= 2L is not TRUE"):
        api.snpgdsCombineGeno([a], verbose=False)
    s = api.snpgdsOpen(os.path.join(GOLDEN, "hapmap_geno.gds"), stream=True)
    with pytest.raises(ValueError, match="The GDS file should allow writing."):
        api.snpgdsAlleleSwitch(s, [x.split("/")[0] for x in s.snp_allele], verbose=False)
