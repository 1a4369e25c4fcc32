"""CPU tests of snpgdsPairScore: exports, the two restatements of tests/pair_score_ref.py against each other, the host finaliser
snpgpu_pair_score_final on numpy tables against the loop form (bit for bit: every sum is an integer far below 2^53 and the
finaliser runs CalcAvgSD's fp64 operations one by one), and the refusals that need no device."""
import numpy as np
import pytest

import pair_score_ref as P
import snprelate_amd
from snprelate_amd import _lib, api

NEW_SYMBOLS = ("snpgpu_pair_tables", "snpgpu_pair_score_final", "snpgpu_pair_score_matrix", "snpgpu_gnrPairScore", "snpgpu_pair_stats")
CASES = [(m, d) for m in P.METHODS for d in (True, False)]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _input(n_samp, n_snp, n_pair, missing, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, (n_snp, n_samp)).astype(np.uint8)
    g[rng.random(g.shape) < missing] = 3
    idx1 = rng.permutation(n_samp)[:n_pair]
    idx2 = rng.permutation(n_samp)[:n_pair]
    if n_pair > 2:
        idx2[0] = idx1[0]                                            # a self pair (swap keeps idx2 free of duplicates)
        dup = np.flatnonzero(idx2[1:] == idx1[0]) + 1
        if len(dup):
            idx2[dup[0]] = rng.permutation(np.setdiff1d(np.arange(n_samp), idx2))[0]
    return g, idx1.astype(np.int32), idx2.astype(np.int32)


def _edge_input(seed=5):
    """12 samples, 40 SNPs, 9 pairs with: a self pair, samples in both lists, an all-missing SNP, an all-missing sample, a pair that
    is called together at one SNP only, a pair never called together, and a SNP at the gsum == n tie"""
    g, idx1, idx2 = _input(12, 40, 9, 0.15, seed)
    idx1 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.int32)
    idx2 = np.array([0, 2, 1, 9, 5, 4, 10, 11, 3], np.int32)
    g[7] = 3                                                         # all-missing SNP
    g[:, 11] = 3                                                     # all-missing sample: pair 7 has Num == 0
    g[:, 10] = 3
    g[3, 10] = 1                                                     # pair 6 (6, 10) is called together at SNP 3 only: Num == 1
    g[3, 6] = 2
    g[9] = 1                                                         # every called genotype 1: gsum == n, no flip
    g[9, 10:] = 3
    g[11] = [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 3, 3]                     # gsum < n: flipped
    g[12] = [2, 2, 2, 2, 1, 2, 2, 2, 2, 2, 3, 3]                     # gsum > n
    return g, idx1, idx2


def test_abi_exports():
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s), s
    assert callable(api.snpgdsPairScore) and snprelate_amd.snpgdsPairScore is api.snpgdsPairScore


@pytest.mark.parametrize("method,dosage", CASES)
def test_vectorised_equals_loop(method, dosage):
    for k, (n, m, npair, miss) in enumerate([(7, 23, 5, 0.2), (30, 17, 30, 0.05), (4, 9, 1, 0.4)]):
        g, idx1, idx2 = _input(n, m, npair, miss, seed=100 + k)
        for type in P.TYPES:
            assert _same(P.pair_score_ref(g, idx1, idx2, method, type, dosage), P.pair_score_loop(g, idx1, idx2, method, type, dosage)), \
                (method, dosage, type, k)
    g, idx1, idx2 = _edge_input()
    for type in P.TYPES:
        assert _same(P.pair_score_ref(g, idx1, idx2, method, type, dosage), P.pair_score_loop(g, idx1, idx2, method, type, dosage))


def test_edge_input_holds_its_cases():
    g, idx1, idx2 = _edge_input()
    _, _, num = P.pair_score_loop(g, idx1, idx2, "IBS", "per.pair")
    assert num[7] == 0 and num[6] == 1 and num[0] > 1
    _, _, flip = P.tables(g, idx1, idx2, True)
    assert flip[9] == 0 and flip[11] == 1 and flip[12] == 0
    r1, r2, _ = P.pair_codes(g, idx1, idx2, False)
    assert ((r1[9] < 3).sum() + (r2[9] < 3).sum()) == (np.where(r1[9] < 3, r1[9], 0).sum() + np.where(r2[9] < 3, r2[9], 0).sum()) > 0
    sums = [(P.pair_score_loop(g, idx1, idx2, m, "per.pair")[0] * P.pair_score_loop(g, idx1, idx2, m, "per.pair")[2])
            for m in ("GVH.major.only", "GVH.minor.only")]
    assert min(np.nanmin(s) for s in sums) < 0                       # a *.only pair whose Sum is negative
    assert (P.pair_score_loop(g, idx1, idx2, "GVH.minor.only", "matrix") == -1).any()


@pytest.mark.parametrize("method,dosage", CASES)
def test_host_finaliser_bit_for_bit(method, dosage):
    _, major = P.score_map(method, dosage)
    for g, idx1, idx2 in (_edge_input(), _input(40, 300, 25, 0.1, seed=9), _input(3, 2, 1, 0.0, seed=2)):
        pair_tab, snp_tab, flip = P.tables(g, idx1, idx2, major)
        got = _lib.pair_score_final(pair_tab, method, dosage)
        want = P.pair_score_loop(g, idx1, idx2, method, "per.pair", dosage)
        for a, b in zip(got, want):
            assert _same(a, b), (method, dosage)
        got = np.stack(_lib.pair_score_final(snp_tab, method, dosage, flip=flip))
        assert _same(got, P.pair_score_loop(g, idx1, idx2, method, "per.snp", dosage)), (method, dosage)
        if not major:                                                # the flip bytes are not read
            assert _same(np.stack(_lib.pair_score_final(snp_tab, method, dosage)), got)


def test_finaliser_large_counts():
    """counts of a 10^6-SNP data set: the sums stay integers below 2^53 and the result is CalcAvgSD of them"""
    tab = np.array([[[400000, 1, 7], [250000, 199999, 3], [0, 150000, 12345]]], np.int64)
    for method in P.METHODS:
        mp, _ = P.score_map(method, True)
        v = mp[:3, :3]
        want = P.calc_avg_sd(float((tab[0] * v).sum()), float((tab[0] * v * v).sum()), int(tab[0].sum()))
        got = _lib.pair_score_final(tab, method, True)
        assert got[0][0] == want[0] and got[1][0] == want[1] and got[2][0] == tab.sum()


def test_refusals_without_a_device(hapmap):
    sid = list(hapmap.sample_id[:6])
    with pytest.raises(ValueError, match=r"'sample1.id' has duplicated element\(s\)."):
        api.snpgdsPairScore(hapmap, [sid[0], sid[0]], sid[1:3], verbose=False)
    with pytest.raises(ValueError, match=r"'sample2.id' has duplicated element\(s\)."):
        api.snpgdsPairScore(hapmap, sid[1:3], [sid[0], sid[0]], verbose=False)
    with pytest.raises(ValueError, match=r"length\(sample1.id\) == length\(sample2.id\)"):
        api.snpgdsPairScore(hapmap, sid[:3], sid[3:5], verbose=False)
    with pytest.raises(ValueError, match="'output' should be NULL, if 'type' is not \"gds.file\"."):
        api.snpgdsPairScore(hapmap, sid[:3], sid[3:6], type="matrix", output="x.gds", verbose=False)
    with pytest.raises(ValueError, match="'method' should be one of"):
        api.snpgdsPairScore(hapmap, sid[:3], sid[3:6], method="IBD", verbose=False)
    with pytest.raises(ValueError, match="'type' should be one of"):
        api.snpgdsPairScore(hapmap, sid[:3], sid[3:6], type="per.sample", verbose=False)
    with pytest.raises(TypeError, match="is.logical"):
        api.snpgdsPairScore(hapmap, sid[:3], sid[3:6], dosage=1, verbose=False)
    with pytest.raises(TypeError, match="is.character"):
        api.snpgdsPairScore(hapmap, sid[:3], sid[3:6], type="gds.file", verbose=False)

    # the C ABI refuses before it asks for a device
    L = _lib.lib()
    g = np.zeros((4, 5), np.uint8)
    a, b = np.array([0, 1], np.int32), np.array([2, 5], np.int32)
    pt, st, fl, out = np.zeros(18, np.int64), np.zeros(64, np.int32), np.zeros(4, np.uint8), np.zeros(64, np.float64)
    P_, H = _lib._ptr, _lib.HOST

    def tables(i1, i2, n_pair, *outs):
        return L.snpgpu_pair_tables(P_(g), 4, 5, _lib.GENO_U8, H, P_(i1), P_(i2), n_pair, 0, *[P_(o) for o in outs], H, 0)

    assert tables(a, b, 2, pt, st, fl) == 1 and b"out of range" in L.snpgpu_last_error()
    assert tables(a, np.array([2, -1], np.int32), 2, pt, st, fl) == 1 and b"out of range" in L.snpgpu_last_error()
    assert tables(a, a, 0, pt, st, fl) == 1 and b"no pair" in L.snpgpu_last_error()
    assert tables(a, a, 2, None, None, None) == 1 and b"NULL" in L.snpgpu_last_error()
    assert tables(a, None, 2, pt, st, fl) == 1 and b"NULL" in L.snpgpu_last_error()

    def matrix(i2, n_pair, method, kind, o):
        return L.snpgpu_pair_score_matrix(P_(g), 4, 5, _lib.GENO_U8, H, P_(a), P_(i2), n_pair, method, 1, kind, P_(o), 0)

    assert matrix(a, 2, 8, 0, st) == 1 and b"Invalid 'method'." in L.snpgpu_last_error()
    assert matrix(a, 2, 1, 2, st) == 1 and b"element kind" in L.snpgpu_last_error()
    assert matrix(b, 2, 1, 0, st) == 1 and b"out of range" in L.snpgpu_last_error()
    assert matrix(a, 0, 1, 0, st) == 1 and b"no pair" in L.snpgpu_last_error()
    assert matrix(a, 2, 1, 0, None) == 1 and b"NULL" in L.snpgpu_last_error()

    assert L.snpgpu_pair_score_final(0, P_(pt), None, 2, 0, 1, P_(out)) == 1 and b"Invalid 'method'." in L.snpgpu_last_error()
    assert L.snpgpu_pair_score_final(2, P_(pt), None, 2, 1, 1, P_(out)) == 1 and b"table kind" in L.snpgpu_last_error()
    assert L.snpgpu_pair_score_final(0, P_(pt), None, 2, 1, 1, None) == 1 and b"NULL" in L.snpgpu_last_error()
    assert L.snpgpu_pair_score_final(1, P_(st), None, 4, 4, 1, P_(out)) == 1 and b"needs flip" in L.snpgpu_last_error()
    pt[3] = -1
    assert L.snpgpu_pair_score_final(0, P_(pt), None, 2, 1, 1, P_(out)) == 1 and b"negative" in L.snpgpu_last_error()
    assert L.snpgpu_pair_stats(None) == 1

    assert L.snpgpu_gnrPairScore(P_(a), P_(a), 2, b"IBD", b"per.pair", 1, 0, P_(out)) == 1 and b"Invalid 'method'." in L.snpgpu_last_error()
    assert L.snpgpu_gnrPairScore(P_(a), P_(a), 2, b"IBS", b"per.sample", 1, 0, P_(out)) == 1 and b"Invalid 'type'." in L.snpgpu_last_error()
    assert L.snpgpu_gnrPairScore(P_(a), P_(a), 2, b"IBS", b"per.pair", 1, 0, None) == 1 and b"NULL" in L.snpgpu_last_error()
    assert L.snpgpu_gnrPairScore(P_(a), P_(a), 0, b"IBS", b"per.pair", 1, 0, P_(out)) == 1 and b"no pair" in L.snpgpu_last_error()
