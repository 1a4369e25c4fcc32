"""CPU tests of the restatement of the downhill-simplex and Jacquard IBD-MLE (tests/ibd_methods_ref.py) and of what the new
interfaces decide before any GPU call.  The vectorised restatement is pinned to scalar, loop-by-loop transcriptions of the reference's
routines (NM_Prepare / NM_LogLik / Simplex / SimplexMin, PrIBDTabJacq / EM_Jacq_Alg) on pairs with 1, 3, 4, 5 and 40 SNPs, missing
calls, frequencies 0, 1 and -1, duplicate samples, a sample whose two haplotypes are identical and a pair without a shared call, at
max_niter 0, 2 and 5 and the default.

The restatement sums a pair's log terms in numpy's order and the transcription in SNP order, so their objective values differ by
rounding (<~ 1e-15 relative at these sizes).  A walk is compared decision for decision where its decision margin exceeds
1e-11 max(|L|, 1), as the GPU test does; elsewhere its log-likelihood must be as good to 2 convtol."""
import math

import numpy as np
import pytest

import ibd_methods_ref as mref
import ibd_mle_ref as ref
import ibd_pairs_ref as pref
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import unpack_2bit_rows

SNP_COUNTS = (1, 3, 4, 5, 40)


def _small(m):
    n = 7
    g = unpack_2bit_rows(synth_hash_block_packed(n, 0, m, 3 + m, 0.1, 0, False), n).copy()
    g[:, 1] = g[:, 0]                                   # duplicates
    if m >= 4:
        g[: m // 2, 2] = 3                              # 2 and 3 share no called SNP
        g[m // 2:, 3] = 3
    else:
        g[:, 2] = 3
    rng = np.random.default_rng(m)
    g[:, 6] = np.where(g[:, 6] == 1, 2 * rng.integers(0, 2, m), g[:, 6])      # identical haplotypes: no heterozygous call
    af = rng.uniform(0.05, 0.95, m)
    if m >= 40:
        af[3], af[7], af[11] = 0.0, 1.0, -1.0           # unusable in both tables
    return g.astype(np.uint8), af


def _all_pairs(n):
    i, j = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]          # i == j and i > j included
    return i, j


@pytest.mark.parametrize("m", SNP_COUNTS)
@pytest.mark.parametrize("cc", [False, True])
def test_simplex_matches_transcription(m, cc):
    g, af = _small(m)
    n = g.shape[1]
    i, j = _all_pairs(n)
    afr = ref.init_afreq(g, af)
    e = ref.e_prib(afr)
    m0, m1 = pref.est_plink_kinship(*ref.ibs_counts(g, i, j), e, False)
    s0, s1 = pref.clamp_start(m0, m1)
    compared = 0
    for max_niter in (1000, 5, 2, 0):
        want = mref.simplex(ref.pr_table(g, i, j, afr), s0, s1, pref.RELTOL, max_niter, cc)
        for t in range(len(i)):
            k0, k1, nfunk, ll, margin = mref._simplex(g[:, i[t]], g[:, j[t]], afr, float(s0[t]), float(s1[t]), pref.RELTOL,
                                                      max_niter, cc)
            scale = max(abs(ll), 1.0)
            if min(margin, want["margin"][t]) > 1e-11 * scale:
                compared += 1
                assert want["nfunk"][t] == nfunk, (m, i[t], j[t], max_niter)
                assert abs(want["k0"][t] - k0) <= 1e-9 and abs(want["k1"][t] - k1) <= 1e-9
                assert abs(want["loglik"][t] - ll) <= 1e-9 * scale
            elif math.isnan(k0):
                assert np.isnan(want["k0"][t]) and np.isnan(want["k1"][t]) and want["nfunk"][t] == nfunk == 2
                assert want["loglik"][t] == ll == 0
            else:
                convtol = max(pref.RELTOL * (scale + pref.RELTOL), mref.DBL_EPSILON)
                assert abs(want["loglik"][t] - ll) <= 2 * convtol
            assert 2 <= nfunk and (nfunk <= max(max_niter, 2) + 3)
    assert compared >= len(i)                            # most walks are compared decision for decision


def test_simplex_no_shared_call_and_penalty():
    g, af = _small(40)
    afr = ref.init_afreq(g, af)
    pr = ref.pr_table(g, np.array([2, 0]), np.array([3, 4]), afr)
    # no shared call: NaN start values, three equal values -0.0, the walk stops at once; no candidate is taken (0 < 0 is false)
    for cc in (False, True):
        r = mref.simplex(pr, np.array([np.nan, 0.3]), np.array([np.nan, 0.3]), pref.RELTOL, 1000, cc)
        assert np.isnan(r["k0"][0]) and np.isnan(r["k1"][0]) and r["nfunk"][0] == 2 and r["loglik"][0] == 0
    # the objective: 1e30 outside the triangle and where an opposite-homozygote SNP meets k0 = 0 (d0 > 0, sum = 0)
    d = [a[1] for a in mref.nm_prepare(pr)]
    assert mref.nm_loglik(d, -1e-300, 0.5) == -math.inf and mref.nm_loglik(d, 0.5, 0.5 + 1e-15) == -math.inf
    a, b = g[:, 0], g[:, 4]
    opp = (np.abs(a.astype(int) - b.astype(int)) == 2) & (a < 3) & (b < 3) & (afr > 0) & (afr < 1)
    assert opp.any()
    assert mref.nm_loglik(d, 0.0, 0.5) == -math.inf and math.isfinite(mref.nm_loglik(d, 1e-300, 0.5))
    prn = [(x - z, y - z, z) for x, y, z in zip(*[t[1] for t in pr])]
    assert mref._nm_loglik(prn, 0.0, 0.5) == -math.inf
    assert abs(mref._nm_loglik(prn, 0.3, 0.4) - mref.nm_loglik(d, 0.3, 0.4)) <= 1e-12 * abs(mref.nm_loglik(d, 0.3, 0.4))
    # the start simplex keeps the reference's asymmetry: no "/ 2" in the second vertex's else branch
    p = mref.start_simplex(0.1, 0.7)
    assert p[0] == [0.1, 0.7]
    assert p[1] == [0.1, 0.7 - max(0.7 - (1 - 0.1) / 2, 1 - 0.1 - 0.7)]
    assert p[2] == [0.1 + max(0.1, (1 - 0.7) / 2 - 0.1) / 2, 0.7]
    p = mref.start_simplex(0.7, 0.1)
    assert p[1] == [0.7, 0.1 + max(0.1, (1 - 0.7) / 2 - 0.1) / 2]
    assert p[2] == [0.7 - max(0.7 - (1 - 0.1) / 2, 1 - 0.1 - 0.7) / 2, 0.1]


@pytest.mark.parametrize("m", SNP_COUNTS)
def test_jacquard_matches_transcription(m):
    g, af = _small(m)
    n = g.shape[1]
    i, j = _all_pairs(n)
    afr = ref.init_afreq(g, af)
    tab = mref.jacq_table(g, i, j, afr)
    for t in range(len(i)):
        rows = [mref._pr_tab_jacq(int(a), int(b), float(p)) for a, b, p in zip(g[:, i[t]], g[:, j[t]], afr)]
        assert np.array_equal(tab[:, t, :].T, np.array(rows).reshape(m, 9))
    for max_niter in (1000, 5, 2, 0):
        want = mref.jacquard(tab, max_niter, pref.RELTOL)
        for t in range(len(i)):
            rows = [mref._pr_tab_jacq(int(a), int(b), float(p)) for a, b, p in zip(g[:, i[t]], g[:, j[t]], afr)]
            D, ll, nit = mref._em_jacq(rows, max_niter, pref.RELTOL)
            firm = want["stop_margin"][t] > 1e-11 * max(abs(ll), 1.0)
            assert abs(want["niter"][t] - nit) <= (0 if firm else 1)
            if want["niter"][t] == nit:
                assert np.allclose(want["D"][:, t], D, rtol=0, atol=1e-10, equal_nan=True), (i[t], j[t], max_niter)
                assert pref._div(abs(want["loglik"][t] - ll), max(abs(ll), 1.0)) <= 1e-12 or (math.isnan(ll) and np.isnan(want["loglik"][t]))


def test_jacquard_skips_the_mm_mm_class():
    # PrIBDTabJacq's (MM, MM) entry has no break and falls through to the default: all nine probabilities are 0
    assert mref._pr_tab_jacq(2, 2, 0.3) == [0.0] * 9
    assert mref._pr_tab_jacq(0, 0, 0.3)[0] == 0.7 and mref._pr_tab_jacq(0, 0, 0.3)[8] == 0.7 * 0.7 * 0.7 * 0.7
    g = np.array([[2, 2], [0, 0], [1, 2], [2, 1], [0, 2], [2, 2]], np.uint8)
    af = np.array([0.3, 0.4, 0.5, 0.6, 0.2, 0.9])
    tab = mref.jacq_table(g, np.array([0]), np.array([1]), af)
    assert (tab[:, 0, 0] == 0).all() and (tab[:, 0, 5] == 0).all() and (tab[8, 0, 1:5] > 0).all()
    # so the EM does not see those SNPs: the result equals that of the four other SNPs alone
    a = mref.jacquard(tab)
    b = mref.jacquard(mref.jacq_table(g[1:5], np.array([0]), np.array([1]), af[1:5]))
    assert np.array_equal(a["D"], b["D"]) and np.array_equal(a["loglik"], b["loglik"]) and np.array_equal(a["niter"], b["niter"])
    # the table is not symmetric in the two samples: (j, i) exchanges D3 with D5 and D4 with D6
    g2, af2 = _small(40)
    i, j = np.triu_indices(g2.shape[1], 1)
    x = mref.jacquard_pairs(g2, i, j, af2)
    y = mref.jacquard_pairs(g2, j, i, af2)
    assert np.array_equal(x["niter"], y["niter"])
    assert np.allclose(mref.swap_samples(y["D"]), x["D"], rtol=0, atol=1e-12, equal_nan=True)
    assert not np.allclose(y["D"], x["D"], rtol=0, atol=1e-6, equal_nan=True)
    # the start values: D9 is the left-to-right chain
    D = mref.jacq_start(1)
    assert D[8, 0] == 1 - 0.01 - 0.01 - 0.01 - 0.01 - 0.01 - 0.01 - 0.01 - 0.01


def test_family_inputs_move_every_coefficient():
    p, g = mref.family_genotypes(1025)
    assert not (g[:, mref.INBRED] == 1).any() and np.array_equal(g[:, 3] == 3, g[:, 3] == 3)
    assert not (g[:, mref.INBRED2] == 1).any()
    i, j = mref.listed_pairs(1025, 16)
    r = mref.jacquard_pairs(g, i[:11], j[:11])
    D = r["D"]
    print(np.round(D.T, 3))
    assert (D.max(1) > 0.05).all()                                # each of D1 ... D8 is well above 0.01 at some listed relative
    assert D[0, 3] > 0.5                                          # the inbred sample with itself: D1
    assert D[1, 8] > 0.5                                          # two unrelated inbred samples: D2
    assert D[2, 9] > 0.05 and D[4, 10] > 0.05                     # an inbred parent and its child: D3, and D5 the other way round
    assert D[6, 2] + D[7, 2] > 0.5                                # full sibs: D7 + D8


def test_exports_and_argument_checks_before_the_gpu():
    for s in ("snpgpu_ibd_jacquard_pairs", "snpgpu_gnrIBD_MLE_PairsMethod"):
        assert s in _lib.EXPORTS
    assert callable(_lib.ibd_jacquard_pairs)
    ids = ["a", "b"]
    with pytest.raises(ValueError, match="should be one of"):
        api.snpgdsIBDMLEPairs(None, ids, ids, method="em")
    with pytest.raises(ValueError, match="should be one of"):
        api.snpgdsIBDMLEPairs(None, ids, ids, method="MoM")
    for method in ("EM", "downhill.simplex", "Jacquard"):
        with pytest.raises(TypeError, match="is.logical\\(kinship\\)"):
            api.snpgdsIBDMLEPairs(None, ids, ids, kinship=1, method=method)
        with pytest.raises(ValueError, match="same length"):
            api.snpgdsIBDMLEPairs(None, ids, ids[:1], method=method)
    # `method` is the last keyword: positional calls written before it keep their meaning
    import inspect
    assert list(inspect.signature(api.snpgdsIBDMLEPairs).parameters)[-1] == "method"
    # the old names refuse as before
    with pytest.raises(NotImplementedError, match="not built"):
        api.snpgdsPairIBD(np.array([0.0, 1, 2]), np.array([0.0, 1, 2]), np.array([0.2, 0.3, 0.4]), method="Jacquard")


def test_abi_refusals_before_a_device_is_touched():
    n, m = 5, 20
    p = synth_hash_block_packed(n, 0, m, 1, 0.0, 0, False)
    L = _lib.lib()
    i1 = np.zeros(1, np.int32)
    bad = np.array([5], np.int32)
    d, out = np.empty(8, np.float64), np.empty(1, np.float64)
    head = (_lib._ptr(p), m, n, _lib.GENO_PACKED2, _lib.HOST, None)
    # device 99 does not exist: a refusal that names the argument was made before any device call
    with pytest.raises(_lib.SnpGpuError, match="d is NULL"):
        _lib.check(L.snpgpu_ibd_jacquard_pairs(*head, _lib._ptr(i1), _lib._ptr(i1), 1, 10, 1e-8, None, None, None, None, _lib.HOST, 99))
    with pytest.raises(_lib.SnpGpuError, match="idx1 / idx2 is NULL"):
        _lib.check(L.snpgpu_ibd_jacquard_pairs(*head, None, _lib._ptr(i1), 1, 10, 1e-8, _lib._ptr(d), None, None, None, _lib.HOST, 99))
    with pytest.raises(_lib.SnpGpuError, match="n_pairs < 1"):
        _lib.check(L.snpgpu_ibd_jacquard_pairs(*head, _lib._ptr(i1), _lib._ptr(i1), 0, 10, 1e-8, _lib._ptr(d), None, None, None, _lib.HOST, 99))
    with pytest.raises(_lib.SnpGpuError, match="sample index 5 of pair 0 is out of range"):
        _lib.check(L.snpgpu_ibd_jacquard_pairs(*head, _lib._ptr(i1), _lib._ptr(bad), 1, 10, 1e-8, _lib._ptr(d), None, None, None, _lib.HOST,
                                               99))
    with pytest.raises(_lib.SnpGpuError, match="two samples"):
        _lib.check(L.snpgpu_ibd_jacquard_pairs(_lib._ptr(p), m, 1, _lib.GENO_PACKED2, _lib.HOST, None, _lib._ptr(i1), _lib._ptr(i1), 1, 10,
                                               1e-8, _lib._ptr(d), None, None, None, _lib.HOST, 99))
    with pytest.raises(_lib.SnpGpuError, match="invalid out_mem"):
        _lib.check(L.snpgpu_ibd_jacquard_pairs(*head, _lib._ptr(i1), _lib._ptr(i1), 1, 10, 1e-8, _lib._ptr(d), None, None, None, 7, 99))
    # snpgpu_ibd_mle_pairs: mode 2 passes the mode check (the next refusal is the index), any other mode is named
    tail = (10, 1e-8, 1, _lib._ptr(out), _lib._ptr(out), None, None, None, _lib.HOST, 99)
    with pytest.raises(_lib.SnpGpuError, match="out of range"):
        _lib.check(L.snpgpu_ibd_mle_pairs(*head, _lib._ptr(i1), _lib._ptr(bad), 1, 2, 0, *tail))
    with pytest.raises(_lib.SnpGpuError, match="invalid mode 3"):
        _lib.check(L.snpgpu_ibd_mle_pairs(*head, _lib._ptr(i1), _lib._ptr(i1), 1, 3, 0, *tail))
    with pytest.raises(_lib.SnpGpuError, match="invalid mode -1"):
        _lib.check(L.snpgpu_ibd_mle_pairs(*head, _lib._ptr(i1), _lib._ptr(i1), 1, -1, 0, *tail))
    # the working-space call: method, num.thread and coef before the working space is looked at
    ws = (10, 1e-8, 1)
    with pytest.raises(_lib.SnpGpuError, match="invalid method 3"):
        _lib.check(L.snpgpu_gnrIBD_MLE_PairsMethod(None, _lib._ptr(i1), _lib._ptr(i1), 1, 3, *ws, 1, 0, _lib._ptr(d), None, None, None))
    with pytest.raises(_lib.SnpGpuError, match="num.thread"):
        _lib.check(L.snpgpu_gnrIBD_MLE_PairsMethod(None, _lib._ptr(i1), _lib._ptr(i1), 1, 2, *ws, 0, 0, _lib._ptr(d), None, None, None))
    with pytest.raises(_lib.SnpGpuError, match="coef is NULL"):
        _lib.check(L.snpgpu_gnrIBD_MLE_PairsMethod(None, _lib._ptr(i1), _lib._ptr(i1), 1, 1, *ws, 1, 0, None, None, None, None))
    # the old working-space name refuses methods 1 and 2 as before
    with pytest.raises(_lib.SnpGpuError, match="not built"):
        _lib.check(L.snpgpu_gnrIBD_MLE(None, 0, 10, 1e-8, 1, 2, 1, 1, 0, _lib._ptr(out), _lib._ptr(out), None, None))


def test_margin_cap_of_the_gpu_inputs():
    """the GPU test allows 5 % of a case's pairs inside the decision margin 1e-11 |L|: on the restatement alone (start values from
    the restatement's own method of moments) the listed pairs of the M = 17 and M = 1 025 inputs stay well below it"""
    for m in (17, 1025):
        p, g = mref.family_genotypes(m)
        i, j = mref.listed_pairs(m, mref.N_SIMPLEX)
        af = ref.init_afreq(g)
        m0, m1 = pref.est_plink_kinship(*ref.ibs_counts(g, i, j), ref.e_prib(af), False)
        r = mref.simplex_pairs(g, i, j, m0, m1)
        inside = ~(r["margin"] > 1e-11 * np.abs(r["loglik"]))
        print("M = %d: %d of %d pairs inside the margin, mean nfunk %.1f" % (m, inside.sum(), len(i), r["nfunk"].mean()))
        assert inside.mean() <= 0.05
