"""CPU tests of the listed-pairs IBD-MLE reference (tests/ibd_pairs_ref.py) and of what the three new API functions decide before
any GPU call: the vectorised additions (kinship constraint, log-likelihood after LOGLIK_ADJUST, start values only) are pinned to the
loop-by-loop transcriptions of gnrPairIBD and gnrPairIBDLogLik; snpgdsPairIBDMLELogLik, which is host code, is checked in full; and
every input of tests/test_gpu_ibd_pairs.py is shown to have no near-tie among the coeff.correct candidates, so that the GPU
comparison leaves no pair out."""
import math

import numpy as np
import pytest

import ibd_mle_ref as ref
import ibd_pairs_ref as pref
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import unpack_2bit_rows


def _small():
    n, m = 6, 40
    g = unpack_2bit_rows(synth_hash_block_packed(n, 0, m, 3, 0.1, 0, False), n)
    g[:, 1] = g[:, 0]                                   # duplicates
    g[: m // 2, 2] = 3                                  # 2 and 3 share no called SNP
    g[m // 2:, 3] = 3
    af = np.random.default_rng(1).uniform(0.05, 0.95, m)
    af[3], af[7] = 0.0, 1.0                             # kept by the R filter, unusable in PrIBDTable, counted by the IBS states
    return g, af


def _close(a, b, tol):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b or abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize("constraint", [False, True])
@pytest.mark.parametrize("cc", [False, True])
def test_vectorised_matches_transcription(constraint, cc):
    g, af = _small()
    n = g.shape[1]
    i, j = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]          # i == j and i > j included
    for max_niter in (1000, 3, 0):
        want = pref.ibd_mle_pairs(g, i, j, af, max_niter, pref.RELTOL, cc, 0, constraint)
        mom = pref.ibd_mle_pairs(g, i, j, af, mode=1, constraint=constraint)
        for t in range(len(i)):
            a, b = g[:, i[t]].astype(float), g[:, j[t]].astype(float)
            k0, k1, ll, nit = pref.pair_ibd(a, b, af, "EM", constraint, max_niter, pref.RELTOL, cc)
            # the sums run pairwise in numpy and in SNP order in the transcription
            assert _close(want["k0"][t], k0, 1e-10) and _close(want["k1"][t], k1, 1e-10), (i[t], j[t], want["k0"][t], k0)
            assert _close(want["loglik"][t], ll, 1e-12), (i[t], j[t], want["loglik"][t], ll)
            assert want["niter"][t] == nit
            m0, m1, mll, mnit = pref.pair_ibd(a, b, af, "MoM", constraint)
            assert _close(mom["k0"][t], m0, 0) and _close(mom["k1"][t], m1, 0) and math.isnan(mll) and mnit == 0
            assert np.isnan(mom["loglik"][t]) and mom["niter"][t] == 0
    assert np.isnan(want["k0"][2 * n + 3]) and want["niter"][2 * n + 3] == 0                    # no shared call


def test_additions_agree_with_ibd_mle_ref():
    g, af = _small()
    i, j = np.triu_indices(g.shape[1], 1)
    e = ref.e_prib(ref.init_afreq(g, af))
    cnt = ref.ibs_counts(g, i, j)
    s0, s1 = pref.clamp_start(*pref.est_plink_kinship(*cnt, e, False))
    r0, r1 = ref.plink_start(*cnt, e)
    assert np.array_equal(s0, r0, equal_nan=True) and np.array_equal(s1, r1, equal_nan=True)
    a = pref.ibd_mle_pairs(g, i, j, af)
    b = ref.ibd_mle(g, af, pairs=(i, j))
    for k in ("k0", "k1", "niter", "stop_margin", "cand_gap"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(a["loglik_em"], b["loglik"], equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert (a["loglik"] >= a["loglik_em"])[np.isfinite(a["loglik_em"])].all()
    # the constraint moves start values into the triangle pihat^2 >= k2 and nothing else
    c0, c1 = pref.est_plink_kinship(*cnt, e, True)
    u0, u1 = pref.est_plink_kinship(*cnt, e, False)
    ok = np.isfinite(u0)
    pihat = c1 / 2 + (1 - c0 - c1)
    assert (pihat[ok] ** 2 >= (1 - c0 - c1)[ok] - 1e-12).all()
    same = (u1 / 2 + (1 - u0 - u1)) ** 2 >= (1 - u0 - u1)
    assert np.array_equal(c0[ok & same], u0[ok & same]) and np.array_equal(c1[ok & same], u1[ok & same])
    # a repeated pair is computed once and spread
    r = pref.ibd_mle_pairs(g, [0, 4, 0], [5, 2, 5], af)
    assert r["k0"][0] == r["k0"][2] and r["niter"][0] == r["niter"][2]


def test_pair_loglik_host_function():
    g, af = _small()
    af = af.copy()
    af[11], af[12], af[13] = np.nan, 1.5, -0.2                         # dropped
    g1, g2 = g[:, 0].astype(float), g[:, 4].astype(float)
    g1[5], g2[6] = -1, np.nan                                          # missing
    for rel, ab in api.RELATEDNESS.items():
        k0, k1 = ab if ab is not None else (0.3, 0.45)
        got = api.snpgdsPairIBDMLELogLik(g1, g2, af, k0=0.3, k1=0.45, relatedness=rel, verbose=False)
        assert got == pref.pair_ibd_loglik(g1, g2, af, k0, k1), rel
        assert math.isfinite(got)                                      # sums <= 0 are skipped: never -Inf
    # against the vectorised EM_LogLik where that is finite
    keep = np.isfinite(af) & (af >= 0) & (af <= 1)
    gg = np.stack([np.where((g1 >= 0) & (g1 <= 2), g1, 3), np.where((g2 >= 0) & (g2 <= 2), g2, 3)], 1)[keep].astype(np.uint8)
    v = ref.loglik(ref.pr_table(gg, np.array([0]), np.array([1]), af[keep]), [0.3], [0.45])[0]
    assert abs(api.snpgdsPairIBDMLELogLik(g1, g2, af, 0.3, 0.45, verbose=False) - v) <= 1e-12 * abs(v)
    assert ref.loglik(ref.pr_table(gg, np.array([0]), np.array([1]), af[keep]), [0.0], [0.0])[0] == -np.inf


def test_argument_checks_before_the_gpu():
    ids = ["a", "b"]
    with pytest.raises(TypeError, match="is.logical\\(kinship\\)"):
        api.snpgdsIBDMLEPairs(None, ids, ids, kinship=1)
    with pytest.raises(TypeError, match="is.logical\\(coeff.correct\\)"):
        api.snpgdsIBDMLEPairs(None, ids, ids, coeff_correct="yes")
    with pytest.raises(TypeError, match="is.numeric\\(reltol\\)"):
        api.snpgdsIBDMLEPairs(None, ids, ids, reltol="1e-8")
    with pytest.raises(ValueError, match="same length"):
        api.snpgdsIBDMLEPairs(None, ids, ids[:1])
    with pytest.raises(ValueError, match="no pair"):
        api.snpgdsIBDMLEPairs(None, [], [])

    g, af = np.array([0.0, 1, 2]), np.array([0.2, 0.3, 0.4])
    with pytest.raises(TypeError, match="is.vector\\(geno1\\)"):
        api.snpgdsPairIBD(g.reshape(3, 1), g, af)
    with pytest.raises(TypeError, match="is.numeric\\(allele.freq\\)"):
        api.snpgdsPairIBD(g, g, ["a", "b", "c"])
    with pytest.raises(ValueError, match="length\\(geno1\\) == length\\(geno2\\)"):
        api.snpgdsPairIBD(g, g[:2], af)
    with pytest.raises(ValueError, match="length\\(geno1\\) == length\\(allele.freq\\)"):
        api.snpgdsPairIBD(g, g, af[:2])
    with pytest.raises(TypeError, match="is.logical\\(kinship.constraint\\)"):
        api.snpgdsPairIBD(g, g, af, kinship_constraint=0)
    with pytest.raises(ValueError, match="should be one of"):
        api.snpgdsPairIBD(g, g, af, method="em")
    for m in ("downhill.simplex", "Jacquard"):
        with pytest.raises(NotImplementedError, match="not built"):
            api.snpgdsPairIBD(g, g, af, method=m)

    with pytest.raises(TypeError, match="is.numeric\\(k0\\)"):
        api.snpgdsPairIBDMLELogLik(g, g, af, k0="0.5")
    with pytest.raises(TypeError, match="is.character"):
        api.snpgdsPairIBDMLELogLik(g, g, af, relatedness=1)
    with pytest.raises(ValueError, match="length"):
        api.snpgdsPairIBDMLELogLik(g, g[:2], af)


def test_exports():
    for s in ("snpgpu_ibd_mle_pairs", "snpgpu_ibd_mle_pairs_stats", "snpgpu_gnrIBD_MLE_Pairs"):
        assert s in _lib.EXPORTS
    import snprelate_amd
    for f in ("snpgdsIBDMLEPairs", "snpgdsPairIBD", "snpgdsPairIBDMLELogLik"):
        assert callable(getattr(snprelate_amd, f))


@pytest.mark.parametrize("case", pref.GPU_CASES, ids=["-".join(map(str, c)) for c in pref.GPU_CASES])
def test_gpu_inputs_have_firm_candidates(case):
    _, _, _, i1, i2, want = pref.case_inputs(case)
    assert len(i1) == pref.N_LISTED and (i1 == i2).any() and (i1 > i2).any()
    assert len(np.unique(i1 * pref.N_SAMP + i2)) < len(i1)                               # repeats
    assert not np.isnan(want["k0"]).any() and not np.isnan(want["k1"]).any()
    scale = 1e-9 * np.abs(np.where(np.isfinite(want["loglik_em"]), want["loglik_em"], 0))
    assert (want["cand_gap"] > scale).all()
