"""GPU tests of snpgdsIBDMLE (method "EM") and snpgdsIBDMLELogLik against the numpy reference (tests/ibd_mle_ref.py): HapMap
through the API, edge shapes on synthetic data, known relationships, every log-likelihood form, sampled pairs at N = 2 000 and
the error paths."""
import numpy as np
import pytest

import ibd_mle_ref as ref
from input_forms import scramble_padding as _scramble_padding
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

pytestmark = pytest.mark.gpu


def _firm_shares(r):
    """(share of the non-NaN pairs with a firm stopping margin, share with a firm candidate gap), from the reference alone: what the
    comparison below does NOT mask.  A comparison that demands equality only where the reference is firm goes blind when few pairs are."""
    ok = ~np.isnan(r["k0"])
    scale = 1e-9 * np.abs(np.where(np.isfinite(r["loglik"]), r["loglik"], 0))
    n = max(int(ok.sum()), 1)
    return float(((r["stop_margin"] > scale) & ok).sum()) / n, float(((r["cand_gap"] > scale) & ok).sum()) / n


def _compare(k0, k1, niter, r, check_niter=True, min_firm_stop=None, min_firm_cand=None, what=""):
    """the pass criteria of the reference comparison, on the pairs (r['i'], r['j']) of full n x n results; min_firm_*: the least share
    of the non-NaN pairs whose stopping margin / candidate gap must be firm for the comparison to count"""
    i, j = r["i"], r["j"]
    g0, g1 = k0[i, j], k1[i, j]
    assert np.array_equal(np.isnan(g0), np.isnan(r["k0"])) and np.array_equal(np.isnan(g1), np.isnan(r["k1"]))
    scale = 1e-9 * np.abs(np.where(np.isfinite(r["loglik"]), r["loglik"], 0))
    firm_stop = r["stop_margin"] > scale
    firm_cand = r["cand_gap"] > scale
    share_stop, share_cand = _firm_shares(r)
    print("%s: firm stopping margin at %.4f of the %d non-NaN pairs, firm candidate gap at %.4f"
          % (what or "ibd_mle", share_stop, int((~np.isnan(r["k0"])).sum()), share_cand), flush=True)
    assert min_firm_stop is None or share_stop >= min_firm_stop, "niter is compared at %.4f of the pairs only" % share_stop
    assert min_firm_cand is None or share_cand >= min_firm_cand, "the coefficients are compared at %.4f of the pairs only" % share_cand
    if check_niter:
        gn = niter[i, j]
        bad = firm_stop & (gn != r["niter"])
        assert not bad.any(), "niter differs at %d pairs with a firm stopping margin" % bad.sum()
        assert (np.abs(gn - r["niter"]) <= 1).all()
        same = gn == r["niter"]
    else:
        same = np.ones(len(i), bool)
    d = np.maximum(np.abs(g0 - r["k0"]), np.abs(g1 - r["k1"]))
    d = np.where(np.isnan(d), 0, d)
    cmp = firm_cand
    assert (d[cmp & same] <= 1e-8).all(), "max |dk| %g where niter agrees" % d[cmp & same].max(initial=0)
    assert (d[cmp & ~same] <= 1e-5).all(), "max |dk| %g" % d[cmp & ~same].max(initial=0)
    # symmetric, 0 on the diagonal
    assert np.array_equal(k0, k0.T, equal_nan=True) and np.array_equal(k1, k1.T, equal_nan=True)
    assert (np.diag(k0) == 0).all() and (np.diag(k1) == 0).all()
    if niter is not None:
        assert np.array_equal(niter, niter.T) and (np.diag(niter) == 0).all()


# ---- 1. HapMap through the API ---------------------------------------------------------------------------------------------
def test_hapmap_api(hapmap):
    sid = hapmap.sample_id[:48]
    r = api.snpgdsIBDMLE(hapmap, sample_id=sid, kinship=True, verbose=False)
    assert r["k0"].shape == (48, 48) and r["niter"].dtype == np.int32
    rows = [np.nonzero(hapmap.snp_id == s)[0][0] for s in r["snp_id"]]
    g = unpack_2bit_rows(hapmap.packed[rows], hapmap.n_samp)[:, np.isin(hapmap.sample_id, sid)]
    want = ref.ibd_mle(g)
    af = want["afreq"].copy()
    af[af < 0] = np.nan
    assert np.array_equal(r["afreq"], af, equal_nan=True)
    _compare(r["k0"], r["k1"], r["niter"], want)
    assert np.array_equal(r["kinship"], 0.5 * (1 - r["k0"] - r["k1"]) + 0.25 * r["k1"], equal_nan=True)
    r2 = api.snpgdsIBDMLE(hapmap, sample_id=sid, out_num_iter=False, kinship_constraint=True, verbose=False)
    assert r2["niter"] is None and "kinship" not in r2
    assert np.array_equal(r2["k0"], r["k0"], equal_nan=True) and np.array_equal(r2["k1"], r["k1"], equal_nan=True)


# ---- 2. edge shapes on synthetic data --------------------------------------------------------------------------------------
CASES = [
    # n_samp, n_snp, missing, special allele_freq, max_niter, reltol, coeff_correct
    (2, 1, 0.0, False, 1000, None, True),
    (3, 15, 0.05, False, 1000, None, False),
    (63, 16, 0.3, True, 1000, None, True),
    (64, 17, 0.05, False, 0, None, True),
    (65, 1000, 0.05, False, 1000, 1e-4, True),
    (130, 1000, 0.0, False, 5, None, True),
    (130, 17, 0.3, True, 1000, None, False),
    (64, 1000, 0.3, True, 1000, 1e-4, True),
    # The two short cases at 30 % missing calls above leave a pair some eight SNPs: the likelihood is flat, the EM creeps towards
    # its limit at a linear rate close to 1 (median 54 / 43 iterations, some pairs 1000), and |L - L_old| then comes down on the
    # tolerance 1.5e-8 |L| in steps smaller than the firmness scale 1e-9 |L| -- some iterate lands within the scale of the
    # tolerance, and the stopping margin of 62 % / 57 % of the pairs is not firm (no seed changes that: 47 ... 71 % over four
    # seeds, from the reference alone).  Their niter is therefore compared at well under half of the pairs.  The same shapes and
    # inputs at reltol = 1e-6: the steps at the tolerance are 70 times the scale, 99.0 % / 98.6 % of the margins are firm, and the
    # EM still takes a median of 28 / 21 and up to 579 / 698 iterations.
    (63, 16, 0.3, True, 1000, 1e-6, True),
    (130, 17, 0.3, True, 1000, 1e-6, False),
]
# least share of firm stopping margins by case: 0.99 with 1000 SNPs, 0.90 for the two added cases (reference: 0.990, 0.986); the two
# short cases at the default tolerance are known to be mostly masked (reference: 0.381, 0.433) and state no floor
FIRM_STOP = {c: 0.99 for c in CASES if c[1] == 1000}
FIRM_STOP.update({c: 0.90 for c in CASES[-2:]})


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_edge_shapes(case):
    n, m, miss, special, max_niter, reltol, cc = case
    reltol = ref.RELTOL if reltol is None else reltol
    p = synth_hash_block_packed(n, 0, m, 11 + n + m, miss, 0, False)
    g = unpack_2bit_rows(p, n)
    af = None
    if special:
        af = np.random.default_rng(n).uniform(0.05, 0.95, m)
        af[:: 5][:4] = [np.nan, 0.0, 1.0, 1.5][: len(af[:: 5][:4])]
        if m > 12:
            af[12] = -0.2
    want = ref.ibd_mle(g, af, max_niter, reltol, cc)
    k0, k1, nit, gaf = _lib.ibd_mle(_scramble_padding(p, n), n, af, max_niter, reltol, cc)
    assert np.array_equal(gaf, want["afreq"])
    _compare(k0, k1, nit, want, min_firm_stop=FIRM_STOP.get(case), min_firm_cand=0.99, what="-".join(map(str, case)))


def test_all_missing_pair_and_duplicates():
    n, m = 6, 300
    p = synth_hash_block_packed(n, 0, m, 5, 0.05, 0, False)
    g = unpack_2bit_rows(p, n)
    g[:, 1] = g[:, 0]                    # duplicate samples
    g[: m // 2, 2] = 3                   # 2 and 3 share no called SNP
    g[m // 2:, 3] = 3
    want = ref.ibd_mle(g)
    k0, k1, nit, _ = _lib.ibd_mle(pack_2bit_rows(g), n)
    _compare(k0, k1, nit, want)
    assert np.isnan(k0[2, 3]) and nit[2, 3] == 0
    assert k0[0, 1] + k1[0, 1] <= 0.01


# ---- 3. known relationships (independent of the reference) -----------------------------------------------------------------
def test_known_relationships():
    rng = np.random.default_rng(2024)
    M = 20000
    p = rng.uniform(0.05, 0.95, M)

    def founder():
        return (rng.random((2, M)) < p).astype(np.uint8)

    def child(a, b):
        pick = lambda h: h[rng.integers(0, 2, M), np.arange(M)]
        return np.stack([pick(a), pick(b)])
    F = [founder() for _ in range(6)]
    O1, O2, H = child(F[0], F[1]), child(F[0], F[1]), child(F[0], F[2])
    samples = F + [O1, O2, H, F[3].copy()]
    g = np.stack([h.sum(0) for h in samples], 1).astype(np.uint8)          # [M][10]
    g[rng.random(M) < 0.01, 9] = 3
    # the frequencies are the simulation's: estimated from ten related samples they would bias every estimate
    k0, k1, nit, _ = _lib.ibd_mle(pack_2bit_rows(g), g.shape[1], allele_freq=p)
    near = lambda a, b, t0, t1, tol: abs(k0[a, b] - t0) <= tol and abs(k1[a, b] - t1) <= tol
    for a, b in ((0, 6), (1, 6), (0, 7), (1, 7), (0, 8), (2, 8)):
        assert near(a, b, 0, 1, 0.02), (a, b, k0[a, b], k1[a, b])             # parent - offspring
    assert near(6, 7, 0.25, 0.5, 0.05), (k0[6, 7], k1[6, 7])                  # full sibs
    for a, b in ((6, 8), (7, 8)):
        assert near(a, b, 0.5, 0.5, 0.06), (a, b, k0[a, b], k1[a, b])         # half sibs
    assert k0[3, 9] + k1[3, 9] <= 0.01                                         # duplicates
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 4), (4, 5), (3, 5), (1, 8)):
        assert k0[a, b] >= 0.9, (a, b, k0[a, b])                              # unrelated


# ---- 4. snpgdsIBDMLELogLik -------------------------------------------------------------------------------------------------
def test_loglik_forms(hapmap):
    sid = hapmap.sample_id[:24]
    r = api.snpgdsIBDMLE(hapmap, sample_id=sid, verbose=False)
    rows = [np.nonzero(hapmap.snp_id == s)[0][0] for s in r["snp_id"]]
    g = unpack_2bit_rows(hapmap.packed[rows], hapmap.n_samp)[:, np.isin(hapmap.sample_id, sid)]

    def check(got, want):
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        f = np.isfinite(want)
        assert np.isfinite(got[f]).all()
        np.testing.assert_allclose(got[f], want[f], rtol=1e-9, atol=0)
        assert np.array_equal(got, got.T)
    own = api.snpgdsIBDMLELogLik(hapmap, r)
    check(own, ref.loglik_matrix(g, r["afreq"], r["k0"], r["k1"]))
    for rel, ab in api.RELATEDNESS.items():
        if ab is not None:
            a, b = ab
            check(api.snpgdsIBDMLELogLik(hapmap, r, relatedness=rel), ref.loglik_matrix(g, r["afreq"], a, b))
    check(api.snpgdsIBDMLELogLik(hapmap, r, k0=0.3, k1=0.4), ref.loglik_matrix(g, r["afreq"], 0.3, 0.4))
    # the EM never lowers the likelihood: each pair's value at its MLE >= its value at the PLINK start
    af = ref.init_afreq(g, r["afreq"])
    i, j = np.triu_indices(len(sid), 1)
    s0, s1 = ref.plink_start(*ref.ibs_counts(g, i, j), ref.e_prib(af))
    start = ref.loglik(ref.pr_table(g, i, j, af), s0, s1)
    assert (own[i, j] >= start - 1e-9 * np.abs(start)).all()


# ---- 5. scale ----------------------------------------------------------------------------------------------------------------
def test_scale_sampled_pairs():
    torch = pytest.importorskip("torch")
    N, M = 2000, 20000
    rb = (N + 3) // 4
    geno = torch.empty(M * rb, dtype=torch.uint8, device="cuda")
    for i0 in range(0, M, 8192):
        _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, min(8192, M - i0), seed=99, missing=0.01, spectrum=0)
    torch.cuda.synchronize()
    k0, k1, nit, _ = _lib.ibd_mle(None, N, geno_dev_ptr=geno.data_ptr(), n_snp=M)
    assert not np.isnan(k0).any() and not np.isnan(k1).any()
    g = unpack_2bit_rows(geno.cpu().numpy().reshape(M, rb), N)
    rng = np.random.default_rng(5)
    i = np.concatenate([np.zeros(40, int), np.full(1, N - 2), np.arange(40, 80), rng.integers(0, N - 1, 119)])
    j = np.concatenate([np.arange(1, 41), np.full(1, N - 1), np.arange(41, 81), np.zeros(119, int)])
    j[-119:] = [rng.integers(a + 1, N) for a in i[-119:]]
    want = ref.ibd_mle(g, pairs=(i, j))
    _compare(k0, k1, nit, want)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_errors(hapmap):
    for m in ("Jacquard", "downhill.simplex"):
        with pytest.raises(NotImplementedError):
            api.snpgdsIBDMLE(hapmap, sample_id=hapmap.sample_id[:10], method=m, verbose=False)
    with pytest.raises(ValueError, match="two samples"):
        api.snpgdsIBDMLE(hapmap, sample_id=hapmap.sample_id[:1], verbose=False)
    with pytest.raises(Exception, match="SNP"):
        api.snpgdsIBDMLE(hapmap, sample_id=hapmap.sample_id[:10], maf=0.6, verbose=False)
    with pytest.raises(_lib.SnpGpuError, match="two samples"):
        _lib.ibd_mle(np.zeros((5, 1), np.uint8), 1)
    with pytest.raises(_lib.SnpGpuError, match="not built"):
        _lib.check(_lib.lib().snpgpu_gnrIBD_MLE(None, 0, 1000, 1e-8, 1, 2, 1, 1, 0, None, None, None, None))
