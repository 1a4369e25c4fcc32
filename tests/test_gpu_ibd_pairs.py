"""GPU tests of snpgpu_ibd_mle_pairs (one wave per pair) and of snpgdsIBDMLEPairs / snpgdsPairIBD on top of it, against the numpy
restatement and the transcriptions of tests/ibd_pairs_ref.py and against the same entries of the matrix path (snpgpu_ibd_mle).

Pass criteria of a comparison (restated from test_gpu_ibd_mle, with the log-likelihood added): the NaN pattern is equal; niter
differs by at most 1 at any pair and at no more than 2 of a case's pairs; |dk| <= 1e-8 where niter agrees and <= 1e-5 otherwise;
the log-likelihood agrees to 1e-9 relative.  The CPU file shows that no listed pair of these inputs has a near-tie among the
coeff.correct candidates, so every pair is compared.  The bound of 2 on the niter differences: successive |dL| near the stop are
(1 - rho) tol >~ 1e-11 |L| apart and rounding differences are <~ 1e-14 |L|, a flip per pair has probability <~ 1e-3; the count of
the matrix kernel on the same pairs is printed beside it as the yardstick."""
import numpy as np
import pytest

import ibd_pairs_ref as pref
from input_forms import scramble_padding as _scramble_padding
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

pytestmark = pytest.mark.gpu

MAX_NITER_DIFFS = 2


def _compare(k0, k1, ll, nit, want, label=""):
    """the pass criteria; returns the number of pairs whose niter differs"""
    wk0, wk1, wn = want["k0"], want["k1"], want["niter"]
    assert np.array_equal(np.isnan(k0), np.isnan(wk0)) and np.array_equal(np.isnan(k1), np.isnan(wk1))
    dn = np.abs(nit.astype(np.int64) - wn)
    same = dn == 0
    d = np.maximum(np.abs(k0 - wk0), np.abs(k1 - wk1))
    d = np.where(np.isnan(d), 0, d)
    rel = np.zeros(len(k0))
    if ll is not None:
        wl = want["loglik"]
        fin = np.isfinite(wl)
        assert np.array_equal(ll[~fin], wl[~fin], equal_nan=True)
        rel[fin] = np.abs(ll[fin] - wl[fin]) / np.maximum(np.abs(wl[fin]), 1e-300)
        rel[fin & (ll == wl)] = 0
    print("%s: pairs %d, niter differs at %d (max %d), max |dk| %.3g (niter equal) %.3g (other), max rel dloglik %.3g"
          % (label, len(k0), int((~same).sum()), int(dn.max(initial=0)), d[same].max(initial=0), d[~same].max(initial=0),
             rel.max(initial=0)))
    assert (dn <= 1).all(), "niter differs by more than 1"
    assert (d[same] <= 1e-8).all(), "max |dk| %g where niter agrees" % d[same].max(initial=0)
    assert (d[~same] <= 1e-5).all(), "max |dk| %g" % d[~same].max(initial=0)
    assert (rel <= 1e-9).all(), "max relative loglik difference %g" % rel.max()
    return int((~same).sum())


# ---- 1. the lane-split sweep at its boundaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pref.GPU_CASES, ids=["-".join(map(str, c)) for c in pref.GPU_CASES])
def test_listed_pairs(case):
    m, miss, special, max_niter, reltol, cc = case
    reltol = pref.RELTOL if reltol is None else reltol
    p, g, af, i1, i2, want = pref.case_inputs(case)
    n = pref.N_SAMP
    k0, k1, ll, nit, gaf = _lib.ibd_mle_pairs(_scramble_padding(p, n), n, i1, i2, af, 0, False, max_niter, reltol, cc)
    assert np.array_equal(gaf, want["afreq"])
    diffs = _compare(k0, k1, ll, nit, want, "pairs kernel %s" % (case,))
    # the yardstick: the lane-per-pair kernel of the matrix path on the same pairs (its diagonal is 0 by definition: left out)
    M0, M1, MN, _ = _lib.ibd_mle(_scramble_padding(p, n), n, af, max_niter, reltol, cc)
    off = i1 != i2
    mat = int((MN[i1, i2][off] != want["niter"][off]).sum())
    print("niter differences against the restatement, case %s: pairs kernel %d of %d, matrix kernel %d of %d"
          % (case, diffs, len(i1), mat, int(off.sum())))
    assert diffs <= MAX_NITER_DIFFS
    # a pair listed twice has the same bits
    key = i1 * n + i2
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    for a in (k0, k1, ll, nit):
        assert np.array_equal(a, a[first][inv], equal_nan=True)


def test_all_pairs_against_matrix_path():
    n, m = 24, 1025
    p = synth_hash_block_packed(n, 0, m, 11 + n + m, 0.05, 0, False)
    i, j = np.triu_indices(n, 1)
    k0, k1, ll, nit, _ = _lib.ibd_mle_pairs(p, n, i, j)
    M0, M1, MN, _ = _lib.ibd_mle(p, n)
    want = dict(k0=M0[i, j], k1=M1[i, j], niter=MN[i, j])
    diffs = _compare(k0, k1, None, nit, want, "all pairs against snpgpu_ibd_mle")
    assert diffs <= MAX_NITER_DIFFS
    # (j, i) is the same pair: the likelihood table is symmetric in the two samples, term by term
    r0, r1, rl, rn, _ = _lib.ibd_mle_pairs(p, n, j, i)
    assert np.array_equal(r0, k0) and np.array_equal(r1, k1) and np.array_equal(rl, ll) and np.array_equal(rn, nit)


def test_queue_refill_and_determinism():
    n, m, P = 24, 33, 6000                     # more pairs than the 16 waves x 256 CUs launched: every wave refills
    p = synth_hash_block_packed(n, 0, m, 11 + n + m, 0.05, 0, False)
    g = unpack_2bit_rows(p, n)
    rng = np.random.default_rng(m)
    i1, i2 = rng.integers(0, n, P), rng.integers(0, n, P)
    key, first, inv = np.unique(i1 * n + i2, return_index=True, return_inverse=True)
    want = pref.ibd_mle_pairs(g, i1[first], i2[first])
    assert (want["cand_gap"] > 1e-9 * np.abs(want["loglik_em"])).all()            # no near-tie: every distinct pair is compared
    a = _lib.ibd_mle_pairs(p, n, i1, i2)
    b = _lib.ibd_mle_pairs(p, n, i1, i2)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y, equal_nan=True)                              # a second call: the same bits
        assert np.array_equal(x, x[first][inv], equal_nan=True)                  # every repeat: the bits of its first occurrence
    diffs = _compare(a[0][first], a[1][first], a[2][first], a[3][first], want, "queue refill, %d distinct pairs" % len(first))
    assert diffs <= MAX_NITER_DIFFS * -(-len(first) // pref.N_LISTED)          # the bound per 200 pairs
    ms_em, ms_all, sweeps, pairs = _lib.ibd_mle_pairs_stats()
    assert pairs == P and sweeps >= P and 0 < ms_em <= ms_all


def test_no_shared_call_duplicates_and_start_values():
    n, m = 6, 300
    p = synth_hash_block_packed(n, 0, m, 5, 0.05, 0, False)
    g = unpack_2bit_rows(p, n)
    g[:, 1] = g[:, 0]                    # duplicate samples
    g[: m // 2, 2] = 3                   # 2 and 3 share no called SNP
    g[m // 2:, 3] = 3
    i1, i2 = np.array([2, 0, 3, 4, 5, 1]), np.array([3, 1, 2, 5, 5, 4])
    k0, k1, ll, nit, _ = _lib.ibd_mle_pairs(pack_2bit_rows(g), n, i1, i2)
    assert np.isnan(k0[0]) and np.isnan(k1[0]) and nit[0] == 0 and np.isnan(k0[2]) and nit[2] == 0
    assert k0[1] + k1[1] <= 0.01
    want = pref.ibd_mle_pairs(g, i1, i2)
    _compare(k0, k1, ll, nit, want, "edge pairs")
    # mode 1: the method of moments before the clamp, with and without the constraint of Est_PLINK_Kinship
    for constraint in (False, True):
        w = pref.ibd_mle_pairs(g, i1, i2, mode=1, constraint=constraint)
        s0, s1, sl, sn, _ = _lib.ibd_mle_pairs(pack_2bit_rows(g), n, i1, i2, mode=1, kinship_constraint=constraint)
        assert np.isnan(sl).all() and (sn == 0).all()
        # a few ulps of values in [0, 1]: the device may fuse a multiply-add that numpy rounds twice
        np.testing.assert_allclose(s0, w["k0"], rtol=0, atol=1e-13)
        np.testing.assert_allclose(s1, w["k1"], rtol=0, atol=1e-13)


def test_device_input_equals_host_input():
    torch = pytest.importorskip("torch")
    case = pref.GPU_CASES[6]
    p, g, af, i1, i2, want = pref.case_inputs(case)
    n = pref.N_SAMP
    host = _lib.ibd_mle_pairs(p, n, i1, i2)
    dev = torch.from_numpy(np.ascontiguousarray(p)).cuda()
    torch.cuda.synchronize()
    got = _lib.ibd_mle_pairs(None, n, i1, i2, geno_dev_ptr=dev.data_ptr(), n_snp=p.shape[0])
    for x, y in zip(host, got):
        assert np.array_equal(x, y, equal_nan=True)


# ---- 2. the API -------------------------------------------------------------------------------------------------------------
def test_hapmap_api(hapmap):
    sid = hapmap.sample_id[:48]
    rng = np.random.default_rng(48)
    a, b = rng.integers(0, 48, 60), rng.integers(0, 48, 60)
    b[b == a] = (a[b == a] + 1) % 48                                          # off the diagonal: the matrix path has 0 there
    r = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, kinship=True, verbose=False)
    assert r["k0"].shape == (60,) and r["niter"].dtype == np.int32 and np.array_equal(r["ID1"], sid[a])
    rows = [np.nonzero(hapmap.snp_id == s)[0][0] for s in r["snp_id"]]
    g = unpack_2bit_rows(hapmap.packed[rows], hapmap.n_samp)[:, np.isin(hapmap.sample_id, sid)]
    pos = {s: t for t, s in enumerate(r["sample_id"])}
    i = np.array([pos[s] for s in sid[a]])
    j = np.array([pos[s] for s in sid[b]])
    want = pref.ibd_mle_pairs(g, i, j)
    assert (want["cand_gap"] > 1e-9 * np.abs(want["loglik_em"])).all()
    af = want["afreq"].copy()
    af[af < 0] = np.nan
    assert np.array_equal(r["afreq"], af, equal_nan=True)
    assert _compare(r["k0"], r["k1"], r["loglik"], r["niter"], want, "HapMap against the restatement") <= MAX_NITER_DIFFS
    assert np.array_equal(r["kinship"], 0.5 * (1 - r["k0"] - r["k1"]) + 0.25 * r["k1"], equal_nan=True)
    full = api.snpgdsIBDMLE(hapmap, sample_id=sid, verbose=False)
    assert np.array_equal(full["sample_id"], r["sample_id"]) and np.array_equal(full["snp_id"], r["snp_id"])
    mat = dict(k0=full["k0"][i, j], k1=full["k1"][i, j], niter=full["niter"][i, j])
    assert _compare(r["k0"], r["k1"], None, r["niter"], mat, "HapMap against snpgdsIBDMLE") <= MAX_NITER_DIFFS
    r2 = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, out_num_iter=False, kinship_constraint=True, verbose=False)
    assert r2["niter"] is None and "kinship" not in r2
    assert np.array_equal(r2["k0"], r["k0"], equal_nan=True) and np.array_equal(r2["loglik"], r["loglik"], equal_nan=True)
    with pytest.raises(ValueError, match="no-such-sample"):
        api.snpgdsIBDMLEPairs(hapmap, [sid[0], "no-such-sample"], [sid[1], sid[2]], sample_id=sid, verbose=False)
    with pytest.raises(ValueError, match="sample2.id"):
        api.snpgdsIBDMLEPairs(hapmap, [sid[0]], [hapmap.sample_id[60]], sample_id=sid, verbose=False)


def test_pair_ibd(hapmap):
    L = 1500
    g = unpack_2bit_rows(hapmap.packed[:L], hapmap.n_samp)
    g1, g2 = g[:, 1].astype(np.float64), g[:, 2].astype(np.float64)
    called = g < 3
    af = np.where(called, g, 0).sum(1) / np.maximum(2 * called.sum(1), 1)
    g1[g1 == 3] = np.nan                          # NA
    g1[10], g2[11], g2[12] = -1, 7, np.nan        # codes outside 0..2 are missing
    af[20], af[21], af[22] = np.nan, 1.5, -0.2    # dropped loci
    for method in ("EM", "MoM"):
        for constraint in (False, True):
            want = pref.pair_ibd(g1, g2, af, method, constraint)
            r = api.snpgdsPairIBD(g1, g2, af, method=method, kinship_constraint=constraint, verbose=False)
            print(method, constraint, r, want)
            if method == "MoM":
                assert abs(r["k0"] - want[0]) <= 1e-13 and abs(r["k1"] - want[1]) <= 1e-13
                assert np.isnan(r["loglik"]) and r["niter"] == 0
            else:
                assert abs(r["niter"] - want[3]) <= 1
                tol = 1e-8 if r["niter"] == want[3] else 1e-5
                assert abs(r["k0"] - want[0]) <= tol and abs(r["k1"] - want[1]) <= tol
                assert abs(r["loglik"] - want[2]) <= 1e-9 * abs(want[2])
    # few iterations, no coeff.correct, no niter column
    want = pref.pair_ibd(g1, g2, af, "EM", False, 3, 1e-4, False)
    r = api.snpgdsPairIBD(g1, g2, af, max_niter=3, reltol=1e-4, coeff_correct=False, out_num_iter=False, verbose=False)
    assert "niter" not in r and abs(r["k0"] - want[0]) <= 1e-8 and abs(r["k1"] - want[1]) <= 1e-8
    assert abs(r["loglik"] - want[2]) <= 1e-9 * abs(want[2])
    # the constraint acts here: this pair's start values lie outside the triangle and are moved
    assert pref.pair_ibd(g1, g2, af, "MoM", True)[:2] != pref.pair_ibd(g1, g2, af, "MoM", False)[:2]


# ---- 3. errors of the ABI ---------------------------------------------------------------------------------------------------
def test_abi_errors():
    n, m = 5, 20
    p = synth_hash_block_packed(n, 0, m, 1, 0.0, 0, False)
    with pytest.raises(_lib.SnpGpuError, match="out of range"):
        _lib.ibd_mle_pairs(p, n, [0, 5], [1, 2])
    with pytest.raises(_lib.SnpGpuError, match="out of range"):
        _lib.ibd_mle_pairs(p, n, [0, 1], [1, -1])
    with pytest.raises(_lib.SnpGpuError, match="n_pairs < 1"):
        _lib.ibd_mle_pairs(p, n, [], [])
    with pytest.raises(_lib.SnpGpuError, match="two samples"):
        _lib.ibd_mle_pairs(np.zeros((5, 1), np.uint8), 1, [0], [0])
    L = _lib.lib()
    i1 = np.zeros(1, np.int32)
    out = np.empty(1, np.float64)
    args = (_lib._ptr(p), m, n, _lib.GENO_PACKED2, _lib.HOST, None, _lib._ptr(i1), _lib._ptr(i1), 1, 0, 0, 10, 1e-8, 1)
    with pytest.raises(_lib.SnpGpuError, match="k0 / k1 is NULL"):
        _lib.check(L.snpgpu_ibd_mle_pairs(*args, None, _lib._ptr(out), None, None, None, _lib.HOST, 0))
    with pytest.raises(_lib.SnpGpuError, match="idx1 / idx2 is NULL"):
        _lib.check(L.snpgpu_ibd_mle_pairs(*args[:6], None, _lib._ptr(i1), *args[8:], _lib._ptr(out), _lib._ptr(out), None, None, None,
                                          _lib.HOST, 0))
    with pytest.raises(_lib.SnpGpuError, match="stats is NULL"):
        _lib.check(L.snpgpu_ibd_mle_pairs_stats(None))
    # loglik and niter may be NULL
    k0, k1 = np.empty(1, np.float64), np.empty(1, np.float64)
    _lib.check(L.snpgpu_ibd_mle_pairs(*args, _lib._ptr(k0), _lib._ptr(k1), None, None, None, _lib.HOST, 0))
    full = _lib.ibd_mle_pairs(p, n, [0], [0], max_niter=10, reltol=1e-8)
    assert k0[0] == full[0][0] and k1[0] == full[1][0]
    with pytest.raises(_lib.SnpGpuError, match="num.thread"):
        _lib.check(L.snpgpu_gnrIBD_MLE_Pairs(None, _lib._ptr(i1), _lib._ptr(i1), 1, 10, 1e-8, 1, 0, 0, _lib._ptr(k0), _lib._ptr(k1),
                                             None, None, None))
