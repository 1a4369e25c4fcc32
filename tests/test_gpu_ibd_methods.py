"""GPU tests of the downhill-simplex and Jacquard IBD-MLE of listed pairs (ibd_nm_pairs_kernel, ibd_jacq_pairs_kernel; one wave per
pair) and of snpgdsIBDMLEPairs(method=...) / snpgpu_gnrIBD_MLE_PairsMethod on top of them, against tests/ibd_methods_ref.py.

Simplex.  The restatement starts from the GPU's own method-of-moments values (mode 1 of snpgpu_ibd_mle_pairs, tested in
test_gpu_ibd_pairs), so both walk from the same bits; the simplex geometry is the same fp64 sequence on both sides and the
objective differs by rounding only.  A pair whose decision margin (ibd_methods_ref) exceeds 1e-11 |L| must therefore make the same
decisions: the same nfunk, |dk0|, |dk1| <= 1e-9 (the vertices are affine in the start vertices with coefficients that grow at most
linearly in the iteration count; ~1e-15 is expected and the maximum is printed) and the log-likelihood to 1e-9 relative.  1e-11 is two
orders above the worst log-likelihood disagreement DESIGN.md 12a records for these sweeps (7.1e-14).  A pair inside the margin must
reach a log-likelihood >= the restatement's - 2 convtol, and at most 5 % of a case's pairs may lie inside.

Jacquard.  The rules of test_gpu_ibd_pairs._compare per coefficient: niter differs by at most 1, at no more than 2 pairs of a case;
|dD| <= 1e-8 where niter agrees and <= 1e-5 otherwise; the log-likelihood to 1e-9 relative."""
import numpy as np
import pytest

import ibd_methods_ref as mref
import ibd_pairs_ref as pref
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

pytestmark = pytest.mark.gpu

MAX_NITER_DIFFS = 2
MARGIN = 1e-11
MAX_INSIDE = 0.05
# ... of the non-NaN pairs: what the comparison masks.  The restatement's own figure, from CPU method-of-moments starts
# (tests/ibd_pairs_ref.py, mode 1) over SIMPLEX_CASES: 0, 1, 1, 1, 0, 0, 0, 0, 2 and 2 of 200 pairs, at most 0.010 of a case.


def _compare_simplex(k0, k1, ll, nit, want, reltol, label=""):
    """the pass criteria of a simplex comparison; returns the fraction of the non-NaN pairs inside the margin"""
    wl = want["loglik"]
    assert np.array_equal(np.isnan(k0), np.isnan(want["k0"])) and np.array_equal(np.isnan(k1), np.isnan(want["k1"]))
    nan = np.isnan(want["k0"])
    assert (nit[nan] == 2).all() and (ll[nan] == 0).all() and (want["nfunk"][nan] == 2).all() and (wl[nan] == 0).all()
    firm = (want["margin"] > MARGIN * np.abs(wl)) & ~nan
    loose = ~firm & ~nan
    dk = np.maximum(np.abs(k0 - want["k0"]), np.abs(k1 - want["k1"]))
    rel = np.abs(ll - wl) / np.maximum(np.abs(wl), 1e-300)
    rel[ll == wl] = 0
    print("%s: pairs %d, inside the margin %d, nfunk differs at %d firm pairs, max |dk| %.3g, max rel dloglik %.3g (firm pairs), mean nfunk %.1f"
          % (label, len(k0), int(loose.sum()), int((nit[firm] != want["nfunk"][firm]).sum()), dk[firm].max(initial=0),
             rel[firm].max(initial=0), nit.mean()))
    assert np.array_equal(nit[firm], want["nfunk"][firm]), "nfunk differs at a pair outside the margin"
    assert (dk[firm] <= 1e-9).all(), "max |dk| %g" % dk[firm].max(initial=0)
    assert (rel[firm] <= 1e-9).all(), "max relative loglik difference %g" % rel[firm].max(initial=0)
    convtol = np.maximum(reltol * (np.abs(wl) + abs(reltol)), mref.DBL_EPSILON)      # |y[0]| ~ |L|: the stop test's own scale
    assert (ll[loose] >= wl[loose] - 2 * convtol[loose]).all()
    inside = float(loose.sum()) / max(int((~nan).sum()), 1)
    print("%s: decision margin firm at %.4f of the %d non-NaN pairs (cap on the rest: %.2f)" % (label, 1 - inside, int((~nan).sum()), MAX_INSIDE))
    return inside


def _compare_jacquard(D, ll, nit, want, label=""):
    """_compare of test_gpu_ibd_pairs per coefficient; returns the number of pairs whose niter differs"""
    wD, wn, wl = want["D"], want["niter"], want["loglik"]
    assert np.array_equal(np.isnan(D), np.isnan(wD))
    dn = np.abs(nit.astype(np.int64) - wn)
    same = dn == 0
    d = np.where(np.isnan(wD), 0, np.abs(D - wD)).max(0)
    fin = np.isfinite(wl)
    assert np.array_equal(ll[~fin], wl[~fin], equal_nan=True)
    rel = np.zeros(len(ll))
    rel[fin] = np.abs(ll[fin] - wl[fin]) / np.maximum(np.abs(wl[fin]), 1e-300)
    rel[fin & (ll == wl)] = 0
    print("%s: pairs %d, niter differs at %d (max %d), max |dD| %.3g (niter equal) %.3g (other), max rel dloglik %.3g, mean niter %.1f"
          % (label, len(ll), int((~same).sum()), int(dn.max(initial=0)), d[same].max(initial=0), d[~same].max(initial=0),
             rel.max(initial=0), nit.mean()))
    assert (dn <= 1).all(), "niter differs by more than 1"
    assert (d[same] <= 1e-8).all(), "max |dD| %g where niter agrees" % d[same].max(initial=0)
    assert (d[~same] <= 1e-5).all(), "max |dD| %g" % d[~same].max(initial=0)
    assert (rel <= 1e-9).all(), "max relative loglik difference %g" % rel.max()
    return int((~same).sum())


def _simplex_want(p, g, n, i1, i2, af, max_niter, reltol, cc):
    """the restatement's walk from the GPU's own start values"""
    s0, s1, sl, sn, _ = _lib.ibd_mle_pairs(p, n, i1, i2, af, mode=1)
    return mref.simplex_pairs(g, i1, i2, s0, s1, af, max_niter, reltol, cc)


# ---- 1. simplex against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mref.SIMPLEX_CASES, ids=["-".join(map(str, c)) for c in mref.SIMPLEX_CASES])
def test_simplex(case):
    m, special, max_niter, reltol, cc = case
    reltol = pref.RELTOL if reltol is None else reltol
    n = pref.N_SAMP
    p, g = mref.family_genotypes(m)
    af = mref.special_freq(m) if special else None
    i1, i2 = mref.listed_pairs(m, mref.N_SIMPLEX)
    want = _simplex_want(p, g, n, i1, i2, af, max_niter, reltol, cc)
    k0, k1, ll, nit, gaf = _lib.ibd_mle_pairs(p, n, i1, i2, af, 2, False, max_niter, reltol, cc)
    assert np.array_equal(gaf, want["afreq"])
    inside = _compare_simplex(k0, k1, ll, nit, want, reltol, "simplex %s" % (case,))
    assert inside <= MAX_INSIDE
    if max_niter == 0:
        assert (nit == 2).all()
    # a pair listed twice has the same bits
    _, first, inv = np.unique(i1 * n + i2, return_index=True, return_inverse=True)
    for a in (k0, k1, ll, nit):
        assert np.array_equal(a, a[first][inv], equal_nan=True)


# ---- 2. Jacquard against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mref.JACQUARD_CASES, ids=["-".join(map(str, c)) for c in mref.JACQUARD_CASES])
def test_jacquard(case):
    m, special, max_niter, reltol = case
    reltol = pref.RELTOL if reltol is None else reltol
    n = pref.N_SAMP
    p, g = mref.family_genotypes(m)
    af = mref.special_freq(m) if special else None
    i1, i2 = mref.listed_pairs(m, mref.n_jacquard(m))
    want = mref.jacquard_pairs(g, i1, i2, af, max_niter, reltol)
    D, ll, nit, gaf = _lib.ibd_jacquard_pairs(p, n, i1, i2, af, max_niter, reltol)
    assert np.array_equal(gaf, want["afreq"])
    assert _compare_jacquard(D, ll, nit, want, "Jacquard %s" % (case,)) <= MAX_NITER_DIFFS
    if m >= 1023 and max_niter == 1000:
        assert (D.max(1) > 0.05).all()                       # the listed relatives move every one of D1 ... D8
    _, first, inv = np.unique(i1 * n + i2, return_index=True, return_inverse=True)
    for a in (D.T, ll, nit):
        assert np.array_equal(a, a[first][inv], equal_nan=True)


# ---- 3. further checks for both methods ------------------------------------------------------------------------------------------------
def test_swapped_pairs():
    n, m = pref.N_SAMP, 1025
    p, g = mref.family_genotypes(m)
    i, j = np.triu_indices(n, 1)
    i, j = i[::3], j[::3]
    # simplex: PrIBDTable and ibd_terms are symmetric in the two samples term by term, so (j, i) has the same bits
    a = _lib.ibd_mle_pairs(p, n, i, j, mode=2)
    b = _lib.ibd_mle_pairs(p, n, j, i, mode=2)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y, equal_nan=True)
    # Jacquard: the table is not symmetric.  (j, i) exchanges D3 with D5 and D4 with D6 and leaves D1, D2, D7, D8 (and D9); the
    # nine products are then summed in another order, so the exchange holds to the comparison's bounds, not to the bit
    D, ll, nit, _ = _lib.ibd_jacquard_pairs(p, n, i[:64], j[:64])
    E, el, en, _ = _lib.ibd_jacquard_pairs(p, n, j[:64], i[:64])
    want = dict(D=mref.swap_samples(E), loglik=el, niter=en.astype(np.int64))
    assert _compare_jacquard(D, ll, nit, want, "Jacquard (i, j) against the exchanged (j, i)") <= MAX_NITER_DIFFS
    assert np.abs(E - D)[[2, 3, 4, 5]].max() > 1e-3, "no listed pair tells (i, j) from (j, i)"


@pytest.mark.parametrize("method", ["simplex", "jacquard"])
def test_queue_refill_and_determinism(method):
    n, m, P = 24, 33, 6000                     # more pairs than the 16 waves x 256 CUs launched: every wave refills
    p = synth_hash_block_packed(n, 0, m, 11 + n + m, 0.05, 0, False)
    g = unpack_2bit_rows(p, n)
    rng = np.random.default_rng(m)
    i1, i2 = rng.integers(0, n, P), rng.integers(0, n, P)
    key, first, inv = np.unique(i1 * n + i2, return_index=True, return_inverse=True)
    if method == "simplex":
        call = lambda: _lib.ibd_mle_pairs(p, n, i1, i2, mode=2)[:4]
    else:
        call = lambda: (lambda r: (r[0].T, r[1], r[2]))(_lib.ibd_jacquard_pairs(p, n, i1, i2))
    a, b = call(), call()
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)                              # a second call: the same bits
        assert np.array_equal(x, x[first][inv], equal_nan=True)                  # every repeat: the bits of its first occurrence
    ms_k, ms_all, sweeps, pairs = _lib.ibd_mle_pairs_stats()
    assert pairs == P and sweeps >= P and 0 < ms_k <= ms_all
    if method == "simplex":
        want = _simplex_want(p, g, n, i1[first], i2[first], None, 1000, pref.RELTOL, True)
        inside = _compare_simplex(a[0][first], a[1][first], a[2][first], a[3][first], want, pref.RELTOL,
                                  "queue refill, %d distinct pairs" % len(first))
        assert inside <= MAX_INSIDE
        assert sweeps <= int(a[3].sum()) + 2 * P          # no more sweeps than function evaluations (+ start and candidate sweeps)
    else:
        want = mref.jacquard_pairs(g, i1[first], i2[first])
        diffs = _compare_jacquard(a[0][first].T, a[1][first], a[2][first], want, "queue refill, %d distinct pairs" % len(first))
        assert diffs <= MAX_NITER_DIFFS * -(-len(first) // pref.N_LISTED)          # the bound per 200 pairs
        assert sweeps == int(a[2].sum()) + P              # one sweep per EM iteration 0 .. niter of every pair


def test_device_input_equals_host_input():
    torch = pytest.importorskip("torch")
    m, n = 1025, pref.N_SAMP
    p, g = mref.family_genotypes(m)
    i1, i2 = mref.listed_pairs(m, 64)
    dev = torch.from_numpy(p.copy()).cuda()
    torch.cuda.synchronize()
    host = _lib.ibd_mle_pairs(p, n, i1, i2, mode=2)
    got = _lib.ibd_mle_pairs(None, n, i1, i2, mode=2, geno_dev_ptr=dev.data_ptr(), n_snp=m)
    for x, y in zip(host, got):
        assert np.array_equal(x, y, equal_nan=True)
    host = _lib.ibd_jacquard_pairs(p, n, i1, i2)
    got = _lib.ibd_jacquard_pairs(None, n, i1, i2, geno_dev_ptr=dev.data_ptr(), n_snp=m)
    for x, y in zip(host, got):
        assert np.array_equal(x, y, equal_nan=True)


def test_no_shared_call_and_duplicates():
    n, m = 6, 300
    p = synth_hash_block_packed(n, 0, m, 5, 0.05, 0, False)
    g = unpack_2bit_rows(p, n)
    g[:, 1] = g[:, 0]                    # duplicate samples
    g[: m // 2, 2] = 3                   # 2 and 3 share no called SNP
    g[m // 2:, 3] = 3
    i1, i2 = np.array([2, 0, 3, 4, 5, 1]), np.array([3, 1, 2, 5, 5, 4])
    rows = pack_2bit_rows(g)
    for cc in (False, True):
        # no shared call: NaN coefficients, niter 2, log-likelihood -0.0 (it compares equal to 0); no candidate is taken with cc
        k0, k1, ll, nit, _ = _lib.ibd_mle_pairs(rows, n, i1, i2, mode=2, coeff_correct=cc)
        for t in (0, 2):
            assert np.isnan(k0[t]) and np.isnan(k1[t]) and nit[t] == 2 and ll[t] == 0
        want = _simplex_want(rows, g, n, i1, i2, None, 1000, pref.RELTOL, cc)
        _compare_simplex(k0, k1, ll, nit, want, pref.RELTOL, "edge pairs, coeff_correct %s" % cc)
        if cc:
            assert k0[1] == 0 and k1[1] == 0                                    # duplicates: LOGLIK_ADJUST's "self"
        else:
            assert k0[1] + k1[1] <= 0.01
    D, ll, nit, _ = _lib.ibd_jacquard_pairs(rows, n, i1, i2)
    want = mref.jacquard_pairs(g, i1, i2)
    _compare_jacquard(D, ll, nit, want, "edge pairs")
    # no usable SNP: the log-likelihood is 0 before and after the first sweep, so the EM stops at once and keeps the start values
    assert (D[:, [0, 2]] == 0.01).all() and (nit[[0, 2]] == 0).all() and (ll[[0, 2]] == 0).all()
    assert D[6, 1] > 0.9                                                        # duplicates: D7


# ---- 4. the API and the working space on HapMap --------------------------------------------------------------------------------------
def test_hapmap_api(hapmap):
    sid = hapmap.sample_id[:48]
    rng = np.random.default_rng(48)
    a, b = rng.integers(0, 48, 60), rng.integers(0, 48, 60)
    em = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, kinship=True, verbose=False)
    em2 = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, kinship=True, verbose=False, method="EM")
    assert list(em) == list(em2)
    for k in em:
        assert np.array_equal(em[k], em2[k], equal_nan=True) if em[k].dtype.kind in "fi" else np.array_equal(em[k], em2[k])
    rows = [np.nonzero(hapmap.snp_id == s)[0][0] for s in em["snp_id"]]
    g = unpack_2bit_rows(hapmap.packed[rows], hapmap.n_samp)[:, np.isin(hapmap.sample_id, sid)]
    pos = {s: t for t, s in enumerate(em["sample_id"])}
    i = np.array([pos[s] for s in sid[a]])
    j = np.array([pos[s] for s in sid[b]])
    n = g.shape[1]
    rows2 = pack_2bit_rows(g)

    r = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, kinship=True, verbose=False, method="downhill.simplex")
    assert list(r) == list(em) and r["k0"].shape == (60,) and r["niter"].dtype == np.int32
    want = _simplex_want(rows2, g, n, i, j, None, 1000, pref.RELTOL, True)
    assert _compare_simplex(r["k0"], r["k1"], r["loglik"], r["niter"], want, pref.RELTOL, "HapMap simplex") <= MAX_INSIDE
    assert np.array_equal(r["kinship"], 0.5 * (1 - r["k0"] - r["k1"]) + 0.25 * r["k1"], equal_nan=True)
    assert np.array_equal(r["afreq"], em["afreq"], equal_nan=True)
    # the working-space call equals the direct call
    d = _lib.ibd_mle_pairs(rows2, n, i, j, mode=2)
    assert np.array_equal(d[0], r["k0"]) and np.array_equal(d[1], r["k1"]) and np.array_equal(d[2], r["loglik"])
    assert np.array_equal(d[3], r["niter"])

    q = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, kinship=True, verbose=False, method="Jacquard")
    assert "k0" not in q and "k1" not in q and q["D1"].shape == (60,) and q["niter"].dtype == np.int32
    D = np.stack([q["D%d" % t] for t in range(1, 9)])
    want = mref.jacquard_pairs(g, i, j)
    assert _compare_jacquard(D, q["loglik"], q["niter"], want, "HapMap Jacquard") <= MAX_NITER_DIFFS
    assert np.array_equal(q["kinship"], D[0] + 0.5 * (D[2] + D[4] + D[6]) + 0.25 * D[7], equal_nan=True)
    d = _lib.ibd_jacquard_pairs(rows2, n, i, j)
    assert np.array_equal(d[0], D) and np.array_equal(d[1], q["loglik"]) and np.array_equal(d[2], q["niter"])
    q2 = api.snpgdsIBDMLEPairs(hapmap, sid[a], sid[b], sample_id=sid, out_num_iter=False, coeff_correct=False, verbose=False,
                               method="Jacquard")
    assert q2["niter"] is None and "kinship" not in q2 and np.array_equal(q2["D8"], q["D8"])        # coeff_correct: no effect


def test_abi_mode_and_null_outputs():
    n, m = 5, 20
    p = synth_hash_block_packed(n, 0, m, 1, 0.0, 0, False)
    with pytest.raises(_lib.SnpGpuError, match="invalid mode 3"):
        _lib.ibd_mle_pairs(p, n, [0], [1], mode=3)
    with pytest.raises(_lib.SnpGpuError, match="out of range"):
        _lib.ibd_jacquard_pairs(p, n, [0, 5], [1, 2])
    L = _lib.lib()
    i1, i2 = np.zeros(1, np.int32), np.ones(1, np.int32)
    d = np.empty(8, np.float64)
    _lib.check(L.snpgpu_ibd_jacquard_pairs(_lib._ptr(p), m, n, _lib.GENO_PACKED2, _lib.HOST, None, _lib._ptr(i1), _lib._ptr(i2), 1, 10,
                                           1e-8, _lib._ptr(d), None, None, None, _lib.HOST, 0))
    full = _lib.ibd_jacquard_pairs(p, n, [0], [1], max_niter=10, reltol=1e-8)
    assert np.array_equal(d, full[0][:, 0])
    # max_niter < 0: the start values and niter = max_niter, as the EM kernels
    D, ll, nit, _ = _lib.ibd_jacquard_pairs(p, n, [0], [1], max_niter=-1)
    assert (D == 0.01).all() and nit[0] == -1 and np.isfinite(ll[0])
