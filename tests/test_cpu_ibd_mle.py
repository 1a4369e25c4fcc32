"""CPU tests of the IBD-MLE reference (tests/ibd_mle_ref.py): the vectorised numpy restatement is pinned to a literal, loop-by-loop
transcription of InitAFreq / Init_EPrIBD_IBS / EMAlg / EM_LogLik / Est_PLINK_Kinship (src/genIBD.cpp:253-338, :341-385, :454-656,
:823-832, :1122-1165) written below, on about
twenty pairs with missing calls, special allele frequencies, an all-missing pair, duplicates, few iterations and both
coeff.correct settings.  Also: the new C ABI is exported, and refuses the methods that are not built without needing a GPU."""
import math

import numpy as np
import pytest

import ibd_mle_ref as ref

RELTOL = math.sqrt(np.finfo(float).eps)


# ---- literal transcription --------------------------------------------------------------------------------------------------
def s_table(g1, g2, p):
    if 0 < p < 1:
        q = 1 - p
        if g1 == 0:
            if g2 == 0:
                t2 = q * q; t1 = t2 * q; t0 = t1 * q; return t0, t1, t2
            if g2 == 1:
                t1 = p * q * q; t0 = 2 * t1 * q; return t0, t1, 0.0
            if g2 == 2:
                return p * p * q * q, 0.0, 0.0
            return 0.0, 0.0, 0.0
        if g1 == 1:
            if g2 == 0:
                t1 = p * q * q; t0 = 2 * t1 * q; return t0, t1, 0.0
            if g2 == 1:
                t1 = p * q; return 4 * t1 * t1, t1, 2 * t1
            if g2 == 2:
                t1 = p * p * q; return 2 * p * t1, t1, 0.0
            return 0.0, 0.0, 0.0
        if g1 == 2:
            if g2 == 0:
                return p * p * q * q, 0.0, 0.0
            if g2 == 1:
                t1 = p * p * q; return 2 * p * t1, t1, 0.0
            if g2 == 2:
                t2 = p * p; t1 = t2 * p; t0 = t1 * p; return t0, t1, t2
        return 0.0, 0.0, 0.0
    return 0.0, 0.0, 0.0


def s_loglik(pr, k0, k1):
    k = (k0, k1, 1 - k0 - k1)
    ll = 0.0
    for t in pr:
        s = t[0] * k[0] + t[1] * k[1] + t[2] * k[2]
        if s > 0:
            ll += math.log(s)
        elif t[0] > 0:
            return -math.inf
    return ll


def s_start(ibs0, ibs1, ibs2, E):
    n = ibs0 + ibs1 + ibs2
    e00, e01, e11, e02, e12, e22 = E[0] * n, E[1] * n, E[3] * n, E[2] * n, E[4] * n, 1.0 * n

    def div(a, b):
        if b == 0:
            return math.nan if a == 0 or math.isnan(a) else math.copysign(math.inf, a)
        return a / b
    k0 = div(ibs0, e00)
    k1 = div(ibs1 - k0 * e01, e11)
    k2 = div(ibs2 - k0 * e02 - k1 * e12, e22)
    if k0 > 1: k0 = 1; k1 = k2 = 0
    if k1 > 1: k1 = 1; k0 = k2 = 0
    if k2 > 1: k2 = 1; k0 = k1 = 0
    if k0 < 0: S = k1 + k2; k1 /= S; k2 /= S; k0 = 0
    if k1 < 0: S = k0 + k2; k0 /= S; k2 /= S; k1 = 0
    if k2 < 0: S = k0 + k1; k0 /= S; k1 /= S; k2 = 0
    a, b = k0, k1
    c = 1 - a - b
    if a < 0.005: a = 0.005
    if b < 0.005: b = 0.005
    if c < 0.005: c = 0.005
    s = a + b + c
    return a / s, b / s


def s_em(pr, k0, k1, max_niter, reltol, coeff_correct):
    k = [k0, k1, 1 - k0 - k1]
    old = 0.0
    ll = s_loglik(pr, k[0], k[1])
    if math.isfinite(ll):
        tol = reltol * (abs(ll) + abs(reltol))
        if tol < 0:
            tol = 0
    else:
        ll = 1e8
        tol = reltol
    niter = max_niter
    it = 0
    while it <= max_niter:
        oldk = list(k)
        s0 = s1 = 0.0
        n = 0
        ll = 0.0
        for t in pr:
            m = (t[0] * k[0], t[1] * k[1], t[2] * k[2])
            ms = m[0] + m[1] + m[2]
            if ms > 0:
                s0 += m[0] / ms; s1 += m[1] / ms
                n += 1
                ll += math.log(ms)
        with np.errstate(invalid="ignore", divide="ignore"):
            k[0] = float(np.float64(s0) / n); k[1] = float(np.float64(s1) / n)
        k[2] = 1 - k[0] - k[1]
        if abs(ll - old) <= tol:
            k = oldk
            niter = it
            break
        old = ll
        it += 1
    out = [k[0], k[1], ll]
    if coeff_correct:
        for c0, c1 in ref.CANDIDATES:
            v = s_loglik(pr, c0, c1)
            if math.isfinite(v) and out[2] < v:
                out = [c0, c1, v]
    return out[0], out[1], niter


def s_init_afreq(g, af_in):
    """InitAFreq, :1122-1165"""
    m, n = g.shape
    af = [-1.0] * m
    if af_in is not None:
        for i in range(m):
            if math.isfinite(af_in[i]):
                af[i] = float(af_in[i])
        return np.array(af)
    cnt, tot = [0] * m, [0.0] * m
    for s in range(n):
        for i in range(m):
            b = int(g[i, s])
            if b < 3:
                cnt[i] += 2
                tot[i] += b
    return np.array([tot[i] / cnt[i] if cnt[i] > 0 else -1.0 for i in range(m)])


def s_e_prib(g, af_in):
    """Init_EPrIBD_IBS(in_afreq, NULL, false), :253-338: the caller's frequencies, or (2 AA + AB) / n from the counts"""
    e = [0.0] * 5
    n_valid = 0
    for i in range(g.shape[0]):
        AA = int((g[i] == 2).sum()); AB = int((g[i] == 1).sum()); BB = int((g[i] == 0).sum())
        n = 2 * (AA + AB + BB)
        p = (2 * AA + AB) / n if n > 0 else math.nan
        if af_in is not None:
            p = float(af_in[i])
            if math.isfinite(p) and (p < 0 or p > 1):
                p = math.nan
        q = 1 - p
        a00 = 2 * p * p * q * q
        a01 = 4 * p * p * p * q + 4 * p * q * q * q
        a02 = q * q * q * q + p * p * p * p + 4 * p * p * q * q
        a11 = 2 * p * p * q + 2 * p * q * q
        a12 = p * p * p + q * q * q + p * p * q + p * q * q
        if all(math.isfinite(v) for v in (a00, a01, a02, a11, a12)):
            e[0] += a00; e[1] += a01; e[2] += a02; e[3] += a11; e[4] += a12
            n_valid += 1
    return [v / n_valid if n_valid else math.nan for v in e]


def s_mle(g, af_in, max_niter, reltol, coeff_correct):
    af = s_init_afreq(g, af_in)
    E = s_e_prib(g, af_in)
    n = g.shape[1]
    res = {}
    for i in range(n):
        for j in range(i + 1, n):
            a, b = g[:, i], g[:, j]
            both = (a < 3) & (b < 3)
            d = np.abs(a.astype(int) - b.astype(int))
            st = s_start(int((both & (d == 2)).sum()), int((both & (d == 1)).sum()), int((both & (d == 0)).sum()), E)
            pr = [s_table(int(a[l]), int(b[l]), af[l]) for l in range(g.shape[0])]
            res[(i, j)] = s_em(pr, st[0], st[1], max_niter, reltol, coeff_correct)
    return af, res


def _data(n=7, m=60, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, m)
    g = (rng.random((m, n)) < p[:, None]).astype(np.uint8) + (rng.random((m, n)) < p[:, None]).astype(np.uint8)
    g[rng.random((m, n)) < 0.08] = 3          # missing calls
    g[:, 1] = g[:, 0]                          # duplicate samples
    g[:, 3] = 3                                # an all-missing sample: its pairs share no usable SNP
    g[:5, 4] = 3
    return g


@pytest.mark.parametrize("max_niter", [0, 1, 5, 1000])
@pytest.mark.parametrize("coeff_correct", [True, False])
@pytest.mark.parametrize("special_af", [False, True])
def test_reference_matches_transcription(max_niter, coeff_correct, special_af):
    g = _data()
    af = None
    if special_af:
        af = np.random.default_rng(3).uniform(0.1, 0.9, g.shape[0])
        af[[2, 9, 17, 30]] = [0.0, 1.0, np.nan, 1.5]
    af_s, want = s_mle(g, af, max_niter, RELTOL, coeff_correct)
    got = ref.ibd_mle(g, af, max_niter, RELTOL, coeff_correct)
    assert np.array_equal(got["afreq"], af_s)
    np.testing.assert_allclose(ref.e_prib(got["afreq"]), s_e_prib(g, af), rtol=1e-14, atol=0)
    assert len(got["i"]) == len(want) == 21
    for r, (i, j) in enumerate(zip(got["i"], got["j"])):
        k0, k1, nit = want[(i, j)]
        ll = got["loglik"][r]
        if got["stop_margin"][r] > 1e-9 * abs(ll if np.isfinite(ll) else 0):
            assert got["niter"][r] == nit, (i, j)
        if got["niter"][r] == nit and got["cand_gap"][r] > 1e-9 * abs(ll if np.isfinite(ll) else 0):
            for a, b in ((got["k0"][r], k0), (got["k1"][r], k1)):
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-10, (i, j, a, b)
    # pairs with sample 3 share no called SNP: NaN start values, stopped at iteration 0
    m3 = (got["i"] == 3) | (got["j"] == 3)
    assert np.isnan(got["k0"][m3]).all() and (got["niter"][m3] == (0 if max_niter >= 0 else max_niter)).all()


def test_loglik_matches_transcription():
    g = _data(n=5, m=40, seed=4)
    af = s_init_afreq(g, None)
    for k0, k1 in ref.CANDIDATES + ((0.3, 0.4), (0.7, 0.6), (-0.1, 0.5)):
        m = ref.loglik_matrix(g, None, k0, k1)
        for i in range(5):
            for j in range(i, 5):
                pr = [s_table(int(g[l, i]), int(g[l, j]), af[l]) for l in range(g.shape[0])]
                want = s_loglik(pr, k0, k1)
                got = m[i, j]
                assert (math.isinf(want) and got == want) or abs(got - want) <= 1e-12 * max(1, abs(want)), (k0, k1, i, j)


def test_abi_exports_and_refusals():
    """The IBD-MLE entry points are exported, and the methods that are not built are refused before any device is touched."""
    from snprelate_amd import _lib
    import ctypes
    try:
        L = _lib.lib()
    except _lib.SnpGpuError as e:
        pytest.fail("libsnpgpu.so does not load: %s" % e)
    for name in ("snpgpu_ibd_mle", "snpgpu_ibd_loglik", "snpgpu_ibd_mle_stats", "snpgpu_gnrIBD_MLE", "snpgpu_gnrIBD_LogLik",
                 "snpgpu_gnrIBD_LogLik_k01", "snpgpu_diag_fp64_rate"):
        assert hasattr(L, name), name
    for method, word in ((1, "downhill.simplex"), (2, "Jacquard")):
        rc = L.snpgpu_gnrIBD_MLE(None, 0, 1000, RELTOL, 1, method, 1, 1, 0, None, None, None, None)
        assert rc != 0 and word in L.snpgpu_last_error().decode()
    g = np.zeros((4, 1), np.uint8)
    out = np.empty((1, 1))
    rc = L.snpgpu_ibd_mle(g.ctypes.data_as(ctypes.c_void_p), 4, 1, _lib.GENO_PACKED2, _lib.HOST, None, 1000, RELTOL, 1, 0, 0,
                          out.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), None, None, _lib.HOST, 0)
    assert rc != 0 and "two samples" in L.snpgpu_last_error().decode()
