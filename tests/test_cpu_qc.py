"""CPU tests of the quality-control statistics: exports, argument refusals without a device, the restatements (tests/inb_ref.py,
tests/hwe_ref.py) against independent evaluations, and the measured figures of the MLE comparison (tests/qc_fixtures.py)."""
import math

import numpy as np
import pytest

import hwe_ref as H
import inb_ref as R
import qc_fixtures as Q
import snprelate_amd
from snprelate_amd import _lib, api

NEW_SYMBOLS = ("snpgpu_geno_counts", "snpgpu_hwe", "snpgpu_hwe_counts", "snpgpu_ind_inb", "snpgpu_qc_stats", "snpgpu_gnrSampFreq",
               "snpgpu_gnrHWE", "snpgpu_gnrIndInb")
NEW_FUNCTIONS = ("snpgdsSampMissRate", "snpgdsHWE", "snpgdsIndInb", "snpgdsIndInbCoef", "snpgdsSelectSNP")


def test_abi_exports_and_version():
    L = _lib.lib()
    assert L.snpgpu_abi_version() == 2
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s), s


def test_api_exports():
    for f in NEW_FUNCTIONS:
        assert callable(getattr(api, f)) and getattr(snprelate_amd, f) is getattr(api, f)


def test_refusals_without_a_device(hapmap):
    with pytest.raises(ValueError, match="'method' should be one of"):
        api.snpgdsIndInb(hapmap, method="mom.wrong", verbose=False)
    with pytest.raises(ValueError, match="`reltol' should a real number."):
        api.snpgdsIndInb(hapmap, reltol=[1e-9, 1e-8], verbose=False)
    with pytest.raises(ValueError, match="`reltol' should a real number."):
        api.snpgdsIndInbCoef([0, 1], [0.5, 0.5], method="mle", reltol=np.array([1e-9, 1e-8]))
    with pytest.raises(ValueError, match=r"length\(x\) == length\(p\)"):
        api.snpgdsIndInbCoef([0, 1, 2], [0.5, 0.5])
    with pytest.raises(ValueError, match="'method' should be one of"):
        api.snpgdsIndInbCoef([0, 1], [0.5, 0.5], method="gcta1")
    with pytest.raises(TypeError):
        api.snpgdsIndInb(hapmap, out_num_iter=1, verbose=False)
    with pytest.raises(ValueError, match="genotype rows have the wrong shape"):
        _lib.hwe(np.zeros(8, np.uint8), 8)                     # one row given as a 1-D array
    # the C ABI refuses before it asks for a device
    L = _lib.lib()
    g = np.zeros((4, 2), np.uint8)
    out = np.zeros(8, np.float64)
    assert L.snpgpu_ind_inb(_lib._ptr(g), 4, 2, _lib.GENO_U8, _lib.HOST, None, 9, 1e-9, _lib._ptr(out), None, None, _lib.HOST, 0) == 1
    assert b"invalid method" in L.snpgpu_last_error()
    assert L.snpgpu_ind_inb(_lib._ptr(g), 4, 2, _lib.GENO_U8, _lib.HOST, None, 3, float("nan"), _lib._ptr(out), None, None,
                            _lib.HOST, 0) == 1
    assert b"`reltol' should a real number." in L.snpgpu_last_error()
    assert L.snpgpu_gnrIndInb(None, b"nope", 1e-9, 1, 0, _lib._ptr(out), None) == 1
    assert b"'method' should be one of" in L.snpgpu_last_error()
    assert L.snpgpu_geno_counts(_lib._ptr(g), 4, 2, _lib.GENO_U8, _lib.HOST, None, None, _lib.HOST, 0) == 1
    assert L.snpgpu_hwe_counts(_lib._ptr(np.array([[1, -1, 0]], np.int32)), 1, _lib._ptr(out), _lib.HOST, 0) == 1
    assert b"negative" in L.snpgpu_last_error()


@pytest.mark.parametrize("method", ["mom.weir", "mom.visscher"])
def test_moment_restatement_against_the_r_formula(method):
    """The sequential per-sample sums and R's vectorised formula differ by the order of a sum of M terms: each sum is within
    (M - 1) u sum|term| of the exact one (u = 2^-53), so the quotients agree within 2 (M + 2) u (sum|num| / |sum num| + 1) |F|."""
    g, p = Q.simulate_inbred(12, 1500, np.linspace(0, 0.6, 12), 0.03, seed=4)
    g[7] = 3
    p = p.copy()
    p[9] = np.nan
    p[10], p[11] = 0.0, 1.0
    want, _ = R.ind_inb_moment_ref(g, method, p)
    M = g.shape[0]
    for j in range(g.shape[1]):
        x = g[:, j].astype(np.float64)
        if method == "mom.weir":
            ok = ~np.isnan(p)                  # the R formula drops non-finite terms; the C routine does not (poisoning): compare without
            w = R.ind_inb_moment_ref(g[ok][:, j:j + 1], method, p[ok])[0][0]
        else:
            ok = np.ones(M, bool)
            w = want[j]
        got = R.ind_inb_coef_r(x[ok], p[ok], method)
        assert got == api.snpgdsIndInbCoef(x[ok], p[ok], method)
        xs = np.where(x[ok] > 2, np.nan, x[ok])
        num = xs * xs - (1 + 2 * p[ok]) * xs + 2 * p[ok] * p[ok]
        den = 2 * p[ok] * (1 - p[ok])
        with np.errstate(all="ignore"):
            t = num if method == "mom.weir" else num / den
        t = t[np.isfinite(t)]
        cond = np.abs(t).sum() / abs(t.sum()) + 1
        bound = 2 * (M + 2) * 2.0 ** -53 * cond * abs(w)
        assert abs(got - w) <= bound, (method, j, got, w, bound)
    if method == "mom.weir":
        assert np.isnan(want[g[9] <= 2]).all()          # a NaN frequency poisons the samples called there


def _hwe_grid():
    grid = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 7, 0), (9, 0, 0), (0, 0, 9), (6, 0, 5), (5, 0, 5), (4, 1, 0), (4, 2, 0), (3, 3, 3),
            (10, 5, 3), (57, 14, 50), (100, 3, 200), (0, 200, 0), (1, 198, 1)]
    rng = np.random.default_rng(3)
    for n in (50, 500, 3000, 10000):
        for q in (0.01, 0.2, 0.5):
            pr = np.array([(1 - q) ** 2, 2 * q * (1 - q), q * q])
            for _ in range(2):
                a, b, c = rng.multinomial(n, pr)
                grid.append((int(a), int(b), int(c)))
                grid.append((int(a + b // 2), int(b % 2), int(c + b // 2)))          # no heterozygote, or one
    return grid


def test_hwe_restatement_against_lgamma():
    """P(h) through math.lgamma: seven lgamma values of magnitude <= lgamma(2 n + 1), each taken as accurate to 4 ulp of that
    magnitude (glibc documents lgamma within a few ulp), give a relative error of at most 7 x 4 x 2^-52 lgamma(2 n + 1) per term;
    the recurrence adds (rare / 2 + 2) 2^-52 per term and each sum its own (rare / 2 + 2) 2^-53.  Terms within 1e-6 (relative) of
    the observed one are near ties either evaluation may decide either way, hence the interval [p_lo, p_hi]."""
    seen = dict(het0=0, norare=0, one=0, odd=0, even=0, big=0)
    for n0, n1, n2 in _hwe_grid():
        p = H.hwe_pvalue(n1, n2, n0)
        lo, hi = H.hwe_lgamma(n1, n2, n0)
        n, rare = n0 + n1 + n2, 2 * min(n0, n2) + n1
        tol = 28 * 2.0 ** -52 * math.lgamma(2 * n + 1) + 3 * (rare / 2 + 2) * 2.0 ** -52
        assert lo * (1 - tol) - 1e-300 <= p <= hi * (1 + tol) + 1e-300, ((n0, n1, n2), p, lo, hi, tol)
        assert 0 <= p <= 1
        seen["het0"] += n1 == 0
        seen["norare"] += rare == 0
        seen["one"] += n == 1
        seen["odd"] += rare % 2 == 1
        seen["even"] += rare % 2 == 0
        seen["big"] += n >= 10000
    assert all(v > 0 for v in seen.values()), seen
    assert math.isnan(H.hwe_pvalue(0, 0, 0))
    # no heterozygote among 5 + 5 homozygotes: the least likely table, P = C(10, 5) / C(20, 10)
    assert H.hwe_pvalue(0, 5, 5) == pytest.approx(math.comb(10, 5) / math.comb(20, 10), rel=1e-12)


@pytest.mark.parametrize("f", [0.0, 0.25, 1.0])
def test_ind_inb_coef_mle_recovers_simulated_f(f):
    """Sampling error of the simulation: the Fisher information of one SNP about F is I(F, p) = sum_g (dP_g / dF)^2 / P_g with
    dP_0 = dP_2 = p q, dP_1 = -2 p q (at F = 0 it is p^2 + 2 p q + q^2 = 1 for every p), so the MLE's standard error from M
    independent SNPs is 1 / sqrt(sum I); five of them are allowed.  At F = 1 no heterozygote can occur and the information is
    evaluated at the upper clamp 0.999."""
    M = 20000
    rng = np.random.default_rng(int(100 * f) + 1)
    p = rng.uniform(0.2, 0.8, M)
    a = rng.random(M) < p
    b = np.where(rng.random(M) < f, a, rng.random(M) < p)
    x = a.astype(int) + b
    got = api.snpgdsIndInbCoef(x, p, method="mle")
    # the host routine takes its sums with np.sum: the restatement with its sums in that order is the same arithmetic
    ref = R.mle_ref(np.asarray(x, np.uint8), p, float(np.finfo(float).eps ** 0.75), order="pairwise")
    print("F = %g: MLE %.6f, restatement %.6f (niter %d)" % (f, got, ref["F"], ref["niter"]))
    fe = min(f, 0.999)
    q = 1 - p
    P = np.stack([(1 - fe) * q * q + fe * q, (1 - fe) * 2 * p * q, (1 - fe) * p * p + fe * p])
    dP = np.stack([p * q, -2 * p * q, p * q])
    se = 1.0 / math.sqrt(float((dP * dP / P).sum()))
    print("standard error %.3e" % se)
    assert abs(got - f) <= 5.0 * se + (0.001 if f == 1.0 else 0.0)       # the clamp's own distance from the boundary
    assert got == ref["F"]


def test_mle_spread_and_firmness(hapmap):
    """Re-measures, from the restatement alone, what tests/qc_fixtures.py records: the spread of F and of |dLogLik| between
    sequential, reversed, pairwise and long double sums stays within the recorded figures, and at most 10 % of a fixture's samples
    have a stopping margin that is not firm (<= MLE_FIRM).  HapMap: every 6th sample (the full set was measured once: 2 of 279).
    The slow sample must run at least 1 000 sweeps with a firm margin, the never-stopping set all 10 000 updates."""
    fixtures = []
    g = Q.hapmap_autosomal(hapmap)
    fixtures.append(("HapMap", g[:, ::6], R.snp_freq(g), Q.RELTOL))
    g, p = Q.synthetic_mle()
    fixtures.append(("synthetic, given", g, p, Q.RELTOL))
    fixtures.append(("synthetic, estimated", g, R.snp_freq(g), Q.RELTOL))
    g, p = Q.slow_mle()
    fixtures.append(("slow", g, p, Q.SLOW_RELTOL))
    g, p = Q.never_stopping_mle()
    fixtures.append(("never stopping", g, p, Q.NEVER_RELTOL))
    for name, g, p, reltol in fixtures:
        sF = sD = 0.0
        soft = tot = 0
        for j in range(g.shape[1]):
            r = R.mle_ref(g[:, j], p, reltol)
            if r["niter"] < 0:
                continue
            tot += 1
            soft += r["margin"] <= Q.MLE_FIRM
            if name == "slow":
                assert 1000 <= r["niter"] <= 10000 and r["margin"] > Q.MLE_FIRM and r["F"] < 0.001, (r["niter"], r["margin"])
            if name == "never stopping":
                assert r["niter"] == 10001 and r["margin"] > Q.MLE_FIRM, (j, r["niter"], r["margin"])
            n_it = min(r["niter"], 10000)
            base = R.mle_trace(g[:, j], p, reltol, "seq", n_it)
            for o in ("reversed", "pairwise", "longdouble"):
                tr = R.mle_trace(g[:, j], p, reltol, o, n_it)
                sF = max(sF, float(np.abs(tr[0] - base[0]).max()))
                sD = max(sD, float(np.abs(np.abs(np.diff(tr[1])) - np.abs(np.diff(base[1]))).max()))
        print("%s: spread F %.3e, spread |dLogLik| %.3e, not firm %d / %d" % (name, sF, sD, soft, tot))
        assert sF <= Q.MLE_SPREAD_F and sD <= Q.MLE_SPREAD_D, name
        assert soft <= 0.10 * tot, name
