"""numpy restatement of what snpgpu_ibd_mle_pairs computes for a list of pairs, on top of tests/ibd_mle_ref.py (imported unchanged),
and loop-by-loop transcriptions of the reference's two single-pair routines (test infrastructure only).

Added to ibd_mle_ref:
  est_plink_kinship   Est_PLINK_Kinship with its constraint argument (src/genIBD.cpp:341-383), before the 0.005 clamp
  clamp_start         the clamp of :824-832 / Do_MLE_IBD_Pair :1235-1242
  adjusted_loglik     out_loglik after LOGLIK_ADJUST (:646-655), gnrPairIBD's third output
  ibd_mle_pairs       the listed pairs (any order, i == j and repeats allowed), mode 0 (EM) or 1 (start values only)
Transcriptions (scalar loops in the reference's order of operations):
  pair_ibd            snpgdsPairIBD, R/IBD.R:228-246 + gnrPairIBD :1646-1719 + Do_MLE_IBD_Pair :1230-1266, methods "EM" and "MoM"
  pair_ibd_loglik     snpgdsPairIBDMLELogLik, R/IBD.R:281-320 + gnrPairIBDLogLik :1771-1808

Genotypes are codes g[snp, sample] in {0, 1, 2, 3 = missing}; the single-pair routines take what the user gives (anything outside
0..2, NaN included, is missing)."""
import math

import numpy as np

import ibd_mle_ref as ref

RELTOL = ref.RELTOL


def est_plink_kinship(ibs0, ibs1, ibs2, e, constraint=False):
    """(k0, k1) of Est_PLINK_Kinship for arrays of counts; e = {E00, E01, E02, E11, E12}"""
    n = (ibs0 + ibs1 + ibs2).astype(np.float64)
    e00, e01, e11, e02, e12, e22 = e[0] * n, e[1] * n, e[3] * n, e[2] * n, e[4] * n, 1.0 * n
    with np.errstate(invalid="ignore", divide="ignore"):
        k0 = ibs0 / e00
        k1 = (ibs1 - k0 * e01) / e11
        k2 = (ibs2 - k0 * e02 - k1 * e12) / e22
        m = k0 > 1; k0 = np.where(m, 1, k0); k1 = np.where(m, 0, k1); k2 = np.where(m, 0, k2)
        m = k1 > 1; k1 = np.where(m, 1, k1); k0 = np.where(m, 0, k0); k2 = np.where(m, 0, k2)
        m = k2 > 1; k2 = np.where(m, 1, k2); k0 = np.where(m, 0, k0); k1 = np.where(m, 0, k1)
        m = k0 < 0; S = k1 + k2; k1 = np.where(m, k1 / S, k1); k2 = np.where(m, k2 / S, k2); k0 = np.where(m, 0, k0)
        m = k1 < 0; S = k0 + k2; k0 = np.where(m, k0 / S, k0); k2 = np.where(m, k2 / S, k2); k1 = np.where(m, 0, k1)
        m = k2 < 0; S = k0 + k1; k0 = np.where(m, k0 / S, k0); k1 = np.where(m, k1 / S, k1)
        if constraint:
            k2 = 1 - k0 - k1
            pihat = k1 / 2 + k2
            m = pihat * pihat < k2
            k0 = np.where(m, (1 - pihat) * (1 - pihat), k0)
            k1 = np.where(m, 2 * pihat * (1 - pihat), k1)
    return k0, k1


def clamp_start(k0, k1):
    with np.errstate(invalid="ignore"):
        a, b = k0, k1
        c = 1 - a - b
        a = np.where(a < 0.005, 0.005, a); b = np.where(b < 0.005, 0.005, b); c = np.where(c < 0.005, 0.005, c)
        s = a + b + c
        return a / s, b / s


def adjusted_loglik(pr, out_ll):
    """out_loglik after the six LOGLIK_ADJUST steps, given the EM's final log-likelihood"""
    best = np.array(out_ll, np.float64)
    for ck0, ck1 in ref.CANDIDATES:
        lc = ref.loglik(pr, np.full(len(best), ck0), np.full(len(best), ck1))
        with np.errstate(invalid="ignore"):
            best = np.where(np.isfinite(lc) & (best < lc), lc, best)
    return best


def ibd_mle_pairs(g, i, j, allele_freq=None, max_niter=1000, reltol=RELTOL, coeff_correct=True, mode=0, constraint=False,
                  chunk=256):
    """dict of k0, k1, niter, loglik (after LOGLIK_ADJUST), loglik_em (before it), stop_margin, cand_gap per listed pair, and afreq.
    Repeated pairs are computed once."""
    i, j = np.asarray(i), np.asarray(j)
    af = ref.init_afreq(g, allele_freq)
    e = ref.e_prib(af)
    key, first, inv = np.unique(i.astype(np.int64) * g.shape[1] + j, return_index=True, return_inverse=True)
    ui, uj = i[first], j[first]
    res = {k: [] for k in ("k0", "k1", "niter", "loglik", "loglik_em", "stop_margin", "cand_gap")}
    for c in range(0, len(ui), chunk):
        ii, jj = ui[c:c + chunk], uj[c:c + chunk]
        m0, m1 = est_plink_kinship(*ref.ibs_counts(g, ii, jj), e, constraint)
        if mode == 1:
            P = len(ii)
            r = dict(k0=m0, k1=m1, niter=np.zeros(P, np.int64), loglik=np.full(P, np.nan), loglik_em=np.full(P, np.nan),
                     stop_margin=np.full(P, np.inf), cand_gap=np.full(P, np.inf))
        else:
            pr = ref.pr_table(g, ii, jj, af)
            s0, s1 = clamp_start(m0, m1)
            r = ref.em(pr, s0, s1, max_niter, reltol, coeff_correct)
            r["loglik_em"] = r["loglik"]
            r["loglik"] = adjusted_loglik(pr, r["loglik"]) if coeff_correct else r["loglik"]
        for k in res:
            res[k].append(r[k])
    out = {k: np.concatenate(v)[inv] for k, v in res.items()}
    out.update(afreq=af, i=i, j=j)
    return out


# ---- transcriptions ---------------------------------------------------------------------------------------------------------
def _pr_ibd_table(g1, g2, p):
    """PrIBDTable, :454-502"""
    if 0 < p < 1:
        q = 1 - p
        if g1 == 0:
            if g2 == 0:
                t2 = q * q; t1 = t2 * q; t0 = t1 * q; return t0, t1, t2
            if g2 == 1:
                t1 = p * q * q; t0 = 2 * t1 * q; return t0, t1, 0.0
            if g2 == 2:
                return p * p * q * q, 0.0, 0.0
        elif g1 == 1:
            if g2 == 0:
                t1 = p * q * q; t0 = 2 * t1 * q; return t0, t1, 0.0
            if g2 == 1:
                t1 = p * q; return 4 * t1 * t1, t1, 2 * t1
            if g2 == 2:
                t1 = p * p * q; return 2 * p * t1, t1, 0.0
        elif g1 == 2:
            if g2 == 0:
                return p * p * q * q, 0.0, 0.0
            if g2 == 1:
                t1 = p * p * q; return 2 * p * t1, t1, 0.0
            if g2 == 2:
                t2 = p * p; t1 = t2 * p; t0 = t1 * p; return t0, t1, t2
    return 0.0, 0.0, 0.0


def _div(a, b):
    if b == 0:
        return math.nan if (a == 0 or math.isnan(a)) else math.copysign(math.inf, a)
    return a / b


def _em_loglik(pr, k0, k1):
    """EM_LogLik, :538-575"""
    k = (k0, k1, 1 - k0 - k1)
    ll = 0.0
    for t in pr:
        s = t[0] * k[0] + t[1] * k[1] + t[2] * k[2]
        if s > 0:
            ll += math.log(s)
        elif t[0] > 0:
            return -math.inf
    return ll


def _as_integer(v):
    """R's as.integer on one number: truncation, NA for a non-finite value (None here)"""
    v = float(v)
    return int(v) if math.isfinite(v) else None


def _r_filter(geno1, geno2, allele_freq):
    """R/IBD.R:228-241: non-finite frequencies become -1, loci outside [0, 1] are dropped"""
    af = [(-1.0 if not math.isfinite(float(p)) else float(p)) for p in allele_freq]
    keep = [t for t in range(len(af)) if 0 <= af[t] <= 1]
    return [_as_integer(geno1[t]) for t in keep], [_as_integer(geno2[t]) for t in keep], [af[t] for t in keep]


def pair_ibd(geno1, geno2, allele_freq, method="EM", kinship_constraint=False, max_niter=1000, reltol=RELTOL, coeff_correct=True):
    """(k0, k1, loglik, niter) of snpgdsPairIBD for method "EM" or "MoM" """
    g1, g2, af = _r_filter(geno1, geno2, allele_freq)
    n = len(g1)
    # Init_EPrIBD_IBS(AlleleFreq, NULL, false, n), :253-338
    E = [0.0] * 5
    n_valid = 0
    for p in af:
        if math.isfinite(p) and (p < 0 or p > 1):
            p = math.nan
        q = 1 - p
        a = (2 * p * p * q * q, 4 * p * p * p * q + 4 * p * q * q * q, q * q * q * q + p * p * p * p + 4 * p * p * q * q,
             2 * p * p * q + 2 * p * q * q, p * p * p + q * q * q + p * p * q + p * q * q)
        if all(math.isfinite(v) for v in a):
            for t in range(5):
                E[t] += a[t]
            n_valid += 1
    E = [_div(v, n_valid) for v in E]
    # IBS counts, :1669-1676
    ibs = [0, 0, 0]
    for a, b in zip(g1, g2):
        if a is not None and b is not None and 0 <= a <= 2 and 0 <= b <= 2:
            ibs[2 - abs(a - b)] += 1
    # Est_PLINK_Kinship, :341-383
    nn = ibs[0] + ibs[1] + ibs[2]
    e00, e01, e11, e02, e12, e22 = E[0] * nn, E[1] * nn, E[3] * nn, E[2] * nn, E[4] * nn, 1.0 * nn
    k0 = _div(ibs[0], e00)
    k1 = _div(ibs[1] - k0 * e01, e11)
    k2 = _div(ibs[2] - k0 * e02 - k1 * e12, e22)
    if k0 > 1: k0 = 1; k1 = k2 = 0
    if k1 > 1: k1 = 1; k0 = k2 = 0
    if k2 > 1: k2 = 1; k0 = k1 = 0
    if k0 < 0: S = k1 + k2; k1 = _div(k1, S); k2 = _div(k2, S); k0 = 0
    if k1 < 0: S = k0 + k2; k0 = _div(k0, S); k2 = _div(k2, S); k1 = 0
    if k2 < 0: S = k0 + k1; k0 = _div(k0, S); k1 = _div(k1, S); k2 = 0
    if kinship_constraint:
        k2 = 1 - k0 - k1
        pihat = k1 / 2 + k2
        if pihat * pihat < k2:
            k0 = (1 - pihat) * (1 - pihat)
            k1 = 2 * pihat * (1 - pihat)
    if method == "MoM":
        return k0, k1, math.nan, 0
    # Do_MLE_IBD_Pair, :1235-1266
    a, b, c = k0, k1, 1 - k0 - k1
    if a < 0.005: a = 0.005
    if b < 0.005: b = 0.005
    if c < 0.005: c = 0.005
    s = a + b + c
    out_k0, out_k1 = a / s, b / s
    pr = [_pr_ibd_table(-1 if x is None else x, -1 if y is None else y, p) for x, y, p in zip(g1, g2, af)]
    # EMAlg, :582-656
    k = [out_k0, out_k1, 1 - out_k0 - out_k1]
    old = 0.0
    L = _em_loglik(pr, k[0], k[1])
    if math.isfinite(L):
        tol = reltol * (abs(L) + abs(reltol))
        if tol < 0:
            tol = 0
    else:
        L = 1e8
        tol = reltol
    niter = max_niter
    for it in range(0, max_niter + 1):
        oldk = list(k)
        sm = [0.0, 0.0]
        ns = 0
        L = 0.0
        for t in pr:
            mul = (t[0] * k[0], t[1] * k[1], t[2] * k[2])
            ms = mul[0] + mul[1] + mul[2]
            if ms > 0:
                sm[0] += mul[0] / ms; sm[1] += mul[1] / ms
                ns += 1
                L += math.log(ms)
        k[0] = _div(sm[0], ns); k[1] = _div(sm[1], ns)
        k[2] = 1 - k[0] - k[1]
        if abs(L - old) <= tol:
            k = oldk
            niter = it
            break
        old = L
    out_k0, out_k1, out_ll = k[0], k[1], L
    if coeff_correct:
        for c0, c1 in ref.CANDIDATES:
            lc = _em_loglik(pr, c0, c1)
            if math.isfinite(lc) and out_ll < lc:
                out_ll, out_k0, out_k1 = lc, c0, c1
    return out_k0, out_k1, out_ll, niter


def pair_ibd_loglik(geno1, geno2, allele_freq, k0, k1):
    """snpgdsPairIBDMLELogLik at (k0, k1): sums that are not > 0 are skipped"""
    g1, g2, af = _r_filter(geno1, geno2, allele_freq)
    k = (k0, k1, 1 - k0 - k1)
    ll = 0.0
    for x, y, p in zip(g1, g2, af):
        t = _pr_ibd_table(-1 if x is None else x, -1 if y is None else y, p)
        s = t[0] * k[0] + t[1] * k[1] + t[2] * k[2]
        if s > 0:
            ll += math.log(s)
    return ll


# ---- the inputs of tests/test_gpu_ibd_pairs.py (the CPU file checks on them that no pair's coeff.correct decision is a near-tie) ----
N_SAMP, N_LISTED = 24, 200
# n_snp, missing, special allele_freq, max_niter, reltol (None: the default), coeff_correct.  The SNP counts straddle the 16-SNP word
# and the 64-lane x 16-SNP step of the lane-split sweep.
GPU_CASES = [
    (1, 0.0, False, 1000, None, True),
    (15, 0.05, False, 1000, None, True),
    (16, 0.05, False, 1000, None, True),
    (17, 0.3, False, 1000, None, True),
    (1023, 0.05, False, 1000, None, True),
    (1024, 0.0, False, 1000, None, True),
    (1025, 0.05, False, 1000, None, True),
    (2049, 0.3, False, 1000, None, True),
    (1025, 0.05, True, 1000, None, True),
    (1023, 0.05, False, 0, None, True),
    (1024, 0.0, False, 5, None, True),
    (1025, 0.05, False, 1000, 1e-4, True),
    (2049, 0.3, False, 1000, None, False),
]
_case_cache = {}


def case_inputs(case):
    """(packed rows, codes g, allele_freq or None, idx1, idx2, reference dict) of one of GPU_CASES; computed once per session and
    shared (read-only) by the tests"""
    if case in _case_cache:
        return _case_cache[case]
    from oracle.synth import synth_hash_block_packed
    from snprelate_amd.gds import unpack_2bit_rows
    m, miss, special, max_niter, reltol, cc = case
    n = N_SAMP
    p = synth_hash_block_packed(n, 0, m, 11 + n + m, miss, 0, False)
    g = unpack_2bit_rows(p, n)
    af = None
    if special:                                    # as test_gpu_ibd_mle.CASES
        af = np.random.default_rng(n).uniform(0.05, 0.95, m)
        af[:: 5][:4] = [np.nan, 0.0, 1.0, 1.5][: len(af[:: 5][:4])]
        if m > 12:
            af[12] = -0.2
    rng = np.random.default_rng(m)
    i1 = rng.integers(0, n, N_LISTED)
    i2 = rng.integers(0, n, N_LISTED)
    want = ibd_mle_pairs(g, i1, i2, af, max_niter, RELTOL if reltol is None else reltol, cc)
    for v in want.values():
        v.setflags(write=False)
    _case_cache[case] = (p, g, af, i1, i2, want)
    return _case_cache[case]
