"""numpy restatement of the reference's IBD-MLE (EM) path, vectorised over sample pairs (test infrastructure only).

Follows src/genIBD.cpp in fp64 and in its order of operations:
  init_afreq        InitAFreq               :1122-1165
  e_prib            Init_EPrIBD_IBS(.., false) :253-338 (plain monomials)
  plink_start       Est_PLINK_Kinship(constraint = false) :341-385 + the 0.005 clamp :824-832
  pr_table          PrIBDTable              :454-510
  loglik            EM_LogLik               :538-575
  em                EMAlg + LOGLIK_ADJUST   :582-656
Pairs that have stopped drop out of the active set.  For each pair `em` also returns the final log-likelihood and the margins
of its discrete decisions: the smallest | |dLogLik| - ConvTol | over its iterations, and the gap between the best and the
second-best value among the final log-likelihood and the finite coeff.correct candidates.

Genotypes are codes g[snp, sample] in {0, 1, 2, 3 = missing}."""
import numpy as np

CANDIDATES = ((0.0, 0.0), (0.25, 0.5), (0.0, 1.0), (0.5, 0.5), (0.75, 0.25), (1.0, 0.0))
RELTOL = float(np.sqrt(np.finfo(float).eps))


def init_afreq(g, allele_freq=None):
    if allele_freq is not None:
        a = np.asarray(allele_freq, np.float64)
        return np.where(np.isfinite(a), a, -1.0)
    called = g < 3
    s = np.where(called, g, 0).sum(1).astype(np.float64)
    n = 2 * called.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / np.maximum(n, 1), -1.0)


def e_prib(af):
    """E[IBS | IBD]: {E00, E01, E02, E11, E12} over the SNPs with a finite p in [0, 1], summed in SNP order"""
    tot = np.zeros(5)
    nv = 0
    for p in af:
        if not (0 <= p <= 1):
            continue
        q = 1 - p
        v = (2 * p * p * q * q, 4 * p * p * p * q + 4 * p * q * q * q, q * q * q * q + p * p * p * p + 4 * p * p * q * q,
             2 * p * p * q + 2 * p * q * q, p * p * p + q * q * q + p * p * q + p * q * q)
        for k in range(5):
            tot[k] += v[k]
        nv += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return tot / nv if nv else np.full(5, np.nan)


def ibs_counts(g, i, j):
    a, b = g[:, i].T, g[:, j].T
    both = (a < 3) & (b < 3)
    d = np.abs(a.astype(np.int8) - b.astype(np.int8))
    return ((both & (d == 2)).sum(1), (both & (d == 1)).sum(1), (both & (d == 0)).sum(1))


def plink_start(ibs0, ibs1, ibs2, e):
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
        # the MLE's adjustment of the initial values, :824-832
        a, b = k0, k1
        c = 1 - a - b
        a = np.where(a < 0.005, 0.005, a); b = np.where(b < 0.005, 0.005, b); c = np.where(c < 0.005, 0.005, c)
        s = a + b + c
        return a / s, b / s


def pr_table(g, i, j, af):
    """PrIBDTable for every pair (rows) and SNP (columns): t0, t1, t2"""
    a, b = g[:, i].T.astype(np.int64), g[:, j].T.astype(np.int64)
    p = np.broadcast_to(af, a.shape)
    q = 1 - p
    t0, t1, t2 = np.zeros(a.shape), np.zeros(a.shape), np.zeros(a.shape)

    def put(m, v0, v1, v2):
        t0[m], t1[m], t2[m] = v0[m], v1[m], v2[m]
    z = np.zeros(a.shape)
    ok = (0 < p) & (p < 1)
    # mm,mm: t2 = q*q; t1 = t2*q; t0 = t1*q
    qq = q * q; qqq = qq * q
    put(ok & (a == 0) & (b == 0), qqq * q, qqq, qq)
    pqq = p * q * q
    put(ok & (((a == 0) & (b == 1)) | ((a == 1) & (b == 0))), 2 * pqq * q, pqq, z)
    ppqq = p * p * q * q
    put(ok & (((a == 0) & (b == 2)) | ((a == 2) & (b == 0))), ppqq, z, z)
    pq = p * q
    put(ok & (a == 1) & (b == 1), 4 * pq * pq, pq, 2 * pq)
    ppq = p * p * q
    put(ok & (((a == 1) & (b == 2)) | ((a == 2) & (b == 1))), 2 * p * ppq, ppq, z)
    pp = p * p; ppp = pp * p
    put(ok & (a == 2) & (b == 2), ppp * p, ppp, pp)
    return t0, t1, t2


def loglik(pr, k0, k1):
    """EM_LogLik per pair (k0, k1: arrays over pairs); -Inf when a sum is not > 0 where t0 > 0"""
    t0, t1, t2 = pr
    k0 = np.asarray(k0, np.float64)[:, None] * np.ones((1, t0.shape[1]))
    k1 = np.asarray(k1, np.float64)[:, None] * np.ones((1, t0.shape[1]))
    k2 = 1 - k0 - k1
    with np.errstate(invalid="ignore", divide="ignore"):
        s = t0 * k0 + t1 * k1 + t2 * k2
        pos = s > 0
        ll = np.where(pos, np.log(np.where(pos, s, 1.0)), 0.0).sum(1)
    bad = ((~pos) & (t0 > 0)).any(1)
    return np.where(bad, -np.inf, ll)


def em(pr, k0, k1, max_niter=1000, reltol=RELTOL, coeff_correct=True):
    """EMAlg for every pair (rows of pr) from start values k0 / k1.  Returns dict of k0, k1, niter, loglik, stop_margin,
    cand_gap (arrays over pairs)."""
    t0, t1, t2 = pr
    P = t0.shape[0]
    k0 = np.array(k0, np.float64)
    k1 = np.array(k1, np.float64)
    k2 = 1 - k0 - k1
    L0 = loglik(pr, k0, k1)
    fin = np.isfinite(L0)
    tol = np.where(fin, reltol * (np.abs(np.where(fin, L0, 0)) + abs(reltol)), reltol)
    tol = np.where(tol < 0, 0, tol)
    out_k0, out_k1 = k0.copy(), k1.copy()
    out_ll = np.where(fin, L0, 1e8)
    niter = np.full(P, max_niter, np.int64)
    margin = np.full(P, np.inf)
    old = np.zeros(P)
    active = np.arange(P) if max_niter >= 0 else np.arange(0)
    it = 0
    while active.size and it <= max_niter:
        a0, a1, a2 = t0[active], t1[active], t2[active]
        c0, c1, c2 = k0[active, None], k1[active, None], k2[active, None]
        m0, m1, m2 = a0 * c0, a1 * c1, a2 * c2
        ms = m0 + m1 + m2
        pos = ms > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            r0 = np.where(pos, m0 / np.where(pos, ms, 1), 0).sum(1)
            r1 = np.where(pos, m1 / np.where(pos, ms, 1), 0).sum(1)
            L = np.where(pos, np.log(np.where(pos, ms, 1)), 0).sum(1)
            n = pos.sum(1)
            nk0, nk1 = r0 / n, r1 / n
        d = np.abs(L - old[active]) - tol[active]
        margin[active] = np.minimum(margin[active], np.abs(d))
        stop = d <= 0
        s_idx = active[stop]
        out_k0[s_idx], out_k1[s_idx] = k0[s_idx], k1[s_idx]
        out_ll[s_idx] = L[stop]
        niter[s_idx] = it
        go = active[~stop]
        old[go] = L[~stop]
        k0[go], k1[go] = nk0[~stop], nk1[~stop]
        k2[go] = 1 - k0[go] - k1[go]
        if it == max_niter:
            out_k0[go], out_k1[go] = k0[go], k1[go]
            out_ll[go] = L[~stop]
        active = go
        it += 1
    gap = np.full(P, np.inf)
    if coeff_correct:
        vals = [out_ll.copy()]
        best = out_ll.copy()
        for ck0, ck1 in CANDIDATES:
            lc = loglik(pr, np.full(P, ck0), np.full(P, ck1))
            vals.append(np.where(np.isfinite(lc), lc, np.nan))
            upd = np.isfinite(lc) & (best < lc)
            best = np.where(upd, lc, best)
            out_k0 = np.where(upd, ck0, out_k0)
            out_k1 = np.where(upd, ck1, out_k1)
        V = np.stack(vals, 1)
        for r in range(P):
            v = np.unique(V[r][np.isfinite(V[r])])
            if v.size >= 2:
                gap[r] = v[-1] - v[-2]
    return dict(k0=out_k0, k1=out_k1, niter=niter, loglik=out_ll, stop_margin=margin, cand_gap=gap)


def ibd_mle(g, allele_freq=None, max_niter=1000, reltol=RELTOL, coeff_correct=True, pairs=None, chunk=256):
    """gnrIBD_MLE for the given pairs (arrays i < j; default all pairs): dict of per-pair results plus afreq and the pairs"""
    n = g.shape[1]
    if pairs is None:
        pairs = np.triu_indices(n, 1)
    i, j = np.asarray(pairs[0]), np.asarray(pairs[1])
    af = init_afreq(g, allele_freq)
    e = e_prib(af)
    res = {k: [] for k in ("k0", "k1", "niter", "loglik", "stop_margin", "cand_gap")}
    for c in range(0, len(i), chunk):
        ii, jj = i[c:c + chunk], j[c:c + chunk]
        s0, s1 = plink_start(*ibs_counts(g, ii, jj), e)
        r = em(pr_table(g, ii, jj, af), s0, s1, max_niter, reltol, coeff_correct)
        for k in res:
            res[k].append(r[k])
    out = {k: np.concatenate(v) if v else np.zeros(0) for k, v in res.items()}
    out.update(afreq=af, i=i, j=j)
    return out


def loglik_matrix(g, allele_freq, k0, k1):
    """Do_MLE_LogLik (k0, k1: n x n) or Do_MLE_LogLik_k01 (scalars): n x n, diagonal included"""
    n = g.shape[1]
    af = init_afreq(g, allele_freq)
    i, j = np.triu_indices(n, 0)
    out = np.empty((n, n))
    for c in range(0, len(i), 256):
        ii, jj = i[c:c + 256], j[c:c + 256]
        a = k0[ii, jj] if np.ndim(k0) else np.full(len(ii), k0)
        b = k1[ii, jj] if np.ndim(k1) else np.full(len(ii), k1)
        v = loglik(pr_table(g, ii, jj, af), a, b)
        out[ii, jj] = v
        out[jj, ii] = v
    return out
