"""numpy restatement of the two IBD-MLE methods beside "EM" for listed pairs, on top of tests/ibd_mle_ref.py and tests/ibd_pairs_ref.py
(both imported unchanged), and loop-by-loop transcriptions of the reference's routines (test infrastructure only).

Follows src/genIBD.cpp in fp64 and in its order of operations:
  nm_prepare / nm_loglik   NM_Prepare :661-684, NM_LogLik :687-727 (one pair, vectorised over the SNPs)
  simplex                  Simplex :741-779 + SimplexMin<double, 2> :97-189 + Simplex_Point_Try :63-84, one pair at a time
  jacq_table               PrIBDTabJacq :864-939 for every pair and SNP, with its (MM, MM) fall-through: all nine are 0 there
  jacquard                 EM_Jacq_LogLik :964-982 + EM_Jacq_Alg :987-1072 from IBD_Jacq_InitVal :1074, vectorised over the pairs
Transcriptions (scalar loops): _pr_tab_jacq, _em_jacq, _nm_loglik, _simplex.

The decision margin of a simplex walk is the smallest |a - b| over every comparison it made between two objective values
(the high / next-high / low scan, the acceptance of a trial point, the choice between expansion, contraction and shrink, the
LOGLIK_ADJUST candidates) and over |(y[ihi] - y[ilo]) - convtol| of every stop test.  Comparisons of a value with itself and
comparisons whose two sides are both exactly the 1e30 penalty are left out.  A walk whose margin is far above the rounding
differences of the objective makes the same decisions whatever the order of the sums.

Genotypes are codes g[snp, sample] in {0, 1, 2, 3 = missing}."""
import math

import numpy as np

import ibd_mle_ref as ref
import ibd_pairs_ref as pref

RELTOL = ref.RELTOL
PENALTY = 1e30
DBL_EPSILON = float(np.finfo(float).eps)


# ---- downhill simplex -------------------------------------------------------------------------------------------------------------
def nm_prepare(pr):
    """(d0, d1, t2) of NM_Prepare from PrIBDTable's (t0, t1, t2)"""
    t0, t1, t2 = pr
    return t0 - t2, t1 - t2, t2


def nm_loglik(d, k0, k1):
    """NM_LogLik of one pair (d: three arrays over the SNPs): -Inf outside the triangle and where a sum is not > 0 while d0 > 0"""
    if (k0 < 0) or (k1 < 0) or (k0 + k1 > 1):
        return -math.inf
    d0, d1, t2 = d
    with np.errstate(invalid="ignore"):
        s = d0 * k0 + d1 * k1 + t2
        pos = s > 0
    if ((~pos) & (d0 > 0)).any():
        return -math.inf
    return float(np.log(s[pos]).sum())


class _Margin:
    """the smallest |a - b| over the comparisons of a walk"""

    def __init__(self):
        self.v = math.inf

    def see(self, a, b, same=False):
        if same or (a == PENALTY and b == PENALTY):
            return
        d = abs(a - b)
        if d < self.v:                      # NaN never lowers it
            self.v = d


def _simplex_min(funk, p, reltol, nfunkmax, mg):
    """SimplexMin<double, 2>; p: 3 x 2 list (changed in place).  Returns (outx, outy, nfunk)."""
    ndim = 2
    y = [funk(p[i][0], p[i][1]) for i in range(ndim + 1)]
    nfunk = ndim
    convtol = reltol * (abs(y[0]) + abs(reltol))
    if convtol < DBL_EPSILON:
        convtol = DBL_EPSILON
    psum = [0.0] * ndim
    for j in range(ndim):
        s = 0.0
        for i in range(ndim + 1):
            s += p[i][j]
        psum[j] = s

    def point_try(ihi, fac):
        fac1 = (1.0 - fac) / ndim
        fac2 = fac1 - fac
        ptry = [psum[j] * fac1 - p[ihi][j] * fac2 for j in range(ndim)]
        ytry = funk(ptry[0], ptry[1])
        mg.see(ytry, y[ihi])
        if ytry < y[ihi]:
            y[ihi] = ytry
            for j in range(ndim):
                psum[j] += ptry[j] - p[ihi][j]
                p[ihi][j] = ptry[j]
        return ytry

    while True:
        ilo = 0
        mg.see(y[0], y[1])
        if y[0] > y[1]:
            inhi, ihi = 1, 0
        else:
            inhi, ihi = 0, 1
        for i in range(ndim + 1):
            mg.see(y[i], y[ilo], i == ilo)
            if y[i] <= y[ilo]:
                ilo = i
            mg.see(y[i], y[ihi], i == ihi)
            if y[i] > y[ihi]:
                inhi = ihi
                ihi = i
            else:
                mg.see(y[i], y[inhi], i == inhi)
                if (y[i] > y[inhi]) and (i != ihi):
                    inhi = i
        mg.see(y[ihi] - y[ilo], convtol)
        if ((y[ihi] - y[ilo]) <= convtol) or (nfunk >= nfunkmax):
            return [p[ilo][0], p[ilo][1]], y[ilo], nfunk
        nfunk += 2
        ytry = point_try(ihi, -1.0)
        mg.see(ytry, y[ilo])
        if ytry <= y[ilo]:
            ytry = point_try(ihi, 2.0)
        else:
            mg.see(ytry, y[inhi])
            if ytry >= y[inhi]:
                ysave = y[ihi]
                ytry = point_try(ihi, 0.5)
                mg.see(ytry, ysave)
                if ytry >= ysave:
                    for i in range(ndim + 1):
                        if i != ilo:
                            for j in range(ndim):
                                p[i][j] = psum[j] = 0.5 * (p[i][j] + p[ilo][j])
                            y[i] = funk(psum[0], psum[1])
                    nfunk += ndim
                    for j in range(ndim):
                        s = 0.0
                        for i in range(ndim + 1):
                            s += p[i][j]
                        psum[j] = s
            else:
                nfunk -= 1


def start_simplex(k0, k1):
    """Simplex's three vertices (:745-757): the second vertex's else branch has no / 2, the third's has"""
    def mx(a, b):                           # std::max
        return b if a < b else a
    p = [[k0, k1], [k0, 0.0], [0.0, k1]]
    f = (1 - k0) / 2
    p[1][1] = (k1 + mx(k1, f - k1) / 2) if k1 <= f else (k1 - mx(k1 - f, 1 - k0 - k1))
    f = (1 - k1) / 2
    p[2][0] = (k0 + mx(k0, f - k0) / 2) if k0 <= f else (k0 - mx(k0 - f, 1 - k1 - k0) / 2)
    return p


def _optim_of(loglik):
    def funk(x0, x1):
        rv = -loglik(x0, x1)
        return rv if math.isfinite(rv) else PENALTY
    return funk


def _simplex_one(loglik, k0, k1, reltol, max_niter, coeff_correct):
    mg = _Margin()
    outx, outy, nfunk = _simplex_min(_optim_of(loglik), start_simplex(k0, k1), reltol, max_niter, mg)
    out_k0, out_k1, out_ll = outx[0], outx[1], -outy
    if coeff_correct:
        for c0, c1 in ref.CANDIDATES:
            lc = loglik(c0, c1)
            if math.isfinite(lc):
                mg.see(out_ll, lc)
                if out_ll < lc:
                    out_ll, out_k0, out_k1 = lc, c0, c1
    return out_k0, out_k1, nfunk, out_ll, mg.v


def simplex(pr, k0, k1, reltol=RELTOL, max_niter=1000, coeff_correct=True):
    """Simplex for every pair (rows of pr = PrIBDTable's three arrays) from the clamped start values k0 / k1.  Returns dict of k0,
    k1, nfunk, loglik (after LOGLIK_ADJUST) and margin (the decision margin), arrays over the pairs."""
    d0, d1, t2 = nm_prepare(pr)
    P = d0.shape[0]
    out = dict(k0=np.empty(P), k1=np.empty(P), nfunk=np.empty(P, np.int64), loglik=np.empty(P), margin=np.empty(P))
    for r in range(P):
        d = (d0[r], d1[r], t2[r])
        res = _simplex_one(lambda a, b: nm_loglik(d, a, b), float(k0[r]), float(k1[r]), reltol, max_niter, coeff_correct)
        for key, v in zip(("k0", "k1", "nfunk", "loglik", "margin"), res):
            out[key][r] = v
    return out


def simplex_pairs(g, i, j, k0_mom, k1_mom, allele_freq=None, max_niter=1000, reltol=RELTOL, coeff_correct=True):
    """the listed pairs from given method-of-moments values (before the clamp); repeated pairs are walked once"""
    i, j = np.asarray(i), np.asarray(j)
    af = ref.init_afreq(g, allele_freq)
    key, first, inv = np.unique(i.astype(np.int64) * g.shape[1] + j, return_index=True, return_inverse=True)
    s0, s1 = pref.clamp_start(np.asarray(k0_mom)[first], np.asarray(k1_mom)[first])
    r = simplex(ref.pr_table(g, i[first], j[first], af), s0, s1, reltol, max_niter, coeff_correct)
    out = {k: v[inv] for k, v in r.items()}
    out.update(afreq=af)
    return out


# ---- Jacquard ---------------------------------------------------------------------------------------------------------------------
def jacq_table(g, i, j, af):
    """PrIBDTabJacq for every pair (rows) and SNP (columns): array [9][pairs][SNPs].  (MM, MM) is all zero: the reference's entry
    has no break and falls through to the default."""
    a, b = g[:, i].T.astype(np.int64), g[:, j].T.astype(np.int64)
    p = np.broadcast_to(af, a.shape)
    q = 1 - p
    pr = np.zeros((9,) + a.shape)
    ok = (0 < p) & (p < 1)

    def put(ca, cb, vals):
        m = ok & (a == ca) & (b == cb)
        for t, v in vals.items():
            pr[t][m] = v[m]
    put(0, 0, {0: q, 1: q * q, 2: q * q, 4: q * q, 6: q * q, 3: q * q * q, 5: q * q * q, 7: q * q * q, 8: q * q * q * q})
    put(0, 1, {2: p * q, 3: 2 * p * q * q, 7: p * q * q, 8: 2 * p * q * q * q})
    put(0, 2, {1: p * q, 3: p * p * q, 5: p * q * q, 8: p * p * q * q})
    put(1, 0, {4: p * q, 5: 2 * p * q * q, 7: p * q * q, 8: 2 * p * q * q * q})
    put(1, 1, {6: 2 * p * q, 7: p * q, 8: 4 * p * p * q * q})
    put(1, 2, {4: p * q, 5: 2 * p * p * q, 7: p * p * q, 8: 2 * p * p * p * q})
    put(2, 0, {1: p * q, 3: p * q * q, 5: p * p * q, 8: p * p * q * q})
    put(2, 1, {2: p * q, 3: 2 * p * p * q, 7: p * p * q, 8: 2 * p * p * p * q})
    return pr


def jacq_start(P):
    """IBD_Jacq_InitVal and D9 as the left-to-right chain 1 - D1 - ... - D8: array [9][P]"""
    D = np.full((9, P), 0.01)
    d9 = 1.0
    for t in range(8):
        d9 = d9 - 0.01
    D[8] = d9
    return D


def _jacq_sum(pr, D):
    s = pr[0] * D[0][:, None]
    for t in range(1, 9):
        s = s + pr[t] * D[t][:, None]
    return s


def jacq_loglik(pr, D):
    """EM_Jacq_LogLik per pair; -Inf when a sum is not > 0 where Pr9 > 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = _jacq_sum(pr, D)
        pos = s > 0
        ll = np.where(pos, np.log(np.where(pos, s, 1.0)), 0.0).sum(1)
    bad = ((~pos) & (pr[8] > 0)).any(1)
    return np.where(bad, -np.inf, ll)


def jacquard(pr, max_niter=1000, reltol=RELTOL):
    """EM_Jacq_Alg for every pair (pr = jacq_table's array).  Returns dict of D [8][pairs], loglik, niter, stop_margin (the smallest
    | |dLogLik| - ConvTol | over a pair's iterations), as ibd_mle_ref.em does."""
    P = pr.shape[1]
    D = jacq_start(P)
    L0 = jacq_loglik(pr, D)
    fin = np.isfinite(L0)
    tol = np.where(fin, reltol * (np.abs(np.where(fin, L0, 0)) + abs(reltol)), reltol)
    tol = np.where(tol < 0, 0, tol)
    out_D = D.copy()
    out_ll = np.where(fin, L0, 1e8)
    niter = np.full(P, max_niter, np.int64)
    margin = np.full(P, np.inf)
    old = np.zeros(P)
    active = np.arange(P) if max_niter >= 0 else np.arange(0)
    it = 0
    while active.size and it <= max_niter:
        m = pr[:, active] * D[:, active][:, :, None]
        ms = m[0]
        for t in range(1, 9):
            ms = ms + m[t]
        pos = ms > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            den = np.where(pos, ms, 1)
            S = np.where(pos, m / den, 0).sum(2)
            L = np.where(pos, np.log(den), 0).sum(1)
            nD = S / pos.sum(1)
        d = np.abs(L - old[active]) - tol[active]
        margin[active] = np.minimum(margin[active], np.abs(d))
        stop = d <= 0
        s_idx = active[stop]
        out_D[:, s_idx] = D[:, s_idx]
        out_ll[s_idx] = L[stop]
        niter[s_idx] = it
        go = active[~stop]
        old[go] = L[~stop]
        D[:, go] = nD[:, ~stop]
        if it == max_niter:
            out_D[:, go] = D[:, go]
            out_ll[go] = L[~stop]
        active = go
        it += 1
    return dict(D=out_D[:8], loglik=out_ll, niter=niter, stop_margin=margin)


def jacquard_pairs(g, i, j, allele_freq=None, max_niter=1000, reltol=RELTOL, chunk=64):
    """the listed pairs (any order, repeats allowed; (j, i) is NOT (i, j)): dict of D [8][pairs], loglik, niter, stop_margin, afreq"""
    i, j = np.asarray(i), np.asarray(j)
    af = ref.init_afreq(g, allele_freq)
    key, first, inv = np.unique(i.astype(np.int64) * g.shape[1] + j, return_index=True, return_inverse=True)
    ui, uj = i[first], j[first]
    parts = [jacquard(jacq_table(g, ui[c:c + chunk], uj[c:c + chunk], af), max_niter, reltol) for c in range(0, len(ui), chunk)]
    out = dict(D=np.concatenate([r["D"] for r in parts], 1)[:, inv])
    for k in ("loglik", "niter", "stop_margin"):
        out[k] = np.concatenate([r[k] for r in parts])[inv]
    out.update(afreq=af)
    return out


def swap_samples(D):
    """what listing every pair as (j, i) does to D1 ... D8: D3 <-> D5 and D4 <-> D6 (hom/het and the opposite homozygotes' third
    and fifth states change sides); D1, D2, D7, D8 stay"""
    return D[[0, 1, 4, 5, 2, 3, 6, 7]]


# ---- transcriptions ---------------------------------------------------------------------------------------------------------------
def _pr_tab_jacq(g1, g2, p):
    """PrIBDTabJacq, :864-939, fall-through included"""
    Pr = [0.0] * 9
    if 0 < p < 1:
        q = 1 - p
        if g1 == 0:
            if g2 == 0:
                Pr[0] = q
                Pr[1] = Pr[2] = Pr[4] = Pr[6] = q * q
                Pr[3] = Pr[5] = Pr[7] = q * q * q
                Pr[8] = q * q * q * q
            elif g2 == 1:
                Pr[2] = p * q; Pr[3] = 2 * p * q * q
                Pr[7] = p * q * q; Pr[8] = 2 * p * q * q * q
            elif g2 == 2:
                Pr[1] = p * q; Pr[3] = p * p * q
                Pr[5] = p * q * q; Pr[8] = p * p * q * q
        elif g1 == 1:
            if g2 == 0:
                Pr[4] = p * q; Pr[5] = 2 * p * q * q
                Pr[7] = p * q * q; Pr[8] = 2 * p * q * q * q
            elif g2 == 1:
                Pr[6] = 2 * p * q; Pr[7] = p * q
                Pr[8] = 4 * p * p * q * q
            elif g2 == 2:
                Pr[4] = p * q; Pr[5] = 2 * p * p * q
                Pr[7] = p * p * q; Pr[8] = 2 * p * p * p * q
        elif g1 == 2:
            if g2 == 0:
                Pr[1] = p * q; Pr[3] = p * q * q
                Pr[5] = p * p * q; Pr[8] = p * p * q * q
            elif g2 == 1:
                Pr[2] = p * q; Pr[3] = 2 * p * p * q
                Pr[7] = p * p * q; Pr[8] = 2 * p * p * p * q
            elif g2 == 2:
                Pr[0] = p
                Pr[1] = Pr[2] = Pr[4] = Pr[6] = p * p
                Pr[3] = Pr[5] = Pr[7] = p * p * p
                Pr[8] = p * p * p * p
                Pr = [0.0] * 9              # no break: falls through to default
    return Pr


def _em_jacq(pr, max_niter, reltol):
    """EM_Jacq_Alg on a list of nine-entry rows from IBD_Jacq_InitVal: (D1 ... D8, loglik, niter)"""
    par = [0.01] * 8
    D = par + [1 - par[0] - par[1] - par[2] - par[3] - par[4] - par[5] - par[6] - par[7]]
    # EM_Jacq_LogLik
    L = 0.0
    for p in pr:
        s = (p[0] * D[0] + p[1] * D[1] + p[2] * D[2] + p[3] * D[3] + p[4] * D[4] + p[5] * D[5] + p[6] * D[6] + p[7] * D[7]
             + p[8] * D[8])
        if s > 0:
            L += math.log(s)
        elif p[8] > 0:
            L = -math.inf
            break
    old = 0.0
    if math.isfinite(L):
        tol = reltol * (abs(L) + abs(reltol))
        if tol < 0:
            tol = 0
    else:
        L = 1e8
        tol = reltol
    niter = max_niter
    for it in range(0, max_niter + 1):
        oldD = list(D)
        sm = [0.0] * 9
        ns = 0
        L = 0.0
        for p in pr:
            m = [p[t] * D[t] for t in range(9)]
            ms = m[0] + m[1] + m[2] + m[3] + m[4] + m[5] + m[6] + m[7] + m[8]
            if ms > 0:
                for t in range(9):
                    sm[t] += m[t] / ms
                ns += 1
                L += math.log(ms)
        D = [pref._div(sm[t], ns) for t in range(9)]
        if abs(L - old) <= tol:
            D = oldD
            niter = it
            break
        old = L
    return D[:8], L, niter


def _nm_loglik(prn, k0, k1):
    """NM_LogLik on a list of (d0, d1, t2), :687-727"""
    if (k0 < 0) or (k1 < 0) or (k0 + k1 > 1):
        return -math.inf
    ll = 0.0
    for t in prn:
        s = t[0] * k0 + t[1] * k1 + t[2]
        if s > 0:
            ll += math.log(s)
        elif t[0] > 0:
            return -math.inf
    return ll


def _simplex(g1, g2, af, k0, k1, reltol, max_niter, coeff_correct):
    """NM_Prepare + Simplex on two code vectors from the clamped start values: (k0, k1, nfunk, loglik, margin)"""
    prn = []
    for x, y, p in zip(g1, g2, af):
        t = pref._pr_ibd_table(int(x), int(y), float(p))
        prn.append((t[0] - t[2], t[1] - t[2], t[2]))
    return _simplex_one(lambda a, b: _nm_loglik(prn, a, b), k0, k1, reltol, max_niter, coeff_correct)


# ---- the inputs of tests/test_gpu_ibd_methods.py ----------------------------------------------------------------------------------
# Samples 20 and 21 are children of samples 0 and 1 (parent-offspring with 0 and 1, full sibs of each other), samples 22 and 19 each
# carry two identical haplotypes (no heterozygous call), sample 18 is a child of 22 and 4, sample 23 repeats sample 3.  Between them
# the listed relatives move every one of D1 ... D8 away from its start value.
PARENTS, CHILDREN, INBRED, INBRED2, INBRED_CHILD, TWIN = (0, 1), (20, 21), 22, 19, 18, (3, 23)
_geno_cache = {}


def family_genotypes(m, missing=0.05):
    """(packed rows, codes g) of pref.N_SAMP samples x m SNPs with the relatives above; computed once and shared read-only"""
    if (m, missing) in _geno_cache:
        return _geno_cache[(m, missing)]
    from oracle.synth import synth_hash_block_packed
    from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows
    n = pref.N_SAMP
    g = unpack_2bit_rows(synth_hash_block_packed(n, 0, m, 11 + n + m, 0.0, 0, False), n).copy()
    rng = np.random.default_rng(1000 + m)

    def gamete(s):
        return np.where(g[:, s] == 1, rng.integers(0, 2, m), g[:, s] // 2)
    for c in CHILDREN:
        g[:, c] = gamete(PARENTS[0]) + gamete(PARENTS[1])
    g[:, INBRED] = 2 * gamete(INBRED)
    g[:, INBRED2] = 2 * gamete(INBRED2)
    g[:, INBRED_CHILD] = gamete(INBRED) + gamete(4)
    g[:, TWIN[1]] = g[:, TWIN[0]]
    g[rng.random(g.shape) < missing] = 3
    g = g.astype(np.uint8)
    g.setflags(write=False)
    p = pack_2bit_rows(g)
    p.setflags(write=False)
    _geno_cache[(m, missing)] = (p, g)
    return p, g


def special_freq(m):
    """frequencies with NaN, 0, 1, values outside [0, 1], as pref.case_inputs"""
    af = np.random.default_rng(pref.N_SAMP).uniform(0.05, 0.95, m)
    af[:: 5][:4] = [np.nan, 0.0, 1.0, 1.5][: len(af[:: 5][:4])]
    if m > 12:
        af[12] = -0.2
    return af


def listed_pairs(m, count):
    """`count` pairs: the relatives first, then random ones (i == j, i > j and repeats among them)"""
    fixed = [(0, 20), (20, 1), (20, 21), (INBRED, INBRED), (INBRED, 5), (5, INBRED), TWIN, (0, 20), (INBRED, INBRED2),
             (INBRED, INBRED_CHILD), (INBRED_CHILD, INBRED)]
    rng = np.random.default_rng(m)
    n = pref.N_SAMP
    i = np.concatenate([[a for a, _ in fixed], rng.integers(0, n, count - len(fixed))])
    j = np.concatenate([[b for _, b in fixed], rng.integers(0, n, count - len(fixed))])
    return i.astype(np.int64), j.astype(np.int64)


# n_snp, special allele_freq, max_niter, reltol (None: the default), coeff_correct.  The SNP counts straddle the 16-SNP word and the
# 64-lane x 16-SNP step of the lane-split sweep.
SIMPLEX_CASES = [
    (1, False, 1000, None, True),
    (15, False, 1000, None, False),
    (16, False, 1000, None, True),
    (17, False, 1000, None, True),
    (1023, False, 0, None, True),
    (1024, False, 5, None, True),
    (1025, False, 1000, 1e-4, True),
    (1025, True, 1000, None, True),
    (2049, False, 1000, None, False),
    (2049, False, 1000, None, True),
]
JACQUARD_CASES = [
    (1, False, 1000, None),
    (15, False, 1000, None),
    (16, False, 1000, None),
    (17, False, 1000, None),
    (1023, False, 0, None),
    (1024, False, 5, None),
    (1025, False, 1000, 1e-4),
    (1025, True, 1000, None),
    (2049, False, 1000, None),
]
N_SIMPLEX = 200


def n_jacquard(m):
    return 200 if m < 1023 else 64
