"""Sequential fp64 restatements of the individual inbreeding coefficients of gnrIndInb, written from the formulas.

Moment methods.  With p the frequency of the counted allele at a SNP, h = 2 p (1 - p) and g the genotype of a sample there:
    mom.weir       F = sum (g^2 - g (1 + 2 p) + 2 p^2) / sum h            over the SNPs the sample is called at
    mom.visscher   F = mean of (g^2 - g (1 + 2 p) + 2 p^2) / h            (= gcta3)
    gcta1          F = mean of (g - 2 p)^2 / h - 1
    gcta2          F = mean of 1 - g (2 - g) / h                          over the called SNPs where the value is finite
p = (sum of called g) / (called samples) * 0.5 unless given.  Every sample's sum runs over the SNPs in ascending order.

MLE.  F maximises sum log P(g | F, p) with P(0) = (1-F)(1-p)^2 + F(1-p), P(1) = (1-F) 2 p (1-p), P(2) = (1-F) p^2 + F p by the EM
update F <- mean of the posterior of autozygosity (F / (F + (1-p)(1-F)) for g = 0, 0 for g = 1, F / (F + p (1-F)) for g = 2),
started at the mom.weir ratio clamped to [0.001, 0.999] and stopped once the log-likelihood moves by no more than
reltol |loglik at the start| or after 10 000 updates (then 10 001 is reported).  Non-finite terms are skipped.

np.cumsum(x)[-1] is the sequential left-to-right sum; the other orders serve to measure how far a reordered sum can move."""
import numpy as np

METHODS = ("mom.weir", "mom.visscher", "mle", "gcta1", "gcta2", "gcta3")


def calc_afreq(g):
    """per SNP (rows of g, uint8, > 2 = missing): sum / num * 0.5; NaN without a call"""
    g = np.asarray(g)
    called = g <= 2
    s = np.where(called, g, 0).sum(1).astype(np.float64)
    n = called.sum(1).astype(np.float64)
    with np.errstate(all="ignore"):
        return s / n * 0.5


def snp_freq(g):
    """per SNP: sum / (2 num), the frequency the MLE uses when none is given"""
    g = np.asarray(g)
    called = g <= 2
    s = np.where(called, g, 0).sum(1).astype(np.float64)
    n = (2 * called.sum(1)).astype(np.float64)
    with np.errstate(all="ignore"):
        return s / n


def moment_values(method, p):
    """per SNP the value a genotype 0 / 1 / 2 adds: [M][3], and h [M]"""
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        h = 2 * p * (1 - p)
        p1, p2 = 1 + 2 * p, 2 * p * p
        v = np.empty((len(p), 3), np.float64)
        for g in range(3):
            if method == "gcta1":
                x = g - 2 * p
                v[:, g] = x * x / h - 1
            elif method == "gcta2":
                v[:, g] = 1 - g * (2 - g) / h
            elif method == "mom.weir":
                v[:, g] = g * g - g * p1 + p2
            else:
                v[:, g] = (g * g - g * p1 + p2) / h
    return v, h


def ind_inb_moment_ref(g, method, allele_freq=None):
    """g: uint8 [M][N]; returns (coeff [N], p [M]); sums over the SNPs in ascending order for every sample"""
    g = np.asarray(g, np.uint8)
    M, N = g.shape
    p = calc_afreq(g) if allele_freq is None else np.asarray(allele_freq, np.float64)
    v, h = moment_values(method, p)
    acc = np.zeros(N, np.float64)
    den = np.zeros(N, np.float64)
    cnt = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for l in range(M):
            called = g[l] <= 2
            val = v[l][np.minimum(g[l], 2)]
            if method == "mom.weir":
                acc[called] += val[called]
                den[called] += h[l]
            else:
                ok = called & np.isfinite(val)
                acc[ok] += val[ok]
                cnt[ok] += 1
        return (acc / den if method == "mom.weir" else acc / cnt.astype(np.float64)), p


def _sum(x, order):
    if len(x) == 0:
        return 0.0
    if order == "seq":
        return float(np.cumsum(x)[-1])
    if order == "reversed":
        return float(np.cumsum(x[::-1])[-1])
    if order == "pairwise":
        return float(np.sum(x))
    if order == "longdouble":
        return float(np.sum(x.astype(np.longdouble)))
    raise ValueError(order)


def _mle_steps(g, p, order):
    """The iteration of one sample with its sums taken in `order`: yields (F_k, loglik(F_k)) for k = 0, 1, ... without end; the
    first item is (start value, None) and the only one when the start value is not finite."""
    g = np.asarray(g)
    p = np.asarray(p, np.float64)
    called = g <= 2
    gc, pc = g[called].astype(np.float64), p[called]
    with np.errstate(all="ignore"):
        F = float(np.float64(_sum(gc * gc - (1 + 2 * pc) * gc + 2 * pc * pc, order)) / np.float64(_sum(2 * pc * (1 - pc), order)))
        yield F, None
        if not np.isfinite(F):
            return
        F = min(max(F, 0.001), 1 - 0.001)
        het, hom = gc == 1, gc != 1
        x = np.where(gc == 0, 1 - pc, pc)
        n_het = int(het.sum())
        while True:
            val = np.log(np.where(het, (1 - F) * 2 * pc * (1 - pc), (1 - F) * x * x + F * x))
            yield F, _sum(val[np.isfinite(val)], order)
            tmp = (F / (F + x * (1 - F)))[hom]
            ok = np.isfinite(tmp)
            F = float(np.float64(_sum(tmp[ok], order)) / np.float64(int(ok.sum()) + n_het))


def mle_ref(g, p, reltol, order="seq", force_iter=None, max_iter=10000):
    """One sample: g [M] (> 2 = missing), p [M].  dict(F, niter, loglik, margin, F_forced):
    margin = the smallest | |dLogLik| - contol | over the iterations; F_forced = F after exactly force_iter updates (the stop
    test ignored), when asked for.  niter = -1 and F as it is when the start value is not finite."""
    steps = _mle_steps(g, p, order)
    F, _ = next(steps)
    out = dict(F=F, niter=-1, loglik=float("nan"), margin=float("inf"), F_forced=F if force_iter is not None else None)
    if not np.isfinite(F):
        return out
    if force_iter is not None:
        forced = _mle_steps(g, p, order)
        next(forced)
        for _ in range(int(min(force_iter, max_iter)) + 1):
            out["F_forced"] = next(forced)[0]
    F, L = next(steps)
    contol = abs(L) * reltol
    margin = float("inf")
    it = 1
    while it <= max_iter:
        old = L
        F, L = next(steps)
        d = abs(L - old)
        margin = min(margin, abs(d - contol))
        if d <= contol:
            break
        it += 1
    out.update(F=F, niter=it, loglik=L, margin=margin)
    return out


def mle_trace(g, p, reltol, order, n_iter):
    """F_k and loglik(F_k) for k = 0 ... n_iter of one sample (the stop test ignored), sums taken in `order`; None when the start
    value is not finite"""
    steps = _mle_steps(g, p, order)
    if not np.isfinite(next(steps)[0]):
        return None
    tr = [next(steps) for _ in range(n_iter + 1)]
    return np.array([t[0] for t in tr]), np.array([t[1] for t in tr])


def ind_inb_coef_r(x, p, method):
    """the R-level formulas of snpgdsIndInbCoef (vectorised; sums in numpy's order)"""
    x = np.asarray(x, np.float64).copy()
    p = np.asarray(p, np.float64)
    x[~np.isin(x, (0, 1, 2))] = np.nan
    with np.errstate(all="ignore"):
        num = x * x - (1 + 2 * p) * x + 2 * p * p
        den = 2 * p * (1 - p)
        if method == "mom.weir":
            f = np.isfinite(num) & np.isfinite(den)
            return float(num[f].sum() / den[f].sum())
        d = num / den
        return float(d[np.isfinite(d)].mean())
