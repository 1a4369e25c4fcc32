"""Extended-precision references of the PCA projections (csrc/kernels_proj.hip), each with the error bound the kernels are held to.

A loading is a sum of n_terms products y_i e_i: y_i the centred and scaled genotype of one call (0 for a missing one), e_i the operand
the caller handed over as a double.  The references form y and the sum in np.longdouble (64 mantissa bits; where the platform's long
double has fewer, the exact products of double y and e are summed with math.fsum) and return with every entry

    B = (n_terms + 8) 2^-53 sum_i |y_i| |e_i|.

Any order of n_terms - 1 fp64 additions stays within (n_terms - 1) 2^-53 of that sum of magnitudes to first order, so the bound holds
for the kernels' split ranges and atomics as it does for a loop; a fused multiply-add rounds once per term, which the same count
covers.  The 8 is for what happens outside the sum: a last bit of avg (one division) and of scale (a square root, a division) where
the device's differ from the host's, the roundings of y (a difference and a product) and the final store.  n_terms is the number of
samples on the SNP side and the number of SNPs fed on the sample side.

Operands are taken as the doubles the device gets: eigenvectors as handed to set_eigvec, sload / avg / scale as handed to the feed.
The per-SNP avg and scale of the PCA loadings are results of their own, defined by the reference's double formula (and compared at
rtol 1e-14): snp_stats forms them in double by those operations, the loadings are then summed in long double from them.  (The
formula is not accurate to 1e-14 everywhere: the Bayesian scale of a SNP whose c calls are all 2 loses log2(c) bits in 1 - p, in the
reference as here -- 4.6e-13 against the exact value at 16 400 samples.)
The *_like_oracle wrappers scale the operands the way oracle.pca_snp_loading and its kin do, so that the two can be compared."""
import math

import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63
U = 2.0 ** -53


def _two_prod(a, b):
    """a * b = p + q exactly (Dekker / Veltkamp), elementwise on doubles of moderate size"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _sum_products(y, e, extended=None):
    """y [r][n] (long double, or double without one) times e [k][n] -> [r][k], as doubles rounded once"""
    if EXTENDED if extended is None else extended:
        return np.asarray(np.asarray(y, LD) @ np.asarray(e, LD).T, np.float64)
    y, e = np.asarray(y, np.float64), np.asarray(e, np.float64)
    out = np.empty((y.shape[0], e.shape[0]), np.float64)
    for r in range(y.shape[0]):
        p, q = _two_prod(y[r][None, :], e)
        for j in range(e.shape[0]):
            out[r, j] = math.fsum(np.concatenate([p[j], q[j]]).tolist())
    return out


def _bound(y, e, n_terms):
    return (n_terms + 8) * U * (np.abs(np.asarray(y, np.float64)) @ np.abs(np.asarray(e, np.float64)).T)


def snp_stats(g, bayesian=False):
    """per-SNP average genotype and scale of CPCA_SNPLoad (0 and 0 without a call; scale 0 for a monomorphic SNP unless Bayesian), in
    double by the reference's own operations in their order: these are results the caller gets and parity is defined on them"""
    g = np.asarray(g)
    valid = g < 3
    s = np.where(valid, g, 0).sum(axis=1).astype(np.float64)
    c = valid.sum(axis=1).astype(np.float64)
    some = c > 0
    cs = np.where(some, c, 1.0)
    avg = np.where(some, s / cs, 0.0)
    p = (s + 1) / (2 * cs + 2) if bayesian else avg * 0.5
    ok = some if bayesian else some & (0.0 < p) & (p < 1.0)
    scale = np.where(ok, 1.0 / np.sqrt(np.where(ok, p * (1.0 - p), 1.0)), 0.0)
    return avg, scale


def _centred(g, avg, scale, extended=None):
    ext = EXTENDED if extended is None else extended
    T = LD if ext else np.float64
    g = np.asarray(g)
    return np.where(g < 3, (g.astype(T) - np.asarray(avg, T)[:, None]) * np.asarray(scale, T)[:, None], 0)


def snp_loading(g, eigvec, bayesian=False, avg=None, scale=None, extended=None):
    """g uint8 [L][n], eigvec [k][n] as set on the projector -> (loading [L][k], avg [L], scale [L], bound [L][k]); with avg and
    scale given (the caller's centring and scaling, doubles) they are used as they are"""
    if avg is None:
        avg, scale = snp_stats(g, bayesian)
    y = _centred(g, avg, scale, extended)
    return (_sum_products(y, eigvec, extended), np.asarray(avg, np.float64), np.asarray(scale, np.float64),
            _bound(y, eigvec, np.asarray(g).shape[1]))


def samp_loading(g, sload, avg, scale, extended=None):
    """g uint8 [L][n], sload [L][k], avg / scale [L] as fed -> (sample loadings [k][n], bound [k][n]) of these L SNPs"""
    y = _centred(g, avg, scale, extended)
    st = np.ascontiguousarray(np.asarray(sload, np.float64).T)
    return _sum_products(y.T, st, extended).T, _bound(y.T, st, np.asarray(g).shape[0]).T


def add_feeds(parts):
    """sample loadings of several feeds: the sums of the references and of their bounds (one more addition per feed: within the 8)"""
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


# ---- the operands as oracle/__init__.py forms them ---------------------------------------------------------------------------------

def pca_eigvec_scaled(eigenval, eigenvect, trace_xtx):
    """gnrPCASNPLoading's scaling of the eigenvectors, the same double operations in the same order as csrc/workspace.hip"""
    ev = np.asarray(eigenvect, np.float64)
    return ev * np.sqrt((ev.shape[1] - 1) / trace_xtx / np.asarray(eigenval, np.float64))[:, None]


def eigmix_norm(afreq):
    """(avg [L], scale [L]) of the EIGMIX loadings: 2 p and 1 / sqrt(sum 4 p (1 - p))"""
    af = np.asarray(afreq, np.float64)
    return 2 * af, np.full(af.shape, 1.0 / np.sqrt(np.sum(4 * af * (1 - af))))


def pca_snp_loading_like_oracle(g, eigenval, eigenvect, trace_xtx, bayesian=False):
    return snp_loading(g, pca_eigvec_scaled(eigenval, eigenvect, trace_xtx), bayesian)[:3]


def eigmix_snp_loading_like_oracle(g, eigenval, eigenvect, afreq):
    ev = np.asarray(eigenvect, np.float64) * np.sqrt(1 / np.asarray(eigenval, np.float64))[:, None]
    return snp_loading(g, ev, avg=eigmix_norm(afreq)[0], scale=eigmix_norm(afreq)[1])[0]


def eigmix_samp_loading_like_oracle(g, sload, afreq):
    return samp_loading(g, sload, *eigmix_norm(afreq))[0]


# ---- correlations: what the reference's one-pass moment formula leaves of an entry ---------------------------------------------------

def corr_margin(g, eigvec):
    """Per entry [L][k] of oracle.pca_snp_corr: (degenerate, margin).  degenerate: the entry is NaN because of exactly representable
    constants -- fewer than two calls, called genotypes all equal (m YY - Y^2 = 0 in integers), or an eigenvector constant over the
    calls, whose moments are then exact.  margin: val / (XX YY) elsewhere (1 where degenerate), val = (XX - X^2 / m) (YY - Y^2 / m) being
    what the formula tests against 0: a margin far above the rounding of X^2 / m and Y^2 / m puts the entry clear of that edge."""
    g = np.asarray(g)
    e = np.asarray(eigvec, np.float64)
    valid = g < 3
    v = valid.astype(np.float64)
    y = np.where(valid, g, 0).astype(np.int64)
    m, Y, YY = valid.sum(axis=1), y.sum(axis=1), (y * y).sum(axis=1)
    hi = np.where(valid[:, None, :], e[None], -np.inf).max(axis=2)
    lo = np.where(valid[:, None, :], e[None], np.inf).min(axis=2)
    const = hi <= lo
    degenerate = ((m <= 1) | (m * YY - Y * Y == 0))[:, None] | const
    md = np.maximum(m, 1).astype(np.float64)[:, None]
    X, XX = v @ e.T, v @ (e * e).T
    val = (XX - X * X / md) * (YY[:, None] - (Y * Y)[:, None] / md)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(degenerate, 1.0, val / (XX * YY[:, None]))
    return degenerate, margin
