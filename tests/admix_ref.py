"""The EM for ancestry proportions (include/snpgpu.h section 1s) restated in numpy, its bounds and a generator.

The definitions, over the called genotypes only (a code of 3 contributes nothing anywhere), G [m][n] codes, Q [n][K], F [m][K]:

    h1_ij = sum_k q_ik f_kj            h0_ij = sum_k q_ik (1 - f_kj)      (h0 as its own sum of positive terms, not 1 - h1)
    w1_ij = g_ij / h1_ij               w0_ij = (2 - g_ij) / h0_ij
    a_ik  = sum_j (w1_ij f_kj + w0_ij (1 - f_kj))      q'_ik = q_ik a_ik / sum_k' q_ik' a_ik'   (no called SNP: the row stays)
    u_kj  = f_kj sum_i w1_ij q_ik      v_kj = (1 - f_kj) sum_i w0_ij q_ik
    f'_kj = clamp(u_kj / (u_kj + v_kj), f_min, 1 - f_min)                                        (u + v = 0: f_kj stays)
    L(Q, F) = sum_ij g_ij log h1_ij + (2 - g_ij) log h0_ij

`em_step` evaluates them as written in the dtype it is given (float64 or long double); `order` = (a permutation of the samples, one
of the SNPs) changes the order of every sum and nothing else.

The bounds the device is held to.  With u = 2^-53 and EPS = 2^-52 = 2 u: every one of a_ik, u_kj, v_kj is a sum of T non-negative
terms (T = the called SNPs of sample i, the called samples of SNP j).  A term is made from float64 inputs by at most K + 6 roundings
-- K for the sum h of K non-negative products (each product and each addition rounds; fused or not, a sum of non-negative terms
keeps a relative error of at most one rounding per term), one for 1 - f, one for the division, one for the product with f or q,
and up to three for adding the two halves of a term of a or multiplying the finished sum by f -- so its relative error is at most
(K + 6) u (1 + O(u)), and adding T such terms in ANY order adds at most (T - 1) u relative to their sum, all terms being
non-negative.  Two evaluations (the device's and the long-double reference's, whose own error is 2^-11 of this) therefore differ by at
most (T + K + 5) u relative; the bound used is

    sum_bound(T, K) = (T + 2 K + 16) EPS        relative, about four times that, as DESIGN.md 32 states it.

For L the terms g log h1 and (2 - g) log h0 are not positive and the rounding of h enters log h absolutely, so the bound is taken
relative to the sum of their magnitudes: |L_a - L_b| <= sum_bound(T, K) sum |terms| with T all called genotypes.  q' = x_k / sum_k x_k
with x_k = q_k a_k: numerator and denominator (K non-negative terms) each carry the relative error of a plus K + 1 roundings, the
quotient one more, so q' is within

    q_bound(T, K) = 2 sum_bound(T, K) + (K + 3) EPS      relative,

and its rows sum to 1 within (K + 2) EPS: S = fl(sum x_k) = (sum x_k)(1 + t), |t| <= (K - 1) u, and fl(x_k / S) = x_k / S (1 + d),
|d| <= u, give |sum_k q'_k - 1| <= K u (1 + O(u)).  f' before the clamp is u / (u + v), within f_bound(T, K) = 2 sum_bound(T, K) + 4 EPS
relative; the clamp is a contraction, so after it the absolute error is at most that of the unclamped value.  None of these
figures was tuned to what a device gives.
"""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def sum_bound(T, K):
    return (np.asarray(T, np.float64) + 2 * K + 16) * EPS


def q_bound(T, K):
    return 2 * sum_bound(T, K) + (K + 3) * EPS


def f_bound(T, K):
    return 2 * sum_bound(T, K) + 4 * EPS


def row_sum_bound(K):
    return (K + 2) * EPS


def worst(x, y, bound, scale=None):
    """max over the entries of |x - y| / (scale * bound), scale = |y| unless given: <= 1 means within the bound.  Where the scale is 0
    the two must be equal; NaN entries of the scale are left out."""
    x, y = np.asarray(x, LD), np.asarray(y, LD)
    scale = np.abs(y) if scale is None else np.asarray(scale, LD)
    bound = np.broadcast_to(np.asarray(bound, LD), y.shape)
    keep = ~np.isnan(scale)
    x, y, scale, bound = x[keep], y[keep], scale[keep], bound[keep]
    if x.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(x - y) / (scale * bound)
    e = np.where(scale == 0, np.where(x == y, 0.0, np.inf), e)
    return float(np.max(e))


def called_counts(G):
    """(called SNPs per sample [n], called samples per SNP [m], all called genotypes)"""
    c = np.asarray(G) != 3
    return c.sum(axis=0), c.sum(axis=1), int(c.sum())


def em_step(G, Q, F, f_min, dtype=np.float64, fix_f=False, order=None):
    """One iteration from (Q, F) and the likelihood of (Q, F).  G [m][n] codes 0 / 1 / 2 / 3.  Returns dict(Q, F: the new state; L;
    Labs = sum |terms of L|; a [n][K]; u, v [m][K]; Fraw: f' before the clamp, NaN where u + v = 0)."""
    G = np.asarray(G)
    m, n = G.shape
    if order is not None:
        pi, pj = order
        r = em_step(G[np.ix_(pj, pi)], np.asarray(Q)[pi], np.asarray(F)[pj], f_min, dtype, fix_f)
        ii, jj = np.argsort(pi), np.argsort(pj)
        out = dict(r)
        for k in ("Q", "a"):
            out[k] = r[k][ii]
        for k in ("F", "u", "v", "Fraw"):
            out[k] = r[k][jj]
        return out
    Q = np.asarray(Q, dtype)
    F = np.asarray(F, dtype)
    K = Q.shape[1]
    one = dtype(1)
    called = (G != 3).T                                     # [n][m]
    g = np.where(called, G.T, 0).astype(dtype)
    g2 = np.where(called, 2 - G.T.astype(np.int64), 0).astype(dtype)
    Fc = one - F
    h1 = np.zeros((n, m), dtype)
    h0 = np.zeros((n, m), dtype)
    for k in range(K):
        h1 += Q[:, k, None] * F[None, :, k]
        h0 += Q[:, k, None] * Fc[None, :, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = np.where(called, g / h1, dtype(0))
        w0 = np.where(called, g2 / h0, dtype(0))
        terms = np.where(called, g * np.log(h1) + g2 * np.log(h0), dtype(0))
    L = terms.sum()
    Labs = np.abs(terms).sum()
    a = np.empty((n, K), dtype)
    u = np.empty((m, K), dtype)
    v = np.empty((m, K), dtype)
    for k in range(K):
        a[:, k] = (w1 * F[None, :, k] + w0 * Fc[None, :, k]).sum(axis=1)
        u[:, k] = F[:, k] * (w1 * Q[:, k, None]).sum(axis=0)
        v[:, k] = Fc[:, k] * (w0 * Q[:, k, None]).sum(axis=0)
    x = Q * a
    s = x.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        Qn = np.where(s > 0, x / s, Q)
        d = u + v
        Fraw = np.where(d > 0, u / d, dtype(np.nan))
    lo, hi = dtype(np.float64(f_min)), dtype(np.float64(1.0) - np.float64(f_min))
    Fn = np.where(d > 0, np.clip(Fraw, lo, hi), F)
    if fix_f:
        Fn = F.copy()
    return dict(Q=Qn, F=Fn, L=L, Labs=Labs, a=a, u=u, v=v, Fraw=Fraw)


def loglik(G, Q, F, dtype=np.float64):
    r = em_step(G, Q, F, 0.25, dtype, fix_f=True)
    return r["L"], r["Labs"]


def em_run(G, Q, F, f_min, max_iter, tol, fix_f=False, dtype=np.float64):
    """snpgpu_admix_run restated: (Q, F, trace [n_done + 1], n_done).  trace[t] = L of the state before iteration t; it stops after
    iteration t >= 1 when trace[t] - trace[t - 1] < tol; the last entry belongs to the returned state."""
    Q, F = np.asarray(Q, dtype), np.asarray(F, dtype)
    trace, done = [], 0
    for t in range(max_iter):
        r = em_step(G, Q, F, f_min, dtype, fix_f)
        trace.append(r["L"])
        Q, F = r["Q"], r["F"]
        done = t + 1
        if t >= 1 and trace[t] - trace[t - 1] < tol:
            break
    trace.append(loglik(G, Q, F, dtype)[0])
    return Q, F, np.array(trace, dtype), done


def prepare_start(Q, F, f_min):
    """what snpgpu_admix_set makes of its arguments: rows of q divided by their sums, f clamped (float64)"""
    Q = np.asarray(Q, np.float64)
    return Q / Q.sum(axis=1, keepdims=True), np.clip(np.asarray(F, np.float64), f_min, 1.0 - f_min)


def admixed_case(n, m, K, seed, missing=0.05, fst=0.1, special=True):
    """A simulated admixed sample: ancestral frequencies uniform on [0.1, 0.9], K populations drifted from them (Balding-Nichols
    with `fst`), Q Dirichlet(0.5) with every fourth sample unadmixed (population i / 4 mod K), genotypes Binomial(2, Q F^T), calls
    missing at rate `missing`.  special (where the shape has room: n >= 4, m >= 4): the last sample has every call missing, the last
    SNP has every call missing, the SNP before it is monomorphic (every genotype 0).
    Returns dict(geno [m][n] uint8, Q, F, none_sample, none_snp, mono_snp) -- the last three None without room."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, m)
    c = (1.0 - fst) / fst
    F = np.clip(rng.beta((p * c)[:, None].repeat(K, 1), ((1 - p) * c)[:, None].repeat(K, 1)), 1e-3, 1 - 1e-3)
    Q = rng.dirichlet(np.full(K, 0.5), n)
    for i in range(0, n, 4):
        Q[i] = 0.0
        Q[i, (i // 4) % K] = 1.0
    h = np.clip(Q @ F.T, 0.0, 1.0)                                              # [n][m]
    g = rng.binomial(2, h).T.astype(np.uint8)                                   # [m][n]
    if missing > 0:
        g[rng.random((m, n)) < missing] = 3
    out = dict(Q=Q, F=F, none_sample=None, none_snp=None, mono_snp=None)
    if special and n >= 4 and m >= 4:
        g[:, n - 1] = 3
        g[m - 1, :] = 3
        g[m - 2, :n - 1] = 0
        out.update(none_sample=n - 1, none_snp=m - 1, mono_snp=m - 2)
    out["geno"] = g
    return out


def awkward_state(n, m, K, seed, f_min):
    """A state to start one step from: Q rows on the simplex with entries that are exactly 0 (every third sample has a zero, never a
    whole row), F uniform on [0.05, 0.95] with entries exactly on both clamps."""
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.ones(K), n)
    for i in range(0, n, 3):
        Q[i, i % K] = 0.0
    Q = Q / Q.sum(axis=1, keepdims=True)
    F = rng.uniform(0.05, 0.95, (m, K))
    for j in range(0, m, 5):
        F[j, j % K] = f_min
        F[j, (j + 1) % K] = 1.0 - f_min
    return Q, F


@functools.lru_cache(maxsize=None)
def stop_case(f_min=1e-6):
    """(G, Q0, F0) of the stopping-rule tests: well separated populations, F at the truth and fixed, Q from 1 / K"""
    c = admixed_case(150, 700, 3, 8, fst=0.3)
    Q0, F0 = prepare_start(np.full((150, 3), 1 / 3), c["F"], f_min)
    for a in (c["geno"], Q0, F0):
        a.setflags(write=False)
    return c["geno"], Q0, F0


def stop_choice(inc):
    """(t, tol) from the increments inc[t - 1] = L_t - L_(t - 1) of a trace: the rule is to stop after iteration t = 6 (seven iterations
    made); tol = the geometric mean of the increments on both sides of it"""
    t = 6
    return t, float(np.sqrt(inc[t - 1] * inc[t - 2]))
