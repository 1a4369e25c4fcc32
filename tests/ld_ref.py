"""numpy reference of snpgdsLDMat (gnrLDMat, src/genLD.cpp:177-525 and :957-1010) for the LD tests.

Tables by int64 one-hot matrix products; the five methods restated in fp64 from the formulas, with the same order of operations
and NaN rules.  Test infrastructure only: nothing in snprelate_amd imports it."""
import numpy as np

METHODS = ("composite", "r", "dprime", "corr", "cov")
DBL_EPS = np.finfo(np.float64).eps


def tables(ga, gb=None):
    """uint8 genotype rows [La][N] (and [Lb][N]; 3 or more = missing) -> int64 [La][Lb][3][3], cell [i, j, a, b] = number of
    samples with genotype a at row i of ga and b at row j of gb."""
    ga = np.asarray(ga)
    gb = ga if gb is None else np.asarray(gb)
    pa = [(ga == a).astype(np.int64) for a in range(3)]
    pb = [(gb == b).astype(np.int64) for b in range(3)]
    t = np.empty((ga.shape[0], gb.shape[0], 3, 3), np.int64)
    for a in range(3):
        for b in range(3):
            t[:, :, a, b] = pa[a] @ pb[b].T
    return t


def _haplo(nAA, nAB, nBA, nBB, nDH2):
    """EM haplotype proportions, src/genLD.cpp:254-331, element-wise (int64 counts in, float64 out)"""
    f = 0.01
    tol_rel = np.sqrt(DBL_EPS)
    tot = (nAA + nAB + nBA + nBB + nDH2).astype(np.float64)
    em = (tot > 0) & (nDH2 > 0)
    pAA, pAB, pBA, pBB = (x / tot for x in (nAA, nAB, nBA, nBB))
    if not em.any():
        return pAA, pAB, pBA, pBB
    e = np.nonzero(em)
    a, b, c, d = (x[e].astype(np.float64) for x in (nAA, nAB, nBA, nBB))
    dh = (nDH2[e] // 2).astype(np.float64)
    T = tot[e]
    div = (nAA[e] + nAB[e] + nBA[e] + nBB[e]).astype(np.float64) + 4.0 * f
    qAA, qAB, qBA, qBB = (a + f) / div, (b + f) / div, (c + f) / div, (d + f) / div

    def plog(v):
        return np.log(v + DBL_EPS)

    def loglik(a, b, c, d, dh, qAA, qAB, qBA, qBB):
        return a * plog(qAA) + b * plog(qAB) + c * plog(qBA) + d * plog(qBB) + dh * plog(qAA * qBB + qAB * qBA)

    old = loglik(a, b, c, d, dh, qAA, qAB, qBA, qBB)
    tol = np.abs(tol_rel * old)
    tol = np.where(tol < DBL_EPS, DBL_EPS, tol)
    # only the pairs still iterating are carried along (`idx`: where they go in `res`); a pair keeps the proportions of the
    # iteration at which it stopped
    res = [qAA.copy(), qAB.copy(), qBA.copy(), qBB.copy()]
    q = [qAA, qAB, qBA, qBB]
    idx = np.arange(a.size)
    for _ in range(1000):
        x, y = q[0] * q[3], q[1] * q[2]
        dAA = x / (x + y) * dh
        dAB = dh - dAA
        q = [(a + dAA) / T, (b + dAB) / T, (c + dAB) / T, (d + dAA) / T]
        ll = loglik(a, b, c, d, dh, *q)
        go = ~(np.abs(ll - old) <= tol)
        old = ll
        if not go.all():
            for r, v in zip(res, q):
                r[idx[~go]] = v[~go]
            a, b, c, d, dh, T, tol, old, idx = (v[go] for v in (a, b, c, d, dh, T, tol, old, idx))
            q = [v[go] for v in q]
        if idx.size == 0:
            break
    for r, v in zip(res, q):
        r[idx] = v
    for full, part in zip((pAA, pAB, pBA, pBB), res):
        full[e] = part
    return pAA, pAB, pBA, pBB


def ld_values(tab, method):
    """int64 tables [...][3][3] -> float64 LD values [...] of `method` (name or gnrLDMat code 1 ... 5)"""
    if not isinstance(method, str):
        method = METHODS[int(method) - 1]
    n = np.asarray(tab, np.int64)
    r0, r1, r2 = (n[..., a, :].sum(-1) for a in range(3))
    c0, c1, c2 = (n[..., :, b].sum(-1) for b in range(3))
    tot = r0 + r1 + r2
    with np.errstate(all="ignore"):
        if method == "composite":
            ft = tot.astype(np.float64)
            delta = (n[..., 2, 2] + n[..., 0, 0] - n[..., 0, 2] - n[..., 2, 0]) / (2 * ft) - \
                (r0 - r2).astype(np.float64) * (c0 - c2).astype(np.float64) / (2.0 * ft * ft)
            pa = (2 * r0 + r1) / (2 * ft)
            pA, pAA = 1 - pa, r2 / ft
            pb = (2 * c0 + c1) / (2 * ft)
            pB, pBB = 1 - pb, c2 / ft
            DA, DB = pAA - pA * pA, pBB - pB * pB
            t = (pA * pa + DA) * (pB * pb + DB)
            return np.where((tot > 0) & (t > 0), delta / np.sqrt(t), np.nan)
        if method in ("r", "dprime"):
            hAA = 2 * n[..., 2, 2] + n[..., 2, 1] + n[..., 1, 2]
            hAB = n[..., 1, 0] + 2 * n[..., 2, 0] + n[..., 2, 1]
            hBA = n[..., 0, 1] + 2 * n[..., 0, 2] + n[..., 1, 2]
            hBB = 2 * n[..., 0, 0] + n[..., 0, 1] + n[..., 1, 0]
            pAA, pAB, pBA, pBB = _haplo(hAA, hAB, hBA, hBB, 2 * n[..., 1, 1])
            pA, p_A, pB, p_B = pAA + pAB, pAA + pBA, pBA + pBB, pAB + pBB
            D = pAA - pA * p_A
            if method == "r":
                return D / np.sqrt(pA * p_A * pB * p_B)
            u1, v1 = pA * p_B, pB * p_A
            u2, v2 = -pA * p_A, -pB * p_B
            den = np.where(D >= 0, np.where(v1 < u1, v1, u1), np.where(u2 < v2, v2, u2))
            return D / den
        X, XX, Y, YY = r1 + 2 * r2, r1 + 4 * r2, c1 + 2 * c2, c1 + 4 * c2
        XY = n[..., 1, 1] + 2 * n[..., 1, 2] + 2 * n[..., 2, 1] + 4 * n[..., 2, 2]
        ft = tot.astype(np.float64)
        if method == "corr":
            d1 = XX - X.astype(np.float64) * X / ft
            d2 = YY - Y.astype(np.float64) * Y / ft
            v = d1 * d2
            return np.where((tot > 0) & (v > 0), (XY - X.astype(np.float64) * Y / ft) / np.sqrt(v), np.nan)
        if method == "cov":
            return np.where(tot > 1, (XY - X.astype(np.float64) * Y / ft) / (ft - 1), np.nan)
    raise ValueError("unknown LD method %r" % (method,))


def out_dims(n_snp, slide, mat_trim):
    if slide <= 0:
        return n_snp, n_snp
    slide = min(slide, n_snp)
    return slide, (n_snp - slide if mat_trim else n_snp)


def ld_mat(g, method, slide=-1, mat_trim=False):
    """gnrLDMat's result for uint8 genotype rows g [L][N], as R's (rows, cols) matrix"""
    g = np.asarray(g)
    L = g.shape[0]
    if slide <= 0:
        t = tables(g)
        iu = np.triu_indices(L)
        v = ld_values(t[iu], method)          # each unordered pair once, oriented (min, max), as the reference
        m = np.empty((L, L))
        m[iu] = v
        m[iu[1], iu[0]] = v
        return m
    slide = min(slide, L)
    rows, cols = out_dims(L, slide, mat_trim)
    m = np.full((slide, L), np.nan)
    pc = [(g == a).astype(np.int64) for a in range(3)]
    for k in range(1, slide + 1):
        i = np.arange(0, L - k)
        if i.size == 0:
            continue
        t = np.empty((i.size, 3, 3), np.int64)
        for a in range(3):
            for b in range(3):
                t[:, a, b] = (pc[a][i] * pc[b][i + k]).sum(1)
        m[k - 1, i] = ld_values(t, method)
    return m[:, :cols]


def pairwise_complete(g):
    """(cov, cor) of the genotype rows g [L][N] (3 = missing) over pairwise-complete observations, two-pass per pair with masked
    numpy: what R's cov / cor(use = "pairwise.complete.obs") compute on snpgdsGetGeno's matrix (inst/unitTests/test_LD.R).
    NaN where fewer than two (cov) observations, or a zero variance (cor)."""
    x = np.asarray(g).astype(np.float64)
    called = np.asarray(g) < 3
    L = x.shape[0]
    cov = np.full((L, L), np.nan)
    cor = np.full((L, L), np.nan)
    with np.errstate(all="ignore"):
        for i in range(L):
            m = called[i][None, :] & called
            n = m.sum(1)
            xi = np.where(m, x[i][None, :], 0.0)
            xj = np.where(m, x, 0.0)
            mi = xi.sum(1) / n
            mj = xj.sum(1) / n
            di = np.where(m, xi - mi[:, None], 0.0)
            dj = np.where(m, xj - mj[:, None], 0.0)
            sxy = (di * dj).sum(1)
            sxx = (di * di).sum(1)
            syy = (dj * dj).sum(1)
            cov[i] = np.where(n > 1, sxy / (n - 1), np.nan)
            cor[i] = np.where((n > 1) & (sxx > 0) & (syy > 0), sxy / np.sqrt(sxx * syy), np.nan)
    return cov, cor
