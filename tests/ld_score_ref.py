"""CPU restatement of the LD scores (snpgdsLDScore -> snpgpu_ld_score, include/snpgpu.h section 1d) for the tests: the definition
as plain loops over ld_ref.tables / ld_ref.ld_values.

Per chromosome, SNPs 0 ... M - 1 in file order with non-decreasing positions.  Pair (i, j), i != j, is in the window iff
|i - j| <= max_n and |pos[i] - pos[j]| <= max_bp (pos None: the count alone); the partners of i are one range [lo[i], hi[i]] and
W = max (hi[i] - i).  Each unordered pair is evaluated once with the lower index first: v = its LD value, t = v * v, with `adjust`
t = t - (1 - t) / (n - 2), n = the table's total; valid iff v is not NaN and (adjusting) n > 2.  score[i] = (1.0 if include_self
else 0.0) + t of the valid partners lo[i] ... hi[i] in ascending order, one left fold in float64.  Test infrastructure only."""
import types

import numpy as np

import ld_ref

INT_MAX = 2 ** 31 - 1


def in_window(i, j, pos, max_bp, max_n):
    if abs(i - j) > max_n:
        return False
    return pos is None or abs(int(pos[i]) - int(pos[j])) <= max_bp


def windows(M, pos, max_bp, max_n):
    """(lo, hi, W) by two two-pointer passes (what the library does on the host)"""
    lo, hi = np.arange(M), np.arange(M)
    if max_n <= 0 or max_bp < 0:
        return lo, hi, 0
    h = l = 0
    for i in range(M):
        h = max(h, i)
        while h + 1 < M and in_window(i, h + 1, pos, max_bp, max_n):
            h += 1
        hi[i] = h
        while l < i and not in_window(l, i, pos, max_bp, max_n):
            l += 1
        lo[i] = l
    return lo, hi, int((hi - np.arange(M)).max()) if M else 0


def windows_brute(M, pos, max_bp, max_n):
    """(lo, hi, W, contiguous) straight from the pair test, O(M^2); contiguous: every SNP's partners form one range around it"""
    lo, hi, ok = np.arange(M), np.arange(M), True
    for i in range(M):
        inside = [j for j in range(M) if j != i and max_n > 0 and max_bp >= 0 and in_window(i, j, pos, max_bp, max_n)]
        if inside:
            lo[i], hi[i] = min(min(inside), i), max(max(inside), i)
            ok = ok and sorted(inside + [i]) == list(range(lo[i], hi[i] + 1))
    return lo, hi, int((hi - np.arange(M)).max()) if M else 0, ok


def tables(g):
    """ld_ref.tables(g) for the pairs of g's rows, summed over sample chunks so that a large sample count stays cheap: per chunk
    the one-hot products in float64 (integers far below 2^53: exact), small inputs through ld_ref.tables itself"""
    g = np.asarray(g)
    if g.shape[1] <= 4096:
        return ld_ref.tables(g)
    t = np.zeros((g.shape[0], g.shape[0], 3, 3), np.int64)
    for s in range(0, g.shape[1], 16384):
        c = g[:, s:s + 16384]
        planes = [(c == a).astype(np.float64) for a in range(3)]
        for a in range(3):
            for b in range(3):
                t[:, :, a, b] += np.rint(planes[a] @ planes[b].T).astype(np.int64)
    return t


def pair_values(tab, method):
    """(V, n) of tables [M][M][3][3]: LD value and table total of every pair, each unordered pair evaluated once with the lower
    index first and mirrored; NaN diagonal"""
    tab = np.asarray(tab, np.int64)
    M = tab.shape[0]
    iu = np.triu_indices(M, 1)
    V = np.full((M, M), np.nan)
    if iu[0].size:
        V[iu] = ld_ref.ld_values(tab[iu], method)
        V[iu[1], iu[0]] = V[iu]
    return V, tab.sum((-1, -2))


def pair_terms(V, n, adjust):
    """T[i, j] = the term of pair (i, j), NaN where the pair is not valid (element-wise float64, the definition's order)"""
    with np.errstate(all="ignore"):
        t = V * V
        if adjust:
            t = t - (1 - t) / (n - 2).astype(np.float64)
            t = np.where(n > 2, t, np.nan)
        return np.where(np.isnan(V), np.nan, t)


def fold(T, lo, hi, include_self):
    """(score, n_valid): the left fold of the valid terms of row i over lo[i] ... hi[i], j != i, in Python floats"""
    M = T.shape[0]
    score, n_valid = np.empty(M, np.float64), np.zeros(M, np.int32)
    for i in range(M):
        acc, cnt = (1.0 if include_self else 0.0), 0
        for j in range(int(lo[i]), int(hi[i]) + 1):
            t = float(T[i, j])
            if j == i or t != t:
                continue
            acc += t
            cnt += 1
        score[i], n_valid[i] = acc, cnt
    return score, n_valid


def score_from_values(V, n, pos, max_bp, max_n, adjust, include_self):
    """the definition on given pair values V / totals n [M][M] (symmetric): a namespace with score, n_valid, n_window, lo, hi,
    width, window_pairs, valid_pairs, and the matrices V, n, T for error bounds"""
    M = V.shape[0]
    lo, hi, W = windows(M, pos, max_bp, max_n)
    T = pair_terms(V, n, adjust)
    score, n_valid = fold(T, lo, hi, include_self)
    return types.SimpleNamespace(score=score, n_valid=n_valid, n_window=(hi - lo).astype(np.int32), lo=lo, hi=hi, width=W,
                                 window_pairs=int((hi - np.arange(M)).sum()), valid_pairs=int(n_valid.sum()) // 2, V=V, n=n, T=T,
                                 adjust=adjust)


def ld_score(g, pos, max_bp, max_n, method, adjust=True, include_self=True):
    """the definition on uint8 genotype rows g [M][N] (3 = missing)"""
    V, n = pair_values(tables(g), method)
    return score_from_values(V, n, pos, max_bp, max_n, adjust, include_self)


def ld_score_brute(g, pos, max_bp, max_n, method, adjust=True, include_self=True):
    """(score, n_valid, n_window) by brute force: every ordered pair (i, j) tested and evaluated on its own 3 x 3 table"""
    g = np.asarray(g)
    M = g.shape[0]
    score, n_valid, n_window = np.empty(M), np.zeros(M, np.int32), np.zeros(M, np.int32)
    for i in range(M):
        acc = 1.0 if include_self else 0.0
        for j in range(M):
            if j == i or max_n <= 0 or max_bp < 0 or not in_window(i, j, pos, max_bp, max_n):
                continue
            n_window[i] += 1
            a, b = min(i, j), max(i, j)
            tab = ld_ref.tables(g[a:a + 1], g[b:b + 1])
            v = float(ld_ref.ld_values(tab, method)[0, 0])
            n = int(tab.sum())
            if v != v or (adjust and n <= 2):
                continue
            t = v * v
            if adjust:
                t = t - (1 - t) / (n - 2)
            acc += t
            n_valid[i] += 1
        score[i] = acc
    return score, n_valid, n_window


def error_bound(ref, tol):
    """|score - ref.score| allowed per SNP when every pair value is within `tol` of the reference's: the sum over the valid
    partners of (2 |v| + tol) tol (1 + 1 / (n - 2) when adjusted), plus 1e-13 sum |t| for the summation"""
    M = ref.V.shape[0]
    out = np.zeros(M)
    with np.errstate(all="ignore"):
        per = (2 * np.abs(ref.V) + tol) * tol
        if ref.adjust:
            per = per * (1 + 1 / (ref.n - 2).astype(np.float64))
    for i in range(M):
        sl = slice(int(ref.lo[i]), int(ref.hi[i]) + 1)
        ok = ~np.isnan(ref.T[i, sl])
        out[i] = per[i, sl][ok].sum() + 1e-13 * np.abs(ref.T[i, sl][ok]).sum()
    return out
