"""numpy restatement of the fixation index and of the sliding-window bookkeeping, written from the behaviour of gnrFst
(src/genFst.cpp), gnrSlidingWindow (src/genSlideWin.cpp) and the R functions snpgdsFst / snpgdsSlidingWindow: test
infrastructure, fp64 throughout, every expression in the reference's operation order (numpy rounds each elementwise operation
once, as the C code does without contraction), sums over SNPs sequential in ascending order.

Tolerances.  Besides its values the restatement reports, for every ratio A / B of sums A = sum a_i, B = sum b_i,
    bound = 4 n 2^-53 (sum |a_i| / |B| + |A| sum |b_i| / B^2),
the rounding bound of the same sums taken in another order (n: the number of SNPs in the sum; math.fsum inside).  W&C84 numerators
change sign, so a relative tolerance on the ratio itself would be wrong.  Per-SNP values are fixed expressions of exact integers:
they get the same kind of bound over the expression's own terms -- with every difference that can cancel, (p_k - p)^2 and
p_1 + p_2 - 2 p_1 p_2, entered by the magnitudes of its expanded terms, and n the number of terms.  `exact_*` evaluate the same
formulas in fractions.Fraction (exact) for the tests that check the restatement itself.

n_c of W&C84 sums Cnt_k^2 exactly (the reference multiplies two ints, which overflows beyond 23 170 called samples)."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def pop_counts(g, pop, n_pop):
    """(ACnt, Cnt) int64 [n_snp][n_pop] from uint8 genotypes [n_snp][n_samp] (> 2 missing) and 0-based population indices"""
    g = np.asarray(g)
    pop = np.asarray(pop)
    called = g <= 2
    val = np.where(called, g, 0).astype(np.int64)
    a = np.zeros((g.shape[0], n_pop), np.int64)
    c = np.zeros((g.shape[0], n_pop), np.int64)
    for k in range(n_pop):
        m = pop == k
        a[:, k] = val[:, m].sum(1)
        c[:, k] = 2 * called[:, m].sum(1)
    return a, c


def ratio_bound(a_abs, b_abs, A, B, n):
    """4 n u (sum |a| / |B| + |A| sum |b| / B^2); inf where B == 0"""
    if B == 0 or not math.isfinite(B) or not math.isfinite(A):
        return math.inf
    return 4.0 * n * U * (a_abs / abs(B) + abs(A) * b_abs / (B * B))


def _freq(a, c):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a.astype(np.float64) / c.astype(np.float64)


def wc84_terms(acnt, cnt):
    """per SNP: num, den (WC84, src/genFst.cpp:76-98), valid, and the magnitude sums of their terms for the bounds"""
    acnt, cnt = np.asarray(acnt, np.int64), np.asarray(cnt, np.int64)
    M, K = acnt.shape
    valid = (cnt > 0).all(1)
    at, ct = acnt.sum(1), cnt.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_all = at.astype(np.float64) / ct.astype(np.float64)
        msb = np.zeros(M)
        msw = np.zeros(M)
        n_c = np.zeros(M)
        msb_abs = np.zeros(M)
        for k in range(K):
            p = _freq(acnt[:, k], cnt[:, k])
            c = cnt[:, k].astype(np.float64)
            msb = msb + c * (p - p_all) * (p - p_all)
            msw = msw + c * p * (1 - p)
            n_c = n_c + (cnt[:, k] * cnt[:, k]).astype(np.float64)
            msb_abs = msb_abs + c * (p + p_all) * (p + p_all)
        msb = msb / float(K - 1)
        msb_abs = msb_abs / float(K - 1)
        msw = msw / (ct - K).astype(np.float64)
        n_c = (ct.astype(np.float64) - n_c / ct.astype(np.float64)) / float(K - 1)
        num = msb - msw
        den = msb + (n_c - 1) * msw
        num_abs = msb_abs + msw
        den_abs = msb_abs + np.abs(n_c - 1) * msw
    num = np.where(valid, num, 0.0)
    den = np.where(valid, den, 0.0)
    return num, den, valid, np.where(valid, num_abs, 0.0), np.where(valid, den_abs, 0.0)


def wh02_h(acnt, cnt):
    """per SNP: H [n_snp][K][K], upper triangle (src/genFst.cpp:131-139), valid, and the magnitudes of the expanded terms"""
    acnt, cnt = np.asarray(acnt, np.int64), np.asarray(cnt, np.int64)
    M, K = acnt.shape
    valid = (cnt > 0).all(1)
    H = np.zeros((M, K, K))
    Habs = np.zeros((M, K, K))
    with np.errstate(invalid="ignore", divide="ignore"):
        P = [_freq(acnt[:, k], cnt[:, k]) for k in range(K)]
        for k1 in range(K):
            c = cnt[:, k1].astype(np.float64)
            H[:, k1, k1] = 2.0 * c / (cnt[:, k1] - 1).astype(np.float64) * P[k1] * (1 - P[k1])
            Habs[:, k1, k1] = H[:, k1, k1]
            for k2 in range(k1 + 1, K):
                H[:, k1, k2] = P[k1] + P[k2] - 2 * P[k1] * P[k2]
                Habs[:, k1, k2] = P[k1] + P[k2] + 2 * P[k1] * P[k2]
    H[~valid] = 0
    Habs[~valid] = 0
    return H, valid, Habs


def _wh02_beta(H, K):
    """WH02_beta (src/genFst.cpp:143-166) on one K x K matrix (upper triangle): (1 - H_W / H_B, beta, H_W sum, H_B sum)"""
    hw = hb = 0.0
    for k1 in range(K):
        hw += H[k1, k1]
        for k2 in range(k1 + 1, K):
            hb += H[k1, k2]
    sw, sb = hw, hb
    hw = hw / float(K)
    hb = hb / float(K * (K - 1) // 2)
    beta = np.zeros((K, K))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k1 in range(K):
            for k2 in range(k1, K):
                beta[k1, k2] = beta[k2, k1] = 1 - np.float64(H[k1, k2]) / np.float64(hb)
        r = 1 - np.float64(hw) / np.float64(hb)
    return float(r), beta, sw, sb


def _seq_sum(x):
    """sum in index order, one fp64 addition per element"""
    x = np.asarray(x, np.float64)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def fst_snp(acnt, cnt, method):
    """per-SNP ratios (NaN where a population has no call) and their bounds"""
    acnt, cnt = np.asarray(acnt, np.int64), np.asarray(cnt, np.int64)
    M, K = acnt.shape
    out = np.full(M, np.nan)
    bound = np.full(M, np.inf)
    if method == "W&C84":
        num, den, valid, na, da = wc84_terms(acnt, cnt)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[valid] = num[valid] / den[valid]
        for s in np.nonzero(valid)[0]:
            bound[s] = ratio_bound(na[s], da[s], num[s], den[s], 2 * K)
    else:
        H, valid, Habs = wh02_h(acnt, cnt)
        n_terms = K * (K + 1) // 2
        for s in np.nonzero(valid)[0]:
            r, _, sw, sb = _wh02_beta(H[s], K)
            out[s] = r
            aw = math.fsum(Habs[s, k, k] for k in range(K))
            ab = math.fsum(Habs[s, k1, k2] for k1 in range(K) for k2 in range(k1 + 1, K))
            bound[s] = ratio_bound(aw, ab, sw, sb, n_terms)
    return out, bound


def fst_set(acnt, cnt, method, snps=None):
    """gnrFst over the SNPs `snps` (ascending indices; None = all): dict(Fst, Fst_bound[, Beta, Beta_bound], n)"""
    acnt, cnt = np.asarray(acnt, np.int64), np.asarray(cnt, np.int64)
    if snps is not None:
        acnt, cnt = acnt[np.asarray(snps, np.int64)], cnt[np.asarray(snps, np.int64)]
    M, K = acnt.shape
    if method == "W&C84":
        num, den, valid, na, da = wc84_terms(acnt, cnt)
        A, B = _seq_sum(num[valid]), _seq_sum(den[valid])
        n = int(valid.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            f = float(np.float64(A) / np.float64(B))
        return dict(Fst=f, Fst_bound=ratio_bound(math.fsum(na[valid]), math.fsum(da[valid]), A, B, max(n, 1)), n=n)
    H, valid, Habs = wh02_h(acnt, cnt)
    n = int(valid.sum())
    S = np.zeros((K, K))
    for k1 in range(K):
        for k2 in range(k1, K):
            S[k1, k2] = _seq_sum(H[valid, k1, k2])
    f, beta, sw, sb = _wh02_beta(S, K)
    aw = math.fsum(Habs[valid][:, k, k].sum() for k in range(K)) if n else 0.0
    ab = math.fsum(math.fsum(Habs[valid][:, k1, k2]) for k1 in range(K) for k2 in range(k1 + 1, K)) if n else 0.0
    bb = np.full((K, K), np.inf)
    npair = K * (K - 1) // 2
    for k1 in range(K):
        for k2 in range(k1, K):
            a_abs = math.fsum(Habs[valid][:, k1, k2]) if n else 0.0
            bb[k1, k2] = bb[k2, k1] = ratio_bound(a_abs, ab / npair, S[k1, k2], sb / npair, max(n, 1) + npair)
    return dict(Fst=f, Fst_bound=ratio_bound(aw / K, ab / npair, sw / K, sb / npair, max(n, 1) + npair), Beta=beta, Beta_bound=bb, n=n)


def snpgds_fst(g, pop, n_pop, method):
    """snpgdsFst on genotypes [n_snp][n_samp]: Fst, MeanFst, FstSNP(, Beta) with their bounds"""
    a, c = pop_counts(g, pop, n_pop)
    per, per_bound = fst_snp(a, c, method)
    rv = fst_set(a, c, method)
    ok = ~np.isnan(per)
    rv.update(FstSNP=per, FstSNP_bound=per_bound, MeanFst=float(per[ok].mean()) if ok.any() else float("nan"))
    return rv


# ---- exact rational arithmetic ------------------------------------------------------------------------------------------------
def exact_wc84(a, c):
    """(num, den) of one SNP as Fractions, or None when a population has no call"""
    K = len(a)
    if any(int(x) <= 0 for x in c):
        return None
    a = [Fraction(int(x)) for x in a]
    c = [Fraction(int(x)) for x in c]
    ct = sum(c)
    p_all = sum(a) / ct
    P = [x / y for x, y in zip(a, c)]
    msb = sum(ck * (p - p_all) ** 2 for ck, p in zip(c, P)) / (K - 1)
    msw = sum(ck * p * (1 - p) for ck, p in zip(c, P)) / (ct - K)
    n_c = (ct - sum(ck * ck for ck in c) / ct) / (K - 1)
    return msb - msw, msb + (n_c - 1) * msw


def exact_wh02(a, c):
    """H (dict (k1, k2) -> Fraction, k1 <= k2) of one SNP, or None"""
    K = len(a)
    if any(int(x) <= 0 for x in c):
        return None
    P = [Fraction(int(x), int(y)) for x, y in zip(a, c)]
    H = {}
    for k1 in range(K):
        ck = Fraction(int(c[k1]))
        H[(k1, k1)] = 2 * ck / (ck - 1) * P[k1] * (1 - P[k1])
        for k2 in range(k1 + 1, K):
            H[(k1, k2)] = P[k1] + P[k2] - 2 * P[k1] * P[k2]
    return H


def exact_fst(acnt, cnt, method, snps=None):
    """dict(Fst, FstSNP[, Beta]) in exact arithmetic; values are Fractions, or None for 0 / 0 and x / 0 and SNPs without a value"""
    acnt, cnt = np.asarray(acnt), np.asarray(cnt)
    idx = range(acnt.shape[0]) if snps is None else list(snps)
    K = acnt.shape[1]

    def div(x, y):
        return None if y == 0 else x / y
    per = []
    if method == "W&C84":
        A = B = Fraction(0)
        for s in idx:
            t = exact_wc84(acnt[s], cnt[s])
            if t is None:
                per.append(None)
                continue
            A += t[0]
            B += t[1]
            per.append(div(t[0], t[1]))
        return dict(Fst=div(A, B), FstSNP=per)
    S = {(k1, k2): Fraction(0) for k1 in range(K) for k2 in range(k1, K)}

    def beta_of(H):
        hw = sum(H[(k, k)] for k in range(K)) / K
        hb = sum(H[(k1, k2)] for k1 in range(K) for k2 in range(k1 + 1, K)) / Fraction(K * (K - 1), 2)
        r = div(hw, hb)
        return (None if r is None else 1 - r), hb
    for s in idx:
        H = exact_wh02(acnt[s], cnt[s])
        if H is None:
            per.append(None)
            continue
        per.append(beta_of(H)[0])
        for key in S:
            S[key] += H[key]
    f, hb = beta_of(S)
    beta = [[None] * K for _ in range(K)]
    for (k1, k2), v in S.items():
        r = div(v, hb)
        beta[k1][k2] = beta[k2][k1] = None if r is None else 1 - r
    return dict(Fst=f, FstSNP=per, Beta=beta)


# ---- sliding windows: the loops of gnrSlidingWindow, one window at a time --------------------------------------------------------
def sliding_num_win(start, end, winsize, shift):
    cnt = 0
    end -= winsize
    while start <= end:
        cnt += 1
        start += shift
    return cnt + 1


def sliding_windows(chpos, winsize, shift, unit="basepair", winstart=None):
    """(members per window (ascending indices into chpos), num, pos, posrange) as the for-loop of gnrSlidingWindow gives them"""
    chpos = np.asarray(chpos, np.int64)
    n = len(chpos)
    pos_min, pos_max = int(chpos.min()), int(chpos.max())
    posrange = (pos_min, pos_max)
    if unit == "basepair":
        if winstart is not None:
            pos_min = int(winstart)
    else:
        pos_max = n - 1
        pos_min = 0 if winstart is None else int(winstart) - 1
    n_win = sliding_num_win(pos_min, pos_max, winsize, shift)
    members, num, pos = [], [], []
    key = chpos if unit == "basepair" else np.arange(n, dtype=np.int64)
    x = pos_min
    for _ in range(n_win):
        m = np.nonzero((x <= key) & (key < x + winsize))[0]          # the loop's test, for all SNPs of the chromosome at once
        members.append(m.astype(np.int64))
        num.append(len(m))
        pos.append(float(chpos[m].sum()) / len(m) if len(m) else float("nan"))      # a sum of integers: exact in any order
        x += shift
    return members, np.array(num, np.int32), np.array(pos), posrange


def chromosome_set(chrom, flag):
    """setdiff(unique(chr[flag]), c(0, "")): in order of first appearance"""
    out = []
    for c in np.asarray(chrom)[np.asarray(flag, bool)]:
        if c not in out and c != 0 and c != "":
            out.append(c)
    return out


def get_mean(x):
    """GetMean (src/genSlideWin.cpp:61-75)"""
    s, m = 0.0, 0
    for v in np.asarray(x, np.float64):
        if math.isfinite(v):
            s += float(v)
            m += 1
    return s / m if m else float("nan")
