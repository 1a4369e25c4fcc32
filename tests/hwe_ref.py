"""Sequential fp64 restatement of the exact test of Hardy-Weinberg equilibrium (Wigginton, Cutler & Abecasis 2005) as gnrHWE
evaluates it, written from the formulas: the unnormalised probabilities of every heterozygote count follow from the midpoint by
the two-term recurrences

    P(h - 2) = P(h) h (h - 1) / (4 (r + 1) (c + 1))        P(h + 2) = P(h) 4 r c / ((h + 2) (h + 1))

(r, c: rare and common homozygotes at h), are normalised by their sum and the p-value adds, in ascending order of h, those not
greater than the observed one.  Python floats are IEEE doubles and nothing here is fused, so every step rounds as a C double
expression of the same shape does.  The products of counts are exact Python integers."""
import math

import numpy as np


def hwe_terms(het, hom1, hom2):
    """(normalised probabilities indexed by heterozygote count, rare_copies) or (None, rare_copies) without a genotype"""
    homc, homr = max(hom1, hom2), min(hom1, hom2)
    rare = 2 * homr + het
    n = het + homc + homr
    if n <= 0:
        return None, rare
    probs = [0.0] * (rare + 1)
    mid = rare * (2 * n - rare) // (2 * n)
    if (rare & 1) ^ (mid & 1):
        mid += 1
    probs[mid] = 1.0
    total = 1.0
    h, r, c = mid, (rare - mid) // 2, n - mid - (rare - mid) // 2
    while h > 1:
        probs[h - 2] = probs[h] * h * (h - 1.0) / (4.0 * (r + 1.0) * (c + 1.0))
        total += probs[h - 2]
        r += 1
        c += 1
        h -= 2
    h, r, c = mid, (rare - mid) // 2, n - mid - (rare - mid) // 2
    while h <= rare - 2:
        probs[h + 2] = probs[h] * 4.0 * r * c / ((h + 2.0) * (h + 1.0))
        total += probs[h + 2]
        r -= 1
        c -= 1
        h += 2
    return [x / total for x in probs], rare


def hwe_pvalue(het, hom1, hom2):
    """p-value of one SNP: obs_hets, the two homozygote counts (either order)"""
    probs, _ = hwe_terms(int(het), int(hom1), int(hom2))
    if probs is None:
        return float("nan")
    p = 0.0
    obs = probs[int(het)]
    for x in probs:
        if x > obs:
            continue
        p += x
    return 1.0 if p > 1.0 else p


def hwe_ref(snp_cnt):
    """p-values for counts [n_snp][3] of g = 0, 1, 2 (BB, AB, AA), and rare_copies per SNP"""
    c = np.asarray(snp_cnt, np.int64)
    pv = np.array([hwe_pvalue(b, a2, a0) for a0, b, a2 in c], np.float64)
    rare = 2 * np.minimum(c[:, 0], c[:, 2]) + c[:, 1]
    return pv, rare


def hwe_bound(pv, rare):
    """two orderings of a sum of at most rare / 2 + 1 non-negative terms (and the clamp): 2 (rare / 2 + 2) 2^-53 p"""
    return 2.0 * (np.asarray(rare) / 2.0 + 2.0) * 2.0 ** -53 * np.asarray(pv)


def hwe_lgamma(het, hom1, hom2, slack=1e-6):
    """Independent evaluation through math.lgamma of P(h) = n! 2^h nA! nB! / (r! h! c! (2 n)!): (p_lo, p_hi), the sums over the
    terms not greater than the observed one, without / with those within `slack` (relative) above it -- near ties that the two
    evaluations may decide differently."""
    homc, homr = max(hom1, hom2), min(hom1, hom2)
    rare, n = 2 * homr + het, het + homc + homr
    if n <= 0:
        return float("nan"), float("nan")
    lg = math.lgamma

    def logp(h):
        r = (rare - h) // 2
        c = n - h - r
        return lg(n + 1) - lg(r + 1) - lg(h + 1) - lg(c + 1) + h * math.log(2.0) + lg(rare + 1) + lg(2 * n - rare + 1) - lg(2 * n + 1)

    lo_obs = logp(het)
    p_lo = p_hi = 0.0
    for h in range(rare & 1, rare + 1, 2):
        d = logp(h) - lo_obs
        if d <= -slack or h == het:                  # the observed term itself always counts
            p_lo += math.exp(logp(h))
        if d <= slack:
            p_hi += math.exp(logp(h))
    return min(p_lo, 1.0), min(p_hi, 1.0)
