"""Two restatements of gnrPairScore (genotype scores of listed sample pairs), written from its description.

g is uint8 [n_snp][n_samp] with 0, 1, 2 and anything above 2 for a missing call; idx1 / idx2 are the 0-based sample indices of
the pairs.  A score is MAP[g1][g2] wherever g1 < 3 and g2 < 3 -- also where the map holds -1 (the two *.only methods).  The four
*.major / *.minor methods first flip a SNP (g -> 2 - g for g < 3) when gsum < n over the listed pair members, a sample counting
once per appearance in either list.

pair_score_loop is the naive form: SNP loop, flip, pair loop, running double Sum / SqSum / Num, calc_avg_sd.  pair_score_ref is
the vectorised form through integer tables.  Both return
    "per.pair"  (Avg, SD, Num) float64 [n_pair] each
    "per.snp"   float64 [3][n_snp]
    "matrix"    int32 [n_pair][n_snp] with NA_INTEGER for a missing genotype
"""
import math

import numpy as np

METHODS = ("IBS", "GVH", "HVG", "GVH.major", "GVH.minor", "GVH.major.only", "GVH.minor.only")
TYPES = ("per.pair", "per.snp", "matrix")
NA_INTEGER = -2 ** 31
M = -1

_MAPS = {
    ("IBS", True): [[2, 1, 0, M], [1, 2, 1, M], [0, 1, 2, M], [M, M, M, M]],
    ("IBS", False): [[1, 1, 0, M], [1, 1, 1, M], [0, 1, 1, M], [M, M, M, M]],
    ("GVH", True): [[0, 0, 2, M], [1, 0, 1, M], [2, 0, 0, M], [M, M, M, M]],
    ("GVH", False): [[0, 0, 1, M], [1, 0, 1, M], [1, 0, 0, M], [M, M, M, M]],
    ("HVG", True): [[0, 1, 2, M], [0, 0, 0, M], [2, 1, 0, M], [M, M, M, M]],
    ("HVG", False): [[0, 1, 1, M], [0, 0, 0, M], [1, 1, 0, M], [M, M, M, M]],
    "GVH.major": [[0, 0, 0, M], [1, 0, 0, M], [1, 0, 0, M], [M, M, M, M]],
    "GVH.minor": [[0, 0, 1, M], [0, 0, 1, M], [0, 0, 0, M], [M, M, M, M]],
    "GVH.major.only": [[0, 0, M, M], [1, 0, M, M], [1, 0, 0, M], [M, M, M, M]],
    "GVH.minor.only": [[0, 0, 1, M], [M, 0, 1, M], [M, 0, 0, M], [M, M, M, M]],
}


def score_map(method, dosage):
    """(4 x 4 int64 map, need_major)"""
    if method not in METHODS:
        raise ValueError("Invalid 'method'.")
    if method in ("IBS", "GVH", "HVG"):
        return np.array(_MAPS[(method, bool(dosage))], np.int64), False
    return np.array(_MAPS[method], np.int64), True


def calc_avg_sd(s, sq, num):
    """CalcAvgSD on double sums and an int count: every operation separate, in this order"""
    if num > 1:
        avg = s / float(num)
        t = float(num) * avg
        t = t * avg
        v = (sq - t) / float(num - 1)
        return avg, (math.sqrt(v) if v >= 0 else float("nan"))
    if num == 1:
        return s, float("nan")
    return float("nan"), float("nan")


def pair_score_loop(g, idx1, idx2, method, type, dosage=True):
    mp, major = score_map(method, dosage)
    mp = mp.tolist()
    n_snp, n_pair = g.shape[0], len(idx1)
    sums = [[0.0, 0.0, 0] for _ in range(n_pair)]
    per_snp = np.empty((3, n_snp), np.float64)
    mat = np.empty((n_pair, n_snp), np.int32)
    for i in range(n_snp):
        row = [min(int(x), 3) for x in g[i]]
        if major:
            n = gsum = 0
            for j in range(n_pair):
                for x in (row[idx1[j]], row[idx2[j]]):
                    if x < 3:
                        n += 1
                        gsum += x
            if gsum < n:
                row = [2 - x if x < 3 else x for x in row]
        s = sq = 0.0
        num = 0
        for j in range(n_pair):
            g1, g2 = row[idx1[j]], row[idx2[j]]
            if g1 < 3 and g2 < 3:
                v = float(mp[g1][g2])
                sums[j][0] += v
                sums[j][1] += v * v
                sums[j][2] += 1
                s += v
                sq += v * v
                num += 1
                mat[j, i] = mp[g1][g2]
            else:
                mat[j, i] = NA_INTEGER
        a, d = calc_avg_sd(s, sq, num)
        per_snp[:, i] = (a, d, num)
    if type == "per.pair":
        r = [calc_avg_sd(*x) + (x[2],) for x in sums]
        return tuple(np.array([x[k] for x in r], np.float64) for k in range(3))
    if type == "per.snp":
        return per_snp
    if type == "matrix":
        return mat
    raise ValueError("Invalid 'type'.")


def flip_flags(g1, g2):
    """bool [n_snp]: gsum < n over both lists; g1 / g2 [n_snp][n_pair] clipped to 0 ... 3"""
    n = (g1 < 3).sum(1) + (g2 < 3).sum(1)
    gsum = np.where(g1 < 3, g1, 0).sum(1, dtype=np.int64) + np.where(g2 < 3, g2, 0).sum(1, dtype=np.int64)
    return gsum < n


def pair_codes(g, idx1, idx2, need_major):
    """the codes (clipped to 0 ... 3) of both members [n_snp][n_pair], flipped when need_major, and the flip flags"""
    g = np.minimum(np.asarray(g), 3).astype(np.int8)                 # small types: the sums below name their own
    g1, g2 = g[:, np.asarray(idx1)], g[:, np.asarray(idx2)]
    flip = flip_flags(g1, g2)
    if need_major:
        f = flip[:, None]
        g1 = np.where(f & (g1 < 3), 2 - g1, g1)
        g2 = np.where(f & (g2 < 3), 2 - g2, g2)
    return g1, g2, flip


def tables(g, idx1, idx2, need_major):
    """(pair_tab int64 [n_pair][3][3] after the flip when need_major, snp_tab int32 [n_snp][4][4] as stored, flip uint8 [n_snp])"""
    r1, r2, flip = pair_codes(g, idx1, idx2, False)
    n_snp, n_pair = r1.shape
    snp_tab = np.zeros((n_snp, 16), np.int32)
    for c in range(16):
        snp_tab[:, c] = (4 * r1 + r2 == c).sum(1, dtype=np.int64)
    f1, f2, _ = pair_codes(g, idx1, idx2, need_major)
    pair_tab = np.zeros((n_pair, 9), np.int64)
    ok = (f1 < 3) & (f2 < 3)
    for c in range(9):
        pair_tab[:, c] = (ok & (3 * f1 + f2 == c)).sum(0, dtype=np.int64)
    return pair_tab.reshape(n_pair, 3, 3), snp_tab.reshape(n_snp, 4, 4), flip.astype(np.uint8)


def _avg_sd_vec(s, sq, num):
    s, sq, numf = s.astype(np.float64), sq.astype(np.float64), num.astype(np.float64)
    with np.errstate(all="ignore"):
        avg = s / numf
        t = numf * avg
        t = t * avg
        sd = np.sqrt((sq - t) / (numf - 1.0))
    avg = np.where(num > 1, avg, np.where(num == 1, s, np.nan))
    sd = np.where(num > 1, sd, np.nan)
    return avg, sd, numf


def pair_score_ref(g, idx1, idx2, method, type, dosage=True):
    mp, major = score_map(method, dosage)
    g1, g2, _ = pair_codes(g, idx1, idx2, major)
    ok = (g1 < 3) & (g2 < 3)
    v = mp.astype(np.int8)[g1, g2]
    if type == "matrix":
        return np.where(ok, v.astype(np.int32), np.int32(NA_INTEGER)).T.copy()
    v = np.where(ok, v, np.int8(0))
    axis = 0 if type == "per.pair" else 1
    if type not in ("per.pair", "per.snp"):
        raise ValueError("Invalid 'type'.")
    avg, sd, num = _avg_sd_vec(v.sum(axis, dtype=np.int64), (v * v).sum(axis, dtype=np.int64), ok.sum(axis, dtype=np.int64))
    return (avg, sd, num) if type == "per.pair" else np.stack([avg, sd, num])


def bit2(matrix):
    """the two bits a bit2 node keeps of the byte the reference appends: 3 for NA, value & 3 otherwise"""
    m = np.asarray(matrix).astype(np.int64)
    return np.where(m == NA_INTEGER, 3, m & 3).astype(np.uint8)
