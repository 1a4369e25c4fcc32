"""Individual dissimilarity (snpgdsDiss -> gnrDiss, src/genIBS.cpp:333-419 and :652-683) restated in numpy, plus a loop-by-loop
transcription of the reference that pins the restatement (tests/test_cpu_diss.py).

Genotypes are uint8 [n_snp][n_samp], 0 / 1 / 2 and 3 (or more) for a missing call, the layout the accumulators are fed with.
Per SNP F = sum g / (2 n_called) (0 without a call) and w = 8 F (1 - F); per pair, over the SNPs where BOTH samples are called,
SumGeno = sum g_i (2 - g_j) + (2 - g_i) g_j (an integer) and SumAFreq = sum w.  diss = SumGeno / SumAFreq off the diagonal and twice
that on it, IEEE division unguarded (0/0 = NaN, x/0 = Inf)."""
import numpy as np


def snp_weights(geno):
    """w_s = 8 F (1 - F) per SNP, F as _Do_Diss_ReadBlock computes it"""
    g = np.asarray(geno)
    called = g < 3
    s = np.where(called, g, 0).sum(axis=1, dtype=np.int64).astype(np.float64)
    n = 2.0 * called.sum(axis=1)
    f = np.where(n > 0, s / np.where(n > 0, n, 1), 0.0)
    return 8 * f * (1 - f)


def diss_sums(geno, rows=None, cols=None):
    """(SumGeno int64 [r, c], SumAFreq fp64 [r, c]) for the sample rows / columns given (default: all)"""
    g = np.asarray(geno)
    called = g < 3
    w = snp_weights(g)
    gi = np.where(called, g, 0).astype(np.int64)
    hi = np.where(called, 2 - gi, 0)
    ca = called.astype(np.float64)
    r = slice(None) if rows is None else np.asarray(rows)
    c = slice(None) if cols is None else np.asarray(cols)
    sg = gi[:, r].T @ hi[:, c] + hi[:, r].T @ gi[:, c]
    sa = (ca[:, r] * w[:, None]).T @ ca[:, c]
    return sg, sa


def diss_matrix(geno, rows=None, cols=None):
    """the dissimilarity of the rows x columns given (diagonal: where the row sample is the column sample)"""
    sg, sa = diss_sums(geno, rows, cols)
    n = np.asarray(geno).shape[1]
    ri = np.arange(n) if rows is None else np.asarray(rows)
    ci = np.arange(n) if cols is None else np.asarray(cols)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = sg / sa
    d[ri[:, None] == ci[None, :]] *= 2
    return d


def packed_upper(m):
    """the packed upper triangle (row-major, diagonal included) of a square matrix"""
    return m[np.triu_indices(m.shape[0])]


# ---- the reference, loop by loop --------------------------------------------------------------------------------------------------
def _pack_geno_2b(vals):
    """PackGeno2b: four genotypes per byte, the first in the low bits; the tail byte padded with 3 (missing)"""
    out = []
    for k in range(0, len(vals), 4):
        b = 0
        for i in range(4):
            v = vals[k + i] if k + i < len(vals) else 3
            b |= (min(int(v), 3) & 3) << (2 * i)
        out.append(b)
    return out


def _tables():
    """Gen_Diss_SNP and Gen_Both_Valid (genIBS.cpp:108-121), indexed by (byte of sample 1) << 8 | (byte of sample 2)"""
    diss = np.zeros(65536, np.int64)
    valid = np.zeros(65536, np.int64)
    for t in range(65536):
        p1, p2 = t >> 8, t & 0xFF
        s, f = 0, 0
        for i in range(4):
            b1, b2 = (p1 >> (2 * i)) & 3, (p2 >> (2 * i)) & 3
            if b1 < 3 and b2 < 3:
                s += b1 * (2 - b2) + (2 - b1) * b2
                f |= 1 << i
        diss[t], valid[t] = s, f
    return diss, valid


_TABLES = None


def gnr_diss_loops(geno, block_snps=7):
    """gnrDiss as the reference runs it: reader blocks of `block_snps` SNPs (_Do_Diss_ReadBlock packs them and computes the
    weights), the pair loop over the packed bytes (_Do_Diss_Compute), then the output loop of gnrDiss.  Returns (diss [n, n],
    SumGeno [n, n], SumAFreq [n, n])."""
    global _TABLES
    if _TABLES is None:
        _TABLES = _tables()
    tdiss, tvalid = _TABLES
    g = np.asarray(geno)
    n_snp, n = g.shape
    sum_geno = [[0] * n for _ in range(n)]
    sum_af = [[0.0] * n for _ in range(n)]
    for start in range(0, n_snp, block_snps):
        cnt = min(block_snps, n_snp - start)
        blk = g[start:start + cnt]
        packed = [_pack_geno_2b([int(blk[s, i]) for s in range(cnt)]) for i in range(n)]
        freq = []
        for s in range(cnt):
            f, m = 0.0, 0
            for i in range(n):
                if blk[s, i] < 3:
                    f += float(blk[s, i])
                    m += 2
            f = f / m if m > 0 else 0.0
            freq.append(8 * f * (1 - f))
        freq += [0.0] * 4          # (the flags of the padded tail are never set)
        for i in range(n):
            for j in range(i, n):
                for k in range(len(packed[i])):
                    t = (packed[i][k] << 8) | packed[j][k]
                    sum_geno[i][j] += int(tdiss[t])
                    fl = int(tvalid[t])
                    for b in range(4):
                        if fl & (1 << b):
                            sum_af[i][j] += freq[4 * k + b]
    out = np.empty((n, n))
    sg = np.zeros((n, n), np.int64)
    sa = np.zeros((n, n))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            out[i, i] = 2 * (np.float64(sum_geno[i][i]) / np.float64(sum_af[i][i]))
            for j in range(i + 1, n):
                out[i, j] = out[j, i] = np.float64(sum_geno[i][j]) / np.float64(sum_af[i][j])
            for j in range(i, n):
                sg[i, j] = sg[j, i] = sum_geno[i][j]
                sa[i, j] = sa[j, i] = sum_af[i][j]
    return out, sg, sa
