"""What the PC-Relate row-panel tests share: the inputs (the generator and seeds of test_gpu_pcrelate.py), the cut of a full n x n
result to a panel, and snpgpu_pcr_select restated in numpy on a result dict."""
import functools

import numpy as np

import pcrelate_ref as R

TILE = 128
CUTOFF = 0.1
VALUES = ("kinship", "k0", "k2", "nsnp")
SLABS = R.PLANES + ("CD",)

#         n    M    D  missing training
INPUTS = {(65, 500): (65, 500, 2, 0.03, "fifth"),
          (130, 500): (130, 500, 2, 0.03, "fifth"),
          (130, 1030): (130, 1030, 2, 0.03, "fifth"),
          (257, 500): (257, 500, 2, 0.03, "fifth"),
          (257, 1030): (257, 1030, 2, 0.03, "fifth"),
          (300, 500): (300, 500, 2, 0.03, "fifth")}

# (n, (row_begin, row_end)) at M = 500: less than one tile; a tile and a ragged rest; three tile rows, the last one ragged row with n no
# multiple of 4; two tile rows in one panel; a panel that does not start at 0, with two tile rows, a ragged one and columns to the right
# of its diagonal block
PANEL_CASES = [(65, (0, 65)),
               (130, (0, 128)), (130, (128, 130)),
               (257, (0, 128)), (257, (128, 256)), (257, (256, 257)),
               (257, (0, 256)),
               (300, (128, 300))]


@functools.lru_cache(maxsize=None)
def inputs(n, m):
    """geno [m][n] uint8, pcs [n][D], the training flags: as test_gpu_pcrelate.inputs builds them"""
    n, m, D, miss, train = INPUTS[(n, m)]
    T = np.ones(n, bool) if train == "all" else np.arange(n) % 5 != 4
    d = R.admixed_families(n, m, 1000 + 7 * n + m + D, missing=miss, training=T)
    rng = np.random.default_rng(n + m)
    pcs = np.concatenate([(d["admix"] - d["admix"].mean())[:, None], rng.normal(0, 0.1, (n, 5))], 1)[:, :D]
    g = d["geno"]
    g.setflags(write=False)
    return dict(geno=g, pcs=pcs, T=T)


def partition(n, rows):
    """the panels [(r0, r1), ...] of n samples cut every `rows` rows"""
    return [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)]


def panel_cut(full, r0, r1):
    """rows [r0, r1) x columns [r0, n) of a full n x n array"""
    return np.ascontiguousarray(full[r0:r1, r0:])


def select(res, cutoff, samp_sel=None, rows=None):
    """snpgpu_pcr_select on a result dict of n x n arrays: the pairs r0 <= idx1 < r1, idx1 < idx2 < n with both samples selected and
    kinship >= cutoff -- a NaN kinship never, a non-finite cutoff every pair -- ordered by idx1, then idx2; the values are the
    entries (idx2, idx1), which snpgdsIBDSelection reads.  dict(idx1, idx2 and every name of VALUES that `res` holds)."""
    kin = res["kinship"]
    n = kin.shape[0]
    r0, r1 = (0, n) if rows is None else rows
    sel = np.ones(n, bool) if samp_sel is None else np.asarray(samp_sel) != 0
    i, j = np.triu_indices(n, 1)                                   # row-major: i ascending, then j ascending
    keep = (i >= r0) & (i < r1) & sel[i] & sel[j]
    if np.isfinite(cutoff):
        with np.errstate(invalid="ignore"):
            keep &= kin[j, i] >= cutoff
    i, j = i[keep], j[keep]
    out = dict(idx1=i.astype(np.int32), idx2=j.astype(np.int32))
    for k in VALUES:
        if res.get(k) is not None:
            out[k] = res[k][j, i]
    return out


def same_bits(a, b):
    """equal shapes and equal float64 bit patterns (NaN compared as bits)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
