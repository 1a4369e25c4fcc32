"""The selection rule of the sparse GRM (snpgpu_select_grm, snpgdsGRMPairs) restated in numpy, and a reader of the text files that
snpgdsGRMPairs(out_fn=) writes.  Nothing here imports the HIP library.

selection() takes what the kind's finaliser returns -- the packed slab of a panel's rows, or a whole n x n matrix -- and gives the
table the GPU selection must equal bit for bit: the strict upper trapezoid of the panel in row-major order (i ascending, then j
ascending), `value >= cutoff` (so a NaN value is never selected), every pair when the cutoff is not finite, and both samples in
samp_sel."""
import numpy as np

from snprelate_amd.dist import slab_range


def slab_rc(n, r0, r1):
    """(row, column) of every entry of the packed slab of rows [r0, r1) of an n x n upper triangle"""
    rows = np.arange(r0, min(r1, n))
    i = np.repeat(rows, n - rows)
    start = np.cumsum(np.concatenate([[0], (n - rows)[:-1]]))
    j = np.arange(i.size) - np.repeat(start, n - rows) + i
    return i, j


def selection(slab_or_matrix, n, rows, cutoff, samp_sel=None):
    """dict(idx1, idx2, value, diag): the pairs of the panel rows = (r0, r1) and the diagonal entries of its rows"""
    r0, r1 = rows
    a = np.asarray(slab_or_matrix, np.float64)
    i, j = slab_rc(n, r0, r1)
    if a.ndim == 2:
        assert a.shape == (n, n)
        v = a[i, j]
    else:
        lo, hi = slab_range(n, r0, r1)
        assert a.shape == (hi - lo,), (a.shape, hi - lo)
        v = a
    keep = j > i
    if np.isfinite(cutoff):
        with np.errstate(invalid="ignore"):
            keep &= v >= cutoff
    if samp_sel is not None:
        s = np.asarray(samp_sel) != 0
        keep &= s[i] & s[j]
    return dict(idx1=i[keep], idx2=j[keep], value=v[keep], diag=v[i == j])


def selection_loops(matrix, n, rows, cutoff, samp_sel=None):
    """the same by a plain double loop over a whole matrix (the check of selection() itself)"""
    i1, i2, val = [], [], []
    finite = cutoff == cutoff and cutoff not in (float("inf"), float("-inf"))
    for i in range(rows[0], min(rows[1], n)):
        for j in range(i + 1, n):
            if samp_sel is not None and not (samp_sel[i] and samp_sel[j]):
                continue
            x = matrix[i][j]
            if finite and not (x >= cutoff):
                continue
            i1.append(i); i2.append(j); val.append(x)
    return dict(idx1=np.array(i1, np.int64), idx2=np.array(i2, np.int64), value=np.array(val, np.float64),
                diag=np.array([matrix[i][i] for i in range(rows[0], min(rows[1], n))], np.float64))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same_bits(a, b):
    """equal bit for bit, except that any NaN equals any NaN (the payload of a NaN is not part of the contract)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_selection(got, ref, diag=True):
    """None, or what differs between two selection() tables"""
    if got["idx1"].size != ref["idx1"].size:
        return "%d pairs against %d" % (got["idx1"].size, ref["idx1"].size)
    for k in ("idx1", "idx2"):
        if not np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64)):
            d = np.flatnonzero(np.asarray(got[k], np.int64) != np.asarray(ref[k], np.int64))
            return "%s differs at %d positions, first %d: %d against %d" % (k, d.size, d[0], got[k][d[0]], ref[k][d[0]])
    for k in ("value", "diag") if diag else ("value",):
        if not same_bits(got[k], ref[k]):
            g, r = np.asarray(got[k]), np.asarray(ref[k])
            if g.shape != r.shape:
                return "%s: shape %s against %s" % (k, g.shape, r.shape)
            d = np.flatnonzero(~((bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))))
            return "%s differs at %d positions, first %d: %r against %r" % (k, d.size, d[0], g[d[0]], r[d[0]])
    return None


def read_sparse_grm(prefix):
    """(ids [m] as strings, row, col int64, value float64) of prefix.grm.id / prefix.grm.sp, in file order"""
    ids = []
    with open(prefix + ".grm.id") as f:
        for line in f:
            fam, ind = line.rstrip("\n").split("\t")
            assert fam == ind
            ids.append(ind)
    row, col, val = [], [], []
    with open(prefix + ".grm.sp") as f:
        for line in f:
            r, c, v = line.rstrip("\n").split("\t")
            row.append(int(r)); col.append(int(c)); val.append(float(v))
    return np.array(ids), np.array(row, np.int64), np.array(col, np.int64), np.array(val, np.float64)
