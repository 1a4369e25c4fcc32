"""snpgdsIBDSelection of the reference (R/IBD.R:463-531) restated in numpy, line by line, for tests/test_cpu_ibd_selection.py and
tests/test_gpu_ibd_selection.py.  Nothing here imports the package under test.

    ns <- setdiff(names(ibdobj), c("sample.id", "snp.id", "afreq"))
    if (!is.null(samp.sel)) { sample.id <- sample.id[samp.sel]; every ns entry <- entry[samp.sel, samp.sel] }
    if (is.null(kinship)) { from k0 / k1: (1 - k0 - k1)*0.5 + k1*0.25; from D1..D8: D1 + 0.5*(D3 + D5 + D7) + 0.25*D8; appended to ns;
                            neither and a finite cutoff: stop("There is no kinship coefficient.") }
    flag <- lower.tri(kinship) & (kinship >= cutoff); flag[is.na(flag)] <- FALSE        (finite cutoff)
    flag <- lower.tri(kinship)                                                           (otherwise)
    ii <- which(flag, TRUE)                        column-major walk: (row, col) with col ascending, then row ascending
    ID1 = sample.id[ii[, 2]], ID2 = sample.id[ii[, 1]], ans[[i]] <- ibdobj[[i]][flag]    (the same walk)

Objects are dicts of FULL n x n matrices here; samp_sel is a logical vector or 0-based indices."""
import numpy as np

NOT_PER_PAIR = ("sample_id", "snp_id", "afreq")


def selection(ibdobj, kinship_cutoff=float("nan"), samp_sel=None):
    """-> dict of columns, in the reference's column order"""
    obj = {k: v for k, v in ibdobj.items() if v is not None}                     # (a NULL entry is no entry of an R list)
    ns = [k for k in obj if k not in NOT_PER_PAIR]
    ids = np.asarray(obj["sample_id"])
    if samp_sel is not None:
        s = np.asarray(samp_sel)
        if s.dtype == bool:
            assert s.size == ids.size
        ids = ids[s]
        for k in ns:
            obj[k] = np.asarray(obj[k])[s][:, s]
    if "kinship" not in obj:
        if "k0" in obj and "k1" in obj:
            obj["kinship"] = (1 - obj["k0"] - obj["k1"]) * 0.5 + obj["k1"] * 0.25
            ns = ns + ["kinship"]
        elif "D1" in obj:
            obj["kinship"] = obj["D1"] + 0.5 * (obj["D3"] + obj["D5"] + obj["D7"]) + 0.25 * obj["D8"]
            ns = ns + ["kinship"]
        elif np.isfinite(kinship_cutoff):
            raise ValueError("There is no kinship coefficient.")
    n = ids.size
    r, c = np.indices((n, n))
    lower = r > c                                                                # lower.tri(x)
    if np.isfinite(kinship_cutoff):
        with np.errstate(invalid="ignore"):
            flag = lower & (np.asarray(obj["kinship"]) >= kinship_cutoff)        # NA & ... -> NA -> FALSE: a NaN compares False here
    else:
        flag = lower
    at = np.flatnonzero(flag.ravel(order="F"))                                   # which(): positions in column-major storage
    row, col = at % n, at // n                                                   # arr.ind
    ans = {"ID1": ids[col], "ID2": ids[row]}
    for k in ns:
        ans[k] = np.asarray(obj[k]).ravel(order="F")[at]                         # x[flag]
    return ans


def packed_to_full(p, n):
    """the packed upper triangle (row-major, diagonal included) of a symmetric matrix -> the full matrix"""
    m = np.empty((n, n), np.asarray(p).dtype)
    i, j = np.triu_indices(n)
    m[i, j] = p
    m[j, i] = p
    return m


def slab_to_rows(p, n, r0, r1, fill=np.nan):
    """the packed slab of rows [r0, r1) -> a full n x n matrix, symmetric where the slab covers it, `fill` elsewhere"""
    m = np.full((n, n), fill, np.asarray(p).dtype)
    i, j = np.triu_indices(n)
    keep = (i >= r0) & (i < r1)
    m[i[keep], j[keep]] = p
    m[j[keep], i[keep]] = p
    return m


def panel_selection(obj, n, r0, r1, kinship_cutoff=float("nan"), samp_sel=None):
    """selection() restricted to the pairs whose EARLIER sample (ID1) lies in rows [r0, r1): what one row panel holds.  obj: full
    matrices over sample_id = 0..n-1 (entries outside the panel's rows may be anything)."""
    t = selection(obj, kinship_cutoff, samp_sel)
    keep = (t["ID1"] >= r0) & (t["ID1"] < r1)
    return {k: v[keep] for k, v in t.items()}


def same_table(got, ref):
    """column names in order, then every column bit for bit (NaN equal to NaN); returns a message or None"""
    if list(got) != list(ref):
        return "columns %s against %s" % (list(got), list(ref))
    for k in ref:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.shape != b.shape:
            return "%s: %s rows against %s" % (k, a.shape, b.shape)
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
            bad = ~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))      # (the sign of a zero counts)
        else:
            bad = a != b
        if bad.any():
            w = np.flatnonzero(bad)
            return "%s differs at %d of %d rows, first %d: %r against %r" % (k, w.size, a.size, w[0], a[w[0]], b[w[0]])
    return None
