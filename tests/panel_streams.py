"""Inputs, references and comparisons of the row-panel x finaliser tests (tests/test_cpu_panel_streams.py without a GPU,
tests/test_gpu_panel_finalisers.py with one).  Nothing here imports the HIP library.

A row panel is a context created with row_begin / row_end.  Its finalisers mix panel-relative indices (the accumulator planes, msum,
called), absolute ones (fam, diag, het, dmiss, dsq) and offsets into the packed slab; a slip between the first two is invisible on
every full context (row0 == 0) and wrong on every later panel.  So everything here lives on the smallest shapes with three panels at
PANEL_ALIGN = 256:
  n = 531  bounds 0 / 256 / 512 / 531: the last panel has 19 rows -- not a multiple of the finalisers' 32-row groups, ending in
           padding, 256 padded columns against 19 real ones
  n = 513  bounds 0 / 256 / 512 / 513: the last panel is one row and one entry
and two SNP streams per sample count, fed in blocks of at most BMAX = 1024 SNPs:
  mixed    blocks of 700 (6 % missing), 1024 (none), 300 (6 % missing), 64 (none): both kernel families and the pending het / wc / msum
           terms meet in one result; a monomorphic SNP in a block without missing calls, an all-missing SNP in a block with them
  holes    blocks of 700 and 300, both with missing calls; sample 300 is missing at every SNP, sample 40 is called only in the first
           half of the SNPs and sample 520 (512 at n = 513) only in the second: the pair (40, 520) shares no call and lies in panel 0,
           the pair (300, 520) in panel 1
The family vector of the KING-robust tests is family_vector().

References come from the CPU oracle and tests/diss_ref.py alone, on the whole matrix, once per stream (stream() caches the object,
the object caches its references, all read-only); slab() cuts a panel's range out of one.  The check_* functions are the comparisons
of the GPU tests: each prints its largest figure before it asserts, and names the (row, column) pattern of what failed."""
import functools

import numpy as np

import diss_ref as R
import oracle as orc
from norms import tri_diag_scale
from oracle.synth import synth_geno
from snprelate_amd.dist import slab_range

PANEL_ALIGN = 256
FIN_ROWS = 32                          # rows a finaliser workgroup walks (kernels_final.hip)
BMAX = 1024                            # max_block_snps of every context
SAMPLE_COUNTS = (531, 513)
BLOCKS = {                             # stream: (SNPs, with missing calls) per block
    "mixed": ((700, True), (1024, False), (300, True), (64, False)),
    "holes": ((700, True), (300, True)),
}
MISSING_RATE = 0.06
NEVER_CALLED = 300                     # holes: missing at every SNP
FIRST_HALF_ONLY = 40                   # holes: called in the first half of the SNPs only


def diss_rows(n):
    """the rows tests/diss_ref.py is evaluated on: the first and last rows of every panel, the samples of the holes, some others"""
    last = [512, 513, 520, 528, 529, 530] if n == 531 else [512]
    return np.array([0, 1, 40, 100, 255, 256, 257, 270, 300, 400, 511] + last)


def second_half_only(n):
    """holes: the sample called in the second half of the SNPs only (a column of the last panel)"""
    return 520 if n == 531 else 512


def bounds(n):
    return [0, PANEL_ALIGN, 2 * PANEL_ALIGN, n]


def panels(n):
    """[(row_begin, row_end)] of the three panels"""
    b = bounds(n)
    return list(zip(b[:-1], b[1:]))


def slab(ref, n, r0, r1):
    """the packed rows [r0, r1) of a whole-triangle reference (first axis)"""
    lo, hi = slab_range(n, r0, r1)
    return ref[lo:hi]


@functools.lru_cache(maxsize=None)
def _tri_rc(n):
    i, j = np.triu_indices(n)
    i.setflags(write=False)
    j.setflags(write=False)
    return i, j


def slab_rc(n, r0, r1):
    """(row, column) of every entry of the packed slab of rows [r0, r1)"""
    i, j = _tri_rc(n)
    return slab(i, n, r0, r1), slab(j, n, r0, r1)


def diag_offsets(n, r0, r1):
    """offsets of the diagonal entries (i, i), r0 <= i < r1, within the slab of rows [r0, r1)"""
    i = np.arange(r0, r1, dtype=np.int64)
    return i * n - i * (i - 1) // 2 - slab_range(n, r0, r1)[0]


def tri_idx(n, i, j):
    return j + i * (2 * n - i - 1) // 2


# ---- the family vector ---------------------------------------------------------------------------------------------------------------

def family_pairs(n):
    """the same-family pairs placed on purpose, as {name: (row, column)}; with row0 the first row of the pair's panel, the ids make
    fam[row - row0] == fam[column] false for every pair of a later panel, so a panel-relative lookup gives another answer"""
    hi = second_half_only(n)
    p = {"inside_panel_0": (10, 30), "inside_panel_1": (260, 400), "panel_0_to_last": (100, hi), "panel_1_to_last": (310, hi)}
    if n == 531:
        p["inside_panel_2"] = (514, 530)           # (at n = 513 the last panel is its diagonal entry alone)
    return p


def family_vector(n):
    """int32 [n]: about a third of the samples NA (-1), the others in families of 2 to 4 members.  Placed by hand: {10, 20, 30} inside
    panel 0, {260, 400} inside panel 1, {514, 530} inside panel 2 (n = 531), {100, 310, 520 or 512} with a row in panel 0, a row in
    panel 1 and a column of the last panel.  The samples a panel-relative row lookup would read for the pairs of panels 1 and 2
    (260 - 256, 310 - 256, 514 - 512) are NA."""
    hi = second_half_only(n)
    placed = {10: 1, 20: 1, 30: 1, 260: 2, 400: 2, 100: 3, 310: 3, hi: 3}
    na = {260 - 256, 310 - 256, 514 - 512}
    if n == 531:
        placed.update({514: 4, 530: 4})
    fam = np.full(n, -1, np.int32)
    rng = np.random.default_rng(7 * n)
    pool = rng.permutation([s for s in range(n) if s not in placed and s not in na])
    pool = pool[n // 3 - len(na):]                 # the first ones stay NA
    k, fid = 0, 100
    while k < pool.size:
        size = 2 + fid % 3
        if pool.size - k - size == 1:              # no family of one at the end
            size += 1 if size < 4 else -1
        fam[pool[k:k + size]] = fid
        k, fid = k + size, fid + 1
    for s, f in placed.items():
        fam[s] = f
    fam.setflags(write=False)
    return fam


# ---- the streams ---------------------------------------------------------------------------------------------------------------------

def _make_geno(name, n):
    sizes = [s for s, _ in BLOCKS[name]]
    cuts = np.cumsum([0] + sizes)
    L = int(cuts[-1])
    g = synth_geno(n, L, missing=0.0, seed=2000 + n + (0 if name == "mixed" else 50), special=False)
    rng = np.random.default_rng(n + len(name))
    for b, (_, miss) in enumerate(BLOCKS[name]):
        if miss:
            sub = g[cuts[b]:cuts[b + 1]]
            sub[rng.random(sub.shape) < MISSING_RATE] = 3
    if name == "mixed":
        g[cuts[1] + 5] = 2                         # a monomorphic SNP in a block without missing calls
        g[cuts[0] + 9] = 3                         # an all-missing SNP in a block with them
    else:
        g[:, NEVER_CALLED] = 3
        g[L // 2:, FIRST_HALF_ONLY] = 3
        g[:L // 2, second_half_only(n)] = 3
    g.setflags(write=False)
    return g, cuts


def _frozen(x):
    for a in (x if isinstance(x, tuple) else (x,)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


class Stream:
    """the genotypes of one stream at one sample count and the whole-matrix references, each computed once and left unchanged"""

    def __init__(self, name, n):
        self.name, self.n = name, n
        self.g, self.cuts = _make_geno(name, n)
        self.fam = family_vector(n)
        self._cache = {}

    def blocks(self):
        return [self.g[a:b] for a, b in zip(self.cuts[:-1], self.cuts[1:])]

    def ref(self, key, fn):
        if key not in self._cache:
            self._cache[key] = _frozen(fn())
        return self._cache[key]

    def ibs(self):
        """uint32 [pairs, 3]: IBS0, IBS1, IBS2"""
        return self.ref("ibs", lambda: orc.ibs_count(self.g))

    def ibs_ave(self):
        return self.ref("ibs_ave", lambda: orc.ibs_ave(self.ibs(), self.n))

    def mom_expect(self):
        return self.ref("mom_e", lambda: orc.mom_expect(self.g)[0])

    def mom(self, constraint):
        return self.ref("mom%d" % constraint, lambda: orc.mom_final(self.ibs(), self.n, self.mom_expect(), constraint))

    def king_counts(self):
        return self.ref("king_cnt", lambda: orc.king_robust_count(self.g))

    def king_robust(self, family):
        """family: None, "fam" (the family vector) or "one" (every sample in one family: the family branch at every pair)"""
        vec = {None: None, "fam": self.fam, "one": np.zeros(self.n, np.int32)}[family]
        return self.ref("king_%s" % family, lambda: orc.king_robust_final(self.king_counts(), self.n, vec))

    def king_homo(self):
        return self.ref("king_homo", lambda: orc.king_homo_final(*orc.king_homo_count(self.g), self.n))

    def diss(self):
        """tests/diss_ref.py on the rows diss_rows(n) x every column, as packed triangles with a mask: (known, SumGeno int64, SumAFreq,
        dissimilarity) -- known where the row OR the column of the pair is one of diss_rows(n), so every row of every panel has
        entries.  (diss_ref's integer products take 17 s on the whole matrix at these sizes; SumGeno of every pair comes from the
        oracle's KING-robust counters, see diss_sum_geno_from_king.)"""
        def fn():
            n, rows = self.n, diss_rows(self.n)
            sg, sa = R.diss_sums(self.g, rows=rows)
            with np.errstate(invalid="ignore", divide="ignore"):
                d = sg / sa
            d[np.arange(rows.size), rows] *= 2                        # (diss_ref.diss_matrix, on the sums at hand)
            c = np.arange(n)[None, :]
            at = tri_idx(n, np.minimum(rows[:, None], c), np.maximum(rows[:, None], c))
            size = n * (n + 1) // 2
            known, psg, psa, pd = np.zeros(size, bool), np.zeros(size, np.int64), np.zeros(size), np.zeros(size)
            known[at], psg[at], psa[at], pd[at] = True, sg, sa, d
            return known, psg, psa, pd
        return self.ref("diss", fn)

    def diss_sum_geno_from_king(self):
        """SumGeno = SumSq + N1_Aa + N2_Aa of the oracle's KING-robust counters (the second route of test_gpu_diss)"""
        def fn():
            k = self.king_counts().astype(np.int64)
            return k[:, 2] + k[:, 3] + k[:, 4]
        return self.ref("diss_sg", fn)

    def grm(self):
        return self.ref("grm", lambda: orc.grm_gcta(self.g))

    def cov_raw(self, bayes=False):
        return self.ref("cov%d" % bayes, lambda: orc.pca_cov(self.g, bayes))

    def cov_norm(self, bayes=False):
        """(trace-normalised covariance, TraceXTX)"""
        def fn():
            c = self.cov_raw(bayes).copy()
            tr = orc.trace_normalize(c, self.n)
            return c, tr
        return self.ref("covn%d" % bayes, fn)

    def eigmix(self, diagadj):
        return self.ref("eigmix%d" % diagadj, lambda: orc.eigmix(self.g, diagadj)[0])


@functools.lru_cache(maxsize=None)
def stream(name, n):
    return Stream(name, n)


def holes_nan_pairs(n, diagonal):
    """the pairs (row <= column) of the holes stream without a shared call: every pair with NEVER_CALLED, and (FIRST_HALF_ONLY,
    second_half_only(n)).  diagonal: with (NEVER_CALLED, NEVER_CALLED) (ibs_ave; KING-robust sets its diagonal to constants)"""
    s = {(min(k, NEVER_CALLED), max(k, NEVER_CALLED)) for k in range(n) if k != NEVER_CALLED}
    s.add((FIRST_HALF_ONLY, second_half_only(n)))
    if diagonal:
        s.add((NEVER_CALLED, NEVER_CALLED))
    return s


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
# A context is named by what the messages need: the stream object and the rows (r0, r1) of the slab at hand ((0, n): the whole triangle).

def where(mask, s, rows, got=None, ref=None):
    """the (row, column) pattern of the slab entries flagged in mask, for an assertion message (with got / ref: the first values too)"""
    mask = np.asarray(mask)
    if mask.ndim > 1:
        mask = mask.any(axis=tuple(range(1, mask.ndim)))
    i, j = slab_rc(s.n, *rows)
    k = np.flatnonzero(mask)
    if not k.size:
        return "no entry"
    bi, bj = i[k], j[k]
    return ("%d of %d entries of rows %d..%d (stream %s, n %d): rows %d..%d (%d distinct), columns %d..%d (%d distinct), %d on the diagonal; "
            "first (row, column): %s%s" % (k.size, mask.size, rows[0], rows[1], s.name, s.n, bi.min(), bi.max(), np.unique(bi).size, bj.min(),
                                           bj.max(), np.unique(bj).size, int((bi == bj).sum()), list(zip(bi[:8].tolist(), bj[:8].tolist())),
                                           "" if got is None else "; got %s against %s" % (np.asarray(got)[k[:8]].tolist(),
                                                                                           np.asarray(ref)[k[:8]].tolist())))


def all_of(*checks):
    """run every check; what fails in one does not keep the others from running"""
    failed = []
    for check in checks:
        try:
            check()
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def _report(label, s, rows, figure, bound):
    print("PANEL-FIGURE %-28s stream %-5s n %d rows %3d..%3d: %.3g (bound %.3g)" % (label, s.name, s.n, rows[0], rows[1], figure, bound))


def check_exact(label, got, ref, s, rows):
    """bit for bit (NaN equal to NaN)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, "%s: shape %s against %s" % (label, got.shape, ref.shape)
    if np.issubdtype(got.dtype, np.floating):
        bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    else:
        bad = got != ref
    _report(label + " (entries that differ)", s, rows, float(bad.sum()), 0)
    assert not bad.any(), "%s differs at %s" % (label, where(bad, s, rows, got, ref))


def check_close(label, got, ref, s, rows, rtol, atol=0.0):
    """numpy.testing.assert_allclose(got, ref, rtol, atol, equal_nan=True) -- |got - ref| <= atol + rtol |ref|, NaN where the reference
    has NaN and the same infinities -- with the largest error / bound printed and the failing pattern named"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, "%s: shape %s against %s" % (label, got.shape, ref.shape)
    placed = (np.isnan(got) != np.isnan(ref)) | (np.isinf(got) != np.isinf(ref))
    fin = np.isfinite(ref) & np.isfinite(got)      # (the figure covers every entry that is a number on both sides)
    bad = np.isinf(ref) & ~placed & (got != ref)   # infinities of the same sign
    err = np.abs(got[fin] - ref[fin])
    tol = atol + rtol * np.abs(ref[fin])
    bad[fin] = err > tol
    with np.errstate(divide="ignore", invalid="ignore"):
        fig = float(np.max(np.where(err > 0, err / tol, 0.0))) if err.size else 0.0
    _report(label + " (error / bound)", s, rows, fig, 1.0)
    assert not placed.any(), "%s: NaN / Inf placement differs at %s%s" % (
        label, where(placed, s, rows, got, ref), "; and beyond the tolerance at %s" % where(bad, s, rows, got, ref) if bad.any() else "")
    assert not bad.any(), "%s beyond rtol %g atol %g (largest error / bound %.3g) at %s" % (label, rtol, atol, fig, where(bad, s, rows, got, ref))


def rel_err(got, ref, whole):
    """tests/norms.py on a part of a matrix: per entry |got - ref| / (|ref| + floor), the larger of the contract figure (floor = the
    median diagonal entry) and the off-diagonal figure (floor = the median |entry|), both floors those of the WHOLE reference -- each
    entry is held to the bound the one-shot tests (test_gpu_between_feeds._rel_err) hold it to.  Returns the figure per entry."""
    got, ref, whole = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(whole, np.float64)
    n = int((np.sqrt(8 * whole.size + 1) - 1) / 2 + 0.5)
    a = np.abs(whole[np.isfinite(whole)])
    floor = min(tri_diag_scale(whole, n), float(np.median(a)))
    fin = np.isfinite(ref)
    out = np.zeros(ref.shape)
    out[fin] = np.abs(got[fin] - ref[fin]) / (np.abs(ref[fin]) + floor)
    out[fin & ~np.isfinite(got)] = np.inf
    return out


def check_rel(label, got, ref, whole, s, rows, only=None, bound=1e-5):
    """rel_err < bound (1e-5: `_rel_err < 1e-5` of the one-shot tests) over the slab, or over the offsets `only` of it"""
    e = rel_err(got, ref, whole)
    if only is not None:
        keep = np.zeros(e.shape, bool)
        keep[only] = True
        e = np.where(keep, e, 0.0)
    fig = float(e.max()) if e.size else 0.0
    _report(label + " (rel err)", s, rows, fig, bound)
    assert fig < bound, "%s: rel err %.3g, not below %g, at %s" % (label, fig, bound, where(e >= bound, s, rows))


# what the GPU tests call per kind; `got` is what the panel's finalisers returned, `s` the stream, rows = (r0, r1)

def check_ibs(got_num, got_ave, got_mom, s, rows):
    """counts array_equal; ibs_ave array_equal with the oracle's (test_gpu_parity.test_ibs_counts_bit_exact: `np.array_equal(ave,
    orc.ibs_ave(ref, n))`, NaN at the pairs without a shared call); MoM rtol=1e-12, atol=1e-14, equal_nan
    (test_gpu_between_feeds._check_ibs)"""
    ref = slab(s.ibs(), s.n, *rows)
    for k in range(3):
        check_exact("ibs_num[%d]" % k, got_num[k], ref[:, k].astype(np.int32), s, rows)
    check_exact("ibs_ave", got_ave, slab(s.ibs_ave(), s.n, *rows), s, rows)
    for cons in (False, True):
        for k in range(2):
            check_close("ibd_mom(constraint=%s)[%d]" % (cons, k), got_mom[cons][k], slab(s.mom(cons)[k], s.n, *rows), s, rows,
                        rtol=1e-12, atol=1e-14)


def check_king_counts(got, s, rows):
    check_exact("king_robust_counts", got, slab(s.king_counts(), s.n, *rows), s, rows)


def check_king_robust(got, family, s, rows):
    """`np.array_equal(..., equal_nan=True)` against king_robust_final (test_gpu_api_golden.test_multi_panel_drivers_single_rank)"""
    ref = s.king_robust(family)
    for k, name in enumerate(("ibs0", "kinship")):
        check_exact("king_robust(family=%s) %s" % (family, name), got[k], slab(ref[k], s.n, *rows), s, rows)


def check_king_homo(got, s, rows):
    """test_gpu_between_feeds._check_king_homo: `rtol=1e-5, atol=1e-7, equal_nan=True` (k0), `rtol=1e-5, atol=2e-5, equal_nan=True` (k1)"""
    r0, r1 = s.king_homo()
    all_of(lambda: check_close("king_homo k0", got[0], slab(r0, s.n, *rows), s, rows, rtol=1e-5, atol=1e-7),
           lambda: check_close("king_homo k1", got[1], slab(r1, s.n, *rows), s, rows, rtol=1e-5, atol=2e-5))


def check_diss(got_sg, got_sa, got_d, s, rows):
    """SumGeno exact at every pair (the oracle's KING-robust counters: SumSq + N1_Aa + N2_Aa, the second route of
    test_gpu_diss.test_sum_geno_bit_exact).  Against tests/diss_ref.py, at the pairs whose row or column is one of diss_rows(n):
    SumGeno exact, SumAFreq `rtol=_rtol(g), atol=1e-9` and the dissimilarity `rtol=_rtol(g), equal_nan=True` with
    test_gpu_diss._rtol = 2e-6 (both streams hold blocks with missing calls).  NaN at every pair of the slab exactly where the pair
    shares no call (the oracle's IBS counts), no infinity anywhere."""
    known, rsg, rsa, rd = (slab(x, s.n, *rows) for x in s.diss())
    check_exact("diss SumGeno (KING counters)", got_sg.astype(np.int64), slab(s.diss_sum_geno_from_king(), s.n, *rows), s, rows)
    nan_ref = slab(s.ibs(), s.n, *rows).sum(axis=1) == 0

    def placement():
        bad = (np.isnan(got_d) != nan_ref) | np.isinf(got_d)
        assert not bad.any(), "diss: NaN / Inf placement differs at %s" % where(bad, s, rows, got_d, np.where(nan_ref, np.nan, 0.0))
    sel = np.flatnonzero(known)
    assert sel.size >= rows[1] - rows[0]

    def part(label, got, ref, **tol):              # (slab-sized arrays, so that the messages name entries of the slab)
        full_got, full_ref = np.zeros(known.shape), np.zeros(known.shape)
        full_got[sel], full_ref[sel] = got[sel], ref[sel]
        if tol:
            check_close(label, full_got, full_ref, s, rows, **tol)
        else:
            check_exact(label, full_got, full_ref, s, rows)
    all_of(placement,
           lambda: part("diss SumGeno", got_sg.astype(np.float64), rsg.astype(np.float64)),
           lambda: part("diss SumAFreq", got_sa, rsa, rtol=2e-6, atol=1e-9),
           lambda: part("diss", got_d, rd, rtol=2e-6))


def check_gcta(got, s, rows):
    """`_rel_err < 1e-5` and the finite entries where the reference has them (test_gpu_between_feeds._check_gcta)"""
    ref = slab(s.grm(), s.n, *rows)
    bad = np.isfinite(got) != np.isfinite(ref)
    assert not bad.any(), "grm_gcta: finite / non-finite placement differs at %s" % where(bad, s, rows)
    check_rel("grm_gcta", got, ref, s.grm(), s, rows)


def check_cov(got, s, rows, bayes, normalized):
    whole = s.cov_norm(bayes)[0] if normalized else s.cov_raw(bayes)
    check_rel("pca_cov(normalize=%s%s)" % (normalized, ", bayesian" if bayes else ""), got, slab(whole, s.n, *rows), whole, s, rows)


def check_trace(got, s, bayes):
    """`abs(tr - tr_ref) / tr_ref < 1e-6` (test_gpu_between_feeds._check_pca)"""
    ref = s.cov_norm(bayes)[1]
    fig = abs(got - ref) / ref
    _report("TraceXTX%s (rel)" % (" bayesian" if bayes else ""), s, (0, s.n), fig, 1e-6)
    assert fig < 1e-6, "trace %r against %r" % (got, ref)


def check_eigmix(got, diagadj, s, rows, scale=1.0):
    """`_rel_err < 1e-5` (test_gpu_between_feeds._check_eigmix) over all entries and, separately, over the diagonal entries alone"""
    whole = s.eigmix(diagadj)
    if scale != 1.0:
        whole = s.ref("eigmix%d_x%g" % (diagadj, scale), lambda: whole * scale)
    ref = slab(whole, s.n, *rows)
    label = "eigmix(diagadj=%s%s)" % (diagadj, "" if scale == 1.0 else ", scale=%g" % scale)
    check_rel(label, got, ref, whole, s, rows)
    check_rel(label + " diagonal", got, ref, whole, s, rows, only=diag_offsets(s.n, *rows))
