"""Every finaliser and every gather on ROW PANELS (contexts created with row_begin / row_end: what snpgpu_multi_*, dist.py and the
solver beyond the dense limit run on), not only GRM and PCA.  The finalisers of kernels_final.hip mix panel-relative indices, absolute
ones and packed-slab offsets; a slip between the first two is right on every full context and wrong on every later panel.

Inputs, references (the CPU oracle and tests/diss_ref.py, whole matrix, once) and the comparison functions are tests/panel_streams.py;
tests/test_cpu_panel_streams.py shows without a GPU that those inputs and comparisons catch the defect class.  Here: for every stream
and sample count the three panel contexts of a kind are fed the same blocks, every finaliser of the kind is read with packed=True and
the WHOLE slab is compared, every entry, with the tolerance of the kind's one-shot test (quoted in panel_streams.check_*).  The counter
kinds also equal, bit for bit, the same range of a full context fed the same blocks.  Then EIGMIX panels finalised in place (read-back,
panel_entries, the Krylov solver), and the gathers of snpgpu_multi_king_homo / _eigmix / _ibs_ave / _pca_trace.  No GPU run is ever the
reference of another, except where equality with one is the statement (full context, gather = placed slabs, frozen read-back).

Largest figures of one run on an MI355X (the comparisons print theirs as PANEL-FIGURE lines, `pytest -s`), each against its bound:
  IBS                ibs_num, ibs_ave exact; ibd_mom error 0 of rtol 1e-12; all equal to the full context bit for bit
  KING_ROBUST        counters and both finalisers (with and without the family vector) exact, and equal to the full context
  KING_HOMO          k0 0.0142, k1 0.0136 of their tolerances (holes stream; mixed 0.0039 / 0.0055)
  DISS               SumGeno exact; SumAFreq and the dissimilarity 0.135 of rtol 2e-6 (holes; mixed 0.022)
  GRM_GCTA           2.5e-6 (mixed), 1.4e-6 (holes) against 1e-5
  PCA_COV            2.5e-6, Bayesian 2.6e-6 against 1e-5, raw and normalised; TraceXTX 2.9e-8, Bayesian 4.1e-8 against 1e-6
  EIGMIX             1.1e-6 against 1e-5 for either diagadj and scale = 2; the diagonal alone 3.5e-9 (diagadj) and 4.7e-9
  frozen EIGMIX      read-back error 0 of rtol 1e-13, panel_entries exact; top-8 eigenvalues 3.8e-9 against 2e-5, max_rel_residual
                     3.9e-10 against 1e-8, 42 panel products, 0.3 s for the first of the two tests and 0.07 s for the other
  gathers            each bit for bit the placed slabs of its panels; against the oracle as the kinds above; the object cuts 531
                     samples into the two panels 0..256 and 256..531 in both layouts"""
import contextlib
import functools

import numpy as np
import pytest

import oracle as orc
import panel_streams as P

pytestmark = pytest.mark.gpu

MIXED = [("mixed", 531), ("mixed", 513)]
WITH_HOLES = MIXED + [("holes", 531)]


@contextlib.contextmanager
def _panel_contexts(kind, s, **kw):
    """[(context, (row_begin, row_end))] of the three panels, each fed every block of the stream"""
    from snprelate_amd import _lib
    ctx = []
    try:
        for r0, r1 in P.panels(s.n):
            a = _lib.Accumulator(getattr(_lib, kind), s.n, row_begin=r0, row_end=r1, max_block_snps=P.BMAX, **kw)
            ctx.append((a, (r0, r1)))
            assert not a.full
            lo, hi = P.slab_range(s.n, r0, r1)
            assert a.slab_size() == hi - lo
        for block in s.blocks():
            for a, _ in ctx:
                a.feed(block)
        yield ctx
    finally:
        for a, _ in ctx:
            a.close()


@contextlib.contextmanager
def _full_context(kind, s, **kw):
    from snprelate_amd import _lib
    with _lib.Accumulator(getattr(_lib, kind), s.n, max_block_snps=P.BMAX, **kw) as a:
        for block in s.blocks():
            a.feed(block)
        yield a


def _on_every_panel(ctx, check):
    """check(context, rows) on every panel; what fails on one panel does not keep the others from being checked"""
    failed = []
    for a, rows in ctx:
        try:
            check(a, rows)
        except AssertionError as e:
            failed.append("rows %d..%d: %s" % (rows[0], rows[1], e))
    assert not failed, "\n".join(failed)


def _refuses_full_matrix(read):
    from snprelate_amd import _lib
    with pytest.raises(_lib.SnpGpuError, match="full-matrix output needs a full"):
        read()


# ---- the counter kinds ---------------------------------------------------------------------------------------------------------------

def _read_ibs(a, e):
    return [a.ibs_num(packed=True), a.ibs_ave(packed=True),
            {c: a.ibd_mom(e, constraint=c, packed=True) for c in (False, True)}]


@pytest.mark.parametrize("name,n", WITH_HOLES)
def test_ibs_panels(name, n):
    """ibs_num (per context), ibs_ave and ibd_mom on IBS panels"""
    s = P.stream(name, n)
    e = s.mom_expect()
    with _full_context("IBS", s) as a:
        f_num, f_ave, f_mom = _read_ibs(a, e)
    with _panel_contexts("IBS", s) as ctx:
        for a, rows in ctx:
            num, ave, mom = _read_ibs(a, e)
            P.check_ibs(num, ave, mom, s, rows)
            for k in range(3):
                P.check_exact("ibs_num[%d] against the full context" % k, num[k], P.slab(f_num[k], n, *rows), s, rows)
            P.check_exact("ibs_ave against the full context", ave, P.slab(f_ave, n, *rows), s, rows)
            for c in (False, True):
                for k in range(2):
                    P.check_exact("ibd_mom against the full context", mom[c][k], P.slab(f_mom[c][k], n, *rows), s, rows)
            _refuses_full_matrix(lambda: a.ibs_num(packed=False))
            _refuses_full_matrix(lambda: a.ibs_ave(packed=False))
            _refuses_full_matrix(lambda: a.ibd_mom(e, packed=False))


@pytest.mark.parametrize("name,n", WITH_HOLES)
def test_king_robust_panels_with_a_family_vector(name, n):
    """king_robust_counts, king_robust(family=None) and king_robust with a FAMILY VECTOR (fam[i], fam[j] at absolute i, j)"""
    s = P.stream(name, n)
    with _full_context("KING_ROBUST", s) as a:
        f_cnt = a.king_robust_counts()
        f_fin = {fam: a.king_robust(family=s.fam if fam else None, packed=True) for fam in (None, "fam")}
    with _panel_contexts("KING_ROBUST", s) as ctx:
        for a, rows in ctx:
            cnt = a.king_robust_counts()
            P.check_king_counts(cnt, s, rows)
            P.check_exact("king_robust_counts against the full context", cnt, P.slab(f_cnt, n, *rows), s, rows)
            for fam in (None, "fam", None):                    # (and without the vector again, after a call with one)
                got = a.king_robust(family=s.fam if fam else None, packed=True)
                P.check_king_robust(got, fam, s, rows)
                for k in range(2):
                    P.check_exact("king_robust(family=%s) against the full context" % fam, got[k], P.slab(f_fin[fam][k], n, *rows), s, rows)
            _refuses_full_matrix(lambda: a.king_robust(family=s.fam, packed=False))


@pytest.mark.parametrize("name,n", WITH_HOLES)
def test_king_homo_panels(name, n):
    """king_homo on all three panels, the ragged last one included, on streams that alternate blocks with and without missing calls
    (wc, msum and het_settle together) or hold samples without calls.

    The holes stream found two defects, both fixed.  A sample without any call had k0 = k1 = 0 with all 530 others where the reference
    has NaN: FinKingHomo now reads the `called` flags the dissimilarity has.  And the pair (40, 520) of panel 0 -- two samples that are
    called, one in the first half of the SNPs and one in the second, and share no call -- had k0 = k1 = 0.0 against NaN: the weight sum
    C - M_i - M_j + B_ij is a rounding residue there, not 0.  Such pairs are now found exactly (kernels_final.hip, nosh_*)."""
    s = P.stream(name, n)

    def check(a, rows):
        for _ in range(2):                                     # a second request after the rank-one terms were settled
            P.check_king_homo(a.king_homo(packed=True), s, rows)
        _refuses_full_matrix(lambda: a.king_homo(packed=False))
    with _panel_contexts("KING_HOMO", s) as ctx:
        _on_every_panel(ctx, check)


@pytest.mark.parametrize("name,n", WITH_HOLES)
def test_diss_panels(name, n):
    """diss_sums and diss.

    The pair (40, 520) of the holes stream, two called samples without a shared call, had -0.0 where the reference has NaN: SumGeno 0
    over a SumAFreq of -4.53e-06, a rounding residue (the other SumAFreq of that panel are around 1300).  Fixed with KING-homo's, see
    test_king_homo_panels."""
    s = P.stream(name, n)

    def check(a, rows):
        sg, sa = a.diss_sums()
        P.check_diss(sg, sa, a.diss(packed=True), s, rows)
        _refuses_full_matrix(lambda: a.diss(packed=False))
    with _panel_contexts("DISS", s) as ctx:
        _on_every_panel(ctx, check)


@functools.lru_cache(maxsize=None)
def _interleaved():
    """300 samples x 3 blocks of 400 SNPs with 3 % missing calls; sample 5 is called at the even SNPs only, samples 7 and 290 at the odd
    ones only, sample 100 is missing at a random 55 % and sample 101 at a random 50 % of the SNPs, sample 200 in the whole second block;
    with the references (KING-homo k0, k1 of the oracle, the dissimilarity of tests/diss_ref.py) and the pairs without a shared call"""
    from conftest import synth_geno
    n, L = 300, 1200
    g = synth_geno(n, L, missing=0.03, seed=77, special=False)
    rng = np.random.default_rng(78)
    g[1::2, 5] = 3
    g[0::2, 7] = 3
    g[0::2, 290] = 3
    g[rng.random(L) < 0.55, 100] = 3
    g[rng.random(L) < 0.50, 101] = 3
    g[400:800, 200] = 3
    g.setflags(write=False)
    import diss_ref as R
    ref = list(orc.king_homo_final(*orc.king_homo_count(g), n)) + [R.packed_upper(R.diss_matrix(g))]      # whole matrix, once
    return g, ref, orc.ibs_count(g).sum(axis=1) == 0


@pytest.mark.parametrize("rows", [(0, 300), (0, 256), (256, 300)])
def test_pairs_without_a_shared_call_interleaved(rows):
    """Pairs without a shared call whose calls alternate SNP by SNP (every one of them missing at half the SNPs of every block), next
    to samples that miss as much and share calls with everyone: NaN exactly at (5, 7) and (5, 290), as the reference has it, on a full
    context and on both row panels; the tolerances are those of check_king_homo / test_gpu_diss (rtol 2e-6)."""
    from snprelate_amd import _lib
    g, whole, unshared = _interleaved()
    n = g.shape[1]
    i, j = P.slab_rc(n, *rows)
    lo, hi = P.slab_range(n, *rows)
    none_shared = ((i == 5) & ((j == 7) | (j == 290)))
    assert np.array_equal(unshared[lo:hi], none_shared)
    ref = [x[lo:hi] for x in whole]
    kw = {} if rows == (0, n) else {"row_begin": rows[0], "row_end": rows[1]}
    got = []
    for kind in (_lib.KING_HOMO, _lib.DISS):
        with _lib.Accumulator(kind, n, max_block_snps=512, **kw) as a:
            for k in range(0, g.shape[0], 400):
                a.feed(g[k:k + 400])
            got += list(a.king_homo(packed=True)) if kind == _lib.KING_HOMO else [a.diss(packed=True)]
    for x, r, tol in zip(got, ref, ({"rtol": 1e-5, "atol": 1e-7}, {"rtol": 1e-5, "atol": 2e-5}, {"rtol": 2e-6})):
        if rows[0] == 0:
            assert np.isnan(r[none_shared]).all() and none_shared.sum() == 2
        assert np.array_equal(np.isnan(x), np.isnan(r)) and np.array_equal(np.isinf(x), np.isinf(r)), \
            list(zip(i[np.isnan(x) != np.isnan(r)].tolist(), j[np.isnan(x) != np.isnan(r)].tolist()))[:8]
        np.testing.assert_allclose(x, r, equal_nan=True, **tol)


# ---- the fp64 kinds ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", WITH_HOLES)
def test_gcta_panels(name, n):
    """(the holes stream too: its per-sample missing counts are all, half or 6 % of the SNPs -- diag[i] at absolute i)"""
    s = P.stream(name, n)
    with _panel_contexts("GRM_GCTA", s) as ctx:
        for a, rows in ctx:
            P.check_gcta(a.grm_gcta(packed=True), s, rows)
            _refuses_full_matrix(lambda: a.grm_gcta(packed=False))


@pytest.mark.parametrize("bayes", [False, True])
@pytest.mark.parametrize("name,n", MIXED)
def test_pca_cov_panels(name, n, bayes):
    """pca_cov(normalize=False), pca_panel_trace summed over the panels, pca_cov(normalize=True, trace_in=that sum) and the refusal
    without trace_in; Bayesian panels too"""
    from snprelate_amd import _lib
    s = P.stream(name, n)
    with _panel_contexts("PCA_COV", s, bayesian=bayes) as ctx:
        trace = 0.0
        for a, rows in ctx:
            raw, _ = a.pca_cov(packed=True, normalize=False)
            P.check_cov(raw, s, rows, bayes, normalized=False)
            trace += a.pca_panel_trace()
        P.check_trace(trace, s, bayes)
        for a, rows in ctx:
            norm, _ = a.pca_cov(packed=True, normalize=True, trace_in=trace)
            P.check_cov(norm, s, rows, bayes, normalized=True)
            with pytest.raises(_lib.SnpGpuError, match="needs trace_in"):
                a.pca_cov(packed=True, normalize=True)
            _refuses_full_matrix(lambda: a.pca_cov(packed=False, normalize=False))


@pytest.mark.parametrize("name,n", MIXED)
def test_eigmix_panels_with_and_without_diagadj(name, n):
    """eigmix(diagadj=True): the diagonal branch (dsq[i], het[i] at absolute i) on panels with row0 > 0"""
    s = P.stream(name, n)
    with _panel_contexts("EIGMIX", s) as ctx:
        for a, rows in ctx:
            P.check_eigmix(a.eigmix(diagadj=True, packed=True), True, s, rows)
            P.check_eigmix(a.eigmix(diagadj=False, packed=True), False, s, rows)
            P.check_eigmix(a.eigmix(diagadj=False, scale=2.0, packed=True), False, s, rows, scale=2.0)
            _refuses_full_matrix(lambda: a.eigmix(packed=False))


# ---- EIGMIX panels finalised in place ------------------------------------------------------------------------------------------------

def _check_top_eigenvalues(w, info, s, diagadj, k):
    """`rtol=2e-5` and `max_rel_residual < 1e-8` (test_gpu_api_golden.test_gcta_grm_and_its_eigenvectors_from_one_accumulation)"""
    w_ref = np.linalg.eigvalsh(orc.tri_to_full(s.eigmix(diagadj), s.n))[::-1][:k]
    print("PANEL-FIGURE top-%d eigenvalues diagadj=%s: largest rel err %.3g (bound 2e-05), max_rel_residual %.3g (bound 1e-08), %d products"
          % (k, diagadj, np.max(np.abs(w - w_ref) / np.abs(w_ref)), info["max_rel_residual"], info["matmuls"]))
    np.testing.assert_allclose(w, w_ref, rtol=2e-5)
    assert info["max_rel_residual"] < 1e-8


@pytest.mark.parametrize("diagadj", [True, False])
def test_frozen_eigmix_panels(diagadj):
    """finalize_inplace + eigmix read-back + panel_entries + the Krylov solver on EIGMIX panels"""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.eigen import PanelOperator, topk_eigen
    s, n, k = P.stream("mixed", 531), 531, 8
    with _panel_contexts("EIGMIX", s) as ctx:
        for a, rows in ctx:
            before = a.eigmix(diagadj=diagadj, packed=True)
            a.finalize_inplace(diagadj=diagadj, scale=1.0)
            after = a.eigmix(diagadj=diagadj, packed=True)
            P.check_eigmix(after, diagadj, s, rows)
            # `rtol=1e-13, atol=0` (test_gpu_between_feeds.test_finalize_inplace_then_nothing_may_follow)
            P.check_close("frozen eigmix read back", after, before, s, rows, rtol=1e-13)
            P.check_close("frozen eigmix read back, scale=2", a.eigmix(diagadj=diagadj, scale=2.0, packed=True), 2.0 * before, s, rows,
                          rtol=1e-13)
            with pytest.raises(_lib.SnpGpuError, match="another 'diagadj'"):
                a.eigmix(diagadj=not diagadj, packed=True)
            # the diagonal, the first and the last row, the last column
            r0, r1 = rows
            ri = np.concatenate([np.arange(r0, r1), np.full(n - r0, r0), np.full(n - r1 + 1, r1 - 1), np.arange(r0, r1)])
            ci = np.concatenate([np.arange(r0, r1), np.arange(r0, n), np.arange(r1 - 1, n), np.full(r1 - r0, n - 1)])
            got = a.panel_entries(ri, ci)
            want = after[P.tri_idx(n, ri, ci) - P.tri_idx(n, r0, r0)]
            bad = got != want
            assert not bad.any(), "panel_entries differs from the slab at (row, column) %s" % list(zip(ri[bad][:8].tolist(), ci[bad][:8].tolist()))
        op = PanelOperator([a for a, _ in ctx], n, torch.device("cuda", 0), normalize=False)
        w, v, info = topk_eigen(op, k)
        _check_top_eigenvalues(w.cpu().numpy(), info, s, diagadj, k)


# ---- the gathers of snpgpu_multi ------------------------------------------------------------------------------------------------------

LAYOUTS = [((0, 0, 0), 1), ((0, 0), 2)]


@contextlib.contextmanager
def _multi(kind, s, devices, ppd, **kw):
    from snprelate_amd import _lib
    with _lib.MultiAccumulator(getattr(_lib, kind), s.n, devices=devices, panels_per_device=ppd, max_block_snps=P.BMAX, **kw) as m:
        for block in s.blocks():
            m.feed(block)
        m.sync()
        rows = sorted((r0, r1) for r0, r1, _ in m.panels())
        assert len(rows) >= 2 and rows[0][0] == 0 and rows[-1][1] == s.n and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
        yield m


@contextlib.contextmanager
def _panel_views(m):
    """[(Accumulator view of a resident panel's context, (row_begin, row_end))] in the object's panel order; the object owns them"""
    import ctypes
    from snprelate_amd import _lib
    views = []
    try:
        for i in range(m.info()["n_panels"]):
            h, r0, r1, d = ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
            _lib.check(_lib.lib().snpgpu_multi_panel(m._h, i, ctypes.byref(h), ctypes.byref(r0), ctypes.byref(r1), ctypes.byref(d)))
            a = _lib.Accumulator.__new__(_lib.Accumulator)
            a.kind, a.n, a._h, a.row_begin, a.row_end, a.full = m.kind, m.n, h, r0.value, r1.value, False
            views.append((a, (r0.value, r1.value)))
        yield views
    finally:
        for a, _ in views:
            a._h = None                            # nothing to destroy


def _placed_slabs(m, read, like):
    """the per-panel slabs, read through the Accumulator-level calls on the resident panels' own contexts, each at its place"""
    out = [np.full_like(x, np.nan) for x in like]
    with _panel_views(m) as views:
        for a, rows in views:
            lo, hi = P.slab_range(m.n, *rows)
            assert a.slab_size() == hi - lo
            for o, x in zip(out, read(a)):
                o[lo:hi] = x
    return out


def _whole(s):
    return (0, s.n)


@pytest.mark.parametrize("devices,ppd", LAYOUTS)
def test_multi_king_homo_gather(devices, ppd):
    s = P.stream("mixed", 531)
    with _multi("KING_HOMO", s, devices, ppd) as m:
        got = m.king_homo()
        P.check_king_homo(got, s, _whole(s))
        placed = _placed_slabs(m, lambda a: a.king_homo(packed=True), got)
        for k in range(2):
            P.check_exact("snpgpu_multi_king_homo against the placed slabs", got[k], placed[k], s, _whole(s))


@pytest.mark.parametrize("devices,ppd", LAYOUTS)
def test_multi_ibs_ave_gather(devices, ppd):
    s = P.stream("mixed", 531)
    with _multi("IBS", s, devices, ppd) as m:
        got = m.ibs_ave()
        P.check_exact("snpgpu_multi_ibs_ave", got, s.ibs_ave(), s, _whole(s))
        placed = _placed_slabs(m, lambda a: [a.ibs_ave(packed=True)], [got])
        P.check_exact("snpgpu_multi_ibs_ave against the placed slabs", got, placed[0], s, _whole(s))


@pytest.mark.parametrize("bayes", [False, True])
@pytest.mark.parametrize("devices,ppd", LAYOUTS)
def test_multi_pca_trace(devices, ppd, bayes):
    s = P.stream("mixed", 531)
    with _multi("PCA_COV", s, devices, ppd, bayesian=bayes) as m:
        got = m.pca_trace()
        P.check_trace(got, s, bayes)
        with _panel_views(m) as views:
            assert got == sum(a.pca_panel_trace() for a, _ in views)                  # the same terms in the same order
        assert got == m.pca_cov(want_matrix=False)[1]


@pytest.mark.parametrize("devices,ppd", LAYOUTS)
def test_multi_eigmix_gather_then_frozen_then_eigen(devices, ppd):
    s, k = P.stream("mixed", 531), 8
    with _multi("EIGMIX", s, devices, ppd) as m:
        for diagadj, scale in ((True, 1.0), (False, 2.0)):
            got = m.eigmix(diagadj, scale=scale)
            P.check_eigmix(got, diagadj, s, _whole(s), scale=scale)
            placed = _placed_slabs(m, lambda a: [a.eigmix(diagadj=diagadj, scale=scale, packed=True)], [got])
            P.check_exact("snpgpu_multi_eigmix against the placed slabs", got, placed[0], s, _whole(s))
        before = m.eigmix(True)
        m.finalize_inplace(True)
        after = m.eigmix(True)
        P.check_close("snpgpu_multi_eigmix after finalize_inplace", after, before, s, _whole(s), rtol=1e-13)
        w, v, info = m.topk_eigen(k, scale=1.0)
        _check_top_eigenvalues(w, info, s, True, k)
