"""The sparse GRM straight from the GPU panels: snpgpu_select_grm / snpgpu_multi_select_grm / snpgpu_gnrGRMPairs against the rule of
tests/grm_pairs_ref.py applied to the packed slab that the EXISTING finaliser returns for the same context -- the finalisers are held to
the CPU oracle by test_gpu_panel_finalisers.py / test_gpu_parity.py, so indices, order, every bit of the values, n_found and the
diagonal are compared exactly and no tolerance appears.  Inputs are tests/panel_streams.py (read-only): n = 531 cut into the panels
0 / 256 / 512 / 531, n = 513 whose last panel is one diagonal entry; the streams `mixed` and `holes`, fed in their blocks.

One comparison is not bit for bit: the three panels concatenated against the full context (_panels_against_whole).  The fp64 sums of
a panel and of the full context may differ in their last bits before any finaliser runs, so that one is held to twice the bound that
panel_streams.check_gcta / check_cov / check_eigmix hold a panel to against the oracle (rel_err < 1e-5).

Counts and margins of one run are printed as GRM-PAIRS-FIGURE lines (`pytest -s`)."""
import contextlib
import ctypes

import numpy as np
import pytest

import grm_pairs_ref as R
import panel_streams as P
from norms import tri_diag_scale

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
PANEL_BOUND = 2 * 1e-5                  # twice `check_rel(..., bound=1e-5)` of panel_streams.check_gcta / check_cov / check_eigmix

# variant: (context kind, selection kind, mode, scale)
VARIANTS = {
    "gcta": ("GRM_GCTA", "SEL_GRM_GCTA", 0, 1.0),
    "eigenstrat": ("PCA_COV", "SEL_GRM_EIGENSTRAT", 0, 1.0),
    "eigmix_d0_s1": ("EIGMIX", "SEL_GRM_EIGMIX", 0, 1.0),
    "eigmix_d0_s2": ("EIGMIX", "SEL_GRM_EIGMIX", 0, 2.0),
    "eigmix_d1_s1": ("EIGMIX", "SEL_GRM_EIGMIX", 1, 1.0),
    "eigmix_d1_s2": ("EIGMIX", "SEL_GRM_EIGMIX", 1, 2.0),
    "beta0": ("INDIV_BETA", "SEL_GRM_INDIV_BETA", 0, 1.0),
    "beta1": ("INDIV_BETA", "SEL_GRM_INDIV_BETA", 1, 1.0),
    "beta2": ("INDIV_BETA", "SEL_GRM_INDIV_BETA", 2, 1.0),
}
PANEL_VARIANTS = [v for v in VARIANTS if not v.startswith("beta")]


def _what(variant):
    from snprelate_amd import _lib
    kind, what, mode, scale = VARIANTS[variant]
    return kind, getattr(_lib, what), mode, scale


@contextlib.contextmanager
def _context(kind, n, blocks, rows=None, bmax=P.BMAX):
    from snprelate_amd import _lib
    kw = {} if rows is None or rows == (0, n) else dict(row_begin=rows[0], row_end=rows[1])
    with _lib.Accumulator(getattr(_lib, kind), n, max_block_snps=bmax, **kw) as a:
        for b in blocks:
            a.feed(b)
        yield a


def _finaliser(a, variant, trace_in=0.0):
    """the packed slab of the context's existing finaliser (and IndivBeta's average)"""
    kind, _, mode, scale = VARIANTS[variant]
    if kind == "GRM_GCTA":
        return a.grm_gcta(packed=True), 0.0
    if kind == "PCA_COV":
        return a.pca_cov(packed=True, normalize=True, trace_in=trace_in)[0], 0.0
    if kind == "EIGMIX":
        return a.eigmix(diagadj=bool(mode), scale=scale, packed=True), 0.0
    return a.indiv_beta(mode=mode, packed=True)


def _select(a, variant, cutoff, trace_in=0.0, **kw):
    _, what, mode, scale = _what(variant)
    i1, i2, v, d, avg, found = a.select_grm(what, cutoff, mode=mode, scale=scale, trace_in=trace_in, **kw)
    return dict(idx1=i1, idx2=i2, value=v, diag=d), avg, found


def _realised(slab, n):
    """an off-diagonal entry of the finaliser's own output in the upper quarter of the finite ones: `>=` must keep its pair"""
    i, j = R.slab_rc(n, 0, n)
    v = np.sort(slab[(j > i) & np.isfinite(slab)])
    return float(v[(3 * v.size) // 4])


def _floor(whole, n):
    """the floor of panel_streams.rel_err for the whole reference"""
    a = np.abs(whole[np.isfinite(whole)])
    return min(tri_diag_scale(whole, n), float(np.median(a)))


def _panels_against_whole(parts, whole, cutoff, whole_slab, n, label):
    """The three panels' results concatenated against the full context's, within PANEL_BOUND in the measure of panel_streams.rel_err
    (|a - b| / (|b| + floor), floor from the full context's finaliser output): with a non-finite cutoff the same pairs in the same
    order; with a finite one every pair found on one side only lies within the bound of the cutoff; the values of the common pairs
    agree within the bound.  -> the largest figure / bound seen.
    One run (mixed and holes, n = 531, GCTA, Eigenstrat and the four EIGMIX forms, six cutoffs each): the largest figure was
    0.18 of the bound (the values of common pairs, EIGMIX on `holes`; GCTA and Eigenstrat below 2e-10 of it)."""
    floor = _floor(whole_slab, n)
    key = lambda t: t["idx1"].astype(np.int64) * (1 << 20) + t["idx2"]            # noqa: E731
    kp, kw = key(parts), key(whole)
    assert (np.diff(kp) > 0).all() and (np.diff(kw) > 0).all(), "%s: order" % label
    fig = 0.0
    if not np.isfinite(cutoff):
        assert np.array_equal(kp, kw), "%s: other pairs with a non-finite cutoff" % label
        both_p = both_w = np.ones(kp.size, bool)
    else:
        only_p, only_w = ~np.isin(kp, kw), ~np.isin(kw, kp)
        for t, only in ((parts, only_p), (whole, only_w)):
            d = np.abs(t["value"][only] - cutoff) / (abs(cutoff) + floor)
            if d.size:
                fig = max(fig, float(d.max()) / PANEL_BOUND)
            assert (d < PANEL_BOUND).all(), "%s: a pair far from the cutoff is on one side only" % label
        both_p, both_w = ~only_p, ~only_w
    a, b = parts["value"][both_p], whole["value"][both_w]
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), "%s: NaN / Inf placement" % label
    e = np.abs(a[fin] - b[fin]) / (np.abs(b[fin]) + floor)
    if e.size:
        fig = max(fig, float(e.max()) / PANEL_BOUND)
    assert (e < PANEL_BOUND).all(), "%s: values of common pairs differ by %.3g of the bound" % (label, float(e.max()) / PANEL_BOUND)
    return fig


# ---- 1, 6: every kind x the full context and each panel x the cutoffs; the panels against the whole ------------------------------------

@pytest.mark.parametrize("name", ["mixed", "holes"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_kind_panel_and_cutoff(variant, name):
    """Margin of the panels against the whole observed in one run: the largest figure over all kinds, streams and cutoffs was
    0.18 of the bound (2e-5 in the measure of panel_streams.rel_err): the values of common pairs of EIGMIX on `holes`; GCTA and
    Eigenstrat stayed below 2e-10 of it, and no pair was on one side only.  See _panels_against_whole."""
    n = 531
    s = P.stream(name, n)
    kind = VARIANTS[variant][0]
    contexts = [(0, n)] + (P.panels(n) if variant in PANEL_VARIANTS else [])
    failed = []
    with contextlib.ExitStack() as st:
        ctx = [(st.enter_context(_context(kind, n, s.blocks(), rows)), rows) for rows in contexts]
        trace = ctx[0][0].pca_cov(want_matrix=False)[1] if kind == "PCA_COV" else 0.0
        tin = lambda rows: 0.0 if rows == (0, n) else trace                        # noqa: E731
        slabs = [_finaliser(a, variant, tin(rows)) for a, rows in ctx]
        full_slab = slabs[0][0]
        cutoffs = [NAN, INF, 0.0, 0.05]
        if np.isfinite(full_slab).any():        # (IndivBeta modes 0 / 1 on `holes`: the never-called sample makes the average, so every entry, NaN)
            cutoffs += [_realised(full_slab, n), float(np.max(full_slab[np.isfinite(full_slab)])) + 1.0]
        for cutoff in cutoffs:
            got = []
            for (a, rows), (slab, avg_ref) in zip(ctx, slabs):
                t, avg, found = _select(a, variant, cutoff, tin(rows))
                ref = R.selection(slab, n, rows, cutoff)
                print("GRM-PAIRS-FIGURE %-12s %-5s rows %3d..%3d cutoff %-10.4g: %d pairs" % (variant, name, rows[0], rows[1], cutoff, found))
                try:
                    assert found == ref["idx1"].size == t["idx1"].size, "n_found %d, %d stored, the reference has %d" % (found, t["idx1"].size, ref["idx1"].size)
                    msg = R.same_selection(t, ref)
                    assert msg is None, msg
                    assert t["diag"].size == min(rows[1], n) - rows[0]
                    assert R.same_bits([avg], [avg_ref]), "avg_val %r against %r" % (avg, avg_ref)
                except AssertionError as e:
                    failed.append("rows %d..%d cutoff %r: %s" % (rows[0], rows[1], cutoff, e))
                got.append(t)
            n_pairs = n * (n - 1) // 2
            if not np.isfinite(cutoff):
                assert got[0]["idx1"].size == n_pairs                            # every pair, NaN pairs included
            elif len(cutoffs) > 4 and cutoff == cutoffs[5]:                      # above every finite value
                assert not np.isfinite(got[0]["value"]).any()
            else:
                assert not np.isnan(got[0]["value"]).any() and (got[0]["value"] >= cutoff).all()
                if kind != "INDIV_BETA" and cutoff == 0.0:                       # (mode 2 has no negative entry, modes 0 / 1 may have no number)
                    assert 0 < got[0]["idx1"].size < n_pairs
            if len(cutoffs) > 4 and cutoff == cutoffs[4]:
                assert (got[0]["value"] == cutoff).any(), "the pair whose value is the cutoff was dropped"
            if len(got) > 1:
                parts = {k: np.concatenate([t[k] for t in got[1:]]) for k in got[0]}
                try:
                    fig = _panels_against_whole(parts, got[0], cutoff, full_slab, n, "cutoff %r" % cutoff)
                    print("GRM-PAIRS-FIGURE %-12s %-5s cutoff %-10.4g: panels against the whole, margin %.3g of the bound" % (variant, name, cutoff, fig))
                    assert R.same_bits(parts["diag"], got[0]["diag"]) or P.rel_err(parts["diag"], got[0]["diag"], full_slab).max() < PANEL_BOUND
                except AssertionError as e:
                    failed.append("cutoff %r: %s" % (cutoff, e))
        if name == "holes" and kind == "GRM_GCTA":                               # the never-called sample: no number in its row and column
            t, _, _ = _select(ctx[0][0], variant, NAN)
            bad = (t["idx1"] == P.NEVER_CALLED) | (t["idx2"] == P.NEVER_CALLED)
            assert not np.isfinite(t["value"][bad]).any() and not np.isfinite(t["diag"][P.NEVER_CALLED])
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("variant", ["gcta", "eigenstrat", "eigmix_d1_s2"])
def test_one_entry_panel_has_no_pair_and_one_diagonal_value(variant):
    """n = 513: the last panel is the diagonal entry (512, 512) alone"""
    n = 513
    s = P.stream("mixed", n)
    kind = VARIANTS[variant][0]
    with _context(kind, n, s.blocks()) as full, _context(kind, n, s.blocks(), (512, 513)) as a:
        trace = full.pca_cov(want_matrix=False)[1] if kind == "PCA_COV" else 0.0
        slab, _ = _finaliser(a, variant, trace)
        assert slab.shape == (1,)
        for cutoff in (NAN, -INF, -1e9):
            t, _, found = _select(a, variant, cutoff, trace)
            assert found == 0 and t["idx1"].size == 0 and R.same_bits(t["diag"], slab), (cutoff, t)
        parts = []
        for rows in P.panels(n):
            with _context(kind, n, s.blocks(), rows) as p:
                t, _, _ = _select(p, variant, 0.0, trace)
                msg = R.same_selection(t, R.selection(_finaliser(p, variant, trace)[0], n, rows, 0.0))
                assert msg is None, msg
                parts.append(t)
        assert sum(t["diag"].size for t in parts) == n and sum(t["idx1"].size for t in parts) > 1000


def test_eigenstrat_panel_needs_trace_in_and_kinds_must_match():
    from snprelate_amd import _lib
    n = 531
    s = P.stream("mixed", n)
    with _context("PCA_COV", n, s.blocks(), (256, 512)) as a:
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pca_cov: normalisation of a panel needs trace_in"):
            a.select_grm(_lib.SEL_GRM_EIGENSTRAT, 0.05)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_select_grm: 'what' does not match the context kind"):
            a.select_grm(_lib.SEL_GRM_GCTA, 0.05)
    with _context("INDIV_BETA", n, s.blocks(), (256, 512)) as a:
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_indiv_beta: needs a full"):
            a.select_grm(_lib.SEL_GRM_INDIV_BETA, 0.05, mode=2)


# ---- 2: capacity -------------------------------------------------------------------------------------------------------------------------

def _raw(a, variant, cutoff, capacity, size, trace_in=0.0, outputs=True):
    """snpgpu_select_grm with outputs of `size` elements filled with a pattern; -> (idx1, idx2, value, diag, n_found)"""
    from snprelate_amd import _lib
    _, what, mode, scale = _what(variant)
    o = _lib.GrmSelOpts(what, mode, scale, trace_in, cutoff, None)
    out = [np.full(size, -9, np.int32), np.full(size, -9, np.int32), np.full(size, -9.0)]
    diag = np.full(a.n + 8, -9.0)
    found = ctypes.c_int64(-1)
    ptrs = [_lib._ptr(x) if outputs else None for x in out]
    _lib.check(_lib.lib().snpgpu_select_grm(a._h, ctypes.byref(o), capacity, *ptrs, _lib._ptr(diag), None, ctypes.byref(found)))
    return out[0], out[1], out[2], diag, found.value


@pytest.mark.parametrize("variant,rows", [("gcta", (256, 512)), ("eigmix_d1_s2", (0, 531)), ("beta2", (0, 531))])
def test_capacity_keeps_the_prefix_and_the_fill_pattern(variant, rows):
    n = 531
    s = P.stream("mixed", n)
    with _context(VARIANTS[variant][0], n, s.blocks(), rows) as a:
        whole, _, total = _select(a, variant, 0.0)
        assert total > 300
        n_diag = min(rows[1], n) - rows[0]
        for cap in (total - 1, 1, total + 50):
            i1, i2, v, d, found = _raw(a, variant, 0.0, cap, total + 64)
            keep = min(cap, total)
            assert found == total
            assert np.array_equal(i1[:keep], whole["idx1"][:keep]) and np.array_equal(i2[:keep], whole["idx2"][:keep])
            assert R.same_bits(v[:keep], whole["value"][:keep])
            assert (i1[keep:] == -9).all() and (i2[keep:] == -9).all() and (v[keep:] == -9).all(), "written behind the capacity %d" % cap
            assert R.same_bits(d[:n_diag], whole["diag"]) and (d[n_diag:] == -9).all()
        i1, i2, v, d, found = _raw(a, variant, 0.0, 0, 16, outputs=False)      # count only; the diagonal does not depend on it
        assert found == total and (i1 == -9).all() and (v == -9).all() and R.same_bits(d[:n_diag], whole["diag"])
        t0, _, f0 = _select(a, variant, 0.0, capacity=0)
        assert f0 == total and t0["idx1"].size == 0 and R.same_bits(t0["diag"], whole["diag"])
        again, _, _ = _select(a, variant, 0.0)                                  # the same call gives the same arrays
        assert all(again[k].tobytes() == whole[k].tobytes() for k in whole)


# ---- 3: the sample mask --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["gcta", "eigmix_d0_s2"])
def test_sample_mask_inside_and_at_the_edges_of_a_chunk(variant):
    n = 531
    s = P.stream("holes", n)
    mask = np.ones(n, bool)
    mask[[0, 1, 63, 64, 100, 127, 128, 191, 192, 255, 256, 257, 300, 319, 320, 383, 384, 400, 511, 512, 513, 530]] = False
    for rows in [(0, n)] + P.panels(n):
        with _context(VARIANTS[variant][0], n, s.blocks(), rows) as a:
            slab, _ = _finaliser(a, variant)
            plain, _, _ = _select(a, variant, NAN)
            for cutoff in (NAN, 0.0):
                t, _, found = _select(a, variant, cutoff, samp_sel=mask)
                ref = R.selection(slab, n, rows, cutoff, mask)
                assert found == ref["idx1"].size and found > 0
                msg = R.same_selection(t, ref)
                assert msg is None, "rows %d..%d cutoff %r with a mask: %s" % (rows[0], rows[1], cutoff, msg)
                assert mask[t["idx1"]].all() and mask[t["idx2"]].all()
                assert R.same_bits(t["diag"], plain["diag"]), "the mask changed diag"
                t8, _, _ = _select(a, variant, cutoff, samp_sel=mask.astype(np.uint8) * 7)       # nonzero = selected
                assert R.same_selection(t8, t) is None


# ---- 4: between feeds ----------------------------------------------------------------------------------------------------------------------

def _twin_blocks(s, monkeypatch):
    """Two contexts fed the same blocks hold the same bits only where every panel entry is one sequence of additions in stream order
    (test_gpu_between_feeds.test_reads_leave_gcta_bit_identical): whole tiles (no split along K) and no SNP of at most 128 copies of
    the minor allele (the fp64 atomics of the sparse kernels, whose order changes from run to run).  The blocks of the stream without
    those SNPs, block boundaries kept."""
    monkeypatch.setenv("SNPGPU_I8_TAIL_PARTS", "1")
    called = s.g < 3
    t = np.where(called, s.g, 0).sum(1, dtype=np.int64)
    keep = np.minimum(t, 2 * called.sum(1, dtype=np.int64) - t) > 128
    blocks = [np.ascontiguousarray(s.g[a:b][keep[a:b]]) for a, b in zip(s.cuts[:-1], s.cuts[1:])]
    assert keep.mean() > 0.7 and all(len(x) for x in blocks)
    return blocks


@pytest.mark.parametrize("rows", [(0, 531), (256, 512)])
def test_gcta_selection_between_feeds(rows, monkeypatch):
    """GCTA keeps pending column / row terms and folds them on the fly: a selection does not settle them, further blocks follow.  Every
    selection equals the finaliser's slab at that moment (the stream's own blocks); the final one equals that of a context fed in one
    go by the same blocks (the blocks of _twin_blocks)."""
    n = 531
    s = P.stream("mixed", n)
    for blocks, twin in ((s.blocks(), False), (_twin_blocks(s, monkeypatch), True)):
        with _context("GRM_GCTA", n, blocks[:2], rows) as a, _context("GRM_GCTA", n, blocks, rows) as one_go:
            for cutoff in (NAN, 0.0):
                t, _, _ = _select(a, "gcta", cutoff)
                msg = R.same_selection(t, R.selection(a.grm_gcta(packed=True), n, rows, cutoff))
                assert msg is None, "after two blocks, cutoff %r: %s" % (cutoff, msg)
            for b in blocks[2:]:
                a.feed(b)
            for cutoff in (NAN, 0.0, 0.05):
                t, _, found = _select(a, "gcta", cutoff)
                msg = R.same_selection(t, R.selection(a.grm_gcta(packed=True), n, rows, cutoff))
                assert msg is None, "after all blocks, cutoff %r: %s" % (cutoff, msg)
                assert found > 0
                if twin:
                    msg = R.same_selection(t, _select(one_go, "gcta", cutoff)[0])
                    assert msg is None, "against a context that saw no selection between its feeds, cutoff %r: %s" % (cutoff, msg)


# ---- 5: frozen contexts --------------------------------------------------------------------------------------------------------------------

FROZEN = [("GRM_GCTA", 1, 1.0, ("gcta",)), ("EIGMIX", 1, 1.0, ("eigmix_d1_s1", "eigmix_d1_s2")), ("EIGMIX", 0, 2.0, ("eigmix_d0_s2",))]


@pytest.mark.parametrize("rows", [(0, 531), (256, 512)])
def test_frozen_contexts_select_what_their_twins_select(rows, monkeypatch):
    """After snpgpu_finalize_inplace the selection equals, bit for bit, that of an unfrozen context with the same sums: the same
    context before it was frozen (every kind, the stream's own blocks) and, for GCTA, a second context fed the blocks of _twin_blocks.
    Two EIGMIX contexts fed the same blocks differ in the last bit of their sums even on those blocks (one run: -0.016537551172191977
    against -0.016537551172191974 at the first pair, both contexts unfrozen or not), so there the context itself is the twin.
    EIGMIX with the other diagadj is refused."""
    from snprelate_amd import _lib
    n = 531
    s = P.stream("mixed", n)
    cutoffs = (NAN, 0.0, 0.05)
    for kind, diagadj, frozen_scale, variants in FROZEN:
        with _context(kind, n, s.blocks(), rows) as a:
            before = {(v, c): _select(a, v, c)[0] for v in variants for c in cutoffs}
            a.finalize_inplace(diagadj=bool(diagadj), scale=frozen_scale)
            for (v, c), ref in before.items():
                t, _, _ = _select(a, v, c)
                msg = R.same_selection(t, ref)
                assert msg is None, "%s cutoff %r against the same context before it was frozen: %s" % (v, c, msg)
                if kind == "GRM_GCTA":
                    msg = R.same_selection(t, R.selection(a.grm_gcta(packed=True), n, rows, c))
                    assert msg is None, "%s cutoff %r against the frozen context's finaliser: %s" % (v, c, msg)
            if kind == "EIGMIX":
                with pytest.raises(_lib.SnpGpuError, match="snpgpu_select_grm: the context was finalised in place with another 'diagadj'"):
                    a.select_grm(_lib.SEL_GRM_EIGMIX, 0.05, mode=1 - diagadj, scale=1.0)
    blocks = _twin_blocks(s, monkeypatch)
    for kind, diagadj, frozen_scale, variants in FROZEN[:1]:
        with _context(kind, n, blocks, rows) as a, _context(kind, n, blocks, rows) as twin:
            a.finalize_inplace(diagadj=bool(diagadj), scale=frozen_scale)
            for v in variants:
                for c in cutoffs:
                    msg = R.same_selection(_select(a, v, c)[0], _select(twin, v, c)[0])
                    assert msg is None, "%s cutoff %r against an unfrozen twin: %s" % (v, c, msg)


# ---- 7: a multi-device object on listed copies of one device -----------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["gcta", "eigenstrat", "eigmix_d1_s2"])
def test_multi_device_object_concatenates_its_panels(variant, monkeypatch):
    """The object's panels against single contexts of the same rows, fed the same blocks: exact on the blocks of _twin_blocks for GCTA
    and Eigenstrat.  Two accumulations of the EIGMIX sums differ in their last bits even on those blocks (see
    test_frozen_contexts_select_what_their_twins_select), so EIGMIX is held to the bound of the panels against the whole, and its
    capacity prefixes and the passes' diag rows to the object's own full result."""
    from snprelate_amd import _lib
    n = 531
    s = P.stream("mixed", n)
    kind, what, mode, scale = _what(variant)
    blocks = _twin_blocks(s, monkeypatch)
    with _lib.MultiAccumulator(getattr(_lib, kind), n, devices=(0, 0, 0), panels_per_device=1, max_block_snps=P.BMAX) as m:
        for b in blocks:
            m.feed(b)
        panels = sorted((r0, r1) for r0, r1, _ in m.panels())
        assert len(panels) > 1 and panels[0][0] == 0 and panels[-1][1] >= n
        trace = m.pca_trace() if kind == "PCA_COV" else 0.0
        with _context(kind, n, blocks) as whole:
            whole_slab = _finaliser(whole, variant)[0]
        for cutoff in (NAN, 0.05):
            parts = []
            for rows in panels:
                with _context(kind, n, blocks, (rows[0], min(rows[1], n))) as p:
                    parts.append(_select(p, variant, cutoff, trace)[0])
            ref = {k: np.concatenate([t[k] for t in parts]) for k in parts[0]}
            total = ref["idx1"].size
            assert total > 0
            if kind == "EIGMIX":               # two accumulations of the EIGMIX sums differ in their last bits: the bound of test 6
                i1, i2, v, d, found = m.select_grm(what, cutoff, mode=mode, scale=scale)
                got = dict(idx1=i1, idx2=i2, value=v, diag=d)
                fig = _panels_against_whole(got, ref, cutoff, whole_slab, n, "multi-device object, cutoff %r" % cutoff)
                print("GRM-PAIRS-FIGURE multi %-12s cutoff %-6.4g: margin %.3g of the bound" % (variant, cutoff, fig))
                assert P.rel_err(d, ref["diag"], whole_slab).max() < PANEL_BOUND
                ref, total = got, found                                          # ... and the object's own prefixes below
            for cap in (None, total // 2, 0):
                i1, i2, v, d, found = m.select_grm(what, cutoff, mode=mode, scale=scale, capacity=cap)
                keep = total if cap is None else cap
                assert found == total and i1.size == keep
                assert np.array_equal(i1, ref["idx1"][:keep]) and np.array_equal(i2, ref["idx2"][:keep]) and R.same_bits(v, ref["value"][:keep])
                assert d.shape == (n,) and R.same_bits(d, ref["diag"]), "diag of the multi-device object"
    # a pass of a two-pass object: its own panels' pairs, the other rows of diag untouched
    seen_rows, seen_pairs, untouched = np.zeros(n, int), 0, 0
    for k in range(2):
        with _lib.MultiAccumulator(getattr(_lib, kind), n, devices=(0, 0), panels_per_device=1, n_passes=2, pass_index=k, max_block_snps=P.BMAX) as m:
            for b in blocks:
                m.feed(b)
            own = np.zeros(n, bool)
            empty = dict(idx1=np.zeros(0, np.int32), idx2=np.zeros(0, np.int32), value=np.zeros(0), diag=np.zeros(0))
            parts = [empty]                                                        # (a pass may own no panel when n is small against the plan)
            for r0, r1, _ in sorted(m.panels()):
                own[r0:min(r1, n)] = True
                with _context(kind, n, blocks, (r0, min(r1, n))) as p:
                    parts.append(_select(p, variant, NAN, trace)[0])
            untouched += int((~own).sum())
            ref = {k_: np.concatenate([t[k_] for t in parts]) for k_ in empty}
            i1, i2, v, d, found = m.select_grm(what, NAN, mode=mode, scale=scale, trace_in=trace, diag_fill=-9.0)
            assert found == ref["idx1"].size and np.array_equal(i1, ref["idx1"]) and np.array_equal(i2, ref["idx2"])
            assert own[i1].all() and (d[~own] == -9.0).all(), "diag rows of the other pass were written"
            if kind == "EIGMIX":
                assert (P.rel_err(v, ref["value"], whole_slab) < PANEL_BOUND).all() and (P.rel_err(d[own], ref["diag"], whole_slab) < PANEL_BOUND).all()
            else:
                assert R.same_bits(v, ref["value"]) and R.same_bits(d[own], ref["diag"])
            seen_rows += own
            seen_pairs += found
    assert (seen_rows == 1).all() and seen_pairs == n * (n - 1) // 2 and untouched == n      # (every row was another pass's once)


def test_multi_device_object_refuses_indiv_beta():
    from snprelate_amd import _lib
    n = 531
    with _lib.MultiAccumulator(_lib.GRM_GCTA, n, devices=(0, 0), panels_per_device=1, max_block_snps=P.BMAX) as m:
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_multi_select_grm: INDIV_BETA needs a full context"):
            m.select_grm(_lib.SEL_GRM_INDIV_BETA, 0.05, mode=2)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_multi_select_grm: 'what' does not match the object's kind"):
            m.select_grm(_lib.SEL_GRM_EIGMIX, 0.05, mode=0, scale=2.0)


# ---- 8: the working space and the Python API on the HapMap golden file -------------------------------------------------------------------

@pytest.mark.parametrize("method", ["GCTA", "Eigenstrat", "EIGMIX", "IndivBeta"])
def test_api_pairs_against_the_matrix_of_snpgdsGRM(hapmap, method, tmp_path):
    from snprelate_amd import api
    n = hapmap.n_samp
    full = api.snpgdsGRM(hapmap, method=method, useMatrix=True, verbose=False)
    slab = full["grm"]
    floor = _floor(slab, n)
    for cutoff in (0.05, NAN):
        got = api.snpgdsGRMPairs(hapmap, method=method, cutoff=cutoff, verbose=False)
        ref = R.selection(slab, n, (0, n), cutoff)
        assert got["method"] == method and got["n_pairs"] == got["idx1"].size == got["value"].size
        assert np.array_equal(got["sample_id"], full["sample_id"]) and np.array_equal(got["snp_id"], full["snp_id"])
        assert np.array_equal(got["ID1"], full["sample_id"][got["idx1"]]) and np.array_equal(got["ID2"], full["sample_id"][got["idx2"]])
        assert P.rel_err(got["diag"], ref["diag"], slab).max() < PANEL_BOUND
        t = dict(idx1=got["idx1"], idx2=got["idx2"], value=got["value"], diag=got["diag"])
        fig = _panels_against_whole(t, ref, cutoff, slab, n, "%s cutoff %r" % (method, cutoff))
        print("GRM-PAIRS-FIGURE api %-10s cutoff %-6.4g: %d pairs, margin %.3g of the bound (floor %.3g)" % (method, cutoff, got["n_pairs"], fig, floor))
        assert got["n_pairs"] > 0
        if method == "IndivBeta":
            assert got["avg_val"] == full["avg_val"]
        else:
            assert "avg_val" not in got
    # the text files give the returned arrays back bit for bit
    prefix = str(tmp_path / "sparse")
    got = api.snpgdsGRMPairs(hapmap, method=method, cutoff=0.05, out_fn=prefix, verbose=False)
    ids, row, col, val = R.read_sparse_grm(prefix)
    assert list(ids) == [str(x) for x in got["sample_id"]]
    off = row != col
    order = np.lexsort((got["idx1"], got["idx2"]))                                # the file is sorted by row = idx2, then col = idx1
    assert np.array_equal(row[off], got["idx2"][order]) and np.array_equal(col[off], got["idx1"][order])
    assert R.same_bits(val[off], got["value"][order])
    assert np.array_equal(row[~off], np.arange(n)) and R.same_bits(val[~off], got["diag"])


def test_api_weighted_is_eigmix_and_samp_sel_restricts_the_pairs(hapmap, tmp_path):
    """Each call accumulates the EIGMIX sums anew, and two accumulations differ in their last bits (see
    test_frozen_contexts_select_what_their_twins_select), so calls are compared within the bound of the panels against the whole;
    what one call returns and what it writes are compared exactly."""
    from snprelate_amd import api
    n = hapmap.n_samp
    slab = api.snpgdsGRM(hapmap, method="EIGMIX", useMatrix=True, with_id=False, verbose=False)
    a = api.snpgdsGRMPairs(hapmap, method="EIGMIX", cutoff=0.05, verbose=False)
    b = api.snpgdsGRMPairs(hapmap, method="Weighted", cutoff=0.05, verbose=False)
    table = lambda r: {k: r[k] for k in ("idx1", "idx2", "value", "diag")}        # noqa: E731
    assert b["method"] == "EIGMIX"
    fig = _panels_against_whole(table(b), table(a), 0.05, slab, n, "Weighted against EIGMIX")
    assert P.rel_err(b["diag"], a["diag"], slab).max() < PANEL_BOUND
    mask = np.random.default_rng(5).random(n) < 0.6
    prefix = str(tmp_path / "masked")
    c = api.snpgdsGRMPairs(hapmap, method="EIGMIX", cutoff=0.05, samp_sel=mask, out_fn=prefix, verbose=False)
    keep = mask[a["idx1"]] & mask[a["idx2"]]
    assert mask[c["idx1"]].all() and mask[c["idx2"]].all() and 0 < c["n_pairs"] < a["n_pairs"]
    fig = max(fig, _panels_against_whole(table(c), {k: (v if k == "diag" else v[keep]) for k, v in table(a).items()}, 0.05, slab, n, "with samp_sel"))
    assert P.rel_err(c["diag"], a["diag"], slab).max() < PANEL_BOUND             # (diag is not restricted by samp_sel)
    print("GRM-PAIRS-FIGURE api Weighted / samp_sel against EIGMIX: margin %.3g of the bound" % fig)
    d = api.snpgdsGRMPairs(hapmap, method="EIGMIX", cutoff=0.05, samp_sel=np.flatnonzero(mask), with_id=False, verbose=False)
    assert d["idx1"].size > 0 and mask[d["idx1"]].all() and mask[d["idx2"]].all() and "ID1" not in d and "sample_id" not in d
    ids, row, col, val = R.read_sparse_grm(prefix)
    assert list(ids) == [str(x) for x in np.asarray(c["sample_id"])[mask]]
    new = np.cumsum(mask) - 1
    off = row != col
    order = np.lexsort((c["idx1"], c["idx2"]))
    assert np.array_equal(row[off], new[c["idx2"][order]]) and np.array_equal(col[off], new[c["idx1"][order]])
    assert R.same_bits(val[off], c["value"][order]) and R.same_bits(val[~off], c["diag"][mask])
    with pytest.raises(ValueError, match="strictly increasing"):
        api.snpgdsGRMPairs(hapmap, samp_sel=np.array([5, 3, 9]), verbose=False)
