"""Every input form of a feed block (tests/input_forms.py) on every streaming context: the eight accumulator kinds, LDMatrix,
Projector and MultiAccumulator must give the oracle's result whether one canonical matrix arrives as clean U8 rows, as U8 rows
whose missing cells hold any byte of 3 .. 255, or as 2-bit rows with random bits in the unused codes of the last byte -- from
host memory, from device memory at odd byte offsets, through two page-locked buffers, or with the caller's own per-SNP
statistics (snpgpu_block_stats + snpgpu_feed_stats).  What is under test is the pre-pass of kernels_prep.hip
(repack_stats_kernel, repack_kernel) and kernels_transpose.hip (transpose2_direct_kernel) and its routing in ctx_feed.hip's stage_block.

Data: 700 SNPs fed as ragged blocks of 256, 300 and 144 with max_block_snps = 512; 4 % missing calls except in the middle block,
which has none, so a context alternates between its two kernel routes while the padding stays dirty.  Sample counts: 61 .. 64
(one-pass pre-pass of the counters with 13, 14, 15, 16 samples in the last dword), 65 (two-kernel form, odd row stride), 1037
(one-pass, a partial second 1024-sample workgroup), 1040 (one-pass, whole dwords), 1041 (two-kernel form, n % 4 = 1).

Which of the pre-pass's masks these tests can see (each was disabled in turn and this file run once; the commit that added
the file lists the outcome per test):
  * the clamp of U8 bytes above 3 in repack_stats_kernel's 16-sample path decides sum / num, the missing-call flag and the codes
    of real samples: every test that feeds U8 rows depends on it;
  * the padding mask of repack_stats_kernel's 2-bit path (rem < 4) decides sum / num and the flag wherever a row has padding
    (n % 4 != 0): the statistics forms and every floating-point result depend on it.  The counters of the integer kinds do not
    (a pair counter depends on its two samples alone); there it is the statistics form that notices;
  * the padding masks of transpose2_direct_kernel (rem < 16) and of repack_kernel (rem < 4) only decide which code a sample
    >= n_samp has inside the context's own buffers: the statistics and the missing-call flag of those two paths come from
    elsewhere (the flag is masked separately, the statistics are the caller's), and no result of the C ABI reads such a column.
    Without them every test here still passes: a test of results cannot tell whether they are there."""
import numpy as np
import pytest

import diss_ref
import input_forms as F
import ld_ref
import oracle as orc
from oracle.synth import synth_geno

pytestmark = pytest.mark.gpu

CUTS = [0, 256, 556, 700]
L = CUTS[-1]
MAXB = 512
NS_INT = [61, 62, 63, 64, 65, 1037, 1040, 1041]
NS_FP = [63, 65, 1037]
_CACHE = {}


def _geno(n, special=True):
    """the canonical matrix of n samples (cached; nobody writes to it)"""
    key = ("g", n, special)
    if key not in _CACHE:
        g = synth_geno(n, L, missing=0.04, seed=1000 + n, special=special)
        mid = g[CUTS[1]:CUTS[2]]
        mid[mid > 2] = (np.arange((mid > 2).sum()) % 3).astype(np.uint8)       # the middle block: no missing call at all
        assert (g[:CUTS[1]] > 2).any() and not (mid > 2).any() and (g[CUTS[2]:] > 2).any()
        assert (g[:, n - 1] > 2).any()                                         # a missing call in the last sample of a row
        g.setflags(write=False)
        _CACHE[key] = g
    return _CACHE[key]


def _forms(n, special=True, **kw):
    key = ("f", n, special, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = F.forms(_geno(n, special), CUTS, **kw)
    return _CACHE[key]


def _ref(name, n, fn, special=True):
    """fn(g) once per (name, n): the references are shared between the tests and left unchanged"""
    key = ("r", name, n, special)
    if key not in _CACHE:
        _CACHE[key] = fn(_geno(n, special))
    return _CACHE[key]


def _takes_one_pass(form, n):
    """stage_block: the counters' one-pass pre-pass reads 2-bit rows of whole dwords at a 4-byte aligned address"""
    return form.fmt == F.GENO_PACKED2 and ((n + 3) // 4) % 4 == 0 and form.offset % 4 == 0 and form.mem != "stats"


def _check_stats(form, st, n, special=True):
    """sum / num of snpgpu_block_stats, bit for bit against numpy on the canonical matrix"""
    if form.mem != "stats":
        assert st is None
        return
    s, c = F.snp_stats(_geno(n, special))
    assert st[0].dtype == np.int32 and np.array_equal(st[0], s), form.name
    assert st[1].dtype == np.int32 and np.array_equal(st[1], c), form.name


def _set_backend(monkeypatch, backend):
    monkeypatch.setenv("SNPGPU_PAIR_BACKEND", backend)          # as tests/test_gpu_parity.py's pair_backend fixture sets it


def _routes(form):
    """a 2-bit form runs with the default route and with SNPGPU_PREP_TWO_PASS=1.  The variable changes the path only where
    _takes_one_pass holds for an IBS / KING-robust context on the mfma_i8 counters (ctx_feed.hip, stage_block); everywhere else the
    second run repeats the first one's path"""
    return (False, True) if form.fmt == F.GENO_PACKED2 else (False,)


def _run_counter(kind, n, form, monkeypatch, two_pass, result, **kw):
    from snprelate_amd import _lib
    if two_pass:
        monkeypatch.setenv("SNPGPU_PREP_TWO_PASS", "1")
    else:
        monkeypatch.delenv("SNPGPU_PREP_TWO_PASS", raising=False)
    with _lib.Accumulator(kind, n, max_block_snps=MAXB, **kw) as a:
        st = F.feed(a, form)
        _check_stats(form, st, n)
        return result(a)


# ---- integer kinds: bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["mfma_i8", "popcount"])
@pytest.mark.parametrize("n", NS_INT)
def test_ibs_counts_every_form(n, backend, monkeypatch):
    from snprelate_amd import _lib
    _set_backend(monkeypatch, backend)
    ref = _ref("ibs", n, orc.ibs_count)
    one_pass = 0
    for form in _forms(n):
        for two_pass in _routes(form):
            got = _run_counter(_lib.IBS, n, form, monkeypatch, two_pass, lambda a: np.stack(a.ibs_num(packed=True), 1).astype(np.uint32))
            assert np.array_equal(got, ref), (form.name, two_pass)
            one_pass += backend == "mfma_i8" and not two_pass and _takes_one_pass(form, n)
    assert one_pass == (3 if backend == "mfma_i8" and n in (61, 62, 63, 64, 1037, 1040) else 0)      # host, device + 0, pinned


@pytest.mark.parametrize("backend", ["mfma_i8", "popcount"])
@pytest.mark.parametrize("n", NS_INT)
def test_king_robust_counts_every_form(n, backend, monkeypatch):
    from snprelate_amd import _lib
    _set_backend(monkeypatch, backend)
    ref = _ref("king", n, orc.king_robust_count)
    for form in _forms(n):
        for two_pass in _routes(form):
            got = _run_counter(_lib.KING_ROBUST, n, form, monkeypatch, two_pass, lambda a: a.king_robust_counts())
            assert np.array_equal(got, ref), (form.name, two_pass)


@pytest.mark.parametrize("n", NS_INT)
def test_diss_sum_geno_every_form(n, monkeypatch):
    """the integer plane of diss_sums against tests/diss_ref.py, as tests/test_gpu_diss.py::test_sum_geno_bit_exact compares it.
    (The dissimilarity kind has the MX-fp4 counters only -- snpgpu_create refuses it under SNPGPU_PAIR_BACKEND=popcount -- and
    always takes the two-kernel pre-pass: its runs with SNPGPU_PREP_TWO_PASS=1 repeat the path of the default ones.)"""
    from snprelate_amd import _lib
    _set_backend(monkeypatch, "mfma_i8")
    ref = _ref("diss", n, lambda g: diss_ref.packed_upper(diss_ref.diss_sums(g)[0]))
    for form in _forms(n):
        for two_pass in _routes(form):
            got = _run_counter(_lib.DISS, n, form, monkeypatch, two_pass, lambda a: a.diss_sums()[0])
            assert np.array_equal(got.astype(np.int64), ref), (form.name, two_pass)


# ---- floating-point kinds: the oracle functions and tolerances of tests/test_gpu_parity.py ----------------------------------------
def _rel_err(got, ref):
    """tests/test_gpu_parity.py:189-197 (_rel_err): the larger of the contract figure and the off-diagonal-floor figure"""
    from norms import error_figures, tri_diag_scale
    n = int((np.sqrt(8 * ref.size + 1) - 1) / 2 + 0.5)
    f = error_figures(got, ref, tri_diag_scale(ref, n))
    return max(f["contract"], f["offdiag"])


def _report(kind, n, results):
    """the largest difference between any form and u8_clean (these kernels add with fp64 atomics: no bit-identity is asserted)"""
    base = results["u8_clean"]
    worst, who = 0.0, "-"
    for name, r in results.items():
        for x, y in zip(r, base):
            fin = np.isfinite(y)
            d = float(np.max(np.abs(np.asarray(x)[fin] - np.asarray(y)[fin]))) if fin.any() else 0.0
            if d > worst:
                worst, who = d, name
    scale = max(float(np.nanmax(np.abs(np.asarray(y)[np.isfinite(y)]))) for y in base)
    print("input forms %-14s n = %4d: largest |form - u8_clean| = %.3e (%.3e of the largest entry; %s)" % (kind, n, worst, worst / scale, who))


def _fp_kind(kind, n, monkeypatch, create, result, check, special=True):
    from snprelate_amd import _lib
    monkeypatch.delenv("SNPGPU_PREP_TWO_PASS", raising=False)
    results = {}
    for form in _forms(n, special):
        with _lib.Accumulator(create[0], n, max_block_snps=MAXB, **create[1]) as a:
            _check_stats(form, F.feed(a, form), n, special)
            r = result(a)
        check(r, form.name)
        results[form.name] = r
    _report(kind, n, results)


@pytest.mark.parametrize("n", NS_FP)
def test_king_homo_every_form(n, monkeypatch):
    from snprelate_amd import _lib
    r0, r1 = _ref("king_homo", n, lambda g: orc.king_homo_final(*orc.king_homo_count(g), n))

    def check(r, name):
        np.testing.assert_allclose(r[0], r0, rtol=1e-5, atol=1e-7, equal_nan=True, err_msg=name)      # tests/test_gpu_parity.py:92
        np.testing.assert_allclose(r[1], r1, rtol=1e-5, atol=2e-5, equal_nan=True, err_msg=name)      # tests/test_gpu_parity.py:93
    _fp_kind("KING_HOMO", n, monkeypatch, (_lib.KING_HOMO, {}), lambda a: a.king_homo(packed=True), check)


@pytest.mark.parametrize("n", NS_FP)
def test_grm_gcta_every_form(n, monkeypatch):
    from snprelate_amd import _lib
    ref = _ref("grm", n, orc.grm_gcta)
    s, c = F.snp_stats(_geno(n))
    n_locus = int(((0 < s) & (s < 2 * c)).sum())           # src/genPCA.cpp:1206: the SNPs GCTA counts

    def result(a):
        return a.grm_gcta(packed=True), np.array(a.counts(), np.float64)

    def check(r, name):
        assert _rel_err(r[0], ref) < 1e-5, name                                        # tests/test_gpu_parity.py:218
        assert np.array_equal(np.isfinite(r[0]), np.isfinite(ref)), name               # tests/test_gpu_parity.py:219-220
        assert tuple(r[1]) == (L, n_locus), (name, r[1])
    _fp_kind("GRM_GCTA", n, monkeypatch, (_lib.GRM_GCTA, {}), result, check)


@pytest.mark.parametrize("bayesian", [False, True])
@pytest.mark.parametrize("n", NS_FP)
def test_pca_cov_every_form(n, bayesian, monkeypatch):
    from snprelate_amd import _lib
    special = not bayesian                                  # as tests/test_gpu_parity.py:254
    ref = _ref("pca%d" % bayesian, n, lambda g: orc.pca_cov(g, bayesian), special).copy()
    tr_ref = orc.trace_normalize(ref, n)

    def result(a):
        got, tr = a.pca_cov(packed=True, normalize=True)
        return got, np.array([tr])

    def check(r, name):
        assert abs(r[1][0] - tr_ref) / tr_ref < 1e-6, name                             # tests/test_gpu_parity.py:261
        assert _rel_err(r[0], ref) < 1e-5, name                                        # tests/test_gpu_parity.py:262
    _fp_kind("PCA_COV bayes" if bayesian else "PCA_COV", n, monkeypatch, (_lib.PCA_COV, {"bayesian": bayesian}), result, check, special)


@pytest.mark.parametrize("n", NS_FP)
def test_eigmix_every_form(n, monkeypatch):
    from snprelate_amd import _lib
    ref = _ref("eigmix", n, lambda g: orc.eigmix(g, True)[0])

    def check(r, name):
        assert _rel_err(r[0], ref) < 1e-5, name                                        # tests/test_gpu_parity.py:337
    _fp_kind("EIGMIX", n, monkeypatch, (_lib.EIGMIX, {}), lambda a: (a.eigmix(diagadj=True, packed=True),), check)


@pytest.mark.parametrize("n", NS_FP)
def test_indiv_beta_every_form(n, monkeypatch):
    from snprelate_amd import _lib
    cnt = _ref("beta", n, orc.beta_count)
    refs = ((1, orc.beta_final_ibd(cnt, n, True)), (0, orc.beta_final_ibd(cnt, n, False)), (2, orc.beta_final_grm(cnt, n)))

    def result(a):
        out = []
        for mode, _ in refs:
            got, avg = a.indiv_beta(mode=mode, packed=True)
            out += [got, np.array([avg])]
        return tuple(out)

    def check(r, name):
        for k, (mode, ref) in enumerate(refs):
            np.testing.assert_allclose(r[2 * k], ref[0], rtol=1e-10, atol=1e-12, equal_nan=True, err_msg=name)      # tests/test_gpu_parity.py:320
            np.testing.assert_allclose(r[2 * k + 1][0], ref[1], rtol=1e-11, err_msg=name)                            # tests/test_gpu_parity.py:321
    _fp_kind("INDIV_BETA", n, monkeypatch, (_lib.INDIV_BETA, {}), result, check)


# ---- row panels: col0 != 0 in the one-pass pre-pass ---------------------------------------------------------------------------------
def test_row_panel_ibs_and_grm_from_dirty_2bit_rows(monkeypatch):
    """rows 512 .. 1023 of 1037 samples: the panel's columns start at sample 512, its second 1024-sample workgroup does not exist
    and the first one ends in the 13-sample dword; slabs against the oracle's slab range as tests/test_gpu_parity.py:652-659"""
    from snprelate_amd import _lib
    from snprelate_amd.dist import slab_range
    n, r0, r1 = 1037, 512, 1024
    lo, hi = slab_range(n, r0, r1)
    ibs, grm = _ref("ibs", n, orc.ibs_count), _ref("grm", n, orc.grm_gcta)
    forms = [f for f in _forms(n) if f.name in ("packed_dirty device + 0", "packed_dirty device + 1")]
    assert len(forms) == 2
    for form in forms:
        for two_pass in _routes(form):
            got = _run_counter(_lib.IBS, n, form, monkeypatch, two_pass, lambda a: np.stack(a.ibs_num(packed=True), 1).astype(np.uint32),
                               row_begin=r0, row_end=r1)
            assert np.array_equal(got, ibs[lo:hi]), (form.name, two_pass)
        part = _run_counter(_lib.GRM_GCTA, n, form, monkeypatch, False, lambda a: a.grm_gcta(packed=True), row_begin=r0, row_end=r1)
        fin, f2 = np.isfinite(grm), np.isfinite(grm[lo:hi])
        assert np.array_equal(np.isfinite(part), f2), form.name
        assert np.nanmax(np.abs(part[f2] - grm[lo:hi][f2])) < 1e-5 * np.nanmax(np.abs(grm[fin])), form.name      # tests/test_gpu_parity.py:659


# ---- LDMatrix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["composite", "r"])
@pytest.mark.parametrize("n", [63, 65])
def test_ld_matrix_every_form(n, method):
    """sliding window of 50, every host and device form (snpgpu_ld_feed has no pinned and no statistics entry), compared as
    tests/test_gpu_ld.py::_check compares"""
    from snprelate_amd import _lib
    ref = _ref("ld_" + method, n, lambda x: ld_ref.ld_mat(x, method, 50, False))
    code = list(ld_ref.METHODS).index(method) + 1
    for form in _forms(n, pinned=False, stats=False):
        with _lib.LDMatrix(n, L, code, 50, False, max_block_snps=MAXB) as ld:
            F.feed(ld, form)
            got = ld.result()
        assert got.shape == ref.shape
        assert np.array_equal(np.isnan(got), np.isnan(ref)), form.name
        tol = 1e-6 if method in ("r", "dprime") else 1e-12                          # tests/test_gpu_ld.py: _check
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, equal_nan=True, err_msg=form.name)


# ---- Projector --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 17, 33])
@pytest.mark.parametrize("n", [63, 65, 333])
def test_projector_dirty_forms(n, k):
    """snp_corr, snp_loading and samp_loading_feed with one, two and three column passes (k = 1 / 16, 17, 33) on dirty U8 and dirty
    2-bit rows; oracle functions and tolerances of tests/test_gpu_api_golden.py::test_projector_vs_oracle_synthetic"""
    from snprelate_amd import _lib
    g = _geno(n)
    rng = np.random.default_rng(4 + k)
    ev = rng.normal(size=(k, n))
    w = np.linspace(3.0, 0.5, k)
    tr = 123.4
    rc = orc.pca_snp_corr(g, ev)
    for form in _forms(n)[1:3]:
        assert form.name in ("u8_dirty", "packed_dirty") and form.mem == "host"
        with _lib.Projector(n, k, max_block_snps=MAXB) as p:
            p.set_eigvec(ev)
            corr = np.concatenate([p.snp_corr(b) for b in form.blocks])
            assert np.array_equal(np.isnan(corr), np.isnan(rc)), form.name
            np.testing.assert_allclose(corr, rc, rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=form.name)
            for bayes in (False, True):
                p.set_eigvec(ev * np.sqrt((n - 1) / tr / w)[:, None])
                parts = [p.snp_loading(b, bayesian=bayes) for b in form.blocks]
                rl, ra, rs = orc.pca_snp_loading(g, w, ev, tr, bayesian=bayes)
                np.testing.assert_allclose(np.concatenate([x[1] for x in parts]), ra, rtol=1e-14, err_msg=form.name)
                np.testing.assert_allclose(np.concatenate([x[2] for x in parts]), rs, rtol=1e-14, err_msg=form.name)
                np.testing.assert_allclose(np.concatenate([x[0] for x in parts]), rl, rtol=1e-10, atol=1e-12, err_msg=form.name)
            sload = rl * 0.37
        with _lib.Projector(n, k, max_block_snps=MAXB) as p:
            for (a, b), blk in zip(zip(CUTS[:-1], CUTS[1:]), form.blocks):
                p.samp_loading_feed(blk, sload[a:b], ra[a:b], rs[a:b])
            got = p.samp_loading()
        np.testing.assert_allclose(got, orc.pca_samp_loading(g, sload, ra, rs), rtol=1e-10, atol=1e-11, err_msg=form.name)


# ---- MultiAccumulator -------------------------------------------------------------------------------------------------------------
def test_multi_accumulator_dirty_forms():
    """one device, two panels, 1037 samples: dirty U8 rows from the host and dirty 2-bit rows from the device"""
    from snprelate_amd import _lib
    n = 1037
    ibs, grm = _ref("ibs", n, orc.ibs_count), _ref("grm", n, orc.grm_gcta)
    forms = [f for f in _forms(n) if f.name in ("u8_dirty", "packed_dirty device + 0")]
    assert len(forms) == 2
    for form in forms:
        with _lib.MultiAccumulator(_lib.IBS, n, devices=(0,), panels_per_device=2, max_block_snps=MAXB) as m:
            assert m.info()["n_panels"] == 2
            F.feed(m, form)
            assert np.array_equal(np.stack(m.ibs_num(), 1).astype(np.uint32), ibs), form.name
        with _lib.MultiAccumulator(_lib.GRM_GCTA, n, devices=(0,), panels_per_device=2, max_block_snps=MAXB) as m:
            F.feed(m, form)
            assert m.counts()[0] == L
            got = m.grm_gcta()
        assert _rel_err(got, grm) < 1e-5, form.name
        assert np.array_equal(np.isfinite(got), np.isfinite(grm)), form.name
