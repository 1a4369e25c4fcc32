"""Results read BETWEEN feeds, for every accumulator kind: feed -> result -> feed -> result, as a progress report or a checkpointing
caller does it.  A context carries state from block to block and from call to call -- the pending row / column terms of the SYRK
kernels (colterm / uvterm: folded by snpgpu_grm_gcta, settled into the panel and zeroed by every other reader), sums that are zeroed
only at creation (KING-homo's and the dissimilarity's het_pending / homo_msum / d_homo_w / diss_called, EIGMIX's samp_het / samp_dmiss /
samp_dsq / d_sumden), the eigen solver's fp32 copy of the panel and its mirrored diagonal tiles, and the scratch slots of the
carried-sum GRM kernel.

One stream of ten ragged blocks (with and without missing calls, a monomorphic and an all-missing SNP; rare variants in both kinds of
block at 700 samples) is read after blocks 2, 6 and 10, twice in a row each time.  Every reference is the CPU oracle (or the numpy
restatement tests/diss_ref.py) on the PREFIX fed so far, never a second GPU run; the tolerances are those of each kind's one-shot
test (tests/test_gpu_parity.py, tests/test_gpu_diss.py, tests/test_gpu_api_golden.py)."""
import numpy as np
import pytest

import diss_ref as R
import oracle as orc
from conftest import synth_geno

pytestmark = pytest.mark.gpu

# block sizes around the 1024-slot table chunk; the prefix of checkpoint 2 ends in a block without missing calls, that of checkpoint 6
# in a block with them.  Both 2048 / 2000-SNP blocks are complete: two fp32 runs of the single-product kernel at SNPGPU_H3_PROMOTE=1024
SIZES = (700, 2048, 1, 1024, 1025, 64, 2000, 513, 16, 300)
WITH_MISSING = (True, False, True, False, False, True, False, True, False, True)
CUTS = np.cumsum((0,) + SIZES)
CHECKPOINTS = (2, 6, 10)
BMAX = 2048
PANEL_BOUNDS = (0, 256, 512)          # + n: three row panels, the last one ragged
DISS_ROWS = np.array([0, 1, 100, 255, 256, 257, 270, 300, 400, 511, 512, 513, 520, 528, 529, 530])


def _make_geno(n):
    g = synth_geno(n, int(CUTS[-1]), missing=0.0, seed=1000 + n, special=False)
    rng = np.random.default_rng(n)
    if n == 700:                      # rare variants (at most 128 copies of the minor allele), both allele orientations
        for b in (0, 1, 3, 5, 6, 7):
            for k, row in enumerate(range(CUTS[b] + 11, min(CUTS[b] + 53, CUTS[b + 1]), 7)):
                g[row] = 0
                g[row, rng.choice(n, size=1 + 9 * k, replace=False)] = 1 + k % 2
                if k % 3 == 2:
                    g[row] = 2 - g[row]
    for b, m in enumerate(WITH_MISSING):
        if m:
            sub = g[CUTS[b]:CUTS[b + 1]]
            sub[rng.random(sub.shape) < 0.06] = 3
    g[CUTS[1] + 5] = 2                # a monomorphic SNP in a block without missing calls
    g[CUTS[0] + 9] = 3                # an all-missing SNP in a block with them
    for b, m in enumerate(WITH_MISSING):
        assert bool((g[CUTS[b]:CUTS[b + 1]] > 2).any()) == m
    g.setflags(write=False)
    return g


def _frozen(x):
    for a in (x if isinstance(x, tuple) else (x,)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


class _Stream:
    """the genotypes of one sample count and the references of its prefixes, each computed once and left unchanged"""

    def __init__(self, g):
        self.g, self.n, self._cache = g, g.shape[1], {}

    def prefix(self, b):
        return self.g[:CUTS[b]]

    def ref(self, name, b, fn):
        if (name, b) not in self._cache:
            self._cache[(name, b)] = _frozen(fn(self.prefix(b)))
        return self._cache[(name, b)]

    def grm(self, b):
        return self.ref("grm", b, orc.grm_gcta)

    def cov_raw(self, b, bayes=False):
        return self.ref("cov%d" % bayes, b, lambda p: orc.pca_cov(p, bayes))

    def cov_norm(self, b, bayes=False):
        """(trace-normalised covariance, TraceXTX)"""
        def fn(p):
            c = self.cov_raw(b, bayes).copy()
            tr = orc.trace_normalize(c, self.n)
            return c, tr
        return self.ref("covn%d" % bayes, b, fn)

    def eigmix(self, b, diagadj):
        return self.ref("eigmix%d" % diagadj, b, lambda p: orc.eigmix(p, diagadj)[0])

    def king_homo(self, b):
        return self.ref("king_homo", b, lambda p: orc.king_homo_final(*orc.king_homo_count(p), self.n))

    def ibs(self, b):
        return self.ref("ibs", b, orc.ibs_count)

    def mom(self, b, cons):
        return self.ref("mom%d" % cons, b, lambda p: orc.mom_final(self.ibs(b), self.n, orc.mom_expect(p)[0], cons))

    def beta(self, b, mode):
        def fn(p):
            cnt = self.ref("beta_cnt", b, orc.beta_count)
            return orc.beta_final_grm(cnt, self.n) if mode == 2 else orc.beta_final_ibd(cnt, self.n, mode == 1)
        return self.ref("beta%d" % mode, b, fn)

    def diss_rows(self, b):
        """tests/diss_ref.py on the rows DISS_ROWS x every column: (SumGeno, SumAFreq, dissimilarity).  (Its integer products take
        a minute on the whole matrix; SumGeno of every pair comes from the oracle's KING-robust counters, see diss_sum_geno.)"""
        def fn(p):
            sg, sa = R.diss_sums(p, rows=DISS_ROWS)
            with np.errstate(invalid="ignore", divide="ignore"):
                d = sg / sa
            d[np.arange(DISS_ROWS.size), DISS_ROWS] *= 2          # (diss_ref.diss_matrix, on the sums at hand)
            return sg, sa, d
        return self.ref("diss_rows", b, fn)

    def diss_sum_geno(self, b):
        """SumGeno = SumSq + N1_Aa + N2_Aa of the KING-robust counters (the second route of test_gpu_diss.test_sum_geno_bit_exact)"""
        def fn(p):
            k = orc.king_robust_count(p).astype(np.int64)
            return k[:, 2] + k[:, 3] + k[:, 4]
        return self.ref("diss_sg", b, fn)


@pytest.fixture(scope="module")
def stream531():
    return _Stream(_make_geno(531))


@pytest.fixture(scope="module")
def stream700():
    return _Stream(_make_geno(700))


@pytest.fixture
def stream(request, stream531, stream700):
    return {531: stream531, 700: stream700}[request.param]


both_sizes = pytest.mark.parametrize("stream", [531, 700], indirect=True)


def _rel_err(got, ref):
    """tests/norms.py: the larger of the contract figure and the off-diagonal-floor figure (as tests/test_gpu_parity.py)"""
    from norms import error_figures, tri_diag_scale
    n = int((np.sqrt(8 * ref.size + 1) - 1) / 2 + 0.5)
    f = error_figures(got, ref, tri_diag_scale(ref, n))
    return max(f["contract"], f["offdiag"])


def _equal(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return np.array_equal(x, y, equal_nan=bool(np.issubdtype(x.dtype, np.floating)))


def _checkpoints(feed, g, stops=CHECKPOINTS):
    """feed(block) the blocks up to each stop in turn; yields the stop"""
    done = 0
    for b in stops:
        for k in range(done, b):
            feed(g[CUTS[k]:CUTS[k + 1]])
        done = b
        yield b


def _acc(kind, n, **kw):
    from snprelate_amd import _lib
    return _lib.Accumulator(getattr(_lib, kind), n, max_block_snps=BMAX, **kw)


# ---- what is read of each kind, and how it is checked (the figures of the kind's one-shot test) --------------------------------------

def _read_gcta(a):
    return a.grm_gcta(packed=True), a.grm_gcta(packed=False)


def _check_gcta(out, s, b):
    packed, full = out
    ref = s.grm(b)
    assert _rel_err(packed, ref) < 1e-5
    assert np.array_equal(np.isfinite(packed), np.isfinite(ref))
    assert np.array_equal(full, orc.tri_to_full(packed, s.n))


def _read_pca(a):
    norm, tr = a.pca_cov(packed=True, normalize=True)
    raw, tr_raw = a.pca_cov(packed=True, normalize=False)
    full, _ = a.pca_cov(packed=False, normalize=True)
    return norm, raw, full, np.array([tr, tr_raw])


def _check_pca(out, s, b, bayes=False):
    norm, raw, full, tr = out
    ref, tr_ref = s.cov_norm(b, bayes)
    assert abs(tr[0] - tr_ref) / tr_ref < 1e-6 and tr[0] == tr[1]
    assert _rel_err(norm, ref) < 1e-5
    assert _rel_err(raw, s.cov_raw(b, bayes)) < 1e-5
    assert np.array_equal(full, orc.tri_to_full(norm, s.n))


def _read_eigmix(a):
    return a.eigmix(diagadj=True, packed=True), a.eigmix(diagadj=False, packed=True)


def _check_eigmix(out, s, b):
    assert _rel_err(out[0], s.eigmix(b, True)) < 1e-5
    assert _rel_err(out[1], s.eigmix(b, False)) < 1e-5


def _read_king_homo(a):
    return a.king_homo(packed=True)


def _check_king_homo(out, s, b):
    r0, r1 = s.king_homo(b)
    np.testing.assert_allclose(out[0], r0, rtol=1e-5, atol=1e-7, equal_nan=True)
    np.testing.assert_allclose(out[1], r1, rtol=1e-5, atol=2e-5, equal_nan=True)


def _read_diss(a):
    sg, sa = a.diss_sums()
    return sg, sa, a.diss(packed=True), a.diss(packed=False)


def _check_diss(out, s, b):
    sg, sa, packed, full = out
    n = s.n
    rtol = 2e-6                       # test_gpu_diss._rtol: every prefix holds blocks with missing calls
    assert np.array_equal(sg.astype(np.int64), s.diss_sum_geno(b))
    rsg, rsa, rd = s.diss_rows(b)
    assert np.array_equal(orc.tri_to_full(sg, n)[DISS_ROWS].astype(np.int64), rsg)
    np.testing.assert_allclose(orc.tri_to_full(sa, n)[DISS_ROWS], rsa, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(full[DISS_ROWS], rd, rtol=rtol, equal_nan=True)
    assert np.array_equal(full, full.T, equal_nan=True)
    assert np.array_equal(packed, R.packed_upper(full), equal_nan=True)


def _read_beta(a):
    out = []
    for mode in (1, 0, 2):
        m, avg = a.indiv_beta(mode=mode, packed=True)
        out += [m, np.array([avg])]
    return tuple(out)


def _check_beta(out, s, b):
    for k, mode in enumerate((1, 0, 2)):
        ref = s.beta(b, mode)
        np.testing.assert_allclose(out[2 * k], ref[0], rtol=1e-10, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(out[2 * k + 1][0], ref[1], rtol=1e-11)


def _check_ibs(out, s, b):
    ref = s.ibs(b)
    for k in range(3):
        assert np.array_equal(out[k], ref[:, k])
    for k, cons in enumerate((False, True)):
        r0, r1 = s.mom(b, cons)
        np.testing.assert_allclose(out[3 + 2 * k], r0, rtol=1e-12, atol=1e-14, equal_nan=True)
        np.testing.assert_allclose(out[4 + 2 * k], r1, rtol=1e-12, atol=1e-14, equal_nan=True)


def _reader_ibs(s):
    """PLINK MoM needs the expectations of the prefix: the reader looks them up by the SNPs fed so far"""
    def read(a):
        e = orc.mom_expect(s.g[:a.counts()[0]])[0]
        return tuple(a.ibs_num(packed=True)) + a.ibd_mom(e, constraint=False, packed=True) + a.ibd_mom(e, constraint=True, packed=True)
    return read


KINDS = {                             # name: (context kind, creation keywords, read, check)
    "GRM_GCTA": ("GRM_GCTA", {}, _read_gcta, _check_gcta),
    "PCA_COV": ("PCA_COV", {}, _read_pca, _check_pca),
    "PCA_COV_BAYES": ("PCA_COV", {"bayesian": True}, _read_pca, lambda o, s, b: _check_pca(o, s, b, True)),
    "EIGMIX": ("EIGMIX", {}, _read_eigmix, _check_eigmix),
    "KING_HOMO": ("KING_HOMO", {}, _read_king_homo, _check_king_homo),
    "DISS": ("DISS", {}, _read_diss, _check_diss),
    "INDIV_BETA": ("INDIV_BETA", {}, _read_beta, _check_beta),
    "IBS": ("IBS", {}, None, _check_ibs),
}


def _prefix_parity(name, s, at_checkpoint=None):
    """test 1: at every checkpoint two reads in a row, equal to each other and within the kind's tolerance of the prefix's reference"""
    kind, kw, read, check = KINDS[name]
    read = read or _reader_ibs(s)
    with _acc(kind, s.n, **kw) as a:
        for b in _checkpoints(a.feed, s.g):
            first, second = read(a), read(a)
            assert a.counts()[0] == CUTS[b]
            assert all(_equal(x, y) for x, y in zip(first, second)), "two reads after block %d differ" % b
            check(first, s, b)
            if at_checkpoint:
                at_checkpoint(a, b)


@both_sizes
@pytest.mark.parametrize("name", ["GRM_GCTA", "PCA_COV", "PCA_COV_BAYES", "EIGMIX", "KING_HOMO", "INDIV_BETA", "IBS"])
def test_prefix_parity(name, stream):
    _prefix_parity(name, stream)


def test_prefix_parity_diss(stream531):
    _prefix_parity("DISS", stream531)


# ---- 2. a read does not disturb the sum ----------------------------------------------------------------------------------------------

def _read_at_checkpoints_and_only_at_the_end(kind, g, read, **kw):
    n = g.shape[1]
    with _acc(kind, n, **kw) as a:
        for _ in _checkpoints(a.feed, g):
            often = read(a)
    with _acc(kind, n, **kw) as a:
        for _ in _checkpoints(a.feed, g, stops=(len(SIZES),)):
            pass
        once = read(a)
    return often, once


@pytest.mark.parametrize("kind", ["IBS", "DISS"])
def test_reads_leave_integer_results_unchanged(kind, stream531):
    read = (lambda a: np.stack(a.ibs_num(packed=True))) if kind == "IBS" else (lambda a: a.diss_sums()[0])
    often, once = _read_at_checkpoints_and_only_at_the_end(kind, stream531.g, read)
    assert np.array_equal(often, once)


def _no_rare_variants(g):
    """the stream without the SNPs of at most 128 copies of the minor allele among the called genotypes (the fp64 atomics of the sparse
    kernels, whose order changes from run to run), block boundaries kept -- as test_gpu_carry_all.test_lds_carried_sub_tiles_unchanged"""
    called = g < 3
    s = np.where(called, g, 0).sum(1, dtype=np.int64)
    keep = np.minimum(s, 2 * called.sum(1, dtype=np.int64) - s) > 128
    blocks = [np.ascontiguousarray(g[CUTS[b]:CUTS[b + 1]][keep[CUTS[b]:CUTS[b + 1]]]) for b in range(len(SIZES))]
    return blocks, keep


def test_reads_leave_gcta_bit_identical(stream531, monkeypatch):
    """snpgpu_grm_gcta folds the pending terms into its OUTPUT and leaves panel and terms alone: a context that was read at every
    checkpoint ends bit-identical to one that was read once.  Whole tiles (no split along K), no rare variants: every panel entry is
    one sequence of additions in stream order."""
    monkeypatch.setenv("SNPGPU_I8_TAIL_PARTS", "1")
    blocks, keep = _no_rare_variants(stream531.g)
    assert keep.mean() > 0.7 and all(len(x) for x in blocks)
    n = stream531.n
    res = []
    for stops in (CHECKPOINTS, (len(SIZES),)):
        with _acc("GRM_GCTA", n) as a:
            for b, blk in enumerate(blocks):
                a.feed(blk)
                if b + 1 in stops:
                    got = a.grm_gcta(packed=True)
        res.append(got)
    assert _rel_err(res[0], orc.grm_gcta(np.concatenate(blocks))) < 1e-5
    assert np.array_equal(res[0], res[1])


def test_reads_settle_pca_cov_within_rounding(stream531):
    """every read of a PCA_COV context settles the pending terms INTO the panel: other roundings than one settlement at the end, the
    same tolerance -- against the oracle and against each other"""
    often, once = _read_at_checkpoints_and_only_at_the_end("PCA_COV", stream531.g, lambda a: a.pca_cov(packed=True, normalize=False)[0])
    ref = stream531.cov_raw(len(SIZES))
    assert _rel_err(often, ref) < 1e-5 and _rel_err(once, ref) < 1e-5
    assert _rel_err(often, once) < 1e-5


# ---- 3. kernel paths of GRM_GCTA / PCA_COV at 531 samples ----------------------------------------------------------------------------

WHOLE_TILES = {"SNPGPU_I8_TAIL_PARTS": "1", "SNPGPU_H3_PROMOTE": "1024"}     # 2048-SNP blocks: two runs, carried in LDS and scratch slots
PATHS = {
    "carry": WHOLE_TILES,
    "carry_no_slots": dict(WHOLE_TILES, SNPGPU_UVC_CARRY_SLOTS="0"),          # every work item falls back to the per-run panel flush
    "carry_lds_only": dict(WHOLE_TILES, SNPGPU_UVC_CARRY_ALL="0"),
    "f32": {"SNPGPU_SYRK": "f32"},
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["GRM_GCTA", "PCA_COV"])
def test_prefix_parity_kernel_paths(name, path, stream531, monkeypatch):
    """(the default environment is test_prefix_parity: every tile of 531 samples is split along K there, nothing is carried)"""
    from snprelate_amd import _lib
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    check = None
    if path == "carry":
        d = _lib.diag_plan(getattr(_lib, name), 531, block_snps=2048, max_block_snps=BMAX)
        assert (d["uv_form"], d["uvc_carry_all"], int(d["uv_runs"])) == ("converted_carry", "1", 2)

        def check(a, b):
            assert a.carry_fallbacks() == 0
    _prefix_parity(name, stream531, at_checkpoint=check)


@pytest.mark.parametrize("name", ["GRM_GCTA", "PCA_COV"])
def test_prefix_parity_three_row_panels(name, stream531, monkeypatch):
    """three row panels (a column offset, padding rows) fed side by side; at every checkpoint all of them are read, twice"""
    from snprelate_amd.dist import slab_range
    for k, v in WHOLE_TILES.items():
        monkeypatch.setenv(k, v)
    s, n = stream531, 531
    bounds = list(PANEL_BOUNDS) + [n]
    panels = [_acc(name, n, row_begin=r0, row_end=r1) for r0, r1 in zip(bounds[:-1], bounds[1:])]

    def read():
        out, tr = np.zeros(n * (n + 1) // 2), 0.0
        for a, r0, r1 in zip(panels, bounds[:-1], bounds[1:]):
            lo, hi = slab_range(n, r0, r1)
            if name == "GRM_GCTA":
                out[lo:hi] = a.grm_gcta(packed=True)
            else:
                out[lo:hi] = a.pca_cov(packed=True, normalize=False)[0]
                tr += a.pca_panel_trace()
        return out, tr

    def feed(block):
        for a in panels:
            a.feed(block)
    try:
        for b in _checkpoints(feed, s.g):
            (first, tr), (second, _) = read(), read()
            assert np.array_equal(first, second)
            assert all(a.carry_fallbacks() == 0 for a in panels)
            if name == "GRM_GCTA":
                assert _rel_err(first, s.grm(b)) < 1e-5
            else:
                assert _rel_err(first, s.cov_raw(b)) < 1e-5
                tr_ref = s.cov_norm(b)[1]
                assert abs(tr - tr_ref) / tr_ref < 1e-6
    finally:
        for a in panels:
            a.close()


def test_gcta_ten_runs_carried_on_whole_tiles(monkeypatch):
    """one block of 10 240 SNPs at 1024-slot runs: ten runs (more than UV_QMAX = 8: one weight target), every sub-tile sum carried
    across all of them on tiles that are not split along K"""
    from snprelate_amd import _lib
    for k, v in WHOLE_TILES.items():
        monkeypatch.setenv(k, v)
    n, L = 531, 10240
    d = _lib.diag_plan(_lib.GRM_GCTA, n, block_snps=L, max_block_snps=L)
    assert (d["uv_form"], int(d["uv_runs"])) == ("converted_carry", 10)
    g = synth_geno(n, L, missing=0.0, seed=1531, special=False)
    with _lib.Accumulator(_lib.GRM_GCTA, n, max_block_snps=L) as a:
        a.feed(g)
        got = a.grm_gcta(packed=True)
        assert a.carry_fallbacks() == 0
    assert _rel_err(got, orc.grm_gcta(g)) < 1e-5


# ---- 4. the panel product after further feeds ----------------------------------------------------------------------------------------

M_VEC = 8


def _panel_product(a, q, fp32=False):
    import torch
    y = torch.zeros_like(q)
    torch.cuda.synchronize()
    a.pca_panel_matmul(1.0, q.data_ptr(), M_VEC, y.data_ptr(), fp32=fp32)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@both_sizes
@pytest.mark.parametrize("form", ["tile_mirror", "rocblas"])
def test_panel_product_after_further_feeds(form, stream, monkeypatch):
    """snpgpu_pca_panel_matmul at every checkpoint: the product reads the lower triangles of the diagonal tiles (the whole diagonal
    square in the rocBLAS form), which it mirrors from the upper ones -- after every feed anew, since the feed kernels add below the
    diagonal what is not the transpose of what they add above it.  (Mirrored once per context, the product after block 6 was off
    by 0.19 at 531 samples and 0.15 at 700 in the Frobenius norm, dgemm form; mirrored after every feed: 1.6e-7 and 2.0e-7.)
    fp64 form: relative Frobenius error below 1e-5 against the prefix's oracle covariance (the matrix itself is that good).
    fp32 form (the tile form only: the dgemm form has none) -- its copy of the panel is stale after a feed: the figure of
    test_gpu_api_golden.test_panel_product_fp32_form, error / sum of |terms| < 4e-7, against the same oracle product.  (With the
    stale copy: 0.23 after block 6.  That figure counts the fp32 sums of the product: with 1024 columns per workgroup at every size it
    read 4.7e-7 ... 6.4e-7 at 531 samples and 4.2e-7 ... 6.1e-7 at 700 on a context that was fed and read ONCE; panels too small
    to fill the device now take 128-column chunks, 2.2e-7 ... 3.2e-7 and 2.0e-7 ... 3.2e-7.)"""
    import torch
    if form == "rocblas":
        monkeypatch.setenv("SNPGPU_EIG_BLAS", "1")
    s = stream
    qh = np.random.default_rng(7).normal(size=(M_VEC, s.n))
    q = torch.from_numpy(qh).to("cuda:0")
    with _acc("PCA_COV", s.n) as a:
        for b in _checkpoints(a.feed, s.g):
            cov = orc.tri_to_full(s.cov_raw(b), s.n)
            ref = qh @ cov
            for _ in range(2):
                y = _panel_product(a, q)
                err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
                print("%s n %d after block %d: fp64 product rel Frobenius %.3g" % (form, s.n, b, err))
                assert err < 1e-5
            if form == "tile_mirror":
                y32 = _panel_product(a, q, fp32=True)
                e32 = (np.abs(y32 - ref) / (np.abs(qh) @ np.abs(cov))).max()
                print("%s n %d after block %d: fp32 product err / sum |terms| %.3g" % (form, s.n, b, e32))
                assert e32 < 4e-7
                assert np.abs(y32 - y).max() > 0            # it IS the fp32 form


def test_krylov_eigen_between_feeds(stream531, monkeypatch):
    """snpgpu_pca_eigen on the block-Krylov solver (fp32 and fp64 panel products) after block 6 and again after block 10"""
    monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "0")
    s, n, k = stream531, 531, 8
    with _acc("PCA_COV", n) as a:
        for b in _checkpoints(a.feed, s.g, stops=(6, 10)):
            w, v = a.pca_eigen(k)
            full = orc.tri_to_full(s.cov_norm(b)[0], n)
            w_ref = np.linalg.eigvalsh(full)[::-1][:k]
            np.testing.assert_allclose(w, w_ref, rtol=1e-6, atol=1e-9)
            res = np.linalg.norm(full @ v - v * w, axis=0) / np.abs(w)
            assert res.max() < 1e-5


# ---- 5. frozen contexts --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,diagadj", [("GRM_GCTA", True), ("EIGMIX", True), ("EIGMIX", False)])
def test_finalize_inplace_then_nothing_may_follow(name, diagadj, stream531):
    from snprelate_amd import _lib
    s, last = stream531, len(SIZES)
    read = (lambda a: a.grm_gcta(packed=True)) if name == "GRM_GCTA" else (lambda a: a.eigmix(diagadj=diagadj, packed=True))
    with _acc(name, s.n) as a:
        for _ in _checkpoints(a.feed, s.g, stops=(last,)):
            pass
        before = read(a)
        a.finalize_inplace(diagadj=diagadj)
        first, second = read(a), read(a)
        assert np.array_equal(first, second)
        if name == "GRM_GCTA":
            assert np.array_equal(first, before)           # the stored matrix IS what the finaliser computes
            assert _rel_err(first, s.grm(last)) < 1e-5
        else:                                              # the same kernel wrote it; read back through a multiplication by 1.0
            np.testing.assert_allclose(first, before, rtol=1e-13, atol=0)
            assert _rel_err(first, s.eigmix(last, diagadj)) < 1e-5
        with pytest.raises(_lib.SnpGpuError, match="no blocks may follow"):
            a.feed(s.g[:16])
        assert a.counts()[0] == CUTS[last]
        assert np.array_equal(read(a), first)


# ---- 6. several panels in one process ------------------------------------------------------------------------------------------------

def test_multi_accumulator_gcta_between_feeds(stream531):
    from snprelate_amd import _lib
    s = stream531
    with _lib.MultiAccumulator(_lib.GRM_GCTA, s.n, devices=(0, 0, 0), panels_per_device=1, max_block_snps=BMAX) as m:
        for b in _checkpoints(m.feed, s.g, stops=(5, 10)):
            first, second = m.grm_gcta(), m.grm_gcta()
            assert m.counts()[0] == CUTS[b]
            assert np.array_equal(first, second)
            assert _rel_err(first, s.grm(b)) < 1e-5
