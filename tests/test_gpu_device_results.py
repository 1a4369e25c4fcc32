"""Every call of include/snpgpu.h that takes a result memory kind, handed DEVICE destinations (tests/mem_kinds.py: RESULT_CALLS).

For every call the result is taken twice into host memory and then into DeviceDest buffers 1 and 3 elements past a 256-byte boundary
(a double result 8-byte but not 16-byte aligned, an int32 result 4-byte aligned) between guards of a fill pattern.  read() copies
through a side stream without synchronising anything, so it sees what is in memory when the call has returned (the header: "calls
block until the result is in the caller's buffer"), and asserts that the guards are intact: a finaliser that stores a tile row past
its packed slab is invisible through a host destination, where the bytes land in the slack of the library's temporary.
Where the two host calls agree byte for byte, the device result has those bytes too.  Where the host form itself is not reproducible
(fp64 atomics: the projector; the iterative eigen solvers) both forms are held against the oracle of the call's own test with that
test's tolerance; RESULT_CALLS says which rule a call is under, and a call that turns out not to be reproducible without an oracle
named fails.  Optional outputs are also passed as NULL on the device path.  The projector calls whose every pointer is device memory
are stream-ordered (snpgpu.h, 1b): exactly those are followed by sync() before read().

Shapes: the smallest that cross what the kernels tile on -- full contexts of 37 and 279 samples, packed and full matrix, and the row
panel 256..512 of 600 samples (a slab length that is a multiple of nothing), 700 SNPs fed as 333 + 367 with 3 % missing calls."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import mem_kinds as M
import oracle as orc
import proj_ref
from conftest import synth_geno

pytestmark = pytest.mark.gpu

CONFIGS = [(37, None), (279, None), (600, (256, 512))]
CONFIG_IDS = ["n37", "n279", "n600_rows256_512"]
FULL = CONFIGS[:2]
CUTS = (0, 333, 700)


@functools.lru_cache(maxsize=None)
def _geno(n, L=700, seed=0):
    g = synth_geno(n, L, missing=0.03, seed=seed or 100 + n)
    g.setflags(write=False)
    return g


def _packed(g):
    from snprelate_amd.gds import pack_2bit_rows
    return pack_2bit_rows(np.asarray(g))


def _ctx(kind, n, rows, **kw):
    """an Accumulator over n samples (rows: None = full, or the panel's row range), fed _geno(n) as 333 + 367 SNPs"""
    from snprelate_amd import _lib
    r0, r1 = rows or (0, 0)
    a = _lib.Accumulator(getattr(_lib, kind), n, row_begin=r0, row_end=r1, max_block_snps=512, **kw)
    g = _geno(n)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        a.feed(g[lo:hi])
    return a


def _forms(rows):
    """the `packed` values a context has: both for a full one, the slab only for a panel"""
    return (True,) if rows else (True, False)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_bytes(what, got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.tobytes() != ref.tobytes():
        raw = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8).reshape(x.size, -1)      # noqa: E731
        ne = np.flatnonzero((raw(got) != raw(ref)).any(axis=1))
        k = int(ne[0])
        raise AssertionError("%s: device result differs from the host result in %d of %d elements, the first at flat index %d "
                             "(device %r, host %r)" % (what, ne.size, got.size, k, got.reshape(-1)[k], ref.reshape(-1)[k]))


def device_vs_host(what, call, oracle=None, absent=((),), after=None):
    """call(None) -> the results as a list of numpy arrays laid out as the library writes them; call(ptrs) -> the same call with the
    device addresses ptrs (None = that output is not asked for).  absent: the sets of output positions passed as NULL on the device
    path.  oracle(list of arrays, None where absent): the check against the reference, for calls whose host form is not reproducible.
    after: called between the device call and read() (sync of a stream-ordered call).  Returns the host results."""
    h1 = [np.ascontiguousarray(a) for a in call(None)]
    h2 = [np.ascontiguousarray(a) for a in call(None)]
    reproducible = all(_same(a, b) for a, b in zip(h1, h2))
    print("DEVICE-RESULT %-45s two host calls %s" % (what, "agree byte for byte" if reproducible else "DIFFER: held to the oracle"))
    assert reproducible or oracle is not None, \
        "%s: two host-memory calls differ and no oracle is named for this call (mem_kinds.RESULT_CALLS says 'bytes')" % what
    if oracle is not None:
        oracle(h1)
    for off, gone in itertools.product(M.OFFSETS, absent):
        dests = [None if k in gone else M.DeviceDest(a.shape, a.dtype, off) for k, a in enumerate(h1)]
        call([d.ptr if d else None for d in dests])
        if after is not None:
            after()
        got = [d.read() if d else None for d in dests]           # (asserts the guards)
        tag = "%s, offset %d%s" % (what, off, ", outputs %s NULL" % (sorted(gone),) if gone else "")
        if reproducible:
            for k, (a, r) in enumerate(zip(got, h1)):
                if a is not None:
                    _assert_bytes("%s, output %d" % (tag, k), a, r)
        if oracle is not None:
            oracle(got)
    return h1


# ---- the destination itself ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.uint8])
def test_device_dest_sees_writes_and_reports_those_outside(dtype):
    """the checks of tests/test_cpu_mem_kinds.py on the device buffer itself: a clean write comes back, one element in front of or
    behind the result is reported, untouched elements are told from written ones"""
    import torch
    item = np.dtype(dtype).itemsize
    val = (np.arange(35).reshape(5, 7) % 100 + 1).astype(dtype)
    for off in M.OFFSETS:
        d = M.DeviceDest((5, 7), dtype, off)
        assert (d.ptr - off * item) % 256 == 0 and d.ptr == d.buf.data_ptr() + d.layout.begin
        d.untouched(np.ones((5, 7), bool))
        d.put(val)
        assert np.array_equal(d.read(), val)
        for lo in (d.layout.begin - item, d.layout.end):
            d.buf[lo:lo + item] = 0
            torch.cuda.current_stream().synchronize()
            with pytest.raises(AssertionError, match="write outside a result"):
                d.read()
            d.buf[lo:lo + item] = M.FILL
            torch.cuda.current_stream().synchronize()
        assert np.array_equal(d.read(), val)
        with pytest.raises(AssertionError, match="have been written"):
            d.untouched(np.ones((5, 7), bool))


# ---- accumulator finalisers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_ibs_finalisers(n, rows):
    e, _ = orc.mom_expect(_geno(n))
    with _ctx("IBS", n, rows) as a:
        for packed in _forms(rows):
            device_vs_host("ibs_num packed=%d" % packed, lambda p: a.ibs_num(packed=packed, out_ptrs=p))
            device_vs_host("ibs_ave packed=%d" % packed, lambda p: [a.ibs_ave(packed=packed)] if p is None else a.ibs_ave(packed=packed, out_ptr=p[0]))
            for c in (False, True):
                device_vs_host("ibd_mom packed=%d constraint=%d" % (packed, c), lambda p: a.ibd_mom(e, constraint=c, packed=packed, out_ptrs=p))


@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_king_robust_finalisers(n, rows):
    fam = (np.arange(n) // 3).astype(np.int32)
    fam[::7] = -1
    with _ctx("KING_ROBUST", n, rows) as a:
        device_vs_host("king_robust_counts", lambda p: [a.king_robust_counts()] if p is None else a.king_robust_counts(out_ptr=p[0]))
        for packed in _forms(rows):
            for f in (None, fam, None):
                device_vs_host("king_robust packed=%d family=%s" % (packed, f is not None),
                               lambda p: a.king_robust(family=f, packed=packed, out_ptrs=p))


@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_king_homo_finaliser(n, rows):
    with _ctx("KING_HOMO", n, rows) as a:
        for packed in _forms(rows):
            device_vs_host("king_homo packed=%d" % packed, lambda p: a.king_homo(packed=packed, out_ptrs=p))


@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_diss_finalisers(n, rows):
    with _ctx("DISS", n, rows) as a:
        device_vs_host("diss_sums", lambda p: a.diss_sums(out_ptrs=p))
        for packed in _forms(rows):
            device_vs_host("diss packed=%d" % packed, lambda p: [a.diss(packed=packed)] if p is None else a.diss(packed=packed, out_ptr=p[0]))


@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_grm_gcta_finaliser(n, rows):
    with _ctx("GRM_GCTA", n, rows) as a:
        for packed in _forms(rows):
            device_vs_host("grm_gcta packed=%d" % packed, lambda p: [a.grm_gcta(packed=packed)] if p is None else a.grm_gcta(packed=packed, out_ptr=p[0]))


@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_pca_cov_finaliser(n, rows):
    with _ctx("PCA_COV", n, rows) as a:
        traces = []
        for packed in _forms(rows):
            # normalisation of a panel needs the trace of the whole diagonal: a given one; a full context also takes its own
            for normalize, trace_in in [(False, 0.0), (True, 1234.5)] + ([] if rows else [(True, 0.0)]):
                def call(p):
                    m, tr = a.pca_cov(packed=packed, normalize=normalize, trace_in=trace_in, out_ptr=None if p is None else p[0])
                    traces.append(tr)
                    return [m]
                device_vs_host("pca_cov packed=%d normalize=%d trace_in=%g" % (packed, normalize, trace_in), call)
        assert len(set(traces)) == 1 and traces[0] > 0          # trace_xtx: the panel's own diagonal, a host scalar, whatever the form


@pytest.mark.parametrize("n,rows", CONFIGS, ids=CONFIG_IDS)
def test_eigmix_finaliser(n, rows):
    with _ctx("EIGMIX", n, rows) as a:
        for packed in _forms(rows):
            for diagadj, scale in [(True, 1.0), (False, 2.0)]:
                device_vs_host("eigmix packed=%d diagadj=%d" % (packed, diagadj),
                               lambda p: [a.eigmix(diagadj, scale, packed)] if p is None else a.eigmix(diagadj, scale, packed, out_ptr=p[0]))


@pytest.mark.parametrize("n,rows", FULL, ids=CONFIG_IDS[:2])
def test_indiv_beta_finaliser(n, rows):
    with _ctx("INDIV_BETA", n, rows) as a:
        for packed in (True, False):
            for mode in (0, 1, 2):
                avgs = []

                def call(p):
                    m, avg = a.indiv_beta(mode=mode, packed=packed, out_ptr=None if p is None else p[0])
                    avgs.append(avg)
                    return [m]
                device_vs_host("indiv_beta packed=%d mode=%d" % (packed, mode), call)
                assert len(set(avgs)) == 1


def _eigen_oracle(cov_full, k):
    """the check of the eigen tests: eigenvalues against LAPACK with rtol 2e-5, residual |C v - w v| / |w| below 1e-8"""
    w_ref = np.linalg.eigvalsh(cov_full)[::-1][:k]

    def check(w, vt):
        np.testing.assert_allclose(w, w_ref, rtol=2e-5)
        v = vt.T                                                  # [k][n] as written -> n x k
        res = np.linalg.norm(cov_full @ v - v * w, axis=0) / np.abs(w)
        assert res.max() < 1e-8, res
    return check


@pytest.mark.parametrize("n,rows", FULL, ids=CONFIG_IDS[:2])
def test_pca_eigen(n, rows):
    k = 5
    with _ctx("PCA_COV", n, rows) as a:
        cov, _ = a.pca_cov(packed=False, normalize=True)
        check = _eigen_oracle(cov, k)
        vals = []

        def call(p):
            if p is None:
                w, v = a.pca_eigen(k)
                vals.append(w)
                return [np.ascontiguousarray(v.T)]
            w, v = a.pca_eigen(k, out_ptr=p[0])
            assert v is None
            vals.append(w)
        device_vs_host("pca_eigen", call, oracle=lambda r: check(vals[-1], r[0]))      # (the eigenvalues are host memory either way)


def _panels_topk(panels, n, k, scale, vec_ptr):
    from snprelate_amd import _lib
    w = np.empty(k, np.float64)
    v = np.empty((k, n), np.float64) if vec_ptr is None else None
    handles = (ctypes.c_void_p * len(panels))(*[p._h for p in panels])
    opts = _lib.EigOpts(tol=1e-9, block=0, depth=0, max_restarts=0, seed=20240601, y_buf=None, reduce=_lib.REDUCE_FN(), user=None,
                        fp32_until=0.0)
    info = _lib.EigInfo()
    _lib.check(_lib.lib().snpgpu_panels_topk_eigen(handles, len(panels), float(scale), k, ctypes.byref(opts), _lib._ptr(w),
                                                   _lib._ptr(v) if vec_ptr is None else ctypes.c_void_p(int(vec_ptr)),
                                                   _lib.HOST if vec_ptr is None else _lib.DEVICE, ctypes.byref(info)))
    assert info.max_rel_residual < 1e-8
    return w, v


def test_panels_topk_eigen():
    """snpgpu_panels_topk_eigen on the one panel of a full PCA_COV context of 279 samples: eigenvectors into device memory"""
    n, k = 279, 5
    with _ctx("PCA_COV", n, None) as a:
        cov, tr = a.pca_cov(packed=False, normalize=True)
        scale = (n - 1) / tr
        check = _eigen_oracle(cov, k)
        vals = []

        def call(p):
            w, v = _panels_topk([a], n, k, scale, None if p is None else p[0])
            vals.append(w)
            return [v]
        device_vs_host("panels_topk_eigen", call, oracle=lambda r: check(vals[-1], r[0]))


def test_select_pairs():
    """snpgpu_select_pairs with all five outputs in device memory, and with k0 / k1 NULL; capacity = all pairs found"""
    from snprelate_amd import _lib
    n = 279
    with _ctx("KING_HOMO", n, None) as a:
        found = a.select_pairs(_lib.SEL_KING_HOMO, cutoff=0.0)[5]
        assert 0 < found < n * (n - 1) // 2

        def call(p):
            if p is None:
                return list(a.select_pairs(_lib.SEL_KING_HOMO, cutoff=0.0, capacity=found)[:5])
            assert a.select_pairs(_lib.SEL_KING_HOMO, cutoff=0.0, capacity=found, out_ptrs=p)[5] == found
        device_vs_host("select_pairs", call, absent=((), (2, 3)))


# ---- several panels behind one object ----------------------------------------------------------------------------------------------------

MULTI_N = 600


def _multi(kind):
    from snprelate_amd import _lib
    m = _lib.MultiAccumulator(getattr(_lib, kind), MULTI_N, devices=(0, 0), panels_per_device=2, max_block_snps=512)
    g = _geno(MULTI_N)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        m.feed(g[lo:hi])
    m.sync()
    return m


@pytest.mark.parametrize("kind", ["IBS", "KING_ROBUST", "KING_HOMO", "DISS", "GRM_GCTA", "EIGMIX", "PCA_COV"])
def test_multi_gathers(kind):
    """every gather of snpgpu_multi_* into device memory of the first device: device 0 listed twice, two panels per entry asked for"""
    fam = (np.arange(MULTI_N) // 4).astype(np.int32)
    with _multi(kind) as m:
        assert m.info()["n_panels"] >= 2                        # (panels start at multiples of 256 rows: 600 samples give two)
        one = lambda f: (lambda p: [f()] if p is None else f(out_ptr=p[0]))      # noqa: E731
        if kind == "IBS":
            device_vs_host("multi ibs_num", lambda p: m.ibs_num(out_ptrs=p))
            device_vs_host("multi ibs_ave", one(m.ibs_ave))
        elif kind == "KING_ROBUST":
            device_vs_host("multi king_robust_counts", one(m.king_robust_counts))
            for f in (None, fam):
                device_vs_host("multi king_robust", lambda p: m.king_robust(family=f, out_ptrs=p))
        elif kind == "KING_HOMO":
            device_vs_host("multi king_homo", lambda p: m.king_homo(out_ptrs=p))
        elif kind == "DISS":
            device_vs_host("multi diss", one(m.diss))
        elif kind == "GRM_GCTA":
            device_vs_host("multi grm_gcta", one(m.grm_gcta))
        elif kind == "EIGMIX":
            for diagadj in (True, False):
                device_vs_host("multi eigmix", lambda p: [m.eigmix(diagadj, 2.0)] if p is None else m.eigmix(diagadj, 2.0, out_ptr=p[0]))
        else:
            for normalize in (True, False):
                device_vs_host("multi pca_cov", lambda p: [m.pca_cov(normalize=normalize, out_ptr=None if p is None else p[0])[0]])


def test_multi_topk_eigen():
    n, k = MULTI_N, 5
    with _multi("PCA_COV") as m:
        tri, _ = m.pca_cov(normalize=True)
        check = _eigen_oracle(orc.tri_to_full(tri, n), k)
        vals = []

        def call(p):
            w, v, info = m.topk_eigen(k, out_ptr=None if p is None else p[0])
            assert info["max_rel_residual"] < 1e-8
            vals.append(w)
            return None if v is None else [np.ascontiguousarray(v.T)]
        device_vs_host("multi topk_eigen", call, oracle=lambda r: check(vals[-1], r[0]))


# ---- LD ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["LD_COMPOSITE", "LD_R"])
@pytest.mark.parametrize("slide,trim", [(-1, False), (7, False), (7, True)])
def test_ld_result(method, slide, trim):
    from snprelate_amd import _lib
    n, L = 203, 300
    g = _geno(n, L, seed=31)
    with _lib.LDMatrix(n, L, method=getattr(_lib, method), slide=slide, mat_trim=trim, max_block_snps=128) as ld:
        ld.feed(g[:130])
        ld.feed(g[130:])
        assert ld.dims() == _lib.ld_out_dims(L, slide, trim)
        device_vs_host("ld_result", lambda p: [ld.result().T] if p is None else ld.result(out_ptr=p[0]))


# ---- IBD by maximum likelihood ---------------------------------------------------------------------------------------------------------------

IBD_N, IBD_L = 65, 1000


@functools.lru_cache(maxsize=None)
def _ibd_rows():
    return _packed(_geno(IBD_N, IBD_L, seed=65))


def _filled(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, M.FILL, np.uint8).view(dtype).reshape(shape)


@pytest.mark.parametrize("rows", [(0, 0), (0, 64)], ids=["whole", "rows0_64"])
def test_ibd_mle(rows):
    """k0, k1 and niter of snpgpu_ibd_mle in device memory; niter also NULL.  With a row range the entries outside it are left as they
    were: the host arrays start from the destination's fill pattern, so the comparison covers them, and untouched() says it again."""
    from snprelate_amd import _lib
    n = IBD_N
    pk = _ibd_rows()

    def call(p):
        if p is None:
            out = (_filled((n, n), np.float64), _filled((n, n), np.float64), _filled((n, n), np.int32))
            return list(_lib.ibd_mle(pk, n, max_niter=200, rows=rows, out=out)[:3])
        _lib.ibd_mle(pk, n, max_niter=200, rows=rows, out_ptrs=p)
    device_vs_host("ibd_mle rows=%s" % (rows,), call, absent=((), (2,)))
    if rows != (0, 0):
        # pairs (i, j > i) with i in the range, their mirrors, and the diagonal of those rows are written: here all but (64, 64)
        left = np.zeros((n, n), bool)
        left[rows[1]:, rows[1]:] = True
        assert left.sum() == 1
        for off in M.OFFSETS:
            d = [M.DeviceDest((n, n), t, off) for t in (np.float64, np.float64, np.int32)]
            _lib.ibd_mle(pk, n, max_niter=200, rows=rows, out_ptrs=[x.ptr for x in d])
            for x in d:
                x.read()
                x.untouched(left)


@pytest.mark.parametrize("form", ["matrices", "global_pair"])
def test_ibd_loglik(form):
    """the result in device memory; k0 / k1 are inputs in the result's memory kind: device matrices at misaligned addresses"""
    from snprelate_amd import _lib
    n = IBD_N
    pk = _ibd_rows()
    if form == "global_pair":
        device_vs_host("ibd_loglik global", lambda p: [_lib.ibd_loglik(pk, n, k0_all=0.25, k1_all=0.5)] if p is None
                       else _lib.ibd_loglik(pk, n, k0_all=0.25, k1_all=0.5, out_ptr=p[0]))
        return
    k0, k1 = _lib.ibd_mle(pk, n, max_niter=50)[:2]
    ins = {}
    for off in M.OFFSETS:
        ins[off] = (M.DeviceDest((n, n), np.float64, off), M.DeviceDest((n, n), np.float64, 4 - off))
        ins[off][0].put(k0)
        ins[off][1].put(k1)
    used = iter(M.OFFSETS)

    def call(p):
        if p is None:
            return [_lib.ibd_loglik(pk, n, k0=k0, k1=k1)]
        a, b = ins[next(used)]
        _lib.ibd_loglik(pk, n, k0=a.ptr, k1=b.ptr, out_ptr=p[0])
        assert _same(a.read(), k0) and _same(b.read(), k1)        # inputs: read only, guards intact
    device_vs_host("ibd_loglik matrices", call)


@functools.lru_cache(maxsize=None)
def _pair_list(n, n_pairs, seed=5):
    rng = np.random.default_rng(seed)
    i1 = rng.integers(0, n, n_pairs).astype(np.int32)
    i2 = rng.integers(0, n, n_pairs).astype(np.int32)
    i2[::9] = i1[::9]                                             # a sample with itself
    i1[-7:], i2[-7:] = i1[:7], i2[:7]                             # repeats
    return i1, i2


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ibd_mle_pairs(mode):
    from snprelate_amd import _lib
    i1, i2 = _pair_list(IBD_N, 130)
    pk = _ibd_rows()
    device_vs_host("ibd_mle_pairs mode %d" % mode,
                   lambda p: _lib.ibd_mle_pairs(pk, IBD_N, i1, i2, mode=mode, max_niter=200, out_ptrs=p)[:4] if p is None
                   else _lib.ibd_mle_pairs(pk, IBD_N, i1, i2, mode=mode, max_niter=200, out_ptrs=p),
                   absent=((), (2,), (3,), (2, 3)))


def test_ibd_jacquard_pairs():
    from snprelate_amd import _lib
    i1, i2 = _pair_list(IBD_N, 130)
    pk = _ibd_rows()
    device_vs_host("ibd_jacquard_pairs",
                   lambda p: _lib.ibd_jacquard_pairs(pk, IBD_N, i1, i2, max_niter=100, out_ptrs=p)[:3] if p is None
                   else _lib.ibd_jacquard_pairs(pk, IBD_N, i1, i2, max_niter=100, out_ptrs=p),
                   absent=((), (1,), (2,), (1, 2)))


# ---- QC and counting one-shots -----------------------------------------------------------------------------------------------------------------

QC_N, QC_L = 257, 203


def test_pop_counts():
    from snprelate_amd import _lib
    g = _geno(QC_N, QC_L, seed=7)
    pop = (np.arange(QC_N) % 3).astype(np.int32)
    for src in (g, _packed(g)):
        device_vs_host("pop_counts", lambda p: _lib.pop_counts(src, QC_N, pop, 3, out_ptrs=p))


def test_geno_counts():
    from snprelate_amd import _lib
    g = _geno(QC_N, QC_L, seed=7)
    device_vs_host("geno_counts", lambda p: _lib.geno_counts(g, QC_N, out_ptrs=p), absent=((), (0,), (1,)))


def test_hwe_counts():
    """the memory kind covers the counts and the p-values: counts in device memory (misaligned), p-values into device memory"""
    from snprelate_amd import _lib
    cnt, _ = _lib.geno_counts(_geno(QC_N, QC_L, seed=7), QC_N)
    ins = {off: M.DeviceDest(cnt.shape, np.int32, 4 - off) for off in M.OFFSETS}
    for d in ins.values():
        d.put(cnt)
    used = iter(M.OFFSETS)

    def call(p):
        if p is None:
            return [_lib.hwe_counts(cnt)]
        d = ins[next(used)]
        _lib.hwe_counts(d.ptr, n_snp=cnt.shape[0], out_ptr=p[0])
        assert _same(d.read(), cnt)
    device_vs_host("hwe_counts", call)


@pytest.mark.parametrize("method", ["mom.weir", "mle"])
def test_ind_inb(method):
    from snprelate_amd import _lib
    g = _geno(QC_N, QC_L, seed=7)

    def call(p):
        if p is None:
            coeff, nit, _ = _lib.ind_inb(g, QC_N, method=method)
            return [coeff] if nit is None else [coeff, nit]
        _lib.ind_inb(g, QC_N, method=method, out_ptrs=list(p) + [None] * (2 - len(p)))
    device_vs_host("ind_inb %s" % method, call, absent=((), (1,)) if method == "mle" else ((),))


@pytest.mark.parametrize("need_major", [0, 1])
def test_pair_tables(need_major):
    """all three tables and every proper subset of them in device memory (int64, int32 and byte results)"""
    from snprelate_amd import _lib
    n, L = 130, 255
    g = _geno(n, L, seed=13)
    i1, i2 = _pair_list(n, 70, seed=9)
    device_vs_host("pair_tables need_major=%d" % need_major,
                   lambda p: _lib.pair_tables(g, n, i1, i2, need_major=need_major, out_ptrs=p),
                   absent=((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2)))


def test_geno_select_convert():
    """the dst_mem calls: a sample subset as 2-bit rows, and the same rectangle recoded to BED with the samples as rows"""
    from snprelate_amd import _lib
    n, L = 203, 300
    pk = _packed(_geno(n, L, seed=31))
    rb = pk.shape[1]
    samp = np.random.default_rng(2).permutation(n)[:101].astype(np.int32)
    snp = np.arange(L - 1, 10, -2).astype(np.int32)
    device_vs_host("geno_select", lambda p: [_lib.geno_select(pk, 0, L, n, row_stride_bits=8 * rb, samp_index=samp, snp_index=snp)]
                   if p is None else _lib.geno_select(pk, 0, L, n, row_stride_bits=8 * rb, samp_index=samp, snp_index=snp, out=p[0]))
    kw = dict(src_code=_lib.CODE_GDS, dst_code=_lib.CODE_BED, dst_major=1, row_stride_bits=8 * rb, samp_index=samp, snp_index=snp)
    device_vs_host("geno_convert", lambda p: [_lib.geno_convert(pk, 0, L, n, **kw)] if p is None
                   else _lib.geno_convert(pk, 0, L, n, out=p[0], **kw))


# ---- the projector -------------------------------------------------------------------------------------------------------------------------------

PROJ_N, PROJ_L, PROJ_K = 333, 1500, 11
PROJ_CUTS = [0, 100, 164, 677, 1500]


@functools.lru_cache(maxsize=None)
def _proj_data():
    """the data of test_projector_vs_oracle_synthetic (tests/test_gpu_api_golden.py)"""
    n, L, k = PROJ_N, PROJ_L, PROJ_K
    g = synth_geno(n, L, missing=0.06, seed=91)
    g[7] = 3
    g[8] = 2
    g[9, 5:] = 3
    g[10, 1:] = 3
    ev = np.random.default_rng(4).normal(size=(k, n))
    ev[3] = 1.0
    w = np.linspace(3.0, 0.5, k)
    tr = 123.4
    evs = ev * np.sqrt((n - 1) / tr / w)[:, None]
    return g, ev, w, tr, evs


def _dev(array):
    """(tensor, address) of a numpy array in device memory, complete"""
    import torch
    a = np.ascontiguousarray(array)
    t = torch.from_numpy(a.reshape(-1).view(np.uint8)).cuda()
    torch.cuda.current_stream().synchronize()
    return t, int(t.data_ptr())


def test_projector_device():
    """device eigenvectors, device blocks, device results of snp_corr, snp_loading and snp_loading_ext (device avg / scale), and
    geno=None = the staged block.  Device block in, device result out: stream-ordered, so sync() comes before read()."""
    from snprelate_amd import _lib
    g, ev, w, tr, evs = _proj_data()
    n, k = PROJ_N, PROJ_K
    spans = list(zip(PROJ_CUTS[:-1], PROJ_CUTS[1:]))
    ref_corr = orc.pca_snp_corr(g, ev)

    def close(got, ref, rtol, atol):
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, equal_nan=True)

    with _lib.Projector(n, k, max_block_snps=1024) as p:
        keep_ev, ev_ptr = _dev(ev)
        p.set_eigvec(ev_ptr)                                     # device eigenvectors (stream-ordered; the calls below order after it)
        for a, b in spans:
            blk_t, blk = _dev(g[a:b])
            device_vs_host("snp_corr", lambda q: [p.snp_corr(g[a:b])] if q is None
                           else p.snp_corr(blk, n_snp=b - a, fmt=_lib.GENO_U8, out_ptr=q[0]),
                           oracle=lambda r: close(r[0], ref_corr[a:b], 1e-9, 1e-12), after=p.sync)
            # the staged block again: the same result without handing the block over
            device_vs_host("snp_corr, staged block", lambda q: [p.snp_corr(None)] if q is None else p.snp_corr(None, out_ptr=q[0]),
                           oracle=lambda r: close(r[0], ref_corr[a:b], 1e-9, 1e-12), after=p.sync)
        for bayes in (False, True):
            keep_evs, evs_ptr = _dev(evs)
            p.set_eigvec(evs_ptr)
            rl, ra, rs = orc.pca_snp_loading(g, w, ev, tr, bayesian=bayes)
            xl, _, _, xb = proj_ref.snp_loading(g, evs, bayes)       # in long double, with the bound of fp64 summation in any order

            def oracle(r, a, b):
                np.testing.assert_allclose(r[0], rl[a:b], rtol=1e-10, atol=1e-12)
                assert (np.abs(r[0] - xl[a:b]) <= xb[a:b]).all()
                if r[1] is not None:
                    np.testing.assert_allclose(r[1], ra[a:b], rtol=1e-14)
                if r[2] is not None:
                    np.testing.assert_allclose(r[2], rs[a:b], rtol=1e-14)
            for a, b in spans:
                blk_t, blk = _dev(_packed(g[a:b]))
                device_vs_host("snp_loading", lambda q: list(p.snp_loading(g[a:b], bayesian=bayes)) if q is None
                               else p.snp_loading(blk, bayesian=bayes, n_snp=b - a, out_ptrs=q),
                               oracle=lambda r: oracle(r, a, b), after=p.sync, absent=((), (1, 2)))
                device_vs_host("snp_loading, staged block", lambda q: p.snp_loading(None, bayesian=bayes, out_ptrs=q),
                               oracle=lambda r: oracle(r, a, b), after=p.sync)
        # the caller's centring and scaling, in device memory at misaligned addresses
        keep_ev2, ev_ptr2 = _dev(ev)
        p.set_eigvec(ev_ptr2)
        avg = np.linspace(0.2, 1.7, PROJ_L)
        sc = np.linspace(2.0, 0.3, PROJ_L)
        z = np.where(g < 3, (g.astype(np.float64) - avg[:, None]) * sc[:, None], 0.0)
        ref_ext = z @ ev.T
        for a, b in spans:
            blk_t, blk = _dev(_packed(g[a:b]))
            d_avg, d_sc = M.DeviceDest((b - a,), np.float64, 1), M.DeviceDest((b - a,), np.float64, 3)
            d_avg.put(avg[a:b])
            d_sc.put(sc[a:b])
            device_vs_host("snp_loading_ext", lambda q: [p.snp_loading_ext(g[a:b], avg[a:b], sc[a:b])] if q is None
                           else p.snp_loading_ext(blk, d_avg.ptr, d_sc.ptr, n_snp=b - a, out_ptr=q[0]),
                           oracle=lambda r: np.testing.assert_allclose(r[0], ref_ext[a:b], rtol=1e-10, atol=1e-11), after=p.sync)
            assert _same(d_avg.read(), avg[a:b]) and _same(d_sc.read(), sc[a:b])


def test_projector_samp_loading():
    """device sload / afreq / scale into samp_loading_feed, the sums into device memory, and what snpgpu.h says of the accumulator:
    samp_loading only reads it (a second read has the same bytes, a block fed afterwards adds to the same sums) and reset() makes the
    next accumulation a fresh projector's."""
    from snprelate_amd import _lib
    g, ev, w, tr, evs = _proj_data()
    n, k = PROJ_N, PROJ_K
    spans = list(zip(PROJ_CUTS[:-1], PROJ_CUTS[1:]))
    rl, ra, rs = orc.pca_snp_loading(g, w, ev, tr, bayesian=False)
    sload = rl * 0.37
    ref = orc.pca_samp_loading(g, sload, ra, rs)
    cut = PROJ_CUTS[2]
    ref_head = orc.pca_samp_loading(g[:cut], sload[:cut], ra[:cut], rs[:cut])
    tol = dict(rtol=1e-10, atol=1e-11)

    def feed(p, a, b, device):
        if not device:
            p.samp_loading_feed(g[a:b], sload[a:b], ra[a:b], rs[a:b])
            return
        blk_t, blk = _dev(_packed(g[a:b]))
        ds = [M.DeviceDest(x[a:b].shape, np.float64, o) for x, o in ((sload, 1), (ra, 3), (rs, 1))]
        for d, x in zip(ds, (sload, ra, rs)):
            d.put(x[a:b])
        p.samp_loading_feed(blk, ds[0].ptr, ds[1].ptr, ds[2].ptr, n_snp=b - a)      # all device: stream-ordered
        p.sync()                                                                      # (the inputs go away with this frame)
        for d, x in zip(ds, (sload, ra, rs)):
            assert _same(d.read(), x[a:b])

    with _lib.Projector(n, k, max_block_snps=1024) as p:
        for a, b in spans[:2]:
            feed(p, a, b, device=True)
        # reading leaves the sums as they are: twice the same bytes (device_vs_host's two host calls), in device memory too
        head = device_vs_host("samp_loading after two blocks", lambda q: [p.samp_loading()] if q is None else p.samp_loading(out_ptr=q[0]),
                              oracle=lambda r: np.testing.assert_allclose(r[0], ref_head, **tol))[0]
        assert _same(head, p.samp_loading())
        for a, b in spans[2:]:
            feed(p, a, b, device=True)                           # ... and feeding goes on adding to them
        device_vs_host("samp_loading", lambda q: [p.samp_loading()] if q is None else p.samp_loading(out_ptr=q[0]),
                       oracle=lambda r: np.testing.assert_allclose(r[0], ref, **tol))
        # reset(), then a second accumulation: a fresh projector's
        p.reset()
        assert not p.samp_loading().any()
        for a, b in spans:
            feed(p, a, b, device=False)
        np.testing.assert_allclose(p.samp_loading(), ref, **tol)
        # a staged block fed again without handing it over adds that block once more
        p.reset()
        a, b = spans[1]
        feed(p, a, b, device=False)
        one = p.samp_loading()
        ds = [M.DeviceDest(x[a:b].shape, np.float64, 1) for x in (sload, ra, rs)]
        for d, x in zip(ds, (sload, ra, rs)):
            d.put(x[a:b])
        p.samp_loading_feed(None, ds[0].ptr, ds[1].ptr, ds[2].ptr)
        p.sync()
        np.testing.assert_allclose(p.samp_loading(), 2 * one, **tol)
