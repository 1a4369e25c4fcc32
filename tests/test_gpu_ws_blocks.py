"""The block loop of the genotype working space (csrc/workspace.hip, ws_for_each_block): offsets and lengths at the 8192-SNP block
boundaries, under an identity selection and under a snpgpu_ws_sel_snp_base filter that leaves the selected rows non-contiguous.
37 samples (not a multiple of 4: every 2-bit row ends in padding codes), 2 % missing calls, monomorphic and all-missing SNPs at the
start of the pool and around the first block boundary; the per-block calls that index a caller's per-SNP vectors (the PCA and the
EIGMIX loadings, both directions) get vectors that differ from SNP to SNP.  Everything is compared with numpy or with the oracle functions of the
golden tests; the per-SNP references are computed once for the whole pool and indexed by the selected rows."""
import ctypes

import numpy as np
import pytest

import oracle as orc
from conftest import synth_geno

pytestmark = pytest.mark.gpu

N_SAMP, POOL, K = 37, 16385, 3
EIGVAL, TRACE = np.array([3.0, 1.7, 0.5]), 123.4
# (selected SNPs, through the filter): one SNP, one short of a block, a block, a block and one SNP, two blocks and one SNP
CASES = [(1, False), (8191, False), (8192, False), (8193, False), (8193, True), (16385, False)]


@pytest.fixture(scope="module")
def pool():
    from snprelate_amd.gds import pack_2bit_rows
    g = synth_geno(N_SAMP, POOL, missing=0.02, seed=37)      # plants monomorphic / all-missing SNPs at rows 3, 5, 7, 11
    g[8189] = 0
    g[8191] = 3
    g[8194] = 2
    g[16380] = 3
    valid = g < 3
    num = valid.sum(axis=1).astype(np.int64)
    tot = np.where(valid, g, 0).sum(axis=1).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        af = np.where(num > 0, tot / (2 * num), np.nan)
        maf = np.minimum(af, 1 - af)
    mr = 1 - num / N_SAMP
    ev = np.random.default_rng(5).normal(size=(K, N_SAMP))
    load, avg, scale = orc.pca_snp_loading(g, EIGVAL, ev, TRACE)
    return dict(g=g, packed=np.ascontiguousarray(pack_2bit_rows(g)), af=af, maf=maf, mr=mr, keep=(num > 0) & (maf > 0), ev=ev,
                eigmix_af=np.where(np.isnan(af), 0.5, af),
                corr=orc.pca_snp_corr(g, ev), load=load, avg=avg, scale=scale)


@pytest.mark.parametrize("n_sel,filtered", CASES, ids=["%d%s" % (n, "-filtered" if f else "") for n, f in CASES])
def test_ws_block_boundaries(pool, n_sel, filtered):
    from snprelate_amd import _lib
    L, p = _lib.lib(), _lib._ptr
    if filtered:     # the shortest prefix of the pool that keeps n_sel SNPs
        n_in = int(np.searchsorted(np.cumsum(pool["keep"]), n_sel)) + 1
        idx = np.flatnonzero(pool["keep"][:n_in])
        assert n_in - n_sel >= 5 and (np.diff(idx) > 1).any()      # at least the planted rows 3, 5, 7, 8189, 8191 are dropped
    else:
        n_in, idx = n_sel, np.arange(n_sel)
    g = pool["g"][idx]
    _lib.check(L.snpgpu_ws_set_geno(p(pool["packed"]), n_in, N_SAMP, _lib.GENO_PACKED2, 0))
    try:
        if filtered:
            flags, nex = np.zeros(n_in, np.uint8), ctypes.c_int32(0)
            _lib.check(L.snpgpu_ws_sel_snp_base(1, -1.0, 2.0, ctypes.byref(nex), p(flags)))
            assert np.array_equal(flags.astype(bool), pool["keep"][:n_in]) and nex.value == n_in - n_sel
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(L.snpgpu_ws_get_geno_dim(ctypes.byref(a), ctypes.byref(b)))
        assert (a.value, b.value) == (n_sel, N_SAMP)

        ibs = [np.empty((N_SAMP, N_SAMP), np.int32) for _ in range(3)]
        _lib.check(L.snpgpu_gnrIBSNum(1, 0, *[p(x) for x in ibs]))
        cnt = orc.ibs_count(g)
        for k in range(3):
            assert np.array_equal(ibs[k], orc.tri_to_full(cnt[:, k].astype(np.int32), N_SAMP)), "ibs%d" % k

        af, maf, mr = (np.empty(n_sel, np.float64) for _ in range(3))
        _lib.check(L.snpgpu_ws_snp_rate_freq(p(af), p(maf), p(mr)))
        assert np.array_equal(af, pool["af"][idx], equal_nan=True)
        assert np.array_equal(maf, pool["maf"][idx], equal_nan=True)
        assert np.array_equal(mr, pool["mr"][idx])

        ev = pool["ev"]
        corr = np.empty((n_sel, K), np.float64)
        _lib.check(L.snpgpu_gnrPCACorr(K, p(ev), 1, 0, p(corr)))
        ref = pool["corr"][idx]
        assert np.array_equal(np.isnan(corr), np.isnan(ref))
        np.testing.assert_allclose(corr, ref, rtol=1e-9, atol=1e-12, equal_nan=True)

        load, avg, scale = np.empty((n_sel, K), np.float64), np.empty(n_sel, np.float64), np.empty(n_sel, np.float64)
        _lib.check(L.snpgpu_gnrPCASNPLoading(p(EIGVAL), p(ev), K, TRACE, 1, 0, 0, p(load), p(avg), p(scale)))
        np.testing.assert_allclose(avg, pool["avg"][idx], rtol=1e-14)
        np.testing.assert_allclose(scale, pool["scale"][idx], rtol=1e-14)
        np.testing.assert_allclose(load, pool["load"][idx], rtol=1e-10, atol=1e-12)

        sload = np.ascontiguousarray(pool["load"][idx] * 0.37)
        ra, rs = np.ascontiguousarray(pool["avg"][idx]), np.ascontiguousarray(pool["scale"][idx])
        got = np.empty((K, N_SAMP), np.float64)
        _lib.check(L.snpgpu_gnrPCASampLoading(K, p(sload), p(ra), p(rs), 1, 0, p(got)))
        np.testing.assert_allclose(got, orc.pca_samp_loading(g, sload, ra, rs), rtol=1e-10, atol=1e-11)

        # the EIGMIX twins hand avg + i0 and scale + i0 of their own vectors to every block
        eaf = np.ascontiguousarray(pool["eigmix_af"][idx])
        assert 0 < eaf[0] < 1                                    # (the one-SNP case has a finite scale)
        eload = np.empty((n_sel, K), np.float64)
        _lib.check(L.snpgpu_gnrEigMixSNPLoading(p(EIGVAL), p(ev), K, p(eaf), 1, 0, p(eload)))
        np.testing.assert_allclose(eload, orc.eigmix_snp_loading(g, EIGVAL, ev, eaf), rtol=1e-10, atol=1e-12)
        got = np.empty((K, N_SAMP), np.float64)
        _lib.check(L.snpgpu_gnrEigMixSampLoading(K, p(sload), p(eaf), 1, 0, p(got)))
        np.testing.assert_allclose(got, orc.eigmix_samp_loading(g, sload, eaf), rtol=1e-10, atol=1e-11)
    finally:
        L.snpgpu_ws_clear()
