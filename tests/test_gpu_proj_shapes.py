"""The PCA projection kernels (csrc/kernels_proj.hip behind csrc/proj.hip) entry by entry at every boundary of their launch geometry:
the case table of tests/proj_cases.py, whose geometry tests/test_cpu_proj_grid.py pins on the CPU.  Loadings and sample loadings are
held to the extended-precision references of tests/proj_ref.py at their bound B (a rounding-error bound of fp64 summation in any
order: a term accumulated in fp32 is about 2^29 / n_terms bounds away); correlations to oracle.pca_snp_corr at the project's tolerance
with the same NaN pattern, on inputs that leave no entry at the formula's val > 0 edge.  Every test prints the largest |got - ref| / B
it saw ("ratio ..."), per kernel."""
import functools

import numpy as np
import pytest

import oracle as orc
import proj_cases as pc
import proj_ref as pr

pytestmark = pytest.mark.gpu


def within(what, got, ref, bound):
    """|got - ref| <= bound entry by entry (0 <= 0 where every term is zero); prints the largest ratio"""
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("ratio %s %.3f" % (what, ratio.max()))
    assert (err <= bound).all(), "%s: |got - ref| / B up to %g at %s" % (what, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


def corr_close(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12, equal_nan=True)


@functools.lru_cache(maxsize=None)
def snp_refs(N, n_snp, k):
    """the SNP-side references of one shape, computed once: correlations, plain and Bayesian loadings, loadings under the caller's
    centring and scaling"""
    g, ev, _ = pc.inputs(N, n_snp, k)
    evs = pr.pca_eigvec_scaled(pc.eigenvalues(k), ev, pc.TRACE)
    corr = orc.pca_snp_corr(g, ev)
    degenerate, margin = pr.corr_margin(g, ev)
    # no entry is excluded: NaN comes from exactly representable constants only, every other entry is clear of the val > 0 edge
    assert np.array_equal(np.isnan(corr), degenerate) and margin.min() >= 1e-6, margin.min()
    avg, scale = np.linspace(0.2, 1.7, n_snp), np.linspace(2.0, 0.3, n_snp)
    return dict(g=g, ev=ev, evs=evs, corr=corr, load=[pr.snp_loading(g, evs, bayes) for bayes in (False, True)], avg=avg, scale=scale,
                ext=pr.snp_loading(g, ev, avg=avg, scale=scale))


@functools.lru_cache(maxsize=None)
def samp_refs(N, n_snp, k):
    g, _, sload = pc.inputs(N, n_snp, k)
    avg, scale = (np.asarray(x, np.float64) for x in pr.snp_stats(g))
    return dict(g=g, sload=sload, avg=avg, scale=scale, ref=pr.samp_loading(g, sload, avg, scale))


@pytest.mark.parametrize("case", pc.SNP_CASES, ids=[c.name for c in pc.SNP_CASES])
def test_snp_side(case):
    from snprelate_amd import _lib
    r = snp_refs(case.N, case.n_snp, case.k)
    g = r["g"]
    with _lib.Projector(case.N, case.k, max_block_snps=case.bmax) as p:
        p.set_eigvec(r["ev"])
        corr_close(p.snp_corr(g), r["corr"])
        within("LOAD ext " + case.name, p.snp_loading_ext(g, r["avg"], r["scale"]), r["ext"][0], r["ext"][3])
        p.set_eigvec(r["evs"])
        for bayes in (False, True):
            load, avg, scale = p.snp_loading(g, bayesian=bayes)
            ref, ra, rs, bound = r["load"][bayes]
            np.testing.assert_allclose(avg, ra, rtol=1e-14)
            np.testing.assert_allclose(scale, rs, rtol=1e-14)
            within("LOAD %s %s" % ("bayes" if bayes else "plain", case.name), load, ref, bound)


@pytest.mark.parametrize("case", pc.SAMP_CASES, ids=[c.name for c in pc.SAMP_CASES])
def test_samp_side(case):
    from snprelate_amd import _lib
    r = samp_refs(case.N, case.n_snp, case.k)
    with _lib.Projector(case.N, case.k, max_block_snps=case.bmax) as p:
        p.samp_loading_feed(r["g"], r["sload"], r["avg"], r["scale"])
        within("SAMP " + case.name, p.samp_loading(), *r["ref"])


def test_block_above_max_block_snps_is_refused():
    from snprelate_amd import _lib
    g, ev, _ = pc.inputs(333, 1025, 11)
    assert pr.corr_margin(g[:1024], ev)[1].min() >= 1e-6
    with _lib.Projector(333, 11, max_block_snps=1024) as p:
        p.set_eigvec(ev)
        with pytest.raises(_lib.SnpGpuError, match=r"snpgpu_proj: invalid block \(empty or larger than max_block_snps\)"):
            p.snp_corr(g)
        corr_close(p.snp_corr(g[:1024]), orc.pca_snp_corr(g[:1024], ev))       # ... and the projector goes on working


# ---- staging: a block handed over once serves both sides ----------------------------------------------------------------------------

def test_words_are_built_late_for_a_block_staged_without_them():
    """samp_loading_feed stages the packed rows only; snp_corr(None) and snp_loading(None) then build the sample-major words from
    them.  Two sample parts add into zeroed sums, and x + y = y + x: the results equal those of the calls given the block bit for bit."""
    from snprelate_amd import _lib
    N, L, k = pc.STAGE_N, pc.STAGE_L, pc.STAGE_K
    r, s = snp_refs(N, L, k), samp_refs(N, L, k)
    with _lib.Projector(N, k, max_block_snps=1024) as p:
        p.set_eigvec(r["ev"])
        corr = p.snp_corr(r["g"])
        p.set_eigvec(r["evs"])
        load, avg, scale = p.snp_loading(r["g"])
    with _lib.Projector(N, k, max_block_snps=1024) as p:
        p.set_eigvec(r["ev"])
        p.samp_loading_feed(s["g"], s["sload"], s["avg"], s["scale"])
        late_corr = p.snp_corr(None)
        p.samp_loading_feed(s["g"], s["sload"], s["avg"], s["scale"])         # staged without the words once more
        p.set_eigvec(r["evs"])
        late_load, late_avg, late_scale = p.snp_loading(None)
        again = p.snp_loading(None)[0]                                        # (the words are there now)
    assert np.array_equal(late_corr, corr, equal_nan=True) and np.array_equal(late_load, load) and np.array_equal(again, load)
    assert np.array_equal(late_avg, avg) and np.array_equal(late_scale, scale)
    corr_close(late_corr, r["corr"])
    within("LOAD plain staged late", late_load, r["load"][0][0], r["load"][0][3])


def test_a_block_staged_with_words_feeds_the_sample_side_once():
    from snprelate_amd import _lib
    N, L, k = pc.STAGE_N, pc.STAGE_L, pc.STAGE_K
    r, s = snp_refs(N, L, k), samp_refs(N, L, k)
    with _lib.Projector(N, k, max_block_snps=1024) as p:
        p.set_eigvec(r["ev"])
        corr_close(p.snp_corr(r["g"]), r["corr"])
        p.samp_loading_feed(None, s["sload"], s["avg"], s["scale"])
        within("SAMP staged block", p.samp_loading(), *s["ref"])
        p.samp_loading_feed(None, s["sload"], s["avg"], s["scale"])
        within("SAMP staged block twice", p.samp_loading(), 2 * s["ref"][0], 2 * s["ref"][1])


def test_a_staged_block_of_another_size_is_refused():
    from snprelate_amd import _lib
    N, L, k = pc.STAGE_N, pc.STAGE_L, pc.STAGE_K
    r, s = snp_refs(N, L, k), samp_refs(N, L, k)
    with _lib.Projector(N, k, max_block_snps=1024) as p:
        p.set_eigvec(r["ev"])
        for call in (lambda n: p.snp_corr(None, n_snp=n), lambda n: p.snp_loading(None, n_snp=n),
                     lambda n: p.samp_loading_feed(None, s["sload"][:n], s["avg"][:n], s["scale"][:n], n_snp=n)):
            with pytest.raises(_lib.SnpGpuError, match="snpgpu_proj: no staged block of this size to reuse"):
                call(L)                                                       # nothing staged yet
        p.snp_corr(r["g"])
        for call in (lambda n: p.snp_corr(None, n_snp=n), lambda n: p.snp_loading(None, n_snp=n),
                     lambda n: p.samp_loading_feed(None, s["sload"][:n], s["avg"][:n], s["scale"][:n], n_snp=n)):
            with pytest.raises(_lib.SnpGpuError, match="snpgpu_proj: no staged block of this size to reuse"):
                call(L - 1)
        corr_close(p.snp_corr(None), r["corr"])                               # the staged block is still there
        assert not p.samp_loading().any()                                     # ... and no refused feed added anything


# ---- the default user path: 32 eigenvectors, four SNP-side column passes, two on the sample side ------------------------------------

def test_api_default_eigen_cnt():
    from snprelate_amd import api, gds
    from test_gpu_api_golden import _structured_geno
    n, L, k = 300, 2000, 32
    gs = _structured_geno(n, L, seed=41)
    f = gds.GenoFile(genotype=gs)
    pca = api.snpgdsPCA(f, autosome_only=False, remove_monosnp=True, missing_rate=float("nan"), verbose=False)
    assert pca["eigenvect"].shape == (n, k) and (pca["eigenval"][:k] > 0).all()
    load = api.snpgdsPCASNPLoading(pca, f, verbose=False)
    g = f.read_genotype(snp_sel=np.isin(f.snp_id, pca["snp_id"]))
    assert load["snploading"].shape == (k, g.shape[0])
    ref, ra, rs, bound = pr.snp_loading(g, pr.pca_eigvec_scaled(pca["eigenval"][:k], pca["eigenvect"].T, pca["TraceXTX"]))
    np.testing.assert_allclose(load["avgfreq"], ra, rtol=1e-14)
    np.testing.assert_allclose(load["scale"], rs, rtol=1e-14)
    within("LOAD plain api", np.ascontiguousarray(load["snploading"].T), ref, bound)
    sl = api.snpgdsPCASampLoading(load, f, verbose=False)
    assert sl["eigenvect"].shape == (n, k)
    # the operands as snpgdsPCASampLoading forms them (R/PCA.R:281-285), then the kernel's sum
    sload = np.ascontiguousarray((load["snploading"] * np.sqrt((n - 1) / pca["TraceXTX"] / pca["eigenval"][:k])[:, None]).T)
    within("SAMP api", np.ascontiguousarray(sl["eigenvect"].T), *pr.samp_loading(g, sload, load["avgfreq"], load["scale"]))
    # projecting the analysis' own samples gives back their eigenvectors (to the accuracy of the covariance)
    print("own samples: max |projected - eigenvect| %.3g" % np.abs(sl["eigenvect"] - pca["eigenvect"]).max())
    np.testing.assert_allclose(sl["eigenvect"], pca["eigenvect"], atol=2e-5, rtol=0)
