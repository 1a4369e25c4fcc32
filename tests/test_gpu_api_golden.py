"""The reference's own golden-vector tests (inst/unitTests/test_rel.R) re-run through the
Python mirror of the R API on the MI355X path, plus the reference's GRM self-consistency
test (inst/unitTests/test_GRM.R) and API error behaviour."""
import os

import numpy as np
import pytest

import oracle as orc
import proj_ref
from conftest import GOLDEN, synth_geno

pytestmark = pytest.mark.gpu


def _tri_full(tri, n):
    return orc.tri_to_full(tri, n)


def test_IBS_golden(hapmap):
    """test.IBS, test_rel.R:97-124"""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_ibs.npz"))
    sid = hapmap.sample_id[:90]
    r = api.snpgdsIBS(hapmap, sample_id=sid, missing_rate=float("nan"), num_thread=1, verbose=False)
    assert np.array_equal(r["snp_id"], z["snp_id"])
    assert np.array_equal(r["sample_id"], z["sample_id"])
    assert np.array_equal(r["ibs"], z["ibs"])                      # bit-for-bit (checkEquals is 1.5e-8)
    r2 = api.snpgdsIBS(hapmap, sample_id=sid, missing_rate=float("nan"), num_thread=1, useMatrix=True,
                       verbose=False)
    assert np.array_equal(_tri_full(r2["ibs"], 90), z["ibs"])
    r3 = api.snpgdsIBS(hapmap, sample_id=sid, missing_rate=float("nan"), num_thread=2, verbose=False)
    assert np.array_equal(r3["ibs"], z["ibs"])


def test_IBSNum_known_answers(hapmap):
    from snprelate_amd import api
    r = api.snpgdsIBSNum(hapmap, sample_id=hapmap.sample_id[:90], missing_rate=float("nan"), verbose=False)
    # pairs (1,2), (1,1), (6,78) in R's 1-based numbering
    assert (r["ibs0"][0, 1], r["ibs1"][0, 1], r["ibs2"][0, 1]) == (447, 3160, 5050)
    assert (r["ibs0"][0, 0], r["ibs1"][0, 0], r["ibs2"][0, 0]) == (0, 0, 8668)
    assert (r["ibs0"][5, 77], r["ibs1"][5, 77], r["ibs2"][5, 77]) == (687, 2921, 5051)
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(r[k], r[k].T)


def test_KING_golden(hapmap):
    """test.KING, test_rel.R:228-273"""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_king.npz"))
    sid = hapmap.sample_id[:60]
    r = api.snpgdsIBDKING(hapmap, sample_id=sid, missing_rate=float("nan"), type="KING-robust",
                          num_thread=1, verbose=False)
    assert np.array_equal(r["snp_id"], z["snp_id"])
    assert np.array_equal(r["IBS0"], z["robust_IBS0"])
    assert np.array_equal(r["kinship"], z["robust_kinship"])
    rm = api.snpgdsIBDKING(hapmap, sample_id=sid, missing_rate=float("nan"), type="KING-robust",
                           useMatrix=True, verbose=False)
    assert np.array_equal(_tri_full(rm["kinship"], 60), z["robust_kinship"])
    h = api.snpgdsIBDKING(hapmap, sample_id=sid, missing_rate=float("nan"), type="KING-homo", verbose=False)
    # fp32 MFMA partial sums promoted to fp64: within 1e-5 relative (checkEquals' 1.5e-8 is for fp64)
    np.testing.assert_allclose(h["k0"], z["homo_k0"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(h["k1"], z["homo_k1"], rtol=1e-5, atol=2e-5)


def test_PCA_genmat_golden(hapmap):
    """test.PCA genmat, test_rel.R:128-142"""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_pca.npz"))
    r = api.snpgdsPCA(hapmap, sample_id=hapmap.sample_id[:90], need_genmat=True, eigen_cnt=8,
                      missing_rate=float("nan"), verbose=False)
    scale = np.abs(z["genmat"]).mean()
    assert np.max(np.abs(r["genmat"] - z["genmat"]) / (np.abs(z["genmat"]) + scale)) < 1e-5
    # eigen-decomposition of the golden matrix (LAPACK here = numpy) vs the device solver
    w, v = np.linalg.eigh(z["genmat"])
    w, v = w[::-1][:8], v[:, ::-1][:, :8]
    np.testing.assert_allclose(r["eigenval"][:8], w, rtol=1e-5)
    assert np.all(np.isnan(r["eigenval"][8:]))
    cos = np.abs(np.sum(r["eigenvect"] * v, axis=0))
    assert np.all(cos > 1 - 1e-6)
    np.testing.assert_allclose(r["varprop"][:8], w / 89.0, rtol=1e-5)
    assert r["eigenvect"].shape == (90, 8)


def test_PCA_randomized_pinned_by_the_exact_pca_golden(hapmap):
    """snpgdsPCA(algorithm = "randomized", iter.num = 10) on the call whose exact PCA the reference pins
    (Validate.PCA.RData$genmat, HapMap's first 90 samples): the device path (one pass per iteration, QR basis) returns that
    matrix's top-4 eigenpairs -- subspace within 1e-3 rad, eigenvalues within 1e-6 (the CPU restatement: tests/test_oracle_golden.py)."""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_pca.npz"))
    n, k = 90, 4
    w, v = np.linalg.eigh(z["genmat"])
    w, v = w[::-1][:k], v[:, ::-1][:, :k]
    aux = np.random.default_rng(2024).normal(size=(2 * k, n))
    r = api.snpgdsPCA(hapmap, sample_id=hapmap.sample_id[:n], missing_rate=float("nan"), algorithm="randomized", eigen_cnt=k,
                      aux_dim=2 * k, iter_num=10, aux_mat=aux, verbose=False)
    np.testing.assert_allclose(r["eigenval"][:k], w, rtol=1e-6)
    qa, qb = np.linalg.qr(r["eigenvect"][:, :k])[0], v
    ang = np.arccos(np.clip(np.linalg.svd(qa.T @ qb, compute_uv=False), -1.0, 1.0))
    assert ang.max() < 1e-3, ang
    np.testing.assert_allclose(r["varprop"][:k], w / (n - 1.0), rtol=1e-6)


def _sign_fix(got, gold, axis):
    s = np.sign(np.nansum(got * gold, axis=axis, keepdims=True))
    s[s == 0] = 1
    return got * s


def test_PCA_projections_golden(hapmap, tmp_path):
    """inst/unitTests/test_rel.R:128-160 (test.PCA): snpgdsPCACorr, snpgdsPCASNPLoading and
    snpgdsPCASampLoading against Validate.PCA.RData (rounded to 3 / 3 / 4 decimals by the reference;
    eigenvectors are defined up to sign)."""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_pca.npz"))
    pca = api.snpgdsPCA(hapmap, sample_id=hapmap.sample_id[:90], missing_rate=float("nan"), need_genmat=True,
                        eigen_cnt=8, verbose=False)
    corr = api.snpgdsPCACorr(pca, hapmap, eig_which=[1, 2], verbose=False)["snpcorr"]
    assert corr.shape == (2, 9088)
    assert np.array_equal(np.isnan(corr), np.isnan(z["corr"]))
    # half a unit of the reference's rounding + the 1e-5 relative tolerance of the covariance the
    # eigenvectors come from
    assert np.nanmax(np.abs(_sign_fix(corr, z["corr"], 1) - z["corr"])) < 5.01e-4
    # the outgds leg (test_rel.R:148-152): the stored packedreal16 node reads back as round(corr, 4)
    from snprelate_amd import gds
    fn = str(tmp_path / "test.gds")
    assert api.snpgdsPCACorr(pca, hapmap, eig_which=[1, 2], outgds=fn, verbose=False) is None
    f = gds.read_output(fn)
    np.testing.assert_allclose(f["correlation"], np.round(corr, 4), atol=1.01e-4, equal_nan=True)  # atol: run-to-run ulps at a rounding edge
    assert np.array_equal(f["snp.id"], hapmap.snp_id) and np.array_equal(f["sample.id"], hapmap.sample_id[:90])
    load = api.snpgdsPCASNPLoading(pca, hapmap, verbose=False)
    assert load["snploading"].shape == (8, 8695)
    assert np.abs(_sign_fix(load["snploading"], z["snploading"], 1) - z["snploading"]).max() < 5.01e-4
    sl = api.snpgdsPCASampLoading(load, hapmap, sample_id=hapmap.sample_id[:100], verbose=False)
    assert sl["eigenvect"].shape == (100, 8) and np.isnan(sl["eigenval"]).all()
    # golden rounded to 4 decimals (half a unit = 5e-5) + the eigenvectors' share of the covariance's fp32-accumulation error
    # (<= 1e-5 relative by contract; 1.3e-6 observed at an entry that sits on a rounding edge)
    assert np.abs(_sign_fix(sl["eigenvect"], z["samploading"], 0) - z["samploading"]).max() < 5e-5 + 3e-6
    # projecting the PCA's own samples gives back their eigenvectors (to the accuracy of the covariance)
    np.testing.assert_allclose(np.abs(sl["eigenvect"][:90]), np.abs(pca["eigenvect"]), atol=2e-5)


def test_projector_vs_oracle_synthetic():
    """Projector (block level) vs the numpy oracle: several blocks, k not a multiple of 8, missing calls,
    monomorphic and all-missing SNPs, Bayesian scaling."""
    from snprelate_amd import _lib
    n, L, k = 333, 1500, 11
    g = synth_geno(n, L, missing=0.06, seed=91)
    g[7] = 3
    g[8] = 2
    g[9, 5:] = 3                      # five calls left
    g[10, 1:] = 3                     # a single call -> NaN correlation
    rng = np.random.default_rng(4)
    ev = rng.normal(size=(k, n))
    ev[3] = 1.0                       # a constant "eigenvector": zero variance -> NaN
    cuts = [0, 100, 164, 677, 1500]
    blocks = list(zip(cuts[:-1], cuts[1:]))
    with _lib.Projector(n, k, max_block_snps=1024) as p:
        p.set_eigvec(ev)
        corr = np.concatenate([p.snp_corr(g[a:b]) for a, b in blocks])
        ref = orc.pca_snp_corr(g, ev)
        assert np.array_equal(np.isnan(corr), np.isnan(ref))
        np.testing.assert_allclose(corr, ref, rtol=1e-9, atol=1e-12, equal_nan=True)
        for bayes in (False, True):
            w = np.linspace(3.0, 0.5, k)
            tr = 123.4
            p.set_eigvec(ev * np.sqrt((n - 1) / tr / w)[:, None])
            parts = [p.snp_loading(g[a:b], bayesian=bayes) for a, b in blocks]
            load = np.concatenate([x[0] for x in parts])
            af = np.concatenate([x[1] for x in parts])
            sc = np.concatenate([x[2] for x in parts])
            rl, ra, rs = orc.pca_snp_loading(g, w, ev, tr, bayesian=bayes)
            np.testing.assert_allclose(af, ra, rtol=1e-14)
            np.testing.assert_allclose(sc, rs, rtol=1e-14)
            np.testing.assert_allclose(load, rl, rtol=1e-10, atol=1e-12)
            # ... and the long-double reference at the bound of fp64 summation in any order (tests/proj_ref.py)
            xl, _, _, xb = proj_ref.snp_loading(g, ev * np.sqrt((n - 1) / tr / w)[:, None], bayes)
            assert (np.abs(load - xl) <= xb).all()
        sload = rl * 0.37
    with _lib.Projector(n, k, max_block_snps=1024) as p:
        for a, b in blocks:
            p.samp_loading_feed(g[a:b], sload[a:b], ra[a:b], rs[a:b])
        got = p.samp_loading()
    np.testing.assert_allclose(got, orc.pca_samp_loading(g, sload, ra, rs), rtol=1e-10, atol=1e-11)
    xs, xb = proj_ref.add_feeds([proj_ref.samp_loading(g[a:b], sload[a:b], ra[a:b], rs[a:b]) for a, b in blocks])
    assert (np.abs(got - xs) <= xb).all()


def test_eigmix_loadings_vs_oracle(hapmap):
    """snpgdsPCASNPLoading / snpgdsPCASampLoading on a snpgdsEIGMIX object (gnrEigMixSNPLoading / SampLoading,
    src/genEIGMIX.cpp:739-803) against the numpy restatement (no golden in the reference's tests: parity
    unpinned), plus the projection of the analysis' own samples on data without missing calls."""
    from snprelate_amd import api, gds
    sid = hapmap.sample_id[:90]
    em = api.snpgdsEIGMIX(hapmap, sample_id=sid, missing_rate=float("nan"), eigen_cnt=6, diagadj=False, verbose=False)
    load = api.snpgdsPCASNPLoading(em, hapmap, verbose=False)
    sel = np.isin(hapmap.snp_id, em["snp_id"])
    g = hapmap.read_genotype(snp_sel=sel, samp_sel=np.arange(90))
    ref = orc.eigmix_snp_loading(g, em["eigenval"][:6], em["eigenvect"].T, em["afreq"])
    np.testing.assert_allclose(load["snploading"].T, ref, rtol=1e-9, atol=1e-12)
    sl = api.snpgdsPCASampLoading(load, hapmap, sample_id=hapmap.sample_id[:120], verbose=False)
    g120 = hapmap.read_genotype(snp_sel=sel, samp_sel=np.arange(120))
    sload = ref * np.sqrt(1 / em["eigenval"][:6])[None, :]
    np.testing.assert_allclose(sl["eigenvect"].T, orc.eigmix_samp_loading(g120, sload, em["afreq"]), rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError):
        api.snpgdsPCASNPLoading(dict(em, diagadj=True), hapmap, verbose=False)
    # no missing calls: projecting the analysis' own samples returns their eigenvectors
    gs = _structured_geno(300, 2000, seed=3)
    gs[gs == 3] = 0
    f = gds.GenoFile(genotype=gs)
    em = api.snpgdsEIGMIX(f, autosome_only=False, remove_monosnp=True, missing_rate=float("nan"), eigen_cnt=4,
                          diagadj=False, verbose=False)
    sl = api.snpgdsPCASampLoading(api.snpgdsPCASNPLoading(em, f, verbose=False), f, verbose=False)
    np.testing.assert_allclose(np.abs(sl["eigenvect"][:, :2]), np.abs(em["eigenvect"][:, :2]), atol=2e-5)


@pytest.mark.parametrize("missing", [0.02, 0.0])
def test_panel_product_matches_dense_many_vectors(missing):
    """snpgpu_pca_panel_matmul with more vectors than one kernel pass holds (48) and a row count that is not a
    multiple of the tile sizes, against the dense product of the device's own covariance; both forms.  (missing = 0: the
    single-product kernel's row terms R[i] are settled into the panel first -- they must stay out of the padding columns,
    which the product reads up to the next multiple of 16; with missing calls: the rare variants' terms likewise.)"""
    import torch
    from snprelate_amd import _lib
    n, L, m = 1237, 700, 61
    g = synth_geno(n, L, missing=missing, seed=8)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    q = torch.from_numpy(rng.normal(size=(m, n))).to(dev)
    # forms: the one-pass kernel on the tile-major panel (default) and on a row-major one, the two rocBLAS dgemms (their
    # switch is read when the context is created: the panel must be row-major for them)
    for env in ({}, {"SNPGPU_ACC_LAYOUT": "row"}, {"SNPGPU_EIG_BLAS": "1"}):
        os.environ.update(env)
        try:
            with _lib.Accumulator(_lib.PCA_COV, n, max_block_snps=1024) as a:
                a.feed(g)
                cov = orc.tri_to_full(a.pca_cov(packed=True, normalize=False)[0], n)
                ref = (q.cpu().numpy() @ cov) * 0.5
                y = torch.zeros_like(q)
                torch.cuda.synchronize()
                a.pca_panel_matmul(0.5, q.data_ptr(), m, y.data_ptr())
                torch.cuda.synchronize()
        finally:
            for k in env:
                os.environ.pop(k, None)
        np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-11, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("layout", ["tile", "row"])
def test_panel_product_fp32_form(layout, monkeypatch):
    """snpgpu_pca_panel_matmul_f32 (what the Krylov solver runs on while its residual is far above fp32 rounding): panel and
    vectors rounded to fp32, fp32 matrix instructions, fp64 result.  Against the dense fp64 product on three row panels with a
    ragged sample count and more vectors than one launch holds: error a few fp32 roundings of |C| |q|, i.e. every result row
    lands where the fp64 form puts it (the two instructions differ in their result lane map)."""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.dist import panel_rows
    if layout == "row":
        monkeypatch.setenv("SNPGPU_ACC_LAYOUT", "row")
    n, L, m = 2331, 900, 53
    g = synth_geno(n, L, missing=0.02, seed=18)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    qh = rng.normal(size=(m, n)) * (1.0 + np.arange(m)[:, None])          # every vector its own scale: rows cannot swap unseen
    q = torch.from_numpy(qh).to(dev)
    with _lib.Accumulator(_lib.PCA_COV, n, max_block_snps=1024) as a:
        a.feed(g)
        cov = orc.tri_to_full(a.pca_cov(packed=True, normalize=False)[0], n)
    ref = (qh @ cov) * 0.25
    bounds = panel_rows(n, 3)
    y32, y64 = torch.zeros_like(q), torch.zeros_like(q)
    for r in range(3):
        with _lib.Accumulator(_lib.PCA_COV, n, row_begin=bounds[r], row_end=bounds[r + 1], max_block_snps=1024) as a:
            a.feed(g)
            torch.cuda.synchronize()
            a.pca_panel_matmul(0.25, q.data_ptr(), m, y32.data_ptr(), fp32=True)
            a.pca_panel_matmul(0.25, q.data_ptr(), m, y64.data_ptr())
            torch.cuda.synchronize()
    np.testing.assert_allclose(y64.cpu().numpy(), ref, rtol=1e-11, atol=1e-9 * np.abs(ref).max())
    bound = 0.25 * (np.abs(qh) @ np.abs(cov))                             # sum of |terms| of every result
    err = np.abs(y32.cpu().numpy() - ref) / bound
    assert err.max() < 4e-7, err.max()                                    # 2^-24 = 6e-8 per rounding, a handful in a row
    assert err.max() > 1e-12                                              # it IS the fp32 form


def _structured_geno(n, L, seed):
    """three sub-populations -> two well separated leading eigenvalues"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, size=(L, 1))
    pop = np.arange(n) * 3 // n
    shift = rng.normal(0, 0.15, size=(L, 3))
    pp = np.clip(p + shift[:, pop], 0.02, 0.98)
    g = (rng.random((L, n)) < pp).astype(np.uint8) + (rng.random((L, n)) < pp).astype(np.uint8)
    g[rng.random((L, n)) < 0.02] = 3
    return g


@pytest.mark.parametrize("n,L,aux,it", [(400, 3000, 8, 4), (150, 2500, 16, 10)])
def test_randomized_pca_vs_oracle(n, L, aux, it):
    """snpgdsPCA(algorithm="randomized") (CRandomPCA, src/genPCA.cpp:472-803) against the numpy restatement
    from the same start matrix; both SVD branches (n_samp >= / < aux.dim * (iter.num + 1)).  The reference's
    tests hold no golden for this algorithm; the restatement is pinned through the exact PCA's golden
    (test_pca_randomized_pinned_by_the_exact_pca_golden).  The oracle follows the reference's two-pass
    SVD formulation, the device path uses one pass per iteration and a QR basis."""
    from snprelate_amd import api, gds
    g = _structured_geno(n, L, seed=n)
    f = gds.GenoFile(genotype=g)
    rng = np.random.default_rng(7)
    aux_mat = rng.normal(size=(aux, n))
    k = 6
    r = api.snpgdsPCA(f, autosome_only=False, remove_monosnp=False, missing_rate=float("nan"), algorithm="randomized",
                      eigen_cnt=k, aux_dim=aux, iter_num=it, aux_mat=aux_mat, verbose=False)
    sig, vt, tr2 = orc.pca_randomized(g, aux_mat, it)
    np.testing.assert_allclose(r["TraceXTX"], tr2, rtol=1e-12)
    ref_val = (n - 1) * 2 * sig[:k] ** 2 / tr2
    np.testing.assert_allclose(r["eigenval"][:k], ref_val, rtol=1e-7)
    assert r["eigenvect"].shape == (n, k)
    cos = np.abs(np.sum(r["eigenvect"] * vt[:k].T, axis=0))
    gap = np.abs(np.diff(np.r_[ref_val, ref_val[-1] * 0.5])) / ref_val[0]
    assert np.all(cos[:2] > 1 - 1e-9), cos              # the two structural components
    assert np.all(cos[gap > 1e-3] > 1 - 1e-6), (cos, gap)
    # and they are the exact PCA's leading components
    cov = orc.pca_cov(g)
    orc.trace_normalize(cov, n)
    w, v = np.linalg.eigh(orc.tri_to_full(cov, n))
    assert np.all(np.abs(np.sum(r["eigenvect"][:, :2] * v[:, ::-1][:, :2], axis=0)) > 0.999)


def test_PCA_documented_varprop(hapmap):
    """man/snpgdsPCA.Rd:101-118: variance proportions / first eigenvector rows of the full
    example (the documented numbers correspond to missing.rate=NaN, i.e. 8722 SNPs)."""
    from snprelate_amd import api
    r = api.snpgdsPCA(hapmap, missing_rate=float("nan"), verbose=False)
    assert len(r["snp_id"]) == 8722
    pc = np.round(r["varprop"][:6] * 100, 2)
    assert pc.tolist() == [12.23, 5.84, 1.01, 0.95, 0.84, 0.74]
    doc = np.array([[-0.08411287, -0.01226860], [-0.08360644, -0.01085849], [-0.08110808, -0.01184524],
                    [-0.08680864, -0.01447106], [0.03109761, 0.07709255], [0.03228450, 0.08155730]])
    ev = r["eigenvect"][:6, :2]
    ev = ev * np.sign(ev[0] * doc[0])           # eigenvector signs are arbitrary
    np.testing.assert_allclose(ev, doc, atol=2e-6)


def test_GRM_hapmap_strict_per_entry_tolerance(hapmap):
    """configs[0] at the north_star's literal wording: every entry of the 279 x 279 GCTA matrix of the example file (8039 SNPs,
    1583 missing calls) within rtol = 1e-5 of the fp64 oracle with an EXPLICIT absolute floor of 2e-8 (the matrix's entries are
    ~0.13 in the median, ~1.3 on the diagonal; measured: rtol 1e-5 + atol 1e-8 holds with a factor 2 to spare, atol 1e-9 does not --
    0.01 % of the entries are sums that cancel to below 1e-3 of the typical entry and miss a purely relative 1e-5)."""
    from snprelate_amd import api
    r = api.snpgdsGRM(hapmap, method="GCTA", verbose=False)
    g = hapmap.read_genotype(snp_sel=np.isin(hapmap.snp_id, r["snp_id"]))
    ref = orc.tri_to_full(orc.grm_gcta(g), 279)
    np.testing.assert_allclose(r["grm"], ref, rtol=1e-5, atol=2e-8)
    rel = np.abs(r["grm"] - ref) / np.abs(ref)
    assert (rel > 1e-5).mean() < 5e-4


def test_GRM_known_answers_and_methods(hapmap):
    from snprelate_amd import api
    r = api.snpgdsGRM(hapmap, method="GCTA", verbose=False)
    g = r["grm"]
    assert len(r["snp_id"]) == 8039 and g.shape == (279, 279)
    np.testing.assert_allclose(g[0, 0], 1.3925009439720786, rtol=1e-5)
    np.testing.assert_allclose(g[1, 1], 1.3087163456244955, rtol=1e-5)
    np.testing.assert_allclose(g[0, 1], 0.2421021559446208, rtol=1e-5)
    np.testing.assert_allclose(g[0, 278], -0.09733479032489507, rtol=1e-5)
    np.testing.assert_allclose(np.trace(g), 305.28199493848285, rtol=1e-6)
    tri = api.snpgdsGRM(hapmap, method="GCTA", useMatrix=True, with_id=False, verbose=False)
    assert np.array_equal(_tri_full(tri, 279), g)
    corr = api.snpgdsGRM(hapmap, method="Corr", verbose=False)["grm"]
    d = np.sqrt(np.diag(g))
    np.testing.assert_allclose(corr, g / np.outer(d, d), rtol=1e-12, atol=1e-12)
    eig = api.snpgdsGRM(hapmap, method="Eigenstrat", verbose=False)["grm"]
    np.testing.assert_allclose(np.trace(eig), 278.0, rtol=1e-9)
    with pytest.raises(ValueError):
        api.snpgdsGRM(hapmap, method="bogus", verbose=False)


@pytest.fixture(params=["f16", "f16_x1"])
def syrk_backend_all(request, monkeypatch):
    """the default GRM / PCA path, and the exact-row kernel for every block (SNPGPU_SYRK_UV=0)"""
    monkeypatch.setenv("SNPGPU_SYRK", "f16")
    monkeypatch.setenv("SNPGPU_SYRK_UV", "0" if request.param == "f16_x1" else "1")
    return request.param


@pytest.mark.parametrize("which", ["default_filter", "all_autosomal_with_missing"])
def test_GRM_GCTA_hapmap_full_matrix_vs_oracle(hapmap, which, syrk_backend_all):
    """The path the headline benchmark measures (CGCTA_AlgArith::Run, src/genPCA.cpp:1148-1237) on real data with
    missing calls: EVERY entry of the 279 x 279 HapMap GRM against the pinned oracle -- with the default SNP filter
    (8039 SNPs, 1583 missing cells) and with all autosomal SNPs (missing.rate = NaN: up to 30 % missing per SNP,
    monomorphic SNPs kept for the reader and dropped by the kernel's own 0 < p < 1 rule)."""
    import oracle as orc
    from snprelate_amd import api
    from norms import error_figures, tri_diag_scale
    kw = {} if which == "default_filter" else dict(remove_monosnp=False, missing_rate=float("nan"))
    r = api.snpgdsGRM(hapmap, method="GCTA", useMatrix=True, with_id=True, verbose=False, **kw)
    sel = np.isin(hapmap.snp_id, r["snp_id"])
    g = np.ascontiguousarray(hapmap.read_genotype(snp_sel=sel))
    assert g.shape == (len(r["snp_id"]), 279) and int((g > 2).sum()) > 1000
    if which == "default_filter":
        assert g.shape[0] == 8039 and int((g > 2).sum()) == 1583
    ref = orc.grm_gcta(g)
    got = np.asarray(r["grm"])
    f = error_figures(got, ref, tri_diag_scale(ref, 279))
    assert f["contract"] < 1e-5 and f["offdiag"] < 1e-5, f


@pytest.mark.parametrize("method", ["GCTA", "IndivBeta"])
def test_GRM_merge_self_consistency(hapmap, method, tmp_path):
    """test.merge.GCTA.grm / test.merge.beta.grm, test_GRM.R:14-87: GRMs of a SNP partition written with out.fn,
    merged by snpgdsMergeGRM, equal the GRM of the whole SNP set (RUnit checkEquals tolerance 1.5e-8)."""
    from snprelate_amd import api
    rf = api.snpgdsSNPRateFreq(hapmap)
    snpid = hapmap.snp_id[rf["MissingRate"] == 0]
    parts = [snpid[:1000], snpid[1000:3000], snpid[3000:]]
    files = []
    for i, p in enumerate(parts):
        fn = str(tmp_path / ("tmp%d.gds" % (i + 1)))
        assert api.snpgdsGRM(hapmap, snp_id=p, method=method, out_fn=fn, verbose=False) is None
        files.append(fn)
    out_fn = str(tmp_path / "tmp.gds")
    assert api.snpgdsMergeGRM(files, out_fn, verbose=False) is None
    whole = api.snpgdsGRM(hapmap, snp_id=snpid, method=method, verbose=False)
    from snprelate_amd import gds
    f = gds.read_output(out_fn)
    tol = dict(rtol=2e-5, atol=2e-6) if method == "GCTA" else dict(rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(f["grm"], whole["grm"], **tol)
    assert np.array_equal(f["snp.id"], whole["snp_id"]) and np.array_equal(f["sample.id"], whole["sample_id"])
    # in-memory return and the oracle's gnrGRMMerge restatement on the same files
    mem = api.snpgdsMergeGRM(files, verbose=False)
    np.testing.assert_allclose(mem["grm"], f["grm"], rtol=1e-12, atol=1e-14)   # the baseline sums use fp64 atomics
    ins = [gds.read_output(fn) for fn in files]
    w = np.array([len(x["snp.id"]) for x in ins], float)
    ref, avg = orc.grm_merge([x["grm"] for x in ins], w / w.sum(), str(ins[0]["command"][1]),
                             [float(x["avg_val"]) for x in ins] if method == "IndivBeta" else None)
    np.testing.assert_allclose(mem["grm"], ref, rtol=1e-12, atol=1e-14)
    if method == "IndivBeta":
        np.testing.assert_allclose(mem["avg_val"], avg, rtol=1e-12)
        np.testing.assert_allclose(float(f["avg_val"]), whole["avg_val"], rtol=1e-9)
    # logical weights: subtracting the last set from the whole leaves the first two (R/IBD.R:682-689, 704-712)
    if method == "GCTA":
        wfn = str(tmp_path / "whole.gds")
        api.snpgdsGRM(hapmap, snp_id=snpid, method=method, out_fn=wfn, verbose=False)
        sub = api.snpgdsMergeGRM([wfn, files[2]], weight=[True, False], verbose=False)
        two = api.snpgdsMergeGRM(files[:2], verbose=False)
        np.testing.assert_allclose(sub["grm"], two["grm"], rtol=2e-5, atol=2e-6)
        assert np.array_equal(np.sort(sub["snp_id"]), np.sort(two["snp_id"]))
        with pytest.raises(ValueError, match="different command"):
            bfn = str(tmp_path / "b.gds")
            api.snpgdsGRM(hapmap, snp_id=parts[0], method="IndivBeta", out_fn=bfn, verbose=False)
            api.snpgdsMergeGRM([files[0], bfn], verbose=False)


def test_SNPRateFreq_vs_numpy(hapmap):
    """test_Func.R:14-31: allele frequency / missing rate vs column means."""
    from snprelate_amd import api
    rf = api.snpgdsSNPRateFreq(hapmap)
    g = hapmap.read_genotype().astype(float)
    g[g > 2] = np.nan
    np.testing.assert_allclose(rf["AlleleFreq"], np.nanmean(g, axis=1) / 2, rtol=1e-14)
    np.testing.assert_allclose(rf["MissingRate"], np.isnan(g).mean(axis=1), rtol=1e-14, atol=1e-16)


def test_error_behaviour(hapmap):
    from snprelate_amd import api, _lib
    with pytest.raises(ValueError, match="Some of sample.id do not exist!"):
        api.snpgdsIBS(hapmap, sample_id=["nope"], verbose=False)
    with pytest.raises(ValueError, match="should be the number of samples"):
        api.snpgdsIBDKING(hapmap, family_id=[1, 2, 3], verbose=False)
    with pytest.raises(_lib.SnpGpuError, match="wrong context kind"):
        with _lib.Accumulator(_lib.IBS, 64) as a:
            a.grm_gcta()
    with pytest.raises(_lib.SnpGpuError, match="larger than max_block_snps"):
        with _lib.Accumulator(_lib.IBS, 64, max_block_snps=64) as a:
            a.feed(np.zeros((128, 64), np.uint8))
    with pytest.raises(_lib.SnpGpuError, match="multiple of 256"):
        _lib.Accumulator(_lib.IBS, 1000, row_begin=100, row_end=500)


def test_edge_inputs():
    """empty feed, single sample, single SNP, all-missing data, ragged tail blocks."""
    from snprelate_amd import _lib
    g = synth_geno(5, 70, missing=0.3, seed=5)
    with _lib.Accumulator(_lib.IBS, 5, max_block_snps=64) as a:
        a.feed(g[:0])
        a.feed(g[:64]); a.feed(g[64:])
        got = np.stack(a.ibs_num(packed=True), 1).astype(np.uint32)
    assert np.array_equal(got, orc.ibs_count(g))
    one = np.array([[1], [3], [2]], np.uint8)
    with _lib.Accumulator(_lib.KING_ROBUST, 1) as a:
        a.feed(one)
        assert np.array_equal(a.king_robust_counts(), orc.king_robust_count(one))
    allmiss = np.full((40, 9), 3, np.uint8)
    with _lib.Accumulator(_lib.GRM_GCTA, 9) as a:
        a.feed(allmiss)
        out = a.grm_gcta(packed=True)
    assert np.all(~np.isfinite(out))            # 0/0, not "fixed" 
    with _lib.Accumulator(_lib.IBS, 9) as a:
        a.feed(allmiss)
        ave = a.ibs_ave(packed=True)
    assert np.all(np.isnan(ave))
    # values > 3 in byte input are clamped to missing (vec_u8_geno_valid, dGenGWAS.cpp:1388)
    gg = synth_geno(33, 100, missing=0.0, seed=9)
    gg2 = gg.copy(); gg2[gg2 == 2][:0] = 2
    gg3 = gg.copy(); gg3[5, 7] = 200; gg_ref = gg.copy(); gg_ref[5, 7] = 3
    with _lib.Accumulator(_lib.IBS, 33) as a:
        a.feed(gg3)
        got = np.stack(a.ibs_num(packed=True), 1).astype(np.uint32)
    assert np.array_equal(got, orc.ibs_count(gg_ref))
    # 2-bit packed input path == byte input path
    from snprelate_amd.gds import pack_2bit_rows
    with _lib.Accumulator(_lib.KING_ROBUST, 33) as a:
        a.feed(pack_2bit_rows(gg_ref), fmt=_lib.GENO_PACKED2)
        assert np.array_equal(a.king_robust_counts(), orc.king_robust_count(gg_ref))


@pytest.mark.parametrize("missing", [0.04, 0.0])
def test_row_panels_reassemble(missing):
    """Row-panel contexts (the multi-GPU sharding unit) reproduce the full triangle (missing = 0: the
    exact-row-side SYRK with its column term, panels that start past sample 0 and end in padding rows)."""
    from snprelate_amd import _lib
    from snprelate_amd.dist import panel_rows, slab_range
    n, L = 1100, 900
    g = synth_geno(n, L, missing=missing, seed=21, special=missing > 0)
    ref_k = orc.king_robust_count(g)
    ref_g = orc.grm_gcta(g)
    for world in (2, 3):
        b = panel_rows(n, world)
        assert b[0] == 0 and b[-1] == n
        gk = np.zeros_like(ref_k)
        gg = np.zeros_like(ref_g)
        for r in range(world):
            if b[r + 1] <= b[r]:
                continue
            lo, hi = slab_range(n, b[r], b[r + 1])
            with _lib.Accumulator(_lib.KING_ROBUST, n, row_begin=b[r], row_end=b[r + 1]) as a:
                a.feed(g)
                assert a.slab_size() == hi - lo
                gk[lo:hi] = a.king_robust_counts()
            with _lib.Accumulator(_lib.GRM_GCTA, n, row_begin=b[r], row_end=b[r + 1]) as a:
                a.feed(g)
                gg[lo:hi] = a.grm_gcta(packed=True)
        assert np.array_equal(gk, ref_k)
        assert np.nanmax(np.abs(gg - ref_g) / (np.abs(ref_g) + np.median(np.abs(ref_g)))) < 1e-5


def test_multi_panel_drivers_single_rank():
    """The multi-GPU drivers with several panels per rank (memory balancing, dist.panel_plan) on one device:
    GRM (both methods), KING and the distributed PCA agree with the oracle."""
    import torch
    from snprelate_amd import multigpu
    n, L = 1300, 1200
    g = synth_geno(n, L, missing=0.03, seed=33)
    blocks = [g[:700], g[700:]]
    ref = orc.grm_gcta(g)
    for k in (1, 3):
        got = multigpu.grm_distributed(blocks, n, method="GCTA", panels_per_rank=k).cpu().numpy()
        assert np.nanmax(np.abs(got - ref) / (np.abs(ref) + np.median(np.abs(ref)))) < 1e-5
    cov = orc.pca_cov(g)
    orc.trace_normalize(cov, n)
    got = multigpu.grm_distributed(blocks, n, method="Eigenstrat", panels_per_rank=3).cpu().numpy()
    assert np.nanmax(np.abs(got - cov) / (np.abs(cov) + np.median(np.abs(cov)))) < 1e-5
    r0, rk = orc.king_robust_final(orc.king_robust_count(g), n, None)
    g0, gk = multigpu.king_distributed(blocks, n, panels_per_rank=3)
    assert np.array_equal(g0.cpu().numpy(), r0, equal_nan=True)
    assert np.array_equal(gk.cpu().numpy(), rk, equal_nan=True)
    w_ref = np.linalg.eigvalsh(orc.tri_to_full(cov, n))[::-1][:8]
    res = multigpu.pca_distributed(blocks, n, eigen_cnt=8, panels_per_rank=3)
    np.testing.assert_allclose(res["eigenval"].cpu().numpy(), w_ref, rtol=2e-5)


def test_eigen_solver_never_returns_unconverged_pairs(monkeypatch):
    """(a) A cycle budget that runs out ends with an fp64 check of the vectors at hand: pairs that miss the tolerance are an ERROR
    (as LAPACK's dspevx reports INFO > 0), never returned as if exact -- here one restart cycle of two blocks on a flat spectrum.
    (b) A request for a large share of the spectrum (k > n / 8, n <= 16 384) takes the dense solver whatever
    SNPGPU_EIG_DENSE_MAX says: k = n / 3 of n = 2304 samples against numpy."""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.eigen import PanelOperator, topk_eigen
    n, L = 2304, 1500
    g = synth_geno(n, L, missing=0.01, seed=23, special=False)
    with _lib.Accumulator(_lib.PCA_COV, n) as a:
        a.feed(g)
        op = PanelOperator([a], n, torch.device("cuda", 0))
        with pytest.raises(_lib.SnpGpuError, match="not converged after 1 restart"):
            topk_eigen(op, 8, depth=2, max_restarts=1, tol=1e-12)
        w8, _, info = topk_eigen(op, 8)
        assert info["max_rel_residual"] < 1e-9
        monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "0")          # "always Krylov" -- except for requests like this one
        k = n // 3
        w, v = a.pca_eigen(k)
    cov = orc.pca_cov(g)
    orc.trace_normalize(cov, n)
    full = orc.tri_to_full(cov, n)
    w_ref = np.linalg.eigvalsh(full)[::-1]
    np.testing.assert_allclose(w, w_ref[:k], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(w8.cpu().numpy(), w_ref[:8], rtol=2e-5)
    res = np.linalg.norm(full @ v[:, :16] - v[:, :16] * w[:16], axis=0) / np.abs(w[:16])
    assert res.max() < 1e-5


@pytest.mark.parametrize("panel_product", ["sym_kernel", "rocblas"])
@pytest.mark.parametrize("large_n_algebra", [False, True])
def test_iterative_eigen_matches_dense(large_n_algebra, panel_product, monkeypatch):
    """Distributed-style top-k solver (panel matmul + block Krylov) vs the dense device solver and
    vs numpy on the oracle's covariance; panels on one device stand in for several ranks.
    large_n_algebra: force the split-K Gram products and CholeskyQR2 that the solver uses for N >= 32768."""
    import torch
    from snprelate_amd import _lib, eigen
    from snprelate_amd.dist import panel_rows
    from snprelate_amd.eigen import PanelOperator, topk_eigen
    if panel_product == "rocblas":          # the two-dgemm form of snpgpu_pca_panel_matmul
        monkeypatch.setenv("SNPGPU_EIG_BLAS", "1")
    if large_n_algebra:                     # read by the solver when it starts (csrc/eigen.hip)
        monkeypatch.setenv("SNPGPU_EIG_CHOLQR_MIN_N", "0")
        monkeypatch.setenv("SNPGPU_EIG_GRAM_CHUNK", "128")
    n, L, k = 1500, 3000, 16
    rng = np.random.default_rng(5)
    # two sub-populations so that there is real structure in the top eigenvectors
    p = rng.uniform(0.1, 0.9, size=(L, 1))
    shift = rng.normal(0, 0.12, size=(L, 1))
    pp = np.clip(np.where(np.arange(n)[None, :] < n // 3, p + shift, p - shift / 2), 0.02, 0.98)
    g = (rng.random((L, n)) < pp).astype(np.uint8) + (rng.random((L, n)) < pp).astype(np.uint8)
    g[rng.random((L, n)) < 0.01] = 3
    ref = orc.pca_cov(g)
    orc.trace_normalize(ref, n)
    w_ref, v_ref = np.linalg.eigh(orc.tri_to_full(ref, n))
    w_ref, v_ref = w_ref[::-1][:k], v_ref[:, ::-1][:, :k]
    dev = torch.device("cuda", 0)
    bounds = panel_rows(n, 3)
    panels = []
    for r in range(3):
        if bounds[r + 1] > bounds[r]:
            a = _lib.Accumulator(_lib.PCA_COV, n, row_begin=bounds[r], row_end=bounds[r + 1])
            a.feed(g[:2000]); a.feed(g[2000:])
            panels.append(a)
    op = PanelOperator(panels, n, dev)
    w, v, info = topk_eigen(op, k)
    # most products are fp32 (never with the dgemm form); what is accepted is the fp64 product of the returned vectors: same
    # answer as the fp64-only solve to the solver's tolerance, and the same with the mixed cycles switched off
    assert (info["matmuls_fp32"] > 0) == (panel_product == "sym_kernel") and info["matmuls_fp32"] < info["matmuls"]
    w64, v64, info64 = topk_eigen(op, k, fp32_until=-1.0)
    assert info64["matmuls_fp32"] == 0 and info64["max_rel_residual"] < 1e-8
    np.testing.assert_allclose(w.cpu().numpy(), w64.cpu().numpy(), rtol=1e-12)
    monkeypatch.setenv("SNPGPU_EIG_MIXED", "0")          # fp32 cycles, then fp64 cycles only
    w2, v2, info2 = topk_eigen(op, k)
    monkeypatch.delenv("SNPGPU_EIG_MIXED")
    assert info2["max_rel_residual"] < 1e-8
    np.testing.assert_allclose(w2.cpu().numpy(), w64.cpu().numpy(), rtol=1e-12)
    monkeypatch.setenv("SNPGPU_EIG_KEEP", "1")           # restart from one block of Ritz vectors (round 2's restart)
    w3, v3, info3 = topk_eigen(op, k, depth=6)
    monkeypatch.delenv("SNPGPU_EIG_KEEP")
    wt, vt, infot = topk_eigen(op, k, depth=6)           # thick restart (2 of 6 blocks kept): fewer products
    assert info3["max_rel_residual"] < 1e-8 and infot["max_rel_residual"] < 1e-8 and infot["matmuls"] <= info3["matmuls"]
    np.testing.assert_allclose(w3.cpu().numpy(), w64.cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(wt.cpu().numpy(), w64.cpu().numpy(), rtol=1e-12)
    w, v = w.cpu().numpy(), v.cpu().numpy()
    np.testing.assert_allclose(w, w_ref, rtol=2e-5)
    cos = np.abs(np.sum(v * v_ref, axis=0))
    gap_ok = np.r_[True, np.abs(np.diff(w_ref)) > 1e-3 * w_ref[0]] & np.r_[np.abs(np.diff(w_ref)) > 1e-3 * w_ref[0], True]
    assert np.all(cos[gap_ok] > 1 - 1e-4), (cos, info)
    assert info["max_rel_residual"] < 1e-8
    for a in panels:
        a.close()
    # dense device solver on a full context agrees as well
    with _lib.Accumulator(_lib.PCA_COV, n) as a:
        a.feed(g[:2000]); a.feed(g[2000:])
        wd, vd = a.pca_eigen(k)
        cf = orc.tri_to_full(a.pca_cov(packed=True, normalize=True)[0], n)
    np.testing.assert_allclose(wd, w_ref, rtol=2e-5)
    # the residual the solver reports is the residual of what it returned, against the device's own matrix in fp64 numpy
    res = np.linalg.norm(cf @ v - v * w, axis=0) / np.abs(w)
    assert res.max() < 1e-8 and abs(res.max() - info["max_rel_residual"]) < 1e-9, (res.max(), info)


def test_krylov_solver_when_fewer_than_two_blocks_fit():
    """snpgpu_panels_topk_eigen on a matrix smaller than two Krylov blocks (the ABI accepts any n; the wrappers send such
    sizes to the dense solver): one block that is the whole space, exact after the first fp64 cycle."""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.eigen import PanelOperator, topk_eigen
    n, L, k = 70, 400, 32
    g = synth_geno(n, L, missing=0.02, seed=21)
    with _lib.Accumulator(_lib.PCA_COV, n) as a:
        a.feed(g)
        cov = orc.tri_to_full(a.pca_cov(packed=True, normalize=True)[0], n)
        w, v, info = topk_eigen(PanelOperator([a], n, torch.device("cuda", 0)), k)
    w_ref = np.linalg.eigvalsh(cov)[::-1][:k]
    np.testing.assert_allclose(w.cpu().numpy(), w_ref, rtol=1e-10)
    assert info["max_rel_residual"] < 1e-9 and info["block"] == n


@pytest.mark.parametrize("missing", [0.0, 0.03])
def test_gcta_grm_and_its_eigenvectors_from_one_accumulation(missing):
    """north_star: "GCTA-method GRM + top-k eigenvectors" -- the GCTA accumulators are finalised IN PLACE
    (snpgpu_finalize_inplace: numerator / (2 (nLocus - Denom)) written over the sums), the same panels then serve the
    finaliser (the GRM itself) and the eigen solver.  Three row panels on one device vs the oracle's GRM and numpy's eigh."""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.dist import panel_rows
    from snprelate_amd.eigen import PanelOperator, topk_eigen
    n, L, k = 1100, 2600, 10
    g = _structured_geno(n, L, seed=77)                       # carries 2 % missing calls
    if missing == 0:
        g[g > 2] = 1                                          # blocks without missing calls: the single-product kernel
    ref = orc.grm_gcta(g)
    full = orc.tri_to_full(ref, n)
    w_ref, v_ref = np.linalg.eigh(full)
    w_ref, v_ref = w_ref[::-1][:k], v_ref[:, ::-1][:, :k]
    bounds = panel_rows(n, 3)
    panels, got = [], np.empty_like(ref)
    for r in range(3):
        a = _lib.Accumulator(_lib.GRM_GCTA, n, row_begin=bounds[r], row_end=bounds[r + 1], max_block_snps=1024)
        for i in range(0, L, 1000):
            a.feed(g[i:i + 1000])
        before = a.grm_gcta(packed=True)
        a.finalize_inplace()
        after = a.grm_gcta(packed=True)
        assert np.array_equal(before, after)                  # the stored matrix IS what the finaliser computes
        with pytest.raises(_lib.SnpGpuError):
            a.feed(g[:10])                                    # no block may follow
        lo = bounds[r] * n - bounds[r] * (bounds[r] - 1) // 2
        got[lo:lo + after.size] = after
        panels.append(a)
    assert np.nanmax(np.abs(got - ref) / (np.abs(ref) + np.median(np.abs(ref)))) < 1e-5
    op = PanelOperator(panels, n, torch.device("cuda", 0), normalize=False)
    w, v, info = topk_eigen(op, k)
    np.testing.assert_allclose(w.cpu().numpy(), w_ref, rtol=2e-5)
    cos = np.abs(np.sum(v.cpu().numpy() * v_ref, axis=0))
    gap = np.abs(np.diff(np.r_[w_ref, np.linalg.eigvalsh(full)[::-1][k]]))
    assert np.all(cos[:3] > 1 - 1e-6) and np.all(cos[gap > 1e-3 * w_ref[0]] > 1 - 1e-4), (cos, info)
    assert info["max_rel_residual"] < 1e-8
    for a in panels:
        a.close()


def test_PCA_api_iterative_path_matches_documented_example(hapmap, monkeypatch):
    """Force snpgdsPCA through the large-N (block-Krylov) path and re-check the documented example."""
    from snprelate_amd import api
    monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "100")       # snpgpu_pca_eigen: block Krylov beyond 100 samples
    r = api.snpgdsPCA(hapmap, missing_rate=float("nan"), eigen_cnt=8, verbose=False)
    pc = np.round(r["varprop"][:6] * 100, 2)
    assert pc.tolist() == [12.23, 5.84, 1.01, 0.95, 0.84, 0.74]
    assert np.all(np.isnan(r["eigenval"][8:]))
    assert abs(abs(r["eigenvect"][0, 0]) - 0.08411287) < 2e-6


def test_pinned_double_buffered_feed():
    """The R shim's feeding pattern: two page-locked block buffers, asynchronous copies overlapping
    the kernels; results identical to synchronous feeds."""
    from snprelate_amd import _lib
    n, L, blk = 700, 5000, 512
    g = synth_geno(n, L, missing=0.04, seed=31)
    ref = orc.king_robust_count(g)
    bufs = [_lib.PinnedBuffer((blk, n)), _lib.PinnedBuffer((blk, n))]
    with _lib.Accumulator(_lib.KING_ROBUST, n, max_block_snps=blk) as a:
        for k, i in enumerate(range(0, L, blk)):
            b = bufs[k & 1]
            a.host_wait(b)
            m = min(blk, L - i)
            b.array[:m] = g[i:i + m]
            a.feed_pinned(b, m)
        got = a.king_robust_counts()
    assert np.array_equal(got, ref)
    for b in bufs:
        b.free()


def test_MoM_golden(hapmap):
    """test.PLINK.MoM, test_rel.R:193-224"""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_mom.npz"))
    sid = hapmap.sample_id[:90]
    r = api.snpgdsIBDMoM(hapmap, sample_id=sid, missing_rate=float("nan"), num_thread=1, verbose=False)
    assert np.array_equal(r["snp_id"], z["snp_id"])
    np.testing.assert_allclose(r["afreq"], z["afreq"], rtol=1e-14)
    np.testing.assert_allclose(r["k0"], z["k0"], rtol=1e-12, atol=1e-14)     # integer counts + fp64 closed form
    np.testing.assert_allclose(r["k1"], z["k1"], rtol=1e-12, atol=1e-14)
    rm = api.snpgdsIBDMoM(hapmap, sample_id=sid, missing_rate=float("nan"), useMatrix=True, kinship=True,
                          verbose=False)
    assert np.array_equal(_tri_full(rm["k0"], 90), r["k0"]) and np.array_equal(_tri_full(rm["k1"], 90), r["k1"])
    assert rm["kinship"].shape == rm["k0"].shape


def test_MoM_allele_freq_in_caller_order_drives_the_filter(hapmap):
    """snpgdsIBDMoM(allele.freq=) with snp.id NOT in dataset order and NaN / 0 / 1 frequencies: the reference brings the
    frequencies into dataset order (allele.freq[match(snp.ids[snp.id], tmp.id)], R/Internal.R:355,370) and filters on
    THEM (gnrSelSNP_Base_Ex -> Select_SNP_Base_Ex, src/dGenGWAS.cpp:399-469: non-finite -> dropped, monomorphic /
    MAF tests on the supplied values, missing rate from the genotypes)."""
    from snprelate_amd import api
    from snprelate_amd.gds import unpack_2bit_rows
    rng = np.random.default_rng(41)
    n = 60
    sid = hapmap.sample_id[:n]
    snp = rng.permutation(hapmap.snp_id)[:3000]                  # shuffled: not the dataset order
    af = rng.uniform(0.02, 0.98, len(snp))
    af[::50], af[1::50], af[2::50] = np.nan, 0.0, 1.0
    r = api.snpgdsIBDMoM(hapmap, sample_id=sid, snp_id=snp, allele_freq=af, missing_rate=0.05, maf=0.03, verbose=False)
    # the same selection from the definitions
    chrom = hapmap.snp_chromosome
    in_ds = np.isin(hapmap.snp_id, snp) & (chrom >= 1) & (chrom <= 22)
    ds_ids = hapmap.snp_id[in_ds]
    af_ds = af[[int(np.nonzero(snp == s)[0][0]) for s in ds_ids]]
    g = unpack_2bit_rows(hapmap.packed[in_ds], hapmap.n_samp)[:, :n]
    missrate = 1.0 - (g <= 2).sum(1) / n
    with np.errstate(invalid="ignore"):
        mf = np.minimum(af_ds, 1 - af_ds)
        keep = np.isfinite(af_ds) & (mf > 0) & (mf >= 0.03) & (missrate <= 0.05)
    assert 0 < keep.sum() < len(keep) and (~np.isfinite(af_ds)).any()
    assert np.array_equal(r["snp_id"], ds_ids[keep])
    assert np.array_equal(r["afreq"], af_ds[keep])
    gk = np.ascontiguousarray(g[keep])
    e, _ = orc.mom_expect(gk, in_afreq=af_ds[keep])
    k0, k1 = orc.mom_final(orc.ibs_count(gk), n, e, False)
    np.testing.assert_allclose(r["k0"], _tri_full(k0, n), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["k1"], _tri_full(k1, n), rtol=1e-12, atol=1e-14)
    with pytest.raises(ValueError):
        api.snpgdsIBDMoM(hapmap, sample_id=sid, snp_id=snp, allele_freq=af[:-1], verbose=False)


def test_KING_family_id_levels(hapmap):
    """family.id: every non-NA value is a level of as.factor (negative integers too, R/IBD.R:359-364); '' and NaN are NA."""
    from snprelate_amd import api
    n = 30
    sid = hapmap.sample_id[:n]
    fam_int = np.array([-5, -5, 7, 7, 0, 0] + list(range(100, 100 + n - 6)))
    fam_str = np.array(["a", "a", "b", "b", "", ""] + ["s%d" % i for i in range(n - 6)])
    ri = api.snpgdsIBDKING(hapmap, sample_id=sid, family_id=fam_int, missing_rate=float("nan"), verbose=False)
    rs = api.snpgdsIBDKING(hapmap, sample_id=sid, family_id=fam_str, missing_rate=float("nan"), verbose=False)
    r0 = api.snpgdsIBDKING(hapmap, sample_id=sid, missing_rate=float("nan"), verbose=False)
    # pairs (0,1) and (2,3) share a family in both codings -> the within-family estimator (differs from the default)
    for r in (ri, rs):
        assert r["kinship"][0, 1] != r0["kinship"][0, 1] and r["kinship"][2, 3] != r0["kinship"][2, 3]
    assert ri["kinship"][0, 1] == rs["kinship"][0, 1]
    assert ri["kinship"][4, 5] != r0["kinship"][4, 5]           # integer 0 is a level ...
    assert rs["kinship"][4, 5] == r0["kinship"][4, 5]           # ... the empty string is NA
    assert ri["kinship"][6, 7] == r0["kinship"][6, 7]


def test_IndivBeta_golden(hapmap):
    """test.IndivBeta, test_rel.R:277-304"""
    from snprelate_amd import api
    z = np.load(os.path.join(GOLDEN, "validate_beta.npz"))
    sid = hapmap.sample_id[:90]
    r = api.snpgdsIndivBeta(hapmap, sample_id=sid, missing_rate=float("nan"), verbose=False)
    assert np.array_equal(r["snp_id"], z["snp_id"])
    np.testing.assert_allclose(r["beta"], z["beta"], rtol=1e-11, atol=1e-13)
    rm = api.snpgdsIndivBeta(hapmap, sample_id=sid, missing_rate=float("nan"), useMatrix=True, verbose=False)
    np.testing.assert_allclose(_tri_full(rm["beta"], 90), z["beta"], rtol=1e-11, atol=1e-13)
    # snpgdsGRM(method="IndivBeta") vs the oracle's CalcIndivBetaGRM restatement
    auto = (hapmap.snp_chromosome >= 1) & (hapmap.snp_chromosome <= 22)
    g = hapmap.read_genotype(snp_sel=auto, samp_sel=np.arange(90))
    g = np.ascontiguousarray(g[orc.select_snp_base(g, True)])
    ref, avg = orc.beta_final_grm(orc.beta_count(g), 90)
    gr = api.snpgdsGRM(hapmap, sample_id=sid, missing_rate=float("nan"), method="IndivBeta", verbose=False)
    np.testing.assert_allclose(gr["grm"], orc.tri_to_full(ref, 90), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(gr["avg_val"], avg, rtol=1e-12)


@pytest.mark.parametrize("solver", ["dense", "krylov"])
def test_EIGMIX_golden(hapmap, solver, monkeypatch):
    """test.EIGMIX, test_rel.R:308-327; `krylov`: gnrEigMix beyond the dense solver's size -- the coancestry matrix is
    finalised in place and the block-Krylov solver runs on the panel (forced here with SNPGPU_EIG_DENSE_MAX)"""
    from snprelate_amd import api
    if solver == "krylov":
        monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "50")
    z = np.load(os.path.join(GOLDEN, "validate_eigmix.npz"))
    sid = hapmap.sample_id[:90]
    r = api.snpgdsEIGMIX(hapmap, sample_id=sid, ibdmat=True, missing_rate=float("nan"), eigen_cnt=8, verbose=False)
    scale = np.abs(z["ibd"]).mean()
    assert np.max(np.abs(r["ibd"] - z["ibd"]) / (np.abs(z["ibd"]) + scale)) < 1e-5
    w = np.linalg.eigvalsh(z["ibd"])[::-1][:8]
    np.testing.assert_allclose(r["eigenval"][:8], w, rtol=1e-4, atol=1e-6)
    assert np.all(np.isnan(r["eigenval"][8:])) and r["eigenvect"].shape == (90, 8)
    # snpgdsGRM(method="EIGMIX") = 2 x the coancestry without the diagonal adjustment
    auto = (hapmap.snp_chromosome >= 1) & (hapmap.snp_chromosome <= 22)
    g = hapmap.read_genotype(snp_sel=auto, samp_sel=np.arange(90))
    g = np.ascontiguousarray(g[orc.select_snp_base(g, True)])
    ref, af = orc.eigmix(g, diagadj=False)
    gr = api.snpgdsGRM(hapmap, sample_id=sid, missing_rate=float("nan"), method="EIGMIX", verbose=False)["grm"]
    ref2 = 2 * orc.tri_to_full(ref, 90)
    assert np.max(np.abs(gr - ref2) / (np.abs(ref2) + np.abs(ref2).mean())) < 1e-5
    np.testing.assert_allclose(r["afreq"], af, rtol=1e-13)


def test_man_page_examples(hapmap, tmp_path):
    """The calls of the reference's man-page examples for this path (man/snpgdsGRM.Rd, snpgdsMergeGRM.Rd,
    snpgdsIBDKING.Rd, snpgdsIBS.Rd, snpgdsIBSNum.Rd; run by inst/unitTests/test_examples.R), checked against the
    oracle.  (The fixture has no sample.annot node: the first 60 samples stand in for the CEU subset.)"""
    from snprelate_amd import api, gds
    auto = (hapmap.snp_chromosome >= 1) & (hapmap.snp_chromosome <= 22)

    def selected(samp, missing_rate):
        g = hapmap.read_genotype(snp_sel=auto, samp_sel=samp)
        return np.ascontiguousarray(g[orc.select_snp_base(g, True, float("nan"), missing_rate)])

    # snpgdsIBS / snpgdsIBSNum with defaults
    g = selected(None, 0.01)
    n = g.shape[1]
    cnt = orc.ibs_count(g)
    ibs = api.snpgdsIBS(hapmap, verbose=False)
    assert np.array_equal(ibs["ibs"], orc.tri_to_full(orc.ibs_ave(cnt, n), n))
    rv = api.snpgdsIBSNum(hapmap, verbose=False)
    assert np.array_equal(rv["ibs0"], orc.tri_to_full(cnt[:, 0].astype(np.int32), n)) and len(rv["snp_id"]) == g.shape[0]

    # snpgdsIBDKING: robust, robust + useMatrix, robust + family.id, homo, homo + useMatrix
    ceu = hapmap.sample_id[:60]
    g = selected(np.arange(60), 0.01)
    kc = orc.king_robust_count(g)
    r0, rk = orc.king_robust_final(kc, 60, None)
    a = api.snpgdsIBDKING(hapmap, sample_id=ceu, verbose=False)
    assert sorted(a) == ["IBS0", "afreq", "kinship", "sample_id", "snp_id"]
    assert np.array_equal(a["kinship"], orc.tri_to_full(rk, 60), equal_nan=True)
    m = api.snpgdsIBDKING(hapmap, sample_id=ceu, useMatrix=True, verbose=False)
    assert np.array_equal(m["IBS0"], r0, equal_nan=True) and np.array_equal(m["kinship"], rk, equal_nan=True)
    fam_names = np.array(["f%d" % (i // 3) for i in range(60)])
    f0, fk = orc.king_robust_final(kc, 60, (np.arange(60) // 3 + 1).astype(np.int32))
    b = api.snpgdsIBDKING(hapmap, sample_id=ceu, family_id=fam_names, verbose=False)
    assert np.array_equal(b["kinship"], orc.tri_to_full(fk, 60), equal_nan=True)
    hc, hf = orc.king_homo_count(g)
    h0, h1 = orc.king_homo_final(hc, hf, 60)
    h = api.snpgdsIBDKING(hapmap, sample_id=ceu, type="KING-homo", verbose=False)
    np.testing.assert_allclose(h["k0"], orc.tri_to_full(h0, 60), rtol=1e-5, atol=1e-7, equal_nan=True)
    hm = api.snpgdsIBDKING(hapmap, sample_id=ceu, type="KING-homo", useMatrix=True, verbose=False)
    np.testing.assert_allclose(hm["k1"], h1, rtol=1e-5, atol=2e-5, equal_nan=True)

    # snpgdsMergeGRM: two halves of the complete SNPs, file and in-memory results
    rf = api.snpgdsSNPRateFreq(hapmap)
    snpid = hapmap.snp_id[rf["MissingRate"] == 0]
    grm = api.snpgdsGRM(hapmap, snp_id=snpid, method="GCTA", verbose=False)
    set1 = grm["snp_id"][:len(grm["snp_id"]) // 2]
    set2 = np.setdiff1d(grm["snp_id"], set1)
    f1, f2, fo = (str(tmp_path / x) for x in ("tmp1.gds", "tmp2.gds", "tmp.gds"))
    api.snpgdsGRM(hapmap, method="GCTA", snp_id=set1, out_fn=f1, verbose=False)
    api.snpgdsGRM(hapmap, method="GCTA", snp_id=set2, out_fn=f2, verbose=False)
    api.snpgdsMergeGRM([f1, f2], fo, verbose=False)
    grm2 = api.snpgdsMergeGRM([f1, f2], verbose=False)
    mfile = gds.read_output(fo)["grm"]
    np.testing.assert_allclose(mfile, grm["grm"], rtol=2e-5, atol=2e-6)      # "~zero"
    np.testing.assert_allclose(mfile, grm2["grm"], rtol=1e-13, atol=1e-15)   # "zero"


def test_gds_stream_blocks_feed_pinned_buffers(hapmap):
    """The streaming GDS reader (snprelate_amd/gds.py: GenoStream) as the feed of the accumulators: HapMap's `genotype`
    node block by block straight into two page-locked 2-bit buffers (no whole-file load, no byte inflation),
    asynchronous SNPGPU_HOST_PINNED feeds -- IBS counts and GCTA GRM equal the oracle's on the whole matrix."""
    from snprelate_amd import _lib
    from snprelate_amd.gds import open_gds_stream
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    n, blk, rb = gs.n_samp, 1500, (gs.n_samp + 3) // 4
    g = hapmap.read_genotype()
    bufs = [_lib.PinnedBuffer((blk, rb)) for _ in range(2)]
    with _lib.Accumulator(_lib.IBS, n, max_block_snps=blk) as a, _lib.Accumulator(_lib.GRM_GCTA, n, max_block_snps=blk) as b:
        turn = 0
        it = gs.blocks(blk, buffers=[p.array for p in bufs])
        while True:
            pb = bufs[turn % 2]
            a.host_wait(pb); b.host_wait(pb)                 # the buffer the reader fills next must have been copied
            try:
                lo, m, rows = next(it)
            except StopIteration:
                break
            a.feed_pinned(pb, m, _lib.GENO_PACKED2)
            b.feed_pinned(pb, m, _lib.GENO_PACKED2)
            turn += 1
        i0, i1, i2 = a.ibs_num(packed=True)
        grm = b.grm_gcta(packed=True)
    ref = orc.ibs_count(g)
    assert np.array_equal(np.stack([i0, i1, i2], 1).astype(np.uint32), ref)
    rg = orc.grm_gcta(g)
    assert np.nanmax(np.abs(grm - rg) / (np.abs(rg) + np.nanmedian(np.abs(rg)))) < 1e-5
    for p in bufs:
        p.free()
