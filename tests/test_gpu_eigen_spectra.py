"""Every route to the top-k eigen solver on multiple and clustered eigenvalues (tests/eigen_spectra.py): the block-Krylov solver
behind snpgpu_panels_topk_eigen with all its switches, the dense route, snpgpu_multi_topk_eigen, snpgdsPCA / snpgdsEIGMIX, the SVD
at the end of the randomised PCA -- and a fixed sweep of tools/fuzz_eigen.py's generic spectra through the same comparison.

The reference of every case is numpy's eigh of the DEVICE's own gathered matrix, so what is tested is the solver: eigenvalues with
their multiplicity (a missed copy moves a value by a whole cluster gap), residuals, orthonormality of the returned vectors, and
cluster subspaces -- every vector is checked, none is masked because its eigenvalue has a neighbour.  The solver's own fp64 residual
check cannot see a missed copy, a vector returned twice or a loss of orthogonality inside a cluster; these tests can
(tests/test_cpu_eigen_spectra.py plants each of them)."""
import functools

import numpy as np
import pytest

import eigen_spectra as E
import oracle as orc
from conftest import synth_geno

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 7, 16)
KINDS = ("PCA_COV", "GRM_GCTA", "EIGMIX")
DATA = [("n140", False), ("n210", False), ("n540", False), ("n210", True), ("n540", True)]
DATA_IDS = ["%s%s" % (name, "-near" if near else "") for name, near in DATA]

# route: (row panels asked for, environment, arguments of topk_eigen)
LARGE_N = {"SNPGPU_EIG_CHOLQR_MIN_N": "0", "SNPGPU_EIG_GRAM_CHUNK": "128"}
ROUTES = {
    "one_panel": (1, {}, {}),
    "three_panels": (3, {}, {}),
    "fp64_products": (3, {}, {"fp32_until": -1.0}),
    # the all-fp64 phase by its switch, and fp32 products that convert the fp64 plane on the fly: the form the solver takes by itself
    # when the device has no room for the fp32 copy of the plane (eigen.hip, ctx_panel_matmul_enqueue) -- at these sizes only the
    # switches reach them
    "fp64_phase_by_switch": (3, {"SNPGPU_EIG_FP32": "0"}, {}),
    "fp32_without_the_copy": (3, {"SNPGPU_EIG_F32_PANEL": "0"}, {}),
    "no_mixed_cycles": (3, {"SNPGPU_EIG_MIXED": "0"}, {}),
    "rocblas_products": (3, {"SNPGPU_EIG_BLAS": "1"}, {}),
    "large_n_algebra": (3, LARGE_N, {}),
    "depth6_thick_restart": (3, {}, {"depth": 6}),
    "depth6_keep1": (3, {"SNPGPU_EIG_KEEP": "1"}, {"depth": 6}),
}


@functools.lru_cache(maxsize=None)
def _geno(name, near):
    g = E.size_geno(name, near)[0]
    g.setflags(write=False)
    return g


def _close(panels):
    for a in panels:
        a.close()


def _solve(op, k, **kw):
    from snprelate_amd.eigen import topk_eigen
    w, v, info = topk_eigen(op, k, **kw)
    return w.cpu().numpy(), v.cpu().numpy(), info


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,near", DATA, ids=DATA_IDS)
def test_krylov_routes(name, near, kind, route, monkeypatch):
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.eigen import PanelOperator
    world, env, kw = ROUTES[route]
    g = _geno(name, near)
    n = g.shape[1]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    # (below 257 samples every split is one panel; asked for as a panel with a row range all the same)
    panels, rows = E.open_panels(_lib, kind, g, E.three_panels(n) if world == 3 else None)
    try:
        assert len(panels) == (3 if n == 540 and world == 3 else 1)
        full = E.gathered(kind, panels, rows, n)
        ref = E.reference(full)
        op = PanelOperator(panels, n, torch.device("cuda", 0), normalize=(kind == "PCA_COV"))
        for k in KS:
            w, v, info = _solve(op, k, **kw)
            E.check_topk(w, v, full, k, "%s %s %s k=%d (%d products, %d fp32)" % (DATA_IDS[DATA.index((name, near))], kind, route, k,
                                                                                 info["matmuls"], info["matmuls_fp32"]), ref=ref)
            assert info["max_rel_residual"] < 1e-9
            if route in ("fp64_products", "rocblas_products") or env.get("SNPGPU_EIG_FP32") == "0":
                assert info["matmuls_fp32"] == 0
            if env.get("SNPGPU_EIG_F32_PANEL") == "0":
                assert info["matmuls_fp32"] > 0
    finally:
        _close(panels)


def test_fp32_panel_product_without_the_fp32_copy(monkeypatch):
    """snpgpu_pca_panel_matmul_f32 with SNPGPU_EIG_F32_PANEL=0 (the fp64 plane converted on the fly, no fp32 copy beside it) on the
    case and at the bound of test_panel_product_fp32_form (tests/test_gpu_api_golden.py): three row panels of 2331 samples, 53
    vectors, error below 4e-7 of the sum of |terms|.  Whether it equals the copy form bit for bit is printed, not asserted: both
    round the same fp64 entries to fp32, the copy once and this form at every use."""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.dist import panel_rows
    n, L, m = 2331, 900, 53
    g = synth_geno(n, L, missing=0.02, seed=18)
    dev = torch.device("cuda", 0)
    qh = np.random.default_rng(1).normal(size=(m, n)) * (1.0 + np.arange(m)[:, None])
    q = torch.from_numpy(qh).to(dev)
    with _lib.Accumulator(_lib.PCA_COV, n, max_block_snps=1024) as a:
        a.feed(g)
        cov = orc.tri_to_full(a.pca_cov(packed=True, normalize=False)[0], n)
    ref = (qh @ cov) * 0.25
    bounds = panel_rows(n, 3)
    out = {}
    for form in ("copy", "on_the_fly"):
        if form == "on_the_fly":
            monkeypatch.setenv("SNPGPU_EIG_F32_PANEL", "0")
        y = torch.zeros_like(q)
        for r in range(3):
            with _lib.Accumulator(_lib.PCA_COV, n, row_begin=bounds[r], row_end=bounds[r + 1], max_block_snps=1024) as a:
                a.feed(g)
                torch.cuda.synchronize()
                a.pca_panel_matmul(0.25, q.data_ptr(), m, y.data_ptr(), fp32=True)
                torch.cuda.synchronize()
        out[form] = y.cpu().numpy()
    bound = 0.25 * (np.abs(qh) @ np.abs(cov))
    err = {form: float((np.abs(y - ref) / bound).max()) for form, y in out.items()}
    print("fp32 panel product: error / sum |terms| copy %.2e on the fly %.2e (bound 4e-7); bit-equal to the copy form: %s"
          % (err["copy"], err["on_the_fly"], np.array_equal(out["copy"], out["on_the_fly"])), flush=True)
    assert err["on_the_fly"] < 4e-7 and err["copy"] < 4e-7, err
    assert err["on_the_fly"] > 1e-12                                      # it IS an fp32 form


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,block", [("n210", 2), ("n540", 2), ("n140", 1)])
def test_block_smaller_than_the_multiplicity(name, block, kind):
    """One Krylov space of block width b holds at most b copies of a multiple eigenvalue in exact arithmetic.  Asking for a block of
    2 on triples (1 on doubles): either the answer passes the whole comparison or the call fails with the solver's "not converged"
    error -- never the next cluster's value in place of the missing copy.  (The solver widens the block to k, so k = 1 and 2 are the
    requests whose block stays below the multiplicity; k = 3 and 4 run with the block they get.)"""
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.eigen import PanelOperator
    g = _geno(name, False)
    n = g.shape[1]
    panels, rows = E.open_panels(_lib, kind, g, E.three_panels(n))
    try:
        full = E.gathered(kind, panels, rows, n)
        ref = E.reference(full)
        op = PanelOperator(panels, n, torch.device("cuda", 0), normalize=(kind == "PCA_COV"))
        for k in (1, 2, 3, 4):
            try:
                w, v, info = _solve(op, k, block=block)
            except _lib.SnpGpuError as e:
                assert "not converged" in str(e), e
                print("%s %s block=%d k=%d: refused: %s" % (name, kind, block, k, e), flush=True)
                continue
            assert info["block"] == max(block, k)
            E.check_topk(w, v, full, k, "%s %s block=%d k=%d (%d restarts, %d products)" % (name, kind, info["block"], k, info["restarts"],
                                                                                          info["matmuls"]), ref=ref)
    finally:
        _close(panels)


@pytest.mark.parametrize("name,near", DATA, ids=DATA_IDS)
def test_dense_route_and_the_same_call_forced_to_krylov(name, near, monkeypatch):
    """snpgpu_pca_eigen: hipSOLVER's dense solver on the negated matrix, the same call sent to the Krylov solver with
    SNPGPU_EIG_DENSE_MAX=0, and k = n // 3, which is dense whatever the switch says.  (The dense route used to ask syevdx for the
    index range 1 .. k; on these matrices that returned values from elsewhere in the spectrum with vectors of relative residual 0.4
    to 8, at k = 1 as at k = 16: DESIGN.md 4.5.  It decomposes the whole matrix with syevd now.)"""
    from snprelate_amd import _lib
    g = _geno(name, near)
    n = g.shape[1]
    with _lib.Accumulator(_lib.PCA_COV, n, max_block_snps=1024) as a:
        for i in range(0, g.shape[0], 1024):
            a.feed(g[i:i + 1024])
        full = orc.tri_to_full(a.pca_cov(packed=True, normalize=True)[0], n)
        ref = E.reference(full)
        for forced in (False, True):
            if forced:
                monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "0")
            for k in KS + (n // 3,):
                w, v = a.pca_eigen(k)
                E.check_topk(w, v, full, k, "%s pca_eigen %s k=%d" % (name, "dense" if not forced or k == n // 3 else "krylov", k), ref=ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(E.SIZES))
def test_multi_device_object(name, kind):
    """snpgpu_multi_topk_eigen over listed copies of device 0; the object's own plan makes two panels of 540 samples (0-256, 256-540:
    panel_rows weighs the triangle's rows) and one of the smaller sizes"""
    from snprelate_amd import _lib
    g = _geno(name, False)
    n = g.shape[1]
    with _lib.MultiAccumulator(getattr(_lib, kind), n, devices=(0, 0, 0), panels_per_device=1, max_block_snps=1024) as m:
        assert m.info()["n_panels"] == (2 if n == 540 else 1)
        for i in range(0, g.shape[0], 1024):
            m.feed(g[i:i + 1024])
        m.sync()
        if kind == "PCA_COV":
            tri = m.pca_cov(normalize=True)[0]
        else:
            tri = m.grm_gcta() if kind == "GRM_GCTA" else m.eigmix()
            m.finalize_inplace()
        full = orc.tri_to_full(tri, n)
        ref = E.reference(full)
        for k in KS:
            w, v, info = m.topk_eigen(k, scale=0.0 if kind == "PCA_COV" else 1.0)
            E.check_topk(w, v, full, k, "%s %s multi k=%d (%d products)" % (name, kind, k, info["matmuls"]), ref=ref)


@pytest.mark.parametrize("solver", ["dense", "krylov"])
@pytest.mark.parametrize("fn", ["snpgdsPCA", "snpgdsEIGMIX"])
@pytest.mark.parametrize("name", list(E.SIZES))
def test_api(name, fn, solver, monkeypatch):
    """snpgdsPCA / snpgdsEIGMIX on the genotypes, against the matrix the same call returns (genmat / ibd)"""
    from snprelate_amd import api, gds
    if solver == "krylov":
        monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "50")
    g = _geno(name, False)
    n = g.shape[1]
    f = gds.GenoFile(genotype=g)
    common = dict(autosome_only=False, remove_monosnp=False, missing_rate=float("nan"), verbose=False)
    for k in KS:
        if fn == "snpgdsPCA":
            r = api.snpgdsPCA(f, eigen_cnt=k, need_genmat=True, **common)
            full = r["genmat"]
        else:
            r = api.snpgdsEIGMIX(f, eigen_cnt=k, ibdmat=True, **common)
            full = r["ibd"]
        assert r["eigenvect"].shape == (n, k) and np.all(np.isnan(r["eigenval"][k:]))
        E.check_topk(r["eigenval"][:k], r["eigenvect"], full, k, "%s %s %s k=%d" % (name, fn, solver, k))


@pytest.mark.parametrize("aux,it", [(8, 4), (24, 10)])
@pytest.mark.parametrize("name,near", [("n210", False), ("n210", True)], ids=["n210", "n210-near"])
def test_randomized_pca(name, near, aux, it):
    """snpgdsPCA(algorithm="randomized") against oracle.pca_randomized from the same start matrix, both SVD branches
    (n = 210 >= 8 * 5 and < 24 * 11): TraceXTX and the eigenvalues at the bounds of test_randomized_pca_vs_oracle, the vectors by
    cluster subspace -- the oracle's own values say which of them form a cluster"""
    from snprelate_amd import api, gds
    g = _geno(name, near)
    n, k = g.shape[1], 6
    assert (n >= aux * (it + 1)) == (aux == 8)
    aux_mat = np.random.default_rng(7).normal(size=(aux, n))
    r = api.snpgdsPCA(gds.GenoFile(genotype=g), autosome_only=False, remove_monosnp=False, missing_rate=float("nan"), algorithm="randomized",
                      eigen_cnt=k, aux_dim=aux, iter_num=it, aux_mat=aux_mat, verbose=False)
    sig, vt, tr2 = orc.pca_randomized(g, aux_mat, it)
    all_val = (n - 1) * 2 * sig ** 2 / tr2
    V = r["eigenvect"]
    cl, cut = E.clusters(all_val, k)
    inside = span = 1.0
    for lo, hi in cl:
        coef = vt[lo:hi] @ V[:, lo:min(hi, k)]
        inside = min(inside, float(np.linalg.norm(coef, axis=0).min()))
        if hi <= k:
            span = min(span, float(np.linalg.svd(coef, compute_uv=False).min()))
    ortho = float(np.abs(V.T @ V - np.eye(k)).max())
    print("%s randomized aux=%d it=%d: TraceXTX %.1e eigenvalues %.1e orthonormality %.1e in-cluster %.1e span %.1e; clusters %s"
          % (name, aux, it, abs(r["TraceXTX"] / tr2 - 1), np.abs(r["eigenval"][:k] / all_val[:k] - 1).max(), ortho, 1 - inside, 1 - span, cl),
          flush=True)
    np.testing.assert_allclose(r["TraceXTX"], tr2, rtol=1e-12)
    np.testing.assert_allclose(r["eigenval"][:k], all_val[:k], rtol=1e-7)
    assert V.shape == (n, k)
    assert inside >= 1 - E.SUBSPACE_BOUND and span >= 1 - E.SUBSPACE_BOUND


# twelve cases of tools/fuzz_eigen.py's generator, one seed each
FUZZ_SEEDS = (101, 102, 103, 113, 105, 106, 107, 108, 109, 110, 111, 112)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_sweep(seed):
    import torch
    from snprelate_amd import _lib
    from snprelate_amd.dist import panel_rows
    from snprelate_amd.eigen import PanelOperator
    c = E.fuzz_case(np.random.default_rng(seed), synth_geno)
    n, k, kind = c["n"], c["k"], c["kind"]
    panels, rows = E.open_panels(_lib, kind, c["g"], panel_rows(n, c["world"]) if c["world"] > 1 else None, c["blk"])
    try:
        full = E.gathered(kind, panels, rows, n)
        assert np.isfinite(full).all()
        op = PanelOperator(panels, n, torch.device("cuda", 0), normalize=(kind == "PCA_COV"))
        w, v, info = _solve(op, k)
        E.check_topk(w, v, full, k, "fuzz %d %s n=%d L=%d k=%d miss=%.2f panels=%d (%d products)" % (seed, kind, n, c["L"], k, c["miss"],
                                                                                                  len(panels), info["matmuls"]))
    finally:
        _close(panels)
