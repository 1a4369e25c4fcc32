"""CPU-side tests of the LD feature (snpgdsLDMat): the library exports the LD entry points, the numpy reference helper
(tests/ld_ref.py) agrees with the definition the reference's own unit test uses, and the result dimensions follow gnrLDMat."""
import os
import re

import numpy as np
import pytest

import ld_ref
from snprelate_amd import _lib
from snprelate_amd.gds import unpack_2bit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_SYMBOLS = ["snpgpu_ld_create", "snpgpu_ld_destroy", "snpgpu_ld_out_dims", "snpgpu_ld_feed", "snpgpu_ld_result",
              "snpgpu_ld_set_timing", "snpgpu_ld_get_timing", "snpgpu_ld_pair_tables", "snpgpu_gnrLDMat"]


def test_library_exports_the_ld_symbols():
    hdr = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    for s in LD_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsnpgpu.so not built")
    L = _lib.lib()
    assert all(hasattr(L, s) for s in LD_SYMBOLS)
    assert L.snpgpu_abi_version() == 2


def test_product_path_does_not_import_ld_ref():
    for dp, _, files in os.walk(os.path.join(ROOT, "snprelate_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "ld_ref" not in open(os.path.join(dp, f)).read(), f


def test_ld_ref_cov_corr_equal_pairwise_complete_on_hapmap(hapmap):
    """inst/unitTests/test_LD.R: cov / corr of the first 1000 SNPs = cov / cor(use = "pairwise.complete.obs")"""
    g = unpack_2bit_rows(hapmap.packed[:1000], hapmap.n_samp)
    assert (g == 3).any()
    cov, cor = ld_ref.pairwise_complete(g)
    t = ld_ref.tables(g)
    got_cov = ld_ref.ld_values(t, "cov")
    got_cor = ld_ref.ld_values(t, "corr")
    assert np.array_equal(np.isnan(got_cov), np.isnan(cov))
    assert np.array_equal(np.isnan(got_cor), np.isnan(cor))
    np.testing.assert_allclose(got_cov, cov, rtol=1e-12, atol=1e-13, equal_nan=True)
    np.testing.assert_allclose(got_cor, cor, rtol=1e-12, atol=1e-13, equal_nan=True)
    # the diagonal of cov is the sample variance over the calls
    d = np.array([np.var(r[r < 3], ddof=1) if (r < 3).sum() > 1 else np.nan for r in g])
    np.testing.assert_allclose(np.diag(got_cov), d, rtol=1e-12, equal_nan=True)


def test_ld_ref_tables_and_methods_on_small_cases():
    g = np.array([[0, 1, 2, 3, 1, 2, 0], [0, 1, 2, 2, 3, 1, 0], [1, 1, 1, 1, 1, 1, 3]], np.uint8)
    t = ld_ref.tables(g)
    assert t[0, 1].tolist() == [[2, 0, 0], [0, 1, 0], [0, 1, 1]]
    assert t[0, 1].sum() == 5 and (t[1, 0] == t[0, 1].T).all()
    v = ld_ref.ld_values(t, "corr")
    assert np.isnan(v[2]).all()                    # monomorphic SNP: zero variance
    v = ld_ref.ld_values(t, "dprime")
    assert np.all(np.abs(v[:2, :2]) <= 1 + 1e-12)
    r = ld_ref.ld_values(t, "r")
    np.testing.assert_allclose(np.diag(r)[:2], 1.0, rtol=1e-9)
    e = np.zeros((3, 3), np.int64)
    for m in ld_ref.METHODS:
        assert np.isnan(ld_ref.ld_values(e, m))    # no sample called at both SNPs


@pytest.mark.parametrize("n_snp,slide,trim,dims", [
    (100, -1, False, (100, 100)), (100, 0, True, (100, 100)), (100, 10, False, (10, 100)), (100, 10, True, (10, 90)),
    (100, 250, False, (100, 100)), (100, 250, True, (100, 0)), (100, 100, True, (100, 0)), (1, 5, False, (1, 1)),
])
def test_output_dims_follow_gnrLDMat(n_snp, slide, trim, dims):
    assert _lib.ld_out_dims(n_snp, slide, trim) == dims
    assert ld_ref.out_dims(n_snp, slide, trim) == dims
    g = np.random.default_rng(1).integers(0, 4, (n_snp, 9)).astype(np.uint8)
    assert ld_ref.ld_mat(g, "cov", slide, trim).shape == dims


def test_band_layout_of_ld_ref():
    g = np.random.default_rng(2).integers(0, 4, (30, 50)).astype(np.uint8)
    full = ld_ref.ld_mat(g, "composite")
    band = ld_ref.ld_mat(g, "composite", 7, False)
    for k in range(1, 8):
        for i in range(30):
            if i + k < 30:
                assert band[k - 1, i] == full[i, i + k] or (np.isnan(band[k - 1, i]) and np.isnan(full[i, i + k]))
            else:
                assert np.isnan(band[k - 1, i])
    assert np.array_equal(ld_ref.ld_mat(g, "composite", 7, True), band[:, :23], equal_nan=True)
