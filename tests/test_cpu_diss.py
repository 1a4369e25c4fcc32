"""CPU-side tests of the individual dissimilarity (snpgdsDiss): the numpy restatement (tests/diss_ref.py) against the loop-by-loop
transcription of _Do_Diss_ReadBlock / _Do_Diss_Compute / gnrDiss, the KING-counter identity the GPU tests use as a second route, the
library's exports, the R shim's registration and the no-GPU failure mode."""
import ctypes
import os
import re

import numpy as np
import pytest

import diss_ref as R
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISS_SYMBOLS = ["snpgpu_diss", "snpgpu_diss_sums", "snpgpu_gnrDiss", "snpgpu_multi_diss"]


def _edge_genotypes(n=9, m=23, seed=3):
    """m SNPs (not a multiple of 4), an all-missing SNP, monomorphic SNPs, a sample without any call, 10 % missing elsewhere"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, (m, n)).astype(np.uint8)
    g[rng.random((m, n)) < 0.1] = 3
    g[4] = 3                       # all missing
    g[7] = 0                       # monomorphic (weight 0)
    g[11] = 2
    g[:, 5] = 3                    # a sample with no call: NaN on its row and column
    return g


@pytest.mark.parametrize("block", [1, 4, 7, 64])
def test_restatement_matches_loop_transcription(block):
    g = _edge_genotypes()
    want, wsg, wsa = R.gnr_diss_loops(g, block_snps=block)
    sg, sa = R.diss_sums(g)
    assert np.array_equal(sg, wsg)
    np.testing.assert_allclose(sa, wsa, rtol=1e-13, atol=1e-13)
    got = R.diss_matrix(g)
    np.testing.assert_allclose(got, want, rtol=1e-12, equal_nan=True)
    assert np.isnan(got[5]).all() and np.isnan(got[:, 5]).all()        # 0 / 0
    assert np.array_equal(got, got.T, equal_nan=True)


def test_diagonal_counts_hets():
    g = _edge_genotypes()
    sg, _ = R.diss_sums(g)
    assert np.array_equal(np.diag(sg), 2 * (g == 1).sum(axis=0))


def test_unguarded_division():
    # two samples, one SNP: called pair at a monomorphic SNP -> 0 / 0; a het pair at a monomorphic one cannot exist, but x / 0 does
    # once the only polymorphic SNP of a pair is missing for one of them
    g = np.array([[0, 0], [1, 3]], np.uint8)
    d = R.diss_matrix(g)
    assert np.isnan(d[0, 1]) and np.isnan(d[1, 1])
    g = np.array([[1, 1, 0], [3, 1, 1]], np.uint8)     # SNP 0: F = 1/3; SNP 1: all het, F = 1/2
    sg, sa = R.diss_sums(g)
    assert sg[0, 1] == 2 and sa[0, 1] == pytest.approx(8 / 3 * (2 / 3))


def test_rows_and_columns_subset():
    g = _edge_genotypes(n=13, m=31, seed=8)
    full = R.diss_matrix(g)
    rows, cols = np.array([2, 5, 11]), np.array([0, 2, 7, 11, 12])
    np.testing.assert_array_equal(R.diss_matrix(g, rows, cols), full[np.ix_(rows, cols)])
    assert np.array_equal(R.packed_upper(full), full[np.triu_indices(13)], equal_nan=True)


def test_king_counter_identity():
    """SumGeno = 2 (2 ibs0) + ibs1 + N1_Aa + N2_Aa with the KING-robust counters over the SNPs both samples are called at"""
    rng = np.random.default_rng(12)
    g = rng.integers(0, 3, (301, 17)).astype(np.uint8)
    g[rng.random(g.shape) < 0.05] = 3
    c = (g < 3).astype(np.int64)
    e = [((g == k) & (g < 3)).astype(np.int64) for k in range(3)]
    ibs0 = e[0].T @ e[2] + e[2].T @ e[0]
    het_i = e[1].T @ c                        # row het, column called
    het_j = c.T @ e[1]
    ibs1 = het_i + het_j - 2 * (e[1].T @ e[1])
    sg, _ = R.diss_sums(g)
    assert np.array_equal(sg, 2 * (2 * ibs0) + ibs1 + het_i + het_j)


def test_snp_weights_equal_king_homo_first_weight_times_8():
    rng = np.random.default_rng(4)
    g = rng.integers(0, 3, (200, 31)).astype(np.uint8)
    g[rng.random(g.shape) < 0.2] = 3
    s = np.where(g < 3, g, 0).sum(1)
    num = (g < 3).sum(1)
    p = np.where(num > 0, 0.5 * s / np.maximum(num, 1), 0.0)          # src/genKING.cpp:236-246
    assert np.array_equal(R.snp_weights(g), 8 * (p * (1 - p)))


def test_library_exports_the_diss_symbols():
    hdr = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    assert re.search(r"SNPGPU_DISS\s*=\s*8", hdr)
    assert _lib.DISS == 8
    for s in DISS_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsnpgpu.so not built")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in DISS_SYMBOLS:
        assert hasattr(L, s), s


def test_shim_registers_gnrDiss():
    reg = open(os.path.join(ROOT, "r_shim", "registration.inc")).read()
    assert re.search(r'"gnrDiss",\s*\(DL_FUNC\)&gpu_gnrDiss,\s*2', reg)
    assert "gpu_gnrDiss" in open(os.path.join(ROOT, "r_shim", "gpu_shim.cpp")).read()


def _has_gpu():
    try:
        return _lib.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_snpgdsDiss_fails_loudly_without_gpu():
    f = GenoFile(genotype=np.array([[0, 1, 2, 1], [1, 1, 0, 2], [2, 0, 1, 1]], np.uint8))
    with pytest.raises(_lib.SnpGpuError):
        api.snpgdsDiss(f, verbose=False)
    with pytest.raises(_lib.SnpGpuError):
        _lib.Accumulator(_lib.DISS, 16)
