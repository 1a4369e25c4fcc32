"""GPU tests of snpgdsLDMat: exact MX-fp4 genotype tables (snpgpu_ld_pair_tables), the five LD methods in both output forms
against the numpy reference (tests/ld_ref.py), streaming in odd block sizes, invariants, the Python API and a sampled check at
N = 100 000."""
import numpy as np
import pytest

import ld_ref
from input_forms import scramble_padding as _scramble_padding
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import unpack_2bit_rows

pytestmark = pytest.mark.gpu

CODES = {m: i + 1 for i, m in enumerate(ld_ref.METHODS)}


def _synth(n_samp, n_snp, missing, spectrum=0, special=False, seed=7):
    p = synth_hash_block_packed(n_samp, 0, n_snp, seed, missing, spectrum, special)
    return p, unpack_2bit_rows(p, n_samp)


def _run(rows, n_samp, method, slide, trim, blocks=None, max_block=0):
    L = rows.shape[0]
    with _lib.LDMatrix(n_samp, L, CODES[method], slide, trim, max_block_snps=max_block) as ld:
        i = 0
        for b in (blocks or [L]):
            b = min(b, L - i)
            if b > 0:
                ld.feed(rows[i:i + b], _lib.GENO_PACKED2)
            i += b
        if i < L:
            ld.feed(rows[i:], _lib.GENO_PACKED2)
        return ld.result()


def _check(got, ref, method):
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), method
    tol = 1e-6 if method in ("r", "dprime") else 1e-12
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, equal_nan=True)


# ---- 2. bit-exact tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samp", [1, 3, 63, 64, 65, 279, 1000, 70001])
@pytest.mark.parametrize("missing", [0.0, 0.03, 0.3])
def test_pair_tables_bit_exact(n_samp, missing):
    n_a, n_b = (37, 70) if n_samp < 70001 else (21, 45)
    spectrum = 4 if n_samp % 2 else 0
    # rows 0 ... n_a - 1 and 997 ... 997 + n_b - 1 hold planted monomorphic / all-missing SNPs (snp % 997 in {3, 5, 7})
    pa = synth_hash_block_packed(n_samp, 0, n_a, 7, missing, spectrum, True)
    pb = synth_hash_block_packed(n_samp, 997, n_b, 7, missing, spectrum, True)
    ga, gb = unpack_2bit_rows(pa, n_samp), unpack_2bit_rows(pb, n_samp)
    ref = ld_ref.tables(ga, gb)
    got = _lib.ld_pair_tables(_scramble_padding(pa, n_samp), _scramble_padding(pb, n_samp, seed=4), n_samp, fmt=_lib.GENO_PACKED2)
    assert np.array_equal(got, ref)
    assert np.array_equal(_lib.ld_pair_tables(ga, gb, n_samp, fmt=_lib.GENO_U8), ref)      # the same through the unpacked form


# ---- 3. all methods x forms -----------------------------------------------------------------------------------------------------
FORMS = [(-1, False), (1, False), (1, True), (7, False), (7, True), (250, False), (250, True)]


@pytest.mark.parametrize("method", ld_ref.METHODS)
@pytest.mark.parametrize("data", ["spectrum0", "spectrum4", "hapmap"])
def test_methods_and_forms(method, data, hapmap):
    if data == "hapmap":
        rows = np.ascontiguousarray(hapmap.packed[200:520])
        n = hapmap.n_samp
        g = unpack_2bit_rows(rows, n)
    else:
        n = 203
        rows, g = _synth(n, 300, 0.03, spectrum=0 if data == "spectrum0" else 4, special=True)
    for slide, trim in FORMS:
        got = _run(rows, n, method, slide, trim)
        _check(got, ld_ref.ld_mat(g, method, slide, trim), "%s slide=%d trim=%s" % (method, slide, trim))


# ---- 4. streaming ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["composite", "r"])
@pytest.mark.parametrize("slide", [-1, 5, 64, 250])
def test_streaming_block_sizes(slide, method):
    """one feed / odd feed sizes / tiny feeds, the latter two with internal blocks of 128 and 64 rows, so that the halo of
    `slide` rows is carried across many block boundaries"""
    n = 150
    rows, g = _synth(n, 1400, 0.02, spectrum=4, special=True, seed=11)
    one = _run(rows, n, method, slide, False)
    odd = _run(rows, n, method, slide, False, blocks=[1000, 37, 1, 200, 63, 99], max_block=128)
    small = _run(rows, n, method, slide, False, blocks=[3] * 40 + [17, 250], max_block=64)
    assert np.array_equal(one, odd, equal_nan=True)
    assert np.array_equal(one, small, equal_nan=True)
    _check(one, ld_ref.ld_mat(g, method, slide, False), method)


# ---- 5. invariants --------------------------------------------------------------------------------------------------------------
def test_invariants(hapmap):
    rows = np.ascontiguousarray(hapmap.packed[:400])
    n = hapmap.n_samp
    g = unpack_2bit_rows(rows, n)
    poly = np.array([len(np.unique(r[r < 3])) > 1 for r in g])
    for method in ld_ref.METHODS:
        m = _run(rows, n, method, -1, False)
        assert np.array_equal(m, m.T, equal_nan=True), method
        if method in ("corr", "r"):
            np.testing.assert_allclose(np.diag(m)[poly], 1.0, rtol=1e-12 if method == "corr" else 1e-6)
        if method == "cov":
            var = np.array([np.var(r[r < 3], ddof=1) if (r < 3).sum() > 1 else np.nan for r in g])
            np.testing.assert_allclose(np.diag(m), var, rtol=1e-12, equal_nan=True)
        if method == "dprime":
            assert np.nanmax(np.abs(m)) <= 1 + 1e-12


# ---- 1. the reference's own unit test + 6. Python API ---------------------------------------------------------------------------
def test_reference_unit_test_cov_corr(hapmap):
    """inst/unitTests/test_LD.R through api.snpgdsLDMat"""
    snpset = hapmap.snp_id[:1000]
    g = unpack_2bit_rows(hapmap.packed[:1000], hapmap.n_samp)
    cov, cor = ld_ref.pairwise_complete(g)
    c1 = api.snpgdsLDMat(hapmap, snp_id=snpset, method="cov", slide=-1, with_id=False, verbose=False)
    c2 = api.snpgdsLDMat(hapmap, snp_id=snpset, method="corr", slide=-1, with_id=False, verbose=False)
    for got, ref in ((c1, cov), (c2, cor)):
        assert got.shape == (1000, 1000)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-14, equal_nan=True)


def test_api_selection_and_options(hapmap):
    sid = hapmap.sample_id[5:200:2]
    snp = hapmap.snp_id[100:400:3]
    r = api.snpgdsLDMat(hapmap, sample_id=sid, snp_id=snp, slide=20, method="r", verbose=False)
    assert set(r) == {"sample_id", "snp_id", "LD", "slide"}
    assert list(r["sample_id"]) == list(sid) and list(r["snp_id"]) == list(snp) and r["slide"] == 20
    samp = np.isin(hapmap.sample_id, sid)
    snpf = np.isin(hapmap.snp_id, snp)
    g = unpack_2bit_rows(hapmap.packed[snpf], hapmap.n_samp)[:, samp]
    _check(r["LD"], ld_ref.ld_mat(g, "r", 20, False), "r")
    bare = api.snpgdsLDMat(hapmap, sample_id=sid, snp_id=snp, slide=20, method="r", with_id=False, verbose=False)
    assert isinstance(bare, np.ndarray) and np.array_equal(bare, r["LD"], equal_nan=True)
    full = api.snpgdsLDMat(hapmap, snp_id=snp, slide=None, method="composite", verbose=False)
    assert full["LD"].shape == (len(snp), len(snp)) and full["slide"] == -1
    trim = api.snpgdsLDMat(hapmap, snp_id=snp, slide=10, mat_trim=True, method="dprime", verbose=False)
    assert trim["LD"].shape == (10, len(snp) - 10)
    big = api.snpgdsLDMat(hapmap, snp_id=snp, slide=5000, method="cov", verbose=False)
    assert big["slide"] == len(snp) and big["LD"].shape == (len(snp), len(snp))
    with pytest.raises(ValueError):
        api.snpgdsLDMat(hapmap, snp_id=snp, method="lewontin", verbose=False)
    with pytest.raises(TypeError):
        api.snpgdsLDMat(hapmap, snp_id=snp, mat_trim="yes", verbose=False)
    with pytest.raises(TypeError):
        api.snpgdsLDMat(hapmap, snp_id=snp, mat_trim=None, verbose=False)


# ---- 7. scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["composite", "r"])
def test_scale_sampled_pairs(method):
    import torch
    N, L, slide = 100000, 4096, 250
    rb = (N + 3) // 4
    blk = torch.empty(L * rb, dtype=torch.uint8, device="cuda")
    _lib.synth_block(blk.data_ptr(), N, 0, L, seed=5, missing=0.02, spectrum=4, special=True)
    torch.cuda.synchronize()
    with _lib.LDMatrix(N, L, CODES[method], slide, False) as ld:
        for i0 in range(0, L, 1500):
            n = min(1500, L - i0)
            ld.feed_device(blk.data_ptr() + i0 * rb, n)
        got = ld.result()
    host = blk.cpu().numpy().reshape(L, rb)
    rng = np.random.default_rng(9)
    i = rng.integers(0, L - 1, 2000)
    k = rng.integers(1, slide + 1, 2000)
    ok = i + k < L
    i, k = i[ok], k[ok]
    assert i.size >= 1900
    rows = np.unique(np.r_[i, i + k])
    g = unpack_2bit_rows(host[rows], N)
    pos = {r: q for q, r in enumerate(rows)}
    pc = [(g == a).astype(np.int64) for a in range(3)]
    ia = np.array([pos[x] for x in i])
    ib = np.array([pos[x] for x in i + k])
    t = np.empty((i.size, 3, 3), np.int64)
    for a in range(3):
        for b in range(3):
            t[:, a, b] = (pc[a][ia] * pc[b][ib]).sum(1)
    ref = ld_ref.ld_values(t, method)
    _check(got[k - 1, i], ref, method)
    assert np.isnan(got[:, L - 1]).all()
