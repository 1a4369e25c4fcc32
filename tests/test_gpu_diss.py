"""GPU tests of the individual dissimilarity (snpgdsDiss -> SNPGPU_DISS contexts): the MX-fp4 SumGeno counter bit for bit against
the numpy restatement (tests/diss_ref.py) and against the KING-robust counters on the same feeds, the weight sums and the finished
matrix against the restatement, the denominator against KING-homo's, the Python API on HapMap, the working-space mirror, the
multi-context gather and one size test at N = 100 000."""
import numpy as np
import pytest

import diss_ref as R
from oracle.synth import synth_geno
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

pytestmark = pytest.mark.gpu


def _feed(a, g, blk, how="host", fmt=_lib.GENO_U8):
    for s in range(0, g.shape[0], blk):
        x = np.ascontiguousarray(g[s:s + blk])
        if fmt == _lib.GENO_PACKED2:
            x = pack_2bit_rows(x)
        if how == "host":
            a.feed(x, fmt)
        elif how == "pinned":
            buf = _lib.PinnedBuffer(x.shape)
            buf.array[...] = x
            a.feed_pinned(buf, x.shape[0], fmt)
            a.host_wait(buf)
            a.sync()
            buf.free()
        else:
            import torch
            d = torch.from_numpy(x).to("cuda:0")
            torch.cuda.synchronize()
            a.feed_device(d.data_ptr(), x.shape[0], fmt)
            a.sync()
            del d


def _mixed(n, L, missing, seed, clean_blocks=(), blk=None):
    g = synth_geno(n, L, missing=missing, seed=seed, special=missing > 0)
    for b in clean_blocks:                                   # a block without missing calls: its gaps become called genotypes
        sl = g[b * blk:(b + 1) * blk]
        sl[sl > 2] = (np.arange((sl > 2).sum()) % 3).astype(np.uint8)
    return g


def _run(kind, n, g, blk, **kw):
    with _lib.Accumulator(kind, n, max_block_snps=blk, **kw) as a:
        _feed(a, g, blk)
        return a.diss_sums() if kind == _lib.DISS else a.king_robust_counts()


def _rtol(g):
    """1e-12 where no block has missing calls (fp64 weight sums), 2e-6 otherwise (the fp16 u.v factors of the weight product)"""
    return 2e-6 if (g > 2).any() else 1e-12


def _panel_slice(n, r0, r1):
    return slice(r0 * n - r0 * (r0 - 1) // 2, r1 * n - r1 * (r1 - 1) // 2)


CASES = [                       # (n, L, missing, blk, blocks without missing calls)
    (300, 1500, 0.0, 1024, ()),
    (517, 2049, 0.002, 700, ()),
    (333, 3001, 0.02, 1024, ()),
    (129, 777, 0.3, 300, ()),
    (611, 3000, 0.02, 1000, (0, 2)),          # blocks with and without missing calls in one stream
]


@pytest.mark.parametrize("n, L, missing, blk, clean", CASES)
def test_sum_geno_bit_exact(n, L, missing, blk, clean):
    g = _mixed(n, L, missing, 17 + n, clean, blk)
    sg, sa = _run(_lib.DISS, n, g, blk)
    rsg, rsa = R.diss_sums(g)
    assert np.array_equal(sg.astype(np.int64), R.packed_upper(rsg))
    # second route: 2 (2 ibs0) + ibs1 + N1_Aa + N2_Aa = SumSq + N1_Aa + N2_Aa of the KING-robust counters on the same feeds
    k = _run(_lib.KING_ROBUST, n, g, blk).astype(np.int64)
    assert np.array_equal(sg.astype(np.int64), k[:, 2] + k[:, 3] + k[:, 4])
    np.testing.assert_allclose(sa, R.packed_upper(rsa), rtol=_rtol(g), atol=1e-9)


@pytest.mark.parametrize("n, L, missing, blk, clean", CASES)
def test_diss_matrix(n, L, missing, blk, clean):
    g = _mixed(n, L, missing, 29 + n, clean, blk)
    with _lib.Accumulator(_lib.DISS, n, max_block_snps=blk) as a:
        _feed(a, g, blk)
        full = a.diss(packed=False)
        packed = a.diss(packed=True)
    np.testing.assert_allclose(full, R.diss_matrix(g), rtol=_rtol(g), equal_nan=True)
    assert np.array_equal(full, full.T, equal_nan=True)
    assert np.array_equal(packed, R.packed_upper(full), equal_nan=True)


@pytest.mark.parametrize("how, fmt", [("host", _lib.GENO_PACKED2), ("pinned", _lib.GENO_U8), ("device", _lib.GENO_PACKED2),
                                      ("device", _lib.GENO_U8)])
def test_feeds_and_formats(how, fmt):
    n, L, blk = 401, 1300, 512
    g = _mixed(n, L, 0.02, 5, (1,), blk)
    with _lib.Accumulator(_lib.DISS, n, max_block_snps=blk) as a:
        _feed(a, g, blk, how, fmt)
        sg, _ = a.diss_sums()
        d = a.diss(packed=True)
    assert np.array_equal(sg.astype(np.int64), R.packed_upper(R.diss_sums(g)[0]))
    np.testing.assert_allclose(d, R.packed_upper(R.diss_matrix(g)), rtol=2e-6, equal_nan=True)


def test_edge_samples_and_snps():
    """a sample without calls (NaN row and column), an all-missing SNP, monomorphic SNPs, a ragged tail"""
    n, L, blk = 260, 1031, 512
    g = synth_geno(n, L, missing=0.01, seed=44)
    g[:, 7] = 3
    g[100] = 3
    g[200] = 0
    g[300] = 2
    with _lib.Accumulator(_lib.DISS, n, max_block_snps=blk) as a:
        _feed(a, g, blk)
        sg, _ = a.diss_sums()
        d = a.diss()
    assert np.array_equal(sg.astype(np.int64), R.packed_upper(R.diss_sums(g)[0]))
    np.testing.assert_allclose(d, R.diss_matrix(g), rtol=2e-6, equal_nan=True)
    assert np.isnan(d[7]).all() and np.isnan(d[:, 7]).all()


@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_row_panels(missing):
    n, L, blk = 700, 2000, 1024
    g = synth_geno(n, L, missing=missing, seed=61, special=missing > 0)
    rsg = R.packed_upper(R.diss_sums(g)[0])
    want = R.packed_upper(R.diss_matrix(g))
    for r0, r1 in [(0, 256), (256, 512), (512, 700)]:
        with _lib.Accumulator(_lib.DISS, n, row_begin=r0, row_end=r1, max_block_snps=blk) as a:
            _feed(a, g, blk)
            sg, _ = a.diss_sums()
            d = a.diss(packed=True)
            with pytest.raises(_lib.SnpGpuError, match="full"):
                a.diss(packed=False)
        sl = _panel_slice(n, r0, r1)
        assert np.array_equal(sg.astype(np.int64), rsg[sl])
        np.testing.assert_allclose(d, want[sl], rtol=_rtol(g), equal_nan=True)


@pytest.mark.parametrize("missing", [0.0, 0.05])
def test_denominator_is_8_times_king_homo_weight_sum(missing):
    """KING-homo's first masked weight sum S, recovered from its (k0, k1) and the KING counters of the same feeds:
    theta = (2 - 2 k0 - k1) / 4 = 0.5 - SumSq / (8 S), so 8 S = SumSq / (0.5 - theta) is the dissimilarity's SumAFreq"""
    n, L, blk = 300, 2500, 1024
    g = synth_geno(n, L, missing=missing, seed=71, special=missing > 0)
    _, sa = _run(_lib.DISS, n, g, blk)
    k = _run(_lib.KING_ROBUST, n, g, blk).astype(np.float64)
    with _lib.Accumulator(_lib.KING_HOMO, n, max_block_snps=blk) as a:
        _feed(a, g, blk)
        k0, k1 = a.king_homo(packed=True)
    theta = (2 - 2 * k0 - k1) / 4
    off = np.ones(sa.size, bool)
    off[np.cumsum(np.r_[0, np.arange(n, 1, -1)])] = False          # KING-homo leaves its diagonal at 0
    ok = off & (k[:, 2] > 0) & np.isfinite(theta)
    assert ok.sum() > sa.size // 2
    np.testing.assert_allclose(sa[ok], k[ok, 2] / (0.5 - theta[ok]), rtol=1e-9)


def _selected_genotypes(gf, sample_id, snp_id):
    """u8 [n_snp][n_samp] of the selected samples / SNPs from the file's genotypes"""
    sid = {v: i for i, v in enumerate(np.asarray(gf.sample_id).tolist())}
    mid = {v: i for i, v in enumerate(np.asarray(gf.snp_id).tolist())}
    ps = np.array([sid[v] for v in np.asarray(sample_id).tolist()])
    pm = np.array([mid[v] for v in np.asarray(snp_id).tolist()])
    full = unpack_2bit_rows(gf.packed, gf.n_samp)
    return np.ascontiguousarray(full[np.ix_(pm, ps)])


@pytest.mark.parametrize("subset", [False, True])
def test_hapmap_api(hapmap, subset):
    kw = {}
    if subset:
        kw = dict(sample_id=np.asarray(hapmap.sample_id)[::3][:50], snp_id=np.asarray(hapmap.snp_id)[::2])
    r = api.snpgdsDiss(hapmap, verbose=False, **kw)
    n = len(r["sample_id"])
    assert set(r) == {"sample_id", "snp_id", "diss"} and r["diss"].shape == (n, n)
    if subset:
        assert n == 50 and len(r["snp_id"]) <= len(kw["snp_id"])
    g = _selected_genotypes(hapmap, r["sample_id"], r["snp_id"])
    np.testing.assert_allclose(r["diss"], R.diss_matrix(g), rtol=2e-6, equal_nan=True)
    assert np.array_equal(r["diss"], r["diss"].T, equal_nan=True)


def test_hapmap_verbose_line(hapmap, capsys):
    api.snpgdsDiss(hapmap, verbose=True)
    assert "Individual dissimilarity analysis on genotypes:" in capsys.readouterr().out


def test_workspace_mirror(hapmap):
    ws = api._init_file2(None, hapmap, None, None, True, True, float("nan"), 0.01, 1, False, 0)
    n = ws["n_samp"]
    out = np.empty((n, n))
    _lib.check(_lib.lib().snpgpu_gnrDiss(1, 0, _lib._ptr(out)))
    g = _selected_genotypes(hapmap, ws["sample_id"], ws["snp_id"])
    np.testing.assert_allclose(out, R.diss_matrix(g), rtol=2e-6, equal_nan=True)


def test_multi_listed_copies_of_one_device():
    n, L, blk = 600, 2000, 1024
    g = synth_geno(n, L, missing=0.02, seed=83)
    with _lib.Accumulator(_lib.DISS, n, max_block_snps=blk) as a:
        _feed(a, g, blk)
        one = a.diss(packed=True)
    with _lib.MultiAccumulator(_lib.DISS, n, devices=(0, 0), max_block_snps=blk) as m:
        for s in range(0, L, blk):
            m.feed(g[s:s + blk])
        got = m.diss()
    np.testing.assert_allclose(got, one, rtol=1e-12, equal_nan=True)


def test_wrong_kind_is_refused():
    with _lib.Accumulator(_lib.KING_HOMO, 64) as a:
        with pytest.raises(_lib.SnpGpuError, match="wrong context kind"):
            a.diss()
    with _lib.Accumulator(_lib.DISS, 64) as a:
        with pytest.raises(_lib.SnpGpuError, match="wrong context kind"):
            a.king_homo()


def _weights_from_packed(host, n):
    """w = 8 F (1 - F) per SNP from 2-bit rows [L][ceil(n / 4)], a few thousand samples at a time"""
    L = host.shape[0]
    s = np.zeros(L, np.int64)
    c = np.zeros(L, np.int64)
    for b0 in range(0, host.shape[1], 2048):
        byte = host[:, b0:b0 + 2048]
        for k in range(4):
            real = (np.arange(b0, b0 + byte.shape[1]) * 4 + k) < n
            v = ((byte >> (2 * k)) & 3)[:, real]
            ok = v < 3
            s += np.where(ok, v, 0).sum(1, dtype=np.int64)
            c += ok.sum(1)
    f = np.where(c > 0, s / np.maximum(2 * c, 1), 0.0)
    return 8 * f * (1 - f)


def test_size_panel_n100k():
    """N = 100 000, a 512-row panel, 16 384 SNPs with 2 % missing fed from device memory; a seeded sample of 200 rows x 2 000
    columns of the panel, the diagonal entries of those rows included, against the restatement"""
    import torch
    n, L, r0, r1 = 100_000, 16_384, 25_600, 26_112
    buf = torch.empty((L, (n + 3) // 4), dtype=torch.uint8, device="cuda:0")
    _lib.synth_block(buf.data_ptr(), n, 0, L, 1234, missing=0.02)
    with _lib.Accumulator(_lib.DISS, n, row_begin=r0, row_end=r1, max_block_snps=L) as a:
        a.feed_device(buf.data_ptr(), L, _lib.GENO_PACKED2)
        a.sync()
        d = a.diss(packed=True)
        sg, _ = a.diss_sums()
    host = buf.cpu().numpy()
    del buf
    rng = np.random.default_rng(7)
    rows = np.sort(rng.choice(np.arange(r0, r1), 200, replace=False))
    cols = np.unique(np.concatenate([rng.choice(np.arange(r0, n), 2000, replace=False), rows]))
    need = np.unique(np.concatenate([rows, cols]))
    g = ((host[:, need >> 2] >> (2 * (need & 3)).astype(np.uint8)) & 3).astype(np.uint8)      # [L][len(need)]
    w = _weights_from_packed(host, n)                       # the weights need every sample of the block
    ri, ci = np.searchsorted(need, rows), np.searchsorted(need, cols)
    called = g < 3
    gi = np.where(called, g, 0).astype(np.int64)
    hi = np.where(called, 2 - gi, 0)
    ca = called.astype(np.float64)
    rsg = gi[:, ri].T @ hi[:, ci] + hi[:, ri].T @ gi[:, ci]
    rsa = (ca[:, ri] * w[:, None]).T @ ca[:, ci]
    with np.errstate(invalid="ignore", divide="ignore"):
        want = rsg / rsa
    diag = rows[:, None] == cols[None, :]
    want[diag] *= 2
    I, J = np.meshgrid(rows, cols, indexing="ij")
    upper = J >= I
    idx = (I * n - I * (I - 1) // 2 + (J - I)) - (r0 * n - r0 * (r0 - 1) // 2)
    assert diag.sum() == 200 and upper.sum() > 100_000
    assert np.array_equal(sg[idx[upper]].astype(np.int64), rsg[upper])
    np.testing.assert_allclose(d[idx[upper]], want[upper], rtol=2e-6, equal_nan=True)
