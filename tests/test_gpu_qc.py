"""GPU tests of the quality-control statistics (snpgdsSampMissRate, snpgdsHWE, snpgdsIndInb).

Counters, missing rates and the five moment methods are compared bit for bit with numpy / the sequential restatement
(tests/inb_ref.py).  HWE: NaN pattern equal and |p_gpu - p_ref| <= 2 (rare_copies / 2 + 2) 2^-53 p_ref (tests/hwe_ref.py: two
orderings of a sum of that many non-negative terms).  MLE: F against the restatement's F at the iteration count the GPU reports,
within MLE_F_TOL, and niter equal wherever the restatement's stopping margin exceeds MLE_FIRM; both figures were measured on the
CPU from the restatement alone (tests/qc_fixtures.py: spread of F 1.4e-14, recorded as 2.0e-14, of |dLogLik| 2.1e-10, recorded as
2.5e-10, over sequential / reversed / pairwise / long double sums; 10 x each is allowed).  Every fixture asserts that at most 10 % of
its margins are not firm.  Besides HapMap and the synthetic set there are a sample at the lower clamp that runs 1 021 sweeps with a
firm margin (its reltol puts the stop midway between two consecutive |dLogLik|, chosen from the restatement alone) and a set run
at a negative reltol, which no |dLogLik| can meet: 10 001 is reported after all 10 000 updates."""
import numpy as np
import pytest

import hwe_ref as H
import inb_ref as R
import qc_fixtures as Q
from input_forms import scramble_padding as _scramble_padding
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

pytestmark = pytest.mark.gpu
MOMENTS = ("mom.weir", "mom.visscher", "gcta1", "gcta2", "gcta3")


def _geno(n, m, missing, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, (m, n)).astype(np.uint8)
    g[rng.random((m, n)) < missing] = 3
    return g


def _np_counts(g):
    return np.stack([(g == k).sum(1) for k in range(3)], 1).astype(np.int32), (g > 2).sum(0).astype(np.int32)


@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 63, 64, 65, 130, 2049])
def test_counters_bit_exact(n, monkeypatch):
    import torch
    for m in (1, 15, 16, 17, 254, 255, 256, 511):                   # around the 16-SNP block unit and the 255-SNP chunk
        g = _geno(n, m, 0.1, seed=n * 1000 + m)
        wc, wm = _np_counts(g)
        packed = _scramble_padding(pack_2bit_rows(g), n)
        raw = g.copy()
        raw[(g == 3) & (np.random.default_rng(1).random(g.shape) < 0.5)] = 200
        dev = torch.from_numpy(packed).cuda()
        dev8 = torch.from_numpy(raw).cuda()
        shifted = torch.full((packed.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        shifted[5:5 + packed.size] = dev.reshape(-1)
        torch.cuda.synchronize()
        inputs = (("packed host", packed, _lib.GENO_PACKED2, None), ("u8 host", raw, _lib.GENO_U8, None),
                  ("packed device", int(dev.data_ptr()), _lib.GENO_PACKED2, m), ("u8 device", int(dev8.data_ptr()), _lib.GENO_U8, m),
                  ("packed device + 5 bytes", int(shifted.data_ptr()) + 5, _lib.GENO_PACKED2, m))
        for block in (None, "16", "48"):
            if block is None:
                monkeypatch.delenv("SNPGPU_QC_BLOCK_SNPS", raising=False)
            else:
                monkeypatch.setenv("SNPGPU_QC_BLOCK_SNPS", block)
            for name, src, fmt, n_snp in inputs:
                c, s = _lib.geno_counts(src, n, fmt=fmt, n_snp=n_snp)
                assert np.array_equal(c, wc) and np.array_equal(s, wm), (name, n, m, block)
            if block == "16" and m > 16:
                assert _lib.qc_stats()["count_launches"] == (m + 15) // 16
        c, s = _lib.geno_counts(packed, n, fmt=_lib.GENO_PACKED2, want_samp=False)
        assert s is None and np.array_equal(c, wc)
        c, s = _lib.geno_counts(packed, n, fmt=_lib.GENO_PACKED2, want_snp=False)
        assert c is None and np.array_equal(s, wm)


def _moment_input(n, m, seed):
    g = _geno(n, m, 0.08, seed)
    g[3] = 0                      # monomorphic, p = 0
    g[4] = 2                      # monomorphic, p = 1
    g[5] = 3                      # no call at all: frequency NaN
    g[11, ::2] = 3
    if n > 2:
        g[:, n - 1] = 3           # a sample without a call
    return g


@pytest.mark.parametrize("method", MOMENTS)
@pytest.mark.parametrize("n", [1, 7, 64, 257])
def test_moment_methods_bit_exact(method, n, monkeypatch):
    import torch
    m = 203
    g = _moment_input(n, m, seed=n + 17)
    packed = _scramble_padding(pack_2bit_rows(g), n)
    rng = np.random.default_rng(5)
    af = rng.uniform(0.01, 0.99, m)
    af[[0, 9]] = np.nan
    af[1], af[2] = 0.0, 1.0
    dev = torch.from_numpy(packed).cuda()
    torch.cuda.synchronize()
    for freq in (None, af):
        want, p_used = R.ind_inb_moment_ref(g, method, freq)
        results = []
        for block in (None, "16", "64"):
            if block is None:
                monkeypatch.delenv("SNPGPU_QC_BLOCK_SNPS", raising=False)
            else:
                monkeypatch.setenv("SNPGPU_QC_BLOCK_SNPS", block)
            for src, fmt, n_snp in ((packed, _lib.GENO_PACKED2, None), (g, _lib.GENO_U8, None),
                                    (int(dev.data_ptr()), _lib.GENO_PACKED2, m)):
                got, nit, p_got = _lib.ind_inb(src, n, method, allele_freq=freq, fmt=fmt, n_snp=n_snp)
                assert nit is None
                assert np.array_equal(p_got, p_used, equal_nan=True)
                results.append(got)
        for got in results:                                       # streamed and resident input: identical bits
            assert np.array_equal(got, want, equal_nan=True), (method, n, freq is None)
        if method == "mom.weir":
            # a NaN frequency poisons every sample called at that SNP
            bad = np.isnan(p_used)
            poisoned = ((g[bad] <= 2).any(0))
            assert np.isnan(want[poisoned]).all() and (freq is None or poisoned.any())
        if n > 2:
            assert np.isnan(want[n - 1])                          # 0 / 0


def test_samp_miss_rate_and_api(hapmap):
    g = unpack_2bit_rows(hapmap.packed, hapmap.n_samp)
    rv = api.snpgdsSampMissRate(hapmap)
    assert rv.dtype == np.float64 and np.array_equal(rv, (g > 2).sum(0) / float(g.shape[0]))
    sid, snp = hapmap.sample_id[5:90:3], hapmap.snp_id[100:3000:7]
    r = api.snpgdsSampMissRate(hapmap, sample_id=sid, snp_id=snp, with_id=True)
    sub = g[np.isin(hapmap.snp_id, snp)][:, np.isin(hapmap.sample_id, sid)]
    assert np.array_equal(r["MissingRate"], (sub > 2).sum(0) / float(sub.shape[0])) and list(r["sample_id"]) == list(sid)
    _, miss = _lib.geno_counts(pack_2bit_rows(sub), sub.shape[1], fmt=_lib.GENO_PACKED2)
    assert np.array_equal(r["MissingRate"], miss / float(sub.shape[0]))

    # snpgdsSelectSNP = the snp_id of _init_file2
    sel = api.snpgdsSelectSNP(hapmap, maf=0.05, missing_rate=0.05, verbose=False)
    ws = api._init_file2(None, hapmap, None, None, True, True, 0.05, 0.05, 1, False, 0)
    assert np.array_equal(sel, ws["snp_id"]) and 0 < len(sel) < len(hapmap.snp_id)


def _check_hwe(got, cnt, what):
    want, rare = H.hwe_ref(cnt)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = H.hwe_bound(want, rare)[ok]
    print("%s: %d SNPs, max |diff| %.3e, max diff / bound %.3f, bit-equal %d" %
          (what, ok.sum(), err.max() if err.size else 0, (err / np.maximum(bound, 1e-320)).max() if err.size else 0,
           int((got[ok] == want[ok]).sum())))
    assert (err <= bound).all(), what
    assert (got[ok] >= 0).all() and (got[ok] <= 1).all()


def test_hwe_hapmap_api(hapmap):
    g = unpack_2bit_rows(hapmap.packed, hapmap.n_samp)
    pv = api.snpgdsHWE(hapmap)
    _check_hwe(pv, _np_counts(g)[0], "HapMap")
    assert np.array_equal(pv, _lib.hwe(np.ascontiguousarray(hapmap.packed), hapmap.n_samp, fmt=_lib.GENO_PACKED2), equal_nan=True)
    sid, snp = hapmap.sample_id[::2], hapmap.snp_id[50:2500:5]
    r = api.snpgdsHWE(hapmap, sample_id=sid, snp_id=snp, with_id=True)
    sub = g[np.isin(hapmap.snp_id, snp)][:, np.isin(hapmap.sample_id, sid)]
    _check_hwe(r["pvalue"], _np_counts(sub)[0], "HapMap subset")
    assert list(r["sample_id"]) == list(sid) and list(r["snp_id"]) == list(snp)
    assert np.array_equal(r["pvalue"], _lib.hwe_counts(_np_counts(sub)[0]), equal_nan=True)


def test_hwe_extreme_tables_and_large_counts():
    grid = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 5, 0), (5, 0, 0), (0, 0, 7), (3, 0, 3), (4, 0, 3), (10, 1, 0), (0, 1, 10),
            (20, 20, 20), (0, 40, 0), (1, 40, 1), (50, 0, 50), (100, 3, 0), (100, 4, 0), (2, 2, 300), (300, 7, 2)]
    _check_hwe(_lib.hwe_counts(np.array(grid, np.int32)), np.array(grid), "extreme tables")
    rng = np.random.default_rng(8)
    rows = []
    for n in (1000, 10000, 40000, 100000):
        for q in (0.001, 0.05, 0.3, 0.5):
            for f in (0.0, 0.05):
                pr = np.array([(1 - q) ** 2 + f * q * (1 - q), 2 * q * (1 - q) * (1 - f), q * q + f * q * (1 - q)])
                rows.append(rng.multinomial(n - rng.integers(0, n // 50 + 1), pr))
    cnt = np.array(rows, np.int32)
    _check_hwe(_lib.hwe_counts(cnt), cnt, "synthetic counts up to N = 1e5")


# The comparison of niter is masked where the restatement's stopping margin is not firm.  Largest share of the compared samples that
# may be masked, per fixture, with the restatement's own figure beside it (computed on the CPU from tests/inb_ref.py alone):
MLE_NOT_FIRM = {                                          # cap       the restatement's figure
    "HapMap": 0.02,                                       #           2 of 279 = 0.0072
    "synthetic, given frequencies": 0.0,                  #           0 of 19
    "synthetic, estimated frequencies": 0.06,             #           1 of 19 = 0.0526
    "slow": 0.0,                                          #           0 of 1
    "never stopping": 0.0,                                #           0 of 6
}


def _check_mle(g, p_in, reltol, name):
    n = g.shape[1]
    F, nit, p_used = _lib.ind_inb(pack_2bit_rows(g), n, "mle", allele_freq=p_in, reltol=reltol, fmt=_lib.GENO_PACKED2)
    st = _lib.qc_stats()
    p_ref = R.snp_freq(g) if p_in is None else p_in
    assert np.array_equal(p_used, p_ref, equal_nan=True)
    worst, soft, compared = 0.0, 0, 0
    for j in range(n):
        ref = R.mle_ref(g[:, j], p_ref, reltol)
        if ref["niter"] < 0:
            assert nit[j] == -1 and np.array_equal(F[j], ref["F"], equal_nan=True), (name, j)
            continue
        compared += 1
        assert 1 <= nit[j] <= 10001, (name, j, nit[j])
        firm = ref["margin"] > Q.MLE_FIRM
        soft += 0 if firm else 1
        if firm:
            assert nit[j] == ref["niter"], (name, j, int(nit[j]), ref["niter"], ref["margin"])
        at = ref["F"] if nit[j] == ref["niter"] else R.mle_ref(g[:, j], p_ref, reltol, force_iter=min(int(nit[j]), 10000))["F_forced"]
        worst = max(worst, abs(F[j] - at))
        assert abs(F[j] - at) <= Q.MLE_F_TOL, (name, j, F[j], at, int(nit[j]), ref["niter"])
    print("%s: %d samples, max |F_gpu - F_ref| %.3e (allowed %.1e), margin not firm %d (%.1f %%), niter max %d, last-stride fill %.3f, "
          "kernel %.2f ms" % (name, compared, worst, Q.MLE_F_TOL, soft, 100.0 * soft / max(compared, 1), int(nit.max()),
                              st["mle_lane_steps_useful"] / max(st["mle_lane_steps_issued"], 1), st["mle_ms"]))
    assert soft <= 0.10 * compared, name
    assert soft <= MLE_NOT_FIRM[name] * compared, "%s: niter is compared at %d of %d samples only" % (name, compared - soft, compared)
    return F, nit


def test_mle_hapmap(hapmap):
    g = Q.hapmap_autosomal(hapmap)
    assert g.shape[1] == 279 and 7000 < g.shape[0] < 9500
    _check_mle(g, None, Q.RELTOL, "HapMap")


def test_mle_synthetic():
    g, p = Q.synthetic_mle()
    F, nit = _check_mle(g, p, Q.RELTOL, "synthetic, given frequencies")
    assert nit[19] == -1 and np.isnan(F[19])
    assert abs(F[:7].mean() - 0.25) < 0.05 and abs(F[7:14].mean() - 0.5) < 0.05
    _check_mle(g, None, Q.RELTOL, "synthetic, estimated frequencies")


def test_mle_slow_sample_at_the_lower_clamp():
    g, p = Q.slow_mle()
    ref = R.mle_ref(g[:, 0], p, Q.SLOW_RELTOL)
    assert ref["niter"] >= 1000 and ref["margin"] > Q.MLE_FIRM
    F, nit = _check_mle(g, p, Q.SLOW_RELTOL, "slow")
    assert nit[0] == ref["niter"] and nit[0] >= 1000 and F[0] < 0.001          # below the clamp it started from


def test_mle_never_stopping_reports_10001():
    g, p = Q.never_stopping_mle()
    F, nit = _check_mle(g, p, Q.NEVER_RELTOL, "never stopping")
    assert (nit == 10001).all()


@pytest.mark.parametrize("method", R.METHODS)
def test_ind_inb_api(hapmap, method):
    sid = hapmap.sample_id[3:120:2]
    r = api.snpgdsIndInb(hapmap, sample_id=sid, method=method, maf=0.05, missing_rate=0.05, reltol=Q.RELTOL, verbose=False)
    assert list(r["sample_id"]) == list(sid) and np.array_equal(r["snp_id"], api.snpgdsSelectSNP(
        hapmap, sample_id=sid, maf=0.05, missing_rate=0.05, verbose=False))
    rows = np.isin(hapmap.snp_id, r["snp_id"])
    g = unpack_2bit_rows(hapmap.packed[rows], hapmap.n_samp)[:, np.isin(hapmap.sample_id, sid)]
    coeff, nit, _ = _lib.ind_inb(pack_2bit_rows(g), g.shape[1], method, reltol=Q.RELTOL, fmt=_lib.GENO_PACKED2)
    assert np.array_equal(r["inbreeding"], coeff, equal_nan=True)
    if method == "mle":
        assert r["out_num_iter"].dtype == np.int32 and np.array_equal(r["out_num_iter"], nit)
        r2 = api.snpgdsIndInb(hapmap, sample_id=sid, method=method, maf=0.05, missing_rate=0.05, reltol=Q.RELTOL, out_num_iter=False,
                              verbose=False)
        assert "out_num_iter" not in r2 and np.array_equal(r2["inbreeding"], coeff, equal_nan=True)
    else:
        assert "out_num_iter" not in r
        assert np.array_equal(coeff, R.ind_inb_moment_ref(g, method)[0], equal_nan=True)
    # given frequencies, per entry of snp_id
    snp = r["snp_id"][::3]
    af = np.random.default_rng(2).uniform(0.05, 0.95, len(snp))
    r3 = api.snpgdsIndInb(hapmap, sample_id=sid, snp_id=snp, method=method, allele_freq=af, remove_monosnp=False, reltol=Q.RELTOL,
                          verbose=False)
    g3 = g[np.isin(r["snp_id"], r3["snp_id"])]
    af3 = af[np.isin(snp, r3["snp_id"])]
    c3, _, _ = _lib.ind_inb(pack_2bit_rows(g3), g3.shape[1], method, allele_freq=af3, reltol=Q.RELTOL, fmt=_lib.GENO_PACKED2)
    assert np.array_equal(r3["inbreeding"], c3, equal_nan=True)
