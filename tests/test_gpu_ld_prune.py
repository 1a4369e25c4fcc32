"""GPU tests of LD pruning (snpgdsLDpruning -> snpgpu_ld_prune): the threshold bits against snpgdsLDMat's values bit for bit, kept
sets against the loop transcription of Perform_LD_Pruning (tests/ld_prune_ref.py) on HapMap and on synthetic data with planted LD,
odd sample counts, missing calls, unsorted / duplicated positions, several streamed blocks, host and device inputs in both row
formats, the working-space mirror, the Python API and one size test at N = 100 000."""
import itertools
import re
import warnings

import numpy as np
import pytest

import ld_prune_ref as R
import ld_ref
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import unpack_2bit_rows

pytestmark = pytest.mark.gpu

METHODS = ("composite", "r", "dprime", "corr")
CODES = {m: i + 1 for i, m in enumerate(METHODS)}
TOL = {"composite": 1e-12, "corr": 1e-12, "r": 1e-6, "dprime": 1e-6}   # the LD tests' value tolerances (test_gpu_ld.py)
BIG = 10 ** 9


def _positions(M, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "sorted":         # uneven spacing with dense stretches
        gaps = rng.exponential(3000, M).astype(np.int64)
        gaps[rng.random(M) < 0.3] //= 50
        return np.cumsum(gaps).astype(np.int32)
    if kind == "unsorted":
        return rng.integers(0, 60000, M).astype(np.int32)
    # duplicated: runs of equal positions
    return np.repeat(np.sort(rng.integers(0, 200000, (M + 3) // 4)), 4)[:M].astype(np.int32)


def _check_margin(ref, method):
    assert ref.tests == 0 or ref.margin > TOL[method], \
        "an |LD| lies within the value tolerance of the threshold (%g): kept sets cannot be compared" % ref.margin


# ---- 1. bits against snpgdsLDMat ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_bits_equal_thresholded_ldmat(method):
    N, M, W, start, thr = 279, 300, 70, 150, 0.2
    p = synth_hash_block_packed(N, 0, M, 21, 0.03, 4, True)
    with _lib.LDMatrix(N, M, CODES[method], W, False) as ld:
        ld.feed(p, _lib.GENO_PACKED2)
        band = ld.result()                                   # band[k - 1, x] = LD(x, x + k)
    with _lib.LDMatrix(N, M, CODES[method], -1, False) as ld:
        ld.feed(p, _lib.GENO_PACKED2)
        full = ld.result()                                   # full[y, x], y > x: the transposed table (first SNP y)
    bits, info = _lib.ld_prune_bits(p, N, start, W, thr, CODES[method], fmt=_lib.GENO_PACKED2, max_block_snps=100)
    assert info["width"] == W and info["table_launches"] >= 3
    with np.errstate(invalid="ignore"):
        want = np.zeros((M, W), bool)
        for x in range(M):
            k = np.arange(1, min(W, M - 1 - x) + 1)
            v = band[k - 1, x] if x >= start else full[x + k, x]
            want[x, k - 1] = np.abs(v) > thr
    assert np.array_equal(bits, want)
    assert bits.any() and not bits.all()


# ---- 2. kept sets on HapMap against the transcription ----------------------------------------------------------------------------
def _hapmap_grid(hapmap, ch, methods, bps):
    c = hapmap.snp_chromosome
    p = np.ascontiguousarray(hapmap.packed[c == ch])
    g = unpack_2bit_rows(p, hapmap.n_samp)
    pos = hapmap.snp_position[c == ch]
    M = p.shape[0]
    for method in methods:
        if max(bps) >= 10 ** 7:
            ld = R.ld_from_geno(g, method)
        else:
            ld = R.ld_from_geno(g, method, max(R.band_width(M, s, pos, max(bps), R.INT_MAX) for s in (0, M // 2, M - 1)))
        for start, thr, bp, n in itertools.product((0, M // 2, M - 1), (0.1, 0.2, 0.5), bps, (R.INT_MAX, 10, 100)):
            ref = R.prune(M, start, pos, bp, n, thr, ld)
            _check_margin(ref, method)
            got, info = _lib.ld_prune(p, hapmap.n_samp, pos, start, bp, n, thr, CODES[method], fmt=_lib.GENO_PACKED2)
            assert np.array_equal(got, ref.keep), (ch, method, start, thr, bp, n)
            assert info["width"] == R.band_width(M, start, pos, bp, n) and info["n_kept"] == ref.keep.sum()


@pytest.mark.parametrize("ch", [21, 22])
def test_hapmap_kept_sets_full_grid(hapmap, ch):
    _hapmap_grid(hapmap, ch, METHODS, (500000, 10 ** 7, 3 * 10 ** 8))


def test_hapmap_kept_sets_largest_chromosome(hapmap):
    _hapmap_grid(hapmap, 1, ("composite", "corr"), (500000, 10 ** 7, 3 * 10 ** 8))
    _hapmap_grid(hapmap, 1, ("r", "dprime"), (500000,))


# ---- 3. synthetic data --------------------------------------------------------------------------------------------------------
SYN = [(n, miss) for n in (1, 3, 65, 1000, 70001) for miss in (0.0, 0.03, 0.3)]


@pytest.mark.parametrize("n_samp, missing", SYN)
def test_synthetic_equals_transcription(n_samp, missing):
    import torch
    idx = SYN.index((n_samp, missing))
    M = 240
    method = METHODS[idx % 4]
    kind = ("sorted", "unsorted", "duplicated")[idx % 3]
    p = synth_hash_block_packed(n_samp, 0, M, 31 + idx, missing, 4, False)
    g = unpack_2bit_rows(p, n_samp)
    pos = _positions(M, kind, idx)
    tab = _lib.ld_pair_tables(p, p, n_samp, fmt=_lib.GENO_PACKED2)      # bit-exact (test_gpu_ld.py)
    V = ld_ref.ld_values(tab, method)                                    # V[j, i]: j first
    dp = torch.from_numpy(p).cuda()
    dg = torch.from_numpy(np.ascontiguousarray(g)).cuda()
    torch.cuda.synchronize()
    combos = [(0, 20000, R.INT_MAX, 0.21, 64), (M // 3, 8000, 30, 0.37, 50), (M - 1, 40000, 100, 0.21, 1),
              (M // 2, BIG, R.INT_MAX, 0.37, 64)]                        # the last: W = M - 1
    for start, bp, n, thr, blk in combos:
        ref = R.prune(M, start, pos, bp, n, thr, lambda j, i: V[j, i])
        _check_margin(ref, method)
        W = R.band_width(M, start, pos, bp, n)
        runs = [
            _lib.ld_prune(p, n_samp, pos, start, bp, n, thr, CODES[method], fmt=_lib.GENO_PACKED2, max_block_snps=blk),
            _lib.ld_prune(g, n_samp, pos, start, bp, n, thr, CODES[method], fmt=_lib.GENO_U8, max_block_snps=blk),
            _lib.ld_prune(dp.data_ptr(), n_samp, pos, start, bp, n, thr, CODES[method], fmt=_lib.GENO_PACKED2, n_snp=M,
                          max_block_snps=blk),
            _lib.ld_prune(dg.data_ptr(), n_samp, pos, start, bp, n, thr, CODES[method], fmt=_lib.GENO_U8, n_snp=M),
        ]
        for got, info in runs:
            assert np.array_equal(got, ref.keep), (n_samp, missing, method, kind, start, bp, n)
            assert info["width"] == W
        if W > 0 and blk < M - W:
            assert runs[0][1]["table_launches"] > 1          # several streamed blocks and their halos
        # the working-space mirror on the same rows
        _lib.check(_lib.lib().snpgpu_ws_set_geno(_lib._ptr(p), M, n_samp, _lib.GENO_PACKED2, 0))
        keep = np.zeros(M, np.uint8)
        _lib.check(_lib.lib().snpgpu_gnrLDpruning(start, _lib._ptr(pos), bp, n, thr, CODES[method], 1, 0, _lib._ptr(keep)))
        assert np.array_equal(keep.astype(bool), ref.keep)
    assert any(R.band_width(M, s, pos, bp, n) == M - 1 for s, bp, n, _, _ in combos)


def test_errors():
    p = synth_hash_block_packed(10, 0, 5, 1)
    pos = np.arange(5, dtype=np.int32)
    for kw, msg in [(dict(method=5), "invalid LD method"), (dict(method=0), "invalid LD method"),
                    (dict(start_idx=5), "invalid start index"), (dict(start_idx=-1), "invalid start index")]:
        a = dict(start_idx=0, method=1)
        a.update(kw)
        with pytest.raises(_lib.SnpGpuError, match=msg):
            _lib.ld_prune(p, 10, pos, a["start_idx"], BIG, BIG, 0.2, a["method"], fmt=_lib.GENO_PACKED2)


# ---- 4. the Python API ------------------------------------------------------------------------------------------------------
def _ws_rows(hapmap, **kw):
    ws = api._init_file2(None, hapmap, kw.get("sample_id"), kw.get("snp_id"), kw.get("autosome_only", True), True, 0.005, 0.01,
                         1, False)
    flag = np.isin(hapmap.snp_id, ws["snp_id"])
    return ws, hapmap.snp_chromosome[flag], hapmap.snp_position[flag]


def test_api_keys_selection_and_level1(hapmap):
    samp = hapmap.sample_id[::2]
    snps = hapmap.snp_id[hapmap.snp_id % 5 != 0]
    for kw in (dict(), dict(sample_id=samp, snp_id=snps, autosome_only=False)):
        res = api.snpgdsLDpruning(hapmap, verbose=False, seed=7, **kw)
        ws, chrom, pos = _ws_rows(hapmap, **kw)
        want_keys = ["chr%d" % c for c in range(1, 24 if kw else 23)]
        assert list(res) == want_keys
        rng = np.random.default_rng(7)
        for key, ch in zip(want_keys, range(1, 24)):
            sel = chrom == ch
            n = int(sel.sum())
            start = int(rng.integers(1, min(n, 500) + 1)) - 1
            keep, _ = _lib.ld_prune(ws["packed"][sel], ws["n_samp"], pos[sel], start, 500000, R.INT_MAX, 0.2, 1,
                                    fmt=_lib.GENO_PACKED2)
            assert np.array_equal(res[key], ws["snp_id"][sel][keep]), key


def test_api_seed_start_pos_and_methods(hapmap):
    a = api.snpgdsLDpruning(hapmap, verbose=False, seed=3, start_pos="random")
    b = api.snpgdsLDpruning(hapmap, verbose=False, seed=3, start_pos="random")
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    f = api.snpgdsLDpruning(hapmap, verbose=False, start_pos="first", method="r", ld_threshold=0.3, slide_max_n=50)
    ws, chrom, pos = _ws_rows(hapmap)
    sel = chrom == 4
    keep, _ = _lib.ld_prune(ws["packed"][sel], ws["n_samp"], pos[sel], 0, 500000, 50, 0.3, 2, fmt=_lib.GENO_PACKED2)
    assert np.array_equal(f["chr4"], ws["snp_id"][sel][keep])
    last = api.snpgdsLDpruning(hapmap, verbose=False, start_pos="last", method="dprime", slide_max_bp=2e6)
    assert all(len(v) > 0 for v in last.values())


def test_api_infinite_window_keeps_everything(hapmap):
    with pytest.warns(RuntimeWarning, match="coercion to integer range"):
        res = api.snpgdsLDpruning(hapmap, verbose=False, slide_max_bp=float("inf"), seed=1)
    ws, chrom, _ = _ws_rows(hapmap)
    assert np.array_equal(np.concatenate(list(res.values())), ws["snp_id"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        api.snpgdsLDpruning(hapmap, verbose=False, seed=1)
    assert not [x for x in w if "coercion" in str(x.message)]      # the default window coerces without a warning


def test_api_verbose_lines(hapmap, capsys):
    res = api.snpgdsLDpruning(hapmap, seed=2)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "SNP pruning based on LD:"
    assert "    sliding window: 500,000 basepairs, Inf SNPs" in out
    assert "    |LD| threshold: 0.2" in out and "    method: composite" in out
    chrom_lines = [x for x in out if x.startswith("Chrom ")]
    assert len(chrom_lines) == 22 and re.match(r"Chrom 1: \|=*\|=*\|$", chrom_lines[0])
    pct = [x for x in out if re.match(r"    \d+\.\d\d%, [\d,]+ / [\d,]+ \(", x)]
    assert len(pct) == 22
    total = sum(len(v) for v in res.values())
    assert out[-1] == "{:,} markers are selected in total.".format(total)


def test_api_result_feeds_pca(hapmap):
    res = api.snpgdsLDpruning(hapmap, verbose=False, seed=11)
    ids = np.concatenate(list(res.values()))
    assert 0 < len(ids) < hapmap.n_snp
    pca = api.snpgdsPCA(hapmap, snp_id=ids, verbose=False)
    assert np.all(np.isfinite(pca["eigenval"][:8])) and pca["eigenval"][0] > 0
    assert len(pca["snp_id"]) <= len(ids)


# ---- 5. one size test -----------------------------------------------------------------------------------------------------------
def test_size_n100000():
    import torch
    N, M, W_blk = 100000, 20480, 1024
    rb = (N + 3) // 4
    geno = torch.empty(M * rb, dtype=torch.uint8, device="cuda")
    for i0 in range(0, M, 8192):
        n = min(8192, M - i0)
        _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, n, seed=77, missing=0.02, spectrum=4)
    torch.cuda.synchronize()
    pos = _positions(M, "sorted", 77)
    start = 123
    got, info = _lib.ld_prune(geno.data_ptr(), N, pos, start, 500000, R.INT_MAX, 0.2, 1, fmt=_lib.GENO_PACKED2, n_snp=M)
    W = info["width"]
    assert W == R.band_width(M, start, pos, 500000, R.INT_MAX) and 50 < W < 1000
    host = geno.cpu().numpy().reshape(M, rb)
    # band tables of the transcription from snpgpu_ld_pair_tables (bit-exact), in row blocks
    band = np.zeros((M, W, 3, 3), np.int64)
    for x0 in range(0, M, W_blk):
        x1 = min(M, x0 + W_blk)
        y1 = min(M, x1 + W)
        t = _lib.ld_pair_tables(host[x0:x1], host[x0:y1], N, fmt=_lib.GENO_PACKED2)
        for x in range(x0, x1):
            k = np.arange(1, min(W, M - 1 - x) + 1)
            band[x, k - 1] = t[x - x0, x - x0 + k]
    ref = R.prune(M, start, pos, 500000, R.INT_MAX, 0.2, R.ld_from_band(band, "composite"))
    _check_margin(ref, "composite")
    assert ref.max_dist <= W
    assert np.array_equal(got, ref.keep)
    assert 0.05 < got.mean() < 0.95
