"""GPU tests of the LD scores (snpgdsLDScore -> snpgpu_ld_score): the scores against a float64 fold of snpgdsLDMat's own band
values bit for bit, independence of the block partition, the row format, the memory kind and the entry point, the numpy
restatement (tests/ld_score_ref.py) within a bound computed from its own values, the pair counts, and the Python function on HapMap.
Synthetic data as in test_gpu_ld_prune.py: M = 240 SNPs, odd sample counts, missing calls, sorted and duplicated positions."""
import functools
import types

import numpy as np
import pytest

import ld_score_ref as S
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoFile, pack_2bit_rows, unpack_2bit_rows
from test_gpu_ld_prune import _positions

pytestmark = pytest.mark.gpu

METHODS = ("composite", "r", "dprime", "corr")
CODES = {m: i + 1 for i, m in enumerate(METHODS)}
TOL = {"composite": 1e-12, "corr": 1e-12, "r": 1e-6, "dprime": 1e-6}   # the LD tests' value tolerances (test_gpu_ld.py)
BIG = 10 ** 9
M = 240
SYN = [(n, miss) for n in (1, 3, 65, 1000) for miss in (0.0, 0.03, 0.3)] + [(70001, 0.03)]
# (positions, slide_max_bp, slide_max_n); None: the case's own kind
WINDOWS = [(None, 20000, S.INT_MAX), (None, 8000, 30), (None, BIG, S.INT_MAX), ("duplicated", 0, S.INT_MAX), (None, 20000, 0)]
FLAGS = [(True, True), (False, True), (True, False), (False, False)]                 # (adjust, include_self)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _case(idx):
    """one synthetic data set and its reference pair values (computed once, shared by the tests, never modified)"""
    n_samp, missing = SYN[idx]
    method = METHODS[idx % 4]
    p = synth_hash_block_packed(n_samp, 0, M, 31 + idx, missing, 4, False)
    g = unpack_2bit_rows(p, n_samp)
    V, n = S.pair_values(S.tables(g), method)
    kind = ("sorted", "duplicated")[idx % 2]
    return types.SimpleNamespace(n_samp=n_samp, method=method, p=p, g=g, V=V, n=n,
                                 pos={kind: _positions(M, kind, idx), "duplicated": _positions(M, "duplicated", idx)}, kind=kind)


def _window(c, widx):
    kind, bp, n = WINDOWS[widx]
    return c.pos[kind or c.kind], bp, n


@functools.lru_cache(maxsize=None)
def _ref(idx, widx, adjust, include_self):
    c = _case(idx)
    pos, bp, n = _window(c, widx)
    return S.score_from_values(c.V, c.n, pos, bp, n, adjust, include_self)


# ---- 1. bits against the project's own LD values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_bits_equal_fold_of_ldmat_band(method):
    for idx in (5, 7, 11):                                         # N = 3 / 65 / 1000, missing 0.3 / 0.03 / 0.3
        c = _case(idx)
        N = c.n_samp
        tot = _lib.ld_pair_tables(c.p, c.p, N, fmt=_lib.GENO_PACKED2).astype(np.int64).sum((-1, -2))
        for widx in range(len(WINDOWS)):
            pos, bp, n = _window(c, widx)
            W = S.windows(M, pos, bp, n)[2]
            V = np.full((M, M), np.nan)
            if W > 0:
                with _lib.LDMatrix(N, M, CODES[method], W, False) as ld:
                    ld.feed(c.p, _lib.GENO_PACKED2)
                    band = ld.result()                             # band[k - 1, x] = LD(x, x + k)
                for k in range(1, W + 1):
                    x = np.arange(M - k)
                    V[x, x + k] = band[k - 1, x]
                    V[x + k, x] = band[k - 1, x]
            for adjust, include_self in FLAGS:
                want = S.score_from_values(V, tot, pos, bp, n, adjust, include_self)       # the fold in Python float64
                score, n_valid, n_window, info = _lib.ld_score(c.p, N, pos, bp, n, CODES[method], adjust, include_self,
                                                               fmt=_lib.GENO_PACKED2)
                key = (idx, widx, method, adjust, include_self)
                assert np.array_equal(_bits(score), _bits(want.score)), key
                assert np.array_equal(n_valid, want.n_valid) and np.array_equal(n_window, want.n_window), key
                assert info["width"] == W
                if W == 0:
                    assert np.all(score == (1.0 if include_self else 0.0)) and not n_window.any() and not n_valid.any()


# ---- 2 - 4. independence, the numpy restatement, conservation ------------------------------------------------------------------
@pytest.mark.parametrize("n_samp, missing", SYN)
def test_synthetic(n_samp, missing):
    import torch
    idx = SYN.index((n_samp, missing))
    c = _case(idx)
    code = CODES[c.method]
    dp = torch.from_numpy(c.p).cuda()
    dg = torch.from_numpy(np.ascontiguousarray(c.g)).cuda()
    torch.cuda.synchronize()
    for widx in range(len(WINDOWS)):
        pos, bp, n = _window(c, widx)
        adjust, include_self = FLAGS[(idx + widx) % 4]
        ref = _ref(idx, widx, adjust, include_self)
        key = (n_samp, missing, c.method, widx, adjust, include_self)

        def run(geno, fmt, **kw):
            return _lib.ld_score(geno, n_samp, pos, bp, n, code, adjust, include_self, fmt=fmt, **kw)
        score, n_valid, n_window, info = run(c.p, _lib.GENO_PACKED2)
        # 3. the restatement: counts exactly, scores within the bound its own values give
        assert np.array_equal(n_valid, ref.n_valid) and np.array_equal(n_window, ref.n_window), key
        bound = S.error_bound(ref, TOL[c.method])
        err = np.abs(score - ref.score)
        print("ld_score", key, "W", ref.width, "max err %.3g" % np.max(err[np.isfinite(err)], initial=0.0), "max bound %.3g" % bound.max())
        assert np.all((err <= bound) | (_bits(score) == _bits(ref.score))), key
        # 4. conservation
        assert n_valid.sum() == 2 * info["valid_pairs"] and n_window.sum() == 2 * info["window_pairs"], key
        assert info["width"] == ref.width and info["window_pairs"] == ref.window_pairs
        assert info["band_pairs"] == sum(min(ref.width, M - 1 - x) for x in range(M))
        # 2. independence: block partition, row format, memory kind, entry point, repetition
        runs = [run(c.p, _lib.GENO_PACKED2, max_block_snps=blk) for blk in (50, 64, 100)]
        if ref.width > 0:
            assert all(r[3]["table_launches"] > 1 for r in runs), key
        runs += [
            run(c.g, _lib.GENO_U8, max_block_snps=64),
            run(dp.data_ptr(), _lib.GENO_PACKED2, n_snp=M, max_block_snps=50),
            run(dg.data_ptr(), _lib.GENO_U8, n_snp=M),
            run(c.p, _lib.GENO_PACKED2),
        ]
        _lib.check(_lib.lib().snpgpu_ws_set_geno(_lib._ptr(c.p), M, n_samp, _lib.GENO_PACKED2, 0))
        ws = (np.empty(M), np.empty(M, np.int32), np.empty(M, np.int32))
        flags = (_lib.LDSCORE_ADJUST if adjust else 0) | (_lib.LDSCORE_SELF if include_self else 0)
        _lib.check(_lib.lib().snpgpu_gnrLDScore(_lib._ptr(pos), bp, n, code, flags, 1, 0, *[_lib._ptr(a) for a in ws]))
        runs.append(ws)
        for r in runs:
            assert np.array_equal(_bits(r[0]), _bits(score)), key
            assert np.array_equal(r[1], n_valid) and np.array_equal(r[2], n_window), key


def test_counts_may_be_null_and_positions_too():
    c = _case(7)
    score = np.empty(M)
    o = _lib.Opts(device=0)
    _lib.check(_lib.lib().snpgpu_ld_score(_lib._ptr(c.p), M, c.n_samp, _lib.GENO_PACKED2, _lib.HOST, None, 5, 25, CODES[c.method], 3,
                                          _lib._ptr(score), None, None, _lib.ctypes.byref(o), None))
    want = S.score_from_values(c.V, c.n, None, 5, 25, True, True)                    # no positions: the count alone
    assert want.width == 25 and np.all(np.abs(score - want.score) <= S.error_bound(want, TOL[c.method]))
    got = _lib.ld_score(c.p, c.n_samp, None, -1, 25, CODES[c.method], fmt=_lib.GENO_PACKED2)
    assert got[3]["width"] == 0 and np.all(got[0] == 1.0)                               # slide_max_bp < 0: no pair


# ---- 5. the cases bite -----------------------------------------------------------------------------------------------------------
def test_the_cases_bite():
    refs = [(idx, widx, _ref(idx, widx, *FLAGS[(idx + widx) % 4])) for idx in range(len(SYN)) for widx in range(len(WINDOWS))]
    assert any(r.valid_pairs < r.window_pairs for _, _, r in refs)                      # an invalid pair inside a window
    assert any(np.any((r.n_valid == 0) & (r.n_window > 0)) for _, _, r in refs)
    assert any(np.any((r.n_valid > 0) & (r.n_valid < r.n_window)) for _, _, r in refs)
    assert any(r.width == M - 1 for _, _, r in refs) and any(r.width == 0 for _, _, r in refs)
    assert any(0 < r.width < 16 for _, _, r in refs) and any(16 < r.width < 64 for _, _, r in refs)      # below / above one tile
    by_bp = by_count = False
    for idx, widx, r in refs:
        pos, bp, n = _window(_case(idx), widx)
        if n == S.INT_MAX or n <= 0:
            continue
        for i in np.nonzero(r.hi < M - 1)[0]:
            nxt = r.hi[i] + 1                                      # the first SNP above i's window
            bp_ok, count_ok = int(pos[nxt]) - int(pos[i]) <= bp, nxt - i <= n
            by_bp |= count_ok and not bp_ok
            by_count |= bp_ok and not count_ok
    assert by_bp and by_count
    dup = [r for _, widx, r in refs if WINDOWS[widx][1] == 0]
    assert all(3 <= r.width <= 7 for r in dup)                     # 0 bp: only the runs of four (or, by chance, eight) equal positions


# ---- 6. the Python function on HapMap ----------------------------------------------------------------------------------------------
def _chrom_rows(hapmap, ch):
    sel = hapmap.snp_chromosome == ch
    return np.ascontiguousarray(hapmap.packed[sel]), hapmap.snp_position[sel], hapmap.snp_id[sel]


def test_api_two_chromosomes(hapmap, capsys):
    parts = {ch: _chrom_rows(hapmap, ch) for ch in (21, 22)}
    ids = np.concatenate([parts[21][2], parts[22][2]])
    assert len(parts[21][2]) == 126 and len(parts[22][2]) == 116
    res = api.snpgdsLDScore(hapmap, snp_id=ids, remove_monosnp=False, verbose=False)
    assert list(res) == ["sample_id", "snp_id", "chromosome", "position", "score", "n_valid", "n_window"]
    assert np.array_equal(res["snp_id"], ids) and np.array_equal(res["sample_id"], hapmap.sample_id)
    assert np.array_equal(res["chromosome"], np.repeat([21, 22], [126, 116]))
    assert np.array_equal(res["position"], np.concatenate([parts[21][1], parts[22][1]]))
    off = 0
    for ch in (21, 22):
        p, pos, snp = parts[ch]
        score, n_valid, n_window, info = _lib.ld_score(p, hapmap.n_samp, pos, 1000000, S.INT_MAX, _lib.LD_CORR, True, True,
                                                       fmt=_lib.GENO_PACKED2)
        sl = slice(off, off + len(snp))
        off += len(snp)
        assert np.array_equal(_bits(res["score"][sl]), _bits(score)), ch
        assert np.array_equal(res["n_valid"][sl], n_valid) and np.array_equal(res["n_window"][sl], n_window)
        assert 0 < info["width"] < len(snp) - 1 and n_valid.sum() > 0
        alone = api.snpgdsLDScore(hapmap, snp_id=snp, remove_monosnp=False, verbose=False)      # no window crosses the boundary
        assert np.array_equal(_bits(alone["score"]), _bits(score)) and np.array_equal(alone["n_window"], n_window)
    bare = api.snpgdsLDScore(hapmap, snp_id=ids, remove_monosnp=False, verbose=False, with_id=False)
    assert isinstance(bare, np.ndarray) and np.array_equal(_bits(bare), _bits(res["score"]))
    capsys.readouterr()
    # other arguments reach the library: method, flags, the count limit
    r = api.snpgdsLDScore(hapmap, snp_id=parts[22][2], remove_monosnp=False, method="r", slide_max_bp=float("nan"), slide_max_n=20,
                          adjust=False, include_self=False)
    want = _lib.ld_score(parts[22][0], hapmap.n_samp, None, S.INT_MAX, 20, _lib.LD_R, False, False, fmt=_lib.GENO_PACKED2)
    assert np.array_equal(_bits(r["score"]), _bits(want[0])) and np.array_equal(r["n_window"], want[2])
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "LD scores:"
    assert "    sliding window: Inf basepairs, 20 SNPs" in out and "    method: R" in out
    assert "    adjusted: FALSE, self term: FALSE" in out
    assert len([x for x in out if x.startswith("Chrom 22: 116 SNPs, ")]) == 1


def test_api_sample_subset_and_default_lines(hapmap, capsys):
    p, pos, snp = _chrom_rows(hapmap, 21)
    samp = hapmap.sample_id[::2]
    res = api.snpgdsLDScore(hapmap, sample_id=samp, snp_id=snp, remove_monosnp=False)
    out = capsys.readouterr().out.splitlines()
    assert "    sliding window: 1,000,000 basepairs, Inf SNPs" in out and "    method: correlation" in out
    assert "    adjusted: TRUE, self term: TRUE" in out
    sub = pack_2bit_rows(unpack_2bit_rows(p, hapmap.n_samp)[:, ::2])
    want = _lib.ld_score(sub, len(samp), pos, 1000000, S.INT_MAX, _lib.LD_CORR, fmt=_lib.GENO_PACKED2)
    assert np.array_equal(res["sample_id"], samp)
    assert np.array_equal(_bits(res["score"]), _bits(want[0])) and np.array_equal(res["n_valid"], want[1])


def test_api_errors(hapmap):
    p, pos, snp = _chrom_rows(hapmap, 22)
    shuffled = np.random.default_rng(1).permutation(pos)
    assert np.any(np.diff(shuffled) < 0)
    f = GenoFile(packed=p, n_samp=hapmap.n_samp, snp_position=shuffled, snp_chromosome=np.full(len(pos), 22))
    with pytest.raises(ValueError, match="snp.position decreases on chromosome 22"):
        api.snpgdsLDScore(f, remove_monosnp=False, verbose=False)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ld_score: invalid positions"):
        _lib.ld_score(p, hapmap.n_samp, shuffled, 1000000, S.INT_MAX, fmt=_lib.GENO_PACKED2)
    with pytest.raises(ValueError, match='method should be one of "composite", "r", "dprime" and "corr"'):
        api.snpgdsLDScore(hapmap, method="cov", verbose=False)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ld_score: invalid LD method"):
        _lib.ld_score(p, hapmap.n_samp, pos, 1000000, S.INT_MAX, _lib.LD_COV, fmt=_lib.GENO_PACKED2)
    # without positions only a window in SNPs is possible
    g = GenoFile(packed=p, n_samp=hapmap.n_samp)
    with pytest.raises(ValueError, match="snp.position"):
        api.snpgdsLDScore(g, remove_monosnp=False, verbose=False)
    res = api.snpgdsLDScore(g, autosome_only=False, remove_monosnp=False, slide_max_bp=float("inf"), slide_max_n=15, verbose=False)
    want = _lib.ld_score(p, hapmap.n_samp, None, S.INT_MAX, 15, _lib.LD_CORR, fmt=_lib.GENO_PACKED2)
    assert res["position"] is None and np.array_equal(_bits(res["score"]), _bits(want[0]))
