"""CPU-side tests of the LD scores (snpgdsLDScore): the restatement of the definition (tests/ld_score_ref.py) against a brute-force
evaluation, its windows against the pair test, the library's exports, and the argument errors of the C call and of the Python
function, all raised before anything reaches a device."""
import os
import re

import numpy as np
import pytest

import ld_score_ref as S
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_SYMBOLS = ["snpgpu_ld_score", "snpgpu_gnrLDScore"]
BIG = 10 ** 9

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnpgpu.so not built")


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _small_input():
    rng = np.random.default_rng(12)
    g = rng.integers(0, 3, (12, 9)).astype(np.uint8)
    g[rng.random(g.shape) < 0.15] = 3
    g[4] = 3                                        # never called: every pair with it is invalid
    g[7] = g[2]                                     # a duplicate: |LD| = 1 where both are called
    pos = np.array([0, 10, 10, 25, 40, 41, 41, 41, 90, 100, 140, 150], np.int32)
    return g, pos


@pytest.mark.parametrize("method", ["composite", "r", "dprime", "corr"])
@pytest.mark.parametrize("adjust, include_self", [(True, True), (True, False), (False, True), (False, False)])
def test_restatement_equals_brute_force(method, adjust, include_self):
    g, pos = _small_input()
    for bp, n in [(30, S.INT_MAX), (60, 3), (BIG, S.INT_MAX), (0, S.INT_MAX), (BIG, 0), (-1, 5)]:
        ref = S.ld_score(g, pos, bp, n, method, adjust, include_self)
        score, n_valid, n_window = S.ld_score_brute(g, pos, bp, n, method, adjust, include_self)
        assert np.array_equal(ref.score.view(np.uint64), score.view(np.uint64)), (bp, n)
        assert np.array_equal(ref.n_valid, n_valid) and np.array_equal(ref.n_window, n_window)
        assert ref.window_pairs * 2 == n_window.sum() and ref.valid_pairs * 2 == n_valid.sum()
        assert np.all(n_valid[4] == 0)
    full = S.ld_score(g, pos, BIG, S.INT_MAX, method, adjust, include_self)
    assert full.width == 11 and np.all(full.n_window == 11) and full.n_valid[4] == 0 < full.n_window[4]
    none = S.ld_score(g, pos, BIG, 0, method, adjust, include_self)
    assert none.width == 0 and np.all(none.score == (1.0 if include_self else 0.0)) and not none.n_window.any()


def test_adjustment_and_self_term():
    # two identical fully called SNPs: v = 1, t = 1, adjusted 1 - 0 / (n - 2) = 1; with the self term 2
    g = np.array([[0, 1, 2, 1, 0], [0, 1, 2, 1, 0]], np.uint8)
    for adjust in (False, True):
        r = S.ld_score(g, None, BIG, S.INT_MAX, "corr", adjust, True)
        assert r.score.tolist() == [2.0, 2.0] and r.n_valid.tolist() == [1, 1]
    # n = 2 called at both: valid without the adjustment, not valid with it
    g2 = np.array([[0, 2, 3, 3], [0, 2, 3, 3]], np.uint8)
    assert S.ld_score(g2, None, BIG, 5, "corr", False, False).n_valid.tolist() == [1, 1]
    r = S.ld_score(g2, None, BIG, 5, "corr", True, False)
    assert r.n_valid.tolist() == [0, 0] and r.score.tolist() == [0.0, 0.0] and r.n_window.tolist() == [1, 1]
    # the adjustment of an uncorrelated pair is negative: t = 0 -> -1 / (n - 2)
    g3 = np.array([[0, 0, 2, 2], [0, 2, 0, 2]], np.uint8)
    assert S.ld_score(g3, None, BIG, 5, "corr", True, False).score.tolist() == [-0.5, -0.5]


def test_windows_equal_brute_force():
    rng = np.random.default_rng(3)
    for trial in range(90):
        M = int(rng.integers(1, 40))
        kind = trial % 3
        if kind == 0:
            pos = np.sort(rng.integers(0, 300, M))
        elif kind == 1:
            pos = np.repeat(np.sort(rng.integers(0, 300, (M + 3) // 4)), 4)[:M]          # duplicated
        else:
            pos = np.full(M, 17)                                                          # constant
        bp = int(rng.integers(-1, 80)) if trial % 5 else BIG
        n = int(rng.integers(0, 12)) if trial % 7 else S.INT_MAX
        for p in (pos.astype(np.int32), None):
            lo, hi, W = S.windows(M, p, bp, n)
            blo, bhi, bW, contiguous = S.windows_brute(M, p, bp, n)
            assert contiguous
            assert np.array_equal(lo, blo) and np.array_equal(hi, bhi) and W == bW, (trial, bp, n)
            assert np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0)
    assert S.windows(30, np.full(30, 5, np.int32), 0, S.INT_MAX)[2] == 29          # equal positions: everything at 0 bp
    assert S.windows(30, np.arange(30, dtype=np.int32), 0, S.INT_MAX)[2] == 0
    # differences beyond int32: -2^31 ... 0 is 2^31 > max_bp (a 32-bit difference would wrap), 0 ... 2^31 - 1 is inside
    far = np.array([-2 ** 31, -5, 0, 7, 2 ** 31 - 1, 2 ** 31 - 1], np.int32)
    lo, hi, W = S.windows(6, far, 2 ** 31 - 1, S.INT_MAX)
    assert hi.tolist() == [1, 3, 5, 5, 5, 5] and lo.tolist() == [0, 0, 1, 1, 2, 2] and W == 3
    blo, bhi, bW, _ = S.windows_brute(6, far, 2 ** 31 - 1, S.INT_MAX)
    assert np.array_equal(lo, blo) and np.array_equal(hi, bhi) and bW == 3


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_header_and_exports():
    hdr = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    for s in SCORE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
    assert "snpgpu_ld_score_info" in hdr and "SNPGPU_LDSCORE_ADJUST = 1" in hdr and "SNPGPU_LDSCORE_SELF = 2" in hdr
    assert re.search(r"#define\s+SNPGPU_ABI_VERSION\s+2\b", hdr)
    assert [k for k, _ in _lib.LDScoreInfo._fields_] == ["width", "band_pairs", "window_pairs", "valid_pairs", "table_launches",
                                                         "table_tiles", "ms_stage", "ms_tables", "ms_values", "ms_fold", "ms_copy"]


@needs_lib
def test_library_has_the_symbols():
    L = _lib.lib()
    assert all(hasattr(L, s) for s in SCORE_SYMBOLS)


@needs_lib
@pytest.mark.parametrize("kw, msg", [
    (dict(method=0), "snpgpu_ld_score: invalid LD method"),
    (dict(method=5), "snpgpu_ld_score: invalid LD method"),                      # cov is refused, as in pruning
    (dict(flags=4), "snpgpu_ld_score: invalid flags"),
    (dict(flags=-1), "snpgpu_ld_score: invalid flags"),
    (dict(geno=None), "snpgpu_ld_score: NULL argument: geno"),
    (dict(score=None), "snpgpu_ld_score: NULL argument: score"),
    (dict(pos=np.array([0, 5, 4, 9], np.int32)), "snpgpu_ld_score: invalid positions"),
    (dict(n_samp=2 ** 24), "snpgpu_ld_score: invalid number of samples"),
    (dict(n_snp=0), "snpgpu_ld_score: invalid number of SNPs"),
    (dict(fmt=7), "snpgpu_ld_score: invalid genotype format"),
    (dict(mem=9), "snpgpu_ld_score: invalid memory kind"),
])
def test_c_argument_errors_before_the_device(kw, msg):
    a = dict(geno=np.zeros((4, 3), np.uint8), n_snp=4, n_samp=10, fmt=_lib.GENO_PACKED2, mem=_lib.HOST,
             pos=np.array([0, 5, 5, 9], np.int32), method=4, flags=3, score=np.zeros(4))
    a.update(kw)
    rc = _lib.lib().snpgpu_ld_score(_lib._ptr(a["geno"]), a["n_snp"], a["n_samp"], a["fmt"], a["mem"], _lib._ptr(a["pos"]), 1000, 100,
                                    a["method"], a["flags"], _lib._ptr(a["score"]), None, None, None, None)
    assert rc != 0
    assert msg in _lib.lib().snpgpu_last_error().decode()


@needs_lib
def test_working_space_entry_needs_a_score_vector():
    rc = _lib.lib().snpgpu_gnrLDScore(None, 1000, 100, 4, 3, 1, 0, None, None, None)
    assert rc != 0 and _lib.lib().snpgpu_last_error()


# ---- R-style argument errors of the Python function ----------------------------------------------------------------------------
def _tiny_file():
    g = np.zeros((4, 3), np.uint8)
    return GenoFile(genotype=g, snp_position=np.arange(4, dtype=np.int32) * 1000)


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(slide_max_bp="x"), TypeError, "is.na(slide.max.bp) | is.numeric(slide.max.bp) is not TRUE"),
    (dict(slide_max_n=True), TypeError, "is.na(slide.max.n) | is.numeric(slide.max.n) is not TRUE"),
    (dict(num_thread="2"), TypeError, "is.numeric(num.thread) is not TRUE"),
    (dict(num_thread=0), ValueError, "num.thread > 0L is not TRUE"),
    (dict(adjust=1), TypeError, "is.logical(adjust) is not TRUE"),
    (dict(include_self="yes"), TypeError, "is.logical(include.self) is not TRUE"),
    (dict(with_id=None), TypeError, "is.logical(with.id) is not TRUE"),
    (dict(verbose=1), TypeError, "is.logical(verbose) is not TRUE"),
    (dict(method="cov"), ValueError, 'method should be one of "composite", "r", "dprime" and "corr"'),
    (dict(method="pearson"), ValueError, 'method should be one of "composite", "r", "dprime" and "corr"'),
])
def test_argument_errors_before_the_device(kw, exc, msg):
    with pytest.raises(exc) as e:
        api.snpgdsLDScore(_tiny_file(), **kw)
    assert msg in str(e.value)


def test_not_a_gds_object():
    with pytest.raises(TypeError, match="SNP GDS object"):
        api.snpgdsLDScore("hapmap_geno.gds")


def test_file_without_positions_needs_an_infinite_bp_window():
    with pytest.raises(ValueError, match="snp.position"):
        api.snpgdsLDScore(GenoFile(genotype=np.zeros((2, 2), np.uint8)))
    with pytest.raises(ValueError, match="snp.position"):
        api.snpgdsLDScore(GenoFile(genotype=np.zeros((2, 2), np.uint8)), slide_max_bp=5e5, slide_max_n=10)
