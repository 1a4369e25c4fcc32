"""CPU-side tests of LD pruning (snpgdsLDpruning): the loop transcription of Perform_LD_Pruning (tests/ld_prune_ref.py) on hand-made
cases, the band width it implies, the snp.position node of the HapMap file, the library's exports and the R-level argument
errors of the Python mirror (raised before anything reaches the device)."""
import math
import os
import re

import numpy as np
import pytest

import ld_prune_ref as R
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRUNE_SYMBOLS = ["snpgpu_ld_prune", "snpgpu_ld_prune_bits", "snpgpu_gnrLDpruning"]
BIG = 10 ** 9


def _table_ld(vals):
    """ld(j, i) from a dict {(j, i): value}; a pair not in it is an error (the scan must not test it)"""
    def ld(j, i):
        return vals[(j, i)]
    return ld


# ---- the transcription ---------------------------------------------------------------------------------------------------------
def test_duplicated_snps_are_pruned():
    # SNPs 1 and 3 duplicate SNP 0 (|LD| = 1), SNP 2 is unlinked
    lv = {0: 0, 1: 0, 2: 1, 3: 0}
    r = R.prune(4, 0, [10, 20, 30, 40], BIG, BIG, 0.2, lambda j, i: 1.0 if lv[j] == lv[i] else 0.05)
    assert r.keep.tolist() == [True, False, True, False]
    assert r.margin == pytest.approx(0.15)


def test_nan_never_prunes():
    r = R.prune(3, 0, [1, 2, 3], BIG, BIG, 0.2, lambda j, i: float("nan"))
    assert r.keep.all()
    assert r.margin == math.inf and r.tests == 3


def test_negative_ld_prunes_by_absolute_value():
    r = R.prune(2, 0, [1, 2], BIG, BIG, 0.2, lambda j, i: -0.9)
    assert r.keep.tolist() == [True, False]


def test_unsorted_position_erases_a_kept_snp_for_good():
    # SNP 1 lies far away: at candidate 1, kept SNP 0 is erased; at candidate 2 (back near SNP 0) it is not tested any more,
    # so SNP 2 survives although LD(0, 2) is above the threshold
    pos = [100, 10 ** 7, 150]
    vals = {(1, 2): 0.0}

    def ld(j, i):
        if (j, i) == (0, 2):
            raise AssertionError("erased SNP tested")
        return vals[(j, i)]
    r = R.prune(3, 0, pos, 1000, BIG, 0.2, ld)
    assert r.keep.tolist() == [True, True, True]
    # with a window wide enough nothing is erased and SNP 2 goes
    r = R.prune(3, 0, pos, BIG, BIG, 0.2, _table_ld({(0, 1): 0.0, (0, 2): 0.9, (1, 2): 0.0}))
    assert r.keep.tolist() == [True, True, False]


def test_backward_initial_list_stops_at_the_first_kept_snp_outside_the_window():
    # start = 1; kept after the forward pass: 1, 2, 4 (3 pruned by 1).  Window of 2 SNPs: the backward list takes 1 and 2, then
    # stops at 4 (outside) -- and would stop there even if a later kept SNP were inside again.  Candidate 0 is tested against 1
    # and 2 only.
    pos = [0, 1, 2, 3, 4]
    vals = {(1, 2): 0.0, (1, 3): 0.5, (2, 4): 0.0, (1, 0): 0.0, (2, 0): 0.0}
    tested = []

    def ld(j, i):
        tested.append((j, i))
        return vals[(j, i)]
    r = R.prune(5, 1, pos, BIG, 2, 0.2, ld)
    assert r.keep.tolist() == [True, True, True, False, True]
    assert [t for t in tested if t[1] == 0] == [(1, 0), (2, 0)]
    # the scan's `break`: with positions that bring SNP 4 back inside the window of the start after SNP 3 left it, only the
    # SNPs before the first kept one outside are listed
    pos2 = [0, 1, 2, 10 ** 6, 3]
    vals2 = {(1, 2): 0.0, (1, 0): 0.0, (2, 0): 0.0}
    r2 = R.prune(5, 1, pos2, 100, BIG, 0.2, _table_ld(vals2))
    assert r2.keep.all()
    # SNP 4 would prune SNP 0 if it were listed; it is not: the initial list stopped at SNP 3
    vals2[(4, 0)] = 0.9
    r3 = R.prune(5, 1, pos2, 100, BIG, 0.2, _table_ld(vals2))
    assert r3.keep.all()


@pytest.mark.parametrize("max_n", [0, -5])
def test_slide_max_n_not_positive_keeps_everything(max_n):
    r = R.prune(6, 2, list(range(6)), BIG, max_n, 0.0, lambda j, i: 1.0)
    assert r.keep.all() and r.tests == 0
    assert R.band_width(6, 2, list(range(6)), BIG, max_n) == 0


def test_infinite_bp_window_keeps_everything():
    # slide.max.bp = Inf -> .Machine$double.xmax -> Rf_asInteger -> NA_integer_ (INT_MIN): no distance is <= INT_MIN
    bp = R.as_integer(np.finfo(np.float64).max)
    assert bp == R.NA_INTEGER
    r = R.prune(5, 0, [0] * 5, bp, R.INT_MAX, 0.0, lambda j, i: 1.0)
    assert r.keep.all() and r.tests == 0
    with pytest.warns(RuntimeWarning):
        assert api._as_integer(np.finfo(np.float64).max) == R.NA_INTEGER


def test_as_integer_truncates():
    for v, want in [(5e5, 500000), (2.9, 2), (-2.9, -2), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert R.as_integer(v) == want
        assert api._as_integer(v) == want
    with pytest.warns(RuntimeWarning):
        assert api._as_integer(2.0 ** 31) == R.NA_INTEGER


def test_band_width_bounds_every_tested_pair():
    """The reach rule: on random unsorted / duplicated positions the transcription never tests a pair further apart than the band
    width (what the GPU path sizes its tables by), and a window spanning everything gives W = M - 1."""
    rng = np.random.default_rng(5)
    for trial in range(60):
        M = int(rng.integers(1, 40))
        pos = rng.integers(0, 50, M) if trial % 2 else np.sort(rng.integers(0, 200, M))
        start = int(rng.integers(0, M))
        bp, n = int(rng.integers(0, 60)), int(rng.integers(1, 12))
        vals = rng.random((M, M))
        r = R.prune(M, start, pos, bp, n, 0.5, lambda j, i: vals[j, i])
        assert r.max_dist <= R.band_width(M, start, pos, bp, n)
    assert R.band_width(30, 7, [5] * 30, BIG, R.INT_MAX) == 29


# ---- the file and the library --------------------------------------------------------------------------------------------------
def test_open_gds_reads_snp_position(hapmap):
    p = hapmap.snp_position
    assert p is not None and p.dtype == np.int32 and p.shape == (9088,)
    for ch in np.unique(hapmap.snp_chromosome):
        assert np.all(np.diff(p[hapmap.snp_chromosome == ch]) >= 0), ch


def test_library_exports_the_pruning_symbols():
    hdr = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    for s in PRUNE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsnpgpu.so not built")
    L = _lib.lib()
    assert all(hasattr(L, s) for s in PRUNE_SYMBOLS)


def test_shim_registers_gnrLDpruning():
    reg = open(os.path.join(ROOT, "r_shim", "registration.inc")).read()
    assert re.search(r'"gnrLDpruning",\s*\(DL_FUNC\)&gpu_gnrLDpruning,\s*8', reg)
    assert "gpu_gnrLDpruning" in open(os.path.join(ROOT, "r_shim", "gpu_shim.cpp")).read()


# ---- R-level argument errors ---------------------------------------------------------------------------------------------------
def _tiny_file():
    g = np.zeros((4, 3), np.uint8)
    return GenoFile(genotype=g, snp_position=np.arange(4, dtype=np.int32) * 1000)


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(slide_max_bp="x"), TypeError, "is.na(slide.max.bp) | is.numeric(slide.max.bp) is not TRUE"),
    (dict(slide_max_n=True), TypeError, "is.na(slide.max.n) | is.numeric(slide.max.n) is not TRUE"),
    (dict(ld_threshold="0.2"), TypeError, "is.numeric(ld.threshold) is not TRUE"),
    (dict(ld_threshold=float("inf")), ValueError, "is.finite(ld.threshold) is not TRUE"),
    (dict(ld_threshold=float("nan")), ValueError, "is.finite(ld.threshold) is not TRUE"),
    (dict(num_thread=0), ValueError, "num.thread > 0L is not TRUE"),
    (dict(autosave=3), TypeError, "is.null(autosave) | is.character(autosave) is not TRUE"),
    (dict(autosave=""), ValueError, "'autosave' should be NULL or a file name."),
    (dict(start_pos="middle"), ValueError, "'arg' should be one of"),
    (dict(verbose=1), TypeError, "is.logical(verbose) is not TRUE"),
    (dict(method="cov"), ValueError, 'method should be one of "composite", "r", "dprime" and "corr"'),
    (dict(autosave="res.rds"), NotImplementedError, "saveRDS"),
])
def test_argument_errors_before_the_device(kw, exc, msg):
    with pytest.raises(exc) as e:
        api.snpgdsLDpruning(_tiny_file(), **kw)
    assert msg in str(e.value)


def test_file_without_positions_is_an_error():
    with pytest.raises(ValueError, match="snp.position"):
        api.snpgdsLDpruning(GenoFile(genotype=np.zeros((2, 2), np.uint8)))
