"""CPU-side tests of snpgdsFst / snpgdsSlidingWindow: the numpy restatement (tests/fst_ref.py) against exact rational arithmetic
and against answers known without the reference, the window bookkeeping of the API against the reference's direct loop, every
argument error of the C ABI and of the Python functions raised without a device, the library's exports, the R shim's registration
and the no-GPU failure mode."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import fst_ref as R
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FST_SYMBOLS = ["snpgpu_pop_counts", "snpgpu_fst", "snpgpu_fst_windows", "snpgpu_pop_stats", "snpgpu_gnrFst",
               "snpgpu_gnrSlidingWindowFst"]
METHODS = ("W&C84", "W&H02")


def _edge_genotypes(n_pop, n=37, m=41, seed=5):
    """n samples (not a multiple of 4); a population of ONE sample; SNPs where a whole population is missing, monomorphic SNPs (all
    0, all 2), an all-missing SNP, 12 % missing elsewhere"""
    rng = np.random.default_rng(seed)
    pop = np.concatenate([[0], rng.integers(1, n_pop, n - 1)]).astype(np.int32)      # population 0: sample 0 alone
    pop[1:n_pop] = np.arange(1, n_pop)                                                # every population present
    p = rng.uniform(0.05, 0.95, m)
    g = ((rng.random((m, n)) < p[:, None]).astype(np.uint8) + (rng.random((m, n)) < p[:, None]).astype(np.uint8))
    g[rng.random((m, n)) < 0.12] = 3
    g[3] = 0
    g[8] = 2
    g[13] = 3
    g[17][pop == 1] = 3                     # population 1 without any call
    g[21, 0] = 3                            # the one-sample population missing
    g[25][pop == n_pop - 1] = 3
    return g, pop


def _close(got, exact, bound):
    if exact is None:
        return not math.isfinite(got)
    return math.isfinite(got) and abs(got - float(exact)) <= bound


@pytest.mark.parametrize("n_pop", [2, 7])
@pytest.mark.parametrize("method", METHODS)
def test_restatement_matches_exact_arithmetic(n_pop, method):
    g, pop = _edge_genotypes(n_pop)
    a, c = R.pop_counts(g, pop, n_pop)
    assert (c[17, 1] == 0) and (c[21, 0] == 0) and (c[13] == 0).all()
    got = R.snpgds_fst(g, pop, n_pop, method)
    want = R.exact_fst(a, c, method)
    # a population without a call -> NaN and left out of every sum
    for s in (13, 17, 21, 25):
        assert np.isnan(got["FstSNP"][s]) and want["FstSNP"][s] is None
    assert got["n"] == sum(1 for s in range(len(g)) if (c[s] > 0).all())
    # monomorphic SNPs: 0 / 0
    for s in (3, 8):
        assert np.isnan(got["FstSNP"][s]) and want["FstSNP"][s] is None and (c[s] > 0).all()
    n_val = 0
    for s in range(len(g)):
        assert _close(got["FstSNP"][s], want["FstSNP"][s], got["FstSNP_bound"][s]), (s, got["FstSNP"][s], want["FstSNP"][s])
        n_val += want["FstSNP"][s] is not None
    assert n_val >= 20
    assert _close(got["Fst"], want["Fst"], got["Fst_bound"])
    assert got["Fst_bound"] < 1e-9          # the bound is far below the values it guards (|Fst| ~ 1e-2 ... 1)
    if method == "W&H02":
        for k1 in range(n_pop):
            for k2 in range(n_pop):
                assert _close(got["Beta"][k1, k2], want["Beta"][k1][k2], got["Beta_bound"][k1, k2])
        assert np.array_equal(got["Beta"], got["Beta"].T)
    # a subset of SNPs, as a window takes it
    sub = np.array([1, 2, 3, 17, 20, 30, 40])
    ws, we = R.fst_set(a, c, method, sub), R.exact_fst(a, c, method, sub)
    assert _close(ws["Fst"], we["Fst"], ws["Fst_bound"])


def test_populations_fixed_for_opposite_alleles():
    g = np.zeros((5, 10), np.uint8)
    g[:, 5:] = 2
    pop = np.array([0] * 5 + [1] * 5, np.int32)
    r = R.snpgds_fst(g, pop, 2, "W&C84")
    assert r["Fst"] == 1.0 and (r["FstSNP"] == 1.0).all() and r["MeanFst"] == 1.0
    r = R.snpgds_fst(g, pop, 2, "W&H02")
    assert r["Fst"] == 1.0 and (r["FstSNP"] == 1.0).all()
    assert np.array_equal(np.diag(r["Beta"]), [1.0, 1.0]) and r["Beta"][0, 1] == 0.0 and r["Beta"][1, 0] == 0.0


@pytest.mark.parametrize("n_pop,n_each", [(2, 4), (3, 5), (7, 3)])
def test_identical_allele_counts_give_the_negative_value_of_the_formula(n_pop, n_each):
    """MSB = 0: numerator -MSW, denominator (n_c - 1) MSW with n_c = 2 n for K populations of n samples: Fst = -1 / (2 n - 1)"""
    one = np.array([0, 1, 2] + [1] * (n_each - 3), np.uint8)[:n_each]
    g = np.tile(one, (4, n_pop))
    pop = np.repeat(np.arange(n_pop), n_each).astype(np.int32)
    a, c = R.pop_counts(g, pop, n_pop)
    assert (a == a[:, :1]).all() and (c == 2 * n_each).all()
    num, den, valid, _, _ = R.wc84_terms(a, c)
    ex = R.exact_wc84(a[0], c[0])
    assert ex[0] < 0 and ex[0] / ex[1] == Fraction(-1, 2 * n_each - 1)
    assert (num < 0).all() and valid.all()
    r = R.snpgds_fst(g, pop, n_pop, "W&C84")
    assert r["Fst"] < 0 and abs(r["Fst"] + 1.0 / (2 * n_each - 1)) <= r["Fst_bound"]


# ---- window bookkeeping ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,end,winsize,shift", [(1, 100, 10, 5), (1, 5, 10, 3), (7, 7, 1, 1), (0, 99, 100, 10), (50, 40, 5, 5),
                                                     (3, 1000, 17, 13)])
def test_sliding_num_win(start, end, winsize, shift):
    assert api.sliding_num_win(start, end, winsize, shift) == R.sliding_num_win(start, end, winsize, shift)


def _api_windows(chpos, winsize, shift, unit, winstart):
    """the membership snpgdsSlidingWindow computes for one chromosome (the code path of the named FUNs)"""
    chpos = np.asarray(chpos, np.int64)
    if unit == "basepair":
        start, end, key = (int(chpos.min()) if winstart is None else winstart), int(chpos.max()), chpos
    else:
        start, end, key = (0 if winstart is None else winstart - 1), len(chpos) - 1, np.arange(len(chpos), dtype=np.int64)
    n_win = api.sliding_num_win(start, end, winsize, shift)
    return api._window_members(start + shift * np.arange(n_win, dtype=np.int64), key, winsize)


@pytest.mark.parametrize("unit", ["basepair", "locus"])
@pytest.mark.parametrize("winstart", [None, 1, 40, 500])
@pytest.mark.parametrize("sorted_pos", [True, False])
def test_window_membership_matches_the_direct_loop(unit, winstart, sorted_pos):
    rng = np.random.default_rng(9)
    pos = np.concatenate([rng.integers(30, 400, 60), rng.integers(900, 1300, 45), [400, 400, 1299]])   # a gap: empty windows; ties
    pos = np.sort(pos) if sorted_pos else pos
    winsize, shift = (90, 25) if unit == "basepair" else (11, 4)
    members, num, mean_pos, posrange = R.sliding_windows(pos, winsize, shift, unit, winstart)
    offsets, idx = _api_windows(pos, winsize, shift, unit, winstart)
    assert len(offsets) - 1 == len(members)
    assert np.array_equal(np.diff(offsets), num)
    for w, m in enumerate(members):
        assert np.array_equal(idx[offsets[w]:offsets[w + 1]], m), w
    if unit == "basepair" and winstart in (None, 1, 40):
        assert (num == 0).any()
    assert posrange == (pos.min(), pos.max())


def _cpu_workspace(monkeypatch):
    """snpgdsSlidingWindow with a callable FUN is host-only once the working space is chosen: replace .InitFile2 (which installs
    the genotypes on the device) by the plain selection"""
    def init(cmd, gdsobj, sample_id, snp_id, *a, **k):
        sid = api._working_sample_ids(gdsobj, sample_id)
        flag = np.ones(gdsobj.n_snp, bool) if snp_id is None else np.isin(gdsobj.snp_id, snp_id)
        return dict(sample_id=sid, snp_id=gdsobj.snp_id[flag], n_snp=int(flag.sum()), n_samp=len(sid), packed=gdsobj.packed[flag])
    monkeypatch.setattr(api, "_init_file2", init)


def _file(seed=2):
    rng = np.random.default_rng(seed)
    chrom = np.array([2] * 30 + [0] * 4 + [1] * 25 + [2] * 6 + [5] * 12, np.int32)       # order of first appearance: 2, 1, 5
    pos = rng.integers(1, 3000, len(chrom)).astype(np.int32)                               # unsorted
    pos[[3, 40]] = 0                                                                       # dropped
    g = rng.integers(0, 3, (len(chrom), 9)).astype(np.uint8)
    return GenoFile(genotype=g, snp_chromosome=chrom, snp_position=pos, snp_id=np.arange(100, 100 + len(chrom)))


@pytest.mark.parametrize("unit", ["basepair", "locus"])
@pytest.mark.parametrize("with_id", ["snp.id", "snp.id.in.window", "none"])
def test_callable_fun_follows_the_r_loop(monkeypatch, unit, with_id):
    _cpu_workspace(monkeypatch)
    f = _file()
    winsize, shift = (700, 300) if unit == "basepair" else (7, 3)
    calls = []

    def fun(samples, snp_ids, positions, scale=1):
        calls.append((len(samples), list(snp_ids)))
        return scale * len(snp_ids)
    r = api.snpgdsSlidingWindow(f, FUN=fun, winsize=winsize, shift=shift, unit=unit, winstart=[1, 2, 3] if unit == "locus" else None,
                                as_is="numeric", with_id=with_id, verbose=False, scale=2)
    assert [k for k in r if k.startswith("chr") and k.count(".") == 0] == ["chr2", "chr1", "chr5"]
    assert ("snp_id" in r) == (with_id != "none") and ("chr2.snpid" in r) == (with_id == "snp.id.in.window")
    chrom, pos, ids = f.snp_chromosome, f.snp_position, f.snp_id
    for ci, ch in enumerate((2, 1, 5)):
        flag = (chrom == ch) & (pos > 0)
        p, sid = pos[flag].astype(np.int64), ids[flag]
        key = "chr%d" % ch
        assert tuple(r[key + ".posrange"]) == (p.min(), p.max())
        if unit == "basepair":
            n = R.sliding_num_win(int(p.min()), int(p.max()), winsize, shift)
            assert len(r[key]) == n
            for i in range(n):
                x = int(p.min()) + i * shift
                k = (x <= p) & (p < x + winsize)
                assert r[key + ".num"][i] == k.sum() and r[key][i] == 2 * k.sum()
                assert (np.isnan(r[key + ".pos"][i]) and not k.any()) or r[key + ".pos"][i] == p[k].mean()
                if with_id == "snp.id.in.window":
                    assert np.array_equal(r[key + ".snpid"][i], sid[k])
        else:
            n = R.sliding_num_win(ci + 1, len(p), winsize, shift)          # winstart enters the count only
            assert len(r[key]) == n
            for i in range(n):
                lo = i * shift
                m = min(lo + winsize, len(p)) - lo
                assert r[key + ".num"][i] == winsize and r[key][i] == 2 * max(m, 0)
                assert r[key + ".pos"][i] == p[lo:lo + winsize].mean() if m == winsize else np.isnan(r[key + ".pos"][i])
    assert all(c[0] == 9 for c in calls)
    lst = api.snpgdsSlidingWindow(f, FUN=lambda s, i, p: {"n": len(i)}, winsize=winsize, shift=shift, unit=unit, as_is="list",
                                  verbose=False)
    assert lst["chr1"][0] == {"n": int(r["chr1"][0]) // 2}


# ---- argument errors, all before a device is touched --------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_c_abi_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    g = np.zeros((6, 2), np.uint8)             # 6 SNPs x 5 samples, 2-bit rows
    pop = np.array([0, 0, 1, 1, 1], np.int32)
    a, c = np.zeros((6, 3), np.int32), np.zeros((6, 3), np.int32)
    out = np.zeros(64)

    def err():
        return L.snpgpu_last_error().decode()

    def counts(p, k):
        return L.snpgpu_pop_counts(_vp(g), 6, 5, _lib.GENO_PACKED2, _lib.HOST, _vp(p), k, _vp(a), _vp(c), _lib.HOST, 0)
    assert counts(pop, 1) != 0 and "at least two populations" in err()
    assert counts(np.array([0, 0, 1, 2, 1], np.int32), 2) != 0 and "outside the populations" in err()
    assert counts(np.array([0, -1, 1, 1, 1], np.int32), 2) != 0 and "outside the populations" in err()
    assert counts(pop, 3) != 0 and "at least one individual" in err()
    assert L.snpgpu_pop_counts(_vp(g), 6, 5, 7, _lib.HOST, _vp(pop), 2, _vp(a), _vp(c), _lib.HOST, 0) != 0 and "format" in err()
    assert L.snpgpu_pop_counts(None, 6, 5, _lib.GENO_PACKED2, _lib.HOST, _vp(pop), 2, _vp(a), _vp(c), _lib.HOST, 0) != 0
    assert L.snpgpu_fst(_vp(g), 6, 5, _lib.GENO_PACKED2, _lib.HOST, _vp(pop), 2, 3, _vp(out), None, None, 0) != 0
    assert "Fst method" in err()

    def windows(off, idx):
        off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int32)
        return L.snpgpu_fst_windows(_vp(g), 6, 5, _lib.GENO_PACKED2, _lib.HOST, _vp(pop), 2, 1, _vp(off), _vp(idx), len(off) - 1,
                                    _vp(out), None, None, 0)
    assert windows([0, 2, 4], [0, 1, 3, 2]) != 0 and "ascend" in err()
    assert windows([0, 2, 4], [0, 1, 1, 1]) != 0 and "ascend" in err()
    assert windows([0, 2, 4], [0, 1, 3, 6]) != 0 and "outside the genotype rows" in err()
    assert windows([0, 3, 2], [0, 1, 2]) != 0 and "decrease" in err()
    assert windows([1, 2], [0, 1]) != 0 and "offsets[0]" in err()
    # workspace level: method and population count come first
    one = np.array([1, 1, 2, 2, 2], np.int32)
    assert L.snpgpu_gnrFst(_vp(one), 2, b"W&C85", _vp(out), None, None) != 0 and "W&C84" in err()
    assert L.snpgpu_gnrFst(_vp(one), 1, b"W&C84", _vp(out), None, None) != 0 and "at least two populations" in err()
    off = np.array([0, 1], np.int64)
    assert L.snpgpu_gnrSlidingWindowFst(_vp(one), 2, b"x", _vp(off), _vp(one), 1, _vp(out), None, None) != 0 and "method" in err()
    assert L.snpgpu_gnrSlidingWindowFst(_vp(one), 2, b"W&H02", None, None, 1, _vp(out), None, None) != 0 and "offsets" in err()


def test_python_argument_errors_need_no_device():
    f = _file()
    pop = ["a", "b", "c"] * 3
    W = api.snpgdsSlidingWindow
    with pytest.raises(TypeError, match="is.numeric\\(winsize\\)"):
        W(f, FUN="snpgdsSNPRateFreq", winsize="100")
    with pytest.raises(TypeError, match="is.numeric\\(shift\\)"):
        W(f, FUN="snpgdsSNPRateFreq", shift=None)
    with pytest.raises(ValueError, match="is.finite"):
        W(f, FUN="snpgdsSNPRateFreq", winsize=float("nan"))
    with pytest.raises(ValueError, match="is.finite"):
        W(f, FUN="snpgdsSNPRateFreq", shift=float("inf"))
    with pytest.raises(TypeError, match="'FUN' should be a function, or a character"):
        W(f)
    with pytest.raises(ValueError, match="'FUN' should be one of snpgdsFst,snpgdsSNPRateFreq"):
        W(f, FUN="snpgdsIBS")
    with pytest.raises(ValueError, match='FUN="snpgdsFst"'):
        W(f, FUN=api.snpgdsFst)
    with pytest.raises(ValueError, match="Unused additional parameters"):
        W(f, FUN="snpgdsSNPRateFreq", population=pop)
    with pytest.raises(ValueError, match="'winstart' should be specified according to the chromosome set \\(2,1,5\\)"):
        W(f, FUN="snpgdsSNPRateFreq", winstart=[1, 2, 3, 4])
    with pytest.raises(TypeError, match="winstart"):
        W(f, FUN="snpgdsSNPRateFreq", winstart="1")
    with pytest.raises(ValueError, match="unit"):
        W(f, FUN="snpgdsSNPRateFreq", unit="kb")
    with pytest.raises(ValueError, match="as.is"):
        W(f, FUN="snpgdsSNPRateFreq", as_is="matrix")
    with pytest.raises(NotImplementedError, match="stride npop \\+ 1"):
        W(f, FUN="snpgdsFst", as_is="array", population=pop)
    with pytest.raises(TypeError, match="is.factor\\(population\\)"):
        W(f, FUN="snpgdsFst")
    # .paramFst
    F = api.snpgdsFst
    with pytest.raises(ValueError, match="number of samples in the GDS file"):
        F(f, pop[:8])
    with pytest.raises(ValueError, match="same as the length of 'sample.id'"):
        F(f, pop, sample_id=[1, 2, 3])
    with pytest.raises(ValueError, match="missing values"):
        F(f, ["a", None, "b"] * 3)
    with pytest.raises(ValueError, match="missing values"):
        F(f, [1.0, float("nan"), 2.0] * 3)
    with pytest.raises(ValueError, match="at least two populations"):
        F(f, ["a"] * 9)
    with pytest.raises(ValueError, match="'method' should be one of"):
        F(f, pop, method="W&C85")
    with pytest.raises(TypeError, match="is.factor"):
        F(f, None)


def test_param_fst_reorders_like_match():
    ws_ids = np.array([1, 2, 3, 4, 5, 6])
    v = api._param_fst(None, ["y", "x", "y", "z", "x", "z"], None, ws_ids)
    assert v["levels"] == ["x", "y", "z"] and list(v["population"]) == [2, 1, 2, 3, 1, 3] and v["method"] == "W&C84"
    # sample.id in another order than the file's: population[match(ws$sample.id, sample.id)]
    v = api._param_fst([5, 3, 1, 2], ["p", "q", "r", "q"], ("W&C84", "W&H02"), np.array([1, 2, 3, 5]))
    assert list(v["population"]) == [3, 2, 2, 1] and list(v["sizes"]) == [1, 2, 1]
    with pytest.raises(ValueError, match="at least one individual"):
        api._param_fst([5, 3, 1, 1], ["p", "q", "r", "s"], "W&H02", np.array([1, 3, 5]))     # level "s" is never matched


def test_open_gds_reads_the_sample_annotation(hapmap):
    grp = hapmap.sample_annot["pop.group"]
    assert len(grp) == hapmap.n_samp == 279 and sorted(set(grp)) == ["CEU", "HCB", "JPT", "YRI"]
    assert set(hapmap.sample_annot) >= {"family.id", "father.id", "mother.id", "sex", "pop.group"}


def test_library_exports_the_fst_symbols():
    hdr = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    assert re.search(r"SNPGPU_ABI_VERSION\s+2\b", hdr)
    for s in FST_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in FST_SYMBOLS:
        assert hasattr(L, s), s


def test_shim_registers_gnrFst():
    """gnrSlidingWindow has no shim body: it needs the working space's SNP selection vector, which the kept header's mock does not
    declare (INTEGRATION.md says so)"""
    reg = open(os.path.join(ROOT, "r_shim", "registration.inc")).read()
    assert re.search(r'"gnrFst",\s*\(DL_FUNC\)&gpu_gnrFst,\s*3', reg)
    assert "gpu_gnrFst" in open(os.path.join(ROOT, "r_shim", "gpu_shim.cpp")).read()
    assert "gnrSlidingWindow" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _has_gpu():
    try:
        return _lib.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_snpgdsFst_fails_loudly_without_gpu():
    f = GenoFile(genotype=np.array([[0, 1, 2, 1], [1, 1, 0, 2], [2, 0, 1, 1]], np.uint8))
    with pytest.raises(_lib.SnpGpuError):
        api.snpgdsFst(f, ["a", "a", "b", "b"], verbose=False)
    with pytest.raises(_lib.SnpGpuError):
        _lib.pop_counts(np.zeros((3, 4), np.uint8), 4, [0, 0, 1, 1], 2)
