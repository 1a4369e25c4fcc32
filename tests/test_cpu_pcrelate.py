"""PC-Relate without a GPU: the numpy restatement (tests/pcrelate_ref.py) against the pedigree it simulates and against itself in
extended precision, the header and the binding, the refusals that need no device, snpgdsIBDSelection on a result."""
import ctypes
import os

import numpy as np
import pytest

import mem_kinds as M
import pcrelate_ref as R
from conftest import ROOT
from snprelate_amd import _lib, api

HEADER = os.path.join(ROOT, "include", "snpgpu.h")
NAMES = ("snpgpu_pcr_create", "snpgpu_pcr_feed", "snpgpu_pcr_result", "snpgpu_pcr_sums", "snpgpu_pcr_stats", "snpgpu_pcr_destroy",
         "snpgpu_gnrPCRelate")


@pytest.fixture(scope="module")
def pedigree():
    """240 samples x 4 000 SNPs, 3 % missing calls; the PC is the true admixture fraction, beta is fitted on the founders"""
    d = R.admixed_families(240, 4000, 7, missing=0.03)
    pcs = (d["admix"] - d["admix"].mean())[:, None]
    d["pcs"] = pcs
    d["ref"] = R.pcrelate(d["geno"], pcs, d["founder"], 0.01)
    return d


def _means(res, pairs):
    i, j = pairs[:, 0], pairs[:, 1]
    return [float(np.nanmean(res[k][i, j])) for k in ("kinship", "k0", "k2")]


def test_pedigree_expectations(pedigree):
    res, pairs = pedigree["ref"]["result"], pedigree["pairs"]
    assert len(pairs["po"]) == 236 and len(pairs["sibs"]) == 59 and len(pairs["spouses"]) == 59 and len(pairs["dup"]) == 1
    for kind, want in (("po", (0.25, 0.0, 0.0)), ("sibs", (0.25, 0.25, 0.25)), ("spouses", (0.0, 1.0, 0.0)), ("unrelated", (0.0, 1.0, 0.0)),
                       ("dup", (0.5, 0.0, 1.0))):
        got = _means(res, pairs[kind])
        print(kind, got)
        assert np.all(np.abs(np.array(got) - np.array(want)) < 0.03), (kind, got)
    i, j = pairs["unrelated"].T
    sd = float(np.nanstd(res["kinship"][i, j]))
    plain = R.pcrelate(pedigree["geno"], None, pedigree["founder"], 0.01, ibd=False)["result"]["kinship"]
    sd_plain = float(np.nanstd(plain[i, j]))
    print("sd of unrelated founders: %.4f with the PC, %.4f without" % (sd, sd_plain))
    assert sd < 0.011 and sd_plain > 1.2 * sd                         # the adjustment is what tightens them
    # the diagonal: kinship_ii = (1 + f_i) / 2 with f ~ 0 for the called samples
    ok = np.isfinite(res["inbreed"])
    assert ok.sum() == 239 and abs(float(res["inbreed"][ok].mean())) < 0.03
    assert np.allclose(np.diag(res["kinship"])[ok], (1 + res["inbreed"][ok]) / 2, rtol=0, atol=1e-15)


def test_generator_plants_what_it_says():
    d = R.admixed_families(77, 500, 3, missing=0.03)
    g, f = d["geno"], d["founder"]
    assert g.shape == (500, 77) and g.dtype == np.uint8 and g.max() == 3
    assert np.all(g[-1, f] == 3) and np.any(g[-1, ~f] < 3)               # no called founder, some called child
    assert np.all((g[-2] == 0) | (g[-2] == 3))                          # monomorphic
    assert np.all(g[:, -2] == 3)                                         # the sample without a call
    both = (g[:, 0] < 3) & (g[:, -1] < 3)
    assert np.array_equal(g[both, 0], g[both, -1]) and both.sum() > 400   # the duplicate
    assert 0.01 < np.mean(g[:-2, :-2] == 3) < 0.06


def test_float64_against_long_double():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is double on this platform")
    d = R.admixed_families(77, 500, 3, missing=0.03)
    g, T = d["geno"], d["founder"]
    pcs = np.stack([d["admix"] - d["admix"].mean(), np.random.default_rng(5).normal(0, 0.1, 77)], 1)
    lo = R.pcrelate(g, pcs, T, 0.01)
    b_hi, used, bound = R.beta(g, lo["W"], T, np.longdouble)
    assert np.array_equal(used, lo["used"]) and used.sum() == 499
    err = np.abs((lo["beta"] - b_hi).astype(np.float64))
    print("beta: worst error / bound %.3g" % float((err[bound > 0] / bound[bound > 0]).max()))     # (a monomorphic SNP: 0 <= 0)
    assert np.all(err <= bound)
    hi = R.pcrelate(g, pcs, T, 0.01, dtype=np.longdouble, b=lo["beta"])
    assert np.array_equal(hi["ops"]["valid"], lo["ops"]["valid"])
    for name in R.PLANES:
        tol = R.plane_bound(hi["mag"][name], 500, 2)
        e = float(np.abs(lo["planes"][name] - hi["planes"][name]).max())
        print("%s: worst error %.3g, bound %.3g (%.2f %%)" % (name, e, tol, 100 * e / tol))
        assert e <= tol
    assert np.array_equal(lo["planes"]["NS"], hi["planes"]["NS"].astype(np.float64))
    assert np.array_equal(lo["planes"]["IBS0"], hi["planes"]["IBS0"].astype(np.float64))


def test_regression_matrix_is_a_left_inverse():
    rng = np.random.default_rng(1)
    V = R.design(rng.normal(0, 0.1, (40, 3)), 40)
    T = np.arange(40) % 5 != 4
    W = R.regression_matrix(V, T)
    assert np.all(W[~T] == 0)
    assert np.allclose(W[T].T @ V[T], np.eye(4), atol=1e-12)
    assert np.allclose(W.sum(0), [1, 0, 0, 0], atol=1e-12)               # sum_{i in T} W_i = e_0
    with pytest.raises(ValueError, match="collinear"):
        R.regression_matrix(R.design(np.ones((16, 1)), 16))


# ---- the header and the binding ----------------------------------------------------------------------------------------------------

def test_header_declares_the_seven_functions():
    text = open(HEADER).read()
    protos = M.header_prototypes(text)
    L = _lib.lib()
    for f in NAMES:
        assert f in protos and f in _lib.EXPORTS and hasattr(L, f), f
    assert protos["snpgpu_pcr_create"] == ["n_samp", "n_pc", "pcs", "training", "maf_thresh", "flags", "opts", "out"]
    assert protos["snpgpu_pcr_feed"] == ["pcr", "geno", "n_snp", "format", "mem", "beta"]
    assert protos["snpgpu_pcr_result"] == ["pcr", "kinship", "inbreed", "k0", "k2", "nsnp"]
    assert protos["snpgpu_pcr_sums"] == ["pcr", "which", "plane"]
    assert protos["snpgpu_pcr_stats"] == ["pcr", "stats"]
    assert protos["snpgpu_pcr_destroy"] == ["pcr"]
    assert protos["snpgpu_gnrPCRelate"] == ["n_pc", "pcs", "training", "maf_thresh", "flags", "kinship", "inbreed", "k0", "k2", "nsnp"]
    for f in NAMES:
        assert "out_mem" not in protos[f] and "dst_mem" not in protos[f] and protos[f][0] not in ("ctx", "m")
    assert "enum { SNPGPU_PCR_IBD = 1 };" in text and _lib.PCR_IBD == 1
    assert "#define SNPGPU_ABI_VERSION 2\n" in text                      # additions only: the version stays
    assert text.index("snpgpu_pcr_create") > text.index("int snpgpu_diag_carry_fallbacks")      # the additions come last
    assert _lib.PCR_PLANES == R.PLANES


def test_python_interface():
    import inspect
    import snprelate_amd
    assert snprelate_amd.snpgdsPCRelate is api.snpgdsPCRelate
    sig = inspect.signature(api.snpgdsPCRelate)
    assert list(sig.parameters) == ["gdsobj", "pcs", "n_pcs", "sample_id", "snp_id", "autosome_only", "remove_monosnp", "maf", "missing_rate",
                                    "training_id", "maf_thresh", "ibd_probs", "verbose", "device"]
    p = sig.parameters
    assert p["n_pcs"].default is None and p["maf_thresh"].default == 0.01 and p["ibd_probs"].default is True
    assert np.isnan(p["maf"].default) and np.isnan(p["missing_rate"].default) and p["autosome_only"].default is True
    assert "inbreed" in api._IBD_NOT_PER_PAIR


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------

def _refused(rc, fn, text):
    assert rc != 0
    msg = _lib.lib().snpgpu_last_error().decode()
    assert msg.startswith(fn + ": ") and text in msg, msg


def _create(n, pcs, training=None, maf=0.01, flags=1, out=True):
    L = _lib.lib()
    h = ctypes.c_void_p()
    pcs = None if pcs is None else np.ascontiguousarray(pcs, np.float64)
    n_pc = 0 if pcs is None else pcs.shape[1]
    tr = None if training is None else np.ascontiguousarray(training, np.uint8)
    rc = L.snpgpu_pcr_create(n, n_pc, _lib._ptr(pcs), _lib._ptr(tr), maf, flags, None, ctypes.byref(h) if out else None)
    assert not h.value
    return rc


def test_create_refusals():
    fn = "snpgpu_pcr_create"
    rng = np.random.default_rng(0)
    pcs = rng.normal(0, 0.1, (20, 2))
    _refused(_create(20, pcs, out=False), fn, "out is NULL")
    _refused(_create(0, None), fn, "invalid number of samples")
    L = _lib.lib()
    h = ctypes.c_void_p()
    _refused(L.snpgpu_pcr_create(20, 33, _lib._ptr(np.zeros((20, 33))), None, 0.01, 1, None, ctypes.byref(h)), fn, "0 ... 32")
    _refused(L.snpgpu_pcr_create(20, -1, None, None, 0.01, 1, None, ctypes.byref(h)), fn, "0 ... 32")
    _refused(L.snpgpu_pcr_create(20, 2, None, None, 0.01, 1, None, ctypes.byref(h)), fn, "pcs is NULL")
    for bad in (0.0, 0.5, -0.1, 0.7, float("nan")):
        _refused(_create(20, pcs, maf=bad), fn, "maf_thresh must be inside (0, 0.5)")
    _refused(_create(20, pcs, flags=2), fn, "unknown flags")
    _refused(_create(20, pcs, flags=-1), fn, "unknown flags")
    tr = np.zeros(20, np.uint8)
    tr[:3] = 1
    _refused(_create(20, pcs, training=tr), fn, "too few training samples: 3")
    _refused(_create(1, None), fn, "too few training samples: 1")
    for bad in (np.nan, np.inf):
        q = pcs.copy()
        q[7, 1] = bad
        _refused(_create(20, q), fn, "not finite")
    _refused(_create(16, np.ones((16, 1))), fn, "the principal components are collinear in the training set")
    q = pcs.copy()
    q[:, 1] = 3 * q[:, 0]
    _refused(_create(20, q), fn, "the principal components are collinear in the training set")
    tr = np.ones(20, np.uint8)
    q = pcs.copy()
    q[:10, 0] = 0.25                                                       # constant on the training set only
    tr[10:] = 0
    _refused(_create(20, q, training=tr), fn, "collinear in the training set")


def test_other_refusals():
    L = _lib.lib()
    buf = np.zeros(16, np.float64)
    g = np.zeros((2, 4), np.uint8)
    _refused(L.snpgpu_pcr_feed(None, _lib._ptr(g), 2, 7, _lib.HOST, None), "snpgpu_pcr_feed", "invalid genotype format")
    _refused(L.snpgpu_pcr_feed(None, _lib._ptr(g), 2, _lib.GENO_U8, 5, None), "snpgpu_pcr_feed", "invalid memory kind")
    _refused(L.snpgpu_pcr_feed(None, _lib._ptr(g), -1, _lib.GENO_U8, _lib.HOST, None), "snpgpu_pcr_feed", "invalid number of SNPs")
    _refused(L.snpgpu_pcr_feed(None, _lib._ptr(g), 2, _lib.GENO_U8, _lib.HOST, None), "snpgpu_pcr_feed", "pcr is NULL")
    _refused(L.snpgpu_pcr_result(None, _lib._ptr(buf), None, None, None, None), "snpgpu_pcr_result", "pcr is NULL")
    _refused(L.snpgpu_pcr_sums(None, 0, _lib._ptr(buf)), "snpgpu_pcr_sums", "NULL argument")
    _refused(L.snpgpu_pcr_stats(None, _lib._ptr(buf)), "snpgpu_pcr_stats", "NULL argument")
    assert L.snpgpu_pcr_destroy(None) == 0
    _lib.check(L.snpgpu_ws_clear())
    _refused(L.snpgpu_gnrPCRelate(0, None, None, 0.01, 1, _lib._ptr(buf), None, None, None, None), "snpgpu_gnrPCRelate",
             "no genotype working space")
    with pytest.raises(_lib.SnpGpuError, match="maf_thresh"):
        _lib.PCRelate(20, maf_thresh=0.6)
    with pytest.raises(ValueError, match="one row per sample"):
        _lib.PCRelate(20, pcs=np.zeros((19, 2)))
    with pytest.raises(ValueError, match="one flag per sample"):
        _lib.PCRelate(20, training=np.ones(3))


# ---- snpgdsIBDSelection on a result --------------------------------------------------------------------------------------------------

def test_ibd_selection_tabulates_a_result(pedigree):
    res = pedigree["ref"]["result"]
    n = 240
    ids = np.array(["s%03d" % i for i in range(n)])
    obj = dict(sample_id=ids, snp_id=np.arange(4000), kinship=res["kinship"], k0=res["k0"], k1=res["k1"], k2=res["k2"], nsnp=res["nsnp"],
               inbreed=res["inbreed"])
    tab = api.snpgdsIBDSelection(obj, 0.1)
    assert list(tab) == ["ID1", "ID2", "kinship", "k0", "k1", "k2", "nsnp"]
    with np.errstate(invalid="ignore"):
        want = {(int(j), int(i)) for i, j in zip(*np.nonzero(np.tril(res["kinship"] >= 0.1, -1)))}
    got = {(int(a[1:]), int(b[1:])) for a, b in zip(tab["ID1"], tab["ID2"])}
    assert got == want
    planted = {tuple(sorted(map(int, p))) for k in ("po", "sibs", "dup") for p in pedigree["pairs"][k]}
    planted = {p for p in planted if 238 not in p}                        # the sample without a call has no kinship
    assert planted <= got and len(got - planted) <= 2
    i = np.array([int(a[1:]) for a in tab["ID1"]])
    j = np.array([int(b[1:]) for b in tab["ID2"]])
    assert np.array_equal(tab["kinship"], res["kinship"][j, i]) and np.array_equal(tab["nsnp"], res["nsnp"][j, i])
    every = api.snpgdsIBDSelection(obj)
    assert len(every["ID1"]) == n * (n - 1) // 2
