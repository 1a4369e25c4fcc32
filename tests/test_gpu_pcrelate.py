"""PC-Relate on the GPU (snpgpu_pcr_*, snpgpu_gnrPCRelate, snpgdsPCRelate) against the numpy restatement of its definitions
(tests/pcrelate_ref.py).

The shapes: n in {1, 3, 17, 65, 130, 257} (less than one MFMA tile, one plus one, a workgroup tile plus a ragged edge, three
workgroup tiles, n no multiple of 4 or 16), M in {1, 3, 500, 1030}, D in {0, 1, 2, 5}, missing rates {0, 0.03, 0.3}, the training
set all samples or every sample except each fifth -- a dozen combinations that cover every value.  n = 1 cannot be created: the
library refuses fewer than n_pc + 2 training samples, so that combination asserts the refusal (at the device, whose presence the
other combinations show) and the smallest shape that computes is n = 3.  The three samples go with D = 0: the third is the
duplicate of the first, so one PC fits them exactly, every residual is rounding alone and the plane bound -- relative to
sum |x| |y| -- has nothing to hold on to.

Per combination the device is run once (one object, the whole set in one feed, beta returned) and the reference once, in long
double, from the beta the device returned; every test of the combination reads those.  Bounds (pcrelate_ref): beta within
2 (n_T + 8) 2^-53 sum |g~ W| per entry; a plane within 2 (M + 8 (D + 2)) 2^-53 max_ij sum_s |x_is| |y_js|; IBS0 and NS equal.
Observed on an MI355X: the worst beta entry at 0.10 of its bound, the worst plane at 0.059 of its bound (K0D at M = 3)."""
import functools

import numpy as np
import pytest

import pcrelate_ref as R
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows

pytestmark = pytest.mark.gpu

LD = np.longdouble
#        n    M    D  missing  training
CASES = [(3, 500, 0, 0.0, "all"),
         (3, 1030, 0, 0.3, "fifth"),
         (17, 500, 5, 0.03, "all"),
         (17, 3, 2, 0.0, "fifth"),
         (65, 500, 2, 0.3, "fifth"),
         (65, 1030, 1, 0.03, "all"),
         (130, 1030, 2, 0.03, "fifth"),
         (130, 1, 0, 0.0, "all"),
         (130, 500, 5, 0.3, "all"),
         (257, 500, 5, 0.03, "fifth"),
         (257, 3, 1, 0.3, "all")]
REFUSED = (1, 3, 0, 0.0, "all")
IDS = ["n%d-M%d-D%d-miss%g-%s" % c for c in CASES]
RICH = [c for c in CASES if c[0] >= 17 and c[1] >= 500]        # families, the planted sample without a call, the special SNPs


def test_the_combinations_cover_every_value():
    every = CASES + [REFUSED]
    assert {c[0] for c in every} == {1, 3, 17, 65, 130, 257} and {c[1] for c in every} == {1, 3, 500, 1030}
    assert {c[2] for c in every} == {0, 1, 2, 5} and {c[3] for c in every} == {0.0, 0.03, 0.3} and {c[4] for c in every} == {"all", "fifth"}
    assert len(every) == 12


@functools.lru_cache(maxsize=None)
def inputs(case):
    n, m, D, miss, train = case
    T = np.ones(n, bool) if train == "all" else np.arange(n) % 5 != 4
    d = R.admixed_families(n, m, 1000 + 7 * n + m + D, missing=miss, training=T)
    rng = np.random.default_rng(n + m)
    pcs = np.concatenate([(d["admix"] - d["admix"].mean())[:, None], rng.normal(0, 0.1, (n, 5))], 1)[:, :D]
    g = d["geno"]
    g.setflags(write=False)
    return dict(geno=g, packed=pack_2bit_rows(g), pcs=pcs, T=T, pairs=d["pairs"])


def _object(case, ibd=True):
    i = inputs(case)
    return _lib.PCRelate(case[0], pcs=i["pcs"] if case[2] else None, training=None if case[4] == "all" else i["T"], maf_thresh=0.01, ibd=ibd)


def _planes(p, names=R.PLANES):
    return {k: p.sums(k) for k in names}


@functools.lru_cache(maxsize=None)
def run(case):
    """the device's beta, planes, results and statistics of one feed of the whole set; the long-double reference from that beta"""
    i = inputs(case)
    with _object(case) as p:
        b = p.feed(i["packed"], fmt=_lib.GENO_PACKED2, want_beta=True)
        planes, res, stats = _planes(p), p.result(), p.stats()
    ref = R.pcrelate(i["geno"], i["pcs"], i["T"], 0.01, dtype=LD, b=b)
    for a in list(planes.values()) + list(res.values()) + [b]:
        a.setflags(write=False)
    return dict(beta=b, planes=planes, res=res, stats=stats, ref=ref)


def test_one_sample_is_refused_by_the_training_rule():
    assert _lib.device_count() >= 1
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_create: too few training samples: 1"):
        _lib.PCRelate(REFUSED[0])


# ---- 1. beta ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_beta(case):
    r = run(case)
    ref = r["ref"]
    assert r["beta"].shape == (case[1], case[2] + 1)
    err = np.abs((r["beta"].astype(LD) - ref["beta"]).astype(np.float64))
    ok = ref["beta_bound"] > 0
    print("beta: worst error / bound %.3g" % (float((err[ok] / ref["beta_bound"][ok]).max()) if ok.any() else 0.0))
    assert np.all(err <= ref["beta_bound"])
    assert np.all(r["beta"][~ref["used"]] == 0)                           # a SNP without a called training sample


# ---- 2. planes -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_from_the_device_beta(case):
    r = run(case)
    ref = r["ref"]
    for name in R.PLANES:
        got, want = r["planes"][name], ref["planes"][name]
        assert got.shape == want.shape == (case[0], case[0])
        tol = R.plane_bound(ref["mag"][name], case[1], case[2])
        e = float(np.abs(got.astype(LD) - want).max())
        print("%s: worst error %.3g, bound %.3g" % (name, e, tol))
        assert np.all(np.isfinite(got)) and e <= tol, name
    for name in ("IBS0", "NS"):
        assert np.array_equal(r["planes"][name], ref["planes"][name].astype(np.float64)), name
        assert np.array_equal(r["planes"][name], np.rint(r["planes"][name]))
    for name in R.PLANES:
        if name != "DC":
            assert np.array_equal(r["planes"][name], r["planes"][name].T), name       # mirrored at result time


# ---- 3. results ------------------------------------------------------------------------------------------------------------------------

def _propagated(P, tol):
    """First-order bounds on kinship, inbreed, k2 and k0 for planes within tol of P (long double), doubled for the higher orders,
    plus the handful of fp64 roundings of the finaliser itself (1e-12 relative and absolute, the figure of the direct comparison)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        f = R.finalise(P)
        kin = np.abs(f["kinship"])
        d_kin = (tol["RR"] + 4 * kin * tol["SS"]) / (4 * P["SS"])
        d_e = 2 * np.diag(d_kin)
        e = np.abs(1 + f["inbreed"])
        ei, ej, di, dj = e[:, None], e[None, :], d_e[:, None], d_e[None, :]
        DC, CC = np.abs(P["DC"]), np.abs(P["CC"])
        d_num = (tol["DD"] + ej * tol["DC"] + ei * tol["DC"] + ei * ej * tol["CC"] + dj * DC + di * DC.T + (di * ej + ei * dj) * CC)
        d_k2 = (d_num + np.abs(f["k2"]) * tol["CC"]) / CC
        d_k0 = np.where(f["kinship"] < R.KIN_SPLIT, np.abs(f["k0"]) * tol["K0D"] / P["K0D"], 4 * d_kin + d_k2)
    slop = lambda x, d: (2 * d + 1e-12 * np.abs(x) + 1e-12).astype(np.float64)
    return dict(kinship=slop(f["kinship"], d_kin), inbreed=slop(f["inbreed"], d_e), k2=slop(f["k2"], d_k2), k0=slop(f["k0"], d_k0)), f


def _assert_within(got, want, bound, name):
    want = np.asarray(want).astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), name
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=name)        # NaN where the denominator is zero
    assert np.all(np.abs(got[fin] - want[fin]) <= bound[fin]), name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_results(case):
    r = run(case)
    res = r["res"]
    assert set(res) == {"kinship", "inbreed", "k0", "k2", "nsnp"}
    mine = R.finalise(r["planes"])                                          # float64, on the device's own planes
    for k in ("kinship", "inbreed", "k0", "k2", "nsnp"):
        assert res[k].shape == mine[k].shape
        np.testing.assert_allclose(res[k], mine[k], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=k)
    assert np.array_equal(res["nsnp"], r["planes"]["NS"])
    ref = r["ref"]
    tol = {k: R.plane_bound(ref["mag"][k], case[1], case[2]) for k in R.PLANES}
    bound, want = _propagated(ref["planes"], tol)
    for k in ("kinship", "inbreed", "k0", "k2"):
        _assert_within(res[k], want[k], bound[k], k)


# ---- 4. what the inputs must be for the comparisons to mean something ----------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_decision_of_the_inputs_is_close(case):
    ref = run(case)["ref"]
    i = inputs(case)
    mu = ref["ops"]["mu"].astype(np.float64)
    called = (i["geno"] < 3) & ref["used"][:, None]
    if called.any():
        assert np.abs(mu[called] - 0.01).min() > 1e-9 and np.abs(mu[called] - 0.99).min() > 1e-9
    kin = ref["result"]["kinship"].astype(np.float64)
    assert not np.any(np.abs(kin[np.isfinite(kin)] - R.KIN_SPLIT) < 1e-6)


@pytest.mark.parametrize("case", RICH, ids=["n%d-M%d-D%d-miss%g-%s" % c for c in RICH])
def test_inputs_reach_every_branch(case):
    ref = run(case)["ref"]
    i = inputs(case)
    kin = ref["result"]["kinship"].astype(np.float64)
    off = ~np.eye(case[0], dtype=bool)
    assert np.any(kin[off] < R.KIN_SPLIT) and np.any(kin[off] > R.KIN_SPLIT)       # pairs on both sides of the k0 rule
    assert np.any(ref["planes"]["SS"] == 0) and np.any(np.isnan(kin))              # a zero denominator
    called = (i["geno"] < 3) & ref["used"][:, None]
    assert np.any(called & ~ref["ops"]["valid"])                                   # a frequency outside [maf_thresh, 1 - maf_thresh]
    assert not ref["used"].all()                                                   # a SNP without a called training sample
    assert len(i["pairs"]["po"]) and len(i["pairs"]["dup"]) == 1


# ---- 5. partition ----------------------------------------------------------------------------------------------------------------------

def _fed_in(case, cuts, names=R.PLANES, ibd=True):
    i = inputs(case)
    with _object(case, ibd) as p:
        for a, b in zip(cuts[:-1], cuts[1:]):
            p.feed(i["packed"][a:b], fmt=_lib.GENO_PACKED2)
        return _planes(p, names), p.stats()


@pytest.mark.parametrize("case", [(65, 500, 2, 0.3, "fifth"), (130, 1030, 2, 0.03, "fifth")])
def test_partition_of_the_feeds(case):
    m = case[1]
    r = run(case)
    tol = {k: R.plane_bound(r["ref"]["mag"][k], m, case[2]) for k in R.PLANES}
    two, _ = _fed_in(case, [0, m // 3 + 1, m])
    seven, st = _fed_in(case, [0, 1, 18, 19, 150, 151 + m // 4, m - 5, m])
    assert st["blocks"] == 7
    again, _ = _fed_in(case, [0, m // 3 + 1, m])
    for k in R.PLANES:
        for other in (two[k], seven[k]):
            assert float(np.abs(other.astype(LD) - r["planes"][k]).max()) <= tol[k], k
        assert np.array_equal(again[k], two[k]), k                             # the same calls: the same bits
    for k in ("IBS0", "NS"):
        assert np.array_equal(two[k], r["planes"][k]) and np.array_equal(seven[k], r["planes"][k])


# ---- 6. the second trip of the internal block loop -------------------------------------------------------------------------------------

def test_small_stage_takes_several_internal_blocks(monkeypatch):
    case = (130, 500, 5, 0.3, "all")
    r = run(case)
    assert r["stats"]["blocks"] == 1 and r["stats"]["product_launches"] == 3
    monkeypatch.setenv("SNPGPU_PCR_STAGE_BYTES", str(9 * 256 * 8 * 48))       # 48 SNPs of nine planes at n_pad = 256
    planes, st = _fed_in(case, [0, 500])
    assert st["block_snps"] == 48 and st["blocks"] == 11 and st["product_launches"] == 33
    assert st["plane_bytes"] == 8 * 8 * 130 * 130
    for k in R.PLANES:
        tol = R.plane_bound(r["ref"]["mag"][k], 500, 5)
        assert float(np.abs(planes[k].astype(LD) - r["ref"]["planes"][k]).max()) <= tol, k
    for k in ("IBS0", "NS"):
        assert np.array_equal(planes[k], r["planes"][k])


def test_forced_block_size_takes_several_internal_blocks(monkeypatch):
    """SNPGPU_PCR_BLOCK_SNPS=48 cuts the same feed at the same SNPs inside a staging window of the default size (RowBlocks::open):
    eleven blocks and their launches as above, the planes at the same bounds, the counters bit for bit"""
    case = (130, 500, 5, 0.3, "all")
    r = run(case)
    monkeypatch.setenv("SNPGPU_PCR_BLOCK_SNPS", "48")
    planes, st = _fed_in(case, [0, 500])
    assert st["block_snps"] > 500                                  # the window itself would hold the feed in one block
    assert st["blocks"] == 11 and st["product_launches"] == 33
    assert st["plane_bytes"] == 8 * 8 * 130 * 130
    for k in R.PLANES:
        tol = R.plane_bound(r["ref"]["mag"][k], 500, 5)
        assert float(np.abs(planes[k].astype(LD) - r["ref"]["planes"][k]).max()) <= tol, k
    for k in ("IBS0", "NS"):
        assert np.array_equal(planes[k], r["planes"][k])


# ---- 7. formats and memory -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(65, 1030, 1, 0.03, "all"), (257, 500, 5, 0.03, "fifth")])
def test_u8_host_rows_against_packed_device_rows(case):
    import torch
    i = inputs(case)
    r = run(case)
    with _object(case) as p:
        b = p.feed(np.ascontiguousarray(i["geno"]), fmt=_lib.GENO_U8, want_beta=True)
        host = _planes(p)
    dev_rows = torch.from_numpy(i["packed"].copy()).cuda()
    with _object(case) as p:
        b2 = p.feed(int(dev_rows.data_ptr()), fmt=_lib.GENO_PACKED2, n_snp=case[1], want_beta=True)
        dev = _planes(p)
    assert np.array_equal(b, b2) and np.array_equal(b, r["beta"])
    for k in R.PLANES:
        assert np.array_equal(host[k], dev[k]) and np.array_equal(host[k], r["planes"][k]), k


# ---- 8. flags --------------------------------------------------------------------------------------------------------------------------

def test_without_the_ibd_flag():
    case = (130, 1030, 2, 0.03, "fifth")
    r = run(case)
    i = inputs(case)
    with _object(case, ibd=False) as p:
        p.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        for k in ("RR", "SS", "NS"):
            assert np.array_equal(p.sums(k), r["planes"][k]), k
        for k in ("DD", "DC", "CC", "IBS0", "K0D"):
            with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_sums: this plane needs a handle created with SNPGPU_PCR_IBD"):
                p.sums(k)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_result: k0 and k2 need a handle created with SNPGPU_PCR_IBD"):
            p.result(probs=True)
        res = p.result()
        assert set(res) == {"kinship", "inbreed", "nsnp"}
        for k in res:
            assert np.array_equal(res[k], r["res"][k], equal_nan=True), k
        st = p.stats()
        assert st["product_launches"] == st["blocks"] == 1 and st["plane_bytes"] == 3 * 8 * 130 * 130
        with pytest.raises(_lib.SnpGpuError, match="invalid plane"):
            p.sums(8)


# ---- 9. Python -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hapmap_runs():
    from snprelate_amd.gds import open_gds
    from conftest import GOLDEN
    import os
    f = open_gds(os.path.join(GOLDEN, "hapmap_geno.gds"))
    pca = api.snpgdsPCA(f, eigen_cnt=4, verbose=False)
    res = api.snpgdsPCRelate(f, pca, verbose=False)
    g = api.snpgdsGetGeno(f, snp_id=res["snp_id"], snpfirstdim=True, verbose=False)
    n = g.shape[1]
    pcs = np.ascontiguousarray(pca["eigenvect"][:, :4])
    # the object path, fed in the working space's blocks
    with _lib.PCRelate(n, pcs=pcs) as p:
        packed = pack_2bit_rows(g)
        b = np.concatenate([p.feed(packed[s:s + 8192], fmt=_lib.GENO_PACKED2, want_beta=True) for s in range(0, len(packed), 8192)])
        obj = p.result()
    return dict(file=f, pca=pca, res=res, geno=g, pcs=pcs, beta=b, obj=obj)


def test_snpgdspcrelate_on_hapmap():
    h = hapmap_runs()
    res, g = h["res"], h["geno"]
    m, n = g.shape
    assert list(res) == ["sample_id", "snp_id", "kinship", "k0", "k1", "k2", "nsnp", "inbreed"]
    assert np.array_equal(res["sample_id"], h["pca"]["sample_id"]) and n == 279 and m > 8000
    # snpgpu_gnrPCRelate equals the object path bit for bit
    for k in ("kinship", "k0", "k2", "nsnp", "inbreed"):
        assert np.array_equal(res[k], h["obj"][k], equal_nan=True), k
    assert np.array_equal(res["k1"], 1.0 - res["k0"] - res["k2"], equal_nan=True)
    # the float64 restatement from the device's beta: the device and the restatement are each within the plane bound of the exact
    # sums, so within twice the bound of each other
    ref = R.pcrelate(g, h["pcs"], None, 0.01, b=h["beta"])
    err = np.abs(h["beta"] - ref["beta"])
    assert np.all(err <= 2 * ref["beta_bound"])
    mu = ref["ops"]["mu"]
    called = (g < 3) & ref["used"][:, None]
    assert np.abs(mu[called] - 0.01).min() > 1e-9 and np.abs(mu[called] - 0.99).min() > 1e-9
    tol = {k: 2 * R.plane_bound(ref["mag"][k], m, 4) for k in R.PLANES}
    P = {k: v.astype(LD) for k, v in ref["planes"].items()}
    bound, want = _propagated(P, tol)
    for k in ("kinship", "inbreed", "k0", "k2"):
        _assert_within(res[k], want[k], bound[k], k)
    assert np.array_equal(res["nsnp"], ref["planes"]["NS"])
    # snpgdsIBDSelection: exactly the pairs the reference's kinship puts at or above 0.1 (none of them within the bound of it)
    kin = want["kinship"].astype(np.float64)
    assert np.all(np.abs(kin - 0.1) > bound["kinship"])
    tab = api.snpgdsIBDSelection(res, 0.1)
    assert list(tab) == ["ID1", "ID2", "kinship", "k0", "k1", "k2", "nsnp"]
    ids = res["sample_id"]
    r_, c_ = np.nonzero(np.tril(kin >= 0.1, -1))
    want_pairs = sorted(zip(ids[c_].tolist(), ids[r_].tolist()))
    assert sorted(zip(tab["ID1"].tolist(), tab["ID2"].tolist())) == want_pairs and len(want_pairs) > 20


def test_snpgdspcrelate_with_an_array_and_training_ids():
    h = hapmap_runs()
    f, g = h["file"], h["geno"]
    n = g.shape[1]
    ids = h["res"]["sample_id"]
    T = np.arange(n) % 3 != 1
    res = api.snpgdsPCRelate(f, h["pcs"], n_pcs=2, training_id=ids[T], maf_thresh=0.05, ibd_probs=False, verbose=False)
    assert res["k0"] is None and res["k1"] is None and res["k2"] is None
    with _lib.PCRelate(n, pcs=h["pcs"][:, :2], training=T, maf_thresh=0.05, ibd=False) as p:
        packed = pack_2bit_rows(g)
        for s in range(0, len(packed), 8192):
            p.feed(packed[s:s + 8192], fmt=_lib.GENO_PACKED2)
        obj = p.result()
    for k in ("kinship", "nsnp", "inbreed"):
        assert np.array_equal(res[k], obj[k], equal_nan=True), k
    assert not np.array_equal(res["kinship"], h["res"]["kinship"], equal_nan=True)
    # a result object whose samples come in another order is matched by sample_id
    perm = np.random.default_rng(0).permutation(n)
    shuffled = dict(sample_id=np.asarray(h["pca"]["sample_id"])[perm], eigenvect=h["pca"]["eigenvect"][perm])
    again = api.snpgdsPCRelate(f, shuffled, n_pcs=4, verbose=False)
    assert np.array_equal(again["kinship"], h["res"]["kinship"], equal_nan=True)
    with pytest.raises(ValueError, match="training.id"):
        api.snpgdsPCRelate(f, h["pcs"], training_id=["nobody"], verbose=False)
    with pytest.raises(ValueError, match="one row per selected sample"):
        api.snpgdsPCRelate(f, h["pcs"][:-1], verbose=False)
