"""PC-Relate row panels on the GPU (snpgpu_pcr_create_panel, _panel_result, _panel_sums, snpgpu_pcr_select, snpgpu_gnrPCRelatePairs,
snpgdsPCRelatePairs) against the full object on the same feeds.

The one rule under test: every sum, result and selected value of a panel equals, bit for bit, what a full object holds at the same
(i, j).  So every comparison is equality of float64 bit patterns (NaN included) against _lib.PCRelate, whose own agreement with the
definitions test_gpu_pcrelate.py establishes; the selection is compared with its numpy restatement (pcrelate_panels_ref.select) on
the full object's result().  The full object of a shape is run once and shared.  The one tolerance, rtol = atol = 1e-12 of k0 / k2
against R.finalise on the panel's own sums, is the figure test_gpu_pcrelate.test_results uses for that comparison."""
import ctypes
import functools

import numpy as np
import pytest

import pcrelate_panels_ref as P
import pcrelate_ref as R
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows

pytestmark = pytest.mark.gpu

RESULTS = ("kinship", "k0", "k2", "nsnp")


@functools.lru_cache(maxsize=None)
def packed(n, m):
    return pack_2bit_rows(P.inputs(n, m)["geno"])


def _kw(n, m):
    i = P.inputs(n, m)
    return dict(pcs=i["pcs"], training=i["T"], maf_thresh=0.01)


@functools.lru_cache(maxsize=None)
def full(n, m, ibd=True):
    """the full object fed the whole set at once: its planes, results, statistics and the selection through its own handle"""
    with _lib.PCRelate(n, ibd=ibd, **_kw(n, m)) as p:
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        sums = {k: p.sums(k) for k in (R.PLANES if ibd else ("RR", "SS", "NS"))}
        out = dict(sums=sums, res=p.result(), stats=p.stats())
    for a in list(out["sums"].values()) + list(out["res"].values()):
        a.setflags(write=False)
    return out


def _panel(n, m, rows, ibd=True):
    return _lib.PCRelatePanel(n, rows=rows, ibd=ibd, **_kw(n, m))


def _assert_panel_equals(p, f_sums, f_res, rows, names=R.PLANES, results=RESULTS):
    r0, r1 = rows
    for k in names:
        assert P.same_bits(p.sums(k), P.panel_cut(f_sums[k], r0, r1)), k
    if "DC" in names:
        assert P.same_bits(p.sums("CD"), P.panel_cut(f_sums["DC"].T, r0, r1)), "CD"
    res = p.result()
    assert set(res) == set(results) | {"inbreed"}
    for k in results:
        assert P.same_bits(res[k], P.panel_cut(f_res[k], r0, r1)), k
    assert P.same_bits(res["inbreed"], f_res["inbreed"])                   # every sample's, whatever the panel


# ---- 1. panels against the full object -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,rows", P.PANEL_CASES, ids=["n%d-%d-%d" % (n, r[0], r[1]) for n, r in P.PANEL_CASES])
def test_panel_equals_the_full_object(n, rows):
    m = 500
    f = full(n, m)
    with _panel(n, m, rows) as p:
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        assert p.shape == (rows[1] - rows[0], n - rows[0])
        _assert_panel_equals(p, f["sums"], f["res"], rows)
        st = p.stats()
        n_pad = (n + 127) // 128 * 128
        assert st["plane_bytes"] == 9 * 8 * p.shape[0] * p.shape[1] + 2 * 8 * n_pad * 128
        assert st["blocks"] == f["stats"]["blocks"] == 1 and st["block_snps"] == f["stats"]["block_snps"]
        # the full object's three, the strips, and the CD job where there are columns right of the panel's diagonal block
        cd = rows[1] < n
        assert st["product_launches"] == (5 if cd else 4)
        ps = p.panel_stats()
        assert 0 < ps["strip_ms"] < st["product_ms"] and (0 < ps["cd_ms"] < st["product_ms"] if cd else ps["cd_ms"] == 0)
        for name, got in (("panel_result", p.panel_result()["k2"]), ("panel_sums", p.panel_sums("CD"))):
            assert got.shape == p.shape, name                               # the panel's shape on the panel class too
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_result: this handle is a row panel.*snpgpu_pcr_panel_result"):
            _lib.PCRelate.result(p)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_sums: this handle is a row panel.*snpgpu_pcr_panel_sums"):
            _lib.PCRelate.sums(p, "RR")
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_panel_sums: invalid plane: 0 ... 8"):
            p.sums(9)


def test_a_full_handle_is_the_panel_of_all_rows():
    n, m = 257, 500
    f = full(n, m)
    with _lib.PCRelate(n, **_kw(n, m)) as p:
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        for k in R.PLANES:
            assert P.same_bits(p.panel_sums(k), f["sums"][k]), k
        assert P.same_bits(p.panel_sums("CD"), f["sums"]["DC"].T)
        res = p.panel_result()
        for k in RESULTS + ("inbreed",):
            assert P.same_bits(res[k], f["res"][k]), k
        assert p.stats()["plane_bytes"] == 8 * 8 * n * n and p.stats()["product_launches"] == 3
        assert p.panel_stats() == dict(cd_ms=0.0, strip_ms=0.0)


def test_k0_and_k2_of_a_panel_against_the_restated_finaliser():
    """the existing yardstick of test_results, on the panel's own sums: R.finalise in float64, rtol = atol = 1e-12"""
    n, m, rows = 300, 500, (128, 300)
    f = full(n, m)
    mine = R.finalise(f["sums"])                                            # (the panel's sums are these bits: the test above)
    with _panel(n, m, rows) as p:
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        res = p.result()
    for k in ("kinship", "k0", "k2"):
        np.testing.assert_allclose(res[k], P.panel_cut(mine[k], *rows), rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=k)
    np.testing.assert_allclose(res["inbreed"], mine["inbreed"], rtol=1e-12, atol=1e-12, equal_nan=True)


# ---- 2. several internal blocks, several feeds, results between them ----------------------------------------------------------------

def test_several_internal_blocks_and_feeds(monkeypatch):
    n, m = 257, 1030
    monkeypatch.setenv("SNPGPU_PCR_BLOCK_SNPS", "48")
    rows = packed(n, m)
    cut = 400                                                              # 9 + 14 internal blocks
    panels = [_panel(n, m, r) for r in P.partition(n, 128)]
    try:
        with _lib.PCRelate(n, **_kw(n, m)) as whole:
            for a, b in ((0, cut), (cut, m)):
                whole.feed(rows[a:b], fmt=_lib.GENO_PACKED2)
                sums = {k: whole.sums(k) for k in R.PLANES}
                res = whole.result()
                for p in panels:
                    p.feed(rows[a:b], fmt=_lib.GENO_PACKED2)
                    _assert_panel_equals(p, sums, res, p.rows)             # also between the feeds
            st = whole.stats()
            assert st["blocks"] == 23 and st["blocks"] > 2
            for p in panels:
                ps = p.stats()
                assert ps["blocks"] == st["blocks"] and ps["block_snps"] == st["block_snps"] and ps["product_launches"] == (5 if p.rows[1] < n else 4) * 23
    finally:
        for p in panels:
            p.close()


# ---- 3. without the IBD slabs ---------------------------------------------------------------------------------------------------------

def test_without_the_ibd_flag():
    n, m, rows = 257, 500, (128, 257)
    f = full(n, m, ibd=False)
    assert P.same_bits(f["res"]["kinship"], full(n, m)["res"]["kinship"])
    with _panel(n, m, rows, ibd=False) as p:
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        _assert_panel_equals(p, f["sums"], f["res"], rows, names=("RR", "SS", "NS"), results=("kinship", "nsnp"))
        for k in ("DD", "DC", "CC", "IBS0", "K0D", "CD"):
            with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_panel_sums: this plane needs a handle created with SNPGPU_PCR_IBD"):
                p.sums(k)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_panel_result: k0 and k2 need a handle created with SNPGPU_PCR_IBD"):
            p.result(probs=True)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_select: k0 and k2 need a handle created with SNPGPU_PCR_IBD"):
            p.select(P.CUTOFF, probs=True)
        assert p.stats()["plane_bytes"] == 3 * 8 * 129 * 129 + 2 * 8 * 384 * 128 and p.stats()["product_launches"] == 2
        got = p.select(P.CUTOFF)
        want = P.select(f["res"], P.CUTOFF, rows=rows)
        assert set(got) == {"idx1", "idx2", "kinship", "nsnp", "inbreed", "n_found"} and got["n_found"] == len(want["idx1"]) > 0
        for k in ("idx1", "idx2"):
            assert np.array_equal(got[k], want[k]), k
        for k in ("kinship", "nsnp"):
            assert P.same_bits(got[k], want[k]), k


# ---- 4. input forms --------------------------------------------------------------------------------------------------------------------

def test_u8_host_rows_against_packed_device_rows():
    import torch
    n, m, rows = 257, 500, (128, 256)
    f = full(n, m)
    with _panel(n, m, rows) as p:
        b = p.feed(np.ascontiguousarray(P.inputs(n, m)["geno"]), fmt=_lib.GENO_U8, want_beta=True)
        _assert_panel_equals(p, f["sums"], f["res"], rows)
    dev_rows = torch.from_numpy(packed(n, m).copy()).cuda()
    with _panel(n, m, rows) as p:
        b2 = p.feed(int(dev_rows.data_ptr()), fmt=_lib.GENO_PACKED2, n_snp=m, want_beta=True)
        _assert_panel_equals(p, f["sums"], f["res"], rows)
    assert P.same_bits(b, b2)


# ---- 5. selection ----------------------------------------------------------------------------------------------------------------------

def _select_union(n, m, rows_per_panel, cutoff, samp_sel=None):
    """the selections of the panels of a partition, concatenated in ascending row order, and the counts of the panels"""
    parts, counts = [], []
    for r in P.partition(n, rows_per_panel):
        with _panel(n, m, r) as p:
            p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
            s = p.select(cutoff, samp_sel=samp_sel)
            assert s["n_found"] == len(s["idx1"])
            parts.append(s)
            counts.append(s["n_found"])
    out = {k: np.concatenate([s[k] for s in parts]) for k in ("idx1", "idx2") + RESULTS}
    out["inbreed"] = parts[0]["inbreed"]
    for s in parts:
        assert P.same_bits(s["inbreed"], out["inbreed"])
    return out, counts


def _assert_selection(got, want):
    assert len(got["idx1"]) == len(want["idx1"])
    for k in ("idx1", "idx2"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in RESULTS:
        assert P.same_bits(got[k], want[k]), k


@pytest.mark.parametrize("n", [257, 300])
@pytest.mark.parametrize("cutoff", [P.CUTOFF, float("nan"), 10.0], ids=["0.1", "nan", "above"])
def test_selection_of_every_partition(n, cutoff):
    m = 500
    f = full(n, m)
    want = P.select(f["res"], cutoff)
    assert len(want["idx1"]) == (n * (n - 1) // 2 if np.isnan(cutoff) else 0 if cutoff > 1 else {257: 320, 300: 373}[n])
    for rows_per_panel in (128, 256, n):
        got, counts = _select_union(n, m, rows_per_panel, cutoff)
        _assert_selection(got, want)
        assert P.same_bits(got["inbreed"], f["res"]["inbreed"])
        if rows_per_panel == 128 and cutoff == P.CUTOFF:
            assert counts == {257: [163, 157, 0], 300: [163, 160, 50]}[n]      # the panel [256, 257) finds nothing
    with _lib.PCRelate(n, **_kw(n, m)) as p:                               # the full handle: the panel [0, n)
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        s = p.select(cutoff)
        _assert_selection(s, want)
        assert s["n_found"] == len(want["idx1"]) and P.same_bits(s["inbreed"], f["res"]["inbreed"])
        st = _lib.pcr_select_stats()
        assert st["total_ms"] > 0 and st["count_ms"] >= 0 and st["scan_ms"] >= 0 and (s["n_found"] > 0 or st["write_ms"] == 0)


def test_selection_with_dropped_samples():
    """samples dropped at the edge of a 64-column chunk of the walk and at the edge of a panel"""
    n, m = 257, 500
    f = full(n, m)
    sel = np.ones(n, bool)
    sel[[0, 63, 64, 127, 128, 200, 256]] = False
    want = P.select(f["res"], P.CUTOFF, samp_sel=sel)
    assert 0 < len(want["idx1"]) < 320
    dropped = P.select(f["res"], P.CUTOFF)
    lost = ~(sel[dropped["idx1"]] & sel[dropped["idx2"]])
    assert lost.any()                                                      # the mask takes pairs away that the cutoff selects
    for rows_per_panel in (128, n):
        got, _ = _select_union(n, m, rows_per_panel, P.CUTOFF, samp_sel=sel)
        _assert_selection(got, want)
    got, _ = _select_union(n, m, 128, float("nan"), samp_sel=sel)
    _assert_selection(got, P.select(f["res"], float("nan"), samp_sel=sel))
    assert len(got["idx1"]) == 250 * 249 // 2


def test_selection_capacity_keeps_the_prefix():
    n, m, rows = 257, 500, (0, 128)
    f = full(n, m)
    want = P.select(f["res"], P.CUTOFF, rows=rows)
    total = len(want["idx1"])
    assert total == 163
    L = _lib.lib()
    o = _lib.PcrSelOpts(P.CUTOFF, None)
    with _panel(n, m, rows) as p:
        p.feed(packed(n, m), fmt=_lib.GENO_PACKED2)
        for cap in (1, 64, 100, total, total + 40):
            i1, i2 = np.full(total + 40, -77, np.int32), np.full(total + 40, -77, np.int32)
            v = {k: np.full(total + 40, -77.5) for k in RESULTS}
            inb = np.full(n, -77.5)
            found = ctypes.c_int64(-1)
            _lib.check(L.snpgpu_pcr_select(p._h, ctypes.byref(o), cap, _lib._ptr(i1), _lib._ptr(i2), _lib._ptr(v["kinship"]), _lib._ptr(v["k0"]),
                                           _lib._ptr(v["k2"]), _lib._ptr(v["nsnp"]), _lib._ptr(inb), ctypes.byref(found)))
            k = min(cap, total)
            assert found.value == total                                     # all selected pairs, whatever is stored
            assert np.array_equal(i1[:k], want["idx1"][:k]) and np.array_equal(i2[:k], want["idx2"][:k])
            assert np.all(i1[k:] == -77) and np.all(i2[k:] == -77)          # nothing is written behind the stored pairs
            for name in RESULTS:
                assert P.same_bits(v[name][:k], want[name][:k]) and np.all(v[name][k:] == -77.5), name
            assert P.same_bits(inb, f["res"]["inbreed"])
        # count only
        s = p.select(P.CUTOFF, capacity=0)
        assert s["n_found"] == total and len(s["idx1"]) == 0 and P.same_bits(s["inbreed"], f["res"]["inbreed"])
        s = p.select(P.CUTOFF, capacity=10)
        assert s["n_found"] == total and np.array_equal(s["idx2"], want["idx2"][:10])
        # some outputs only
        found = ctypes.c_int64(-1)
        i2 = np.full(total, -77, np.int32)
        _lib.check(L.snpgpu_pcr_select(p._h, ctypes.byref(o), total, None, _lib._ptr(i2), None, None, None, None, None, ctypes.byref(found)))
        assert found.value == total and np.array_equal(i2, want["idx2"])


# ---- 6. the working space and the API -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hapmap():
    import os
    from conftest import GOLDEN
    from snprelate_amd.gds import open_gds
    f = open_gds(os.path.join(GOLDEN, "hapmap_geno.gds"))
    pca = api.snpgdsPCA(f, eigen_cnt=4, verbose=False)
    return dict(file=f, pca=pca, res=api.snpgdsPCRelate(f, pca, verbose=False))


def _assert_table(got, tab, res, n_panels=None):
    assert list(got) == ["sample_id", "snp_id", "ID1", "ID2", "idx1", "idx2", "kinship", "k0", "k1", "k2", "nsnp", "inbreed", "n_panels"]
    assert np.array_equal(got["sample_id"], res["sample_id"]) and np.array_equal(got["snp_id"], res["snp_id"])
    assert len(tab["ID1"]) == len(got["ID1"])
    for k in ("ID1", "ID2"):
        assert np.array_equal(got[k], tab[k]), k
    assert np.array_equal(got["sample_id"][got["idx1"]], got["ID1"]) and np.array_equal(got["sample_id"][got["idx2"]], got["ID2"])
    for k in ("kinship", "k0", "k1", "k2", "nsnp"):
        assert P.same_bits(got[k], tab[k]), k
    assert P.same_bits(got["inbreed"], res["inbreed"])
    if n_panels is not None:
        assert got["n_panels"] == n_panels


def test_snpgdspcrelatepairs_on_hapmap():
    h = hapmap()
    f, pca, res = h["file"], h["pca"], h["res"]
    assert len(res["sample_id"]) == 279
    tab = api.snpgdsIBDSelection(res, P.CUTOFF)
    assert list(tab) == ["ID1", "ID2", "kinship", "k0", "k1", "k2", "nsnp"] and len(tab["ID1"]) > 20
    got = api.snpgdsPCRelatePairs(f, pca, kinship_cutoff=P.CUTOFF, panel_rows=128, verbose=False)
    _assert_table(got, tab, res, n_panels=3)
    _assert_table(api.snpgdsPCRelatePairs(f, pca, kinship_cutoff=P.CUTOFF, panel_rows=None, verbose=False), tab, res, n_panels=1)
    _assert_table(api.snpgdsPCRelatePairs(f, pca, kinship_cutoff=P.CUTOFF, panel_rows=256, verbose=False), tab, res, n_panels=2)
    # the default cutoff, a sample selection, the kinship slabs alone
    sel = np.arange(279) % 7 != 3
    tab = api.snpgdsIBDSelection(res, 2 ** -5.5, samp_sel=sel)
    got = api.snpgdsPCRelatePairs(f, pca, samp_sel=sel, panel_rows=128, verbose=False)
    _assert_table(got, tab, res, n_panels=3)
    got = api.snpgdsPCRelatePairs(f, pca, kinship_cutoff=P.CUTOFF, ibd_probs=False, panel_rows=128, verbose=False)
    assert got["k0"] is None and got["k1"] is None and got["k2"] is None
    tab = api.snpgdsIBDSelection(res, P.CUTOFF)
    assert np.array_equal(got["ID1"], tab["ID1"]) and np.array_equal(got["ID2"], tab["ID2"])
    assert P.same_bits(got["kinship"], tab["kinship"]) and P.same_bits(got["nsnp"], tab["nsnp"])
    with pytest.raises(ValueError, match="strictly increasing"):
        api.snpgdsPCRelatePairs(f, pca, samp_sel=np.array([3, 1]), verbose=False)


def test_working_space_call_refusals_and_kept_result():
    h = hapmap()
    api.snpgdsPCRelatePairs(h["file"], h["pca"], kinship_cutoff=P.CUTOFF, panel_rows=128, verbose=False)     # sets the working space
    L = _lib.lib()
    found, n_p = ctypes.c_int64(0), ctypes.c_int64(0)
    for bad in (1, 64, 127, 129, 200):
        assert L.snpgpu_gnrPCRelatePairs(0, None, None, 0.01, 1, bad, 0.1, None, 0, ctypes.byref(found), ctypes.byref(n_p)) != 0
        assert L.snpgpu_last_error().decode().startswith("snpgpu_gnrPCRelatePairs: panel_rows must be")
    r = _lib.gnr_pcrelate_pairs(279, panel_rows=279, kinship_cutoff=10.0)   # one panel, no pair: inbreed still comes
    assert r["n_panels"] == 1 and len(r["idx1"]) == 0 and np.isfinite(r["inbreed"]).any()
    r = _lib.gnr_pcrelate_pairs(279, panel_rows=128, kinship_cutoff=P.CUTOFF)
    assert r["n_panels"] == 3 and len(r["idx1"]) > 0
    _lib.check(L.snpgpu_ws_clear())                                          # the kept pairs go with the working space
    i1 = np.full(len(r["idx1"]), -77, np.int32)
    assert L.snpgpu_gnrPCRelatePairs_get(_lib._ptr(i1), None, None, None, None, None, None) == 0 and np.all(i1 == -77)
