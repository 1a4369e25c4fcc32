"""PC-Relate row panels without a GPU: the header and the binding, the refusals that come before the first HIP call, and the
conditions on the test inputs that the GPU tests (test_gpu_pcrelate_panels.py) rely on, on the float64 restatement."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import mem_kinds as M
import pcrelate_panels_ref as P
import pcrelate_ref as R
from conftest import ROOT
from snprelate_amd import _lib, api

HEADER = os.path.join(ROOT, "include", "snpgpu.h")
NAMES = ("snpgpu_pcr_create_panel", "snpgpu_pcr_panel_result", "snpgpu_pcr_panel_sums", "snpgpu_pcr_panel_stats", "snpgpu_pcr_select", "snpgpu_pcr_select_stats",
         "snpgpu_gnrPCRelatePairs", "snpgpu_gnrPCRelatePairs_get")


# ---- the header and the binding ----------------------------------------------------------------------------------------------------

def test_header_declares_the_panel_functions():
    text = open(HEADER).read()
    protos = M.header_prototypes(text)
    L = _lib.lib()
    for f in NAMES:
        assert f in protos and f in _lib.EXPORTS and hasattr(L, f), f
    assert protos["snpgpu_pcr_create_panel"] == ["n_samp", "n_pc", "pcs", "training", "maf_thresh", "flags", "row_begin", "row_end", "opts", "out"]
    assert protos["snpgpu_pcr_panel_result"] == ["pcr", "kinship", "inbreed", "k0", "k2", "nsnp"]
    assert protos["snpgpu_pcr_panel_sums"] == ["pcr", "which", "plane"]
    assert protos["snpgpu_pcr_panel_stats"] == ["pcr", "ms2"]
    assert protos["snpgpu_pcr_select"] == ["pcr", "o", "capacity", "idx1", "idx2", "kinship", "k0", "k2", "nsnp", "inbreed", "n_found"]
    assert protos["snpgpu_pcr_select_stats"] == ["ms4"]
    assert protos["snpgpu_gnrPCRelatePairs"] == ["n_pc", "pcs", "training", "maf_thresh", "flags", "panel_rows", "kinship_cutoff", "samp_sel",
                                                 "verbose", "n_found", "n_panels"]
    assert protos["snpgpu_gnrPCRelatePairs_get"] == ["idx1", "idx2", "kinship", "k0", "k2", "nsnp", "inbreed"]
    for f in NAMES:
        assert "out_mem" not in protos[f] and "dst_mem" not in protos[f] and protos[f][0] not in ("ctx", "m")
    assert "typedef struct snpgpu_pcr_sel_opts { double kinship_cutoff; const uint8_t *samp_sel; } snpgpu_pcr_sel_opts;" in text
    assert "#define SNPGPU_ABI_VERSION 2\n" in text                      # additions only: the version stays
    assert text.index("snpgpu_pcr_create_panel") > text.index("int snpgpu_gnrPCRelate(")       # appended after the section's declarations
    assert _lib.PCR_SLABS == P.SLABS and _lib.PCR_TILE == P.TILE
    assert [f[0] for f in _lib.PcrSelOpts._fields_] == ["kinship_cutoff", "samp_sel"]
    # what the section no longer lists as not built, and what it still does
    not_built = text[text.index("Not built: the small-sample correction"):text.index("Every sum has one owner")]
    assert "row panels" not in not_built and "sparse selection" not in not_built
    for still in ("multi-device objects", "results in device memory", "anything below fp64"):
        assert still in " ".join(not_built.replace(" * ", " ").split()), still


def test_python_interface():
    import snprelate_amd
    assert snprelate_amd.snpgdsPCRelatePairs is api.snpgdsPCRelatePairs
    sig = inspect.signature(api.snpgdsPCRelatePairs)
    assert list(sig.parameters) == ["gdsobj", "pcs", "n_pcs", "sample_id", "snp_id", "autosome_only", "remove_monosnp", "maf", "missing_rate",
                                    "training_id", "maf_thresh", "ibd_probs", "kinship_cutoff", "samp_sel", "panel_rows", "verbose", "device"]
    p = sig.parameters
    assert p["kinship_cutoff"].default == 2 ** -5.5 and p["samp_sel"].default is None and p["panel_rows"].default is None
    assert p["n_pcs"].default is None and p["maf_thresh"].default == 0.01 and p["ibd_probs"].default is True
    assert np.isnan(p["maf"].default) and np.isnan(p["missing_rate"].default) and p["autosome_only"].default is True
    assert list(inspect.signature(_lib.PCRelatePanel.__init__).parameters)[:3] == ["self", "n_samp", "rows"]
    for cls in (_lib.PCRelate, _lib.PCRelatePanel):
        for name in ("feed", "result", "sums", "select", "stats"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(_lib.gnr_pcrelate_pairs)


def test_both_calls_match_pcs_through_one_helper(monkeypatch):
    """snpgdsPCRelate and snpgdsPCRelatePairs hand pcs, n_pcs and training_id to the same helper, right after the working space"""
    class Reached(Exception):
        pass

    def helper(ws, pcs, n_pcs, training_id, verbose):
        assert ws == "the working space"
        raise Reached((pcs, n_pcs, training_id))

    monkeypatch.setattr(api, "_init_file2", lambda *a, **k: "the working space")
    monkeypatch.setattr(api, "_pcr_match", helper)
    for f in (api.snpgdsPCRelate, api.snpgdsPCRelatePairs):
        with pytest.raises(Reached) as e:
            f("a file", "the pcs", n_pcs=3, training_id="the ids", verbose=False)
        assert e.value.args[0] == ("the pcs", 3, "the ids")


# ---- refusals that precede the first HIP call ------------------------------------------------------------------------------------------

def _refused(rc, fn, text):
    assert rc != 0
    msg = _lib.lib().snpgpu_last_error().decode()
    assert msg.startswith(fn + ": ") and text in msg, msg


def _create_panel(n, r0, r1, pcs=None, maf=0.01, flags=1, out=True):
    h = ctypes.c_void_p()
    pcs = None if pcs is None else np.ascontiguousarray(pcs, np.float64)
    rc = _lib.lib().snpgpu_pcr_create_panel(n, 0 if pcs is None else pcs.shape[1], _lib._ptr(pcs), None, maf, flags, r0, r1, None,
                                            ctypes.byref(h) if out else None)
    assert not h.value
    return rc


def test_create_panel_refusals():
    fn = "snpgpu_pcr_create_panel"
    # check_create's, under the new name
    _refused(_create_panel(300, 0, 128, out=False), fn, "out is NULL")
    _refused(_create_panel(0, 0, 128), fn, "invalid number of samples")
    _refused(_create_panel(300, 0, 128, maf=0.5), fn, "maf_thresh must be inside (0, 0.5)")
    _refused(_create_panel(300, 0, 128, flags=2), fn, "unknown flags")
    _refused(_create_panel(1, 0, 1), fn, "too few training samples: 1")
    _refused(_create_panel(16, 0, 16, pcs=np.ones((16, 1))), fn, "collinear")
    # its own
    for r0 in (-128, -1, 1, 64, 127, 129):
        _refused(_create_panel(300, r0, 300), fn, "row_begin must be a non-negative multiple of 128")
    for r0, r1 in ((128, 128), (128, 0), (256, 128), (0, 0), (0, -5)):
        _refused(_create_panel(300, r0, r1), fn, "row_end <= row_begin")
    for r1 in (301, 384, 10 ** 9):
        _refused(_create_panel(300, 0, r1), fn, "row_end is beyond the samples")
    for r0, r1 in ((0, 1), (0, 127), (0, 129), (128, 299), (256, 257)):
        _refused(_create_panel(300, r0, r1), fn, "row_end must be a multiple of 128 or the number of samples")
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_pcr_create_panel: row_begin"):
        _lib.PCRelatePanel(300, rows=(5, 300))
    with pytest.raises(ValueError, match="one row per sample"):
        _lib.PCRelatePanel(300, rows=(0, 128), pcs=np.zeros((299, 2)))


def test_other_refusals():
    L = _lib.lib()
    buf = np.zeros(16, np.float64)
    idx = np.zeros(16, np.int32)
    found = ctypes.c_int64(-7)
    o = _lib.PcrSelOpts(0.1, None)
    fake = ctypes.c_void_p(8)                                              # never dereferenced: every refusal below precedes that
    _refused(L.snpgpu_pcr_panel_result(None, _lib._ptr(buf), None, None, None, None), "snpgpu_pcr_panel_result", "pcr is NULL")
    _refused(L.snpgpu_pcr_panel_sums(None, 0, _lib._ptr(buf)), "snpgpu_pcr_panel_sums", "NULL argument")
    _refused(L.snpgpu_pcr_panel_sums(fake, 0, None), "snpgpu_pcr_panel_sums", "NULL argument")
    _refused(L.snpgpu_pcr_panel_stats(None, _lib._ptr(buf)), "snpgpu_pcr_panel_stats", "NULL argument")
    fn = "snpgpu_pcr_select"
    _refused(L.snpgpu_pcr_select(None, ctypes.byref(o), 0, None, None, None, None, None, None, None, ctypes.byref(found)), fn, "pcr is NULL")
    _refused(L.snpgpu_pcr_select(fake, None, 0, None, None, None, None, None, None, None, ctypes.byref(found)), fn, "the options are NULL")
    _refused(L.snpgpu_pcr_select(fake, ctypes.byref(o), 0, None, None, None, None, None, None, None, None), fn, "n_found is NULL")
    _refused(L.snpgpu_pcr_select(fake, ctypes.byref(o), -1, None, None, None, None, None, None, None, ctypes.byref(found)), fn, "negative capacity")
    for k in range(6):                                                      # any pair output with capacity 0
        outs = [None] * 6
        outs[k] = _lib._ptr(idx if k < 2 else buf)
        _refused(L.snpgpu_pcr_select(fake, ctypes.byref(o), 0, *outs, None, ctypes.byref(found)), fn, "capacity 0 with a non-NULL output")
    assert found.value == -7
    _refused(L.snpgpu_pcr_select_stats(None), "snpgpu_pcr_select_stats", "NULL output")
    _lib.check(L.snpgpu_ws_clear())
    n_p = ctypes.c_int64(0)
    _refused(L.snpgpu_gnrPCRelatePairs(0, None, None, 0.01, 1, 128, 0.1, None, 0, ctypes.byref(found), ctypes.byref(n_p)),
             "snpgpu_gnrPCRelatePairs", "no genotype working space")
    assert L.snpgpu_gnrPCRelatePairs_get(None, None, None, None, None, None, None) == 0         # nothing kept: nothing copied


def test_panel_rows_refusals():
    """a negative panel_rows is refused before the working space is looked at; the other values need its n (test_gpu_pcrelate_panels)"""
    L = _lib.lib()
    found, n_p = ctypes.c_int64(0), ctypes.c_int64(0)
    for bad in (-1, -128):
        _refused(L.snpgpu_gnrPCRelatePairs(0, None, None, 0.01, 1, bad, 0.1, None, 0, ctypes.byref(found), ctypes.byref(n_p)),
                 "snpgpu_gnrPCRelatePairs", "panel_rows must be")
    with pytest.raises(ValueError, match="panel_rows"):
        api.snpgdsPCRelatePairs(None, None, panel_rows=0)
    with pytest.raises(TypeError, match="kinship.cutoff"):
        api.snpgdsPCRelatePairs(None, None, kinship_cutoff="0.1")


# ---- the restated selection on the restated results: what the GPU tests rely on ------------------------------------------------------

@pytest.fixture(scope="module")
def restated():
    out = {}
    for key in ((257, 500), (300, 500), (130, 1030)):
        i = P.inputs(*key)
        out[key] = R.pcrelate(i["geno"], i["pcs"], i["T"], 0.01)["result"]
    return out


@pytest.mark.parametrize("key,total,per_panel,n_nan", [((257, 500), 320, (163, 157, 0), 256), ((300, 500), 373, (163, 160, 50), 299),
                                                        ((130, 1030), 163, (163, 0), 129)])
def test_inputs_give_the_selections_the_gpu_tests_need(restated, key, total, per_panel, n_nan):
    res = restated[key]
    n = key[0]
    every = P.select(res, float("nan"))
    assert len(every["idx1"]) == n * (n - 1) // 2
    assert np.all(every["idx1"] < every["idx2"])
    order = every["idx1"].astype(np.int64) * n + every["idx2"]
    assert np.all(np.diff(order) > 0)                                      # idx1 ascending, then idx2 ascending
    assert int(np.isnan(every["kinship"]).sum()) == n_nan                  # the sample without a call
    hits = P.select(res, P.CUTOFF)
    assert len(hits["idx1"]) == total
    panels = P.partition(n, P.TILE)
    counts = tuple(len(P.select(res, P.CUTOFF, rows=r)["idx1"]) for r in panels)
    print(key, counts)
    assert counts == per_panel
    # hits in at least two panels (n = 257, 300), a panel without a hit (n = 257: the ragged last row; n = 130: the ragged rest)
    assert sum(c > 0 for c in counts) >= (2 if n > 256 else 1) and (0 in counts) == (n != 300)
    # the union of the panels is the whole selection, in its order
    for k in ("idx1", "idx2") + P.VALUES:
        assert P.same_bits(np.concatenate([P.select(res, P.CUTOFF, rows=r)[k] for r in panels]).astype(np.float64), hits[k].astype(np.float64)), k
    kin = every["kinship"][np.isfinite(every["kinship"])]
    assert np.abs(kin - P.CUTOFF).min() > 1e-6                             # no decision of the selection is close
    assert np.any(kin < R.KIN_SPLIT) and np.any(hits["kinship"] > R.KIN_SPLIT)     # both branches of k0 among the pairs that are compared
    assert not np.any(np.isnan(hits["kinship"])) and hits["kinship"].min() >= P.CUTOFF
    # the values are the lower triangle's, the entries snpgdsIBDSelection reads
    ids = np.arange(n)
    tab = api.snpgdsIBDSelection(dict(sample_id=ids, kinship=res["kinship"], k0=res["k0"], k2=res["k2"], nsnp=res["nsnp"]), P.CUTOFF)
    assert np.array_equal(tab["ID1"], hits["idx1"]) and np.array_equal(tab["ID2"], hits["idx2"])
    for k in P.VALUES:
        assert P.same_bits(tab[k], hits[k]), k


def test_selection_rule_on_a_small_matrix():
    kin = np.array([[0.5, 0.3, np.nan, 0.1], [0.3, 0.5, 0.05, np.nan], [np.nan, 0.05, 0.5, 0.26], [0.1, np.nan, 0.26, 0.5]])
    res = dict(kinship=kin, nsnp=np.arange(16.0).reshape(4, 4))
    s = P.select(res, 0.1)
    assert s["idx1"].tolist() == [0, 0, 2] and s["idx2"].tolist() == [1, 3, 3] and s["nsnp"].tolist() == [4.0, 12.0, 14.0]
    assert "k0" not in s
    for cut in (float("nan"), float("inf"), float("-inf")):
        assert len(P.select(res, cut)["idx1"]) == 6                        # a non-finite cutoff: every pair, NaN pairs included
    assert len(P.select(res, 0.6)["idx1"]) == 0
    assert P.select(res, 0.1, samp_sel=[1, 0, 1, 1])["idx2"].tolist() == [3, 3]
    assert P.select(res, 0.1, rows=(2, 4))["idx1"].tolist() == [2]
    assert P.partition(300, 128) == [(0, 128), (128, 256), (256, 300)] and P.partition(130, 256) == [(0, 130)]
    assert P.panel_cut(np.arange(16).reshape(4, 4), 1, 3).tolist() == [[5, 6, 7], [9, 10, 11]]
    assert P.same_bits(np.array([np.nan, 1.0]), np.array([np.nan, 1.0])) and not P.same_bits(np.array([0.0]), np.array([-0.0]))
