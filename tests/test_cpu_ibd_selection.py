"""snpgdsIBDSelection on the host (R/IBD.R:463-531) and what of the selection ABI needs no GPU: the exported symbols and the refusals
that are decided before any device is touched.  tests/ibd_selection_ref.py is the restated reference; the 5 x 5 object below and its
expected tables are written out by hand."""
import ctypes

import numpy as np
import pytest

import ibd_selection_ref as R

NAN = float("nan")
IDS = np.array(["a", "b", "c", "d", "e"])
# symmetric, kinship of the pair (row, col); (c, e) is NaN; (a, d) is exactly 0.125
K5 = np.array([[0.5, 0.30, 0.02, 0.125, -0.01],
               [0.30, 0.5, 0.25, 0.01, 0.26],
               [0.02, 0.25, 0.5, 0.06, NAN],
               [0.125, 0.01, 0.06, 0.5, 0.0],
               [-0.01, 0.26, NAN, 0.0, 0.5]])
I5 = np.arange(25, dtype=np.float64).reshape(5, 5)
I5 = (I5 + I5.T) / 100.0                                   # IBS0 stand-in: entry (r, c) = (5 r + c + 5 c + r) / 100 = 0.06 (r + c)
ALL_PAIRS = [("a", "b"), ("a", "c"), ("a", "d"), ("a", "e"), ("b", "c"), ("b", "d"), ("b", "e"), ("c", "d"), ("c", "e"), ("d", "e")]


def _obj5():
    return dict(sample_id=IDS, snp_id=np.arange(7), afreq=None, IBS0=I5, kinship=K5)


def _sel(*a, **k):
    from snprelate_amd.api import snpgdsIBDSelection
    return snpgdsIBDSelection(*a, **k)


def _pairs(t):
    return list(zip(t["ID1"].tolist(), t["ID2"].tolist()))


def test_hand_written_finite_cutoff():
    t = _sel(_obj5(), 0.1)
    assert list(t) == ["ID1", "ID2", "IBS0", "kinship"]
    assert _pairs(t) == [("a", "b"), ("a", "d"), ("b", "c"), ("b", "e")]
    assert t["kinship"].tolist() == [0.30, 0.125, 0.25, 0.26]
    assert np.allclose(t["IBS0"], [0.06, 0.18, 0.18, 0.30], rtol=0, atol=1e-15)


def test_hand_written_cutoff_equal_to_an_entry_is_included():
    assert _pairs(_sel(_obj5(), 0.125)) == [("a", "b"), ("a", "d"), ("b", "c"), ("b", "e")]
    assert _pairs(_sel(_obj5(), np.nextafter(0.125, 1.0))) == [("a", "b"), ("b", "c"), ("b", "e")]
    assert _pairs(_sel(_obj5(), 0.0)) == [p for p in ALL_PAIRS if p not in (("a", "e"), ("c", "e"))]      # d-e is exactly 0.0


@pytest.mark.parametrize("cutoff", [NAN, float("inf"), float("-inf")])
def test_hand_written_non_finite_cutoff_is_every_pair(cutoff):
    t = _sel(_obj5(), cutoff)
    assert _pairs(t) == ALL_PAIRS
    k = t["kinship"]
    assert np.isnan(k[8]) and np.isnan(k).sum() == 1                           # the NaN pair (c, e) is present
    assert k[[0, 1, 2, 3, 9]].tolist() == [0.30, 0.02, 0.125, -0.01, 0.0]


def test_hand_written_nan_entry_is_excluded_with_a_finite_cutoff():
    assert ("c", "e") not in _pairs(_sel(_obj5(), -1.0))
    assert len(_pairs(_sel(_obj5(), -1.0))) == 9
    assert _pairs(_sel(_obj5(), 10.0)) == []


def _random_obj(n, seed, keys=("kinship",)):
    rng = np.random.default_rng(seed)
    obj = dict(sample_id=np.arange(100, 100 + n), snp_id=None, afreq=None)
    for k in keys:
        m = rng.random((n, n))
        m = (m + m.T) / 2
        m[rng.random((n, n)) < 0.03] = NAN
        m = np.where(np.isnan(m.T), NAN, m)
        obj[k] = m
    return obj


@pytest.mark.parametrize("n", [2, 7, 33])
def test_reference_order_is_row_then_column_of_the_upper_triangle(n):
    """which(lower.tri & flag, arr.ind=TRUE) in column-major order = i ascending, then j ascending, i < j"""
    obj = _random_obj(n, n)
    for cutoff in (NAN, 0.5):
        t = R.selection(obj, cutoff)
        i, j = np.triu_indices(n, 1)                                           # row-major walk of the strict upper triangle
        if np.isfinite(cutoff):
            with np.errstate(invalid="ignore"):
                keep = obj["kinship"][i, j] >= cutoff
            i, j = i[keep], j[keep]
        assert np.array_equal(t["ID1"], obj["sample_id"][i]) and np.array_equal(t["ID2"], obj["sample_id"][j])
        assert np.array_equal(t["kinship"], obj["kinship"][i, j], equal_nan=True)
        assert R.same_table(_sel(obj, cutoff), t) is None


def test_k0_k1_objects_derive_and_append_kinship():
    obj = _random_obj(9, 3, keys=("k0", "k1"))
    obj["afreq"] = np.linspace(0.1, 0.9, 4)
    obj["niter"] = None                                                        # snpgdsIBDMLE(out_num_iter=False)
    t = _sel(obj, 0.2)
    assert list(t) == ["ID1", "ID2", "k0", "k1", "kinship"]
    assert R.same_table(t, R.selection(obj, 0.2)) is None
    assert t["ID1"].size and np.array_equal(t["kinship"], (1 - t["k0"] - t["k1"]) * 0.5 + t["k1"] * 0.25)
    assert (t["kinship"] >= 0.2).all()
    obj["kinship"] = np.full((9, 9), 0.3)                                      # an object that has one keeps it (snpgdsIBDMoM(kinship=TRUE))
    t = _sel(obj, 0.2)
    assert list(t) == ["ID1", "ID2", "k0", "k1", "kinship"] and t["ID1"].size == 36 and (t["kinship"] == 0.3).all()


def test_jacquard_objects():
    keys = tuple("D%d" % k for k in range(1, 9))
    obj = _random_obj(8, 5, keys=keys)
    t = _sel(obj, 1.0)
    assert list(t) == ["ID1", "ID2"] + list(keys) + ["kinship"]
    assert R.same_table(t, R.selection(obj, 1.0)) is None
    assert t["ID1"].size and np.array_equal(t["kinship"], t["D1"] + 0.5 * (t["D3"] + t["D5"] + t["D7"]) + 0.25 * t["D8"])


def test_object_without_a_kinship_coefficient():
    obj = _random_obj(6, 8, keys=("ibs",))
    with pytest.raises(ValueError, match="There is no kinship coefficient."):
        _sel(obj, 0.1)
    t = _sel(obj, NAN)
    assert list(t) == ["ID1", "ID2", "ibs"] and t["ID1"].size == 15
    assert R.same_table(t, R.selection(obj, NAN)) is None


def test_argument_checks():
    with pytest.raises(TypeError, match="snpgdsIBDClass"):
        _sel([1, 2, 3])
    with pytest.raises(TypeError, match=r"is.numeric\(kinship.cutoff\)"):
        _sel(_obj5(), "0.1")
    with pytest.raises(ValueError, match=r"length\(samp.sel\)"):
        _sel(_obj5(), 0.1, samp_sel=np.array([True, False]))
    with pytest.raises(TypeError, match="samp.sel"):
        _sel(_obj5(), 0.1, samp_sel=np.array(["a"]))


def test_packed_triangle_input():
    n = 11
    obj = _random_obj(n, 21, keys=("IBS0", "kinship"))
    i, j = np.triu_indices(n)
    packed = dict(obj, IBS0=obj["IBS0"][i, j], kinship=obj["kinship"][i, j])
    for cutoff in (NAN, 0.4):
        assert R.same_table(_sel(packed, cutoff), R.selection(obj, cutoff)) is None
    assert np.array_equal(R.packed_to_full(packed["kinship"], n), obj["kinship"], equal_nan=True)


@pytest.mark.parametrize("cutoff", [NAN, 0.1])
def test_samp_sel_logical_increasing_and_permuting(cutoff):
    n = 14
    obj = _random_obj(n, 2, keys=("k0", "k1"))
    rng = np.random.default_rng(4)
    logical = rng.random(n) < 0.6
    increasing = np.flatnonzero(logical)
    permuting = rng.permutation(n)[:9]
    assert np.any(np.diff(permuting) < 0)
    for sel in (logical, increasing, permuting, permuting.astype(np.float64)):
        ref = R.selection(obj, cutoff, sel.astype(np.int64) if sel.dtype.kind == "f" else sel)
        assert ref["ID1"].size
        assert R.same_table(_sel(obj, cutoff, sel), ref) is None
    assert R.same_table(_sel(obj, cutoff, logical), _sel(obj, cutoff, increasing)) is None
    t = _sel(obj, NAN, permuting)                                              # ID1 follows the ORDER of the selection, as R's indexing
    assert t["ID1"][0] == obj["sample_id"][permuting[0]] and t["ID2"][0] == obj["sample_id"][permuting[1]]


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("snpgpu_select_pairs", "snpgpu_multi_select_pairs", "snpgpu_gnrIBDPairs", "snpgpu_gnrIBDPairs_get")


def test_new_symbols_are_exported():
    from snprelate_amd import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s), s
    assert L.snpgpu_abi_version() == 2
    assert hasattr(_lib.Accumulator, "select_pairs") and hasattr(_lib.MultiAccumulator, "select_pairs")


def _opts(what, e=None, cutoff=NAN):
    from snprelate_amd import _lib
    return _lib.SelOpts(what, 0, None, None if e is None else e.ctypes.data_as(ctypes.c_void_p), cutoff, None)


@pytest.mark.parametrize("fn", ["snpgpu_select_pairs", "snpgpu_multi_select_pairs"])
def test_refusals_before_any_device(fn):
    """NULL context / object, NULL opts, MOM without e, a negative capacity, an output with capacity 0: nonzero, with the word in
    snpgpu_last_error -- no context exists here, so none of these may reach a device"""
    from snprelate_amd import _lib
    L = _lib.lib()
    call = getattr(L, fn)
    found = ctypes.c_int64(-7)
    e = np.array([0.1, 0.2, 0.3, 0.2, 0.2])
    buf = np.full(4, 77, np.int32)

    def refused(opts, capacity, idx1, word):
        rc = call(None, None if opts is None else ctypes.byref(opts), capacity, idx1, None, None, None, None, _lib.HOST, ctypes.byref(found))
        msg = L.snpgpu_last_error().decode()
        assert rc != 0 and word in msg and fn in msg, (rc, msg)

    refused(None, 0, None, "NULL opts")
    refused(_opts(_lib.SEL_KING_ROBUST), 0, None, "NULL context" if fn == "snpgpu_select_pairs" else "NULL object")
    refused(_opts(_lib.SEL_MOM), 0, None, "e is NULL")
    refused(_opts(_lib.SEL_MOM, e), -1, None, "negative capacity")
    refused(_opts(_lib.SEL_KING_HOMO), 0, buf.ctypes.data_as(ctypes.c_void_p), "capacity 0")
    refused(_opts(9), 0, None, "invalid 'what'")
    assert found.value == -7 and (buf == 77).all()


def test_working_space_route_refuses_without_a_working_space():
    from snprelate_amd import _lib
    L = _lib.lib()
    L.snpgpu_ws_clear()
    found = ctypes.c_int64(0)
    assert L.snpgpu_gnrIBDPairs(_lib.SEL_KING_ROBUST, None, None, 0, 0.1, None, 1, 0, ctypes.byref(found)) != 0
    assert "no genotype working space" in L.snpgpu_last_error().decode()
    assert L.snpgpu_gnrIBDPairs(0, None, None, 0, 0.1, None, 1, 0, ctypes.byref(found)) != 0
    assert "invalid 'what'" in L.snpgpu_last_error().decode()
    assert L.snpgpu_gnrIBDPairs_get(None, None, None, None, None) == 0         # nothing kept: nothing to copy
