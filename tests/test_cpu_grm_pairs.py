"""The sparse GRM without a GPU: the selection rule of tests/grm_pairs_ref.py against a plain double loop, the new symbols, every
refusal of snpgpu_select_grm / snpgpu_multi_select_grm / snpgpu_gnrGRMPairs that needs no device, and the .grm.id / .grm.sp writer on
hand-made arrays."""
import ctypes

import numpy as np
import pytest

import grm_pairs_ref as R

NAN = float("nan")
INF = float("inf")
NEW_SYMBOLS = ["snpgpu_select_grm", "snpgpu_multi_select_grm", "snpgpu_gnrGRMPairs", "snpgpu_gnrGRMPairs_get", "snpgpu_select_grm_stats"]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def _random_matrix(n, seed):
    """symmetric, with planted NaN, +Inf, -Inf and entries equal to the cutoffs used below"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 0.1, (n, n))
    a = np.triu(a) + np.triu(a, 1).T
    for k, x in enumerate((NAN, INF, -INF, 0.05, 0.05, 0.0, NAN)):
        i, j = sorted(rng.choice(n, 2, replace=False).tolist())
        a[i, j] = a[j, i] = x
    a[n // 2, n // 2] = NAN                     # a diagonal entry too
    return a


def _packed(a, n, rows):
    i, j = R.slab_rc(n, *rows)
    return a[i, j]


@pytest.mark.parametrize("n,rows", [(23, (0, 23)), (23, (0, 8)), (23, (8, 16)), (23, (16, 23)), (9, (8, 9)), (1, (0, 1))])
@pytest.mark.parametrize("cutoff", [NAN, INF, -INF, 0.0, 0.05, 10.0, -10.0])
def test_selection_equals_a_double_loop(n, rows, cutoff):
    a = _random_matrix(n, 100 + n) if n > 2 else np.array([[0.7]])
    rng = np.random.default_rng(n)
    for mask in (None, rng.random(n) < 0.6):
        ref = R.selection_loops(a.tolist(), n, rows, cutoff, None if mask is None else mask.tolist())
        for form in (a, _packed(a, n, rows)):
            got = R.selection(form, n, rows, cutoff, mask)
            assert R.same_selection(got, ref) is None, R.same_selection(got, ref)
        assert (ref["idx1"] < ref["idx2"]).all() and ref["diag"].size == min(rows[1], n) - rows[0]
        key = ref["idx1"] * n + ref["idx2"]
        assert (np.diff(key) > 0).all()                                          # row-major order
        if np.isfinite(cutoff):
            assert not np.isnan(ref["value"]).any() and (ref["value"] >= cutoff).all()
        elif mask is None and rows == (0, n):
            assert ref["idx1"].size == n * (n - 1) // 2                          # NaN pairs included


def test_selection_keeps_an_entry_equal_to_the_cutoff_and_drops_nan():
    a = np.array([[1.0, 0.05, NAN, -INF], [0.05, 1.0, INF, np.nextafter(0.05, 0.0)], [NAN, INF, 1.0, 0.3], [-INF, 0.04, 0.3, NAN]])
    a = np.triu(a) + np.triu(a, 1).T
    t = R.selection(a, 4, (0, 4), 0.05)
    assert list(zip(t["idx1"].tolist(), t["idx2"].tolist())) == [(0, 1), (1, 2), (2, 3)]
    assert R.same_bits(t["diag"], [1.0, 1.0, 1.0, NAN])
    t = R.selection(a, 4, (0, 4), NAN)
    assert t["idx1"].size == 6 and np.isnan(t["value"][1])
    assert not R.same_bits([0.1], [np.nextafter(0.1, 1.0)]) and R.same_bits([NAN, 0.0], [-NAN, 0.0]) and not R.same_bits([0.0], [-0.0])


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported():
    from snprelate_amd import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s), s
    assert L.snpgpu_abi_version() == 2
    assert hasattr(_lib.Accumulator, "select_grm") and hasattr(_lib.MultiAccumulator, "select_grm")
    assert ctypes.sizeof(_lib.GrmSelOpts) == 40                                  # 2 x int32, 3 x double, a pointer
    import snprelate_amd
    assert callable(snprelate_amd.snpgdsGRMPairs)


def _opts(what=1, mode=0, scale=1.0, trace_in=0.0, cutoff=0.05):
    from snprelate_amd import _lib
    return _lib.GrmSelOpts(what, mode, scale, trace_in, cutoff, None)


@pytest.mark.parametrize("fn", ["snpgpu_select_grm", "snpgpu_multi_select_grm"])
def test_refusals_before_any_device(fn):
    """no context exists here, so none of these may reach a device: nonzero, the function's name and the reason in snpgpu_last_error,
    the outputs and *n_found untouched"""
    from snprelate_amd import _lib
    L = _lib.lib()
    call = getattr(L, fn)
    multi = fn == "snpgpu_multi_select_grm"

    def refused(o, capacity, with_outputs, word):
        i1, i2 = np.full(4, -9, np.int32), np.full(4, -9, np.int32)
        v, d = np.full(4, -9.0), np.full(4, -9.0)
        avg, found = ctypes.c_double(-9.0), ctypes.c_int64(-9)
        outs = [_lib._ptr(x) if with_outputs else None for x in (i1, i2, v)]
        tail = [_lib._ptr(d)] + ([] if multi else [ctypes.byref(avg)]) + [ctypes.byref(found)]
        rc = call(None, ctypes.byref(o) if o is not None else None, capacity, *outs, *tail)
        msg = L.snpgpu_last_error().decode()
        assert rc != 0 and word in msg and fn in msg, (rc, msg)
        assert found.value == -9 and avg.value == -9.0
        assert all((x == -9).all() for x in (i1, i2, v, d))

    refused(None, 0, False, "NULL opts")
    refused(_opts(what=0), 0, False, "invalid 'what'")
    refused(_opts(what=5), 4, True, "invalid 'what'")
    for scale in (0.0, -1.0, NAN, INF):
        refused(_opts(what=3, scale=scale), 0, False, "invalid scale")
    refused(_opts(what=3, mode=2, scale=2.0), 0, False, "invalid mode")
    refused(_opts(what=3, mode=-1, scale=2.0), 0, False, "invalid mode")
    refused(_opts(what=1), -1, False, "negative capacity")
    refused(_opts(what=1), 0, True, "capacity 0 with a non-NULL output")
    if multi:
        for mode in (0, 1, 2):
            refused(_opts(what=4, mode=mode), 0, False, "INDIV_BETA needs a full context")
        refused(_opts(what=4, mode=3), 0, False, "invalid mode")
    else:
        refused(_opts(what=4, mode=3), 0, False, "invalid mode")
        refused(_opts(what=4, mode=-1), 4, True, "invalid mode")
        refused(_opts(what=4, mode=2), 4, True, "NULL context")
    for what in (1, 2, 3):
        refused(_opts(what=what, scale=2.0), 4, True, "NULL object" if multi else "NULL context")
        refused(_opts(what=what, scale=2.0), 0, False, "NULL object" if multi else "NULL context")


def test_select_pairs_still_refuses_the_grm_kinds():
    """snpgpu_select_pairs and its options are unchanged: what = 4 is no kind of it"""
    from snprelate_amd import _lib
    L = _lib.lib()
    o = _lib.SelOpts(4, 0, None, None, 0.1, None)
    found = ctypes.c_int64(-9)
    assert L.snpgpu_select_pairs(None, ctypes.byref(o), 0, None, None, None, None, None, _lib.HOST, ctypes.byref(found)) != 0
    assert "invalid 'what'" in L.snpgpu_last_error().decode() and found.value == -9


def test_stats_need_an_output():
    from snprelate_amd import _lib
    L = _lib.lib()
    assert L.snpgpu_select_grm_stats(None) != 0 and "snpgpu_select_grm_stats" in L.snpgpu_last_error().decode()
    assert set(_lib.select_grm_stats()) == {"count_ms", "scan_ms", "write_ms", "diag_ms", "call_ms"}


def test_working_space_route_refusals():
    from snprelate_amd import _lib
    L = _lib.lib()
    L.snpgpu_ws_clear()
    found = ctypes.c_int64(-9)
    for method in (b"GCTA", b"Eigenstrat", b"EIGMIX", b"IndivBeta"):
        assert L.snpgpu_gnrGRMPairs(method, 0.05, None, 1, 0, ctypes.byref(found)) != 0
        msg = L.snpgpu_last_error().decode()
        assert "no genotype working space" in msg and "snpgpu_gnrGRMPairs" in msg
    for method in (b"Corr", b"Weighted", b"gcta", b""):
        assert L.snpgpu_gnrGRMPairs(method, 0.05, None, 1, 0, ctypes.byref(found)) != 0
        msg = L.snpgpu_last_error().decode()
        assert "snpgpu_gnrGRMPairs" in msg and "'%s'" % method.decode() in msg, msg
    assert L.snpgpu_gnrGRMPairs(b"Corr", 0.05, None, 1, 0, ctypes.byref(found)) != 0
    assert "not built" in L.snpgpu_last_error().decode()
    assert L.snpgpu_gnrGRMPairs(None, 0.05, None, 1, 0, ctypes.byref(found)) != 0
    assert found.value == -9
    avg = ctypes.c_double(-9.0)
    assert L.snpgpu_gnrGRMPairs_get(None, None, None, None, ctypes.byref(avg)) == 0 and avg.value == 0.0     # nothing kept


def test_api_refuses_corr_and_unknown_methods_before_opening_anything():
    from snprelate_amd import api
    with pytest.raises(ValueError, match="'Corr' is not built"):
        api.snpgdsGRMPairs(None, method="Corr")
    with pytest.raises(ValueError, match="should be one of"):
        api.snpgdsGRMPairs(None, method="gcta")
    with pytest.raises(TypeError, match=r"is.numeric\(cutoff\)"):
        api.snpgdsGRMPairs(None, cutoff="0.05")


# ---- the text files -----------------------------------------------------------------------------------------------------------------------

def _hand_made():
    ids = np.array(["s0", "s1", "s2", "s3", "s4"])
    idx1 = np.array([0, 0, 1, 2], np.int32)
    idx2 = np.array([2, 4, 2, 4], np.int32)
    value = np.array([0.1, np.nextafter(0.05, 1.0), 1.0 / 3.0, -2.5e-300])
    diag = np.array([1.0000000000000002, 0.9, NAN, 1.1, 5e-324])
    return ids, idx1, idx2, value, diag


def test_writer_layout(tmp_path):
    from snprelate_amd import api
    ids, idx1, idx2, value, diag = _hand_made()
    prefix = str(tmp_path / "hand")
    api.write_sparse_grm(prefix, ids, idx1, idx2, value, diag)
    assert open(prefix + ".grm.id").read() == "".join("%s\t%s\n" % (s, s) for s in ids)
    rid, row, col, val = R.read_sparse_grm(prefix)
    assert list(rid) == list(ids)
    assert (row >= col).all()
    assert list(zip(row.tolist(), col.tolist())) == [(0, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 3), (4, 0), (4, 2), (4, 4)]
    assert (np.diff(row * 5 + col) > 0).all()                                    # sorted by row, then by column
    d = row == col
    assert np.array_equal(row[d], np.arange(5)) and R.same_bits(val[d], diag)    # every diagonal present, float(text) == value
    assert R.same_bits(val[~d], [0.1, 1.0 / 3.0, np.nextafter(0.05, 1.0), -2.5e-300])
    for k in np.flatnonzero(d):                                                  # the diagonal closes its row
        assert k + 1 == row.size or row[k + 1] == row[k] + 1
    lines = open(prefix + ".grm.sp").read().splitlines()
    assert lines[0] == "0\t0\t1.0000000000000002" and lines[2] == "2\t0\t0.10000000000000001" and all(x.count("\t") == 2 for x in lines)


def test_writer_renumbers_with_samp_sel(tmp_path):
    from snprelate_amd import api
    ids, idx1, idx2, value, diag = _hand_made()
    mask = np.array([1, 0, 1, 0, 1], np.uint8)
    keep = mask[idx1].astype(bool) & mask[idx2].astype(bool)
    prefix = str(tmp_path / "sel")
    api.write_sparse_grm(prefix, ids, idx1[keep], idx2[keep], value[keep], diag, mask)
    rid, row, col, val = R.read_sparse_grm(prefix)
    assert list(rid) == ["s0", "s2", "s4"]
    assert list(zip(row.tolist(), col.tolist())) == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    assert R.same_bits(val, [diag[0], 0.1, diag[2], np.nextafter(0.05, 1.0), -2.5e-300, diag[4]])
    with pytest.raises(ValueError, match="leaves out"):
        api.write_sparse_grm(prefix, ids, idx1, idx2, value, diag, mask)
    with pytest.raises(ValueError, match="idx1 < idx2"):
        api.write_sparse_grm(prefix, ids, idx2, idx1, value, diag)
    # no pair at all: the diagonal alone
    api.write_sparse_grm(prefix, ids, idx1[:0], idx2[:0], value[:0], diag)
    rid, row, col, val = R.read_sparse_grm(prefix)
    assert np.array_equal(row, np.arange(5)) and np.array_equal(col, np.arange(5)) and R.same_bits(val, diag)
