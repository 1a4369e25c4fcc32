"""tests/mem_kinds.py without a GPU: the guard and fill checks of a device destination on a numpy twin of its buffer, and the table of
calls with a result memory kind against include/snpgpu.h and against tests/test_gpu_device_results.py -- an entry point that takes
out_mem / dst_mem cannot be added to the header without a device-destination test."""
import ast
import os

import numpy as np
import pytest

import mem_kinds as M
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "snpgpu.h")
GPU_TESTS = os.path.join(ROOT, "tests", "test_gpu_device_results.py")


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.uint32, np.int64, np.uint8])
@pytest.mark.parametrize("offset", M.OFFSETS)
def test_layout_alignment_and_guards(dtype, offset):
    lay = M.DestLayout((7, 5), dtype, offset)
    item = np.dtype(dtype).itemsize
    assert lay.begin >= 4096 and lay.total - lay.end >= 4096 and lay.total % 256 == 0
    assert (lay.begin - offset * item) % 256 == 0          # `offset` elements past a 256-byte boundary of an aligned allocation
    if item == 8:
        assert lay.begin % 8 == 0 and lay.begin % 16 == 8   # 8-byte but not 16-byte aligned
    if item == 4:
        assert lay.begin % 4 == 0 and lay.begin % 8 == 4
    raw = lay.new_buffer()
    assert np.all(raw == M.FILL)
    lay.check(raw)                                          # nothing written: clean
    lay.untouched(raw, np.ones((7, 5), bool))


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.uint8])
def test_clean_write_passes_and_is_returned(dtype):
    lay = M.DestLayout((3, 11), dtype, 3)
    raw = lay.new_buffer()
    val = (np.arange(33).reshape(3, 11) % 200).astype(dtype)
    lay.result(raw)[...] = val
    got = lay.check(raw)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, val)


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.uint8])
@pytest.mark.parametrize("where", ["before", "after"])
def test_one_element_outside_is_reported(dtype, where):
    lay = M.DestLayout((19,), dtype, 1)
    item = np.dtype(dtype).itemsize
    raw = lay.new_buffer()
    lay.result(raw)[...] = 1
    lo = lay.begin - item if where == "before" else lay.end
    raw[lo:lo + item] = np.ones(1, dtype).view(np.uint8)
    with pytest.raises(AssertionError, match="written %s the result" % where.upper()):
        lay.check(raw)
    # ... and the far end of either guard is watched as well
    raw = lay.new_buffer()
    raw[0 if where == "before" else lay.total - 1] = 0
    with pytest.raises(AssertionError, match="write outside a result"):
        lay.check(raw)


def test_untouched_elements():
    lay = M.DestLayout((4, 4), np.float64, 1)
    raw = lay.new_buffer()
    r = lay.result(raw)
    r[0, 1:] = 0.25                                          # row 0 written, the rest left
    mask = np.ones((4, 4), bool)
    mask[0, 1:] = False
    lay.untouched(raw, mask)
    r[2, 3] = 0.0
    with pytest.raises(AssertionError, match=r"have been written, the first at \(2, 3\)"):
        lay.untouched(raw, mask)
    lay.check(raw)                                           # (the guards are a separate statement)


def test_header_parser_on_known_prototypes():
    protos = M.header_prototypes(open(HEADER).read())
    assert protos["snpgpu_ibs_ave"] == ["ctx", "out", "packed", "mem"]
    assert protos["snpgpu_ld_result"] == ["ld", "out", "out_mem"]
    assert protos["snpgpu_geno_select"][-3:] == ["dst_mem", "device", "stream"]
    assert protos["snpgpu_multi_select_pairs"][-2:] == ["mem", "n_found"]
    assert len(protos) > 150


def test_every_result_memory_kind_of_the_header_is_in_the_table():
    protos = M.header_prototypes(open(HEADER).read())
    must = sorted(f for f, params in protos.items() if "out_mem" in params or "dst_mem" in params)
    assert len(must) >= 15
    missing = [f for f in must if f not in M.RESULT_CALLS]
    assert not missing, "calls with a result memory kind and no device-destination test: %s" % ", ".join(missing)
    # the finalisers and gathers name theirs `mem`: every finaliser of a context or of a multi-device object that takes one
    fin = [f for f, params in protos.items()
           if params and params[0] in ("ctx", "m") and "mem" in params and f not in ("snpgpu_feed", "snpgpu_feed_stats", "snpgpu_multi_feed",
                                                                                      "snpgpu_multi_select_pairs")]
    missing = [f for f in fin if f not in M.RESULT_CALLS]
    assert len(fin) >= 20 and not missing, "finalisers with a memory kind and no device-destination test: %s" % ", ".join(missing)


def test_every_table_entry_is_in_the_header_with_its_parameter():
    protos = M.header_prototypes(open(HEADER).read())
    for f, e in M.RESULT_CALLS.items():
        assert f in protos, "%s is not declared in include/snpgpu.h" % f
        assert e["param"] in ("mem", "out_mem", "dst_mem") and e["param"] in protos[f], \
            "%s has no parameter %s (it has %s)" % (f, e["param"], protos[f])
        other = {"mem", "out_mem", "dst_mem"} - {e["param"]}
        if e["param"] != "mem":
            assert not (other - {"mem"}) & set(protos[f])
        assert e["compare"] == M.BYTES or e["compare"].startswith("oracle: ")
        assert e["tests"]


def test_every_named_test_exists_and_is_a_gpu_test():
    tree = ast.parse(open(GPU_TESTS).read())
    defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    named = {t for e in M.RESULT_CALLS.values() for t in e["tests"]}
    assert not named - defined, "named in RESULT_CALLS, absent from test_gpu_device_results.py: %s" % sorted(named - defined)
    src = open(GPU_TESTS).read()
    assert "pytestmark = pytest.mark.gpu" in src
    # every C function of the table is reached: its wrapper's name occurs in the file that claims to test it
    for f in M.RESULT_CALLS:
        stem = f[len("snpgpu_"):]
        for prefix in ("multi_", "proj_", "ld_", "panels_"):
            if stem.startswith(prefix):
                stem = stem[len(prefix):]
        assert stem in src, "%s: no call of `%s` in test_gpu_device_results.py" % (f, stem)
