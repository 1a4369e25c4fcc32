"""CPU tests of the text formats (no device): the restatements of the reference's writers and of gnrParsePED (tests/text_ref.py)
reproduce the hand-derived literals; the package's host side of snpgdsOpenPED -- GetCell splitting by space and tab, the MAP
order, the choice of the reference allele -- equals the restatement on every irregular form; every refusal of the new ABI calls
that needs no device returns its status with a message; the header declares the calls, without a result memory kind."""
import os

import numpy as np
import pytest

import mem_kinds as M
import text_ref as R
from conftest import ROOT
from snprelate_amd import _lib, ped, vcf


# ---- the literals -----------------------------------------------------------------------------------------------------------------
GENO = [[0, 1, 2, 3], [2, 3, 1, 0], [1, 0, 3, 2]]
ALLELES = ["A/G", "T/", "AT/A", "C/G/T"]
PED_IN = (b"F1\ts1\t0\t0\t1\t-9\tA G\tT T\t0 0\n"
          b"F1 s2 s1 0 2 1  G G T C C 0\n"
          b"F2\ts3\t0\t0\t0\t2\tA A\tT T\tC C\n")


def test_restatements_reproduce_the_out_literals():
    ids = ["s1", "s2", "s3"]
    assert R.ped_text(ids, ALLELES, GENO, 1) == (b"0\ts1\t0\t0\t0\t-9\tG G\tT 0\tAT AT\t0 0\n"
                                                 b"0\ts2\t0\t0\t0\t-9\tA A\t0 0\tAT A\tG G\n"
                                                 b"0\ts3\t0\t0\t0\t-9\tA G\t0 0\t0 0\tC C\n")
    assert R.ped_text(ids, None, GENO, 2).split(b"\n")[0] == b"0\ts1\t0\t0\t0\t-9\tB B\tA B\tA A\t0 0"
    assert R.ped_text(ids, None, GENO, 3).split(b"\n")[0] == b"0\ts1\t0\t0\t0\t-9\t2 2\t1 2\t1 1\t0 0"
    assert R.eigen_text(np.array(GENO).T) == b"021\n190\n219\n902\n"


def test_restatement_reproduces_the_in_literal():
    d = R.parse_ped(PED_IN, 3)
    assert d["allele"] == ["A/G", "T/C", "C/0"]
    assert d["geno"].tolist() == [[1, 2, 3], [0, 1, 3], [2, 2, 2]]
    assert d["sex"] == ["M", "F", "0"] and d["phenotype"] == ["-9", "1", "2"]
    assert d["sample_id"] == ["s1", "s2", "s3"] and d["family"] == ["F1", "F1", "F2"] and d["father"] == ["0", "s1", "0"]


def test_split_alleles_as_the_writer_splits_them():
    from snprelate_amd.text import split_alleles
    assert split_alleles(ALLELES + ["", "/", "/G", "A"]) == [b"A", b"G", b"T", b"0", b"AT", b"A", b"C", b"G", b"0", b"0", b"0", b"0",
                                                              b"0", b"G", b"A", b"0"]


# ---- GetCell by space and tab: the package's host side against the restatement ---------------------------------------------------------
HEAD = b"F\ti\t0\t0\t1\t-9"
LINES = [
    HEAD + b"\tA G\tT T",                       # regular
    HEAD + b"\tA\tG\tT\tT",                     # one tab between alleles
    b"F i 0 0 1 -9 A G T T",                    # spaces
    b"F  i   0 0 1 -9  A   G T T   ",           # runs of spaces, trailing spaces behind the last column
    HEAD + b"\tA G\tT T\r",                     # (the '\r' is stripped with the line end: see below)
    HEAD + b"\tA\t\tG\tT",                      # \t\t: an empty cell, which is an allele ""
    HEAD + b"\tA \tG\tT",                       # space then tab: an empty cell
    HEAD + b"\t\"AT\" 'G'\tT \"",               # quoted tokens lose their quotes when two or more bytes long
    HEAD + b"\tAT A\tT TTT",                    # indels
    HEAD + b"\tA G\tT",                         # one token too few
    HEAD + b"\tA G\tT T\tC",                    # one token too many
    HEAD + b"\tA G\tT T\t",                     # a tab behind the last column
    HEAD,                                       # no allele at all
    b"",                                        # a blank line
    b"F\ti\t0",                                 # the leading columns cut short
]


def _ref_cells(line, n_snp):
    rl = R.ReadLine(line + b"\n")
    cell, out = b"", []
    try:
        for k in range(6 + 2 * n_snp):
            cell = rl.get_cell(k >= 6 + 2 * n_snp - 1)
            out.append(cell)
    except ValueError as e:
        return ("error", str(e), rl.column_no, cell)
    return out


def _pkg_cells(line, n_snp):
    if line.endswith(b"\r"):
        line = line[:-1]
    try:
        head, p = ped.host_head(line)
        return head + ped.host_tokens(line, n_snp)
    except vcf.VcfFormatError as e:
        return ("error", e.message, e.column, e.cell)


@pytest.mark.parametrize("k", range(len(LINES)))
def test_cells_of_irregular_lines_equal_the_restatement(k):
    want, got = _ref_cells(LINES[k], 2), _pkg_cells(LINES[k], 2)
    assert got == want
    if k == 5:
        assert want[6:] == [b"A", b"", b"G", b"T"]
    if k == 7:
        assert want[6:] == [b"AT", b"G", b"T", b"\""]
    if k in (9, 12, 13, 14):
        assert want[:2] == ("error", "fewer columns than what expected.")
    if k in (10, 11):
        assert want[:2] == ("error", "more columns than what expected.")
    if k == 13:
        assert want[2] == 1
    if k == 9:
        assert want[2:] == (10, b"T")


def test_last_cell_is_what_the_reference_still_holds():
    assert ped.last_cell(b"a b\tC  ") == b"C" and ped.last_cell(b"a\t\"xy\"") == b"xy" and ped.last_cell(b"q") == b"q"
    d = None
    with pytest.raises(R.PedError) as e:
        d = R.parse_ped(b"F i 0 0 1 -9 A G\n\nF j 0 0 1 -9 A G\n", 1)
    assert d is None and (e.value.message, e.value.line, e.value.column, e.value.cell) == ("fewer columns than what expected.", 2, 1, b"G")


def test_pick_alleles_ties_and_orders():
    assert ped.pick_alleles({b"G": 3, b"A": 3}) == (b"A", b"G")
    assert ped.pick_alleles({b"T": 3, b"C": 1}) == (b"T", b"C")
    assert ped.pick_alleles({b"C": 1}) == (b"C", b"0") and ped.pick_alleles({}) == (b"0", b"0")
    assert ped.pick_alleles({b"AT": 2, b"A": 2, b"": 1, b"T": 5}) == (b"T", b",A,AT")


# ---- the MAP order ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chrom,pos", [
    (["2", "1", "1", "10", "1"], [5, 9, 3, 2, 3]),                              # numeric, ties keep the file's order
    (["2", "NA", "1", "NA"], [5, 1, 3, 0]),                                     # numeric with NA: last, then 0
    (["2", "X", "1", "Y", "10", "X", "MT", "1"], [5, 9, 3, 2, 7, 1, 1, 3]),     # mixed labels: integers first, labels as bytes
    (["chr2", "chr10", "chr1", "NA"], [1, 1, 1, 1]),                            # all labels
    (["1.5", "1", "2"], [1, 2, 3]),                                             # numeric, not integer
])
def test_map_order_equals_the_restatement(chrom, pos):
    ii, col = ped.map_order(chrom, pos)
    wi, wc = R.map_order(chrom, pos)
    assert list(ii) == wi
    assert [str(c) for c in col] == [str(int(c)) if isinstance(c, float) else str(c) for c in wc]


def test_map_order_known_answers(tmp_path):
    ii, col = ped.map_order(["2", "X", "1", "Y", "10", "X", "MT", "1"], [5, 9, 3, 2, 7, 1, 1, 3])
    assert list(ii) == [2, 7, 0, 4, 6, 5, 1, 3] and list(col) == ["1", "1", "2", "10", "MT", "X", "X", "Y"]
    ii, col = ped.map_order(["2", "NA", "1", "NA"], [5, 1, 3, 0])
    assert list(ii) == [2, 0, 3, 1] and col.dtype == np.int32 and list(col) == [1, 2, 0, 0]
    fn = str(tmp_path / "m.map")
    with open(fn, "w") as f:
        f.write("2 rsB 0 50\n1\trsA\t0\t70\n\n1 rsC 0.5 60\n")
    m = ped.read_map(fn)
    assert list(m["ii"]) == [2, 1, 0] and list(m["snp_rs_id"]) == ["rsC", "rsA", "rsB"] and list(m["snp_position"]) == [60, 70, 50]
    assert list(m["snp_chromosome"]) == [1, 1, 2]
    with open(fn, "w") as f:
        f.write("2 rsB 0\n")
    with pytest.raises(ValueError, match="four columns"):
        ped.read_map(fn)


# ---- the ABI: refusals that touch no device ---------------------------------------------------------------------------------------------
def _render(**kw):
    a = dict(rows=4096, n_rows=2, n_cols=3, fmt=_lib.TEXT_PED_ALLELE, alleles=list("ACGTAC"), prefixes=[b"x", b"yy"], text=8192)
    a.update(kw)
    return _lib.text_render(a["rows"], a["n_rows"], a["n_cols"], a["fmt"], alleles=a["alleles"], prefixes=a["prefixes"], text=a["text"])


@pytest.mark.parametrize("kw,message", [
    (dict(rows=0), "NULL argument: rows is NULL"),
    (dict(fmt=4), "invalid format"),
    (dict(fmt=-1), "invalid format"),
    (dict(n_cols=0, alleles=None), r"invalid number of columns \(1 ... 2\^30 - 1\)"),
    (dict(n_cols=1 << 30, alleles=None, fmt=0), r"invalid number of columns \(1 ... 2\^30 - 1\)"),
    (dict(n_rows=0, prefixes=None), r"invalid number of rows \(1 ... 2\^31 - 1\)"),
    (dict(alleles=None), "NULL argument: allele_pool is NULL"),
    (dict(alleles=(np.zeros(8, np.uint8), np.array([0, 1, 2, 2, 3, 4, 5], np.int64))), "allele_off is not ascending .*: allele 2"),
    (dict(alleles=(np.zeros(8, np.uint8), np.array([-1, 1, 2, 3, 4, 5, 6], np.int64))), "allele_off is not ascending: a negative offset"),
    (dict(prefixes=(np.zeros(8, np.uint8), np.array([0, 3, 2], np.int64))), "prefix_off is not ascending: row 1"),
])
def test_render_refusals_touch_no_device(kw, message):
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_text_render: " + message):
        _render(**kw)


def test_render_null_host_arrays_and_sizing_without_a_device():
    import ctypes
    L = _lib.lib()
    off = np.zeros(3, np.int64)
    pool, aoff = _lib._pool(list("ACGTAC"))
    args = [ctypes.c_void_p(4096), 2, 3, _lib.TEXT_PED_ALLELE, _lib._ptr(pool), _lib._ptr(aoff), None, None, None, _lib._ptr(off), 0, None]
    for k, name in ((5, "allele_off"), (9, "line_off")):
        a = list(args)
        a[k] = None
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_text_render: NULL argument: %s is NULL" % name):
            _lib.check(L.snpgpu_text_render(*a))
    a = list(args)
    a[6] = _lib._ptr(pool)
    with pytest.raises(_lib.SnpGpuError, match="prefix_pool and prefix_off go together"):
        _lib.check(L.snpgpu_text_render(*a))
    assert L.snpgpu_text_stats(None) != 0 and L.snpgpu_ped_stats(None) != 0
    # fixed-width formats are sized by arithmetic: no device is needed
    assert list(_lib.text_render(4096, 3, 5, _lib.TEXT_DIGIT)) == [0, 6, 12, 18]
    assert list(_lib.text_render(4096, 2, 5, _lib.TEXT_PED_12, prefixes=[b"abc", b""])) == [0, 24, 45]
    assert list(_lib.text_render(4096, 2, 2, _lib.TEXT_PED_ALLELE, alleles=list("ACGT"), prefixes=[b"", b"z"])) == [0, 9, 19]


def _tokens(**kw):
    a = dict(text=4096, n_bytes=7, cell_begin=[0], line_end=[7], n_snp=2, tokens=8192)
    a.update(kw)
    return _lib.ped_tokens(a["text"], a["n_bytes"], a["cell_begin"], a["line_end"], a["n_snp"], a["tokens"])


@pytest.mark.parametrize("kw,message", [
    (dict(text=0), "NULL argument: text is NULL"),
    (dict(tokens=0), "NULL argument: tokens is NULL"),
    (dict(n_bytes=0), "invalid n_bytes"),
    (dict(n_snp=0), r"invalid number of SNPs \(1 ... 2\^30 - 1\)"),
    (dict(n_snp=1 << 30), r"invalid number of SNPs \(1 ... 2\^30 - 1\)"),
    (dict(cell_begin=[], line_end=[]), r"invalid number of lines \(1 ... 2\^31 - 1\)"),
    (dict(line_end=[8]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[-1]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[5], line_end=[4]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
])
def test_ped_tokens_refusals_touch_no_device(kw, message):
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_tokens: " + message):
        _tokens(**kw)


def test_ped_census_and_codes_refusals_touch_no_device():
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_census: NULL argument: tokens is NULL"):
        _lib.ped_census(0, [0], 2, 4096)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_census: NULL argument: table is NULL"):
        _lib.ped_census(4096, [0], 2, 0)
    with pytest.raises(_lib.SnpGpuError, match=r"snpgpu_ped_census: invalid number of lines"):
        _lib.ped_census(4096, [], 2, 4096)
    with pytest.raises(_lib.SnpGpuError, match=r"snpgpu_ped_census: invalid number of SNPs"):
        _lib.ped_census(4096, [0], 0, 4096)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_codes: NULL argument: tokens is NULL"):
        _lib.ped_codes(0, 1, 2, [65, 66], 4096)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_codes: NULL argument: rows is NULL"):
        _lib.ped_codes(4096, 1, 2, [65, 66], 0)
    with pytest.raises(_lib.SnpGpuError, match=r"snpgpu_ped_codes: invalid number of lines"):
        _lib.ped_codes(4096, 0, 2, [65, 66], 4096)
    import ctypes
    L = _lib.lib()
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_codes: NULL argument: ref is NULL"):
        _lib.check(L.snpgpu_ped_codes(ctypes.c_void_p(4096), 1, 2, None, ctypes.c_void_p(4096), 0, None))
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_ped_census: NULL argument: line_flags is NULL"):
        _lib.check(L.snpgpu_ped_census(ctypes.c_void_p(4096), None, 1, 2, ctypes.c_void_p(4096), 0, None))


def test_header_declares_the_calls_and_no_result_memory_kind():
    protos = M.header_prototypes(open(os.path.join(ROOT, "include", "snpgpu.h")).read())
    for f in ("snpgpu_text_render", "snpgpu_text_stats", "snpgpu_ped_tokens", "snpgpu_ped_census", "snpgpu_ped_codes", "snpgpu_ped_stats"):
        assert f in protos and f in _lib.EXPORTS and hasattr(_lib.lib(), f)
        assert not {"out_mem", "dst_mem", "mem"} & set(protos[f])
    assert protos["snpgpu_text_render"][-4:] == ["text", "line_off", "device", "stream"]
    assert _lib.lib().snpgpu_abi_version() == 2
    s, p = _lib.text_stats(), _lib.ped_stats()
    assert s["segment_bytes"] == 16 and s["tile_columns"] == 1024
    assert p["chunk_bytes"] % p["segment_bytes"] == 0 and p["segment_bytes"] == 16 and p["halo_bytes"] >= 16


def test_gds_readers_carry_snp_rs_id():
    from conftest import GOLDEN
    from snprelate_amd import gds
    fn = os.path.join(GOLDEN, "hapmap_geno.gds")
    a, b = gds.open_gds(fn), gds.open_gds_stream(fn)
    assert len(a.snp_rs_id) == a.n_snp and a.snp_rs_id[0] == "rs1695824" and list(a.snp_rs_id) == list(b.snp_rs_id)
    assert gds.GenoFile(genotype=np.zeros((2, 3), np.uint8)).snp_rs_id is None


def test_without_a_device_the_converters_fail_loudly(tmp_path):
    from snprelate_amd.text import device_visible
    if device_visible():
        return                                             # (with a device the GPU tests cover the calls)
    from snprelate_amd import snpgdsGDS2Eigen, snpgdsGDS2PED, snpgdsOpenPED
    from snprelate_amd.gds import GenoFile
    g = GenoFile(genotype=np.zeros((2, 3), np.uint8), snp_position=[1, 2], snp_allele=["A/C", "G/T"])
    for f in (snpgdsGDS2PED, snpgdsGDS2Eigen):
        with pytest.raises(_lib.SnpGpuError, match="no HIP device"):
            f(g, str(tmp_path / "x"), verbose=False)
    fn = str(tmp_path / "p")
    open(fn + ".map", "w").write("1 a 0 1\n")
    open(fn + ".ped", "w").write("F i 0 0 1 -9 A A\n")
    with pytest.raises(_lib.SnpGpuError, match="no HIP device"):
        snpgdsOpenPED(fn + ".ped", fn + ".map", verbose=False)
