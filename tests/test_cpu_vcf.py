"""CPU tests of the VCF layer: the restatement (tests/vcf_ref.py) against known answers of the reference's loop, snpgpu_vcf_index
against Python's split, the refusals of snpgpu_vcf_genotypes (all before any device is touched), and what snprelate_amd/vcf.py does
on the host -- header, metadata rules, ref_allele, the re-parse of flagged lines -- against the restatement.  None needs a device."""
import gzip
import math
import os

import numpy as np
import pytest

import mem_kinds as M
import vcf_cases as C
import vcf_ref as R
from conftest import GOLDEN, ROOT
from snprelate_amd import _lib, api, vcf

SEQ = os.path.join(GOLDEN, "sequence.vcf")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,num_allele,want", [
    ("10/0", 11, 1), ("0/10", 11, 1), ("0|0", 2, 2), ("./.", 2, 3), (".", 2, 3), (".|1", 2, 3), ("1|.", 2, 3), ("0", 2, 1), ("1", 2, 0),
    ("", 2, 0), (":35", 2, 0), ("0/0/0", 2, 2), ("0/0/1", 2, 2), ("0/1/1", 2, 1), (" 0/1", 2, 1), ("0x/1", 2, 1), ("+0/1", 2, 1),
    ("0/", 2, 1)])
def test_restatement_known_answers(cell, num_allele, want):
    assert R.cell_code(cell, num_allele) == want
    assert vcf.gt_code(cell.encode(), num_allele, 0) == want


@pytest.mark.parametrize("cell,message", [
    ("/0", 'Invalid integer conversion "/0".'), ("0//0", 'Invalid integer conversion "/0".'),
    ("2/0", 'Genotype code is out of range "2/0".'), ("-1/0", 'Genotype code should be non-negative "-1/0".')])
def test_restatement_known_errors(cell, message):
    with pytest.raises(R.RefError) as e:
        R.cell_code(cell, 2)
    assert e.value.message == message
    with pytest.raises(vcf.VcfFormatError) as e:
        vcf.gt_code(cell.encode(), 2, 0)
    assert e.value.message == message


def test_sequence_vcf_through_the_restatement():
    text = open(SEQ).read()
    d = R.parse_vcf(text, "biallelic.only")
    assert d["sample_id"] == ["NA00001", "NA00002", "NA00003"]
    assert d["geno"] == [[2, 1, 0], [2, 1, 2]] and d["snp_id"] == [1, 2] and d["pos"] == [14370, 17330]
    assert d["rs"] == ["rs6054257", ""] and d["allele"] == ["G/A", "T/A"] and d["qual"] == [29.0, 3.0]
    assert d["filter"] == ["PASS", "q10"] and d["chrom"] == ["20", "20"]
    d = R.parse_vcf(text, "copy.num.of.ref")
    assert d["geno"] == [[2, 1, 0], [2, 1, 2], [0, 0, 0], [2, 2, 2], [1, 1, 0]] and d["snp_id"] == [1, 2, 3, 4, 5]
    assert d["allele"] == ["G/A", "T/A", "A/G,T", "T/.", "GTC/G,GTCT"]


# ---- snpgpu_vcf_index --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lines():
    codes = np.random.default_rng(5).integers(0, 4, (23, 11))
    fixed, cells, na = C.make_lines(codes, seed=5, id_lens=list(range(0, 17)))
    return codes, fixed, cells, na


@pytest.mark.parametrize("newline,final_newline", [("\n", True), ("\r\n", True), ("\n", False), ("\r\n", False)])
def test_index_equals_split(lines, newline, final_newline):
    _, fixed, cells, _ = lines
    data = C.join_lines(fixed, cells, newline, final_newline).encode()
    col, end, used = _lib.vcf_index(data)
    wcol, wend = C.python_index(data)
    assert used == len(data) and np.array_equal(col, wcol) and np.array_equal(end, wend)
    for i in (0, 7, 22):
        assert data[col[i, 9]:end[i]].decode() == "\t".join(cells[i])


def test_index_of_a_cut_buffer(lines):
    _, fixed, cells, _ = lines
    data = C.join_lines(fixed, cells).encode()
    wcol, wend = C.python_index(data)
    starts = list(wcol[:, 0]) + [len(data)]
    for cut in (0, 1, int(wend[0]), int(wend[0]) + 1, int(wcol[5, 9]) + 3, len(data) - 1, len(data)):
        col, end, used = _lib.vcf_index(data[:cut], final=False)
        whole = max(i for i, s in enumerate(starts) if s <= cut)             # lines that end with their '\n' inside the cut
        assert used == starts[whole] and len(col) == whole
        assert np.array_equal(col, wcol[:whole]) and np.array_equal(end, wend[:whole])
    # the rest of the buffer, given as final, completes the index
    col, end, used = _lib.vcf_index(data[starts[5]:], final=True, line_base=5)
    assert np.array_equal(col + starts[5], wcol[5:]) and np.array_equal(end + starts[5], wend[5:])


def test_index_refusals(lines):
    _, fixed, cells, _ = lines
    data = C.join_lines(fixed, cells).encode()
    with pytest.raises(_lib.SnpGpuError, match=r"line 103 has 9 columns"):
        _lib.vcf_index(b"\t".join([b"x"] * 10) + b"\n" + b"\t".join([b"x"] * 10) + b"\n" + b"\t".join([b"x"] * 9) + b"\n", line_base=100)
    with pytest.raises(_lib.SnpGpuError, match=r"line 2 is empty"):
        _lib.vcf_index(b"\t".join([b"x"] * 10) + b"\n\n")
    with pytest.raises(_lib.SnpGpuError, match=r"line 2 is empty"):
        _lib.vcf_index(b"\t".join([b"x"] * 10) + b"\r\n\r\n")
    with pytest.raises(_lib.SnpGpuError, match=r"line 4: more lines than max_lines = 3"):
        _lib.vcf_index(data, max_lines=3)
    col, end, used = _lib.vcf_index(b"\t".join([b"x"] * 9) + b"\t")           # ten columns, the last one empty: the kernel's to flag
    assert len(col) == 1 and col[0, 9] == end[0] == 18


# ---- snpgpu_vcf_genotypes: refused before any device is touched -------------------------------------------------------------------------
def _call(**kw):
    a = dict(text=b"0|1\t1|1", cell_begin=[0], line_end=[7], num_allele=[2], ref_index=[0], n_samp=2, rows=4096, text_mem=None,
             n_bytes=None)
    a.update(kw)
    return _lib.vcf_genotypes(a["text"], a["cell_begin"], a["line_end"], a["num_allele"], a["ref_index"], a["n_samp"], a["rows"],
                              n_bytes=a["n_bytes"], text_mem=a["text_mem"])


@pytest.mark.parametrize("kw,message", [
    (dict(rows=0), "NULL argument: rows is NULL"),
    (dict(text=0, n_bytes=7), "NULL argument: text is NULL"),
    (dict(text_mem=7), "invalid text_mem"),
    (dict(n_samp=0), r"invalid number of samples \(1 ... 2\^30 - 1\)"),
    (dict(n_samp=1 << 30), r"invalid number of samples \(1 ... 2\^30 - 1\)"),
    (dict(line_end=[8]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[-1]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[5], line_end=[4]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(num_allele=[0]), "invalid num_allele: line 0"),
    (dict(ref_index=[-2]), "invalid ref_index: line 0"),
    (dict(cell_begin=[], line_end=[], num_allele=[], ref_index=[]), "invalid number of lines"),
])
def test_genotypes_refusals_touch_no_device(kw, message):
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_vcf_genotypes: " + message):
        _call(**kw)


def test_genotypes_null_host_arrays():
    import ctypes
    L = _lib.lib()
    one64, one32 = np.zeros(1, np.int64), np.ones(1, np.int32)
    text = np.frombuffer(b"0|1", np.uint8)
    args = [_lib._ptr(text), _lib.HOST, 3, _lib._ptr(one64), _lib._ptr(np.full(1, 3, np.int64)), _lib._ptr(one32), _lib._ptr(one32), 1, 1,
            ctypes.c_void_p(4096), _lib._ptr(np.zeros(1, np.int32)), _lib._ptr(one64.copy()), 0, None]
    for k, name in ((3, "cell_begin"), (4, "line_end"), (5, "num_allele"), (6, "ref_index"), (10, "line_flags"), (11, "line_cells")):
        a = list(args)
        a[k] = None
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_vcf_genotypes: NULL argument: %s is NULL" % name):
            _lib.check(L.snpgpu_vcf_genotypes(*a))
    assert L.snpgpu_vcf_stats(None) != 0


def test_header_declares_the_calls_and_no_result_memory_kind():
    protos = M.header_prototypes(open(os.path.join(ROOT, "include", "snpgpu.h")).read())
    for f in ("snpgpu_vcf_index", "snpgpu_vcf_genotypes", "snpgpu_vcf_stats"):
        assert f in protos and f in _lib.EXPORTS and hasattr(_lib.lib(), f)
        assert not {"out_mem", "dst_mem", "mem"} & set(protos[f])
    assert "text_mem" in protos["snpgpu_vcf_genotypes"]
    s = _lib.vcf_stats()
    assert s["chunk_bytes"] % s["segment_bytes"] == 0 and s["segment_bytes"] == 16 and s["halo_bytes"] >= 16


# ---- the reader on the host ----------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, text, gz=False):
    fn = str(tmp_path / name)
    with (gzip.open(fn, "wb") if gz else open(fn, "wb")) as f:
        f.write(text.encode())
    return fn


def _scan(reader):
    """run the reader's host side alone: the kept lines' cell texts, and the nodes on the reader"""
    out = []
    for buf, n, kept in reader.chunks():
        for b, e in zip(kept["cell_begin"], kept["line_end"]):
            out.append(bytes(buf[b:e]).decode())
    return out


def _same_nodes(r, d):
    assert list(r.snp_id) == d["snp_id"] and list(r.snp_chromosome) == d["chrom"] and list(r.snp_position) == d["pos"]
    assert list(r.snp_rs_id) == d["rs"] and list(r.snp_allele) == d["allele"] and list(r.snp_annot["filter"]) == d["filter"]
    q = np.array(d["qual"], np.float32)
    assert r.snp_annot["qual"].dtype == np.float32 and np.array_equal(r.snp_annot["qual"], q, equal_nan=True)
    assert r.next_snp_id == d["next_id"] and r.lines_seen == d["lines"]


@pytest.mark.parametrize("method", ["biallelic.only", "copy.num.of.ref"])
@pytest.mark.parametrize("gz", [False, True])
def test_reader_metadata_of_sequence_vcf(tmp_path, method, gz):
    text = open(SEQ).read()
    fn = _write(tmp_path, "s.vcf.gz" if gz else "s.vcf", text, gz)
    r = vcf.VcfReader(fn, method=method)
    assert list(r.sample_id) == ["NA00001", "NA00002", "NA00003"]
    cells = _scan(r)
    d = R.parse_vcf(text, method)
    _same_nodes(r, d)
    assert [R.line_codes(c, 3, 3) for c in cells] == d["geno"]
    with pytest.raises(ValueError, match="goes through its file once"):
        next(r.chunks())


def test_reader_metadata_rules_small_chunks_and_crlf(tmp_path):
    """chunks far smaller than the file, CRLF, prefixes, '.' columns, multi-allelic ALT: the nodes equal the restatement's"""
    codes = np.random.default_rng(2).integers(0, 4, (60, 5))
    fixed, cells, na = C.make_lines(codes, seed=2, id_lens=[0, 4, 9], num_allele=[2 if i % 7 == 0 else 1 + i % 5 + 2 for i in range(60)])
    for i, f in enumerate(fixed):
        f[0] = ["chr1", "CHR2", "chX", "22", "Chr", "ch"][i % 6]
        f[5] = [".", "1e3", " 7.5", "0.25", "3"][i % 5]
        if i % 14 == 0:
            f[3], f[4] = "g", "t"
    text = C.vcf_text(fixed, cells, newline="\r\n", final_newline=False)
    fn = _write(tmp_path, "m.vcf", text)
    for method in vcf.VcfReader.METHODS:
        r = vcf.VcfReader(fn, method=method, chunk_bytes=700, snp_id_start=11, line_start=4)
        got = _scan(r)
        d = R.parse_vcf(text, method, first_id=11, first_line=4)
        _same_nodes(r, d)
        assert len(got) == len(d["geno"]) > 5
    assert math.isnan(d["qual"][0]) and d["chrom"][:6] == ["1", "2", "chX", "22", "", "ch"]
    with pytest.raises(ValueError, match="a line longer than the 64 bytes of a chunk"):
        _scan(vcf.VcfReader(fn, method="copy.num.of.ref", chunk_bytes=64))


def test_reader_ref_allele(tmp_path):
    text = open(SEQ).read()
    fn = _write(tmp_path, "s.vcf", text)
    ref = ["A", None, "T", "C", "GTCT"]            # ALT of line 1, keep, second ALT of line 3, absent from line 4, second ALT of line 5
    r = vcf.VcfReader(fn, method="copy.num.of.ref", ref_allele=ref)
    idx = []
    for _, _, kept in r.chunks():
        idx += list(kept["ref_index"])
    d = R.parse_vcf(text, "copy.num.of.ref", ref_allele=ref)
    _same_nodes(r, d)
    assert idx == [1, 0, 2, -1, 2] and d["allele"] == ["A/G", "T/A", "T/A,G", "C/T,.", "GTCT/GTC,G"]
    # indexed by the global line count: with biallelic.only the third entry is still line 3's
    r = vcf.VcfReader(fn, method="biallelic.only", ref_allele=ref)
    _scan(r)
    _same_nodes(r, R.parse_vcf(text, "biallelic.only", ref_allele=ref))
    with pytest.raises(ValueError, match=r"'ref.allele' has fewer alleles than what expected.\nFILE: .*s.vcf\nLINE: 22\n"):
        _scan(vcf.VcfReader(fn, method="copy.num.of.ref", ref_allele=["G", "T"]))


def test_header_errors_and_sample_ids(tmp_path):
    with pytest.raises(ValueError, match="Error VCF format: invalid sample id!"):
        vcf.VcfReader(_write(tmp_path, "a.vcf", "##x\n1\t2\t3\n"))
    with pytest.raises(ValueError, match="No sample in the VCF file!"):
        vcf.VcfReader(_write(tmp_path, "b.vcf", "##x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\n"))
    with pytest.raises(ValueError, match="'method' should be one of"):
        vcf.VcfReader(SEQ, method="all")
    other = _write(tmp_path, "c.vcf", open(SEQ).read().replace("NA00003", "NA00004"))
    with pytest.raises(ValueError, match="'%s' has different sample id." % other.replace("\\", "\\\\")):
        api.snpgdsOpenVCF([SEQ, other], verbose=False)
    with pytest.raises(TypeError):
        api.snpgdsOpenVCF(5)
    with pytest.raises(ValueError, match="should be one of"):
        api.snpgdsOpenVCF(SEQ, method="x")


def test_fixed_column_errors_carry_file_and_line(tmp_path):
    text = open(SEQ).read()
    fn = _write(tmp_path, "p.vcf", text.replace("\t17330\t", "\t17k\t"))
    with pytest.raises(ValueError, match=r'Invalid integer conversion "k".\nFILE: .*p.vcf\nLINE: 21, COLUMN: 5, '):
        _scan(vcf.VcfReader(fn))
    with pytest.raises(R.RefError) as e:
        R.parse_vcf(text.replace("\t17330\t", "\t17k\t"))
    assert (e.value.message, e.value.line, e.value.column) == ('Invalid integer conversion "k".', 21, 5)
    # a skipped line is still walked: a multi-allelic line with a cell too many fails under biallelic.only as well
    bad = text.replace("2/2:35:4\n", "2/2:35:4\t0/0\n")
    fn = _write(tmp_path, "q.vcf", bad)
    with pytest.raises(ValueError, match=r"more columns than what expected.\nFILE: .*q.vcf\nLINE: 22, COLUMN: 12, "):
        _scan(vcf.VcfReader(fn))
    with pytest.raises(R.RefError) as e:
        R.parse_vcf(bad)
    assert (e.value.message, e.value.line, e.value.column) == ("more columns than what expected.", 22, 12)


IRREGULAR = [" 0/1", "+0/1", "\"0|1\"", "'1/1'", "0/ 0", "0000000000/1", "00000000001|0", "0|1\"", "0/-0x", "4294967296/0"]
ERRORS = ["\"", "/0", "0//0", "2/0", "-1/0", "x", "\"0|1\":3", "99999999999999999999/0", "4294967298/0"]


def test_host_cells_equals_the_restatement_on_irregular_cells():
    """the host path of flagged lines: values where the reference accepts, its message and column where it does not"""
    for k, cell in enumerate(IRREGULAR + ERRORS):
        cells = ["0|0", "1/1:5", cell, "./.", "0/1"]
        text = "\t".join(cells)
        try:
            want = R.line_codes(text, 5, 2)
        except R.RefError as e:
            assert cell in ERRORS
            with pytest.raises(vcf.VcfFormatError) as g:
                vcf.host_cells(text.encode(), 5, 2, 0)
            assert (g.value.message, g.value.column) == (e.message, 12) and g.value.column == e.column
            continue
        assert cell in IRREGULAR
        assert list(vcf.host_cells(text.encode(), 5, 2, 0)) == want
    for text, n, msg, column in (("0|0\t0|1", 3, "fewer columns than what expected.", 12), ("0|0\t0|1\t", 3, "fewer", 12),
                                 ("0|0\t0|1\t1|1\t0|0", 3, "more columns than what expected.", 12), ("", 1, "fewer", 10)):
        with pytest.raises(vcf.VcfFormatError, match=msg) as g:
            vcf.host_cells(text.encode(), n, 2, 0)
        with pytest.raises(R.RefError, match=msg) as e:
            R.line_codes(text, n, 2)
        assert g.value.column == e.value.column == column


def test_no_device_no_fallback():
    try:
        n = _lib.device_count()
    except _lib.SnpGpuError:
        n = 0
    if n > 0:
        return                                                               # with a device the GPU tests cover the call
    with pytest.raises(_lib.SnpGpuError):
        api.snpgdsOpenVCF(SEQ, verbose=False)
    with pytest.raises(_lib.SnpGpuError):
        next(vcf.VcfReader(SEQ).blocks(16))
