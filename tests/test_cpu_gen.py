"""Oxford GEN without a GPU: the restatement of the reference's reader (tests/gen_ref.py) pinned against literals worked by hand from
src/ConvToGDS.cpp, snpgpu_gen_line_host against the restatement, the sample file and the leading columns as snprelate_amd.gen reads
them, and the kernel's rounding rule, restated in Python, against the C library's strtof."""
import os

import numpy as np
import pytest

import gen_ref as G
from snprelate_amd import _lib, gen
from snprelate_amd.vcf import VcfFormatError

HEAD = b"snp1 rs1 100 A G "


def codes_of(cells, n_samp, thr=0.9):
    return list(G.parse_line(HEAD + cells, n_samp, thr)[1])


# ---- the restatement against the reference's code, by hand ------------------------------------------------------------------------------
def test_threshold_is_compared_with_the_float():
    # strtof("0.9") = 0.89999997615814208984375 < 0.9 (the double); strtof("0.90000001") = 0.900000035762786865234375
    assert G.strtof(b"0.9")[0] == 0.89999997615814208984375
    assert G.strtof(b"0.90000001")[0] == 0.900000035762786865234375
    assert codes_of(b"0.9 0 0", 1) == [3]
    assert codes_of(b"0.90000001 0 0", 1) == [2]
    assert codes_of(b"0.9 0 0", 1, thr=0.89999997615814208984375) == [2]


@pytest.mark.parametrize("cells, code", [
    (b"1 0 0", 2), (b"0.5 0.3 0.2", 3),                    # AA >= AB, AA >= BB
    (b"0.05 0 0.95", 0), (b"0.3 0.2 0.5", 3),              # AA >= AB, AA < BB: the branch that never looks at AB again
    (b"0 1 0", 1), (b"0.2 0.5 0.3", 3),                    # AA < AB, AB >= BB
    (b"0 0.05 0.95", 0), (b"0.1 0.4 0.5", 3),              # AA < AB, AB < BB
    (b"0.95 0.95 0", 2),                                   # AA = AB: >= takes AA
    (b"0 0.95 0.95", 1),                                   # AB = BB: >= takes AB
    (b"0.95 0 0.95", 2),                                   # AA = BB: >= takes AA
    (b"0.95 0.95 0.95", 2), (b"0 0 0", 3),                 # all equal
])
def test_every_leaf_of_the_tree(cells, code):
    assert codes_of(cells, 1) == [code]
    assert list(_lib.gen_line_host(cells, 1, 0.9)[0]) == [code]


@pytest.mark.parametrize("cells, code", [
    (b". 0 0.95", 0),                                      # NaN >= 0 false -> else: AB = 0 >= BB false -> BB
    (b". 0.95 0", 1),                                      # else: AB >= BB
    (b"0.95 . 0", 3),                                      # AA >= NaN false; NaN >= BB false; BB = 0 < thr
    (b"0 . 0.95", 0),
    (b"0.95 0 .", 3),                                      # AA >= AB; AA >= NaN false -> the leaf (BB >= thr) ? 0 : 3 with BB = NaN
    (b". . .", 3),
])
def test_dot_is_nan_in_each_position(cells, code):
    assert codes_of(cells, 1) == [code]
    assert list(_lib.gen_line_host(cells, 1, 0.9)[0]) == [code]


@pytest.mark.parametrize("line, message, column, cell", [
    (HEAD + b"1 0 0 NA 0 0", 'Invalid float conversion "NA".', 9, b"NA"),
    (HEAD + b"1 0 0 0.5x 0 0", 'Invalid float conversion "x".', 9, b"0.5x"),
    (HEAD + b"1 0 0 1\t\t0 0", 'Invalid float conversion "".', 10, b""),          # an empty cell between two tabs
    (HEAD + b"1 0 0 1 0", "fewer columns than what expected.", 11, b"0"),
    (HEAD + b"1 0 0 1 0 0 1", "more columns than what expected.", 11, b"0"),
    (HEAD + b"1 0 0 1 0 0\t", "more columns than what expected.", 11, b"0"),
    (b"snp1 rs1 100 A G", "fewer columns than what expected.", 6, b"100"),        # the alleles are not read into `cell`
    (b"snp1 rs1 100 A", "fewer columns than what expected.", 5, b"100"),
    (b"snp1 rs1 1x0 A G 1 0 0 1 0 0", 'Invalid integer conversion "x0".', 3, b"1x0"),
    (b"", "fewer columns than what expected.", 1, b"prev"),
    (HEAD + b"1 0 0 123456789012345678901234567890x 0 0", 'Invalid float conversion "x".', 9, b"123456789012345678901234567890x"),
    (HEAD + b"1 0 0 abcdefghijklmnopqrstuvwxyz 0 0", 'Invalid float conversion "abcdefghijklmnop...".', 9, b"abcdefghijklmnopqrstuvwxyz"),
])
def test_exact_messages(line, message, column, cell):
    with pytest.raises(G.GenError) as e:
        G.parse_line(line, 2, 0.9, b"prev")
    assert (e.value.message, e.value.column, e.value.cell) == (message, column, cell)


def test_accepted_oddities():
    assert codes_of(b"1 0 0\r", 1) == [2]                  # isspace bytes after the number are skipped
    assert codes_of(b"1 0 0   ", 1) == [2]                 # spaces behind the last column
    assert codes_of(b"\"1\" '0' 0", 1) == [2]              # matching quotes are dropped
    assert codes_of(b"1e0 0 0 9.5E-1 0 0 +1 -0 0 inf 0 0 0x1p0 0 0", 5) == [2, 2, 2, 2, 2]
    assert codes_of(b"nan 0 0.95 .x 0 0.95", 2) == [0, 0]  # ".x": nothing converts and the cell starts with '.': NaN, no error
    assert codes_of(b"1   0\t0", 1) == [2]                 # a run of spaces is one separator, a tab is one
    with pytest.raises(G.GenError, match="more columns"):   # a tab beside a space: "0", "", "0" are one cell more than the line has
        codes_of(b"1 0 \t0", 1)


def test_parse_text_formats_errors_as_the_reference():
    text = HEAD + b"1 0 0 0 1 0\n" + HEAD + b"1 0 0 NA 0 0\n"
    with pytest.raises(ValueError) as e:
        G.parse_text(text, 2, path="a.gen")
    assert str(e.value) == 'Invalid float conversion "NA".\nFILE: a.gen\nLINE: 2, COLUMN: 9, NA\n'
    heads, codes = G.parse_text(text[:text.index(b"\n") + 1], 2)
    assert heads == [("snp1", "rs1", 100, "A/G")] and codes.tolist() == [[2, 1]]
    assert G.pack_rows(codes).tolist() == [[0x06]]


# ---- snpgpu_gen_line_host against the restatement -------------------------------------------------------------------------------------------
_ODD = ["1e-3", "9E-1", "9.5e-1", "+0.95", "-0", "-1", "inf", "nan", "NaN", "Infinity", "0x1p-1", "0x1.ep-1", "\"1\"", "'0.95'", "\"1", ".",
        "NA", "0.5x", "1..", "..", "1e", "e1", "0.95\r", "\r1", "\v1", "1\f", "0." + "9" * 20, "0." + "0" * 22 + "1", "9" * 40,
        "1" + "0" * 70, "0.123456789012345678", "x", "\"\"", "''", "0.9", "0.90000001"]


def _random_line(rng, n_samp):
    """the cells of a line from its sixth column on: mostly fast-grammar tokens, some odd ones, sometimes broken"""
    toks = []
    for _ in range(3 * n_samp):
        u = rng.random()
        toks.append(_ODD[int(rng.integers(len(_ODD)))] if u < 0.15 else G.token(rng, G.FORMS[int(rng.integers(len(G.FORMS)))]))
    seps = []
    for _ in range(len(toks) - 1):
        u = rng.random()
        seps.append(" " if u < 0.6 else "\t" if u < 0.8 else "  " if u < 0.95 else ["\t\t", " \t", "\t "][int(rng.integers(3))])
    line = "".join(t + s for t, s in zip(toks, seps + [""]))
    u = rng.random()
    if u < 0.05:
        line += " 1"                                       # more cells
    elif u < 0.10:
        line = line[:line.rfind(" ")] if " " in line else ""                                  # fewer
    elif u < 0.15:
        line += ["  ", "\t", " \t", "\r"][int(rng.integers(4))]
    elif u < 0.17:
        line = "\t" + line                                 # a separator first: the sixth column is empty
    return line.encode("latin1")


def test_line_host_equals_the_restatement():
    rng = np.random.default_rng(20)
    n_ok = n_err = 0
    for it in range(3000):
        n_samp = int(rng.integers(1, 7))
        thr = [0.9, 0.5, 0.95][it % 3]
        cells = _random_line(rng, n_samp)
        got = _lib.gen_line_host(cells, n_samp, thr)
        try:
            _, want, _ = G.parse_line(HEAD + cells, n_samp, thr)
        except G.GenError as err:
            assert got[0] is None and (got[2], got[1] + 5) == (err.message, err.column), (cells, got, err.message, err.column)
            full = HEAD + cells
            assert gen.error_cell(full, err.column, err.message, b"t") == err.cell, (cells, err.message, err.column)
            n_err += 1
            continue
        assert got[1] == 0 and np.array_equal(got[0], want), (cells, got, want)
        n_ok += 1
    assert n_ok > 500 and n_err > 500, (n_ok, n_err)


def test_line_host_stops_at_a_nul_and_refuses_bad_arguments():
    assert _lib.gen_line_host(b"1 0 0\x00 junk", 1, 0.9)[1] == 0
    got = _lib.gen_line_host(b"1 0\x000", 1, 0.9)
    assert got[1:] == (3, "fewer columns than what expected.")
    with pytest.raises(_lib.SnpGpuError, match="invalid number of samples"):
        _lib.gen_line_host(b"1 0 0", 0, 0.9)
    L = _lib.lib()
    assert L.snpgpu_gen_line_host(None, 0, 1, 0.9, None, None, None, 0) != 0
    assert "line is NULL" in L.snpgpu_last_error().decode()
    with pytest.raises(_lib.SnpGpuError, match="stats is NULL"):
        _lib.check(L.snpgpu_gen_stats(None))


# ---- the host side of snprelate_amd.gen ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [">=2.0", "<=1.1.5"])
def test_sample_file_versions(tmp_path, version):
    ids = ["s%d" % i for i in range(5)]
    fn = str(tmp_path / "x.sample")
    G.write_sample(fn, ids, version, extra=dict(pheno=[1.5, 2, "NA", 4, 5], sex=list("MFMFM")))
    sid, annot = gen.read_sample(fn, version)
    names, rows = G.read_sample(fn, version)
    assert list(sid) == ids == [r[0] for r in rows]
    assert list(annot) == names == ["ID_1", "ID_2", "missing", "pheno", "sex"]
    for j, name in enumerate(names):
        assert annot[name].dtype.kind == "U" and list(annot[name]) == [r[j] for r in rows]
    # the other version reads one line more or less
    other = "<=1.1.5" if version == ">=2.0" else ">=2.0"
    assert len(gen.read_sample(fn, other)[0]) == (6 if version == ">=2.0" else 4)
    with pytest.raises(ValueError):
        gen.read_sample(fn, "3")


def test_leading_columns_on_the_host():
    cells, p = gen.host_head(b"snp7\t\"rs7\"  12345 A\tGT 1 0 0")
    assert cells == (b"snp7", b"rs7", 12345, b"A", b"GT") and p == len(b"snp7\t\"rs7\"  12345 A\tGT ")
    assert gen.host_head(b"s\t\t.\tA\tG\t1")[0] == (b"s", b"", G.NA_INTEGER, b"A", b"G")        # an empty rs id; '.' is NA
    for line in (b"snp1 rs1 1x0 A G 1 0 0", b"snp1 rs1 99999999999 A G 1 0 0", b"snp1 rs1 pos A G", b"snp1 rs1 100 A", b"snp1 rs1 100", b"snp1", b""):
        with pytest.raises(VcfFormatError) as e:
            gen.host_head(line)
        with pytest.raises(G.GenError) as w:
            G.parse_line(line, 1, 0.9, b"")
        assert (e.value.message, e.value.column) == (w.value.message, w.value.column), line
        if w.value.column > 1:
            assert e.value.cell == w.value.cell, line


def test_open_gen_checks_its_arguments_before_any_device(tmp_path):
    from snprelate_amd import snpgdsOpenGEN
    with pytest.raises(ValueError, match="Please specify the argument 'chr.code', e.g., 'chr.code=1'."):
        snpgdsOpenGEN("a.gen", "a.sample")
    with pytest.raises(ValueError, match=r"length\(gen.fn\) == length\(chr.code\) is not TRUE"):
        snpgdsOpenGEN(["a.gen", "b.gen"], "a.sample", chr_code=[1])
    with pytest.raises(TypeError):
        snpgdsOpenGEN(["a.gen", "b.gen"], "a.sample", chr_code=[1, "X"])
    with pytest.raises(ValueError, match="should be one of"):
        snpgdsOpenGEN("a.gen", "a.sample", chr_code=1, version="2")
    with pytest.raises(TypeError):
        snpgdsOpenGEN("a.gen", "a.sample", chr_code=1, call_threshold=float("nan"))


# ---- the rounding rule of DESIGN section 28, executable ---------------------------------------------------------------------------------------
def test_rounding_rule_on_the_midpoint_strings():
    for s in G.MIDPOINTS:
        a = G.strtof(s.encode())[0]
        assert G.round_rule(s.encode()) == a, s
    # the first two are the cases the rule exists for: rounding the double once more goes the other way
    for s in G.MIDPOINTS[:2]:
        assert G.float_of_double(G.strtod(s.encode())[0]) != G.strtof(s.encode())[0], s
    assert G.strtof(b"16777217")[0] == 16777216.0           # a true tie above 2^24: to the even float
    more = G.double_rounding_cases(np.random.default_rng(5), 200)
    assert len(more) == 200
    for s in more:
        assert G.round_rule(s.encode()) == G.strtof(s.encode())[0], s


def test_rounding_rule_on_random_strings():
    rng = np.random.default_rng(6)
    n = 0
    for it in range(60000):
        nd, k = int(rng.integers(1, 16)), int(rng.integers(0, 23))
        digs = "".join(str(int(x)) for x in rng.integers(0, 10, nd))
        s = "0." + "0" * (k - nd) + digs if k >= nd else digs if k == 0 else digs[:nd - k] + "." + digs[nd - k:]
        if it % 7 == 0:
            s = "00" + s
        r = G.round_rule(s.encode())
        assert r is not None, s
        assert r == G.strtof(s.encode())[0], s
        n += 1
    # floats and their midpoints written out exactly are ties and near-ties by construction
    for it in range(5000):
        f = np.float32(rng.random())
        mid = (float(f) + float(np.nextafter(f, np.float32(2)))) / 2
        for s in ("%.15f" % mid, "%.14f" % mid, "%.15f" % float(f), "%.9f" % float(f)):
            assert G.round_rule(s.encode()) == G.strtof(s.encode())[0], s
    for s, why in ((b"0.1234567890123456", "16 significant digits"), (b"0." + b"0" * 22 + b"1", "k = 23"), (b"1e5", "an exponent"),
                   (b".", "no digit"), (b"-1", "a sign")):
        assert G.round_rule(s) is None, why
    assert G.round_rule(b"0.0000000000000000000001") == G.strtof(b"1e-22")[0]
    assert G.round_rule(b"000.000") == 0.0 and G.round_rule(b"1.") == 1.0 and G.round_rule(b".5") == 0.5


def test_predicted_flags_of_the_grammar():
    P = G.predict_flags
    assert P(b"1 0 0 0.5 .5 1.", 2) == (0, 6)
    assert P(b"1  0\t0", 1) == (0, 3)
    assert P(b"1 0 0  ", 1) == (0, 3)                      # spaces behind the last cell
    assert P(b"1 0 0\t", 1)[0] == G.FLAG_EMPTY
    assert P(b" 1 0 0", 1)[0] == G.FLAG_EMPTY
    assert P(b"1 \t0 0", 1)[0] == G.FLAG_EMPTY and P(b"1\t 0 0", 1)[0] == G.FLAG_EMPTY and P(b"1\t\t0 0", 1)[0] == G.FLAG_EMPTY
    assert P(b"1e-3 0 0", 1)[0] == G.FLAG_BYTE and P(b"1 0 0\r", 1)[0] == G.FLAG_BYTE and P(b"1.2.3 0 0", 1)[0] == G.FLAG_BYTE
    assert P(b". 0 0", 1)[0] == G.FLAG_DOT
    assert P(b"0.1234567890123456 0 0", 1)[0] == G.FLAG_DIGITS and P(b"0.00000000000000000000001 0 0", 1)[0] == G.FLAG_DIGITS
    assert P(b"0.123456789012345 0.0000000000000000000001 0", 1)[0] == 0
    assert P(b"0" * 65 + b" 0 0", 1)[0] == G.FLAG_LONG and P(b"0" * 64 + b" 0 0", 1)[0] == 0
    assert P(b"1 0", 1) == (G.FLAG_COUNT, 2) and P(b"1 0 0 1", 1) == (G.FLAG_COUNT, 4) and P(b"", 1) == (G.FLAG_COUNT, 0)


def test_exports_and_constants():
    assert {"snpgpu_gen_genotypes", "snpgpu_gen_line_host", "snpgpu_gen_stats"} <= set(_lib.EXPORTS)
    assert (_lib.GEN_FLAG_BYTE, _lib.GEN_FLAG_DOT, _lib.GEN_FLAG_DIGITS, _lib.GEN_FLAG_LONG, _lib.GEN_FLAG_EMPTY, _lib.GEN_FLAG_COUNT) == \
        (G.FLAG_BYTE, G.FLAG_DOT, G.FLAG_DIGITS, G.FLAG_LONG, G.FLAG_EMPTY, G.FLAG_COUNT)
    assert os.path.exists(os.path.join(os.path.dirname(gen.__file__), "csrc", "kernels_gen.hip"))
    row = gen.pack_row(np.array([2, 1, 0, 3, 1], np.uint8))
    assert row.tolist() == [0xC6, 0x01] and np.array_equal(row, G.pack_rows(np.array([[2, 1, 0, 3, 1]], np.uint8))[0])


# ---- snpgpu_gen_genotypes: refused before any device is touched -------------------------------------------------------------------------
def _call(**kw):
    a = dict(text=b"1 0 0 0 1 0", cell_begin=[0], line_end=[11], n_samp=2, thr=0.9, rows=4096, text_mem=None, n_bytes=None)
    a.update(kw)
    return _lib.gen_genotypes(a["text"], a["cell_begin"], a["line_end"], a["n_samp"], a["thr"], a["rows"], n_bytes=a["n_bytes"],
                              text_mem=a["text_mem"])


REFUSALS = [
    (dict(rows=0), "NULL argument: rows is NULL"),
    (dict(text=0, n_bytes=11), "NULL argument: text is NULL"),
    (dict(text_mem=7), "invalid text_mem"),
    (dict(n_samp=0), r"invalid number of samples \(1 ... 2\^30 - 1\)"),
    (dict(n_samp=1 << 30), r"invalid number of samples \(1 ... 2\^30 - 1\)"),
    (dict(line_end=[12]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[-1]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[5], line_end=[4]), "an offset outside n_bytes or cell_begin > line_end: line 0"),
    (dict(cell_begin=[], line_end=[]), "invalid number of lines"),
]


@pytest.mark.parametrize("kw,message", REFUSALS)
def test_genotypes_refusals_touch_no_device(kw, message):
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_gen_genotypes: " + message):
        _call(**kw)


def test_a_line_longer_than_a_window_is_refused(monkeypatch):
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", "10")
    with pytest.raises(_lib.SnpGpuError, match=r"a line longer than the 10 bytes of a chunk \(SNPGPU_TEXT_STAGE_BYTES\): line 0"):
        _call()


def test_genotypes_null_host_arrays():
    import ctypes
    L = _lib.lib()
    one64 = np.zeros(1, np.int64)
    text = np.frombuffer(b"1 0 0", np.uint8)
    args = [_lib._ptr(text), _lib.HOST, 5, _lib._ptr(one64), _lib._ptr(np.full(1, 5, np.int64)), 1, 1, 0.9, ctypes.c_void_p(4096),
            _lib._ptr(np.zeros(1, np.int32)), _lib._ptr(one64.copy()), 0, None]
    for k, name in ((3, "cell_begin"), (4, "line_end"), (9, "line_flags"), (10, "line_cells")):
        a = list(args)
        a[k] = None
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_gen_genotypes: NULL argument: %s is NULL" % name):
            _lib.check(L.snpgpu_gen_genotypes(*a))


def test_header_declares_the_calls_and_no_result_memory_kind():
    import mem_kinds as M
    from conftest import ROOT
    protos = M.header_prototypes(open(os.path.join(ROOT, "include", "snpgpu.h")).read())
    for f in ("snpgpu_gen_genotypes", "snpgpu_gen_line_host", "snpgpu_gen_stats"):
        assert f in protos and f in _lib.EXPORTS and hasattr(_lib.lib(), f)
        assert not {"out_mem", "dst_mem", "mem"} & set(protos[f])
    assert protos["snpgpu_gen_genotypes"] == ["text", "text_mem", "n_bytes", "cell_begin", "line_end", "n_lines", "n_samp", "call_threshold",
                                              "rows", "line_flags", "line_cells", "device", "stream"]
