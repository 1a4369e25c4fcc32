"""Oxford GEN on the device: snpgpu_gen_genotypes, snprelate_amd.gen.GenReader and snpgdsOpenGEN against the restatement of the
reference's reader (tests/gen_ref.py) -- rows byte for byte, flags as the grammar predicts them, messages character for character."""
import gzip
import os

import numpy as np
import pytest

import gen_ref as G
import mem_kinds as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _lib():
    from snprelate_amd import _lib
    return _lib


def _index(data):
    """(cell_begin, line_end, the bytes from the sixth column on) of the lines of a .gen text, by the restatement's GetCell"""
    cb, le, cells, p = [], [], [], 0
    for line in G.split_lines(data):
        rl = G.Line(line)
        for _ in range(5):
            rl.get_cell(False)
        cb.append(p + rl.p)
        le.append(p + len(line))
        cells.append(line[rl.p:])
        p += len(line) + 1
    return np.array(cb, np.int64), np.array(le, np.int64), cells


def _expected(data, n, thr=0.9):
    return G.pack_rows(G.parse_text(data, n, thr)[1])


def _parse(data, cb, le, n, thr=0.9, text="device", offset=1, stream=None, text_offset=0):
    """one snpgpu_gen_genotypes call into a guarded device destination: (rows, flags, cells)"""
    import torch
    L = _lib()
    dest = M.DeviceDest((len(cb), (n + 3) // 4), np.uint8, offset)
    if text == "device":
        keep = torch.zeros(len(data) + text_offset, dtype=torch.uint8, device="cuda")
        keep[text_offset:].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        torch.cuda.synchronize()
        flags, cells = L.gen_genotypes(int(keep.data_ptr()) + text_offset, cb, le, n, thr, dest.ptr, n_bytes=len(data), stream=stream)
    elif text == "pinned":
        keep = L.PinnedBuffer((len(data),))
        keep.array[:] = np.frombuffer(data, np.uint8)
        flags, cells = L.gen_genotypes(keep.ptr, cb, le, n, thr, dest.ptr, n_bytes=len(data), text_mem=L.HOST_PINNED, stream=stream)
        keep.free()
    else:
        flags, cells = L.gen_genotypes(data, cb, le, n, thr, dest.ptr, stream=stream)
    return dest.read(), flags, cells


def _files(tmp_path, data, n, name="x.gen", version=">=2.0"):
    fn, sfn = str(tmp_path / name), str(tmp_path / "x.sample")
    op = gzip.open if name.endswith(".gz") else open
    with op(fn, "wb") as f:
        f.write(data)
    G.write_sample(sfn, ["id%d" % i for i in range(n)], version)
    return fn, sfn


# ---- an example written out --------------------------------------------------------------------------------------------------------------
def test_two_samples_two_lines():
    data = (b"snp1 rs1 1000 A G 1 0 0 0.02 0.95 0.03\n"        # AA; AB
            b"snp2 rs2 2000 C T 0 0.05 0.95 0.3 0.3 0.4\n")    # BB; nothing reaches 0.9: missing
    cb, le, _ = _index(data)
    assert cb.tolist() == [18, 57] and le.tolist() == [38, 80]
    rows, flags, cells = _parse(data, cb, le, 2)
    assert flags.tolist() == [0, 0] and cells.tolist() == [6, 6]
    assert rows.tolist() == [[2 | 1 << 2], [0 | 3 << 2]]
    assert np.array_equal(rows, _expected(data, 2))
    s = _lib().gen_stats()
    assert s["launches"] == 1 and s["text_bytes"] == len(data) and (s["chunk_bytes"], s["segment_bytes"], s["halo_bytes"]) == (4096, 16, 64)


# ---- regular grammar: equal to the restatement, nothing flagged -----------------------------------------------------------------------
@pytest.mark.parametrize("n_lines", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 700])
def test_regular_texts_equal_the_restatement_and_flag_nothing(n, n_lines):
    rng = np.random.default_rng(1000 * n + n_lines)
    for sep in (" ", "runs", "\t"):
        for final_newline in (True, False):
            data = G.make_text(rng, n, n_lines, sep=sep, final_newline=final_newline)
            cb, le, cells = _index(data)
            assert all(G.predict_flags(c, n) == (0, 3 * n) for c in cells)
            want = _expected(data, n)
            for text, offset in (("device", 1), ("host", 3)):
                rows, flags, ncell = _parse(data, cb, le, n, text=text, offset=offset)
                assert not flags.any(), "regular cells flagged: lines %s, flags %s" % (np.flatnonzero(flags)[:8], flags[flags != 0][:8])
                assert np.array_equal(ncell, np.full(n_lines, 3 * n))
                assert np.array_equal(rows, want), "rows differ on lines %s" % np.flatnonzero((rows != want).any(1))[:8]
    again, _, _ = _parse(data, cb, le, n)
    assert again.tobytes() == rows.tobytes()                                  # a pure function of its input


# ---- the chunk's end and the segment ends at every byte of a token and every component of a triple -------------------------------------
@pytest.mark.parametrize("digits", [3, 15])
def test_chunk_phases(digits):
    n = 700
    rng = np.random.default_rng(digits)
    lines = []
    for shift in range(24):                                # the length of the rs id column: every line starts its cells at another phase
        toks = ["0." + ("9" if rng.random() < 0.7 else "1") + "".join(str(int(x)) for x in rng.integers(0, 10, digits - 1))
                for _ in range(3 * n)]
        lines.append(G.make_line(rng, n, sep=" ", snp="s", rs="r" * shift, pos=7, tokens=toks, head_sep="\t"))
    data = b"\n".join(lines) + b"\n"
    cb, le, cells = _index(data)
    starts = np.concatenate(([0], le[:-1] + 1))
    assert len(cells[0]) == 3 * n * (digits + 3) - 1 > 3 * 4096 and np.array_equal(cb - starts, 9 + np.arange(24))
    want = _expected(data, n)
    assert len(np.unique(want)) > 20                       # the codes vary
    for text_offset in (0, 5):
        rows, flags, ncell = _parse(data, cb, le, n, text_offset=text_offset)
        assert not flags.any() and np.array_equal(ncell, np.full(24, 3 * n))
        assert np.array_equal(rows, want), "rows differ on lines %s" % np.flatnonzero((rows != want).any(1))


# ---- one rounding, not two ------------------------------------------------------------------------------------------------------------------
def test_rounding_to_single_precision_once():
    cases = list(G.MIDPOINTS) + G.double_rounding_cases(np.random.default_rng(9), 20)
    differ = 0
    for s in cases:
        a, b = G.strtof(s.encode())[0], G.float_of_double(G.strtod(s.encode())[0])
        thr = max(a, b)
        # sample 1: s as AA; sample 2: s as AB; sample 3: s as BB; sample 4: well above
        data = ("snp rs 1 A G %s 0 0 0 %s 0 0 0 %s %s 0 0\n" % (s, s, s, "1" if a < 2 else "99999999")).encode()
        cb, le, _ = _index(data)
        want = G.parse_text(data, 4, thr)[1][0]
        called = [2, 1, 0, 2] if a >= thr else [3, 3, 3, 2]
        assert want.tolist() == called, s
        rows, flags, _ = _parse(data, cb, le, 4, thr=thr)
        assert not flags.any() and rows.tolist() == G.pack_rows(want[None, :]).tolist(), (s, a, b)
        if a != b:                                          # the other rounding would call the other way
            differ += 1
            assert [G.call(b, 0.0, 0.0, thr), G.call(a, 0.0, 0.0, thr)] in ([2, 3], [3, 2]), s
        # one float above the larger of the two nothing is called
        up = float(np.nextafter(np.float32(thr), np.float32(np.inf)))
        rows, _, _ = _parse(data, cb, le, 4, thr=up)
        assert rows.tolist() == G.pack_rows(np.array([[3, 3, 3, 2]], np.uint8)).tolist(), s
    assert differ >= 22 and G.strtof(b"16777217")[0] == 16777216.0 > 2.0 ** 23


def test_thresholds():
    data = b"snp rs 1 A G 0.9 0 0 0.90000001 0 0 0 0.9 0 0 0 0.90000001 0.5 0.25 0.25 0.25 0.5 0.25\n"
    cb, le, _ = _index(data)
    for thr, want in ((0.9, [3, 2, 3, 0, 3, 3]), (0.5, [2, 2, 1, 0, 2, 1]), (0.89999997615814208984375, [2, 2, 1, 0, 3, 3]), (0.0, [2, 2, 1, 0, 2, 1]),
                      (1.5, [3] * 6)):
        assert G.parse_text(data, 6, thr)[1][0].tolist() == want
        rows, flags, _ = _parse(data, cb, le, 6, thr=thr)
        assert not flags.any() and rows.tolist() == G.pack_rows(np.array([want], np.uint8)).tolist(), thr


# ---- what the kernel leaves to the host ---------------------------------------------------------------------------------------------------------
_HOST_TOKENS = ["1e-3", "9E-1", "+0.95", "-0", "inf", "nan", "0x1p-1", "\"0.95\"", "'1'", "0.9512345678901234", "0." + "0" * 22 + "1",
                "0." + "9" * 68, "."]


def _planted(rng, n, n_lines, newline=b"\n"):
    """lines of regular cells; every third one holds one of _HOST_TOKENS, not as its last cell (with CRLF a quote would not match
    there): (data, the planted lines)"""
    lines, planted = [], []
    for i in range(n_lines):
        toks = [G.token(rng, G.FORMS[int(rng.integers(len(G.FORMS)))]) for _ in range(3 * n)]
        if i % 3 == 1:
            toks[int(rng.integers(3 * n - 1))] = _HOST_TOKENS[(i // 3) % len(_HOST_TOKENS)]
            planted.append(i)
        lines.append(G.make_line(rng, n, sep=" ", snp="snp%d" % i, rs="rs%d" % i, pos=i, tokens=toks))
    return newline.join(lines) + newline, planted


def test_exactly_the_planted_lines_are_flagged():
    n, n_lines = 300, 3 * len(_HOST_TOKENS)
    assert len(_HOST_TOKENS[-2]) == 70
    data, planted = _planted(np.random.default_rng(3), n, n_lines)
    cb, le, cells = _index(data)
    rows, flags, ncell = _parse(data, cb, le, n)
    assert np.array_equal(flags, [G.predict_flags(c, n)[0] for c in cells])
    assert np.flatnonzero(flags).tolist() == planted and np.array_equal(ncell, np.full(n_lines, 3 * n))
    F = G
    byte, nodigit = F.FLAG_BYTE, F.FLAG_BYTE | F.FLAG_DOT                     # "inf" and "nan" hold no digit either
    assert flags[planted].tolist() == [byte] * 4 + [nodigit] * 2 + [byte] * 3 + [F.FLAG_DIGITS, F.FLAG_DIGITS, F.FLAG_LONG | F.FLAG_DIGITS, F.FLAG_DOT]
    want = _expected(data, n)
    clean = np.flatnonzero(flags == 0)
    assert np.array_equal(rows[clean], want[clean])


@pytest.mark.parametrize("newline", [b"\n", b"\r\n"])
def test_reader_settles_flagged_lines_on_the_host(tmp_path, newline):
    from snprelate_amd import gen, snpgdsGetGeno, snpgdsOpenGEN
    n, n_lines = 41, 3 * len(_HOST_TOKENS)
    data, planted = _planted(np.random.default_rng(4), n, n_lines, newline)
    fn, sfn = _files(tmp_path, data, n)
    heads, codes = G.parse_text(data, n)
    r = gen.GenReader(fn, n)
    got = np.concatenate([rows.cpu().numpy() for _, _, rows in r.blocks(7)])
    assert np.array_equal(got, G.pack_rows(codes))
    assert r.flagged_lines == (len(planted) if newline == b"\n" else n_lines) and r.n_snp == n_lines
    f = snpgdsOpenGEN(fn, sfn, chr_code=7, verbose=False)
    assert np.array_equal(snpgdsGetGeno(f, snpfirstdim=True, verbose=False), codes)
    assert [(a, b, int(c), d) for a, b, c, d in zip(f.snp_id, f.snp_rs_id, f.snp_position, f.snp_allele)] == heads
    assert f.snp_chromosome.dtype == np.int32 and set(f.snp_chromosome) == {7} and list(f.sample_id) == ["id%d" % i for i in range(n)]


# ---- errors: the reference's message with FILE, LINE, COLUMN ----------------------------------------------------------------------------------------
def _broken(kind):
    rng = np.random.default_rng(11)
    n = 5
    lines = [G.make_line(rng, n, sep=" ", snp="snp%d" % i, rs="rs%d" % i, pos=i) for i in range(6)]
    t = lines[3].split(b" ")
    if kind == "fewer":
        lines[3] = b" ".join(t[:-1])
    elif kind == "more":
        lines[3] += b" 0.5"
    elif kind == "blank":
        lines[3] = b""
    elif kind == "tab at the end":
        lines[3] += b"\t"
    elif kind == "empty cell":
        lines[3] = b" ".join(t[:9]) + b"\t\t" + b" ".join(t[9:])
    elif kind == "NA":
        t[11] = b"NA"
        lines[3] = b" ".join(t)
    elif kind == "position":
        t[2] = b"12x"
        lines[3] = b" ".join(t)
    elif kind == "no cells":
        lines[3] = b" ".join(t[:5])
    elif kind == "first line blank":
        lines[0] = b""
    return b"\n".join(lines) + b"\n", n


@pytest.mark.parametrize("kind, message, column", [
    ("fewer", "fewer columns than what expected.", 20), ("more", "more columns than what expected.", 20), ("blank", "fewer columns than what expected.", 1),
    ("tab at the end", "more columns than what expected.", 20), ("empty cell", "Invalid float conversion \"\".", 10),
    ("NA", "Invalid float conversion \"NA\".", 12), ("position", "Invalid integer conversion \"x\".", 3),
    ("no cells", "fewer columns than what expected.", 6), ("first line blank", "fewer columns than what expected.", 1)])
def test_errors_carry_file_line_column(tmp_path, kind, message, column):
    from snprelate_amd import snpgdsOpenGEN
    data, n = _broken(kind)
    fn, sfn = _files(tmp_path, data, n)
    with pytest.raises(ValueError) as want:
        G.parse_text(data, n, path=fn)
    line = 1 if kind == "first line blank" else 4
    assert str(want.value).startswith("%s\nFILE: %s\nLINE: %d, COLUMN: %d, " % (message, fn, line, column))
    with pytest.raises(ValueError) as got:
        snpgdsOpenGEN(fn, sfn, chr_code=1, verbose=False)
    assert str(got.value) == str(want.value)


# ---- memory kinds of the text, staging windows, several files -----------------------------------------------------------------------------------------
def test_text_memory_kinds_and_staging_windows(monkeypatch):
    L = _lib()
    n, n_lines = 279, 23
    data = G.make_text(np.random.default_rng(77), n, n_lines)
    cb, le, _ = _index(data)
    want = _expected(data, n)
    for text in ("host", "pinned"):
        rows, flags, _ = _parse(data, cb, le, n, text=text)
        assert not flags.any() and np.array_equal(rows, want)
        s = L.gen_stats()
        assert s["launches"] == 1 and s["text_bytes"] == le[-1] - cb[0]
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", str(3 * int((le - cb).max()) + 200))          # about three lines to a window
    rows, flags, _ = _parse(data, cb, le, n, text="host")
    assert not flags.any() and np.array_equal(rows, want) and 6 <= L.gen_stats()["launches"] <= 12
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", str(int((le - cb).max()) - 1))
    with pytest.raises(L.SnpGpuError, match=r"a line longer than the \d+ bytes of a chunk \(SNPGPU_TEXT_STAGE_BYTES\)"):
        _parse(data, cb, le, n, text="host")
    monkeypatch.delenv("SNPGPU_TEXT_STAGE_BYTES")
    for off in (1, 2, 3, 7, 13):                           # misaligned device text between guards
        src = M.DeviceDest((len(data),), np.uint8, off)
        src.put(np.frombuffer(data, np.uint8).copy())
        dest = M.DeviceDest((n_lines, (n + 3) // 4), np.uint8, 1)
        flags, _ = L.gen_genotypes(src.ptr, cb, le, n, 0.9, dest.ptr, n_bytes=len(data))
        assert not flags.any() and np.array_equal(dest.read(), want)
        assert src.read().tobytes() == data


def test_wrong_cell_counts_stay_inside_their_rows():
    n = 21
    rng = np.random.default_rng(31)
    lines = [G.make_line(rng, n, snp="s%d" % i, pos=i) for i in range(8)]
    lines[2] += b" 1 0 0 1 0 0 1"                           # seven tokens more: never stored
    lines[5] = lines[5].rsplit(b" ", 4)[0]                  # four tokens fewer: the last two samples are code 0
    data = b"\n".join(lines) + b"\n"
    cb, le, cells = _index(data)
    for offset in M.OFFSETS:
        rows, flags, ncell = _parse(data, cb, le, n, offset=offset)                           # (the guards are checked in there)
        assert ncell.tolist() == [63, 63, 70, 63, 63, 59, 63, 63] and flags.tolist() == [0, 0, 32, 0, 0, 32, 0, 0]
    clean = [0, 1, 3, 4, 6, 7]
    want = G.pack_rows(np.stack([G.parse_line(lines[i], n)[1] for i in clean]))
    assert np.array_equal(rows[clean], want)
    full = G.parse_line(lines[5] + b" 0 0 0 0", n)[1]
    full[19:] = 0
    assert rows[5].tolist() == G.pack_rows(full[None, :])[0].tolist()


@pytest.mark.parametrize("chr_code", [[3, 21], ["X", "chrUn_1"]])
def test_staged_gz_files_reader_and_open_agree(tmp_path, monkeypatch, chr_code, capsys):
    from snprelate_amd import gen, snpgdsGetGeno, snpgdsOpenGEN
    n = 37
    rng = np.random.default_rng(5)
    parts = [G.make_text(rng, n, 19, sep="runs"), G.make_text(rng, n, 1, sep="\t", final_newline=False)]
    fns = []
    for k, d in enumerate(parts):
        fn, sfn = _files(tmp_path, d, n, name="p%d.gen.gz" % k, version="<=1.1.5")
        fns.append(fn)
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", str(len(parts[0]) // 5))
    want = np.concatenate([G.parse_text(d, n)[1] for d in parts])
    readers = [gen.GenReader(fn, n) for fn in fns]
    blocks = np.concatenate([rows.cpu().numpy() for r in readers for _, _, rows in r.blocks(2)])
    assert readers[0].windows >= 5 and np.array_equal(blocks, G.pack_rows(want))
    f = snpgdsOpenGEN(fns, sfn, chr_code=chr_code, version="<=1.1.5", verbose=True)
    out = capsys.readouterr().out
    assert f.packed.tobytes() == blocks.tobytes() and np.array_equal(snpgdsGetGeno(f, snpfirstdim=True, verbose=False), want)
    assert f.gen_windows >= 6 and f.n_samp == n and f.n_snp == 20
    assert list(f.snp_chromosome) == [chr_code[0]] * 19 + [chr_code[1]]
    assert f.snp_chromosome.dtype.kind == ("i" if isinstance(chr_code[0], int) else "U")
    assert list(f.snp_id) == ["snp%d" % (i + 1) for i in range(19)] + ["snp1"] and list(f.sample_annot) == ["ID_1", "ID_2", "missing"]
    assert out.splitlines() == ["Oxford GEN/BGEN format ---> GDS SNP format:", "The number of samples: 37, with SNPTEST version (<=1.1.5).",
                                "Parsing \"%s\" ..." % fns[0], "\tImport 19 variants on chromosome %s." % chr_code[0],
                                "Parsing \"%s\" ..." % fns[1], "\tImport 1 variant on chromosome %s." % chr_code[1]]
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", "64")
    with pytest.raises(ValueError, match=r"a line longer than the 64 bytes of a chunk \(SNPGPU_TEXT_STAGE_BYTES\)"):
        snpgdsOpenGEN(fns[0], sfn, chr_code=1, version="<=1.1.5", verbose=False)


# ---- the fixture, there and back ----------------------------------------------------------------------------------------------------------------------
def test_hapmap_fixture_as_gen_text(hapmap, tmp_path):
    import snprelate_amd
    from snprelate_amd import api as S
    from snprelate_amd.gds import GenoFile
    assert snprelate_amd.snpgdsOpenGEN is S.snpgdsOpenGEN
    n_snp, N = hapmap.n_snp, hapmap.n_samp
    g = hapmap.read_genotype()
    cell = np.array([" 0 0 1", " 0 1 0", " 1 0 0", " 0.3 0.3 0.4"], dtype=object)
    lines = ["snp%d rs%d %d A G" % (i, i, i + 1) + "".join(cell[g[i]]) for i in range(n_snp)]
    fn, sfn = str(tmp_path / "hapmap.gen"), str(tmp_path / "hapmap.sample")
    with open(fn, "w") as f:
        f.write("\n".join(lines) + "\n")
    G.write_sample(sfn, list(hapmap.sample_id))
    v = S.snpgdsOpenGEN(fn, sfn, chr_code=1, verbose=False)
    assert v.n_snp == n_snp and v.n_samp == N and v.gen_flagged_lines == 0
    assert np.array_equal(S.snpgdsGetGeno(v, snpfirstdim=True, verbose=False), g)
    assert [str(s) for s in v.sample_id] == [str(s) for s in hapmap.sample_id]
    sub = GenoFile(packed=hapmap.packed, n_samp=N, sample_id=v.sample_id, snp_id=v.snp_id, snp_chromosome=np.ones(n_snp, np.int32))
    assert np.array_equal(S.snpgdsGetGeno(sub, snpfirstdim=True, verbose=False), g)
    x = S.snpgdsIBSNum(v, autosome_only=False, verbose=False)
    y = S.snpgdsIBSNum(sub, autosome_only=False, verbose=False)
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes()


# ---- the ABI's refusals, with a device present ---------------------------------------------------------------------------------------------------------
def test_refusals_and_the_callers_stream():
    import torch
    L = _lib()
    data = G.make_text(np.random.default_rng(8), 65, 17)
    cb, le, _ = _index(data)
    want = _expected(data, 65)
    dest = M.DeviceDest((17, 17), np.uint8, 3)
    for kw, message in ((dict(rows=0), "NULL argument: rows is NULL"), (dict(text_mem=7), "invalid text_mem"), (dict(n=0), "invalid number of samples"),
                        (dict(le=le + 2), "an offset outside n_bytes or cell_begin > line_end: line 16"),
                        (dict(cb=cb[:0], le=le[:0]), "invalid number of lines")):
        a = dict(cb=cb, le=le, n=65, rows=dest.ptr, text_mem=None)
        a.update(kw)
        with pytest.raises(L.SnpGpuError, match="snpgpu_gen_genotypes: " + message):
            L.gen_genotypes(data, a["cb"], a["le"], a["n"], 0.9, a["rows"], text_mem=a["text_mem"])
    dest.untouched(np.ones((17, 17), bool))
    # a caller's stream: the text is still the decoy's when the call is made; the stream's order puts the real one there first
    decoy = data.translate(bytes.maketrans(b"019", b"901"))
    real = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    text = torch.from_numpy(np.frombuffer(decoy, np.uint8).copy()).cuda()
    s = torch.cuda.Stream()
    ev = M.delayed_write(s, text, real)
    M.still_pending(ev)
    flags, _ = L.gen_genotypes(int(text.data_ptr()), cb, le, 65, 0.9, dest.ptr, n_bytes=len(data), stream=s.cuda_stream)
    assert ev.query()
    assert not flags.any() and np.array_equal(dest.read(), want)
    assert os.path.exists(os.path.join(GOLDEN, "hapmap_geno.gds"))
