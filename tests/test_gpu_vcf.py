"""GPU tests of the VCF parser (snpgpu_vcf_genotypes, vcf.VcfReader, snpgdsOpenVCF): the rows equal the restatement
(tests/vcf_ref.py) byte for byte, padding codes included, with NO line flagged on any regular-grammar text -- which keeps the
kernel from handing its work to the host -- at every size, byte phase and chunk / segment / halo boundary; exactly the planted
irregular lines are flagged; nothing is stored outside a line's row; every memory kind of the text gives the same rows."""
import gzip
import os

import numpy as np
import pytest

import mem_kinds as M
import vcf_cases as C
import vcf_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEQ = os.path.join(GOLDEN, "sequence.vcf")


def _lib():
    from snprelate_amd import _lib
    return _lib


def _expected(cell_texts, n, na, ri=None):
    rb = (n + 3) // 4
    rows = [R.pack_row(R.line_codes(t, n, int(na[i]), 0 if ri is None else int(ri[i]))) for i, t in enumerate(cell_texts)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(cell_texts), rb)


def _parse(data, cb, le, na, n, ri=None, text="device", offset=1, stream=None, text_offset=0):
    """one snpgpu_vcf_genotypes call into a guarded device destination: (rows, flags, cells)"""
    import torch
    L = _lib()
    nl = len(cb)
    ri = np.zeros(nl, np.int32) if ri is None else ri
    dest = M.DeviceDest((nl, (n + 3) // 4), np.uint8, offset)
    keep = None
    if text == "device":
        keep = torch.zeros(len(data) + text_offset, dtype=torch.uint8, device="cuda")
        keep[text_offset:].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        torch.cuda.synchronize()
        flags, cells = L.vcf_genotypes(int(keep.data_ptr()) + text_offset, cb, le, na, ri, n, dest.ptr, n_bytes=len(data), stream=stream)
    elif text == "pinned":
        keep = L.PinnedBuffer((len(data),))
        keep.array[:] = np.frombuffer(data, np.uint8)
        flags, cells = L.vcf_genotypes(keep.ptr, cb, le, na, ri, n, dest.ptr, n_bytes=len(data), text_mem=L.HOST_PINNED, stream=stream)
        keep.free()
    else:
        flags, cells = L.vcf_genotypes(data, cb, le, na, ri, n, dest.ptr, stream=stream)
    return dest.read(), flags, cells


def _case(L, n, seed, **kw):
    codes = np.random.default_rng(seed).integers(0, 4, (L, n))
    fixed, cells, na = C.make_lines(codes, seed=seed, id_lens=list(range(3, 19)), **kw)
    data = C.join_lines(fixed, cells).encode()
    col, end, used = _lib().vcf_index(data)
    assert used == len(data) and len(col) == L
    return data, col[:, 9].copy(), end, np.array(na, np.int32), ["\t".join(c) for c in cells], codes


# ---- regular grammar: equal to the restatement, nothing flagged -----------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(1, 64), (3, 33), (4, 1), (5, 64), (63, 17), (64, 2), (65, 31), (279, 9), (1025, 5), (4099, 3)])
def test_regular_cells_equal_the_restatement_and_flag_nothing(n, L):
    data, cb, le, na, texts, codes = _case(L, n, 100 + n)
    want = _expected(texts, n, na)
    assert np.array_equal(want, np.frombuffer(b"".join(R.pack_row(c) for c in codes), np.uint8).reshape(want.shape))
    for text, offset in (("device", 1), ("host", 3)):
        rows, flags, cells = _parse(data, cb, le, na, n, text=text, offset=offset)
        assert not flags.any(), "regular cells flagged: lines %s, flags %s" % (np.flatnonzero(flags)[:8], flags[flags != 0][:8])
        assert np.array_equal(cells, np.full(L, n))
        assert np.array_equal(rows, want), "rows differ on lines %s" % np.flatnonzero((rows != want).any(1))[:8]
    again, _, _ = _parse(data, cb, le, na, n)
    assert again.tobytes() == rows.tobytes()                                  # a pure function of its input


def test_line_starts_at_all_16_byte_phases_and_ref_index():
    data, cb, le, na, texts, _ = _case(64, 7, 7)
    assert len(set(int(x) % 16 for x in cb)) == 16
    rng = np.random.default_rng(1)
    ri = np.array([int(rng.integers(-1, a)) for a in na], np.int32)          # another allele is counted, or none (-1)
    for text_offset in (0, 5):                                                # ... and the text itself at another phase
        rows, flags, cells = _parse(data, cb, le, na, 7, ri=ri, text_offset=text_offset)
        assert not flags.any() and np.array_equal(rows, _expected(texts, 7, na, ri))


def _line_with_cell_at(offset, gt, tail=("1/1", "0|1:9", ".")):
    """cells of a line whose cell `gt` starts `offset` bytes behind the start of the first cell"""
    cells, pos = [], 0
    while offset - pos >= 6:
        cells.append("1|0")
        pos += 4
    r = offset - pos                                                          # 0, or 1 ... 5 bytes for one cell and its tab
    if r:
        cells.append(("0:777"[:r - 1]) if r > 1 else "")
    return cells + [gt] + list(tail)


def _aligned(cell_lists):
    """data lines whose first cell starts at a multiple of 16 (the ID is padded), so that with text in aligned device memory the
    chunk and segment grid of every line starts at its first cell: (data, cell_begin, line_end)"""
    out, cb, le = b"", [], []
    for i, cells in enumerate(cell_lists):
        fixed = C.fixed_columns(i, 12, id_len=4)
        head = "\t".join(fixed) + "\t"
        fixed[2] += "x" * (-(len(out) + len(head)) % 16)
        head = "\t".join(fixed) + "\t"
        cb.append(len(out) + len(head))
        out += (head + "\t".join(cells)).encode()
        le.append(len(out))
        out += b"\n"
    assert all(x % 16 == 0 for x in cb)
    return out, np.array(cb, np.int64), np.array(le, np.int64)


def test_boundary_sweep_of_chunk_segment_and_halo():
    s = _lib().vcf_stats()
    chunk, seg, halo = s["chunk_bytes"], s["segment_bytes"], s["halo_bytes"]
    assert chunk % seg == 0 and chunk >= 16 * seg and halo >= 16
    lists = []
    for gt in ("0", "0|1", "10/11"):                                          # GT lengths 1, 3, 5
        for bound in (seg * 5, chunk, chunk + halo):                          # a segment boundary, a chunk boundary, the halo's end
            for d in range(-9, 2):
                lists.append(_line_with_cell_at(bound + d, gt))
                lists.append(_line_with_cell_at(bound + d, gt + ":" + "5" * 11))       # its GT ends inside, its cell crosses
    # a chunk whose first cell index is 1, 2, 3 (mod 4): k two-byte cells in front shift every later index
    first_index = set()
    for k in range(8):
        cells = ["1"] * k + _line_with_cell_at(chunk - 2 * k, "0|0")
        text = "\t".join(cells)
        assert text[chunk - 1] == "\t"                                        # a tab as the last byte of the chunk
        first_index.add(text[:chunk].count("\t") % 4)
        lists.append(cells)
    assert first_index >= {1, 2, 3}
    # chunks that hold no tab: 3 x chunk bytes of annotation in one cell; a GT longer than the halo (64 alleles)
    lists.append(["0|1", "1|1:" + "7" * (3 * chunk), "0/0", ".", "0|0"])
    lists.append(_line_with_cell_at(chunk - 7, "/".join(["0", "1"] * (halo // 2))))
    # one call for all: every line is padded with "." cells to the longest
    n = max(len(c) for c in lists)
    lists = [c + ["."] * (n - len(c)) for c in lists]
    data, cb, le = _aligned(lists)
    na = np.full(len(lists), 12, np.int32)
    rows, flags, cells = _parse(data, cb, le, na, n)
    want = _expected(["\t".join(c) for c in lists], n, na)
    assert not flags.any(), "flagged: %s" % np.flatnonzero(flags)[:8]
    assert np.array_equal(cells, np.full(len(lists), n))
    assert np.array_equal(rows, want), "rows differ on lines %s" % np.flatnonzero((rows != want).any(1))[:8]
    # the same text from the host, where every line's grid starts elsewhere
    rows, flags, _ = _parse(data, cb, le, na, n, text="host")
    assert not flags.any() and np.array_equal(rows, want)


def test_one_line_of_20000_samples():
    rng = np.random.default_rng(3)
    pool = np.array(["0|1:35:99.5,1", "1|1:7:12.25,0", "0|0:120:3.5,22", "./.:.:.,.,.,.", "1|0:35:99.5,1", "0/0:8:0.125,7"])
    cells = list(pool[rng.integers(0, len(pool), 20000)])
    data, cb, le = _aligned([cells])
    assert 12 * 20000 <= le[0] - cb[0] <= 15 * 20000
    na = np.array([2], np.int32)
    want = _expected(["\t".join(cells)], 20000, na)
    for text in ("device", "pinned"):
        rows, flags, ncell = _parse(data, cb, le, na, 20000, text=text)
        assert not flags.any() and ncell[0] == 20000 and np.array_equal(rows, want)


# ---- irregular cells: flagged, and decided by the host -------------------------------------------------------------------------------
PLANTED = [(2, " 0/1", 1), (5, "+0/1", 1), (7, "\"0|1\"", 1), (9, "/0", 1), (11, "0//0", 1), (13, "2/0", 2), (15, "0000000001/0", 4),
           (17, "-1/0", 1), (19, "0/ 1", 1), (21, "'0|1'", 1), (22, "1|0|3", 2)]


def _planted_case(n=9, L=24):
    codes = np.random.default_rng(8).integers(0, 4, (L, n))
    fixed, cells, na = C.make_lines(codes, seed=8, num_allele=2)
    for k, (line, cell, _) in enumerate(PLANTED):
        cells[line][(3 * k) % n] = cell
    return fixed, cells, na


def test_exactly_the_planted_lines_are_flagged():
    fixed, cells, na = _planted_case()
    data = C.join_lines(fixed, cells).encode()
    col, end, _ = _lib().vcf_index(data)
    rows, flags, ncell = _parse(data, col[:, 9], end, np.array(na, np.int32), 9)
    want_flags = np.zeros(24, np.int32)
    for line, _, bit in PLANTED:
        want_flags[line] = bit
    assert np.array_equal(flags, want_flags) and np.array_equal(ncell, np.full(24, 9))
    clean = np.flatnonzero(want_flags == 0)
    want = _expected(["\t".join(cells[i]) for i in clean], 9, na)
    assert np.array_equal(rows[clean], want)


def _write(tmp_path, name, text, gz=False):
    fn = str(tmp_path / name)
    with (gzip.open(fn, "wb") if gz else open(fn, "wb")) as f:
        f.write(text.encode())
    return fn


def _read_all(reader, block_snps):
    out = []
    for lo, m, rows in reader.blocks(block_snps):
        assert lo == sum(len(x) for x in out)
        out.append(rows.cpu().numpy().copy())
    return np.concatenate(out, 0)


def test_reader_patches_accepted_lines_and_raises_the_reference_message(tmp_path):
    from snprelate_amd import vcf
    fixed, cells, na = _planted_case()
    accepted = {" 0/1", "+0/1", "\"0|1\"", "0/ 1", "'0|1'", "0000000001/0"}
    ok_cells = [list(c) for c in cells]
    for k, (line, cell, _) in enumerate(PLANTED):
        if cell not in accepted:
            ok_cells[line][(3 * k) % 9] = "0|1"
    text = C.vcf_text(fixed, ok_cells)
    d = R.parse_vcf(text, "copy.num.of.ref")
    want = np.frombuffer(b"".join(R.pack_row(g) for g in d["geno"]), np.uint8).reshape(24, 3)
    # flagged lines in the middle of a block (one block of 24, blocks of 5) leave their neighbours as the kernel wrote them
    for block in (64, 5):
        r = vcf.VcfReader(_write(tmp_path, "ok%d.vcf" % block, text), method="copy.num.of.ref")
        assert np.array_equal(_read_all(r, block), want)
        assert list(r.snp_id) == d["snp_id"] and list(r.snp_allele) == d["allele"]
    for k, (line, cell, _) in enumerate(PLANTED):
        if cell in accepted:
            continue
        bad = [list(c) for c in ok_cells]
        bad[line][(3 * k) % 9] = cell
        text = C.vcf_text(fixed, bad)
        with pytest.raises(R.RefError) as e:
            R.parse_vcf(text, "copy.num.of.ref")
        fn = _write(tmp_path, "bad%d.vcf" % k, text)
        with pytest.raises(ValueError) as g:
            _read_all(vcf.VcfReader(fn, method="copy.num.of.ref"), 64)
        assert str(g.value).startswith("%s\nFILE: %s\nLINE: %d, COLUMN: %d, " % (e.value.message, fn, e.value.line, e.value.column))
        assert e.value.line == 4 + line and e.value.column == 10 + (3 * k) % 9


@pytest.mark.parametrize("offset", M.OFFSETS)
def test_wrong_cell_counts_are_flagged_and_stay_inside_their_rows(offset):
    n = 21
    data, cb, le, na, texts, _ = _case(12, n, 31)
    lines = data.decode().split("\n")[:-1]
    lines[3] += "\t0|1\t1|1\t0/0"                                             # n + 3 cells
    lines[6] = lines[6].rsplit("\t", 1)[0]                                    # n - 1 cells
    lines[9] += "\t"                                                          # an empty last cell behind n cells
    lines[11] = lines[11].rsplit("\t", 1)[0] + "\t"                           # n cells, the last one empty
    data = ("\n".join(lines) + "\n").encode()
    col, end, _ = _lib().vcf_index(data)
    rows, flags, ncell = _parse(data, col[:, 9], end, na, n, offset=offset)   # (the guards of both sides are checked in there)
    want_cells = np.full(12, n)
    want_cells[[3, 6, 9]] = n + 3, n - 1, n + 1
    assert np.array_equal(ncell, want_cells)
    assert np.array_equal(flags != 0, np.isin(np.arange(12), [3, 6, 9, 11])) and np.all(flags[[3, 6, 9, 11]] == 8)
    clean = [i for i in range(12) if i not in (3, 6, 9, 11)]
    assert np.array_equal(rows[clean], _expected([texts[i] for i in clean], n, na[clean]))
    for text in ("host", "pinned"):
        r2, f2, c2 = _parse(data, col[:, 9], end, na, n, offset=offset, text=text)
        assert np.array_equal(f2, flags) and np.array_equal(c2, ncell) and np.array_equal(r2[clean], rows[clean])


# ---- memory kinds of the text, staging windows, the caller's stream --------------------------------------------------------------------
def test_text_memory_kinds_and_staging_windows(monkeypatch):
    import torch
    L = _lib()
    n = 279
    data, cb, le, na, texts, _ = _case(23, n, 77)
    want = _expected(texts, n, na)
    for text in ("host", "pinned"):
        rows, flags, _ = _parse(data, cb, le, na, n, text=text)
        assert not flags.any() and np.array_equal(rows, want)
        s = L.vcf_stats()
        assert s["launches"] == 1 and s["text_bytes"] == le[-1] - cb[0]
    # windows of whole lines: a staging size that holds about three lines, and one that holds less than a line
    for stage in (3 * int((le - cb).max()) + 200, 100):
        monkeypatch.setenv("SNPGPU_VCF_STAGE_BYTES", str(stage))
        rows, flags, _ = _parse(data, cb, le, na, n, text="host")
        assert not flags.any() and np.array_equal(rows, want)
        assert (6 <= L.vcf_stats()["launches"] <= 12) if stage > 100 else L.vcf_stats()["launches"] == 23
    monkeypatch.delenv("SNPGPU_VCF_STAGE_BYTES")
    # misaligned device text between guards: the text stays as it was and the rows are the same
    for off in (1, 2, 3, 7, 13):
        src = M.DeviceDest((len(data),), np.uint8, off)
        src.put(np.frombuffer(data, np.uint8).copy())
        dest = M.DeviceDest((23, (n + 3) // 4), np.uint8, 1)
        flags, _ = L.vcf_genotypes(src.ptr, cb, le, na, np.zeros(23, np.int32), n, dest.ptr, n_bytes=len(data))
        assert not flags.any() and np.array_equal(dest.read(), want)
        assert src.read().tobytes() == data
    del torch


def test_the_callers_stream_is_honoured():
    import torch
    L = _lib()
    n = 65
    data, cb, le, na, texts, _ = _case(17, n, 5)
    want = _expected(texts, n, na)
    decoy = data.translate(bytes.maketrans(b"01", b"10"))                    # the same layout, other genotypes
    real = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    text = torch.from_numpy(np.frombuffer(decoy, np.uint8).copy()).cuda()
    dest = M.DeviceDest((17, (n + 3) // 4), np.uint8, 3)
    s = torch.cuda.Stream()
    ev = M.delayed_write(s, text, real)
    M.still_pending(ev)                                                       # (the call blocks until it has its flags)
    flags, _ = L.vcf_genotypes(int(text.data_ptr()), cb, le, na, np.zeros(17, np.int32), n, dest.ptr, n_bytes=len(data),
                               stream=s.cuda_stream)
    assert ev.query()
    assert not flags.any() and np.array_equal(dest.read(), want)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["biallelic.only", "copy.num.of.ref"])
def test_open_sequence_vcf(method):
    import snprelate_amd
    from snprelate_amd import api as S
    assert snprelate_amd.snpgdsOpenVCF is S.snpgdsOpenVCF
    f = S.snpgdsOpenVCF(SEQ, method=method, verbose=False)
    d = R.parse_vcf(open(SEQ).read(), method)
    assert list(f.sample_id) == ["NA00001", "NA00002", "NA00003"] and f.n_samp == 3 and f.n_snp == len(d["geno"])
    assert f.read_genotype().tolist() == d["geno"] and f.packed.tobytes() == b"".join(R.pack_row(g) for g in d["geno"])
    assert list(f.snp_id) == d["snp_id"] and list(f.snp_position) == d["pos"] and list(f.snp_rs_id) == d["rs"]
    assert list(f.snp_allele) == d["allele"] and list(f.snp_chromosome) == d["chrom"] and list(f.snp_annot["filter"]) == d["filter"]
    assert f.snp_annot["qual"].dtype == np.float32 and f.snp_annot["qual"].tolist() == d["qual"]
    if method == "biallelic.only":
        assert f.read_genotype().tolist() == [[2, 1, 0], [2, 1, 2]] and list(f.snp_allele) == ["G/A", "T/A"]
    else:
        assert f.read_genotype().tolist()[2:] == [[0, 0, 0], [2, 2, 2], [1, 1, 0]]
    g = S.snpgdsGetGeno(f, snpfirstdim=True, verbose=False)
    assert g.tolist() == d["geno"]
    rf = S.snpgdsSNPRateFreq(f)
    want = [np.mean([x for x in row if x < 3]) / 2 for row in d["geno"]]
    assert np.allclose(rf["AlleleFreq"], want)


def _hapmap_vcf_lines(hapmap, lo, hi):
    """SNPs lo ... hi - 1 of the fixture as VCF data lines: 2 -> 0/0, 1 -> 0/1, 0 -> 1/1, 3 -> ./."""
    g = hapmap.read_genotype(np.arange(lo, hi))
    lut = np.array([b"1/1\t", b"0/1\t", b"0/0\t", b"./.\t"], "S4").view(np.uint32)
    body = lut[g].view(np.uint8).reshape(hi - lo, -1)
    out = []
    for k in range(hi - lo):
        i = lo + k
        head = "%s\t%d\trs%d\tA\tC\t.\t.\t.\tGT\t" % (hapmap.snp_chromosome[i], 0 if hapmap.snp_position is None else hapmap.snp_position[i],
                                                      i)
        out.append(head.encode() + body[k, :-1].tobytes() + b"\n")
    return b"".join(out)


def test_hapmap_fixture_as_vcf_text(hapmap, tmp_path):
    import snprelate_amd
    from snprelate_amd import api as S
    assert snprelate_amd.snpgdsOpenVCF is S.snpgdsOpenVCF
    from snprelate_amd.gds import GenoFile
    n_snp, cut = 2000, 1200
    head = (C.HEADER + "\t".join("#CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split() + [str(s) for s in hapmap.sample_id])
            + "\n").encode()
    a, b = str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf.gz")
    with open(a, "wb") as f:
        f.write(head + _hapmap_vcf_lines(hapmap, 0, cut))
    with gzip.open(b, "wb") as f:
        f.write(head + _hapmap_vcf_lines(hapmap, cut, n_snp))
    v = S.snpgdsOpenVCF([a, b], verbose=False)
    assert v.n_snp == n_snp and v.n_samp == hapmap.n_samp
    assert v.packed.tobytes() == hapmap.packed[:n_snp].tobytes()
    assert list(v.snp_id) == list(range(1, n_snp + 1)) and list(v.snp_rs_id[[0, cut, n_snp - 1]]) == ["rs0", "rs%d" % cut, "rs%d" % (n_snp - 1)]
    sub = GenoFile(packed=hapmap.packed[:n_snp], n_samp=hapmap.n_samp, sample_id=hapmap.sample_id, snp_id=np.arange(1, n_snp + 1),
                   snp_chromosome=hapmap.snp_chromosome[:n_snp])
    x = S.snpgdsIBSNum(v, autosome_only=False, verbose=False)
    y = S.snpgdsIBSNum(sub, autosome_only=False, verbose=False)
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes()
    # the reader alone, in small chunks of the file: the same rows, block by block
    from snprelate_amd import vcf
    r = vcf.VcfReader(a, chunk_bytes=200000)
    assert _read_all(r, 256).tobytes() == hapmap.packed[:cut].tobytes()


def test_the_budget_names_the_block_reader(monkeypatch):
    import snprelate_amd
    from snprelate_amd import api as S
    assert snprelate_amd.snpgdsOpenVCF is S.snpgdsOpenVCF
    monkeypatch.setenv("SNPGPU_VCF_MAX_BYTES", "1")
    with pytest.raises(ValueError, match="VcfReader.blocks"):
        S.snpgdsOpenVCF(SEQ, verbose=False)
