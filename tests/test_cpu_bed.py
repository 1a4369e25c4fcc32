"""CPU tests of the PLINK BED layer (snprelate_amd/bed.py, snpgdsOpenBED, snpgdsGDS2BED, snpgpu_geno_convert's refusals): the
reader's host path, the metadata rules, every refusal and the writer's numpy path against the restatement (tests/bed_ref.py),
byte for byte -- none needs a device."""
import ctypes
import gzip
import os
import warnings

import numpy as np
import pytest

import bed_ref as B
import geno_select_ref as R
import snprelate_amd
from conftest import GOLDEN
from snprelate_amd import _lib, api, bed
from snprelate_amd.gds import GenoFile, GenoStream, open_gds_stream

FIX = [os.path.join(GOLDEN, "plinkhapmap.%s.gz" % e) for e in ("bed", "fam", "bim")]


@pytest.fixture(scope="module")
def fixture_codes():
    """the fixture's genotypes through the restatement alone: GDS codes [5000][60]"""
    with gzip.open(FIX[0], "rb") as f:
        data = f.read()
    assert len(data) == 75003
    return data, B.bed_codes(data, 1, 5000, 60)


def _write_triple(tmp_path, name, g, mode, fam=None, bim=None, gz=False):
    """a .bed of `mode` written by the restatement from GDS codes [L][n], with a .fam and a .bim of matching length"""
    L, n = g.shape
    op = (lambda p: gzip.open(p, "wb")) if gz else (lambda p: open(p, "wb"))
    ext = ".gz" if gz else ""
    fns = [str(tmp_path / (name + e + ext)) for e in (".bed", ".fam", ".bim")]
    with op(fns[0]) as f:
        f.write(B.bed_file(g, mode))
    with op(fns[1]) as f:
        f.write("".join(fam if fam is not None else ["F%d S%d 0 0 %d -9\n" % (i // 2, i, i % 3) for i in range(n)]).encode())
    with op(fns[2]) as f:
        f.write("".join(bim if bim is not None else ["%d\trs%d\t0\t%d\tA\tC\n" % (1 + k % 3, k, 100 + k) for k in range(L)]).encode())
    return fns


def test_exports():
    L = _lib.lib()
    for s in ("snpgpu_geno_convert", "snpgpu_geno_convert_stats"):
        assert s in _lib.EXPORTS and hasattr(L, s), s
    assert callable(_lib.geno_convert) and callable(_lib.geno_convert_stats)
    assert (_lib.CODE_GDS, _lib.CODE_BED) == (0, 1)
    assert issubclass(bed.BedStream, GenoStream)
    assert snprelate_amd.snpgdsOpenBED is api.snpgdsOpenBED and snprelate_amd.snpgdsGDS2BED is api.snpgdsGDS2BED
    assert not hasattr(api, "snpgdsBED2GDS")


def test_the_dword_maps_are_the_tables():
    """the two bit operations of the kernels, on every byte value, against the reference's tables"""
    x = np.arange(256, dtype=np.uint32)
    codes = np.stack([(x >> (2 * k)) & 3 for k in range(4)], 1)
    pack = lambda c: (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint32)
    b2g = ((~x & 0xAA) | ((x ^ (x >> 1)) & 0x55)) & 0xFF
    g2b = ((~x & 0xAA) | (~(x ^ (x >> 1)) & 0x55)) & 0xFF
    assert np.array_equal(b2g, pack(B.BED_TO_GDS[codes])) and np.array_equal(g2b, pack(B.GDS_TO_BED[codes]))
    assert np.array_equal(B.GDS_TO_BED[B.BED_TO_GDS], np.arange(4))


def test_fixture_metadata():
    bs = api.snpgdsOpenBED(*FIX, verbose=False)
    assert isinstance(bs, bed.BedStream) and (bs.n_samp, bs.n_snp, bs.mode, bs.sample_order) == (60, 5000, 1, True)
    assert len(bs.sample_id) == 60 and bs.sample_id[0] == "NA19152"
    assert len(np.unique(bs.snp_id)) == 5000 and bs.snp_rs_id is None
    assert bs.snp_position[0] == 2444790 and bs.snp_allele[0] == "G/C" and bs.snp_chromosome[0] == 1
    assert bs.snp_chromosome.dtype.kind == "i" and set(np.unique(bs.snp_chromosome)) <= set(range(1, 27))
    assert set(bs.sample_annot) == {"sex", "phenotype"} and (bs.sample_annot["sex"] == "").all()
    assert (bs.sample_annot["phenotype"] == -9).all()
    assert set(api.snpgdsOpenBED(*FIX, family=True, verbose=False).sample_annot) == {"family", "father", "mother", "sex", "phenotype"}


@pytest.mark.parametrize("block", [1, 7, 5000])
def test_blocks_on_the_fixture(fixture_codes, block):
    _, g = fixture_codes
    bs = bed.BedStream(*FIX)
    got = [(lo, m, r.copy()) for lo, m, r in bs.blocks(block)]
    assert [lo for lo, _, _ in got] == list(range(0, 5000, block)) and sum(m for _, m, _ in got) == 5000
    assert np.array_equal(np.concatenate([r for _, _, r in got], 0), R.pack_ref(g))
    # a window, and caller's buffers
    bufs = [np.zeros((block, 15), np.uint8) for _ in range(2)]
    rows = np.concatenate([r.copy() for _, _, r in bs.blocks(block, buffers=bufs, snp_begin=1003, snp_end=1013)], 0)
    assert np.array_equal(rows, R.pack_ref(g[1003:1013]))


def test_fixture_against_the_hapmap_gds(fixture_codes, hapmap):
    """An anchor outside this project's BED code: the fixture and tests/golden/hapmap_geno.gds share 60 samples and, matched by
    (chromosome, position), 129 SNPs; 54 of those rows are equal and 75 equal after the allele swap (0 <-> 2, 3 kept).  A wrong
    table, or an exchanged axis, gives rows that are neither."""
    _, g = fixture_codes
    with gzip.open(FIX[2], "rt") as f:
        bim = [ln.split() for ln in f]
    with gzip.open(FIX[1], "rt") as f:
        ids = [ln.split()[1] for ln in f]
    pos = {(int(c), int(p)): i for i, (c, p) in enumerate(zip(hapmap.snp_chromosome, hapmap.snp_position))}
    common = [(k, pos[(int(t[0]), int(t[3]))]) for k, t in enumerate(bim) if (int(t[0]), int(t[3])) in pos]
    assert len(common) == 129
    where = {s: i for i, s in enumerate(hapmap.sample_id)}
    G = hapmap.read_genotype()[:, [where[s] for s in ids]]
    swap = np.array([2, 1, 0, 3], np.uint8)
    same = sum(np.array_equal(g[k], G[j]) for k, j in common)
    swapped = sum((not np.array_equal(g[k], G[j])) and np.array_equal(swap[g[k]], G[j]) for k, j in common)
    assert (same, swapped) == (54, 75)


@pytest.mark.parametrize("shape", [(60, 5000), (65, 1000), (7, 13), (1, 5), (130, 3)])
def test_both_modes_gz_and_inflated_read_the_same(fixture_codes, tmp_path, shape):
    n, L = shape
    g = fixture_codes[1] if shape == (60, 5000) else R.codes(L, n, 0.1, seed=n + L)
    want = R.pack_ref(g)
    for mode in (0, 1):
        for gz in (False, True):
            fns = _write_triple(tmp_path, "m%d%d" % (mode, gz), g, mode, gz=gz)
            bs = bed.BedStream(*fns)
            assert (bs.mode, bs.sample_order, bs.n_samp, bs.n_snp) == (mode, mode == 1, n, L)
            for block in (1, 7, 64, L):
                got = np.concatenate([r.copy() for _, _, r in bs.blocks(block)], 0)
                assert np.array_equal(got, want), (mode, gz, block)
            assert np.array_equal(bs.read_genotype(), g)
            assert np.array_equal(bs.read_genotype([L - 1, 0], [n - 1]), g[[L - 1, 0]][:, [n - 1]])


def test_bed_refusals_name_the_file(tmp_path, monkeypatch):
    g = R.codes(13, 7, 0.1, seed=1)
    for gz in (False, True):
        fns = _write_triple(tmp_path, "ok%d" % gz, g, 1, gz=gz)
        good = B.bed_file(g, 1)
        op = (lambda p, m: gzip.open(p, m)) if gz else (lambda p, m: open(p, m))

        def put(data):
            with op(fns[0], "wb") as f:
                f.write(data)

        for data, msg in ((b"\x6c\x1c" + good[2:], "not a PLINK BED file"), (b"BM" + good[2:], "not a PLINK BED file"),
                          (b"", "not a PLINK BED file"), (good[:2] + b"\x02" + good[3:], "invalid mode byte 2"),
                          (good[:2], "invalid mode byte missing"), (good[:-1], "holds"), (good + b"\x00", "holds"), (good[:3], "holds")):
            put(data)
            with pytest.raises(ValueError, match=msg) as e:
                bed.BedStream(*fns)
            assert fns[0] in str(e.value), (msg, str(e.value))
        # the same bytes as the other mode: 7 rows of 4 bytes, not 13 of 2
        put(good[:2] + b"\x00" + good[3:])
        with pytest.raises(ValueError, match="holds"):
            bed.BedStream(*fns)
        put(good)
        assert np.array_equal(bed.BedStream(*fns).read_genotype(), g)
        # .fam / .bim row counts that contradict the .bed length
        fam8 = _write_triple(tmp_path, "fam8%d" % gz, R.codes(13, 9, 0, seed=2), 1, gz=gz)[1]
        bim12 = _write_triple(tmp_path, "bim12%d" % gz, R.codes(12, 7, 0, seed=2), 1, gz=gz)[2]
        for trio in ((fns[0], fam8, fns[2]), (fns[0], fns[1], bim12)):
            with pytest.raises(ValueError, match="holds") as e:
                bed.BedStream(*trio)
            assert fns[0] in str(e.value)
    # a .bed.gz beyond the in-memory budget
    monkeypatch.setenv("SNPGPU_GDS_INFLATE_MAX", "20")
    with pytest.raises(ValueError, match="SNPGPU_GDS_INFLATE_MAX"):
        bed.BedStream(*fns)
    # text files with a wrong number of columns
    with open(str(tmp_path / "bad.fam"), "w") as f:
        f.write("0 a 0 0 0\n")
    with pytest.raises(ValueError, match="bad.fam', line 1: 5 columns"):
        bed.read_fam(str(tmp_path / "bad.fam"))
    with pytest.raises(ValueError, match="cvt.chr"):
        bed.BedStream(*fns, cvt_chr="number")
    with pytest.raises(ValueError, match="cvt.snpid"):
        bed.BedStream(*fns, cvt_snpid="rs")


def test_sample_and_snp_id_rules(tmp_path):
    g = R.codes(6, 4, 0.1, seed=3)
    bs = bed.BedStream(*_write_triple(tmp_path, "a", g, 1, fam=["f%d s%d p m %d 1.5\n" % (i, i, i) for i in range(4)]))
    assert list(bs.sample_id) == ["s0", "s1", "s2", "s3"] and list(bs.sample_annot["sex"]) == ["", "M", "F", ""]
    assert bs.sample_annot["phenotype"].dtype.kind == "f"
    # a repeated InvID: FamilyID-InvID; still repeated: refused
    bs = bed.BedStream(*_write_triple(tmp_path, "b", g, 1, fam=["f%d s%d 0 0 0 -9\n" % (i, i % 2) for i in range(4)]), family=True)
    assert list(bs.sample_id) == ["f0-s0", "f1-s1", "f2-s0", "f3-s1"] and list(bs.sample_annot["family"]) == ["f0", "f1", "f2", "f3"]
    with pytest.raises(ValueError, match="IDs in PLINK BED are not unique!"):
        bed.BedStream(*_write_triple(tmp_path, "c", g, 1, fam=["f s%d 0 0 0 -9\n" % (i % 2) for i in range(4)]))
    # numeric ids are integers, as read.table types them
    bs = bed.BedStream(*_write_triple(tmp_path, "d", g, 1, fam=["0 %d 0 0 0 -9\n" % (10 + i) for i in range(4)]))
    assert bs.sample_id.dtype.kind == "i" and list(bs.sample_id) == [10, 11, 12, 13]
    # .bim ids: kept when unique, else 1 ... L with snp_rs_id; cvt_snpid="int" always numbers
    dup = ["1\trs%d\t0\t%d\tA\tG\n" % (k % 5, 10 * k) for k in range(6)]
    bs = bed.BedStream(*_write_triple(tmp_path, "e", g, 1, bim=dup))
    assert list(bs.snp_id) == [1, 2, 3, 4, 5, 6] and list(bs.snp_rs_id) == ["rs0", "rs1", "rs2", "rs3", "rs4", "rs0"]
    fns = _write_triple(tmp_path, "f", g, 1)
    assert list(bed.BedStream(*fns).snp_id) == ["rs%d" % k for k in range(6)] and bed.BedStream(*fns).snp_rs_id is None
    bs = bed.BedStream(*fns, cvt_snpid="int")
    assert list(bs.snp_id) == [1, 2, 3, 4, 5, 6] and list(bs.snp_rs_id) == ["rs%d" % k for k in range(6)]
    assert list(bs.snp_position) == [100 + k for k in range(6)] and list(bs.snp_allele) == ["A/C"] * 6


def test_cvt_chr_both_ways(tmp_path):
    g = R.codes(8, 4, 0.1, seed=4)
    labels = ["1", "22", "X", "XY", "Y", "MT", "M", "chrUn"]
    fns = _write_triple(tmp_path, "chr", g, 1, bim=["%s\ts%d\t0\t%d\tA\tG\n" % (c, k, k + 1) for k, c in enumerate(labels)])
    with pytest.warns(UserWarning, match='Please use cvt.chr="char" for non-numeric chromosome codes'):
        bs = bed.BedStream(*fns)
    assert list(bs.snp_chromosome) == [1, 22, 23, 24, 25, 26, 26, 0] and (bs.autosome_start, bs.autosome_end) == (1, 22)
    with pytest.warns(UserWarning):
        bs = api.snpgdsOpenBED(*fns, option=api.snpgdsOption(autosome_end=38, X=39, Y=40), verbose=False)
    assert list(bs.snp_chromosome) == [1, 22, 39, 0, 40, 0, 0, 0] and bs.autosome_end == 38
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        bs = bed.BedStream(*fns, cvt_chr="char")
    assert list(bs.snp_chromosome) == labels and (bs.autosome_start, bs.autosome_end) == (1, 22)
    val, ok = bed.chrom_numeric(np.array(labels + ["7q", " 12"]))
    assert list(ok) == [True, True] + [False] * 6 + [True, True] and list(val[ok]) == [1, 22, 7, 12]
    with pytest.raises(ValueError, match="'option' should be NULL"):
        bed.BedStream(*fns, cvt_chr="char", option=api.snpgdsOption())
    # named after the .bed when neither is given (and only then)
    assert api.snpgdsOpenBED(fns[0], cvt_chr="char", verbose=False).n_snp == 8
    with pytest.raises(TypeError, match="fam.fn"):
        api.snpgdsOpenBED(fns[0], bim_fn=fns[2], verbose=False)


def test_gds_readers_carry_snp_allele(hapmap):
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    for obj in (hapmap, gs):
        assert obj.snp_allele is not None and len(obj.snp_allele) == obj.n_snp and obj.snp_allele[0] == "G/T"
    assert GenoFile(genotype=np.zeros((2, 3), np.uint8)).snp_allele is None


@pytest.mark.parametrize("snpfirstdim", [False, True, None])
def test_gds2bed_without_a_device(hapmap, tmp_path, monkeypatch, capsys, snpfirstdim):
    """the three files for the HapMap GDS with a sample subset and a SNP subset, the numpy path: .bed bytes equal the
    restatement's, and an opened copy reads the same genotypes"""
    monkeypatch.setattr(api, "_device_visible", lambda: False)
    rng = np.random.default_rng(5)
    samp, snps = rng.permutation(hapmap.n_samp)[:101], rng.permutation(hapmap.n_snp)[:1001]
    out = str(tmp_path / "out")
    api.snpgdsGDS2BED(hapmap, out, sample_id=hapmap.sample_id[samp], snp_id=hapmap.snp_id[snps], snpfirstdim=snpfirstdim, verbose=True)
    text = capsys.readouterr().out
    assert "Working space: 101 samples, 1001 SNPs" in text and text.rstrip().endswith("Done.")
    want = hapmap.read_genotype(np.sort(snps), np.sort(samp))
    mode = 0 if snpfirstdim else 1                                     # None follows the file: sample.order -> SNP-major
    assert hapmap.sample_order
    with open(out + ".bed", "rb") as f:
        assert f.read() == B.bed_file(want, mode)
    with open(out + ".fam") as f:
        assert f.read().splitlines() == ["0\t%s\t0\t0\t0\t-9" % s for s in hapmap.sample_id[np.sort(samp)]]
    k = np.sort(snps)
    with open(out + ".bim") as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    assert [r[1] for r in rows] == [str(i) for i in hapmap.snp_id[k]] and all(r[2] == "0" for r in rows)
    assert [int(r[3]) for r in rows] == list(hapmap.snp_position[k])
    assert ["%s/%s" % (r[4], r[5]) for r in rows] == list(hapmap.snp_allele[k])
    assert [r[0] for r in rows] == [str(c) for c in hapmap.snp_chromosome[k]]           # 1 ... 23 are written as they are
    back = api.snpgdsOpenBED(out + ".bed", verbose=False)
    assert back.mode == mode and np.array_equal(back.read_genotype(), want)
    assert np.array_equal(back.sample_id, hapmap.sample_id[np.sort(samp)]) and np.array_equal(back.snp_id, hapmap.snp_id[k])


def test_gds2bed_chromosome_codes_alleles_and_checks(tmp_path, monkeypatch):
    monkeypatch.setattr(api, "_device_visible", lambda: False)
    g = R.codes(7, 5, 0.2, seed=6)
    gf = GenoFile(genotype=g, sample_id=np.array(["a", "b", "c", "d", "e"]), snp_chromosome=np.array([1, 22, 23, 24, 25, 26, 0]),
                  snp_position=np.arange(7) + 1)
    out = str(tmp_path / "c")
    with pytest.warns(UserWarning, match="There is no allele information in the GDS file"):
        api.snpgdsGDS2BED(gf, out, verbose=False)
    with open(out + ".bim") as f:
        rows = [ln.split("\t") for ln in f.read().splitlines()]
    # the reference's two substitutions, as they stand: 24 -> "XY" -> 25 and 25 -> "Y" -> 24
    assert [r[0] for r in rows] == ["1", "22", "23", "25", "24", "26", "0"]
    assert [r[4:] for r in rows] == [["A", "B"]] * 7
    with open(out + ".bed", "rb") as f:
        assert f.read() == B.bed_file(g, 1)
    # a BedStream as the source: BED -> BED subsetting, in both modes, with its alleles
    src = api.snpgdsOpenBED(*_write_triple(tmp_path, "src", g, 0), verbose=False)
    for first in (True, False):
        api.snpgdsGDS2BED(src, out + "2", sample_id=["S4", "S1", "S2"], snp_id=["rs6", "rs0", "rs3", "rs5", "rs2"], snpfirstdim=first,
                          verbose=False)
        with open(out + "2.bed", "rb") as f:
            assert f.read() == B.bed_file(g[[0, 2, 3, 5, 6]][:, [1, 2, 4]], 0 if first else 1)
    with open(out + "2.bim") as f:
        assert f.readline() == "1\trs0\t0\t100\tA\tC\n"
    api.snpgdsGDS2BED(src, out + "3", verbose=False)                    # snpfirstdim=None follows the individual-major source
    with open(out + "3.bed", "rb") as f:
        assert f.read() == B.bed_file(g, 0)
    with pytest.raises(ValueError, match="Some of sample.id do not exist!"):
        api.snpgdsGDS2BED(gf, out, sample_id=["zz"], verbose=False)
    with pytest.raises(ValueError, match="Some of snp.id do not exist!"):
        api.snpgdsGDS2BED(gf, out, snp_id=[99], verbose=False)
    with pytest.raises(TypeError, match="snpfirstdim"):
        api.snpgdsGDS2BED(gf, out, snpfirstdim=1, verbose=False)
    with pytest.raises(TypeError, match="SNP GDS object"):
        api.snpgdsGDS2BED(12, out, verbose=False)
    with pytest.raises(ValueError, match="snp.position"):
        api.snpgdsGDS2BED(GenoFile(genotype=g), out, verbose=False)


def test_geno_convert_refuses_without_a_device():
    L = _lib.lib()
    bits = np.zeros(64, np.uint8)
    out = np.zeros(1 << 10, np.uint8)
    src = _lib.GenoSrc(bits.ctypes.data, _lib.HOST, 0, 4, 10, 0, 20, None, 64)

    def call(s=src, src_code=0, dst_major=0, dst_code=0, samp=None, n_samp_out=10, snp=None, n_snp_out=4):
        rc = L.snpgpu_geno_convert(ctypes.byref(s), src_code, _lib._ptr(samp), n_samp_out, _lib._ptr(snp), n_snp_out, _lib._ptr(out),
                                   dst_major, dst_code, _lib.HOST, 0, None)
        return rc, L.snpgpu_last_error().decode()

    cases = [(dict(src_code=2), "invalid src_code"), (dict(src_code=-1), "invalid src_code"), (dict(dst_code=2), "invalid dst_code"),
             (dict(dst_code=7), "invalid dst_code"), (dict(dst_major=2), "invalid dst_major"), (dict(dst_major=-1), "invalid dst_major"),
             # what snpgpu_geno_select refuses, under the new name and for either layout of dst
             (dict(s=_lib.GenoSrc(bits.ctypes.data, _lib.HOST, 0, 4, 10, 1, 20, None, 64)), "odd or negative bit position: bit0"),
             (dict(s=_lib.GenoSrc(bits.ctypes.data, _lib.HOST, 2, 4, 10, 0, 20, None, 64)), "invalid major"),
             (dict(s=_lib.GenoSrc(bits.ctypes.data, _lib.HOST, 0, 4, 10, 0, 20, None, 9)), "an element outside n_bytes: row 3"),
             (dict(dst_major=1, samp=np.array([0, 10], np.int32), n_samp_out=2), "an index outside the source: samp_index[1]"),
             (dict(dst_major=1, snp=np.array([4], np.int32), n_snp_out=1), "an index outside the source: snp_index[0]"),
             (dict(dst_major=1, n_snp_out=3), "snp_index is NULL"),
             # the axis dst packs holds at most 2^30 - 1 entries: for sample rows that is the SNPs
             (dict(s=_lib.GenoSrc(bits.ctypes.data, _lib.HOST, 1, 1, 1 << 30, 0, 0, None, 64), n_samp_out=1, n_snp_out=1 << 30, dst_major=1),
              "too many SNPs (< 2^30)"),
             (dict(s=_lib.GenoSrc(bits.ctypes.data, _lib.HOST, 1, 1, 1 << 31, 0, 0, None, 64), n_samp_out=1, n_snp_out=1 << 31),
              "too many SNPs (< 2^31)")]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == 1 and msg in err and err.startswith("snpgpu_geno_convert: "), (msg, err)
        assert "HIP" not in err and "hip" not in err, err              # refused before any device is asked for
    assert L.snpgpu_geno_convert_stats(None) == 1
    with pytest.raises(ValueError, match=r"n_samp_out \* ceil\(n_snp_out / 4\)"):
        _lib.geno_convert(bits, 0, 4, 10, dst_major=1, out=np.zeros(12, np.uint8))
    with pytest.raises(_lib.SnpGpuError, match="invalid dst_code"):
        _lib.geno_convert(bits, 0, 4, 10, dst_code=3)
