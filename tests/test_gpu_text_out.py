"""GPU tests of the text renderer (snpgpu_text_render, snpgdsGDS2PED, snpgdsGDS2Eigen): the files equal the restatements of the
reference's writers (tests/text_ref.py) byte for byte -- the hand-derived literals, the HapMap fixture with and without
selections, and synthetic shapes at every column count, prefix phase and allele length where the kernels can go wrong; nothing
is stored outside the text; the sizing call equals the lengths of the written lines."""
import os

import numpy as np
import pytest

import text_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HAPMAP = os.path.join(GOLDEN, "hapmap_geno.gds")
FMT = {"A/G/C/T": 1, "A/B": 2, "1/2": 3}


def _pkg():
    import snprelate_amd
    return snprelate_amd


def _read(fn):
    with open(fn, "rb") as f:
        return f.read()


# ---- the literals -----------------------------------------------------------------------------------------------------------------
GENO = np.array([[0, 1, 2, 3], [2, 3, 1, 0], [1, 0, 3, 2]], np.uint8)                  # sample x SNP
ALLELES = ["A/G", "T/", "AT/A", "C/G/T"]
PED_ACGT = (b"0\ts1\t0\t0\t0\t-9\tG G\tT 0\tAT AT\t0 0\n"
            b"0\ts2\t0\t0\t0\t-9\tA A\t0 0\tAT A\tG G\n"
            b"0\ts3\t0\t0\t0\t-9\tA G\t0 0\t0 0\tC C\n")
EIGEN = b"021\n190\n219\n902\n"


def _small():
    from snprelate_amd.gds import GenoFile
    g = GenoFile(genotype=GENO.T.copy(), sample_id=["s1", "s2", "s3"], snp_id=[11, 12, 13, 14], snp_chromosome=[1, 23, 24, 26],
                 snp_position=[100, 200, 300, 400], snp_allele=ALLELES)
    return g


def test_literals(tmp_path):
    S = _pkg()
    g = _small()
    fn = str(tmp_path / "a")
    S.snpgdsGDS2PED(g, fn, verbose=False)
    assert _read(fn + ".ped") == PED_ACGT == R.ped_text(g.sample_id, ALLELES, GENO, 1)
    assert _read(fn + ".map") == b"1\t11\t0\t100\nX\t12\t0\t200\nXY\t13\t0\t300\nMT\t14\t0\t400\n"
    S.snpgdsGDS2PED(g, fn, format="A/B", verbose=False)
    assert _read(fn + ".ped").split(b"\n")[0] == b"0\ts1\t0\t0\t0\t-9\tB B\tA B\tA A\t0 0"
    assert _read(fn + ".ped") == R.ped_text(g.sample_id, None, GENO, 2)
    S.snpgdsGDS2PED(g, fn, format="1/2", verbose=False)
    assert _read(fn + ".ped").split(b"\n")[0] == b"0\ts1\t0\t0\t0\t-9\t2 2\t1 2\t1 1\t0 0"
    assert _read(fn + ".ped") == R.ped_text(g.sample_id, None, GENO, 3)
    S.snpgdsGDS2Eigen(g, fn, verbose=False)
    assert _read(fn + ".eigenstratgeno") == EIGEN == R.eigen_text(GENO.T)
    assert _read(fn + ".snp") == b"11\t1\t0\t100\n12\t23\t0\t200\n13\t24\t0\t300\n14\t26\t0\t400\n"
    assert _read(fn + ".ind") == b"s1\tU\tcontrol\ns2\tU\tcontrol\ns3\tU\tcontrol\n"
    g.snp_allele = None
    with pytest.raises(ValueError, match="There is no 'snp.allele' variable in the GDS file."):
        S.snpgdsGDS2PED(g, fn, verbose=False)
    with pytest.raises(ValueError, match="Some of sample.id do not exist!"):
        S.snpgdsGDS2Eigen(g, fn, sample_id=["s1", "zz"], verbose=False)
    g.sample_annot["sex"] = np.array(["M", None, "F"], dtype=object)
    S.snpgdsGDS2Eigen(g, fn, verbose=False)
    assert _read(fn + ".ind") == b"s1\tM\tcontrol\ns2\tU\tcontrol\ns3\tF\tcontrol\n"
    g.sample_annot["sex"] = np.array(["M", "x", "F"], dtype=object)
    with pytest.raises(ValueError, match='The gender variable in GDS file should be either "M" or "F".'):
        S.snpgdsGDS2Eigen(g, fn, verbose=False)


# ---- the HapMap fixture ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hap():
    S = _pkg()
    g = S.api.snpgdsOpen(HAPMAP)
    geno = g.read_genotype()                                                    # SNP x sample
    rng = np.random.default_rng(5)
    samp = np.sort(rng.choice(g.n_samp, 77, replace=False))
    snp = np.sort(rng.choice(g.n_snp, 1031, replace=False))
    return g, geno, samp, snp


@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("fmt", ["A/G/C/T", "A/B", "1/2"])
def test_hapmap_ped(tmp_path, hap, fmt, subset):
    S = _pkg()
    g, geno, samp, snp = hap
    fn = str(tmp_path / "h")
    if subset:
        # the wanted ids in another order: the files follow FILE order
        S.snpgdsGDS2PED(g, fn, sample_id=g.sample_id[samp][::-1], snp_id=g.snp_id[snp][::-1], format=fmt, verbose=False)
        si, ki = samp, snp
    else:
        S.snpgdsGDS2PED(g, fn, format=fmt, verbose=False)
        si, ki = np.arange(g.n_samp), np.arange(g.n_snp)
    want = R.ped_text(g.sample_id[si], g.snp_allele[ki], geno[np.ix_(ki, si)].T, FMT[fmt])
    assert _read(fn + ".ped") == want
    assert _read(fn + ".map").decode() == R.map_text(g.snp_chromosome[ki], g.snp_rs_id[ki], g.snp_position[ki])


def test_hapmap_rs_id_both_ways_on_a_gds_file(tmp_path, hap):
    S = _pkg()
    g, geno, samp, snp = hap
    assert g.snp_rs_id is not None and str(g.snp_rs_id[0]).startswith("rs")
    fn = str(tmp_path / "r")
    # the name of a GDS file: opened as a stream
    S.snpgdsGDS2PED(HAPMAP, fn, snp_id=g.snp_id[snp], sample_id=g.sample_id[samp], use_snp_rsid=False, format="1/2", verbose=False)
    assert _read(fn + ".map").decode() == R.map_text(g.snp_chromosome[snp], g.snp_id[snp], g.snp_position[snp])
    assert _read(fn + ".ped") == R.ped_text(g.sample_id[samp], None, geno[np.ix_(snp, samp)].T, 3)
    S.snpgdsGDS2PED(HAPMAP, fn, snp_id=g.snp_id[snp], sample_id=g.sample_id[samp], use_snp_rsid=True, format="1/2", verbose=False)
    assert _read(fn + ".map").decode() == R.map_text(g.snp_chromosome[snp], g.snp_rs_id[snp], g.snp_position[snp])


@pytest.mark.parametrize("subset", [False, True])
def test_hapmap_eigen(tmp_path, hap, subset):
    S = _pkg()
    g, geno, samp, snp = hap
    fn = str(tmp_path / "e")
    if subset:
        S.snpgdsGDS2Eigen(g, fn, sample_id=g.sample_id[samp], snp_id=g.snp_id[snp], verbose=False)
        si, ki = samp, snp
    else:
        S.snpgdsGDS2Eigen(g, fn, verbose=False)
        si, ki = np.arange(g.n_samp), np.arange(g.n_snp)
    assert _read(fn + ".eigenstratgeno") == R.eigen_text(geno[np.ix_(ki, si)])
    assert _read(fn + ".snp").decode() == R.snp_text(g.snp_id[ki], g.snp_chromosome[ki], g.snp_position[ki])
    assert _read(fn + ".ind").decode() == R.ind_text(g.sample_id[si], g.sample_annot["sex"][si])


def test_small_stage_runs_windows_of_one_line(tmp_path, hap, monkeypatch):
    """a stage smaller than a line: every window holds one line, and there are three or more of them"""
    S = _pkg()
    from snprelate_amd import text as T
    g, geno, samp, snp = hap
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", "100")
    fn = str(tmp_path / "w")
    s5, k9 = samp[:5], snp[:90]
    S.snpgdsGDS2PED(g, fn, sample_id=g.sample_id[s5], snp_id=g.snp_id[k9], verbose=False)
    assert _read(fn + ".ped") == R.ped_text(g.sample_id[s5], g.snp_allele[k9], geno[np.ix_(k9, s5)].T, 1)
    S.snpgdsGDS2Eigen(g, fn, sample_id=g.sample_id[samp], snp_id=g.snp_id[k9[:7]], verbose=False)
    assert _read(fn + ".eigenstratgeno") == R.eigen_text(geno[np.ix_(k9[:7], samp)])
    samp_flag, snp_flag = np.isin(np.arange(g.n_samp), s5), np.isin(np.arange(g.n_snp), k9)
    with open(fn + ".x", "wb") as f:
        assert T.write_ped(f, g, samp_flag, snp_flag, ["i"] * 5, S._lib.TEXT_PED_AB) == 5
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", str(2 * (13 + 4 * 90 + 1) + 100))       # two lines of 374 bytes fit, three do not
    with open(fn + ".x", "wb") as f:
        assert T.write_ped(f, g, samp_flag, snp_flag, ["i"] * 5, S._lib.TEXT_PED_AB) == 3
    assert _read(fn + ".x") == R.ped_text(["i"] * 5, None, geno[np.ix_(k9, s5)].T, 2)


# ---- synthetic shapes through the ABI call -------------------------------------------------------------------------------------------
GUARD = 4096


class _Guarded:
    """a device text buffer of n bytes that starts `phase` bytes behind a 256-byte boundary, 0xA5 everywhere, guards either side"""

    def __init__(self, n, phase):
        import torch
        self.buf = torch.full((GUARD + 256 + phase + n + GUARD + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        base = int(self.buf.data_ptr())
        self.start = (-(base + GUARD)) % 256 + GUARD + phase
        assert (base + self.start) % 256 == phase
        self.ptr, self.n = base + self.start, n

    def read(self):
        import torch
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        assert (a[:self.start] == 0xA5).all() and (a[self.start + self.n:] == 0xA5).all(), "a store outside the text"
        return a[self.start:self.start + self.n].tobytes()


def _alleles(rng, n_cols, kind):
    """2 n_cols pieces: 'one' one-byte alleles; 'mixed' one-byte ones, indels of 2 ... 40 bytes, "0" for an empty one, and one
    allele of 5 000 bytes"""
    letters = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for i in range(2 * n_cols):
        u = rng.random()
        if kind == "one" or u < 0.5:
            out.append(bytes(rng.choice(letters, 1)))
        elif u < 0.6:
            out.append(b"0")
        else:
            out.append(bytes(rng.choice(letters, int(rng.integers(2, 41)))))
    if kind == "mixed":
        out[int(rng.integers(0, 2 * n_cols))] = bytes(rng.choice(letters, 5000))
    return out


def _expected(codes, fmt, alleles, prefixes):
    lines = []
    for r, row in enumerate(codes):
        s = prefixes[r] if prefixes else b""
        for c, g in enumerate(row):
            if fmt == 0:
                s += b"0129"[g:g + 1]
            elif g == 3:
                s += b"\t0 0"
            else:
                s1, s2 = ((b"A", b"B") if fmt == 1 else (b"1", b"2") if fmt == 2 else (alleles[2 * c], alleles[2 * c + 1]))
                s += b"\t" + (s2 if g == 0 else s1) + b" " + (s1 if g == 2 else s2)
        lines.append(s + b"\n")
    return lines


def _render(codes, fmt, alleles, prefixes, phase):
    import torch
    L = _pkg()._lib
    from snprelate_amd.gds import pack_2bit_rows
    n_rows, n_cols = codes.shape
    # the rows one byte behind an aligned address: the kernels load aligned dwords around unaligned rows
    packed = pack_2bit_rows(codes.astype(np.uint8))
    dev = torch.zeros(packed.size + 1, dtype=torch.uint8, device="cuda")
    dev[1:].copy_(torch.from_numpy(packed.reshape(-1)))
    rows = int(dev.data_ptr()) + 1
    size = L.text_render(rows, n_rows, n_cols, fmt, alleles=alleles, prefixes=prefixes)
    g = _Guarded(int(size[-1]), phase)
    off = L.text_render(rows, n_rows, n_cols, fmt, alleles=alleles, prefixes=prefixes, text=g.ptr)
    text = g.read()
    assert np.array_equal(size, off), "the sizing call differs from the writing call"
    st = L.text_stats()
    assert st["text_bytes"] == size[-1] and st["launches"] >= 1
    return text, off


@pytest.mark.parametrize("n_rows", [1, 5, 70])
@pytest.mark.parametrize("n_cols", [1, 3, 4, 5, 63, 64, 65, 257, 1031])
def test_shapes_every_format(n_rows, n_cols):
    rng = np.random.default_rng(1000 * n_rows + n_cols)
    codes = rng.integers(0, 4, (n_rows, n_cols))
    codes[n_rows // 2] = 3                                                     # a row that is all missing
    # prefixes of 0 ... 40 bytes; behind row 40 a length that makes a four-byte-per-column line 1 mod 16 bytes long, so that with 70
    # rows the line starts step through every residue mod 16
    plen = [r if r <= 40 else (-4 * n_cols) % 16 + 16 * (r % 2) for r in range(n_rows)]
    prefixes = [bytes(rng.integers(0x21, 0x7F, k, dtype=np.uint8)) for k in plen]
    starts = set()
    phase = 1 + (n_rows + n_cols) % 15
    for fmt, alleles, pre in ((0, None, None), (0, None, prefixes), (1, None, prefixes), (2, None, None), (2, None, prefixes),
                              (3, _alleles(rng, n_cols, "one"), prefixes), (3, _alleles(rng, n_cols, "mixed"), prefixes),
                              (3, _alleles(rng, n_cols, "mixed"), None)):
        want = _expected(codes, fmt, alleles, pre)
        text, off = _render(codes, fmt, alleles, pre, phase)
        assert text == b"".join(want), (fmt, pre is not None)
        assert list(np.diff(off)) == [len(x) for x in want]
        if fmt == 1:
            starts = {(phase + int(o)) % 16 for o in off[:-1]}
    if n_rows == 70:
        assert len(starts) == 16


def test_render_is_a_pure_function_of_its_input():
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 4, (33, 300))
    al = _alleles(rng, 300, "mixed")
    pre = [b"p%d" % i for i in range(33)]
    a, _ = _render(codes, 3, al, pre, 7)
    b, _ = _render(codes, 3, al, pre, 12)
    assert a == b


def test_bed_and_vcf_objects_go_out_too(tmp_path):
    """the other kinds of SNP GDS object: a BedStream (alleles and rs ids from the .bim) and the VCF GenoFile (text chromosomes)"""
    S = _pkg()
    fix = [os.path.join(GOLDEN, "plinkhapmap.%s.gz" % e) for e in ("bed", "fam", "bim")]
    bs = S.snpgdsOpenBED(fix[0], fix[1], fix[2], verbose=False)
    geno = bs.read_genotype()
    fn = str(tmp_path / "b")
    S.snpgdsGDS2PED(bs, fn, verbose=False)
    assert _read(fn + ".ped") == R.ped_text(bs.sample_id, bs.snp_allele, geno.T, 1)
    rs = bs.snp_id if bs.snp_rs_id is None else bs.snp_rs_id
    assert _read(fn + ".map").decode() == R.map_text(bs.snp_chromosome, rs, bs.snp_position)
    vcf = S.snpgdsOpenVCF(os.path.join(GOLDEN, "sequence.vcf"), method="copy.num.of.ref", verbose=False)
    S.snpgdsGDS2Eigen(vcf, fn, verbose=False)
    assert _read(fn + ".eigenstratgeno") == R.eigen_text(vcf.read_genotype())
    assert _read(fn + ".snp").decode() == R.snp_text(vcf.snp_id, vcf.snp_chromosome, vcf.snp_position)
    S.snpgdsGDS2PED(vcf, fn, verbose=False)
    assert _read(fn + ".ped") == R.ped_text(vcf.sample_id, vcf.snp_allele, vcf.read_genotype().T, 1)
    assert _read(fn + ".map").decode() == R.map_text(vcf.snp_chromosome, vcf.snp_rs_id, vcf.snp_position)
