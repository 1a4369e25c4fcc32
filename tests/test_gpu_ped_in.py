"""GPU tests of the PED reader (snpgpu_ped_tokens / _census / _codes, ped.PedReader, snpgdsOpenPED): the opened object equals the
restatement of gnrParsePED (tests/text_ref.py) exactly -- alleles, genotypes, annotations -- with NO line flagged on any
regular-grammar text, which keeps the kernel from handing its work to the host; irregular lines come out the same through the
flags and the host, or raise the reference's message; the HapMap fixture survives snpgdsGDS2PED -> snpgdsOpenPED."""
import gzip
import os

import numpy as np
import pytest

import text_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HAPMAP = os.path.join(GOLDEN, "hapmap_geno.gds")


def _pkg():
    import snprelate_amd
    return snprelate_amd


def _write(tmp_path, text, chrom=None, pos=None, name="p", gz=False, n_snp=None):
    """a .ped (bytes) and its .map; chrom / pos default to chromosome 1, positions 1, 2, ..."""
    fn = str(tmp_path / name)
    ped = fn + (".ped.gz" if gz else ".ped")
    with (gzip.open(ped, "wb") if gz else open(ped, "wb")) as f:
        f.write(text)
    M = n_snp if chrom is None else len(chrom)
    chrom = ["1"] * M if chrom is None else chrom
    pos = list(range(1, M + 1)) if pos is None else pos
    with open(fn + ".map", "w") as f:
        for j in range(M):
            f.write("%s\trs%d\t0\t%d\n" % (chrom[j], j, pos[j]))
    return ped, fn + ".map"


def _same(gf, d, family=True):
    assert list(gf.snp_allele) == d["allele"]
    assert np.array_equal(gf.read_genotype(), d["geno"].T)
    assert list(gf.sample_id) == d["sample_id"]
    if family:
        for k in ("family", "father", "mother", "sex", "phenotype"):
            assert list(gf.sample_annot[k]) == d[k], k
    else:
        assert gf.sample_annot == {}


# ---- the literal ------------------------------------------------------------------------------------------------------------------
PED_IN = (b"F1\ts1\t0\t0\t1\t-9\tA G\tT T\t0 0\n"
          b"F1 s2 s1 0 2 1  G G T C C 0\n"
          b"F2\ts3\t0\t0\t0\t2\tA A\tT T\tC C\n")


def test_literal(tmp_path):
    S = _pkg()
    ped, mp = _write(tmp_path, PED_IN, n_snp=3)
    gf = S.snpgdsOpenPED(ped, mp, verbose=False)
    assert list(gf.snp_allele) == ["A/G", "T/C", "C/0"]
    assert gf.read_genotype().T.tolist() == [[1, 2, 3], [0, 1, 3], [2, 2, 2]]
    assert list(gf.sample_annot["sex"]) == ["M", "F", "0"] and list(gf.sample_annot["phenotype"]) == ["-9", "1", "2"]
    assert gf.ped_flagged_lines == 0                                           # line 2's double space is regular
    assert list(gf.snp_id) == [1, 2, 3] and list(gf.snp_rs_id) == ["rs0", "rs1", "rs2"] and list(gf.snp_position) == [1, 2, 3]
    _same(gf, R.parse_ped(PED_IN, 3))
    _same(S.snpgdsOpenPED(ped, mp, family=False, verbose=False), R.parse_ped(PED_IN, 3), family=False)


# ---- regular grammar ---------------------------------------------------------------------------------------------------------------
def _sep(rng, kind):
    if kind == "tab":
        return "\t"
    if kind == "space":
        return " "
    if kind == "spaces":
        return " " * int(rng.integers(1, 4))
    return ["\t", " ", "  ", "   "][int(rng.integers(0, 4))]


def _make(rng, N, M, letters, kind, missing=0.08, newline="\n", final_newline=True, trailing=False):
    """a regular .ped text: per SNP two letters, per sample two alleles (or "0" "0", or one "0"), every separator drawn by kind"""
    pair = [rng.choice(len(letters), 2, replace=False) for _ in range(M)]
    freq = rng.random(M)
    lines = []
    for i in range(N):
        cells = ["F%d" % (i // 3), "s%d" % i, "0", "s%d" % (i - 1) if i % 4 == 3 else "0", "120"[i % 3], ["-9", "1", "2"][i % 3]]
        u = rng.random((M, 3))
        for j in range(M):
            a = letters[pair[j][int(u[j, 0] < freq[j])]]
            b = letters[pair[j][int(u[j, 1] < freq[j])]]
            if u[j, 2] < missing:
                a, b = ("0", "0") if u[j, 2] < missing / 2 else (a, "0")
            cells += [a, b]
        s = cells[0]
        for c in cells[1:]:
            s += _sep(rng, kind) + c
        if trailing and i % 2:
            s += "  "
        lines.append(s)
    text = newline.join(lines) + (newline if final_newline else "")
    return text.encode()


@pytest.mark.parametrize("N", [1, 5, 70])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 1023, 1024, 1025, 2100])
def test_regular_texts_equal_the_restatement_and_flag_nothing(tmp_path, N, M):
    S = _pkg()
    case = [1, 3, 4, 5, 1023, 1024, 1025, 2100].index(M) * 3 + [1, 5, 70].index(N)
    rng = np.random.default_rng(100 + case)
    kind = ["tab", "space", "spaces", "mix"][case % 4]
    letters = ["ACGT", "12", "AB"][case % 3]
    text = _make(rng, N, M, letters, kind, newline="\r\n" if case % 5 == 0 else "\n", final_newline=case % 2 == 0,
                 trailing=kind != "tab")
    ped, mp = _write(tmp_path, text, n_snp=M)
    gf = S.snpgdsOpenPED(ped, mp, verbose=False)
    assert gf.ped_flagged_lines == 0
    _same(gf, R.parse_ped(text, M))


def test_every_separator_and_letter_set(tmp_path):
    """the cross of the separator kinds and the letter sets at one size whose lines cross a chunk boundary"""
    S = _pkg()
    for k, kind in enumerate(["tab", "space", "spaces", "mix"]):
        for q, letters in enumerate(["ACGT", "12", "AB"]):
            rng = np.random.default_rng(10 * k + q)
            text = _make(rng, 4, 1100, letters, kind, trailing=True)
            ped, mp = _write(tmp_path, text, n_snp=1100, name="c%d%d" % (k, q))
            gf = S.snpgdsOpenPED(ped, mp, verbose=False)
            assert gf.ped_flagged_lines == 0
            _same(gf, R.parse_ped(text, 1100))


def test_small_stage_gz_and_ibs(tmp_path, monkeypatch):
    """a .gz file read in chunks far smaller than the file: both sweeps run over three or more windows; the opened object goes
    straight into snpgdsIBSNum"""
    S = _pkg()
    from snprelate_amd.gds import GenoFile
    rng = np.random.default_rng(7)
    N, M = 40, 300
    text = _make(rng, N, M, "ACGT", "mix")
    ped, mp = _write(tmp_path, text, n_snp=M, gz=True)
    monkeypatch.setenv("SNPGPU_TEXT_STAGE_BYTES", str(len(text) // 5))
    gf = S.snpgdsOpenPED(ped, mp, verbose=False)
    assert gf.ped_windows >= 3 and gf.ped_flagged_lines == 0
    d = R.parse_ped(text, M)
    _same(gf, d)
    monkeypatch.delenv("SNPGPU_TEXT_STAGE_BYTES")
    want = GenoFile(genotype=d["geno"].T.copy(), sample_id=d["sample_id"], snp_position=np.arange(1, M + 1))
    a = S.api.snpgdsIBSNum(gf, autosome_only=False, remove_monosnp=False, verbose=False)
    b = S.api.snpgdsIBSNum(want, autosome_only=False, remove_monosnp=False, verbose=False)
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(a[k], b[k])


# ---- irregular texts ----------------------------------------------------------------------------------------------------------------
def test_indels_quotes_and_empty_tokens_through_the_host(tmp_path):
    S = _pkg()
    rng = np.random.default_rng(3)
    N, M = 12, 40
    lines = _make(rng, N, M, "ACGT", "tab").split(b"\n")[:-1]

    def cells(i):
        return lines[i].split(b"\t")

    def put(i, c):
        lines[i] = b"\t".join(c)
    c = cells(1); c[6 + 2 * 3] = b"AT"; c[6 + 2 * 3 + 1] = b"ATT"; put(1, c)           # indels at SNP 3
    c = cells(4); c[6 + 2 * 3] = b"AT"; c[6 + 2 * 7] = b"\"G\""; c[6 + 2 * 8] = b"'TT'"; put(4, c)      # quoted tokens
    c = cells(6); c[6 + 2 * 9] = b""; put(6, c)                                        # \t\t: the allele ""
    lines[8] = lines[8].replace(b"\t", b" ", 9) + b"   "                               # (regular: spaces and trailing spaces)
    c = cells(10); c[6 + 2 * 3] = b"AT"; c[6 + 2 * 3 + 1] = b"AT"; put(10, c)
    text = b"\n".join(lines) + b"\n"
    ped, mp = _write(tmp_path, text, n_snp=M)
    gf = S.snpgdsOpenPED(ped, mp, verbose=False)
    assert gf.ped_flagged_lines == 4                                           # exactly the planted lines, mixed with unflagged ones
    d = R.parse_ped(text, M)
    _same(gf, d)
    assert "AT" in d["allele"][3].replace("/", ",").split(",") and "ATT" in d["allele"][3].replace("/", ",").split(",")
    assert "" in d["allele"][9].replace("/", ",").split(",")                   # the empty cell of \t\t is an allele, as in the reference


@pytest.mark.parametrize("what", ["fewer", "more", "blank", "tab_at_end", "head"])
def test_wrong_counts_raise_the_reference_message(tmp_path, what):
    S = _pkg()
    rng = np.random.default_rng(11)
    N, M = 9, 30
    lines = _make(rng, N, M, "ACGT", "tab").split(b"\n")[:-1]
    if what == "fewer":
        lines[5] = lines[5].rsplit(b"\t", 1)[0]
    elif what == "more":
        lines[5] += b"\tC"
    elif what == "blank":
        lines.insert(5, b"")
    elif what == "tab_at_end":
        lines[5] += b"\t"
    else:
        lines[5] = b"F\ts\t0"
    lines[7] = lines[7].rsplit(b"\t", 2)[0]                                    # a later bad line: the first one is reported
    text = b"\n".join(lines) + b"\n"
    with pytest.raises(R.PedError) as ref:
        R.parse_ped(text, M)
    e = ref.value
    assert e.line == 6
    assert e.message == ("more columns than what expected." if what in ("more", "tab_at_end") else "fewer columns than what expected.")
    ped, mp = _write(tmp_path, text, n_snp=M)
    with pytest.raises(ValueError) as got:
        S.snpgdsOpenPED(ped, mp, verbose=False)
    assert str(got.value) == "%s\nFILE: %s\nLINE: %d, COLUMN: %d, %s\n" % (e.message, ped, e.line, e.column, e.cell.decode())
    if what == "fewer":
        assert e.column == 6 + 2 * M
    if what == "blank":
        assert e.column == 1


def test_unsorted_map_permutes_alleles_with_the_rest(tmp_path):
    S = _pkg()
    rng = np.random.default_rng(13)
    N, M = 10, 25
    text = _make(rng, N, M, "ACGT", "space")
    chrom = [["2", "1", "X", "10", "NA"][j % 5] for j in range(M)]
    pos = [int(x) for x in rng.integers(1, 50, M)]
    ped, mp = _write(tmp_path, text, chrom=chrom, pos=pos)
    ii, col = R.map_order(chrom, pos)
    assert ii != sorted(ii)
    gf = S.snpgdsOpenPED(ped, mp, verbose=False)
    d = R.parse_ped(text, M, ii)
    _same(gf, d)
    assert d["allele"] == [d["allele_file"][k] for k in ii] and d["allele"] != d["allele_file"]
    assert list(gf.snp_rs_id) == ["rs%d" % k for k in ii] and list(gf.snp_position) == [pos[k] for k in ii]
    assert list(gf.snp_chromosome) == col and list(gf.snp_id) == list(range(1, M + 1))


# ---- HapMap: snpgdsGDS2PED -> snpgdsOpenPED ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["A/G/C/T", "1/2", "A/B"])
def test_hapmap_round_trip(tmp_path, fmt):
    S = _pkg()
    g = S.api.snpgdsOpen(HAPMAP)
    geno = g.read_genotype().astype(np.int64)                                  # SNP x sample
    geno[5] = 3                                                                # an all-missing SNP
    geno[6][geno[6] != 3] = 2                                                  # monomorphic SNPs, one of each allele
    geno[7][geno[7] != 3] = 0
    from snprelate_amd.gds import GenoFile
    src = GenoFile(genotype=geno.astype(np.uint8), sample_id=g.sample_id, snp_id=g.snp_id, snp_chromosome=g.snp_chromosome,
                   snp_position=g.snp_position, snp_allele=g.snp_allele)
    fn = str(tmp_path / "h")
    S.snpgdsGDS2PED(src, fn, format=fmt, verbose=False)
    gf = S.snpgdsOpenPED(fn + ".ped", fn + ".map", verbose=False)
    assert gf.ped_flagged_lines == 0 and list(gf.sample_id) == list(g.sample_id)

    # what must come back, from the original genotypes and the tie rule
    chrom = ["X" if c == 23 else str(c) for c in g.snp_chromosome]
    ii, col = R.map_order(chrom, [int(p) for p in g.snp_position])
    called = geno != 3
    n1, n2 = np.where(called, geno, 0).sum(1), np.where(called, 2 - geno, 0).sum(1)    # copies of s1 and of s2
    alleles, want = [], np.empty_like(geno)
    for j in range(g.n_snp):
        s1, s2 = {"A/G/C/T": str(g.snp_allele[j]).split("/"), "1/2": ["1", "2"], "A/B": ["A", "B"]}[fmt]
        cnt = {k: v for k, v in ((s1, int(n1[j])), (s2, int(n2[j]))) if v > 0}
        if not cnt:
            alleles.append("0/0")
            want[j] = 3
            continue
        ref = min(cnt, key=lambda k: (-cnt[k], k.encode()))
        other = [k for k in cnt if k != ref]
        alleles.append(ref + "/" + (other[0] if other else "0"))
        want[j] = np.where(called[j], geno[j] if ref == s1 else 2 - geno[j], 3)
    assert alleles[5] == "0/0" and alleles[6].endswith("/0") and alleles[7].endswith("/0")
    assert list(gf.snp_allele) == [alleles[k] for k in ii]
    assert np.array_equal(gf.read_genotype(), want[ii].astype(np.uint8))
    assert list(gf.snp_rs_id) == [str(g.snp_id[k]) for k in ii] and list(gf.snp_chromosome) == col
