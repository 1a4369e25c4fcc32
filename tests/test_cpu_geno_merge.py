"""CPU tests of the merging of data sets (no device): the restatements of tests/geno_merge_ref.py reproduce hand-written cases; the
package's allele-strand rules, intersect and switch decision equal them and the table of the rules; the header declares the new
calls without a result memory kind; every refusal of snpgpu_geno_merge that needs no device returns its message; without a device
the genotype-moving functions fail loudly."""
import ctypes
import os

import numpy as np
import pytest

import geno_merge_ref as R
import geno_select_ref as S
import mem_kinds as M
from conftest import ROOT
from snprelate_amd import _lib, merge
from snprelate_amd.gds import GenoFile

NA = R.NA
NAN = float("nan")


# ---- the restatement of snpgpu_geno_merge against hand-written bytes -------------------------------------------------------------------
def _part(g, **kw):
    data, d = S.make_stream(np.asarray(g, np.uint8), "packed")
    return dict(data=data, kw=d, **kw)


def test_restatement_reproduces_hand_written_rows():
    a = [[0, 1, 2], [3, 0, 1]]                       # 3 samples
    b = [[2, 2], [1, 3]]                             # 2 samples
    got = R.merge_ref([_part(a), _part(b, flip=[1, 0])])
    # row 0: 0 1 2 | flip(2 2) = 0 0 -> codes 0 1 2 0 0 pad pad pad: bytes 0b00100100, 0b11111100
    # row 1: 3 0 1 | 1 3           -> codes 3 0 1 1 3 pad pad pad: bytes 0b01010011, 0b11111111
    assert got.tolist() == [[0b00100100, 0b11111100], [0b01010011, 0b11111111]]
    # a permuted, repeated SNP list and a sample list; missing stays missing under a flip
    got = R.merge_codes([_part(a, snp_index=[1, 1, 0], samp_index=[2, 0], flip=[1, 0, 1]), _part(b, snp_index=[0, 1, 1])])
    assert got.tolist() == [[1, 3, 2, 2], [1, 3, 1, 3], [0, 2, 1, 3]]
    assert R.flip_codes(np.array([0, 1, 2, 3])).tolist() == [2, 1, 0, 3]


def test_the_flip_bit_operation_of_the_kernel_is_the_flip():
    x = np.arange(256, dtype=np.uint32)                                   # every byte of 4 codes
    y = x ^ ((~x & 0x55) << 1)
    want = S.pack_ref(R.flip_codes(R.unpack_ref(x.astype(np.uint8)[:, None], 4)))[:, 0]
    assert np.array_equal(y.astype(np.uint8), want)


# ---- the allele-strand rules ---------------------------------------------------------------------------------------------------------
TABLE = [
    ("A/G", "A/G", 0.2, 0.2, 0),
    ("A/G", "G/A", 0.2, 0.8, 1),
    ("A/G", "T/C", 0.2, 0.2, 2),
    ("A/G", "C/T", 0.2, 0.8, 3),
    ("A/G", "A/C", 0.2, 0.2, NA),
    ("C/G", "C/G", 0.2, 0.3, 4),
    ("C/G", "C/G", 0.2, 0.7, 5),
    ("C/G", "G/C", 0.2, 0.3, 4),
    ("C/G", "G/C", 0.2, 0.7, 5),
    ("C/G", "C/G", 0.5, 0.5, 4),                      # 0.5 is side 0
    ("A/T", "A/T", 0.2, NAN, 5),                      # a NaN frequency counts as side 1
    ("A/T", "T/A", 0.7, NAN, 4),
    ("A/T", "A/T", NAN, NAN, 4),
    ("a/g", "A/G", 0.2, 0.2, 0),
    ("A,G", "A/G", 0.2, 0.2, 0),
    ("A/G,T", "A/G,T", 0.2, 0.2, 0),                  # the first '/' wins over a ','
    ("AT/A", "AT/A", 0.2, 0.2, 0),
    ("AT/A", "A/AT", 0.2, 0.2, 1),
    ("AT/A", "TA/T", 0.2, 0.2, NA),                   # indels have no complement
    ("A", "A", 0.2, 0.2, 0),
    ("A", "T", 0.2, 0.2, NA),
    ("A/G", "A", 0.2, 0.2, NA),
]


@pytest.mark.parametrize("a1,a2,f1,f2,want", TABLE)
def test_allele_strand_table(a1, a2, f1, f2, want):
    assert R.strand_flags([a1], [a2], [f1], [f2])[0] == want
    got = merge.allele_strand([a1], [a2], [f1], [f2], same_strand=False)
    assert got.dtype == np.int32 and got[0] == want


def test_same_strand_gives_only_0_1_na():
    al1, al2, f1, f2 = ([t[k] for t in TABLE] for k in range(4))
    got = merge.allele_strand(al1, al2, f1, f2, same_strand=True)
    assert np.array_equal(got, R.strand_flags(al1, al2, f1, f2, True))
    assert set(got.tolist()) == {0, 1, NA}
    assert got[:5].tolist() == [0, 1, NA, NA, NA] and got[5:9].tolist() == [0, 0, 1, 1]


def test_allele_strand_equals_the_restatement_on_every_pair_of_names():
    names = ["A", "C", "G", "T", "AT", ""]
    al = ["%s/%s" % (x, y) for x in names for y in names]
    al1 = [a for a in al for _ in al]
    al2 = [b for _ in al for b in al]
    for f1, f2 in ((0.2, 0.3), (0.2, 0.9), (NAN, 0.1)):
        n = len(al1)
        assert np.array_equal(merge.allele_strand(al1, al2, [f1] * n, [f2] * n), R.strand_flags(al1, al2, [f1] * n, [f2] * n))


# ---- intersect -----------------------------------------------------------------------------------------------------------------------
def _lst(snp_id, chrom, pos, allele, afreq):
    return merge.SNPList(snp_id=np.array(snp_id), chromosome=np.array(chrom), position=np.array(pos), allele=np.array(allele),
                         afreq=np.array(afreq, float))


L1 = _lst([1, 2, 3, 4, 5, 6], [1, 1, 1, 2, 2, 1], [10, 20, 10, 5, 7, 30], ["A/G", "C/T", "G/A", "A/C", "C/G", "A/G"], [.1, .2, .3, .4, .2, .1])
L2 = _lst([9, 8, 7, 6, 5], [2, 1, 1, 2, 1], [7, 30, 10, 5, 10], ["G/C", "A/T", "G/A", "C/A", "A/G"], [.9, .1, .3, .4, .2])


def test_intersect_position_order_duplicates_and_na_rm():
    rv = merge.snp_list_intersect([L1, L2], na_rm=False)
    # list 1's order, its duplicate 1:10 once (the first occurrence on both sides); 1:20 is not in list 2
    assert rv["idx1"].tolist() == [0, 3, 4, 5] and rv["idx2"].tolist() == [2, 3, 0, 1]
    assert rv["flag2"].tolist() == [1, 1, 5, NA] and rv["flag2"].dtype == np.int32 and rv["idx1"].dtype == np.int32
    rm = merge.snp_list_intersect([L1, L2], na_rm=True)
    assert rm["idx1"].tolist() == [0, 3, 4] and rm["idx2"].tolist() == [2, 3, 0] and rm["flag2"].tolist() == [1, 1, 5]
    for na_rm in (False, True):
        for same in (False, True):
            want = R.intersect_ref([L1, L2], "position", na_rm, same)
            got = merge.snp_list_intersect([L1, L2], na_rm=na_rm, same_strand=same)
            assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)


def test_intersect_exact_and_three_lists():
    L3 = _lst([1, 5, 6], [1, 2, 1], [10, 7, 30], ["A/G", "C/G", "A/G"], [.1, .2, .9])
    rv = merge.snp_list_intersect([L1, L3], method="exact")
    assert sorted(rv) == ["idx1", "idx2"] and rv["idx1"].tolist() == [0, 4, 5] and rv["idx2"].tolist() == [0, 1, 2]
    rv = merge.snp_list_intersect([L1, L2, L3], na_rm=False)
    want = R.intersect_ref([L1, L2, L3], "position", False, False)
    assert sorted(rv) == ["flag2", "flag3", "idx1", "idx2", "idx3"] and all(np.array_equal(rv[k], want[k]) for k in want)
    assert rv["idx1"].tolist() == [0, 4, 5] and rv["flag3"].tolist() == [0, 4, 0]
    from snprelate_amd import snpgdsSNPListIntersect
    assert snpgdsSNPListIntersect(L1, L2, L3, na_rm=False, verbose=False)["idx3"].tolist() == [0, 1, 2]
    with pytest.raises(TypeError, match="All objects should be 'snpgdsSNPListClass'."):
        snpgdsSNPListIntersect(L1, dict(L2))
    with pytest.raises(ValueError, match="'arg' should be one of"):
        snpgdsSNPListIntersect(L1, L2, method="rs")


def test_switch_decision():
    al = ["A/G", "C/T", "G/T/C", "a/g", "A", "AT/A"]
    want = ["G", None, "T/C", "G", "A", "A"]
    flags, new = merge.switch_flags(al, want)
    rf, rn = R.switch_ref(al, want)
    assert np.array_equal(flags, rf) and list(new) == rn
    assert flags.tolist() == [1, NA, 1, NA, 0, 1] and list(new) == ["G/A", "C/T", "T/C/G", "a/g", "A", "A/AT"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_no_result_memory_kind():
    text = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    protos = M.header_prototypes(text)
    for f in ("snpgpu_geno_merge", "snpgpu_geno_merge_stats"):
        assert f in protos and f in _lib.EXPORTS and hasattr(_lib.lib(), f)
        assert not {"out_mem", "dst_mem", "mem"} & set(protos[f])
    assert protos["snpgpu_geno_merge"] == ["parts", "n_parts", "n_snp_out", "rows", "device", "stream"]
    assert "typedef struct snpgpu_merge_part {" in text and "SNPGPU_MERGE_STAGE_BYTES" in text
    assert _lib.lib().snpgpu_abi_version() == 2
    assert ctypes.sizeof(_lib.MergePart) == ctypes.sizeof(_lib.GenoSrc) + 32 and _lib.lib().snpgpu_geno_merge_stats(None) != 0
    assert not any("oracle" in open(os.path.join(ROOT, "snprelate_amd", f)).read() for f in ("merge.py",))


G = np.zeros((3, 2), np.uint8)                       # 3 SNP rows of 2 bytes: up to 8 samples


def _p(**kw):
    a = dict(src=G, major=0, n_rows=3, n_cols=5, row_stride_bits=16)
    a.update(kw)
    return _lib.merge_part(**a)


@pytest.mark.parametrize("parts,kw,message", [
    ([_p()], dict(rows=0), "NULL argument: rows is NULL"),
    ([], dict(n_snp_out=3), r"invalid n_parts \(at least one part\)"),
    ([_p(src=0, n_bytes=6)], {}, "part 0: NULL argument: src->bits is NULL"),
    ([_p(), _p(samp_index=[])], {}, r"part 1: invalid number of samples \(1 ... 2\^30 - 1\)"),
    ([_p(snp_index=[])], dict(n_snp_out=0), "part 0: invalid number of SNPs: no SNP in the working dataset"),
    ([_p(), _p(samp_index=[0, 5])], {}, r"part 1: an index outside the source: samp_index\[1\]"),
    ([_p(samp_index=[-1])], {}, r"part 0: an index outside the source: samp_index\[0\]"),
    ([_p(), _p(snp_index=[0, 1, 3])], {}, r"part 1: an index outside the source: snp_index\[2\]"),
    ([_p(), _p(n_rows=2)], {}, "part 1: snp_index is NULL: n_snp_out should be the source's number of SNPs"),
    ([_p(major=2)], {}, "part 0: invalid major"),
    ([_p(mem=7)], {}, "part 0: invalid memory kind"),
    ([_p(bit0=1)], {}, "part 0: odd or negative bit position: bit0"),
    ([_p(row_stride_bits=15)], {}, "part 0: odd or negative bit position: row_stride_bits"),
    ([_p(n_cols=9)], {}, "part 0: an element outside n_bytes: row 2 ends beyond the source"),
    ([_p(row_bit=[0, 16, 40], row_stride_bits=0)], {}, "part 0: an element outside n_bytes: row 2 ends beyond the source"),
    ([_p(n_bytes=0)], {}, "part 0: invalid n_bytes"),
])
def test_merge_refusals_touch_no_device(parts, kw, message):
    a = dict(rows=4096)
    a.update(kw)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_geno_merge: " + message):
        _lib.geno_merge(parts, a["rows"], n_snp_out=a.get("n_snp_out"))


def test_merge_refuses_null_parts_and_too_many_samples_without_a_device():
    L = _lib.lib()
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_geno_merge: NULL argument: parts is NULL"):
        _lib.check(L.snpgpu_geno_merge(None, 1, 3, ctypes.c_void_p(4096), 0, None))
    # two parts of 2^29 samples each name 2^30 in all: their descriptions are checked by arithmetic, nothing that size is touched
    n = 1 << 29
    big = dict(src=4096, major=0, n_rows=1, n_cols=n, n_bytes=n // 4, mem=_lib.HOST)
    with pytest.raises(_lib.SnpGpuError, match=r"snpgpu_geno_merge: invalid number of samples \(1 ... 2\^30 - 1\): the parts together"):
        _lib.geno_merge([_lib.merge_part(**big), _lib.merge_part(**big)], 4096)


def test_without_a_device_the_merging_functions_fail_loudly():
    from snprelate_amd.text import device_visible
    if device_visible():
        return                                             # (with a device the GPU tests cover the calls)
    from snprelate_amd import snpgdsAlleleSwitch, snpgdsCombineGeno
    mk = lambda ids: GenoFile(genotype=np.zeros((2, 3), np.uint8), sample_id=ids, snp_position=[1, 2], snp_allele=["A/C", "G/T"])  # noqa: E731
    with pytest.raises(_lib.SnpGpuError, match="no HIP device"):
        snpgdsCombineGeno([mk(["a", "b", "c"]), mk(["d", "e", "f"])], verbose=False)
    g = mk(["a", "b", "c"])
    with pytest.raises(_lib.SnpGpuError, match="no HIP device"):
        snpgdsAlleleSwitch(g, ["C", "G"], verbose=False)
    assert list(g.snp_allele) == ["A/C", "G/T"]                # nothing was changed
    # the argument errors of snpgdsAlleleSwitch need no device
    with pytest.raises(ValueError, match="The length of 'A.allele' should correspond to 'snp.allele' in the GDS file."):
        snpgdsAlleleSwitch(g, ["C"], verbose=False)
    with pytest.raises(ValueError, match="There is no allelic information in the GDS file"):
        snpgdsAlleleSwitch(GenoFile(genotype=np.zeros((2, 3), np.uint8)), ["C", "G"], verbose=False)
