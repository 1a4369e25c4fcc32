"""The kernel path of an accumulator context (csrc/ctx_plan.h) through snpgpu_diag_plan: no GPU is touched.

Every expected value below is written down from the rules of snpgpu_create as they stood before the plan existed and from
DESIGN.md 4 / 17a -- which kernel a block takes under which switch -- not printed from the library."""
import os
import subprocess

import pytest

from snprelate_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = ["SNPGPU_ACC_LAYOUT", "SNPGPU_EIG_BLAS", "SNPGPU_PAIR_BACKEND", "SNPGPU_PAIR_FP4", "SNPGPU_PAIR_FP4_GENERAL",
            "SNPGPU_GCTA_MISS_FP4", "SNPGPU_I8_NO_NOMISS", "SNPGPU_GCTA_SPARSE", "SNPGPU_GCTA_SPARSE_MAX_RATE", "SNPGPU_SYRK",
            "SNPGPU_H3_SUPER", "SNPGPU_X1_SUPER", "SNPGPU_SYRK_X1", "SNPGPU_SYRK_MISS3", "SNPGPU_SYRK_FAST", "SNPGPU_H3_PROMOTE",
            "SNPGPU_SYRK_UV", "SNPGPU_UV_TARGETS", "SNPGPU_X1_SPARSE", "SNPGPU_X1_SHORT_RUNS", "SNPGPU_X1_SPARSE_MAC", "SNPGPU_HOMO_UV",
            "SNPGPU_SYRK_UV16", "SNPGPU_UVC_PACE", "SNPGPU_I8_TAIL_PARTS"]
KINDS = {"IBS": _lib.IBS, "KING_ROBUST": _lib.KING_ROBUST, "KING_HOMO": _lib.KING_HOMO, "GRM_GCTA": _lib.GRM_GCTA,
         "PCA_COV": _lib.PCA_COV, "EIGMIX": _lib.EIGMIX, "INDIV_BETA": _lib.INDIV_BETA, "DISS": _lib.DISS}
FP4, FP4_NM, FP4_MISS, I8, POP = ("pair_mfma_fp4_kernel", "pair_mfma_fp4_nomiss_kernel", "pair_mfma_fp4_miss_kernel", "pair_mfma_i8_kernel",
                                  "pair_popcount_kernel")
UVC, UV16, UV32, X1 = "syrk_uv16c_kernel", "syrk_uv16_kernel", "syrk_uv_kernel", "syrk_x1_kernel"
H3_3, H3_2E, H3_2C, F32 = "syrk_h3_kernel<3, false>", "syrk_h3_kernel<2, true>", "syrk_h3_kernel<2, false>", "syrk_mfma_kernel"


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan(kind, n=700, **kw):
    return _lib.diag_plan(KINDS[kind], n, **kw)


def has(d, **want):
    got = {k: d.get(k) for k in want}
    assert got == {k: str(v) for k, v in want.items()}


def kernels(d):
    return (d["counter_kernel_nomiss"], d["counter_kernel_missing"], d["syrk_kernel_nomiss"], d["syrk_kernel_missing"])


def test_exported():
    assert "snpgpu_diag_plan" in _lib.EXPORTS and hasattr(_lib.lib(), "snpgpu_diag_plan")
    assert _lib.lib().snpgpu_abi_version() == 2


def test_geometry_of_a_context():
    # 700 samples: padded to 768 = 3 tiles of 256; 2-bit rows of 768 / 4 bytes; 32 768-SNP blocks = 1024 32-SNP words
    has(plan("GRM_GCTA"), n_samp=700, row0=0, row1=700, col0=0, rows_pad=768, ncols_pad=768, RB=192, Bmax=32768, KWmax=1024, full=1,
        acc_tiles_c=3, tail_parts=0)
    # a row panel [256, 512): columns from 256, 444 of them
    has(plan("GRM_GCTA", rows=(256, 512), max_block_snps=2000), row0=256, row1=512, col0=256, rows_pad=256, ncols_pad=512, full=0,
        acc_tiles_c=2, Bmax=2048, KWmax=64)
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_create: invalid panel rows"):
        plan("GRM_GCTA", rows=(100, 300))
    with pytest.raises(_lib.SnpGpuError, match="snpgpu_create: invalid kind"):
        _lib.diag_plan(9, 700)


@pytest.mark.parametrize("name,value,tiles", [("SNPGPU_ACC_LAYOUT", "row", 0), ("SNPGPU_ACC_LAYOUT", "tile", 3), ("SNPGPU_EIG_BLAS", "0", 0)])
def test_plane_layout(clean_env, name, value, tiles):
    clean_env.setenv(name, value)                # (SNPGPU_EIG_BLAS counts once it is set)
    has(plan("PCA_COV"), acc_tiles_c=tiles)


def test_default_plans_counters():
    d = plan("IBS")
    has(d, counter_mode="ibs", n_u32=3, counter_backend="mfma", nomiss_fp4=1, general_fp4=1, want_het=1, n_lut=0)
    assert kernels(d) == (FP4_NM, FP4, "none", "none")
    d = plan("KING_ROBUST")
    has(d, counter_mode="king_robust", n_u32=5, general_fp4=1, want_het=1, n_lut=0)
    assert kernels(d) == (FP4_NM, FP4, "none", "none")
    d = plan("INDIV_BETA")
    has(d, counter_mode="beta", n_u32=3, general_fp4=1, want_het=0, n_lut=0)
    assert kernels(d) == (FP4, FP4, "none", "none")


def test_default_plans_weight_sums():
    d = plan("KING_HOMO")
    has(d, counter_mode="king_homo", n_u32=2, general_fp4=1, want_het=1, n_lut=2, lut_mode0="homo_w1", lut_mode1="homo_w2", h3_a_kind0=1,
        h3_a_kind1=1, syrk_family="split_fp16", h3_exact_rows=0, want_x1_list=0, uv_enabled=0, homo_uv=1, homo_form="lookup16x16x32",
        homo_weights=2)
    assert kernels(d) == (FP4_NM, FP4, "none", UV16)          # a block without missing calls: two scalars, no product
    d = plan("DISS")
    has(d, counter_mode="diss", n_u32=1, general_fp4=1, nomiss_fp4=1, want_het=1, n_lut=1, lut_mode0="homo_w1", h3_a_kind0=1, homo_uv=1,
        homo_weights=1)
    assert kernels(d) == (FP4_NM, FP4, "none", UV16)


GRM_DEFAULT = dict(n_lut=1, h3_a_kind0=0, syrk_family="split_fp16", h3_super=8, x1_super=4, h3_exact_rows=1, h3_exact_missing=1, h3_w_shift=0,
                   h3_promote=8192, uv_promote=11264, want_x1_list=1, uv_enabled=1, uv_eigmix=0, uv_targets=1, uv_form="converted_carry",
                   uvc_pace=1, eigmix_x1=0, sparse_missing=1, x1_short_runs=1, x1_sparse_mac=128, wt_layout="entry12or8", wt_block_flag=1,
                   homo_uv=0)


def test_default_plans_grm_pca_eigmix():
    d = plan("GRM_GCTA")
    has(d, counter_mode="gcta_miss", n_u32=1, counter_backend="mfma", miss_fp4=1, want_het=0, gcta_sparse=1, sp_max_rate=0.002,
        lut_mode0="gcta", **GRM_DEFAULT)
    assert kernels(d) == ("none", FP4_MISS, UVC, X1)
    d = plan("PCA_COV")
    has(d, counter_mode="none", n_u32=0, counter_backend="none", lut_mode0="gcta", bayesian=0, **GRM_DEFAULT)
    assert kernels(d) == ("none", "none", UVC, X1)
    d = plan("PCA_COV", bayesian=True)
    has(d, lut_mode0="bayes", bayesian=1, **GRM_DEFAULT)
    assert kernels(d) == ("none", "none", UVC, X1)
    # EIGMIX: weight 1 -> the lookup form of the single-product kernel is exact; blocks with missing calls on the exact-row kernel
    # from their own 12 * code words; no weight targets, no sparse path, no column flag in the words
    d = plan("EIGMIX")
    has(d, counter_mode="none", n_lut=2, lut_mode0="eigmix_num", lut_mode1="eigmix_missw", h3_a_kind0=0, h3_a_kind1=2, h3_exact_rows=1,
        h3_exact_missing=0, h3_w_shift=0, want_x1_list=1, uv_enabled=1, uv_eigmix=1, uv_targets=0, uv_form="lookup16x16x32", uvc_pace=0,
        eigmix_x1=1, sparse_missing=0, wt_layout="entry8or16", wt_block_flag=0)
    assert kernels(d) == ("none", "none", UV16, X1)


SYRK_BACKENDS = {     # the fixture of tests/test_gpu_parity.py -> (environment, plan facts, kernel without / with missing calls)
    "f16": ({"SNPGPU_SYRK": "f16"}, GRM_DEFAULT, UVC, X1),
    "f16_uvc": ({"SNPGPU_SYRK": "f16", "SNPGPU_SYRK_UV16": "2"}, dict(GRM_DEFAULT, uv_form="converted"), UVC, X1),
    "f16_uv16": ({"SNPGPU_SYRK": "f16", "SNPGPU_SYRK_UV16": "1"}, dict(GRM_DEFAULT, uv_form="lookup16x16x32", uvc_pace=0), UV16, X1),
    "f16_uv32": ({"SNPGPU_SYRK": "f16", "SNPGPU_SYRK_UV16": "0"}, dict(GRM_DEFAULT, uv_form="mfma32x32x16", uvc_pace=0), UV32, X1),
    "f16_2w": ({"SNPGPU_SYRK": "f16", "SNPGPU_SYRK_X1": "0"},
               dict(GRM_DEFAULT, want_x1_list=0, uv_enabled=0, uv_targets=0, uv_form="lookup16x16x32", uvc_pace=0, sparse_missing=0,
                    wt_layout="entry16"), H3_2E, H3_2E),
    "f16_x1": ({"SNPGPU_SYRK": "f16", "SNPGPU_SYRK_UV": "0"},
               dict(GRM_DEFAULT, uv_enabled=0, uv_targets=0, uv_form="lookup16x16x32", uvc_pace=0, sparse_missing=0, wt_layout="entry12"), X1, X1),
    "h3": ({"SNPGPU_SYRK": "h3"},
           dict(GRM_DEFAULT, h3_a_kind0=-1, h3_exact_rows=0, h3_exact_missing=0, want_x1_list=0, uv_enabled=0, uv_targets=0,
                uv_form="lookup16x16x32", uvc_pace=0, sparse_missing=0, wt_layout="entry8or16", wt_block_flag=0), H3_3, H3_3),
    "f32": ({"SNPGPU_SYRK": "f32"},
            dict(GRM_DEFAULT, syrk_family="fp32", h3_a_kind0=-1, h3_exact_rows=0, h3_exact_missing=0, want_x1_list=0, uv_enabled=0,
                 uv_targets=0, uv_form="lookup16x16x32", uvc_pace=0, sparse_missing=0, wt_layout="entry8or16", wt_block_flag=0), F32, F32),
}


@pytest.mark.parametrize("backend", sorted(SYRK_BACKENDS))
def test_syrk_backends_of_the_parity_suite(clean_env, backend):
    env, facts, k_nomiss, k_missing = SYRK_BACKENDS[backend]
    for k, v in env.items():
        clean_env.setenv(k, v)
    for kind in ("GRM_GCTA", "PCA_COV"):
        d = plan(kind)
        has(d, **facts)
        assert kernels(d)[2:] == (k_nomiss, k_missing)
    # KING-homo under the same switches: the single fp16 product per weight needs the split-fp16 family only; binary tables take
    # a lookup form (32 x 32 x 16 with SNPGPU_SYRK_UV16=0)
    d = plan("KING_HOMO")
    if backend == "f32":
        has(d, homo_uv=0, syrk_family="fp32")
        assert kernels(d)[2:] == ("none", F32)
    else:
        has(d, homo_uv=1, homo_form="mfma32x32x16" if backend == "f16_uv32" else "lookup16x16x32")
        assert kernels(d)[2:] == ("none", UV32 if backend == "f16_uv32" else UV16)


PAIR_BACKENDS = {     # -> (environment, nomiss_fp4 / general_fp4 / miss_fp4, IBS kernels without / with missing calls, GCTA's)
    "mfma_i8": ({"SNPGPU_PAIR_BACKEND": "mfma_i8"}, (1, 1, 1), (FP4_NM, FP4), FP4_MISS),
    "mfma_i8_no_fp4": ({"SNPGPU_PAIR_BACKEND": "mfma_i8", "SNPGPU_PAIR_FP4": "0", "SNPGPU_GCTA_MISS_FP4": "0"}, (0, 0, 0), (I8, I8), I8),
    "mfma_fp4_nomiss_only": ({"SNPGPU_PAIR_BACKEND": "mfma_i8", "SNPGPU_PAIR_FP4_GENERAL": "0"}, (1, 0, 1), (FP4_NM, I8), FP4_MISS),
    "popcount": ({"SNPGPU_PAIR_BACKEND": "popcount"}, None, (POP, POP), POP),
}


@pytest.mark.parametrize("backend", sorted(PAIR_BACKENDS))
def test_pair_backends_of_the_parity_suite(clean_env, backend):
    env, fp4, ibs_kernels, gcta_kernel = PAIR_BACKENDS[backend]
    for k, v in env.items():
        clean_env.setenv(k, v)
    for kind in ("IBS", "KING_ROBUST", "KING_HOMO"):
        d = plan(kind)
        if fp4:
            has(d, counter_backend="mfma", nomiss_fp4=fp4[0], general_fp4=fp4[1], want_het=1)
        else:
            has(d, counter_backend="popcount")
        assert kernels(d)[:2] == ibs_kernels
    d = plan("GRM_GCTA")
    if fp4:
        has(d, miss_fp4=fp4[2], gcta_sparse=1)
    assert kernels(d) == ("none", gcta_kernel, UVC, X1)
    # KING-homo on bit planes has no two-scalar form: the two-product weight kernels for every block
    if backend == "popcount":
        d = plan("KING_HOMO")
        has(d, homo_uv=0)
        assert kernels(d)[2:] == (H3_2C, H3_2C)


def test_dissimilarity_refuses_forms_it_does_not_have(clean_env):
    text = "snpgpu_create: the dissimilarity kind needs the MX-fp4 counter kernels and the fp16 weight product"
    for name, value in (("SNPGPU_PAIR_FP4", "0"), ("SNPGPU_PAIR_FP4_GENERAL", "0"), ("SNPGPU_PAIR_BACKEND", "popcount"), ("SNPGPU_SYRK", "f32")):
        clean_env.setenv(name, value)
        with pytest.raises(_lib.SnpGpuError, match=text):
            plan("DISS")
        clean_env.delenv(name)
    plan("DISS")


def test_single_switches(clean_env):
    clean_env.setenv("SNPGPU_HOMO_UV", "0")
    d = plan("KING_HOMO")
    has(d, homo_uv=0, want_het=1)
    assert kernels(d) == (FP4_NM, FP4, "none", H3_2C)
    clean_env.delenv("SNPGPU_HOMO_UV")
    clean_env.setenv("SNPGPU_UVC_PACE", "0")
    has(plan("GRM_GCTA"), **dict(GRM_DEFAULT, uvc_pace=0))
    clean_env.delenv("SNPGPU_UVC_PACE")
    clean_env.setenv("SNPGPU_GCTA_SPARSE", "0")
    has(plan("GRM_GCTA"), gcta_sparse=0, sp_max_rate=0)
    clean_env.delenv("SNPGPU_GCTA_SPARSE")
    clean_env.setenv("SNPGPU_GCTA_SPARSE_MAX_RATE", "0.03")
    has(plan("GRM_GCTA"), gcta_sparse=1, sp_max_rate=0.03)
    clean_env.setenv("SNPGPU_GCTA_SPARSE_MAX_RATE", "1.5")       # outside [0, 1]: ignored
    has(plan("GRM_GCTA"), gcta_sparse=1, sp_max_rate=0.002)
    clean_env.delenv("SNPGPU_GCTA_SPARSE_MAX_RATE")
    clean_env.setenv("SNPGPU_I8_TAIL_PARTS", "1")
    has(plan("IBS"), tail_parts=1)
    clean_env.setenv("SNPGPU_I8_TAIL_PARTS", "65")               # 1 ... 64
    has(plan("IBS"), tail_parts=0)


@pytest.mark.parametrize("value", ["1", "0"])
def test_presence_switches_count_even_when_zero(clean_env, value):
    """SNPGPU_SYRK_MISS3 and SNPGPU_I8_NO_NOMISS act once they are set, whatever they hold."""
    clean_env.setenv("SNPGPU_SYRK_MISS3", value)
    d = plan("GRM_GCTA")
    has(d, h3_exact_rows=1, h3_exact_missing=0, want_x1_list=0, uv_enabled=0, sparse_missing=0, wt_layout="entry8or16", wt_block_flag=1)
    assert kernels(d)[2:] == (H3_2E, H3_3)
    d = plan("EIGMIX")           # no exact-row list: neither the single-product kernel nor the 12 * code words
    has(d, uv_eigmix=0, eigmix_x1=0, want_x1_list=0, wt_block_flag=1)
    assert kernels(d)[2:] == (H3_2E, H3_3)
    clean_env.delenv("SNPGPU_SYRK_MISS3")
    clean_env.setenv("SNPGPU_I8_NO_NOMISS", value)
    for kind in ("IBS", "KING_ROBUST"):
        d = plan(kind)
        has(d, want_het=0, general_fp4=1)
        assert kernels(d)[:2] == (FP4, FP4)
    d = plan("KING_HOMO")        # ... and KING-homo loses the two-scalar form its single product needs
    has(d, want_het=0, homo_uv=0)
    assert kernels(d) == (FP4, FP4, H3_2C, H3_2C)
    has(plan("DISS"), want_het=1)       # the dissimilarity counter has no other form for such blocks


def test_value_switches_set_to_one_equal_unset(clean_env):
    base = {k: plan(k) for k in ("GRM_GCTA", "EIGMIX", "KING_HOMO", "IBS")}
    for name in ("SNPGPU_SYRK_UV", "SNPGPU_SYRK_X1", "SNPGPU_UV_TARGETS", "SNPGPU_X1_SPARSE", "SNPGPU_X1_SHORT_RUNS", "SNPGPU_HOMO_UV",
                 "SNPGPU_UVC_PACE", "SNPGPU_PAIR_FP4", "SNPGPU_PAIR_FP4_GENERAL", "SNPGPU_GCTA_MISS_FP4", "SNPGPU_GCTA_SPARSE"):
        clean_env.setenv(name, "1")
        assert {k: plan(k) for k in base} == base, name
        clean_env.delenv(name)
    clean_env.setenv("SNPGPU_SYRK_FAST", "0")
    assert plan("GRM_GCTA") == base["GRM_GCTA"]
    clean_env.setenv("SNPGPU_SYRK_FAST", "1")
    has(plan("GRM_GCTA"), h3_promote=32768, uv_promote=32768, uv_targets=0, uv_enabled=1)
    clean_env.delenv("SNPGPU_SYRK_FAST")
    clean_env.setenv("SNPGPU_SYRK_UV", "0")
    has(plan("EIGMIX"), uv_eigmix=0, uv_enabled=0, eigmix_x1=0, want_x1_list=0)
    clean_env.delenv("SNPGPU_SYRK_UV")
    for name, off in (("SNPGPU_UV_TARGETS", dict(uv_targets=0)), ("SNPGPU_X1_SHORT_RUNS", dict(x1_short_runs=0))):
        clean_env.setenv(name, "0")
        has(plan("GRM_GCTA"), **dict(GRM_DEFAULT, **off))
        clean_env.delenv(name)


def test_ranges(clean_env):
    for bad in ("100", "300", "70000"):          # a multiple of 256 in 256 ... 65 536, else ignored
        clean_env.setenv("SNPGPU_H3_PROMOTE", bad)
        has(plan("GRM_GCTA"), h3_promote=8192, uv_promote=11264)
    clean_env.setenv("SNPGPU_H3_PROMOTE", "4096")
    has(plan("GRM_GCTA"), h3_promote=4096, uv_promote=4096)
    clean_env.delenv("SNPGPU_H3_PROMOTE")
    clean_env.setenv("SNPGPU_SYRK_UV16", "7")    # clamped to 3 = the default
    has(plan("GRM_GCTA"), **GRM_DEFAULT)
    clean_env.setenv("SNPGPU_SYRK_UV16", "-2")   # ... and to 0
    has(plan("GRM_GCTA"), uv_form="mfma32x32x16")
    clean_env.delenv("SNPGPU_SYRK_UV16")
    for name, key in (("SNPGPU_H3_SUPER", "h3_super"), ("SNPGPU_X1_SUPER", "x1_super")):
        clean_env.setenv(name, "2")
        has(plan("GRM_GCTA"), **{key: 2})
        clean_env.setenv(name, "33")             # 1 ... 32
        has(plan("GRM_GCTA"), h3_super=8, x1_super=4)
        clean_env.delenv(name)
    clean_env.setenv("SNPGPU_X1_SPARSE_MAC", "1000")
    has(plan("GRM_GCTA"), x1_sparse_mac=128)
    clean_env.setenv("SNPGPU_X1_SPARSE_MAC", "0")
    has(plan("GRM_GCTA"), x1_sparse_mac=1)


@pytest.mark.parametrize("n,shift", [(700, 0), (9000, 1), (150000, 5)])
def test_weight_shift_keeps_the_tables_in_fp16_range(n, shift):
    """|w| <= 4.04 N in a block without missing calls; the tables hold w 2^-s with the smallest s for which 4.04 N 2^-s <= 32768:
    700 -> 2828, 9000 -> 36 360 / 2, 150 000 -> 606 000 / 32 = 18 937.5 (606 000 / 16 = 37 875 is too large)."""
    assert 4.04 * n / 2 ** shift <= 32768 and (shift == 0 or 4.04 * n / 2 ** (shift - 1) > 32768)
    has(plan("GRM_GCTA", n), h3_w_shift=shift)
    has(plan("PCA_COV", n, bayesian=True), h3_w_shift=shift)
    has(plan("EIGMIX", n), h3_w_shift=0)         # weight 1


def test_sparse_rare_variants_need_384_samples(clean_env):
    for value in (None, "1", "0"):
        if value is not None:
            clean_env.setenv("SNPGPU_X1_SPARSE", value)
        has(plan("GRM_GCTA", 383), sparse_missing=0, uv_enabled=1)
        has(plan("GRM_GCTA", 384), sparse_missing=0 if value == "0" else 1)


def test_block_run_geometry(clean_env):
    # 32 chunks of 1024 slots at <= 11 per run: 3 runs of 11 + 11 + 10, a weight target each
    has(plan("GRM_GCTA", block_snps=32768), uv_chunks=32, uv_cpr=11, uv_runs=3, uv_q=3, n_pad=32768, n_q=2048)
    # a small block with weight targets: spread over two chunks = two runs = two targets
    has(plan("GRM_GCTA", block_snps=1000), uv_chunks=2, uv_cpr=1, uv_runs=2, uv_q=2, n_pad=2048, n_q=128)
    # EIGMIX: one target (weight 1), one run, padded to whole 256-SNP rounds
    has(plan("EIGMIX", block_snps=1000), uv_chunks=1, uv_cpr=1, uv_runs=1, uv_q=1, n_pad=1024, n_q=64)
    has(plan("KING_HOMO", block_snps=1030), uv_runs=1, n_pad=1280, n_q=80)        # single product per weight: rounds of 256
    # bench.py's variants: eight 8192-slot runs of a 65 536-SNP block (at most UV_QMAX = 8 targets); one 32 768-SNP run
    clean_env.setenv("SNPGPU_H3_PROMOTE", "8192")
    has(plan("GRM_GCTA", block_snps=65536, max_block_snps=65536), uv_chunks=64, uv_cpr=8, uv_runs=8, uv_q=8, n_pad=65536)
    clean_env.delenv("SNPGPU_H3_PROMOTE")
    clean_env.setenv("SNPGPU_SYRK_FAST", "1")
    has(plan("GRM_GCTA", block_snps=32768), uv_chunks=32, uv_cpr=1, uv_runs=1, uv_q=1, n_pad=32768)
    clean_env.delenv("SNPGPU_SYRK_FAST")
    # without the single-product kernel: rounds of 128 SNPs with the one-wave exact-row kernel, of 64 without
    clean_env.setenv("SNPGPU_SYRK_UV", "0")
    has(plan("GRM_GCTA", block_snps=1030), uv_runs=1, uv_q=1, n_pad=1152, n_q=72)
    clean_env.setenv("SNPGPU_SYRK", "h3")
    has(plan("GRM_GCTA", block_snps=1030), n_pad=1088, n_q=68)


BENCH_CASES = [("grm", 0.0, {}), ("grm", 0.02, {}), ("grm", 0.0, {"SNPGPU_SYRK_UV": "0"}), ("grm", 0.0, {"SNPGPU_H3_PROMOTE": "8192"}),
               ("grm", 0.0, {"SNPGPU_SYRK_FAST": "1"}), ("grm", 0.0, {"SNPGPU_SYRK": "f32"}), ("grm", 0.02, {"SNPGPU_SYRK_UV": "0"}),
               ("grm", 0.02, {"SNPGPU_SYRK": "f32"}), ("ibs", 0.0, {}), ("ibs", 0.05, {}), ("king_homo", 0.0, {}), ("king_homo", 0.05, {})]


@pytest.mark.parametrize("workload,missing,env", BENCH_CASES)
def test_bench_roofline_names_the_kernel_of_the_plan(clean_env, workload, missing, env):
    """bench.py restates the dispatch to name the dominant kernel of a run; under the environments its own runs use it must name
    the kernel the plan leads to (bench.py writes the pair counters' mode behind the name, the plan reports it as counter_mode)."""
    import bench
    for k, v in env.items():
        clean_env.setenv(k, v)
    wl = dict(bench.WORKLOADS[workload], missing=missing)
    roof = bench.roofline(wl, 1, wl["n"] * (wl["n"] + 1) / 2.0, wl["b"], 1.0, 1, dict(os.environ))
    d = plan(wl["kind"], wl["n"], max_block_snps=wl["b"])
    suffix = "missing" if missing > 0 else "nomiss"
    want = d["syrk_kernel_" + suffix] if wl["which"] == 1 else d["counter_kernel_" + suffix]
    assert roof["kernel"].split("<PM_")[0] == want
    if workload == "king_homo":      # its second kernel: the weight product of the blocks with missing calls
        assert d["syrk_kernel_missing"] in roof["kernels_ms_per_step"]


def test_work_lists_against_brute_force(tmp_path):
    """tests/worklist_check.cpp includes only worklist.h (the work lists of the MFMA pair and SYRK kernels, the super-tile tables of
    the others); built with the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own,
    it prints nothing and exits 0"""
    exe = str(tmp_path / "worklist_check")
    r = subprocess.run(["g++", "-std=gnu++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "snprelate_amd", "csrc"), os.path.join(ROOT, "tests", "worklist_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (r.stdout + r.stderr)[-3000:]
