"""ctypes binding of libsnpgpu.so (include/snpgpu.h).

There is no CPU fallback: if the HIP library is missing, fails to load, or no
MI355X is visible, every compute entry point raises ``SnpGpuError``.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SNPGPU_LIB: another build of the same library (A/B measurements of kernel variants on one box)
LIB_PATH = os.environ.get("SNPGPU_LIB") or os.path.join(_HERE, "libsnpgpu.so")

# enums of include/snpgpu.h
IBS, KING_ROBUST, KING_HOMO, GRM_GCTA, PCA_COV, EIGMIX, INDIV_BETA = 1, 2, 3, 4, 5, 6, 7
DISS = 8
GENO_U8, GENO_PACKED2 = 0, 1
LD_COMPOSITE, LD_R, LD_DPRIME, LD_CORR, LD_COV = 1, 2, 3, 4, 5
HOST, DEVICE, HOST_PINNED = 0, 1, 2
CODE_GDS, CODE_BED = 0, 1
TEXT_DIGIT, TEXT_PED_AB, TEXT_PED_12, TEXT_PED_ALLELE = 0, 1, 2, 3

EXPORTS = [
    "snpgpu_abi_version", "snpgpu_last_error", "snpgpu_device_count",
    "snpgpu_create", "snpgpu_destroy", "snpgpu_feed", "snpgpu_sync", "snpgpu_counts",
    "snpgpu_host_alloc", "snpgpu_host_free", "snpgpu_host_wait",
    "snpgpu_slab_size", "snpgpu_set_timing", "snpgpu_get_timing", "snpgpu_ibs_num", "snpgpu_ibs_ave", "snpgpu_king_robust_counts",
    "snpgpu_king_robust", "snpgpu_king_homo", "snpgpu_grm_gcta", "snpgpu_pca_cov", "snpgpu_panel_entries", "snpgpu_block_stats", "snpgpu_feed_stats",
    "snpgpu_ibd_mom", "snpgpu_eigmix", "snpgpu_indiv_beta", "snpgpu_gnrIBD_PLINK", "snpgpu_gnrIBD_Beta",
    "snpgpu_gnrGRM_avg_val", "snpgpu_gnrEigMix",
    "snpgpu_pca_eigen", "snpgpu_pca_panel_matmul", "snpgpu_pca_panel_matmul_f32", "snpgpu_pca_panel_trace", "snpgpu_ws_set_geno", "snpgpu_ws_sel_snp_base",
    "snpgpu_ws_get_geno_dim", "snpgpu_ws_snp_rate_freq", "snpgpu_ws_clear",
    "snpgpu_gnrIBSNum", "snpgpu_gnrIBSAve", "snpgpu_gnrIBD_KING_Robust",
    "snpgpu_gnrIBD_KING_Homo", "snpgpu_gnrGRM", "snpgpu_gnrPCA",
    "snpgpu_proj_create", "snpgpu_proj_destroy", "snpgpu_proj_sync", "snpgpu_proj_set_eigvec", "snpgpu_proj_snp_corr",
    "snpgpu_proj_snp_loading", "snpgpu_proj_samp_loading_feed", "snpgpu_proj_samp_loading",
    "snpgpu_gnrPCACorr", "snpgpu_gnrPCASNPLoading", "snpgpu_gnrPCASampLoading",
    "snpgpu_proj_samp_loading_reset", "snpgpu_gnrPCA_randomized",
    "snpgpu_proj_snp_loading_ext", "snpgpu_gnrEigMixSNPLoading", "snpgpu_gnrEigMixSampLoading",
    "snpgpu_gnrGRMMerge", "snpgpu_synth_block", "snpgpu_ws_sel_snp_base_ex",
    "snpgpu_finalize_inplace", "snpgpu_panels_topk_eigen",
    "snpgpu_multi_create", "snpgpu_multi_destroy", "snpgpu_multi_info", "snpgpu_multi_comm_selftest", "snpgpu_multi_panel", "snpgpu_multi_feed",
    "snpgpu_multi_host_wait", "snpgpu_multi_sync", "snpgpu_multi_counts", "snpgpu_multi_ibs_num", "snpgpu_multi_ibs_ave",
    "snpgpu_multi_king_robust", "snpgpu_multi_king_robust_counts", "snpgpu_multi_king_homo", "snpgpu_multi_grm_gcta",
    "snpgpu_multi_eigmix", "snpgpu_multi_pca_trace", "snpgpu_multi_pca_cov", "snpgpu_multi_finalize_inplace",
    "snpgpu_multi_topk_eigen", "snpgpu_diag_mfma_rate", "snpgpu_diag_device_pci", "snpgpu_multi_get_status",
    "snpgpu_ld_create", "snpgpu_ld_destroy", "snpgpu_ld_out_dims", "snpgpu_ld_feed", "snpgpu_ld_result", "snpgpu_ld_set_timing",
    "snpgpu_ld_get_timing", "snpgpu_ld_pair_tables", "snpgpu_gnrLDMat",
    "snpgpu_ibd_mle", "snpgpu_ibd_loglik", "snpgpu_ibd_mle_stats", "snpgpu_gnrIBD_MLE", "snpgpu_gnrIBD_LogLik",
    "snpgpu_gnrIBD_LogLik_k01", "snpgpu_diag_fp64_rate",
    "snpgpu_ibd_mle_pairs", "snpgpu_ibd_mle_pairs_stats", "snpgpu_gnrIBD_MLE_Pairs",
    "snpgpu_ibd_jacquard_pairs", "snpgpu_gnrIBD_MLE_PairsMethod",
    "snpgpu_ld_prune", "snpgpu_ld_prune_bits", "snpgpu_gnrLDpruning",
    "snpgpu_ld_score", "snpgpu_gnrLDScore",
    "snpgpu_diss", "snpgpu_diss_sums", "snpgpu_gnrDiss", "snpgpu_multi_diss",
    "snpgpu_pop_counts", "snpgpu_fst", "snpgpu_fst_windows", "snpgpu_pop_stats", "snpgpu_gnrFst", "snpgpu_gnrSlidingWindowFst",
    "snpgpu_geno_counts", "snpgpu_hwe", "snpgpu_hwe_counts", "snpgpu_ind_inb", "snpgpu_qc_stats", "snpgpu_gnrSampFreq", "snpgpu_gnrHWE",
    "snpgpu_gnrIndInb",
    "snpgpu_hclust_average", "snpgpu_dist_perm", "snpgpu_gnrDistPerm", "snpgpu_tree_stats",
    "snpgpu_pair_tables", "snpgpu_pair_score_final", "snpgpu_pair_score_matrix", "snpgpu_gnrPairScore", "snpgpu_pair_stats",
    "snpgpu_diag_plan", "snpgpu_diag_carry_fallbacks",
    "snpgpu_select_pairs", "snpgpu_multi_select_pairs", "snpgpu_gnrIBDPairs", "snpgpu_gnrIBDPairs_get", "snpgpu_select_stats",
    "snpgpu_select_grm", "snpgpu_multi_select_grm", "snpgpu_gnrGRMPairs", "snpgpu_gnrGRMPairs_get", "snpgpu_select_grm_stats",
    "snpgpu_geno_select", "snpgpu_geno_select_stats",
    "snpgpu_geno_convert", "snpgpu_geno_convert_stats",
    "snpgpu_vcf_index", "snpgpu_vcf_genotypes", "snpgpu_vcf_stats",
    "snpgpu_text_render", "snpgpu_text_stats",
    "snpgpu_ped_tokens", "snpgpu_ped_census", "snpgpu_ped_codes", "snpgpu_ped_stats",
    "snpgpu_geno_merge", "snpgpu_geno_merge_stats",
    "snpgpu_gen_genotypes", "snpgpu_gen_line_host", "snpgpu_gen_stats",
    "snpgpu_grm_merge_stats",
    "snpgpu_mds", "snpgpu_mds_apply", "snpgpu_gnrMDS", "snpgpu_mds_stats",
    "snpgpu_pcr_create", "snpgpu_pcr_feed", "snpgpu_pcr_result", "snpgpu_pcr_sums", "snpgpu_pcr_stats", "snpgpu_pcr_destroy",
    "snpgpu_gnrPCRelate",
    "snpgpu_pcr_create_panel", "snpgpu_pcr_panel_result", "snpgpu_pcr_panel_sums", "snpgpu_pcr_panel_stats", "snpgpu_pcr_select", "snpgpu_pcr_select_stats",
    "snpgpu_gnrPCRelatePairs", "snpgpu_gnrPCRelatePairs_get",
    "snpgpu_diag_syrk_launches",
    "snpgpu_admix_create", "snpgpu_admix_feed", "snpgpu_admix_set", "snpgpu_admix_run", "snpgpu_admix_get", "snpgpu_admix_stats",
    "snpgpu_admix_destroy", "snpgpu_gnrAdmix",
]
FST_WC84, FST_WH02 = 1, 2
FST_METHODS = ("W&C84", "W&H02")
INB_METHODS = ("mom.weir", "mom.visscher", "mle", "gcta1", "gcta2", "gcta3")      # snpgpu_inb_method = index + 1
INB_MLE = 3
PAIR_METHODS = ("IBS", "GVH", "HVG", "GVH.major", "GVH.minor", "GVH.major.only", "GVH.minor.only")      # snpgpu_pair_method = index + 1
PAIR_TYPES = ("per.pair", "per.snp", "matrix", "gds.file")
PAIR_TABLE, SNP_TABLE = 0, 1
PAIR_ELEM_INT32, PAIR_ELEM_BIT2 = 0, 1
SEL_KING_ROBUST, SEL_KING_HOMO, SEL_MOM = 1, 2, 3
SEL_GRM_GCTA, SEL_GRM_EIGENSTRAT, SEL_GRM_EIGMIX, SEL_GRM_INDIV_BETA = 1, 2, 3, 4
LDSCORE_ADJUST, LDSCORE_SELF = 1, 2
PCR_IBD = 1
PCR_PLANES = ("RR", "SS", "DD", "DC", "CC", "IBS0", "K0D", "NS")      # snpgpu_pcr_sums' `which` = index
PCR_SLABS = PCR_PLANES + ("CD",)                                       # snpgpu_pcr_panel_sums': CD = DC transposed
PCR_TILE = 128                                                         # a panel's row_begin is a multiple of it
ADMIX_FIX_F = 1                                                        # snpgpu_admix_run: F stays, only Q moves


class SnpGpuError(RuntimeError):
    pass


class Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("bayesian", ctypes.c_int32),
                ("row_begin", ctypes.c_int64), ("row_end", ctypes.c_int64),
                ("max_block_snps", ctypes.c_int64), ("stream", ctypes.c_void_p)]


REDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)


class EigOpts(ctypes.Structure):       # snpgpu_eig_opts
    _fields_ = [("tol", ctypes.c_double), ("block", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("max_restarts", ctypes.c_int32), ("seed", ctypes.c_uint32), ("y_buf", ctypes.c_void_p),
                ("reduce", REDUCE_FN), ("user", ctypes.c_void_p), ("fp32_until", ctypes.c_double)]


class MultiOpts(ctypes.Structure):     # snpgpu_multi_opts
    _fields_ = [("devices", ctypes.POINTER(ctypes.c_int32)), ("n_devices", ctypes.c_int32),
                ("panels_per_device", ctypes.c_int32), ("n_passes", ctypes.c_int32), ("pass_", ctypes.c_int32)]


class MultiStatus(ctypes.Structure):   # snpgpu_multi_status
    _fields_ = [(k, ctypes.c_int32) for k in ("n_devices", "n_distinct_devices", "n_panels", "panels_per_device", "uses_rccl", "peer_pairs",
                                              "peer_pairs_enabled", "selftest_comm", "selftest_feed", "selftest_gather")] + \
               [("reserved", ctypes.c_int32 * 6)]


class SelOpts(ctypes.Structure):       # snpgpu_sel_opts
    _fields_ = [("what", ctypes.c_int32), ("kinship_constraint", ctypes.c_int32), ("family", ctypes.c_void_p), ("e", ctypes.c_void_p),
                ("kinship_cutoff", ctypes.c_double), ("samp_sel", ctypes.c_void_p)]


class PcrSelOpts(ctypes.Structure):    # snpgpu_pcr_sel_opts
    _fields_ = [("kinship_cutoff", ctypes.c_double), ("samp_sel", ctypes.c_void_p)]


class GrmSelOpts(ctypes.Structure):    # snpgpu_grm_sel_opts
    _fields_ = [("what", ctypes.c_int32), ("mode", ctypes.c_int32), ("scale", ctypes.c_double), ("trace_in", ctypes.c_double),
                ("cutoff", ctypes.c_double), ("samp_sel", ctypes.c_void_p)]


class GenoSrc(ctypes.Structure):       # snpgpu_geno_src
    _fields_ = [("bits", ctypes.c_void_p), ("mem", ctypes.c_int32), ("major", ctypes.c_int32), ("n_rows", ctypes.c_int64),
                ("n_cols", ctypes.c_int64), ("bit0", ctypes.c_int64), ("row_stride_bits", ctypes.c_int64), ("row_bit", ctypes.c_void_p),
                ("n_bytes", ctypes.c_int64)]


class MergePart(ctypes.Structure):     # snpgpu_merge_part
    _fields_ = [("src", GenoSrc), ("snp_index", ctypes.c_void_p), ("samp_index", ctypes.c_void_p), ("n_samp", ctypes.c_int64),
                ("flip", ctypes.c_void_p)]


class EigInfo(ctypes.Structure):       # snpgpu_eig_info
    _fields_ = [("restarts", ctypes.c_int32), ("matmuls", ctypes.c_int32), ("block", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("max_rel_residual", ctypes.c_double), ("matmuls_fp32", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


_lib = None


def build(force=False):
    """Compile libsnpgpu.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", src_dir] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP/HSA runtime; if it is initialised AFTER the system runtime
    # that libsnpgpu.so links against, torch reports "No HIP GPUs are available".  The other order
    # works, so when torch is installed let it probe the devices first (plumbing only: the library
    # itself has no torch dependency and runs without it, e.g. under R).
    try:
        import torch
        torch.cuda.is_available()
    except Exception:  # pragma: no cover
        pass
    if not os.path.exists(LIB_PATH):
        raise SnpGpuError("libsnpgpu.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                          "there is no CPU fallback")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise SnpGpuError("cannot load %s: %s" % (LIB_PATH, e))
    vp, i64, c_int, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    L.snpgpu_abi_version.restype = c_int
    L.snpgpu_last_error.restype = ctypes.c_char_p
    L.snpgpu_device_count.argtypes = [ctypes.POINTER(c_int)]
    L.snpgpu_diag_mfma_rate.argtypes = [c_int, c_int, dbl, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    L.snpgpu_diag_device_pci.argtypes = [c_int, ctypes.c_char_p, c_int]
    L.snpgpu_diag_plan.argtypes = [c_int, i64, ctypes.POINTER(Opts), i64, ctypes.c_char_p, c_int]
    L.snpgpu_diag_carry_fallbacks.argtypes = [vp, ctypes.POINTER(i64), c_int]
    L.snpgpu_diag_syrk_launches.argtypes = [vp, ctypes.POINTER(i64)]
    L.snpgpu_synth_block.argtypes = [vp, i64, i64, i64, ctypes.c_uint32, dbl, c_int, c_int, c_int, vp]
    L.snpgpu_create.argtypes = [c_int, i64, ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.snpgpu_destroy.argtypes = [vp]
    L.snpgpu_feed.argtypes = [vp, vp, i64, c_int, c_int]
    L.snpgpu_sync.argtypes = [vp]
    L.snpgpu_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(vp)]
    L.snpgpu_host_free.argtypes = [vp]
    L.snpgpu_host_wait.argtypes = [vp, vp]
    L.snpgpu_block_stats.argtypes = [vp, vp, i64, c_int, vp, vp]
    L.snpgpu_feed_stats.argtypes = [vp, vp, i64, c_int, c_int, vp, vp]
    L.snpgpu_counts.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.snpgpu_set_timing.argtypes = [vp, c_int]
    L.snpgpu_get_timing.argtypes = [vp, c_int, ctypes.POINTER(dbl), ctypes.POINTER(i64)]
    L.snpgpu_slab_size.argtypes = [vp]
    L.snpgpu_slab_size.restype = i64
    L.snpgpu_ibs_num.argtypes = [vp, vp, vp, vp, c_int, c_int]
    L.snpgpu_ibs_ave.argtypes = [vp, vp, c_int, c_int]
    L.snpgpu_king_robust_counts.argtypes = [vp, vp, c_int]
    L.snpgpu_king_robust.argtypes = [vp, vp, vp, vp, c_int, c_int]
    L.snpgpu_king_homo.argtypes = [vp, vp, vp, c_int, c_int]
    L.snpgpu_diss.argtypes = [vp, vp, c_int, c_int]
    L.snpgpu_diss_sums.argtypes = [vp, vp, vp, c_int]
    L.snpgpu_gnrDiss.argtypes = [c_int, c_int, vp]
    L.snpgpu_multi_diss.argtypes = [vp, vp, c_int]
    L.snpgpu_grm_gcta.argtypes = [vp, vp, c_int, c_int]
    L.snpgpu_pca_cov.argtypes = [vp, vp, c_int, c_int, dbl, ctypes.POINTER(dbl), c_int]
    L.snpgpu_pca_eigen.argtypes = [vp, c_int, vp, vp, c_int]
    L.snpgpu_ibd_mom.argtypes = [vp, vp, c_int, vp, vp, c_int, c_int]
    L.snpgpu_eigmix.argtypes = [vp, c_int, dbl, vp, c_int, c_int]
    L.snpgpu_indiv_beta.argtypes = [vp, c_int, vp, ctypes.POINTER(dbl), c_int, c_int]
    L.snpgpu_gnrIBD_PLINK.argtypes = [c_int, vp, c_int, c_int, c_int, vp, vp, vp]
    L.snpgpu_gnrIBD_Beta.argtypes = [c_int, c_int, c_int, c_int, vp, ctypes.POINTER(dbl)]
    L.snpgpu_gnrGRM_avg_val.argtypes = [ctypes.POINTER(dbl)]
    L.snpgpu_gnrEigMix.argtypes = [c_int, c_int, c_int, c_int, vp, vp, vp, vp]
    L.snpgpu_pca_panel_matmul.argtypes = [vp, dbl, vp, c_int, vp]
    L.snpgpu_pca_panel_matmul_f32.argtypes = [vp, dbl, vp, c_int, vp]
    L.snpgpu_pca_panel_trace.argtypes = [vp, ctypes.POINTER(dbl)]
    L.snpgpu_finalize_inplace.argtypes = [vp, c_int, dbl]
    L.snpgpu_panel_entries.argtypes = [vp, vp, vp, i64, vp]
    L.snpgpu_panels_topk_eigen.argtypes = [ctypes.POINTER(vp), c_int, dbl, c_int, ctypes.POINTER(EigOpts), vp, vp, c_int,
                                           ctypes.POINTER(EigInfo)]
    L.snpgpu_multi_create.argtypes = [c_int, i64, ctypes.POINTER(Opts), ctypes.POINTER(MultiOpts), ctypes.POINTER(vp)]
    L.snpgpu_multi_destroy.argtypes = [vp]
    L.snpgpu_multi_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.snpgpu_multi_comm_selftest.argtypes = [vp, ctypes.POINTER(c_int)]
    L.snpgpu_multi_get_status.argtypes = [vp, ctypes.POINTER(MultiStatus)]
    L.snpgpu_multi_panel.argtypes = [vp, c_int, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(c_int)]
    L.snpgpu_multi_feed.argtypes = [vp, vp, i64, c_int, c_int]
    L.snpgpu_multi_host_wait.argtypes = [vp, vp]
    L.snpgpu_multi_sync.argtypes = [vp]
    L.snpgpu_multi_counts.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.snpgpu_multi_ibs_num.argtypes = [vp, vp, vp, vp, c_int]
    L.snpgpu_multi_ibs_ave.argtypes = [vp, vp, c_int]
    L.snpgpu_multi_king_robust.argtypes = [vp, vp, vp, vp, c_int]
    L.snpgpu_multi_king_robust_counts.argtypes = [vp, vp, c_int]
    L.snpgpu_multi_king_homo.argtypes = [vp, vp, vp, c_int]
    L.snpgpu_multi_grm_gcta.argtypes = [vp, vp, c_int]
    L.snpgpu_multi_eigmix.argtypes = [vp, c_int, dbl, vp, c_int]
    L.snpgpu_multi_pca_trace.argtypes = [vp, ctypes.POINTER(dbl)]
    L.snpgpu_multi_pca_cov.argtypes = [vp, vp, c_int, ctypes.POINTER(dbl), c_int]
    L.snpgpu_multi_finalize_inplace.argtypes = [vp, c_int, dbl]
    L.snpgpu_multi_topk_eigen.argtypes = [vp, dbl, c_int, ctypes.POINTER(EigOpts), vp, vp, c_int, ctypes.POINTER(EigInfo)]
    L.snpgpu_ws_set_geno.argtypes = [vp, i64, i64, c_int, c_int]
    L.snpgpu_ws_sel_snp_base.argtypes = [c_int, dbl, dbl, ctypes.POINTER(ctypes.c_int32), vp]
    L.snpgpu_ws_sel_snp_base_ex.argtypes = [vp, c_int, dbl, dbl, ctypes.POINTER(ctypes.c_int32), vp]
    L.snpgpu_ws_get_geno_dim.argtypes = [ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.snpgpu_ws_snp_rate_freq.argtypes = [vp, vp, vp]
    L.snpgpu_gnrIBSNum.argtypes = [c_int, c_int, vp, vp, vp]
    L.snpgpu_gnrIBSAve.argtypes = [c_int, c_int, c_int, vp]
    L.snpgpu_gnrIBD_KING_Robust.argtypes = [vp, c_int, c_int, c_int, vp, vp]
    L.snpgpu_gnrIBD_KING_Homo.argtypes = [c_int, c_int, c_int, vp, vp]
    L.snpgpu_gnrGRM.argtypes = [c_int, ctypes.c_char_p, c_int, c_int, vp]
    L.snpgpu_gnrGRMMerge.argtypes = [c_int, i64, ctypes.POINTER(vp), ctypes.c_char_p, vp, vp, vp, c_int]
    L.snpgpu_grm_merge_stats.argtypes = [vp]
    L.snpgpu_gnrPCA.argtypes = [c_int, c_int, c_int, c_int, ctypes.POINTER(dbl), vp, vp, vp,
                                ctypes.POINTER(dbl)]
    L.snpgpu_proj_create.argtypes = [i64, c_int, ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.snpgpu_proj_destroy.argtypes = [vp]
    L.snpgpu_proj_sync.argtypes = [vp]
    L.snpgpu_proj_set_eigvec.argtypes = [vp, vp, c_int]
    L.snpgpu_proj_snp_corr.argtypes = [vp, vp, i64, c_int, c_int, vp, c_int]
    L.snpgpu_proj_snp_loading.argtypes = [vp, vp, i64, c_int, c_int, c_int, vp, vp, vp, c_int]
    L.snpgpu_proj_samp_loading_feed.argtypes = [vp, vp, i64, c_int, c_int, vp, vp, vp, c_int]
    L.snpgpu_proj_samp_loading.argtypes = [vp, vp, c_int]
    L.snpgpu_proj_snp_loading_ext.argtypes = [vp, vp, i64, c_int, c_int, vp, vp, c_int, vp, c_int]
    L.snpgpu_gnrEigMixSNPLoading.argtypes = [vp, vp, c_int, vp, c_int, c_int, vp]
    L.snpgpu_gnrEigMixSampLoading.argtypes = [c_int, vp, vp, c_int, c_int, vp]
    L.snpgpu_proj_samp_loading_reset.argtypes = [vp]
    L.snpgpu_gnrPCA_randomized.argtypes = [c_int, c_int, c_int, vp, c_int, c_int, vp, vp, ctypes.POINTER(dbl)]
    L.snpgpu_gnrPCACorr.argtypes = [c_int, vp, c_int, c_int, vp]
    L.snpgpu_gnrPCASNPLoading.argtypes = [vp, vp, c_int, dbl, c_int, c_int, c_int, vp, vp, vp]
    L.snpgpu_gnrPCASampLoading.argtypes = [c_int, vp, vp, vp, c_int, c_int, vp]
    L.snpgpu_ld_create.argtypes = [i64, i64, c_int, i64, c_int, ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.snpgpu_ld_destroy.argtypes = [vp]
    L.snpgpu_ld_out_dims.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.snpgpu_ld_feed.argtypes = [vp, vp, i64, c_int, c_int]
    L.snpgpu_ld_result.argtypes = [vp, vp, c_int]
    L.snpgpu_ld_set_timing.argtypes = [vp, c_int]
    L.snpgpu_ld_get_timing.argtypes = [vp, c_int, ctypes.POINTER(dbl), ctypes.POINTER(i64)]
    L.snpgpu_ld_pair_tables.argtypes = [vp, i64, vp, i64, i64, c_int, vp, c_int]
    L.snpgpu_gnrLDMat.argtypes = [c_int, i64, c_int, c_int, c_int, vp]
    L.snpgpu_ibd_mle.argtypes = [vp, i64, i64, c_int, c_int, vp, c_int, dbl, c_int, i64, i64, vp, vp, vp, vp, c_int, c_int]
    L.snpgpu_ibd_loglik.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, vp, dbl, dbl, vp, vp, c_int, c_int]
    L.snpgpu_ibd_mle_stats.argtypes = [vp]
    L.snpgpu_gnrIBD_MLE.argtypes = [vp, c_int, c_int, dbl, c_int, c_int, c_int, c_int, c_int, vp, vp, vp, vp]
    L.snpgpu_ibd_mle_pairs.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, vp, i64, c_int, c_int, c_int, dbl, c_int, vp, vp, vp, vp, vp,
                                       c_int, c_int]
    L.snpgpu_ibd_mle_pairs_stats.argtypes = [vp]
    L.snpgpu_gnrIBD_MLE_Pairs.argtypes = [vp, vp, vp, i64, c_int, dbl, c_int, c_int, c_int, vp, vp, vp, vp, vp]
    L.snpgpu_ibd_jacquard_pairs.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, vp, i64, c_int, dbl, vp, vp, vp, vp, c_int, c_int]
    L.snpgpu_gnrIBD_MLE_PairsMethod.argtypes = [vp, vp, vp, i64, c_int, c_int, dbl, c_int, c_int, c_int, vp, vp, vp, vp]
    L.snpgpu_gnrIBD_LogLik.argtypes = [vp, vp, vp, vp]
    L.snpgpu_gnrIBD_LogLik_k01.argtypes = [vp, dbl, dbl, vp]
    L.snpgpu_diag_fp64_rate.argtypes = [c_int, dbl, ctypes.POINTER(dbl)]
    i32 = ctypes.c_int32
    L.snpgpu_ld_prune.argtypes = [vp, i64, i64, c_int, c_int, i64, vp, i32, i32, dbl, c_int, vp, ctypes.POINTER(Opts),
                                  ctypes.POINTER(LDPruneInfo)]
    L.snpgpu_ld_prune_bits.argtypes = [vp, i64, i64, c_int, c_int, i64, i64, dbl, c_int, vp, ctypes.POINTER(Opts),
                                       ctypes.POINTER(LDPruneInfo)]
    L.snpgpu_gnrLDpruning.argtypes = [i64, vp, i32, i32, dbl, c_int, c_int, c_int, vp]
    L.snpgpu_ld_score.argtypes = [vp, i64, i64, c_int, c_int, vp, i32, i32, c_int, c_int, vp, vp, vp, ctypes.POINTER(Opts),
                                  ctypes.POINTER(LDScoreInfo)]
    L.snpgpu_gnrLDScore.argtypes = [vp, i32, i32, c_int, c_int, c_int, c_int, vp, vp, vp]
    L.snpgpu_pop_counts.argtypes = [vp, i64, i64, c_int, c_int, vp, c_int, vp, vp, c_int, c_int]
    L.snpgpu_fst.argtypes = [vp, i64, i64, c_int, c_int, vp, c_int, c_int, vp, vp, vp, c_int]
    L.snpgpu_fst_windows.argtypes = [vp, i64, i64, c_int, c_int, vp, c_int, c_int, vp, vp, i64, vp, vp, vp, c_int]
    L.snpgpu_pop_stats.argtypes = [vp]
    L.snpgpu_gnrFst.argtypes = [vp, c_int, ctypes.c_char_p, vp, vp, vp]
    L.snpgpu_gnrSlidingWindowFst.argtypes = [vp, c_int, ctypes.c_char_p, vp, vp, i64, vp, vp, vp]
    L.snpgpu_geno_counts.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, c_int, c_int]
    L.snpgpu_hwe.argtypes = [vp, i64, i64, c_int, c_int, vp, c_int]
    L.snpgpu_hwe_counts.argtypes = [vp, i64, vp, c_int, c_int]
    L.snpgpu_ind_inb.argtypes = [vp, i64, i64, c_int, c_int, vp, c_int, dbl, vp, vp, vp, c_int, c_int]
    L.snpgpu_qc_stats.argtypes = [vp]
    L.snpgpu_gnrSampFreq.argtypes = [vp]
    L.snpgpu_gnrHWE.argtypes = [vp]
    L.snpgpu_gnrIndInb.argtypes = [vp, ctypes.c_char_p, dbl, c_int, c_int, vp, vp]
    u64 = ctypes.c_uint64
    L.snpgpu_hclust_average.argtypes = [i64, vp, i64, vp, vp, vp]
    L.snpgpu_dist_perm.argtypes = [vp, i64, c_int, vp, c_int, dbl, u64, vp, vp, vp, vp, vp, vp, vp, c_int]
    L.snpgpu_gnrDistPerm.argtypes = [c_int, vp, vp, c_int, dbl, u64, vp, vp, vp, vp, c_int]
    L.snpgpu_tree_stats.argtypes = [vp]
    L.snpgpu_pair_tables.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, i64, c_int, vp, vp, vp, c_int, c_int]
    L.snpgpu_pair_score_final.argtypes = [c_int, vp, vp, i64, c_int, c_int, vp]
    L.snpgpu_pair_score_matrix.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, i64, c_int, c_int, c_int, vp, c_int]
    L.snpgpu_gnrPairScore.argtypes = [vp, vp, i64, ctypes.c_char_p, ctypes.c_char_p, c_int, c_int, vp]
    L.snpgpu_pair_stats.argtypes = [vp]
    L.snpgpu_select_pairs.argtypes = [vp, ctypes.POINTER(SelOpts), i64, vp, vp, vp, vp, vp, c_int, ctypes.POINTER(i64)]
    L.snpgpu_multi_select_pairs.argtypes = [vp, ctypes.POINTER(SelOpts), i64, vp, vp, vp, vp, vp, c_int, ctypes.POINTER(i64)]
    L.snpgpu_gnrIBDPairs.argtypes = [c_int, vp, vp, c_int, dbl, vp, c_int, c_int, ctypes.POINTER(i64)]
    L.snpgpu_gnrIBDPairs_get.argtypes = [vp, vp, vp, vp, vp]
    L.snpgpu_select_stats.argtypes = [vp]
    L.snpgpu_select_grm.argtypes = [vp, ctypes.POINTER(GrmSelOpts), i64, vp, vp, vp, vp, ctypes.POINTER(dbl), ctypes.POINTER(i64)]
    L.snpgpu_multi_select_grm.argtypes = [vp, ctypes.POINTER(GrmSelOpts), i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.snpgpu_gnrGRMPairs.argtypes = [ctypes.c_char_p, dbl, vp, c_int, c_int, ctypes.POINTER(i64)]
    L.snpgpu_gnrGRMPairs_get.argtypes = [vp, vp, vp, vp, ctypes.POINTER(dbl)]
    L.snpgpu_select_grm_stats.argtypes = [vp]
    L.snpgpu_geno_select.argtypes = [ctypes.POINTER(GenoSrc), vp, i64, vp, i64, vp, c_int, c_int, vp]
    L.snpgpu_geno_select_stats.argtypes = [vp]
    L.snpgpu_geno_convert.argtypes = [ctypes.POINTER(GenoSrc), c_int, vp, i64, vp, i64, vp, c_int, c_int, c_int, c_int, vp]
    L.snpgpu_geno_convert_stats.argtypes = [vp]
    L.snpgpu_vcf_index.argtypes = [vp, i64, c_int, i64, i64, vp, vp, vp, vp]
    L.snpgpu_vcf_genotypes.argtypes = [vp, c_int, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, c_int, vp]
    L.snpgpu_vcf_stats.argtypes = [vp]
    L.snpgpu_text_render.argtypes = [vp, i64, i64, c_int, vp, vp, vp, vp, vp, vp, c_int, vp]
    L.snpgpu_text_stats.argtypes = [vp]
    L.snpgpu_ped_tokens.argtypes = [vp, i64, vp, vp, i64, i64, vp, vp, vp, c_int, vp]
    L.snpgpu_ped_census.argtypes = [vp, vp, i64, i64, vp, c_int, vp]
    L.snpgpu_ped_codes.argtypes = [vp, i64, i64, vp, vp, c_int, vp]
    L.snpgpu_ped_stats.argtypes = [vp]
    L.snpgpu_geno_merge.argtypes = [ctypes.POINTER(MergePart), c_int, i64, vp, c_int, vp]
    L.snpgpu_geno_merge_stats.argtypes = [vp]
    L.snpgpu_gen_genotypes.argtypes = [vp, c_int, i64, vp, vp, i64, i64, dbl, vp, vp, vp, c_int, vp]
    L.snpgpu_gen_line_host.argtypes = [ctypes.c_char_p, i64, i64, dbl, vp, vp, ctypes.c_char_p, i64]
    L.snpgpu_gen_stats.argtypes = [vp]
    L.snpgpu_mds.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, vp, ctypes.POINTER(dbl), ctypes.POINTER(c_int), c_int]
    L.snpgpu_mds_apply.argtypes = [vp, i64, i64, c_int, vp, c_int, vp, c_int]
    L.snpgpu_gnrMDS.argtypes = [c_int, c_int, vp, vp, vp, ctypes.POINTER(dbl), ctypes.POINTER(c_int)]
    L.snpgpu_mds_stats.argtypes = [vp]
    L.snpgpu_pcr_create.argtypes = [i64, c_int, vp, vp, dbl, c_int, ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.snpgpu_pcr_feed.argtypes = [vp, vp, i64, c_int, c_int, vp]
    L.snpgpu_pcr_result.argtypes = [vp, vp, vp, vp, vp, vp]
    L.snpgpu_pcr_sums.argtypes = [vp, c_int, vp]
    L.snpgpu_pcr_stats.argtypes = [vp, vp]
    L.snpgpu_pcr_destroy.argtypes = [vp]
    L.snpgpu_gnrPCRelate.argtypes = [c_int, vp, vp, dbl, c_int, vp, vp, vp, vp, vp]
    L.snpgpu_pcr_create_panel.argtypes = [i64, c_int, vp, vp, dbl, c_int, i64, i64, ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.snpgpu_pcr_panel_result.argtypes = [vp, vp, vp, vp, vp, vp]
    L.snpgpu_pcr_panel_sums.argtypes = [vp, c_int, vp]
    L.snpgpu_pcr_panel_stats.argtypes = [vp, vp]
    L.snpgpu_pcr_select.argtypes = [vp, ctypes.POINTER(PcrSelOpts), i64, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.snpgpu_pcr_select_stats.argtypes = [vp]
    L.snpgpu_gnrPCRelatePairs.argtypes = [c_int, vp, vp, dbl, c_int, i64, dbl, vp, c_int, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.snpgpu_gnrPCRelatePairs_get.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.snpgpu_admix_create.argtypes = [i64, c_int, i64, dbl, i64, ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.snpgpu_admix_feed.argtypes = [vp, vp, i64, c_int, c_int]
    L.snpgpu_admix_set.argtypes = [vp, vp, vp]
    L.snpgpu_admix_run.argtypes = [vp, c_int, dbl, c_int, vp, ctypes.POINTER(c_int)]
    L.snpgpu_admix_get.argtypes = [vp, vp, vp]
    L.snpgpu_admix_stats.argtypes = [vp, vp]
    L.snpgpu_admix_destroy.argtypes = [vp]
    L.snpgpu_gnrAdmix.argtypes = [c_int, dbl, i64, vp, vp, c_int, dbl, c_int, vp, ctypes.POINTER(c_int), vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise SnpGpuError(lib().snpgpu_last_error().decode("utf-8", "replace"))


def device_count():
    n = ctypes.c_int(0)
    check(lib().snpgpu_device_count(ctypes.byref(n)))
    return n.value


DIAG_F16_ZERO, DIAG_F16_EXACT_ROW, DIAG_F16_UV, DIAG_FP4, DIAG_F16_UV_16X16X32, DIAG_FP4_16X16X128, DIAG_F16_EXACT_ROW_16X16X32 = 0, 1, 2, 3, 4, 5, 6


def diag_mfma_rate(mode=DIAG_F16_UV, seconds=2.0, device=0):
    """(TFLOP/s, implied shader MHz) a register-only stream of the MFMA instruction of `mode` sustains on `device` right now
    (snpgpu_diag_mfma_rate: the power-capped rate the SYRK / pair-counter kernels run against)."""
    L = lib()
    r, mhz = ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(L.snpgpu_diag_mfma_rate(int(device), int(mode), float(seconds), ctypes.byref(r), ctypes.byref(mhz)))
    return r.value, mhz.value


def device_pci(device=0):
    """PCI address of HIP device `device` ("0000:05:00.0")"""
    buf = ctypes.create_string_buffer(64)
    check(lib().snpgpu_diag_device_pci(int(device), buf, 64))
    return buf.value.decode()


def diag_plan(kind, n_samp, block_snps=0, bayesian=False, rows=None, max_block_snps=0):
    """The kernel path a context would take under the current environment, as a dict of strings (snpgpu_diag_plan: the plan
    snpgpu_create allocates from, the kernels of a block with / without missing calls and, with block_snps, its fp32 run
    geometry).  No GPU is needed; what snpgpu_create would refuse whatever the device raises SnpGpuError with the same text."""
    o = Opts(0, int(bool(bayesian)), int(rows[0]) if rows else 0, int(rows[1]) if rows else 0, int(max_block_snps), None)
    buf = ctypes.create_string_buffer(8192)
    check(lib().snpgpu_diag_plan(int(kind), int(n_samp), ctypes.byref(o), int(block_snps), buf, len(buf)))
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def synth_block(dev_ptr, n_samp, snp_begin, n_snp, seed, missing=0.0, spectrum=0, special=False, device=0, stream=None):
    """Fill DEVICE memory at dev_ptr with SNPs [snp_begin, snp_begin + n_snp) of the seeded synthetic data set as
    2-bit rows [n_snp][ceil(n_samp/4)] (snpgpu_synth_block; counter-based, see oracle/synth.py for the CPU twin)."""
    check(lib().snpgpu_synth_block(ctypes.c_void_p(int(dev_ptr)), int(n_samp), int(snp_begin), int(n_snp),
                                   ctypes.c_uint32(int(seed) & 0xFFFFFFFF), float(missing), int(spectrum),
                                   int(bool(special)), int(device), ctypes.c_void_p(stream) if stream else None))


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _dptr(x):
    """a DEVICE address (int; 0 / None = absent) as the pointer argument of a call"""
    return ctypes.c_void_p(int(x)) if x else None


def _stats(name, k):
    """the k doubles of snpgpu_<name>_stats"""
    s = np.zeros(k, np.float64)
    check(getattr(lib(), "snpgpu_%s_stats" % name)(_ptr(s)))
    return s


def _text_input(text, n_bytes, text_mem):
    """text as the parsers take it -- bytes / a numpy uint8 array (host memory), or an address (int) with n_bytes, device memory
    unless text_mem says HOST or HOST_PINNED: (pointer, memory kind, n_bytes, what keeps the memory alive)"""
    if isinstance(text, int):
        if n_bytes is None:
            raise ValueError("a text address needs n_bytes")
        return ctypes.c_void_p(text), (DEVICE if text_mem is None else int(text_mem)), int(n_bytes), None
    keep = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
    n_bytes = keep.size if n_bytes is None else int(n_bytes)
    if n_bytes > keep.size:
        raise ValueError("n_bytes exceeds the text array")
    return _ptr(keep), (HOST if text_mem is None else int(text_mem)), n_bytes, keep


class PinnedBuffer:
    """Page-locked host block buffer (snpgpu_host_alloc) exposed as a numpy uint8 array."""

    def __init__(self, shape):
        self.shape = tuple(int(x) for x in shape)
        nbytes = int(np.prod(self.shape))
        p = ctypes.c_void_p()
        check(lib().snpgpu_host_alloc(nbytes, ctypes.byref(p)))
        self._p = p
        self.array = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)).reshape(self.shape)

    @property
    def ptr(self):
        return self._p.value

    def free(self):
        if self._p:
            self.array = None
            lib().snpgpu_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def tri_size(n):
    return n * (n + 1) // 2


def _select_pairs(fn, handle, n, what, cutoff, family, e, constraint, samp_sel, capacity, out_ptrs):
    """snpgpu_select_pairs / snpgpu_multi_select_pairs behind Accumulator.select_pairs and MultiAccumulator.select_pairs"""
    fam = None if family is None else np.ascontiguousarray(family, np.int32)
    ev = None if e is None else np.ascontiguousarray(e, np.float64)
    sel = None if samp_sel is None else np.ascontiguousarray(np.asarray(samp_sel) != 0, np.uint8)
    for name, a, size in (("family", fam, n), ("e", ev, 5), ("samp_sel", sel, n)):
        if a is not None and a.shape != (size,):
            raise ValueError("'%s' should have %d entries" % (name, size))
    o = SelOpts(int(what), int(bool(constraint)), _ptr(fam), _ptr(ev), float(cutoff), _ptr(sel))      # (fam, ev, sel stay alive to the end)
    found = ctypes.c_int64(0)
    if out_ptrs is not None:
        if capacity is None:
            raise ValueError("device outputs need a capacity")
        check(fn(handle, ctypes.byref(o), int(capacity), *[ctypes.c_void_p(int(x)) if x else None for x in out_ptrs], DEVICE,
                 ctypes.byref(found)))
        return None, None, None, None, None, found.value
    count_only = capacity is None or int(capacity) == 0
    if count_only:                         # capacity=None: count, then fetch everything
        check(fn(handle, ctypes.byref(o), 0, None, None, None, None, None, HOST, ctypes.byref(found)))
    capacity = found.value if capacity is None else int(capacity)
    out = [np.empty(capacity, np.int32), np.empty(capacity, np.int32)] + [np.empty(capacity, np.float64) for _ in range(3)]
    if capacity > 0:
        check(fn(handle, ctypes.byref(o), capacity, *[_ptr(a) for a in out], HOST, ctypes.byref(found)))
    m = min(capacity, found.value)
    out = [a[:m] for a in out]
    if int(what) == SEL_KING_ROBUST:
        out[3] = None                      # (not written for this kind)
    return out[0], out[1], out[2], out[3], out[4], found.value


def _select_grm(call, n, n_diag, what, cutoff, mode, scale, trace_in, samp_sel, capacity, diag_fill=float("nan")):
    """snpgpu_select_grm / snpgpu_multi_select_grm behind Accumulator.select_grm and MultiAccumulator.select_grm; call(opts, capacity,
    idx1, idx2, value, diag, found) runs one of them.  diag is fetched with the pairs (with the count when capacity is 0); the
    entries the call does not write keep diag_fill."""
    sel = None if samp_sel is None else np.ascontiguousarray(np.asarray(samp_sel) != 0, np.uint8)
    if sel is not None and sel.shape != (n,):
        raise ValueError("'samp_sel' should have %d entries" % n)
    o = GrmSelOpts(int(what), int(mode), float(scale), float(trace_in), float(cutoff), _ptr(sel))      # (sel stays alive to the end)
    found = ctypes.c_int64(0)
    diag = np.full(n_diag, diag_fill, np.float64)
    if capacity is None:                   # count, then fetch everything
        call(o, 0, None, None, None, None, found)
        capacity = found.value
    capacity = int(capacity)
    out = [np.empty(capacity, np.int32), np.empty(capacity, np.int32), np.empty(capacity, np.float64)]
    call(o, capacity, *([_ptr(a) for a in out] if capacity > 0 else [None] * 3), _ptr(diag), found)
    m = min(capacity, found.value)
    return out[0][:m], out[1][:m], out[2][:m], diag, found.value


class Accumulator:
    """One streaming accumulator context (level 1 of the C ABI)."""

    def __init__(self, kind, n_samp, device=0, bayesian=False, row_begin=0, row_end=0,
                 max_block_snps=0, stream=None):
        self.kind, self.n = kind, int(n_samp)
        o = Opts(int(device), int(bool(bayesian)), int(row_begin), int(row_end), int(max_block_snps),
                 ctypes.c_void_p(stream) if stream else None)
        h = ctypes.c_void_p()
        check(lib().snpgpu_create(int(kind), self.n, ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.row_begin = int(row_begin)
        self.row_end = int(row_end) if row_end else self.n
        self.full = (self.row_begin == 0 and self.row_end == self.n)

    def close(self):
        if self._h:
            lib().snpgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- feeding ---------------------------------------------------------
    def feed(self, geno, fmt=None):
        """geno: numpy uint8 [n_snp][n_samp] (U8) or [n_snp][ceil(n/4)] (PACKED2)."""
        g = np.ascontiguousarray(geno, dtype=np.uint8)
        if fmt is None:
            fmt = GENO_U8 if g.shape[1] == self.n else GENO_PACKED2
        exp = self.n if fmt == GENO_U8 else (self.n + 3) // 4
        if g.ndim != 2 or g.shape[1] != exp:
            raise ValueError("genotype block has the wrong shape")
        check(lib().snpgpu_feed(self._h, _ptr(g), g.shape[0], fmt, HOST))

    def feed_pinned(self, buf, n_snp, fmt=GENO_U8):
        """Asynchronous feed out of a PinnedBuffer (call host_wait(buf) before refilling it)."""
        check(lib().snpgpu_feed(self._h, ctypes.c_void_p(buf.ptr), int(n_snp), fmt, HOST_PINNED))

    def host_wait(self, buf):
        check(lib().snpgpu_host_wait(self._h, ctypes.c_void_p(buf.ptr)))

    def feed_device(self, dev_ptr, n_snp, fmt=GENO_PACKED2):
        check(lib().snpgpu_feed(self._h, ctypes.c_void_p(int(dev_ptr)), int(n_snp), fmt, DEVICE))

    def block_stats_device(self, dev_ptr, n_snp, sum_ptr, num_ptr, fmt=GENO_PACKED2):
        """per-SNP (sum, num) of `n_snp` rows at device address dev_ptr into device int32 arrays (snpgpu_block_stats)"""
        check(lib().snpgpu_block_stats(self._h, ctypes.c_void_p(int(dev_ptr)), int(n_snp), fmt, ctypes.c_void_p(int(sum_ptr)),
                                       ctypes.c_void_p(int(num_ptr))))

    def feed_device_stats(self, dev_ptr, n_snp, sum_ptr, num_ptr, fmt=GENO_PACKED2):
        check(lib().snpgpu_feed_stats(self._h, ctypes.c_void_p(int(dev_ptr)), int(n_snp), fmt, DEVICE, ctypes.c_void_p(int(sum_ptr)),
                                      ctypes.c_void_p(int(num_ptr))))

    def sync(self):
        check(lib().snpgpu_sync(self._h))

    def counts(self):
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().snpgpu_counts(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def carry_fallbacks(self, reset=True):
        """Work items of the single-product kernel that found no free slot of the carry scratch since the last reset
        (snpgpu_diag_carry_fallbacks; 0 for contexts without the scratch)."""
        n = ctypes.c_int64(0)
        check(lib().snpgpu_diag_carry_fallbacks(self._h, ctypes.byref(n), int(bool(reset))))
        return n.value

    def syrk_launches(self):
        """Kernel launches of the SYRK family enqueued by this context's feeds since it was created (snpgpu_diag_syrk_launches)."""
        n = ctypes.c_int64(0)
        check(lib().snpgpu_diag_syrk_launches(self._h, ctypes.byref(n)))
        return n.value

    def set_timing(self, on=True):
        check(lib().snpgpu_set_timing(self._h, int(on)))

    def get_timing(self, which):
        """(summed kernel ms, launches) of the pair kernel: which=0 popcount, 1 SYRK."""
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        check(lib().snpgpu_get_timing(self._h, int(which), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def slab_size(self):
        return lib().snpgpu_slab_size(self._h)

    def _shape(self, packed):
        return (self.slab_size(),) if packed else (self.n, self.n)

    # ---- finalisers --------------------------------------------------------
    def ibs_num(self, packed=False, out_ptrs=None):
        if out_ptrs is not None:
            check(lib().snpgpu_ibs_num(self._h, *[ctypes.c_void_p(int(x)) for x in out_ptrs], int(packed), DEVICE))
            return None
        o = [np.empty(self._shape(packed), np.int32) for _ in range(3)]
        check(lib().snpgpu_ibs_num(self._h, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), int(packed), HOST))
        return o

    def ibs_ave(self, packed=False, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_ibs_ave(self._h, _dptr(out_ptr), int(packed), DEVICE))
            return None
        o = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_ibs_ave(self._h, _ptr(o), int(packed), HOST))
        return o

    def king_robust_counts(self, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_king_robust_counts(self._h, _dptr(out_ptr), DEVICE))
            return None
        o = np.empty((self.slab_size(), 5), np.uint32)
        check(lib().snpgpu_king_robust_counts(self._h, _ptr(o), HOST))
        return o

    def king_robust(self, family=None, packed=False, out_ptrs=None):
        fam = None if family is None else np.ascontiguousarray(family, np.int32)
        if out_ptrs is not None:
            check(lib().snpgpu_king_robust(self._h, _ptr(fam), ctypes.c_void_p(int(out_ptrs[0])),
                                           ctypes.c_void_p(int(out_ptrs[1])), int(packed), DEVICE))
            return None
        a = np.empty(self._shape(packed), np.float64)
        b = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_king_robust(self._h, _ptr(fam), _ptr(a), _ptr(b), int(packed), HOST))
        return a, b

    def king_homo(self, packed=False, out_ptrs=None):
        if out_ptrs is not None:
            check(lib().snpgpu_king_homo(self._h, ctypes.c_void_p(int(out_ptrs[0])), ctypes.c_void_p(int(out_ptrs[1])), int(packed), DEVICE))
            return None
        a = np.empty(self._shape(packed), np.float64)
        b = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_king_homo(self._h, _ptr(a), _ptr(b), int(packed), HOST))
        return a, b

    def diss(self, packed=False, out_ptr=None):
        """Individual dissimilarity (gnrDiss); out_ptr: optional DEVICE pointer receiving the result."""
        if out_ptr is not None:
            check(lib().snpgpu_diss(self._h, ctypes.c_void_p(int(out_ptr)), int(packed), DEVICE))
            return None
        o = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_diss(self._h, _ptr(o), int(packed), HOST))
        return o

    def diss_sums(self, out_ptrs=None):
        """(SumGeno uint32, SumAFreq fp64), packed slab: numerator and denominator of the dissimilarity.  out_ptrs: two DEVICE
        pointers receiving them (then nothing is returned)."""
        if out_ptrs is not None:
            check(lib().snpgpu_diss_sums(self._h, _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), DEVICE))
            return None
        g = np.empty(self.slab_size(), np.uint32)
        w = np.empty(self.slab_size(), np.float64)
        check(lib().snpgpu_diss_sums(self._h, _ptr(g), _ptr(w), HOST))
        return g, w

    def grm_gcta(self, packed=False, out_ptr=None):
        """out_ptr: optional DEVICE pointer receiving the result (then nothing is returned)."""
        if out_ptr is not None:
            check(lib().snpgpu_grm_gcta(self._h, ctypes.c_void_p(int(out_ptr)), int(packed), DEVICE))
            return None
        o = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_grm_gcta(self._h, _ptr(o), int(packed), HOST))
        return o

    def pca_cov(self, packed=False, normalize=True, trace_in=0.0, want_matrix=True, out_ptr=None):
        tr = ctypes.c_double(0)
        if out_ptr is not None:
            check(lib().snpgpu_pca_cov(self._h, ctypes.c_void_p(int(out_ptr)), int(packed), int(normalize),
                                       float(trace_in), ctypes.byref(tr), DEVICE))
            return None, tr.value
        o = np.empty(self._shape(packed), np.float64) if want_matrix else None
        check(lib().snpgpu_pca_cov(self._h, _ptr(o), int(packed), int(normalize), float(trace_in),
                                   ctypes.byref(tr), HOST))
        return o, tr.value

    def ibd_mom(self, e, constraint=False, packed=False, out_ptrs=None):
        """e: the five expectations, host memory whatever the destination; out_ptrs: two DEVICE pointers (k0, k1)."""
        e = np.ascontiguousarray(e, np.float64)
        if out_ptrs is not None:
            check(lib().snpgpu_ibd_mom(self._h, _ptr(e), int(bool(constraint)), _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), int(packed),
                                       DEVICE))
            return None
        a = np.empty(self._shape(packed), np.float64)
        b = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_ibd_mom(self._h, _ptr(e), int(bool(constraint)), _ptr(a), _ptr(b), int(packed), HOST))
        return a, b

    def select_pairs(self, what, cutoff=float("nan"), family=None, e=None, constraint=False, samp_sel=None, capacity=None, out_ptrs=None):
        """The pairs idx1 < idx2 of this panel with kinship >= cutoff (non-finite: every pair) among the samples of samp_sel, in the order
        of snpgdsIBDSelection (snpgpu_select_pairs): (idx1, idx2, v0, v1, kinship, n_found) -- v0 / v1 = IBS0 / None for SEL_KING_ROBUST,
        k0 / k1 for SEL_KING_HOMO and SEL_MOM (needs e[5]); the arrays hold min(capacity, n_found) pairs, n_found counts all.
        capacity=None: counts first, then fetches all.  out_ptrs: five DEVICE pointers (0 / None = absent) of `capacity` elements
        each; then only n_found is returned."""
        return _select_pairs(lib().snpgpu_select_pairs, self._h, self.n, what, cutoff, family, e, constraint, samp_sel, capacity, out_ptrs)

    def eigmix(self, diagadj=True, scale=1.0, packed=False, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_eigmix(self._h, int(bool(diagadj)), float(scale), _dptr(out_ptr), int(packed), DEVICE))
            return None
        o = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_eigmix(self._h, int(bool(diagadj)), float(scale), _ptr(o), int(packed), HOST))
        return o

    def select_grm(self, what, cutoff=0.05, mode=0, scale=1.0, trace_in=0.0, samp_sel=None, capacity=None):
        """The sparse GRM of this panel (snpgpu_select_grm): (idx1, idx2, value, diag, avg_val, n_found) -- the pairs idx1 < idx2 with
        samp_sel[idx1] && samp_sel[idx2] and value >= cutoff (non-finite: every pair) in the order idx1, then idx2, with the value the
        kind's finaliser writes; diag: the finaliser's own entry of every row of the panel; avg_val: IndivBeta's average (0 otherwise).
        mode: EIGMIX's diagadj or IndivBeta's mode.  capacity=None fetches every pair; a number stores the first `capacity` (0: count)."""
        avg = ctypes.c_double(0)

        def call(o, cap, i1, i2, v, d, found):
            check(lib().snpgpu_select_grm(self._h, ctypes.byref(o), cap, i1, i2, v, d, ctypes.byref(avg), ctypes.byref(found)))
        r = _select_grm(call, self.n, min(self.row_end, self.n) - self.row_begin, what, cutoff, mode, scale, trace_in, samp_sel, capacity)
        return r[0], r[1], r[2], r[3], avg.value, r[4]

    def indiv_beta(self, mode=1, packed=False, out_ptr=None):
        """(matrix, grm_avg_value); out_ptr: a DEVICE pointer receiving the matrix, then (None, grm_avg_value) -- the average is a
        host scalar either way."""
        avg = ctypes.c_double(0)
        if out_ptr is not None:
            check(lib().snpgpu_indiv_beta(self._h, int(mode), _dptr(out_ptr), ctypes.byref(avg), int(packed), DEVICE))
            return None, avg.value
        o = np.empty(self._shape(packed), np.float64)
        check(lib().snpgpu_indiv_beta(self._h, int(mode), _ptr(o), ctypes.byref(avg), int(packed), HOST))
        return o, avg.value

    def pca_panel_trace(self):
        tr = ctypes.c_double(0)
        check(lib().snpgpu_pca_panel_trace(self._h, ctypes.byref(tr)))
        return tr.value

    def pca_panel_matmul(self, scale, q_ptr, m, y_ptr, fp32=False):
        """Y += scale * (this panel's part of C) Q; q_ptr/y_ptr: device pointers, column-major n x m.
        fp32: the product on fp32 matrix instructions (snpgpu_pca_panel_matmul_f32)."""
        fn = lib().snpgpu_pca_panel_matmul_f32 if fp32 else lib().snpgpu_pca_panel_matmul
        check(fn(self._h, float(scale), ctypes.c_void_p(int(q_ptr)), int(m), ctypes.c_void_p(int(y_ptr))))

    def finalize_inplace(self, diagadj=True, scale=1.0):
        """GRM_GCTA / EIGMIX: the accumulators become the final matrix in place (then usable by the eigen solver)."""
        check(lib().snpgpu_finalize_inplace(self._h, int(bool(diagadj)), float(scale)))

    def panel_entries(self, rows, cols):
        """fp64 result-plane entries (rows[k], cols[k]) of this panel (snpgpu_panel_entries)"""
        return panel_entries(self._h, rows, cols)

    def pca_eigen(self, k, out_ptr=None):
        """(eigenvalues [k], eigenvectors [n, k]); out_ptr: a DEVICE pointer receiving the eigenvectors ([k][n]), then
        (eigenvalues, None) -- the eigenvalues are host memory either way."""
        w = np.empty(k, np.float64)
        if out_ptr is not None:
            check(lib().snpgpu_pca_eigen(self._h, int(k), _ptr(w), _dptr(out_ptr), DEVICE))
            return w, None
        v = np.empty((k, self.n), np.float64)   # column-major n x k
        check(lib().snpgpu_pca_eigen(self._h, int(k), _ptr(w), _ptr(v), HOST))
        return w, v.T


def panel_entries(handle, rows, cols):
    r = np.ascontiguousarray(rows, np.int64)
    c = np.ascontiguousarray(cols, np.int64)
    out = np.empty(r.size, np.float64)
    check(lib().snpgpu_panel_entries(handle, _ptr(r), _ptr(c), r.size, _ptr(out)))
    return out


def ld_out_dims(n_snp, slide, mat_trim=False):
    """(rows, cols) of gnrLDMat's result: slide <= 0 -> n_snp x n_snp; else slide clamped to n_snp, slide x n_snp, or
    slide x (n_snp - slide) with mat_trim (src/genLD.cpp:983-1005)"""
    n_snp, slide = int(n_snp), int(slide)
    if slide <= 0:
        return n_snp, n_snp
    slide = min(slide, n_snp)
    return slide, (n_snp - slide if mat_trim else n_snp)


class LDMatrix:
    """One streaming LD object (snpgpu_ld, include/snpgpu.h section 1d): feed SNP blocks in file order, then result()
    returns the gnrLDMat matrix as a numpy array of R's dimensions (rows, cols)."""

    def __init__(self, n_samp, n_snp, method=LD_COMPOSITE, slide=250, mat_trim=False, device=0, max_block_snps=0, stream=None):
        self.n, self.L = int(n_samp), int(n_snp)
        o = Opts(int(device), 0, 0, 0, int(max_block_snps), ctypes.c_void_p(stream) if stream else None)
        h = ctypes.c_void_p()
        check(lib().snpgpu_ld_create(self.n, self.L, int(method), int(slide), int(bool(mat_trim)), ctypes.byref(o), ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().snpgpu_ld_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def dims(self):
        r, c = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().snpgpu_ld_out_dims(self._h, ctypes.byref(r), ctypes.byref(c)))
        return r.value, c.value

    def feed(self, geno, fmt=None):
        """geno: numpy uint8 [n_snp][n_samp] (U8) or [n_snp][ceil(n/4)] (PACKED2)."""
        g = np.ascontiguousarray(geno, dtype=np.uint8)
        if fmt is None:
            fmt = GENO_U8 if g.shape[1] == self.n else GENO_PACKED2
        exp = self.n if fmt == GENO_U8 else (self.n + 3) // 4
        if g.ndim != 2 or g.shape[1] != exp:
            raise ValueError("genotype block has the wrong shape")
        check(lib().snpgpu_ld_feed(self._h, _ptr(g), g.shape[0], fmt, HOST))

    def feed_device(self, dev_ptr, n_snp, fmt=GENO_PACKED2):
        check(lib().snpgpu_ld_feed(self._h, ctypes.c_void_p(int(dev_ptr)), int(n_snp), fmt, DEVICE))

    def result(self, out_ptr=None):
        """out_ptr: a DEVICE pointer receiving the rows x cols matrix, column-major (then nothing is returned)."""
        if out_ptr is not None:
            check(lib().snpgpu_ld_result(self._h, _dptr(out_ptr), DEVICE))
            return None
        r, c = self.dims()
        out = np.empty((c, r), np.float64)     # rows x cols column-major
        check(lib().snpgpu_ld_result(self._h, _ptr(out), HOST))
        return out.T

    def set_timing(self, on=True):
        check(lib().snpgpu_ld_set_timing(self._h, int(on)))

    def get_timing(self, which):
        """(summed ms, operations): which=0 table kernel, 1 finaliser, 2 device -> result copies."""
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        check(lib().snpgpu_ld_get_timing(self._h, int(which), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


def ld_pair_tables(geno_a, geno_b, n_samp, fmt=None, device=0):
    """int32 [n_a][n_b][3][3] genotype tables of every pair (row of A, row of B) (snpgpu_ld_pair_tables); rows in either format
    (fmt None: U8 when a row holds n_samp bytes -- pass it explicitly for a single sample, where both forms have one byte)."""
    n_samp = int(n_samp)
    a = np.ascontiguousarray(geno_a, dtype=np.uint8)
    b = np.ascontiguousarray(geno_b, dtype=np.uint8)
    if fmt is None:
        fmt = GENO_U8 if a.shape[1] == n_samp else GENO_PACKED2
    exp = n_samp if fmt == GENO_U8 else (n_samp + 3) // 4
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != exp or b.shape[1] != exp:
        raise ValueError("genotype rows have the wrong shape")
    tab = np.empty((a.shape[0], b.shape[0], 3, 3), np.int32)
    check(lib().snpgpu_ld_pair_tables(_ptr(a), a.shape[0], _ptr(b), b.shape[0], n_samp, fmt, _ptr(tab), int(device)))
    return tab


class LDPruneInfo(ctypes.Structure):
    """snpgpu_ld_prune_info (include/snpgpu.h section 1d)"""
    _fields_ = [("width", ctypes.c_int64), ("band_pairs", ctypes.c_int64), ("n_kept", ctypes.c_int64),
                ("table_launches", ctypes.c_int64), ("table_tiles", ctypes.c_int64), ("ms_stage", ctypes.c_double),
                ("ms_tables", ctypes.c_double), ("ms_bits", ctypes.c_double), ("ms_copy", ctypes.c_double),
                ("ms_scan", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _geno_input(geno, n_samp, fmt, n_snp, *, device_fmt_default):
    """(pointer, n_snp, format, memory kind, keep-alive) of host rows (numpy, U8 or PACKED2; fmt None: U8 when a row holds n_samp
    bytes) or device rows (an int address with n_snp; their fmt None means device_fmt_default, which is None where it must be
    named)"""
    n_samp = int(n_samp)
    if isinstance(geno, int):
        fmt = device_fmt_default if fmt is None else fmt
        if n_snp is None or fmt is None:
            raise ValueError("device rows need n_snp and fmt" if device_fmt_default is None else "device rows need n_snp")
        return ctypes.c_void_p(geno), int(n_snp), int(fmt), DEVICE, None
    g = np.ascontiguousarray(geno, dtype=np.uint8)
    if g.ndim != 2:
        raise ValueError("genotype rows have the wrong shape")
    if fmt is None:
        fmt = GENO_U8 if g.shape[1] == n_samp else GENO_PACKED2
    if g.shape[1] != (n_samp if fmt == GENO_U8 else (n_samp + 3) // 4):
        raise ValueError("genotype rows have the wrong shape")
    return _ptr(g), g.shape[0], int(fmt), HOST, g


def _pop_array(pop, n_samp):
    p = np.ascontiguousarray(pop, dtype=np.int32)
    if p.shape != (int(n_samp),):
        raise ValueError("pop should hold one population index per sample")
    return p


def ld_prune(geno, n_samp, pos_bp, start_idx, slide_max_bp, slide_max_n, ld_threshold, method=LD_COMPOSITE, fmt=None, n_snp=None,
             device=0, max_block_snps=0, stream=None):
    """Perform_LD_Pruning on one chromosome (snpgpu_ld_prune): (bool keep [n_snp], info dict).  geno: host rows (numpy, U8 or
    PACKED2; fmt None: U8 when a row holds n_samp bytes) or a device address (int) with n_snp and fmt; start_idx 0-based;
    the window limits are the reference's int32 values."""
    n_samp = int(n_samp)
    ptr, n, fmt, mem, _keep_alive = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=None)
    pos = np.ascontiguousarray(pos_bp, dtype=np.int32)
    if pos.shape != (n,):
        raise ValueError("pos_bp should hold one int32 per SNP")
    keep = np.zeros(n, np.uint8)
    o = Opts(device=int(device), max_block_snps=int(max_block_snps), stream=stream)
    info = LDPruneInfo()
    check(lib().snpgpu_ld_prune(ptr, n, n_samp, fmt, mem, int(start_idx), _ptr(pos), int(slide_max_bp), int(slide_max_n),
                                float(ld_threshold), int(method), _ptr(keep), ctypes.byref(o), ctypes.byref(info)))
    return keep.astype(bool), info.as_dict()


def ld_prune_bits(geno, n_samp, start_idx, width, ld_threshold, method=LD_COMPOSITE, fmt=None, n_snp=None, device=0,
                  max_block_snps=0):
    """The threshold bits snpgpu_ld_prune scans for a band of `width` (snpgpu_ld_prune_bits): bool [n_snp][width], entry
    [x, k - 1] for the pair (x, x + k); and the info dict."""
    n_samp = int(n_samp)
    ptr, n, fmt, mem, _keep_alive = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=None)
    wpr = (int(width) + 63) // 64
    words = np.zeros((n, max(wpr, 1)), np.uint64)
    o = Opts(device=int(device), max_block_snps=int(max_block_snps))
    info = LDPruneInfo()
    check(lib().snpgpu_ld_prune_bits(ptr, n, n_samp, fmt, mem, int(start_idx), int(width), float(ld_threshold), int(method),
                                     _ptr(words), ctypes.byref(o), ctypes.byref(info)))
    bits = np.unpackbits(words[:, :wpr].view(np.uint8).reshape(n, -1), axis=1, bitorder="little").astype(bool)
    return bits[:, :int(width)], info.as_dict()


class LDScoreInfo(ctypes.Structure):
    """snpgpu_ld_score_info (include/snpgpu.h section 1d)"""
    _fields_ = [(k, ctypes.c_int64) for k in ("width", "band_pairs", "window_pairs", "valid_pairs", "table_launches", "table_tiles")] + \
               [(k, ctypes.c_double) for k in ("ms_stage", "ms_tables", "ms_values", "ms_fold", "ms_copy")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def ld_score(geno, n_samp, pos_bp, slide_max_bp, slide_max_n, method=LD_CORR, adjust=True, include_self=True, fmt=None, n_snp=None,
             device=0, max_block_snps=0, stream=None):
    """LD scores of one chromosome (snpgpu_ld_score): (float64 score, int32 n_valid, int32 n_window, info dict), each [n_snp].
    geno: host rows (numpy, U8 or PACKED2; fmt None: U8 when a row holds n_samp bytes) or a device address (int) with n_snp and
    fmt; pos_bp: non-decreasing int32 positions, or None for a window in SNPs alone; the window limits are int32 values."""
    n_samp = int(n_samp)
    ptr, n, fmt, mem, _keep_alive = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=None)
    pos = None
    if pos_bp is not None:
        pos = np.ascontiguousarray(pos_bp, dtype=np.int32)
        if pos.shape != (n,):
            raise ValueError("pos_bp should hold one int32 per SNP")
    score = np.empty(n, np.float64)
    n_valid, n_window = np.empty(n, np.int32), np.empty(n, np.int32)
    o = Opts(device=int(device), max_block_snps=int(max_block_snps), stream=stream)
    info = LDScoreInfo()
    flags = (LDSCORE_ADJUST if adjust else 0) | (LDSCORE_SELF if include_self else 0)
    check(lib().snpgpu_ld_score(ptr, n, n_samp, fmt, mem, _ptr(pos), int(slide_max_bp), int(slide_max_n), int(method), flags,
                                _ptr(score), _ptr(n_valid), _ptr(n_window), ctypes.byref(o), ctypes.byref(info)))
    return score, n_valid, n_window, info.as_dict()


class MultiAccumulator:
    """snpgpu_multi: ONE host process driving several GPUs (the in-process counterpart of the one-process-per-GPU drivers
    of multigpu.py).  `devices` may repeat an ordinal (several panels' worth of "devices" on one GPU in tests)."""

    def __init__(self, kind, n_samp, devices=(0,), panels_per_device=1, n_passes=1, pass_index=0, bayesian=False,
                 max_block_snps=0):
        self.kind, self.n = kind, int(n_samp)
        self._devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
        mo = MultiOpts(self._devs, len(devices), int(panels_per_device), int(n_passes), int(pass_index))
        o = Opts(0, int(bool(bayesian)), 0, 0, int(max_block_snps), None)
        h = ctypes.c_void_p()
        check(lib().snpgpu_multi_create(int(kind), self.n, ctypes.byref(o), ctypes.byref(mo), ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().snpgpu_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().snpgpu_multi_info(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"n_panels": a.value, "uses_rccl": bool(b.value)}

    def status(self):
        """snpgpu_multi_get_status as a dict: devices (listed / distinct), panels, the resolved panels_per_device, whether RCCL carries
        the eigen exchanges, peer access (ordered pairs of distinct devices: all / enabled) and the self-test outcomes (-1 = not run)."""
        st = MultiStatus()
        check(lib().snpgpu_multi_get_status(self._h, ctypes.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in MultiStatus._fields_ if k != "reserved"}

    def comm_selftest(self):
        """One broadcast + sum-reduction of a known pattern over the devices through the exchange path in use, then a known 2-bit block
        through the feed-forward star and a known slab from every device through the gather path; raises on a wrong word.  Returns
        True when the exchange path is RCCL."""
        b = ctypes.c_int(0)
        check(lib().snpgpu_multi_comm_selftest(self._h, ctypes.byref(b)))
        return bool(b.value)

    def panels(self):
        """[(row_begin, row_end, device)] of the resident panels"""
        out = []
        for i in range(self.info()["n_panels"]):
            r0, r1, d = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
            check(lib().snpgpu_multi_panel(self._h, i, None, ctypes.byref(r0), ctypes.byref(r1), ctypes.byref(d)))
            out.append((r0.value, r1.value, d.value))
        return out

    def entries(self, rows, cols):
        """result entries (rows[k] <= cols[k]) wherever their panels live: snpgpu_panel_entries per resident panel"""
        rows = np.asarray(rows, np.int64)
        cols = np.asarray(cols, np.int64)
        out = np.full(rows.size, np.nan)
        for i in range(self.info()["n_panels"]):
            h, r0, r1, d = ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
            check(lib().snpgpu_multi_panel(self._h, i, ctypes.byref(h), ctypes.byref(r0), ctypes.byref(r1), ctypes.byref(d)))
            sel = (rows >= r0.value) & (rows < r1.value)
            if sel.any():
                out[sel] = panel_entries(h, rows[sel], cols[sel])
        return out

    def feed(self, geno, fmt=None):
        g = np.ascontiguousarray(geno, dtype=np.uint8)
        if fmt is None:
            fmt = GENO_U8 if g.shape[1] == self.n else GENO_PACKED2
        exp = self.n if fmt == GENO_U8 else (self.n + 3) // 4
        if g.ndim != 2 or g.shape[1] != exp:
            raise ValueError("genotype block has the wrong shape")
        check(lib().snpgpu_multi_feed(self._h, _ptr(g), g.shape[0], fmt, HOST))

    def feed_device(self, dev_ptr, n_snp, fmt=GENO_PACKED2):
        check(lib().snpgpu_multi_feed(self._h, ctypes.c_void_p(int(dev_ptr)), int(n_snp), fmt, DEVICE))

    def sync(self):
        check(lib().snpgpu_multi_sync(self._h))

    def counts(self):
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().snpgpu_multi_counts(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def _tri(self, dtype, cols=None):
        shape = (tri_size(self.n),) if cols is None else (tri_size(self.n), cols)
        return np.full(shape, -1 if np.issubdtype(dtype, np.integer) else np.nan, dtype)

    def ibs_num(self, out=None, out_ptrs=None):
        """out_ptrs (here and below: out_ptr / out_ptrs): DEVICE pointers on the first device receiving the packed triangle, then
        nothing is returned."""
        if out_ptrs is not None:
            check(lib().snpgpu_multi_ibs_num(self._h, *[_dptr(x) for x in out_ptrs], DEVICE))
            return None
        o = out or [self._tri(np.int32) for _ in range(3)]
        check(lib().snpgpu_multi_ibs_num(self._h, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), HOST))
        return o

    def king_robust(self, family=None, out=None, out_ptrs=None):
        fam = None if family is None else np.ascontiguousarray(family, np.int32)
        if out_ptrs is not None:
            check(lib().snpgpu_multi_king_robust(self._h, _ptr(fam), _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), DEVICE))
            return None
        a, b = out or (self._tri(np.float64), self._tri(np.float64))
        check(lib().snpgpu_multi_king_robust(self._h, _ptr(fam), _ptr(a), _ptr(b), HOST))
        return a, b

    def king_robust_counts(self, out=None, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_multi_king_robust_counts(self._h, _dptr(out_ptr), DEVICE))
            return None
        o = out if out is not None else np.zeros((tri_size(self.n), 5), np.uint32)
        check(lib().snpgpu_multi_king_robust_counts(self._h, _ptr(o), HOST))
        return o

    def king_homo(self, out=None, out_ptrs=None):
        if out_ptrs is not None:
            check(lib().snpgpu_multi_king_homo(self._h, _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), DEVICE))
            return None
        a, b = out or (self._tri(np.float64), self._tri(np.float64))
        check(lib().snpgpu_multi_king_homo(self._h, _ptr(a), _ptr(b), HOST))
        return a, b

    def ibs_ave(self, out=None, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_multi_ibs_ave(self._h, _dptr(out_ptr), DEVICE))
            return None
        o = out if out is not None else self._tri(np.float64)
        check(lib().snpgpu_multi_ibs_ave(self._h, _ptr(o), HOST))
        return o

    def eigmix(self, diagadj=True, scale=1.0, out=None, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_multi_eigmix(self._h, int(bool(diagadj)), float(scale), _dptr(out_ptr), DEVICE))
            return None
        o = out if out is not None else self._tri(np.float64)
        check(lib().snpgpu_multi_eigmix(self._h, int(bool(diagadj)), float(scale), _ptr(o), HOST))
        return o

    def diss(self, out=None, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_multi_diss(self._h, _dptr(out_ptr), DEVICE))
            return None
        o = out if out is not None else self._tri(np.float64)
        check(lib().snpgpu_multi_diss(self._h, _ptr(o), HOST))
        return o

    def grm_gcta(self, out=None, out_ptr=None):
        if out_ptr is not None:
            check(lib().snpgpu_multi_grm_gcta(self._h, ctypes.c_void_p(int(out_ptr)), DEVICE))
            return None
        o = out if out is not None else self._tri(np.float64)
        check(lib().snpgpu_multi_grm_gcta(self._h, _ptr(o), HOST))
        return o

    def select_pairs(self, what, cutoff=float("nan"), family=None, e=None, constraint=False, samp_sel=None, capacity=None, out_ptrs=None):
        """Accumulator.select_pairs over the resident panels in order of row_begin, concatenated (snpgpu_multi_select_pairs); host
        outputs only."""
        if out_ptrs is not None:
            raise ValueError("MultiAccumulator.select_pairs returns host arrays (out_ptrs is for Accumulator.select_pairs)")
        return _select_pairs(lib().snpgpu_multi_select_pairs, self._h, self.n, what, cutoff, family, e, constraint, samp_sel, capacity, None)

    def select_grm(self, what, cutoff=0.05, mode=0, scale=1.0, trace_in=0.0, samp_sel=None, capacity=None, diag_fill=float("nan")):
        """Accumulator.select_grm over the resident panels in order of row_begin, the pairs concatenated (snpgpu_multi_select_grm):
        (idx1, idx2, value, diag [n], n_found).  The rows of diag that no resident panel holds (n_passes > 1) keep diag_fill."""
        def call(o, cap, i1, i2, v, d, found):
            check(lib().snpgpu_multi_select_grm(self._h, ctypes.byref(o), cap, i1, i2, v, d, ctypes.byref(found)))
        return _select_grm(call, self.n, self.n, what, cutoff, mode, scale, trace_in, samp_sel, capacity, diag_fill)

    def pca_trace(self):
        """TraceXTX: the sum of the resident panels' diagonal parts (snpgpu_multi_pca_trace)"""
        tr = ctypes.c_double(0)
        check(lib().snpgpu_multi_pca_trace(self._h, ctypes.byref(tr)))
        return tr.value

    def pca_cov(self, normalize=True, want_matrix=True, out_ptr=None):
        tr = ctypes.c_double(0)
        if out_ptr is not None:
            check(lib().snpgpu_multi_pca_cov(self._h, _dptr(out_ptr), int(normalize), ctypes.byref(tr), DEVICE))
            return None, tr.value
        o = self._tri(np.float64) if want_matrix else None
        check(lib().snpgpu_multi_pca_cov(self._h, _ptr(o), int(normalize), ctypes.byref(tr), HOST))
        return o, tr.value

    def finalize_inplace(self, diagadj=True, scale=1.0):
        check(lib().snpgpu_multi_finalize_inplace(self._h, int(bool(diagadj)), float(scale)))

    def topk_eigen(self, k, scale=0.0, tol=1e-9, block=0, depth=0, seed=20240601, fp32_until=0.0, out_ptr=None):
        """(eigenvalues [k], eigenvectors [n, k], info) on the host; out_ptr: a DEVICE pointer on the first device receiving the
        eigenvectors ([k][n]), then (eigenvalues, None, info)"""
        opts = EigOpts(tol=float(tol), block=int(block), depth=int(depth), max_restarts=0, seed=int(seed), y_buf=None,
                       reduce=REDUCE_FN(), user=None, fp32_until=float(fp32_until))
        w = np.empty(k, np.float64)
        v = np.empty((k, self.n), np.float64)
        info = EigInfo()
        check(lib().snpgpu_multi_topk_eigen(self._h, float(scale), int(k), ctypes.byref(opts), _ptr(w),
                                            _ptr(v) if out_ptr is None else _dptr(out_ptr), HOST if out_ptr is None else DEVICE,
                                            ctypes.byref(info)))
        return w, (v.T if out_ptr is None else None), {"restarts": info.restarts, "matmuls": info.matmuls, "max_rel_residual": info.max_rel_residual,
                        "block": info.block, "depth": info.depth, "matmuls_fp32": info.matmuls_fp32}


class Projector:
    """RAII wrapper over snpgpu_proj (PCA projections, include/snpgpu.h section 1b).
    Matrices follow R's layouts: eigvec [n_eig][n_samp]; per-block results [n_snp][n_eig].

    Every block call takes the block as a numpy array (host), as a DEVICE address (int) with n_snp (and fmt, default 2-bit rows),
    or as None = the block staged by the previous call (n_snp defaults to its size).  Results go to new host arrays, or with
    out_ptr / out_ptrs to DEVICE memory (then nothing is returned).  A call whose every pointer is device memory is only enqueued
    on the projector's stream: sync() is its completion point (include/snpgpu.h)."""

    def __init__(self, n_samp, n_eig, device=0, max_block_snps=16384, stream=None):
        self._h = ctypes.c_void_p()
        self.n, self.k = int(n_samp), int(n_eig)
        self._staged = 0
        o = Opts(device=device, bayesian=0, row_begin=0, row_end=0, max_block_snps=max_block_snps,
                 stream=ctypes.c_void_p(stream) if stream else None)
        check(lib().snpgpu_proj_create(self.n, self.k, ctypes.byref(o), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().snpgpu_proj_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        """wait for everything enqueued on the projector's stream (snpgpu_proj_sync)"""
        check(lib().snpgpu_proj_sync(self._h))

    def reset(self):
        """zero the sample-loading accumulator (snpgpu_proj_samp_loading_reset; stream-ordered)"""
        check(lib().snpgpu_proj_samp_loading_reset(self._h))

    def _block(self, geno, n_snp=None, fmt=None):
        """(pointer, n_snp, format, memory kind, keep-alive) of a block call"""
        if geno is None:                               # the staged block
            n = self._staged if n_snp is None else int(n_snp)
            if n <= 0:
                raise ValueError("no staged block to reuse")
            return None, n, GENO_PACKED2, DEVICE, None
        if isinstance(geno, int):
            if n_snp is None:
                raise ValueError("device rows need n_snp")
            return ctypes.c_void_p(geno), int(n_snp), GENO_PACKED2 if fmt is None else int(fmt), DEVICE, None
        g = np.ascontiguousarray(geno, dtype=np.uint8)
        if fmt is None:
            fmt = GENO_U8 if g.shape[1] == self.n else GENO_PACKED2
        exp = self.n if fmt == GENO_U8 else (self.n + 3) // 4
        if g.ndim != 2 or g.shape[1] != exp:
            raise ValueError("genotype block has the wrong shape")
        return _ptr(g), g.shape[0], int(fmt), HOST, g

    def set_eigvec(self, eigvec):
        """eigvec: numpy [n_eig][n_samp], or a DEVICE address (int) of that array (stream-ordered)"""
        if isinstance(eigvec, int):
            check(lib().snpgpu_proj_set_eigvec(self._h, ctypes.c_void_p(eigvec), DEVICE))
            return
        e = np.ascontiguousarray(eigvec, dtype=np.float64)
        if e.shape != (self.k, self.n):
            raise ValueError("eigvec must be [n_eig][n_samp]")
        check(lib().snpgpu_proj_set_eigvec(self._h, _ptr(e), HOST))

    def snp_corr(self, geno, n_snp=None, fmt=None, out_ptr=None):
        ptr, n, fmt, mem, _keep = self._block(geno, n_snp, fmt)
        if out_ptr is not None:
            check(lib().snpgpu_proj_snp_corr(self._h, ptr, n, fmt, mem, _dptr(out_ptr), DEVICE))
            self._staged = n
            return None
        out = np.empty((n, self.k), dtype=np.float64)
        check(lib().snpgpu_proj_snp_corr(self._h, ptr, n, fmt, mem, _ptr(out), HOST))
        self._staged = n
        return out

    def snp_loading(self, geno, bayesian=False, n_snp=None, fmt=None, out_ptrs=None):
        """(loading [n_snp][n_eig], afreq [n_snp], scale [n_snp]); out_ptrs: three DEVICE pointers for them"""
        ptr, n, fmt, mem, _keep = self._block(geno, n_snp, fmt)
        if out_ptrs is not None:
            check(lib().snpgpu_proj_snp_loading(self._h, ptr, n, fmt, mem, int(bool(bayesian)), _dptr(out_ptrs[0]), _dptr(out_ptrs[1]),
                                                _dptr(out_ptrs[2]), DEVICE))
            self._staged = n
            return None
        out = np.empty((n, self.k), dtype=np.float64)
        af = np.empty(n, dtype=np.float64)
        sc = np.empty(n, dtype=np.float64)
        check(lib().snpgpu_proj_snp_loading(self._h, ptr, n, fmt, mem, int(bool(bayesian)), _ptr(out), _ptr(af), _ptr(sc), HOST))
        self._staged = n
        return out, af, sc

    def snp_loading_ext(self, geno, avg, scale, n_snp=None, fmt=None, out_ptr=None):
        """loading [n_snp][n_eig] with the caller's centring avg [n_snp] and scaling scale [n_snp] (snpgpu_proj_snp_loading_ext):
        both numpy arrays, or both DEVICE addresses (int)"""
        ptr, n, fmt, mem, _keep = self._block(geno, n_snp, fmt)
        if isinstance(avg, int) != isinstance(scale, int):
            raise ValueError("avg and scale are both host arrays or both device addresses")
        if isinstance(avg, int):
            pa, ps, in_mem = ctypes.c_void_p(avg), ctypes.c_void_p(scale), DEVICE
        else:
            av = np.ascontiguousarray(avg, dtype=np.float64)
            sv = np.ascontiguousarray(scale, dtype=np.float64)
            if av.shape != (n,) or sv.shape != (n,):
                raise ValueError("avg / scale do not match the block")
            pa, ps, in_mem = _ptr(av), _ptr(sv), HOST
        if out_ptr is not None:
            check(lib().snpgpu_proj_snp_loading_ext(self._h, ptr, n, fmt, mem, pa, ps, in_mem, _dptr(out_ptr), DEVICE))
            self._staged = n
            return None
        out = np.empty((n, self.k), dtype=np.float64)
        check(lib().snpgpu_proj_snp_loading_ext(self._h, ptr, n, fmt, mem, pa, ps, in_mem, _ptr(out), HOST))
        self._staged = n
        return out

    def samp_loading_feed(self, geno, sload, afreq, scale, n_snp=None, fmt=None):
        """sload / afreq / scale: three numpy arrays, or three DEVICE addresses (int) of [n_snp][n_eig], [n_snp], [n_snp]"""
        ptr, n, fmt, mem, _keep = self._block(geno, n_snp, fmt)
        dev = [isinstance(x, int) for x in (sload, afreq, scale)]
        if any(dev):
            if not all(dev):
                raise ValueError("sload / afreq / scale are all host arrays or all device addresses")
            check(lib().snpgpu_proj_samp_loading_feed(self._h, ptr, n, fmt, mem, ctypes.c_void_p(sload), ctypes.c_void_p(afreq),
                                                      ctypes.c_void_p(scale), DEVICE))
            self._staged = n
            return
        sl = np.ascontiguousarray(sload, dtype=np.float64)
        af = np.ascontiguousarray(afreq, dtype=np.float64)
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        if sl.shape != (n, self.k) or af.shape != (n,) or sc.shape != (n,):
            raise ValueError("sload / afreq / scale do not match the block")
        check(lib().snpgpu_proj_samp_loading_feed(self._h, ptr, n, fmt, mem, _ptr(sl), _ptr(af), _ptr(sc), HOST))
        self._staged = n

    def samp_loading(self, out_ptr=None):
        """the accumulated sample loadings [n_eig][n_samp]; the accumulator is left as it is (reset() clears it)"""
        if out_ptr is not None:
            check(lib().snpgpu_proj_samp_loading(self._h, _dptr(out_ptr), DEVICE))
            return None
        out = np.empty((self.k, self.n), dtype=np.float64)
        check(lib().snpgpu_proj_samp_loading(self._h, _ptr(out), HOST))
        return out


def diag_fp64_rate(seconds=2.0, device=0):
    """TFLOP/s a register-only v_fma_f64 stream sustains on `device` right now (snpgpu_diag_fp64_rate)."""
    r = ctypes.c_double(0)
    check(lib().snpgpu_diag_fp64_rate(int(device), float(seconds), ctypes.byref(r)))
    return r.value


def ibd_mle(geno, n_samp, allele_freq=None, max_niter=1000, reltol=float(np.sqrt(np.finfo(float).eps)), coeff_correct=True,
            rows=(0, 0), device=0, geno_dev_ptr=None, n_snp=None, out=None, out_ptrs=None):
    """snpgpu_ibd_mle on 2-bit rows [n_snp][ceil(n_samp/4)] (numpy, or device memory via geno_dev_ptr + n_snp):
    returns (k0, k1, niter, afreq) with k0 / k1 / niter full n x n and afreq as InitAFreq leaves it (-1 = none).
    rows = (r0, r1): only the pairs of those upper-triangle rows (and their mirrors) are written, into `out` = (k0, k1, niter)
    when given.  out_ptrs: DEVICE pointers (k0, k1, niter; niter may be None) of n x n elements each; then
    (None, None, None, afreq) is returned -- afreq is host memory either way."""
    ptr, n_snp, fmt, mem, _keep = _geno_input(geno if geno_dev_ptr is None else int(geno_dev_ptr), n_samp, GENO_PACKED2, n_snp,
                                              device_fmt_default=GENO_PACKED2)
    af_in = None if allele_freq is None else np.ascontiguousarray(allele_freq, np.float64)
    if out_ptrs is not None:
        af = np.empty(n_snp, np.float64)
        check(lib().snpgpu_ibd_mle(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), int(max_niter), float(reltol),
                                   int(bool(coeff_correct)), int(rows[0]), int(rows[1]), _dptr(out_ptrs[0]), _dptr(out_ptrs[1]),
                                   _dptr(out_ptrs[2]), _ptr(af), DEVICE, int(device)))
        return None, None, None, af
    if out is None:
        out = (np.empty((n_samp, n_samp), np.float64), np.empty((n_samp, n_samp), np.float64),
               np.empty((n_samp, n_samp), np.int32))
    k0, k1, nit = out
    af = np.empty(n_snp, np.float64)
    check(lib().snpgpu_ibd_mle(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), int(max_niter), float(reltol),
                               int(bool(coeff_correct)), int(rows[0]), int(rows[1]), _ptr(k0), _ptr(k1), _ptr(nit), _ptr(af),
                               HOST, int(device)))
    return k0, k1, nit, af


def ibd_mle_pairs(geno, n_samp, idx1, idx2, allele_freq=None, mode=0, kinship_constraint=False, max_niter=1000,
                  reltol=float(np.sqrt(np.finfo(float).eps)), coeff_correct=True, device=0, geno_dev_ptr=None, n_snp=None,
                  out_ptrs=None):
    """snpgpu_ibd_mle_pairs on 2-bit rows [n_snp][ceil(n_samp/4)] (numpy, or device memory via geno_dev_ptr + n_snp) for the
    pairs (idx1[t], idx2[t]), 0-based: returns (k0, k1, loglik, niter, afreq), the first four of one entry per pair.
    mode 0: EM; mode 1: the start values (method of moments), loglik NaN and niter 0; mode 2: the downhill simplex, niter =
    its count of function evaluations.  out_ptrs: DEVICE pointers (k0, k1, loglik, niter; the last two may be None) of n_pairs
    elements each; then (None, None, None, None, afreq) is returned.  idx1 / idx2 and afreq are host memory either way."""
    ptr, n_snp, fmt, mem, _keep = _geno_input(geno if geno_dev_ptr is None else int(geno_dev_ptr), n_samp, GENO_PACKED2, n_snp,
                                              device_fmt_default=GENO_PACKED2)
    af_in = None if allele_freq is None else np.ascontiguousarray(allele_freq, np.float64)
    i1, i2 = np.ascontiguousarray(idx1, np.int32), np.ascontiguousarray(idx2, np.int32)
    if i1.ndim != 1 or i1.shape != i2.shape:
        raise ValueError("idx1 and idx2 should be vectors of one length")
    P = i1.shape[0]
    if out_ptrs is not None:
        af = np.empty(n_snp, np.float64)
        check(lib().snpgpu_ibd_mle_pairs(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), _ptr(i1), _ptr(i2), P, int(mode),
                                         int(bool(kinship_constraint)), int(max_niter), float(reltol), int(bool(coeff_correct)),
                                         _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), _dptr(out_ptrs[2]), _dptr(out_ptrs[3]), _ptr(af),
                                         DEVICE, int(device)))
        return None, None, None, None, af
    k0, k1, ll, nit = np.empty(P, np.float64), np.empty(P, np.float64), np.empty(P, np.float64), np.empty(P, np.int32)
    af = np.empty(n_snp, np.float64)
    check(lib().snpgpu_ibd_mle_pairs(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), _ptr(i1), _ptr(i2), P, int(mode),
                                     int(bool(kinship_constraint)), int(max_niter), float(reltol), int(bool(coeff_correct)),
                                     _ptr(k0), _ptr(k1), _ptr(ll), _ptr(nit), _ptr(af), HOST, int(device)))
    return k0, k1, ll, nit, af


def ibd_jacquard_pairs(geno, n_samp, idx1, idx2, allele_freq=None, max_niter=1000, reltol=float(np.sqrt(np.finfo(float).eps)),
                       device=0, geno_dev_ptr=None, n_snp=None, out_ptrs=None):
    """snpgpu_ibd_jacquard_pairs on 2-bit rows (as ibd_mle_pairs) for the pairs (idx1[t], idx2[t]): returns (D, loglik, niter,
    afreq) with D [8][n_pairs] = D1 ... D8.  SNPs at which both samples carry code 2 are skipped, as in the reference.
    out_ptrs: DEVICE pointers (D [8][n_pairs], loglik, niter; the last two may be None); then (None, None, None, afreq) is returned."""
    ptr, n_snp, fmt, mem, _keep = _geno_input(geno if geno_dev_ptr is None else int(geno_dev_ptr), n_samp, GENO_PACKED2, n_snp,
                                              device_fmt_default=GENO_PACKED2)
    af_in = None if allele_freq is None else np.ascontiguousarray(allele_freq, np.float64)
    i1, i2 = np.ascontiguousarray(idx1, np.int32), np.ascontiguousarray(idx2, np.int32)
    if i1.ndim != 1 or i1.shape != i2.shape:
        raise ValueError("idx1 and idx2 should be vectors of one length")
    P = i1.shape[0]
    if out_ptrs is not None:
        af = np.empty(n_snp, np.float64)
        check(lib().snpgpu_ibd_jacquard_pairs(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), _ptr(i1), _ptr(i2), P, int(max_niter),
                                              float(reltol), _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), _dptr(out_ptrs[2]), _ptr(af),
                                              DEVICE, int(device)))
        return None, None, None, af
    d, ll, nit = np.empty((8, P), np.float64), np.empty(P, np.float64), np.empty(P, np.int32)
    af = np.empty(n_snp, np.float64)
    check(lib().snpgpu_ibd_jacquard_pairs(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), _ptr(i1), _ptr(i2), P, int(max_niter),
                                          float(reltol), _ptr(d), _ptr(ll), _ptr(nit), _ptr(af), HOST, int(device)))
    return d, ll, nit, af


def ibd_mle_pairs_stats():
    """(kernel ms, all kernels ms, wave-sweeps, pairs) of the last ibd_mle_pairs / ibd_jacquard_pairs on this thread"""
    s = _stats("ibd_mle_pairs", 4)
    return float(s[0]), float(s[1]), int(s[2]), int(s[3])


def pop_counts(geno, n_samp, pop, n_pop, fmt=None, n_snp=None, device=0, out_ptrs=None):
    """(ACnt, Cnt) int32 [n_snp][n_pop] of snpgpu_pop_counts: per SNP and population the sum of the called genotypes and twice
    the number of called samples.  geno: host rows (numpy, U8 or PACKED2) or a device address (int) with n_snp (and fmt);
    pop: 0-based population index per sample (host memory); out_ptrs: two DEVICE pointers receiving the arrays."""
    p = _pop_array(pop, n_samp)
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    if out_ptrs is not None:
        check(lib().snpgpu_pop_counts(ptr, n, int(n_samp), fmt, mem, _ptr(p), int(n_pop), _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), DEVICE,
                                      int(device)))
        return None
    a = np.empty((n, int(n_pop)), np.int32)
    c = np.empty((n, int(n_pop)), np.int32)
    check(lib().snpgpu_pop_counts(ptr, n, int(n_samp), fmt, mem, _ptr(p), int(n_pop), _ptr(a), _ptr(c), HOST, int(device)))
    return a, c


def fst(geno, n_samp, pop, n_pop, method=FST_WC84, fmt=None, n_snp=None, device=0):
    """snpgpu_fst: (Fst, FstSNP [n_snp], Beta [n_pop][n_pop] or None)"""
    p = _pop_array(pop, n_samp)
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    f = ctypes.c_double(0)
    per = np.empty(n, np.float64)
    beta = np.empty((int(n_pop), int(n_pop)), np.float64) if int(method) == FST_WH02 else None
    check(lib().snpgpu_fst(ptr, n, int(n_samp), fmt, mem, _ptr(p), int(n_pop), int(method), ctypes.byref(f), _ptr(per), _ptr(beta),
                           int(device)))
    return f.value, per, beta


def fst_windows(geno, n_samp, pop, n_pop, offsets, snp_index, method=FST_WC84, fmt=None, n_snp=None, device=0):
    """snpgpu_fst_windows: (Fst per window, FstSNP [n_snp], Beta [n_win][n_pop][n_pop] or None) for CSR windows"""
    p = _pop_array(pop, n_samp)
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    off = np.ascontiguousarray(offsets, np.int64)
    idx = np.ascontiguousarray(snp_index, np.int32)
    n_win = len(off) - 1
    f = np.empty(max(n_win, 0), np.float64)
    per = np.empty(n, np.float64)
    beta = np.empty((max(n_win, 0), int(n_pop), int(n_pop)), np.float64) if int(method) == FST_WH02 else None
    check(lib().snpgpu_fst_windows(ptr, n, int(n_samp), fmt, mem, _ptr(p), int(n_pop), int(method), _ptr(off), _ptr(idx), n_win,
                                   _ptr(f), _ptr(beta), _ptr(per), int(device)))
    return f, per, beta


def pop_stats():
    """(counter kernel ms, its launches, Fst kernels ms, genotype bytes read, launches of the W&H02 window sums) of the last
    pop_counts / fst call on this thread"""
    s = _stats("pop", 5)
    return float(s[0]), int(s[1]), float(s[2]), float(s[3]), int(s[4])


def geno_counts(geno, n_samp, fmt=None, n_snp=None, device=0, want_snp=True, want_samp=True, out_ptrs=None):
    """(snp_cnt int32 [n_snp][3] for g = 0, 1, 2; samp_missing int32 [n_samp]) of snpgpu_geno_counts; None for a part not asked
    for.  geno: host rows (numpy, U8 or PACKED2) or a device address (int) with n_snp (and fmt).  out_ptrs: two DEVICE pointers
    (either may be None = not asked for) receiving the arrays."""
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    if out_ptrs is not None:
        check(lib().snpgpu_geno_counts(ptr, n, int(n_samp), fmt, mem, _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), DEVICE, int(device)))
        return None
    c = np.empty((n, 3), np.int32) if want_snp else None
    m = np.empty(int(n_samp), np.int32) if want_samp else None
    check(lib().snpgpu_geno_counts(ptr, n, int(n_samp), fmt, mem, _ptr(c), _ptr(m), HOST, int(device)))
    return c, m


def hwe(geno, n_samp, fmt=None, n_snp=None, device=0):
    """snpgpu_hwe: p-value of the exact test of Hardy-Weinberg equilibrium per SNP (NaN without a call)"""
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    p = np.empty(n, np.float64)
    check(lib().snpgpu_hwe(ptr, n, int(n_samp), fmt, mem, _ptr(p), int(device)))
    return p


def hwe_counts(snp_cnt, device=0, n_snp=None, out_ptr=None):
    """snpgpu_hwe_counts on host counts int32 [n_snp][3] (g = 0, 1, 2); or with snp_cnt a DEVICE address (int), n_snp and out_ptr
    (DEVICE, n_snp doubles): the memory kind covers the counts and the p-values alike"""
    if isinstance(snp_cnt, int) or out_ptr is not None:
        if not (isinstance(snp_cnt, int) and out_ptr is not None and n_snp is not None):
            raise ValueError("device counts go with a device result (and n_snp)")
        check(lib().snpgpu_hwe_counts(ctypes.c_void_p(snp_cnt), int(n_snp), _dptr(out_ptr), DEVICE, int(device)))
        return None
    c = np.ascontiguousarray(snp_cnt, np.int32)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("snp_cnt should be [n_snp][3]")
    p = np.empty(c.shape[0], np.float64)
    check(lib().snpgpu_hwe_counts(_ptr(c), c.shape[0], _ptr(p), HOST, int(device)))
    return p


def ind_inb(geno, n_samp, method="mom.weir", allele_freq=None, reltol=float(np.finfo(float).eps ** 0.75), fmt=None, n_snp=None,
            device=0, out_ptrs=None):
    """snpgpu_ind_inb: (coeff [n_samp], niter int32 [n_samp] or None unless "mle", afreq [n_snp] as used).  out_ptrs: DEVICE
    pointers (coeff, niter; niter may be None); then (None, None, afreq) is returned -- afreq is host memory either way."""
    if method not in INB_METHODS:
        raise ValueError("'method' should be one of %s" % ", ".join('"%s"' % m for m in INB_METHODS))
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    af_in = None if allele_freq is None else np.ascontiguousarray(allele_freq, np.float64)
    if af_in is not None and af_in.shape != (n,):
        raise ValueError("allele_freq should hold one frequency per SNP")
    code = INB_METHODS.index(method) + 1
    if out_ptrs is not None:
        af = np.empty(n, np.float64)
        check(lib().snpgpu_ind_inb(ptr, n, int(n_samp), fmt, mem, _ptr(af_in), code, float(reltol), _dptr(out_ptrs[0]),
                                   _dptr(out_ptrs[1]), _ptr(af), DEVICE, int(device)))
        return None, None, af
    coeff = np.empty(int(n_samp), np.float64)
    nit = np.empty(int(n_samp), np.int32) if code == INB_MLE else None
    af = np.empty(n, np.float64)
    check(lib().snpgpu_ind_inb(ptr, n, int(n_samp), fmt, mem, _ptr(af_in), code, float(reltol), _ptr(coeff), _ptr(nit), _ptr(af),
                               HOST, int(device)))
    return coeff, nit, af


def qc_stats():
    """dict of snpgpu_qc_stats for the last geno_counts / hwe / hwe_counts / ind_inb call on this thread"""
    s = _stats("qc", 8)
    return dict(count_ms=float(s[0]), count_launches=int(s[1]), count_bytes=float(s[2]), mom_ms=float(s[3]), mle_ms=float(s[4]),
                mle_lane_steps_useful=int(s[5]), mle_lane_steps_issued=int(s[6]), hwe_ms=float(s[7]))


def ibd_mle_stats():
    """(EM kernel ms, all kernels ms, useful lane-sweeps, issued lane-sweeps) of the last ibd_mle on this thread"""
    s = _stats("ibd_mle", 4)
    return float(s[0]), float(s[1]), int(s[2]), int(s[3])


def ibd_loglik(geno, n_samp, allele_freq=None, k0=None, k1=None, k0_all=float("nan"), k1_all=float("nan"), device=0, n_snp=None,
               out_ptr=None):
    """snpgpu_ibd_loglik: EM_LogLik of every pair at the n x n (k0, k1), or at the global pair when k0 / k1 are None.  out_ptr: a
    DEVICE pointer receiving the n x n result; k0 / k1 are then DEVICE addresses (int) too, or None: the result's memory kind
    covers them."""
    ptr, n_snp, fmt, mem, _keep = _geno_input(geno, n_samp, GENO_PACKED2, n_snp, device_fmt_default=GENO_PACKED2)
    af_in = None if allele_freq is None else np.ascontiguousarray(allele_freq, np.float64)
    if out_ptr is not None:
        if not all(x is None or isinstance(x, int) for x in (k0, k1)):
            raise ValueError("with a device result k0 / k1 are device addresses")
        check(lib().snpgpu_ibd_loglik(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), _dptr(k0), _dptr(k1), float(k0_all),
                                      float(k1_all), _dptr(out_ptr), None, DEVICE, int(device)))
        return None
    if isinstance(k0, int) or isinstance(k1, int):
        raise ValueError("device k0 / k1 go with a device result (out_ptr)")
    m0 = None if k0 is None else np.ascontiguousarray(k0, np.float64)
    m1 = None if k1 is None else np.ascontiguousarray(k1, np.float64)
    out = np.empty((n_samp, n_samp), np.float64)
    check(lib().snpgpu_ibd_loglik(ptr, n_snp, int(n_samp), fmt, mem, _ptr(af_in), _ptr(m0), _ptr(m1),
                                  float(k0_all), float(k1_all), _ptr(out), None, HOST, int(device)))
    return out


def hclust_average(dist):
    """snpgpu_hclust_average on a square float64 matrix (its lower triangle): (merge int32 [n - 1][2], height [n - 1],
    order int32 [n]) as R's hclust(as.dist(dist), method = "average") returns them.  Host code, no device."""
    d = np.ascontiguousarray(dist, np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("dist should be a square matrix")
    n = d.shape[0]
    merge = np.zeros((max(n - 1, 0), 2), np.int32)
    height = np.zeros(max(n - 1, 0), np.float64)
    order = np.zeros(n, np.int32)
    check(lib().snpgpu_hclust_average(n, _ptr(d), n, _ptr(merge), _ptr(height), _ptr(order)))
    return merge, height, order


def dist_perm(dist, merge, n_perm=5000, z_threshold=15.0, seed=0, device=0, n=None):
    """snpgpu_dist_perm: dict(z, n1, n2, group, obs, perm_mean, perm_sd).  dist: a square float64 numpy matrix, or a device
    address (int) with n; merge: int32 [n - 1][2] in R's convention."""
    if isinstance(dist, int):
        if n is None:
            raise ValueError("a device matrix needs n")
        ptr, mem, n = ctypes.c_void_p(dist), DEVICE, int(n)
    else:
        d = np.ascontiguousarray(dist, np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError("dist should be a square matrix")
        ptr, mem, n = _ptr(d), HOST, d.shape[0]
    mg = np.ascontiguousarray(merge, np.int32)
    if mg.shape != (n - 1, 2):
        raise ValueError("merge should be [n - 1][2]")
    nm = max(n - 1, 0)
    z, obs, mean, sd = (np.zeros(nm, np.float64) for _ in range(4))
    n1, n2, group = np.zeros(nm, np.int32), np.zeros(nm, np.int32), np.zeros(n, np.int32)
    check(lib().snpgpu_dist_perm(ptr, n, mem, _ptr(mg), int(n_perm), float(z_threshold), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(z),
                                 _ptr(n1), _ptr(n2), _ptr(group), _ptr(obs), _ptr(mean), _ptr(sd), int(device)))
    return dict(z=z, n1=n1, n2=n2, group=group, obs=obs, perm_mean=mean, perm_sd=sd)


def tree_stats():
    """dict of snpgpu_tree_stats for the last dist_perm on this thread"""
    s = _stats("tree", 6)
    return dict(prep_ms=float(s[0]), perm_ms=float(s[1]), prep_launches=int(s[2]), perm_launches=int(s[3]), gathered=float(s[4]),
                permutations=float(s[5]))


def _pair_lists(idx1, idx2):
    a, b = np.ascontiguousarray(idx1, np.int32), np.ascontiguousarray(idx2, np.int32)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("idx1 and idx2 should be two lists of the same length")
    return a, b


def _pair_method(method):
    if method not in PAIR_METHODS:
        raise ValueError("'method' should be one of %s" % ", ".join('"%s"' % m for m in PAIR_METHODS))
    return PAIR_METHODS.index(method) + 1


def pair_tables(geno, n_samp, idx1, idx2, need_major=False, fmt=None, n_snp=None, device=0, want_pair=True, want_snp=True,
                want_flip=True, out_ptrs=None):
    """(pair_tab int64 [n_pair][3][3], snp_tab int32 [n_snp][4][4], flip uint8 [n_snp]) of snpgpu_pair_tables; None for a part
    not asked for.  geno: host rows (numpy, U8 or PACKED2) or a device address (int) with n_snp (and fmt); idx1 / idx2: 0-based
    sample indices of the pairs (host memory).  out_ptrs: three DEVICE pointers (any may be None = not asked for, not all)
    receiving the tables."""
    a, b = _pair_lists(idx1, idx2)
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    if out_ptrs is not None:
        check(lib().snpgpu_pair_tables(ptr, n, int(n_samp), fmt, mem, _ptr(a), _ptr(b), len(a), int(bool(need_major)),
                                       _dptr(out_ptrs[0]), _dptr(out_ptrs[1]), _dptr(out_ptrs[2]), DEVICE, int(device)))
        return None
    pt = np.empty((len(a), 3, 3), np.int64) if want_pair else None
    st = np.empty((n, 4, 4), np.int32) if want_snp else None
    fl = np.empty(n, np.uint8) if want_flip else None
    check(lib().snpgpu_pair_tables(ptr, n, int(n_samp), fmt, mem, _ptr(a), _ptr(b), len(a), int(bool(need_major)), _ptr(pt), _ptr(st),
                                   _ptr(fl), HOST, int(device)))
    return pt, st, fl


def pair_score_final(table, method="IBS", dosage=True, flip=None):
    """snpgpu_pair_score_final (host code, no device): (Avg, SD, Num) float64 [n] each from a pair table [n][3][3] (int64, counted
    with need_major as the method needs) or from a SNP table [n][4][4] (int32) with its flip bytes."""
    t = np.asarray(table)
    if t.ndim == 3 and t.shape[1:] == (3, 3):
        t, kind = np.ascontiguousarray(t, np.int64), PAIR_TABLE
    elif t.ndim == 3 and t.shape[1:] == (4, 4):
        t, kind = np.ascontiguousarray(t, np.int32), SNP_TABLE
    else:
        raise ValueError("table should be [n][3][3] (pairs) or [n][4][4] (SNPs)")
    f = None if flip is None else np.ascontiguousarray(flip, np.uint8)
    if f is not None and f.shape != (t.shape[0],):
        raise ValueError("flip should hold one byte per row of the table")
    n = t.shape[0]
    out = np.empty(3 * n, np.float64)
    check(lib().snpgpu_pair_score_final(kind, _ptr(t), _ptr(f), n, _pair_method(method), int(bool(dosage)), _ptr(out)))
    r = out.reshape(3, n) if kind == PAIR_TABLE else out.reshape(n, 3).T
    return r[0].copy(), r[1].copy(), r[2].copy()


def pair_score_matrix(geno, n_samp, idx1, idx2, method="IBS", dosage=True, bit2=False, fmt=None, n_snp=None, device=0):
    """snpgpu_pair_score_matrix: [n_snp][n_pair] int32 (INT_MIN = missing), or with bit2 uint8 holding the two bits of a bit2 node"""
    a, b = _pair_lists(idx1, idx2)
    ptr, n, fmt, mem, _keep = _geno_input(geno, n_samp, fmt, n_snp, device_fmt_default=GENO_PACKED2)
    out = np.empty((n, len(a)), np.uint8 if bit2 else np.int32)
    check(lib().snpgpu_pair_score_matrix(ptr, n, int(n_samp), fmt, mem, _ptr(a), _ptr(b), len(a), _pair_method(method), int(bool(dosage)),
                                         PAIR_ELEM_BIT2 if bit2 else PAIR_ELEM_INT32, _ptr(out), int(device)))
    return out


def _geno_convert(call, src, major, n_rows, n_cols, bit0, row_stride_bits, row_bit, samp_index, snp_index, out, device, n_bytes, mem,
                  out_mem, stream, dst_major=0):
    """the argument handling geno_select and geno_convert share; call(desc, samp, n_samp_out, snp, n_snp_out, out pointer, out_mem,
    device, stream) is the C entry point"""
    keep = None
    if isinstance(src, int):
        if n_bytes is None:
            raise ValueError("a source address needs n_bytes")
        ptr, mem = ctypes.c_void_p(src), (DEVICE if mem is None else int(mem))
    else:
        keep = np.ascontiguousarray(src, dtype=np.uint8)
        ptr, mem = _ptr(keep), (HOST if mem is None else int(mem))
        n_bytes = keep.size if n_bytes is None else int(n_bytes)
        if n_bytes > keep.size:
            raise ValueError("n_bytes exceeds the source array")
    major, n_rows, n_cols = int(major), int(n_rows), int(n_cols)
    rbit = None if row_bit is None else np.ascontiguousarray(row_bit, dtype=np.int64)
    if rbit is not None and rbit.shape != (n_rows,):
        raise ValueError("row_bit should hold one bit position per source row")
    samp = None if samp_index is None else np.ascontiguousarray(samp_index, dtype=np.int32).reshape(-1)
    snp = None if snp_index is None else np.ascontiguousarray(snp_index, dtype=np.int32).reshape(-1)
    n_samp_out = (n_rows if major else n_cols) if samp is None else samp.size
    n_snp_out = (n_cols if major else n_rows) if snp is None else snp.size
    shape = (n_samp_out, (n_snp_out + 3) // 4) if dst_major else (n_snp_out, (n_samp_out + 3) // 4)
    if out is None:
        out = np.empty(shape, np.uint8)
    if isinstance(out, int):
        optr, out_mem = ctypes.c_void_p(out), (DEVICE if out_mem is None else int(out_mem))
    else:
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size == shape[0] * shape[1]):
            raise ValueError("out should be a contiguous uint8 array of n_samp_out * ceil(n_snp_out / 4) bytes" if dst_major else
                             "out should be a contiguous uint8 array of n_snp_out * ceil(n_samp_out / 4) bytes")
        optr, out_mem = _ptr(out), (HOST if out_mem is None else int(out_mem))
    d = GenoSrc(ptr, mem, major, n_rows, n_cols, int(bit0), 2 * n_cols if row_stride_bits is None else int(row_stride_bits),
                None if rbit is None else rbit.ctypes.data, int(n_bytes))
    check(call(ctypes.byref(d), _ptr(samp), n_samp_out, _ptr(snp), n_snp_out, optr, out_mem, int(device),
               ctypes.c_void_p(stream) if stream else None))
    return out


def geno_select(src, major, n_rows, n_cols, bit0=0, row_stride_bits=None, row_bit=None, samp_index=None, snp_index=None, out=None,
                device=0, n_bytes=None, mem=None, out_mem=None, stream=None):
    """snpgpu_geno_select: the selected rectangle of a 2-bit genotype stream as PACKED2 rows uint8 [n_snp_out][ceil(n_samp_out / 4)].
    src: a numpy uint8 array (its bytes, host memory) or an address (int) with n_bytes -- device memory unless mem says HOST or
    HOST_PINNED.  major 0: the n_rows rows are SNPs and the n_cols columns samples; major 1: the rows are samples.  Element (r, c)
    lies at bit bit0 + r * row_stride_bits + 2 c (row_stride_bits None: 2 * n_cols, the continuous stream of a GDS node; byte-aligned
    PACKED2 rows have 8 * ceil(n_cols / 4)), or at bit0 + row_bit[r] + 2 c with row_bit (int64 per row).  samp_index / snp_index:
    0-based positions in the source, None = all in order.  out: None = a new host array (returned), a numpy uint8 array of the
    result's size, or an address (device memory unless out_mem says otherwise); returned as given."""
    return _geno_convert(lib().snpgpu_geno_select, src, major, n_rows, n_cols, bit0, row_stride_bits, row_bit, samp_index, snp_index, out,
                         device, n_bytes, mem, out_mem, stream)


def geno_convert(src, major, n_rows, n_cols, src_code=CODE_GDS, dst_code=CODE_GDS, dst_major=0, bit0=0, row_stride_bits=None,
                 row_bit=None, samp_index=None, snp_index=None, out=None, device=0, n_bytes=None, mem=None, out_mem=None, stream=None):
    """snpgpu_geno_convert: geno_select with a code set on either side (CODE_GDS: 0 / 1 / 2 A alleles, 3 missing, padding 3;
    CODE_BED: PLINK's 0 / 1 missing / 2 / 3, padding 0) and the layout of the result: dst_major 0 gives SNP rows uint8
    [n_snp_out][ceil(n_samp_out / 4)] (.bed mode 1), dst_major 1 sample rows uint8 [n_samp_out][ceil(n_snp_out / 4)] (.bed mode 0).
    Every other argument as geno_select."""
    L = lib()

    def call(d, samp, n_samp_out, snp, n_snp_out, optr, out_mem, device, stream):
        return L.snpgpu_geno_convert(d, int(src_code), samp, n_samp_out, snp, n_snp_out, optr, int(dst_major), int(dst_code), out_mem,
                                     device, stream)
    return _geno_convert(call, src, major, n_rows, n_cols, bit0, row_stride_bits, row_bit, samp_index, snp_index, out, device, n_bytes,
                         mem, out_mem, stream, dst_major=1 if dst_major == 1 else 0)


def geno_select_stats():
    """dict of snpgpu_geno_select_stats for the last geno_select call on this thread"""
    s = _stats("geno_select", 8)
    return dict(h2d_ms=float(s[0]), copy_ms=float(s[1]), gather_ms=float(s[2]), transpose_ms=float(s[3]), launches=int(s[4]),
                source_bytes=float(s[5]), d2h_ms=float(s[6]), windows=int(s[7]))


def geno_convert_stats():
    """dict of snpgpu_geno_convert_stats for the last geno_convert (or geno_select) call on this thread: the fields of
    geno_select_stats"""
    s = _stats("geno_convert", 8)
    return dict(h2d_ms=float(s[0]), copy_ms=float(s[1]), gather_ms=float(s[2]), transpose_ms=float(s[3]), launches=int(s[4]),
                source_bytes=float(s[5]), d2h_ms=float(s[6]), windows=int(s[7]))


def vcf_index(buf, n_bytes=None, final=True, line_base=0, max_lines=None):
    """snpgpu_vcf_index: (col_begin int64 [n_lines][10], line_end int64 [n_lines], consumed) of the data lines in buf (bytes, or a
    numpy uint8 array of which the first n_bytes count).  Without `final` a cut last line is left: consumed is where it starts.
    max_lines None: as many as the buffer has line ends."""
    a = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf)
    if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError("buf should be bytes or a contiguous uint8 array")
    n_bytes = a.size if n_bytes is None else int(n_bytes)
    if n_bytes > a.size:
        raise ValueError("n_bytes exceeds the buffer")
    if max_lines is None:
        max_lines = int(np.count_nonzero(a[:n_bytes] == 10)) + 1
    max_lines = int(max_lines)
    col = np.empty((max(max_lines, 1), 10), np.int64)
    end = np.empty(max(max_lines, 1), np.int64)
    n, used = ctypes.c_int64(0), ctypes.c_int64(0)
    keep = a if a.size else np.zeros(1, np.uint8)
    check(lib().snpgpu_vcf_index(_ptr(keep), n_bytes, int(bool(final)), int(line_base), max_lines, _ptr(col), _ptr(end), ctypes.byref(n),
                                 ctypes.byref(used)))
    return col[:n.value], end[:n.value], used.value


def vcf_genotypes(text, cell_begin, line_end, num_allele, ref_index, n_samp, rows, n_bytes=None, text_mem=None, device=0, stream=None):
    """snpgpu_vcf_genotypes: the sample cells of the lines text[cell_begin[i], line_end[i]) as PACKED2 rows in DEVICE memory at the
    address `rows` ([n_lines][ceil(n_samp / 4)]).  text: bytes / a numpy uint8 array (host memory), or an address (int) with n_bytes
    -- device memory unless text_mem says HOST or HOST_PINNED.  Returns (line_flags int32, line_cells int64)."""
    ptr, mem, n_bytes, _keep = _text_input(text, n_bytes, text_mem)
    cb, le = np.ascontiguousarray(cell_begin, np.int64).reshape(-1), np.ascontiguousarray(line_end, np.int64).reshape(-1)
    na, ri = np.ascontiguousarray(num_allele, np.int32).reshape(-1), np.ascontiguousarray(ref_index, np.int32).reshape(-1)
    n = cb.size
    if not (le.size == n and na.size == n and ri.size == n):
        raise ValueError("cell_begin, line_end, num_allele and ref_index should have one entry per line")
    flags, cells = np.zeros(n, np.int32), np.zeros(n, np.int64)
    check(lib().snpgpu_vcf_genotypes(ptr, mem, n_bytes, _ptr(cb), _ptr(le), _ptr(na), _ptr(ri), n, int(n_samp), _dptr(rows),
                                     _ptr(flags), _ptr(cells), int(device), ctypes.c_void_p(stream) if stream else None))
    return flags, cells


def vcf_stats():
    """dict of snpgpu_vcf_stats for the last vcf_genotypes call on this thread"""
    s = _stats("vcf", 7)
    return dict(h2d_ms=float(s[0]), kernel_ms=float(s[1]), launches=int(s[2]), text_bytes=float(s[3]), chunk_bytes=int(s[4]),
                segment_bytes=int(s[5]), halo_bytes=int(s[6]))


def _pool(pieces):
    """(pool uint8, offsets int64) of a list of bytes / str pieces"""
    pieces = [x if isinstance(x, (bytes, bytearray)) else str(x).encode("latin1") for x in pieces]
    off = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([len(x) for x in pieces], out=off[1:])
    pool = np.frombuffer(b"".join(pieces) + b"\0", np.uint8)
    return pool, off


def text_render(rows, n_rows, n_cols, fmt, alleles=None, prefixes=None, text=None, device=0, stream=None):
    """snpgpu_text_render: the n_rows x n_cols codes at the DEVICE address `rows` (PACKED2, [n_rows][ceil(n_cols / 4)]) as lines of
    text at the DEVICE address `text`; text None only sizes.  fmt: TEXT_DIGIT / TEXT_PED_AB / TEXT_PED_12 / TEXT_PED_ALLELE.
    alleles: for TEXT_PED_ALLELE the 2 n_cols pieces s1, s2 per column (bytes or str), or a ready (pool, offsets) pair;
    prefixes: None, n_rows pieces, or a (pool, offsets) pair.  Returns line_off int64 [n_rows + 1]."""
    def pair(x, n):
        if x is None:
            return None, None
        if isinstance(x, tuple) and len(x) == 2 and isinstance(x[1], np.ndarray):
            pool, off = np.ascontiguousarray(x[0], np.uint8), np.ascontiguousarray(x[1], np.int64)
        else:
            pool, off = _pool(x)
        if off.shape != (n + 1,):
            raise ValueError("%d pieces expected" % n)
        if len(off) and off[-1] > pool.size:
            raise ValueError("the offsets exceed the pool")
        return pool, off
    n_rows, n_cols = int(n_rows), int(n_cols)
    apool, aoff = pair(alleles, 2 * n_cols)
    ppool, poff = pair(prefixes, n_rows)
    line_off = np.zeros(max(n_rows, 0) + 1, np.int64)
    check(lib().snpgpu_text_render(_dptr(rows), n_rows, n_cols, int(fmt), _ptr(apool), _ptr(aoff), _ptr(ppool), _ptr(poff),
                                   _dptr(text) if text else None, _ptr(line_off), int(device),
                                   ctypes.c_void_p(stream) if stream else None))
    return line_off


def text_stats():
    """dict of snpgpu_text_stats for the last text_render call on this thread"""
    s = _stats("text", 6)
    return dict(lengths_ms=float(s[0]), write_ms=float(s[1]), launches=int(s[2]), text_bytes=float(s[3]), segment_bytes=int(s[4]),
                tile_columns=int(s[5]))


PED_FLAG_TOKEN, PED_FLAG_EMPTY, PED_FLAG_COUNT = 1, 2, 8
PED_ALLELES = 94


def ped_tokens(text, n_bytes, cell_begin, line_end, n_snp, tokens, device=0, stream=None):
    """snpgpu_ped_tokens: the allele tokens of the lines text[cell_begin[i], line_end[i]) (text: a DEVICE address) into the token
    matrix uint8 [n_lines][2 n_snp] at the DEVICE address `tokens`.  Returns (line_flags int32, line_tokens int64)."""
    cb, le = np.ascontiguousarray(cell_begin, np.int64).reshape(-1), np.ascontiguousarray(line_end, np.int64).reshape(-1)
    if cb.size != le.size:
        raise ValueError("cell_begin and line_end should have one entry per line")
    flags, count = np.zeros(cb.size, np.int32), np.zeros(cb.size, np.int64)
    check(lib().snpgpu_ped_tokens(_dptr(text), int(n_bytes), _ptr(cb), _ptr(le), cb.size, int(n_snp), _dptr(tokens), _ptr(flags),
                                  _ptr(count), int(device), ctypes.c_void_p(stream) if stream else None))
    return flags, count


def ped_census(tokens, line_flags, n_snp, table, device=0, stream=None):
    """snpgpu_ped_census: the tokens of the unflagged lines of the token matrix (DEVICE address) added to the DEVICE table uint32
    [n_snp][94]"""
    fl = np.ascontiguousarray(line_flags, np.int32).reshape(-1)
    check(lib().snpgpu_ped_census(_dptr(tokens), _ptr(fl), fl.size, int(n_snp), _dptr(table), int(device),
                                  ctypes.c_void_p(stream) if stream else None))


def ped_codes(tokens, n_lines, n_snp, ref, rows, device=0, stream=None):
    """snpgpu_ped_codes: the token matrix (DEVICE address) against the reference allele bytes ref (uint8 [n_snp], 0 = none) as PACKED2
    sample rows at the DEVICE address `rows`"""
    r = np.ascontiguousarray(ref, np.uint8).reshape(-1)
    if r.size != int(n_snp):
        raise ValueError("ref should hold one byte per SNP")
    check(lib().snpgpu_ped_codes(_dptr(tokens), int(n_lines), int(n_snp), _ptr(r), _dptr(rows), int(device),
                                 ctypes.c_void_p(stream) if stream else None))


def ped_stats():
    """dict of snpgpu_ped_stats on this thread"""
    s = _stats("ped", 8)
    return dict(tokens_ms=float(s[0]), census_ms=float(s[1]), codes_ms=float(s[2]), launches=int(s[3]), text_bytes=float(s[4]),
                chunk_bytes=int(s[5]), segment_bytes=int(s[6]), halo_bytes=int(s[7]))


GEN_FLAG_BYTE, GEN_FLAG_DOT, GEN_FLAG_DIGITS, GEN_FLAG_LONG, GEN_FLAG_EMPTY, GEN_FLAG_COUNT = 1, 2, 4, 8, 16, 32


def gen_genotypes(text, cell_begin, line_end, n_samp, call_threshold, rows, n_bytes=None, text_mem=None, device=0, stream=None):
    """snpgpu_gen_genotypes: the probability triples of the lines text[cell_begin[i], line_end[i]) called to PACKED2 rows in DEVICE
    memory at the address `rows` ([n_lines][ceil(n_samp / 4)], padding codes 0).  text: bytes / a numpy uint8 array (host memory),
    or an address (int) with n_bytes -- device memory unless text_mem says HOST or HOST_PINNED.  Returns (line_flags int32,
    line_cells int64)."""
    ptr, mem, n_bytes, _keep = _text_input(text, n_bytes, text_mem)
    cb, le = np.ascontiguousarray(cell_begin, np.int64).reshape(-1), np.ascontiguousarray(line_end, np.int64).reshape(-1)
    n = cb.size
    if le.size != n:
        raise ValueError("cell_begin and line_end should have one entry per line")
    flags, cells = np.zeros(n, np.int32), np.zeros(n, np.int64)
    check(lib().snpgpu_gen_genotypes(ptr, mem, n_bytes, _ptr(cb), _ptr(le), n, int(n_samp), float(call_threshold), _dptr(rows),
                                     _ptr(flags), _ptr(cells), int(device), ctypes.c_void_p(stream) if stream else None))
    return flags, cells


def gen_line_host(line, n_samp, call_threshold):
    """snpgpu_gen_line_host: the 3 n_samp cells of one line (bytes from its sixth column on, without the line end) as the reference
    reads them.  Returns (codes uint8 [n_samp], 0, "") or (None, column, message): the 1-based cell counted from `line` at which
    the reference raises `message`.  No device is needed."""
    line = bytes(line)
    codes = np.zeros(max(int(n_samp), 1), np.uint8)
    col = ctypes.c_int64(0)
    msg = ctypes.create_string_buffer(256)
    check(lib().snpgpu_gen_line_host(line, len(line), int(n_samp), float(call_threshold), _ptr(codes), ctypes.byref(col), msg, len(msg)))
    if col.value:
        return None, col.value, msg.value.decode("latin1")
    return codes, 0, ""


def gen_stats():
    """dict of snpgpu_gen_stats for the last gen_genotypes call on this thread"""
    s = _stats("gen", 7)
    return dict(h2d_ms=float(s[0]), kernel_ms=float(s[1]), launches=int(s[2]), text_bytes=float(s[3]), chunk_bytes=int(s[4]),
                segment_bytes=int(s[5]), halo_bytes=int(s[6]))


def merge_part(src, major, n_rows, n_cols, bit0=0, row_stride_bits=None, row_bit=None, samp_index=None, snp_index=None, flip=None,
               n_bytes=None, mem=None):
    """One part of geno_merge: a source described as for geno_select (src: a numpy uint8 array in host memory, or an address with
    n_bytes -- device memory unless mem says HOST or HOST_PINNED), the samples it contributes (samp_index, None = all in order), the
    source SNP of every output row (snp_index, None = in order) and flip (None, or one entry per output row: non-zero re-codes that
    row 0 / 1 / 2 / 3 -> 2 / 1 / 0 / 3)."""
    return dict(src=src, major=major, n_rows=n_rows, n_cols=n_cols, bit0=bit0, row_stride_bits=row_stride_bits, row_bit=row_bit,
                samp_index=samp_index, snp_index=snp_index, flip=flip, n_bytes=n_bytes, mem=mem)


def geno_merge(parts, rows, n_snp_out=None, device=0, stream=None):
    """snpgpu_geno_merge: the parts (merge_part(...) each) side by side as PACKED2 rows [n_snp_out][ceil(N / 4)] in DEVICE memory at
    the address `rows`, N = the samples of all parts, part i from code n_0 + ... + n_(i-1) on.  n_snp_out None: the length of the
    first part's snp_index, else its number of SNPs.  Returns (n_snp_out, N)."""
    keep, arr = [], (MergePart * max(len(parts), 1))()
    N = 0
    for i, p in enumerate(parts):
        src, major, n_rows, n_cols = p["src"], int(p["major"]), int(p["n_rows"]), int(p["n_cols"])
        if isinstance(src, int):
            if p.get("n_bytes") is None:
                raise ValueError("a source address needs n_bytes")
            ptr, mem, n_bytes = src, (DEVICE if p.get("mem") is None else int(p["mem"])), int(p["n_bytes"])
        else:
            a = np.ascontiguousarray(src, dtype=np.uint8)
            keep.append(a)
            ptr, mem = a.ctypes.data, (HOST if p.get("mem") is None else int(p["mem"]))
            n_bytes = a.size if p.get("n_bytes") is None else int(p["n_bytes"])
            if n_bytes > a.size:
                raise ValueError("n_bytes exceeds the source array")

        def host(x, dtype):
            if x is None:
                return None, None
            x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
            keep.append(x)
            return x, x.ctypes.data
        rbit, rbit_p = host(p.get("row_bit"), np.int64)
        if rbit is not None and rbit.shape != (n_rows,):
            raise ValueError("row_bit should hold one bit position per source row")
        samp, samp_p = host(p.get("samp_index"), np.int32)
        snp, snp_p = host(p.get("snp_index"), np.int32)
        n_samp = (n_rows if major else n_cols) if samp is None else samp.size
        n_snp = (n_cols if major else n_rows) if snp is None else snp.size
        if n_snp_out is None:
            n_snp_out = n_snp
        flip = p.get("flip")
        flip, flip_p = host(None if flip is None else (np.asarray(flip) != 0), np.uint8)
        if (snp is not None and snp.size != int(n_snp_out)) or (flip is not None and flip.size != int(n_snp_out)):
            raise ValueError("snp_index and flip should hold one entry per output row")
        stride = p.get("row_stride_bits")
        arr[i] = MergePart(GenoSrc(ptr, mem, major, n_rows, n_cols, int(p.get("bit0") or 0), 2 * n_cols if stride is None else int(stride),
                                   rbit_p, n_bytes), snp_p, samp_p, n_samp, flip_p)
        N += n_samp
    n_snp_out = 0 if n_snp_out is None else int(n_snp_out)
    check(lib().snpgpu_geno_merge(arr, len(parts), n_snp_out, _dptr(rows), int(device),
                                  ctypes.c_void_p(stream) if stream else None))
    return n_snp_out, N


def geno_merge_stats():
    """dict of snpgpu_geno_merge_stats for the last geno_merge call on this thread"""
    s = _stats("geno_merge", 5)
    return dict(stage_ms=float(s[0]), splice_ms=float(s[1]), launches=int(s[2]), windows=int(s[3]), bytes_written=float(s[4]))


def grm_merge(grms, weight, cmd=":method = GCTA", avg_val=None, device=0):
    """snpgpu_gnrGRMMerge: (merged N x N matrix, avg_val or None) of the N x N float64 matrices `grms`; cmd: the second element of
    the files' "command" node, ":method = IndivBeta" selects the beta merge, which needs the avg_val of every input"""
    mats = [np.ascontiguousarray(g, np.float64) for g in grms]
    n = mats[0].shape[0]
    if any(m.shape != (n, n) for m in mats):
        raise ValueError("every GRM should be N x N")
    w = np.ascontiguousarray(weight, np.float64)
    if w.shape != (len(mats),):
        raise ValueError("one weight per GRM")
    beta = cmd == ":method = IndivBeta"
    avg_in = np.ascontiguousarray(avg_val, np.float64) if beta else None
    if beta and avg_in.shape != (len(mats),):
        raise ValueError("one avg_val per GRM")
    ptrs = (ctypes.c_void_p * len(mats))(*[m.ctypes.data for m in mats])
    out = np.empty((n, n), np.float64)
    check(lib().snpgpu_gnrGRMMerge(len(mats), n, ptrs, cmd.encode(), _ptr(avg_in), _ptr(w), _ptr(out), int(device)))
    if not beta:
        return out, None
    avg = ctypes.c_double(0)
    check(lib().snpgpu_gnrGRM_avg_val(ctypes.byref(avg)))
    return out, avg.value


def grm_merge_stats():
    """dict of snpgpu_grm_merge_stats for the last grm_merge (api.snpgdsMergeGRM) on this thread"""
    s = _stats("grm_merge", 2)
    return dict(slabs=int(s[0]), launches=int(s[1]))


def select_grm_stats():
    """ms of the last select_grm call on this thread: count pass, scan, write pass, diagonal kernel (device) and the whole call (host clock)"""
    v = np.zeros(5, np.float64)
    check(lib().snpgpu_select_grm_stats(_ptr(v)))
    return dict(count_ms=v[0], scan_ms=v[1], write_ms=v[2], diag_ms=v[3], call_ms=v[4])


def select_stats():
    """ms of the last select_pairs call on this thread: count pass, scan, write pass (device) and the whole call (host clock)"""
    s = _stats("select", 4)
    return dict(count_ms=s[0], scan_ms=s[1], write_ms=s[2], call_ms=s[3])


def pair_stats():
    """dict of snpgpu_pair_stats for the last pair_tables / pair_score_matrix call on this thread"""
    s = _stats("pair", 8)
    return dict(snp_table_ms=float(s[0]), snp_table_launches=int(s[1]), snp_table_bytes=float(s[2]), words_ms=float(s[3]),
                pair_count_ms=float(s[4]), matrix_ms=float(s[5]), other_launches=int(s[6]), other_bytes=float(s[7]))


def _mds_matrix(dist, n, ld, device):
    """(pointer, n, ld, mem, device, keep-alive) of a distance matrix: a square float64 numpy array (host memory; a view of a wider
    array keeps its leading dimension), a device address (int) with n, or a torch tensor on a GPU, used where it lies"""
    if isinstance(dist, int):
        if n is None:
            raise ValueError("a device matrix needs n")
        return ctypes.c_void_p(dist), int(n), int(n if ld is None else ld), DEVICE, int(device), None
    if not isinstance(dist, np.ndarray) and hasattr(dist, "data_ptr") and hasattr(dist, "is_cuda"):
        import torch
        if not dist.is_cuda or dist.dtype != torch.float64 or dist.dim() != 2 or dist.shape[0] != dist.shape[1]:
            raise ValueError("dist should be a square float64 matrix (a torch tensor: on a GPU)")
        if dist.stride(1) != 1 and dist.shape[1] > 1:
            dist = dist.contiguous()
        torch.cuda.current_stream(dist.device).synchronize()      # the library's stream waits for no other: the matrix is complete
        return (ctypes.c_void_p(dist.data_ptr()), int(dist.shape[0]), int(max(dist.stride(0), dist.shape[1])), DEVICE,
                int(dist.device.index or 0), dist)
    d = np.asarray(dist)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("dist should be a square matrix")
    if d.dtype != np.float64 or d.strides[1] != 8 or d.strides[0] % 8 or d.strides[0] < 8 * d.shape[1]:
        d = np.ascontiguousarray(d, np.float64)
    return _ptr(d), int(d.shape[0]), int(d.strides[0] // 8), HOST, int(device), d


def _mds_result(n, k, call):
    eigval, vectors, all_eigval = np.zeros(k, np.float64), np.zeros((k, n), np.float64), np.zeros(n, np.float64)
    trace, route = ctypes.c_double(0), ctypes.c_int(-1)
    check(call(_ptr(eigval), _ptr(vectors), _ptr(all_eigval), ctypes.byref(trace), ctypes.byref(route)))
    return dict(eigval=eigval, vectors=vectors, all_eigval=all_eigval if route.value == 0 else None, trace=trace.value,
                route=route.value, pos_tol=mds_stats()["pos_tol"])


def mds(dist, k, device=0, n=None, ld=None):
    """snpgpu_mds: dict(eigval [k], vectors [k][n], all_eigval [n] or None (Krylov route), trace, route, pos_tol) of the classical
    scaling of a distance matrix.  dist: a square float64 numpy array, a device address (int) with n (and ld), or a torch tensor on
    a GPU, used where it lies (then its device is the call's)."""
    ptr, n, ld, mem, device, _keep = _mds_matrix(dist, n, ld, device)
    k = int(k)
    if n < 2:
        raise ValueError("'d' must have at least two rows")
    if k < 1 or k > n - 1:
        raise ValueError("'k' must be in {1, 2, ..  n - 1}")
    return _mds_result(n, k, lambda w, v, a, t, r: lib().snpgpu_mds(ptr, n, ld, mem, k, w, v, a, t, r, device))


def gnr_mds(what, k, n_samp):
    """snpgpu_gnrMDS on the working space of n_samp samples: what = 0 (1 - IBS) or 1 (dissimilarity); the dict of mds()"""
    n_samp, k = int(n_samp), int(k)
    if k < 1 or k > n_samp - 1:
        raise ValueError("'k' must be in {1, 2, ..  n - 1}")
    return _mds_result(n_samp, k, lambda w, v, a, t, r: lib().snpgpu_gnrMDS(int(what), k, w, v, a, t, r))


def mds_apply(dist, Q, device=0, n=None, ld=None):
    """snpgpu_mds_apply: Y = B Q for Q [b][n] (host), B = -1/2 J (D o D) J of the distance matrix (as mds() takes it)"""
    ptr, n, ld, mem, device, _keep = _mds_matrix(dist, n, ld, device)
    q = np.ascontiguousarray(Q, np.float64)
    if q.ndim != 2 or q.shape[1] != n or q.shape[0] < 1:
        raise ValueError("Q should be [b][n]")
    y = np.zeros_like(q)
    check(lib().snpgpu_mds_apply(ptr, n, ld, mem, _ptr(q), int(q.shape[0]), _ptr(y), device))
    return y


def mds_stats():
    """dict of snpgpu_mds_stats for the last mds / mds_apply / gnr_mds on this thread"""
    s = _stats("mds", 9)
    return dict(stage_ms=float(s[0]), scan_ms=float(s[1]), eigen_ms=float(s[2]), total_ms=float(s[3]), route=int(s[4]),
                products=int(s[5]), product_ms=float(s[6]), windows=int(s[7]), pos_tol=float(s[8]))


def _pcr_inputs(pcs, training, n_samp):
    """(pcs as float64 [n][n_pc] or None, n_pc, training as uint8 [n] or None) of the PC-Relate calls"""
    n_samp = int(n_samp)
    p = None if pcs is None else np.ascontiguousarray(pcs, np.float64)
    if p is not None and p.ndim == 1:
        p = p.reshape(n_samp, -1) if p.size else None
    if p is not None and (p.ndim != 2 or p.shape[0] != n_samp):
        raise ValueError("'pcs' should have one row per sample")
    t = None
    if training is not None:
        t = np.ascontiguousarray(np.asarray(training) != 0, np.uint8)
        if t.shape != (n_samp,):
            raise ValueError("'training' should have one flag per sample")
    return p, (0 if p is None else int(p.shape[1])), t


class PCRelate:
    """One streaming PC-Relate object (snpgpu_pcr, include/snpgpu.h section 1r): feed SNP blocks, then result() / sums()."""

    def __init__(self, n_samp, pcs=None, training=None, maf_thresh=0.01, ibd=True, device=0, stream=None):
        self.n = int(n_samp)
        p, self.n_pc, t = _pcr_inputs(pcs, training, self.n)
        self.ibd = bool(ibd)
        o = Opts(int(device), 0, 0, 0, 0, ctypes.c_void_p(stream) if stream else None)
        h = ctypes.c_void_p()
        self._h = None
        check(lib().snpgpu_pcr_create(self.n, self.n_pc, _ptr(p), _ptr(t), float(maf_thresh), PCR_IBD if self.ibd else 0, ctypes.byref(o),
                                      ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().snpgpu_pcr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def feed(self, geno, fmt=None, n_snp=None, want_beta=False):
        """geno: numpy uint8 rows (U8 or PACKED2) or a device address (int, with n_snp; PACKED2 unless fmt says U8).  want_beta: the
        regression coefficients [n_snp][n_pc + 1] of these SNPs are returned."""
        ptr, m, fmt, mem, _keep = _geno_input(geno, self.n, fmt, n_snp, device_fmt_default=GENO_PACKED2)
        beta = np.empty((m, self.n_pc + 1), np.float64) if want_beta else None
        check(lib().snpgpu_pcr_feed(self._h, ptr, m, fmt, mem, _ptr(beta)))
        return beta

    def result(self, probs=None):
        """dict(kinship, inbreed, nsnp and -- probs, by default where the object accumulates them -- k0, k2)"""
        probs = self.ibd if probs is None else bool(probs)
        n = self.n
        r = dict(kinship=np.empty((n, n), np.float64), inbreed=np.empty(n, np.float64), nsnp=np.empty((n, n), np.float64))
        if probs:
            r.update(k0=np.empty((n, n), np.float64), k2=np.empty((n, n), np.float64))
        check(lib().snpgpu_pcr_result(self._h, _ptr(r["kinship"]), _ptr(r["inbreed"]), _ptr(r.get("k0")), _ptr(r.get("k2")), _ptr(r["nsnp"])))
        return r

    def sums(self, which):
        """one accumulated plane (a name of PCR_PLANES or its index) as a full n x n matrix"""
        w = PCR_PLANES.index(which) if isinstance(which, str) else int(which)
        out = np.empty((self.n, self.n), np.float64)
        check(lib().snpgpu_pcr_sums(self._h, w, _ptr(out)))
        return out

    def stats(self):
        s = np.zeros(8, np.float64)
        check(lib().snpgpu_pcr_stats(self._h, _ptr(s)))
        return dict(blocks=int(s[0]), product_launches=int(s[1]), beta_ms=s[2], operand_ms=s[3], product_ms=s[4], final_ms=s[5],
                    plane_bytes=int(s[6]), block_snps=int(s[7]))

    def panel_stats(self):
        """snpgpu_pcr_panel_stats: ms of the CD job and of the strips of diagonal tiles (both inside stats()["product_ms"])"""
        s = np.zeros(2, np.float64)
        check(lib().snpgpu_pcr_panel_stats(self._h, _ptr(s)))
        return dict(cd_ms=float(s[0]), strip_ms=float(s[1]))

    def panel_result(self, probs=None):
        """result() through snpgpu_pcr_panel_result, which takes a full object as the panel [0, n)"""
        return _pcr_panel_result(self._h, (self.n, self.n), self.n, self.ibd if probs is None else bool(probs))

    def panel_sums(self, which):
        """sums() through snpgpu_pcr_panel_sums (a name of PCR_SLABS or its index; "CD": DC transposed)"""
        return _pcr_panel_sums(self._h, (self.n, self.n), which)

    def select(self, cutoff, samp_sel=None, capacity=None, probs=None):
        """snpgpu_pcr_select: the related pairs of this object's rows, selected on the device.  dict(idx1, idx2, kinship, nsnp, inbreed,
        n_found and -- probs, by default where the object accumulates them -- k0, k2).  capacity=None: a count, then all pairs; a
        number: at most so many pairs are stored (0: count only, the pair arrays are empty)."""
        probs = self.ibd if probs is None else bool(probs)
        mask = None
        if samp_sel is not None:
            mask = np.ascontiguousarray(np.asarray(samp_sel) != 0, np.uint8)
            if mask.shape != (self.n,):
                raise ValueError("'samp_sel' should have one flag per sample")
        o = PcrSelOpts(float(cutoff), None if mask is None else mask.ctypes.data)
        found = ctypes.c_int64(0)
        inb = np.empty(self.n, np.float64)
        if capacity is None:
            check(lib().snpgpu_pcr_select(self._h, ctypes.byref(o), 0, None, None, None, None, None, None, None, ctypes.byref(found)))
            capacity = found.value
        m = int(capacity)
        r = dict(idx1=np.empty(m, np.int32), idx2=np.empty(m, np.int32), kinship=np.empty(m, np.float64), nsnp=np.empty(m, np.float64))
        if probs:
            r.update(k0=np.empty(m, np.float64), k2=np.empty(m, np.float64))
        out = [_ptr(r[k]) if m > 0 and k in r else None for k in ("idx1", "idx2", "kinship", "k0", "k2", "nsnp")]
        check(lib().snpgpu_pcr_select(self._h, ctypes.byref(o), m, *out, _ptr(inb), ctypes.byref(found)))
        k = min(m, found.value)
        for name in list(r):
            r[name] = r[name][:k]
        r.update(inbreed=inb, n_found=int(found.value))
        return r


def pcr_select_stats():
    """dict of snpgpu_pcr_select_stats for the last select on this thread"""
    s = np.zeros(4, np.float64)
    check(lib().snpgpu_pcr_select_stats(_ptr(s)))
    return dict(count_ms=float(s[0]), scan_ms=float(s[1]), write_ms=float(s[2]), total_ms=float(s[3]))


class PCRelatePanel(PCRelate):
    """A PC-Relate object that holds the row panel rows = (r0, r1) x columns [r0, n) (snpgpu_pcr_create_panel): feed as a PCRelate;
    result() / sums() give [r1 - r0][n - r0] arrays equal to the full object's [r0:r1, r0:] (inbreed: all n samples)."""

    def __init__(self, n_samp, rows, pcs=None, training=None, maf_thresh=0.01, ibd=True, device=0, stream=None):
        self.n = int(n_samp)
        self.rows = (int(rows[0]), int(rows[1]))
        p, self.n_pc, t = _pcr_inputs(pcs, training, self.n)
        self.ibd = bool(ibd)
        o = Opts(int(device), 0, 0, 0, 0, ctypes.c_void_p(stream) if stream else None)
        h = ctypes.c_void_p()
        self._h = None
        check(lib().snpgpu_pcr_create_panel(self.n, self.n_pc, _ptr(p), _ptr(t), float(maf_thresh), PCR_IBD if self.ibd else 0,
                                            self.rows[0], self.rows[1], ctypes.byref(o), ctypes.byref(h)))
        self._h = h

    @property
    def shape(self):
        return (self.rows[1] - self.rows[0], self.n - self.rows[0])

    def result(self, probs=None):
        return _pcr_panel_result(self._h, self.shape, self.n, self.ibd if probs is None else bool(probs))

    def sums(self, which):
        """one accumulated slab (a name of PCR_SLABS or its index) as [r1 - r0][n - r0]"""
        return _pcr_panel_sums(self._h, self.shape, which)

    panel_result, panel_sums = result, sums         # (the base class's would shape them n x n)


def _pcr_panel_result(h, shape, n, probs):
    r = dict(kinship=np.empty(shape, np.float64), inbreed=np.empty(n, np.float64), nsnp=np.empty(shape, np.float64))
    if probs:
        r.update(k0=np.empty(shape, np.float64), k2=np.empty(shape, np.float64))
    check(lib().snpgpu_pcr_panel_result(h, _ptr(r["kinship"]), _ptr(r["inbreed"]), _ptr(r.get("k0")), _ptr(r.get("k2")), _ptr(r["nsnp"])))
    return r


def _pcr_panel_sums(h, shape, which):
    w = PCR_SLABS.index(which) if isinstance(which, str) else int(which)
    out = np.empty(shape, np.float64)
    check(lib().snpgpu_pcr_panel_sums(h, w, _ptr(out)))
    return out


def gnr_pcrelate_pairs(n_samp, pcs=None, training=None, maf_thresh=0.01, ibd=True, panel_rows=0, kinship_cutoff=float("nan"),
                       samp_sel=None, verbose=False):
    """snpgpu_gnrPCRelatePairs on the working space of n_samp samples: dict(idx1, idx2, kinship, nsnp, inbreed, n_panels and, with
    ibd, k0, k2); panel_rows 0: as many rows per panel as the device holds"""
    n = int(n_samp)
    p, n_pc, t = _pcr_inputs(pcs, training, n)
    mask = None
    if samp_sel is not None:
        mask = np.ascontiguousarray(np.asarray(samp_sel) != 0, np.uint8)
        if mask.shape != (n,):
            raise ValueError("'samp_sel' should have one flag per sample")
    found, panels = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().snpgpu_gnrPCRelatePairs(n_pc, _ptr(p), _ptr(t), float(maf_thresh), PCR_IBD if ibd else 0, int(panel_rows), float(kinship_cutoff),
                                        _ptr(mask), int(bool(verbose)), ctypes.byref(found), ctypes.byref(panels)))
    m = found.value
    r = dict(idx1=np.empty(m, np.int32), idx2=np.empty(m, np.int32), kinship=np.empty(m, np.float64), nsnp=np.empty(m, np.float64),
             inbreed=np.empty(n, np.float64))
    if ibd:
        r.update(k0=np.empty(m, np.float64), k2=np.empty(m, np.float64))
    check(lib().snpgpu_gnrPCRelatePairs_get(_ptr(r["idx1"]), _ptr(r["idx2"]), _ptr(r["kinship"]), _ptr(r.get("k0")), _ptr(r.get("k2")),
                                            _ptr(r["nsnp"]), _ptr(r["inbreed"])))
    r["n_panels"] = int(panels.value)
    return r


def gnr_pcrelate(n_samp, pcs=None, training=None, maf_thresh=0.01, ibd=True):
    """snpgpu_gnrPCRelate on the working space of n_samp samples: the dict of PCRelate.result()"""
    n = int(n_samp)
    p, n_pc, t = _pcr_inputs(pcs, training, n)
    r = dict(kinship=np.empty((n, n), np.float64), inbreed=np.empty(n, np.float64), nsnp=np.empty((n, n), np.float64))
    if ibd:
        r.update(k0=np.empty((n, n), np.float64), k2=np.empty((n, n), np.float64))
    check(lib().snpgpu_gnrPCRelate(n_pc, _ptr(p), _ptr(t), float(maf_thresh), PCR_IBD if ibd else 0, _ptr(r["kinship"]), _ptr(r["inbreed"]),
                                   _ptr(r.get("k0")), _ptr(r.get("k2")), _ptr(r["nsnp"])))
    return r


def _admix_matrix(x, rows, k, name):
    """x as float64 [rows][k] (None stays None)"""
    if x is None:
        return None
    a = np.ascontiguousarray(x, np.float64)
    if a.shape != (int(rows), int(k)):
        raise ValueError("'%s' should be a %d x %d matrix" % (name, rows, k))
    return a


class Admix:
    """One EM object for ancestry proportions (snpgpu_admix, include/snpgpu.h section 1s): feed SNP rows, set(q, f), run(), get().
    Creation makes no HIP call; the first feed or set opens the device."""

    def __init__(self, n_samp, n_pop, max_snps, f_min=1e-6, block_snps=0, device=0, stream=None):
        self.n, self.k, self.max_snps = int(n_samp), int(n_pop), int(max_snps)
        self.m = 0                  # rows fed
        self.f_rows = 0             # rows F was set for
        o = Opts(int(device), 0, 0, 0, 0, ctypes.c_void_p(stream) if stream else None)
        h = ctypes.c_void_p()
        self._h = None
        check(lib().snpgpu_admix_create(self.n, self.k, self.max_snps, float(f_min), int(block_snps), ctypes.byref(o), ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().snpgpu_admix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def feed(self, geno, fmt=None, n_snp=None):
        """geno: numpy uint8 rows (U8 or PACKED2) or a device address (int, with n_snp; PACKED2 unless fmt says U8)"""
        ptr, m, fmt, mem, _keep = _geno_input(geno, self.n, fmt, n_snp, device_fmt_default=GENO_PACKED2)
        check(lib().snpgpu_admix_feed(self._h, ptr, m, fmt, mem))
        self.m += m

    def set(self, q=None, f=None):
        """q [n][K] (rows normalised on entry), f [rows fed][K] (clamped on entry); None keeps what is there"""
        q = _admix_matrix(q, self.n, self.k, "q")
        f = _admix_matrix(f, self.m, self.k, "f")
        check(lib().snpgpu_admix_set(self._h, _ptr(q), _ptr(f)))
        if f is not None:
            self.f_rows = self.m

    def run(self, max_iter, tol=1e-4, fix_f=False):
        """(loglik [n_done + 1], n_done): loglik[t] belongs to the state before iteration t, the last entry to the state get() returns"""
        if int(max_iter) < 0:
            raise ValueError("'max_iter' should be non-negative")
        ll = np.full(int(max_iter) + 1, np.nan, np.float64)
        done = ctypes.c_int(0)
        check(lib().snpgpu_admix_run(self._h, int(max_iter), float(tol), ADMIX_FIX_F if fix_f else 0, _ptr(ll), ctypes.byref(done)))
        return ll[:done.value + 1].copy(), done.value

    def get(self):
        """(Q [n][K], F [rows F was set for][K]; F is None while it has no values)"""
        q = np.empty((self.n, self.k), np.float64)
        f = np.empty((self.f_rows, self.k), np.float64) if self.f_rows else None
        check(lib().snpgpu_admix_get(self._h, _ptr(q), _ptr(f)))
        return q, f

    def stats(self):
        s = np.zeros(6, np.float64)
        check(lib().snpgpu_admix_stats(self._h, _ptr(s)))
        return dict(blocks=int(s[0]), launches=int(s[1]), pass_ms=float(s[2]), resident_bytes=int(s[3]), block_snps=int(s[4]),
                    iterations=int(s[5]))


def gnr_admix(n_samp, n_snp, q, f, f_min=1e-6, max_iter=500, tol=1e-4, fix_f=False, block_snps=0):
    """snpgpu_gnrAdmix on the working space of n_samp samples and n_snp selected SNPs: (Q, F, loglik [n_done + 1], n_done)"""
    n, m = int(n_samp), int(n_snp)
    q = np.ascontiguousarray(q, np.float64)
    if q.ndim != 2 or q.shape[0] != n:
        raise ValueError("'q' should have one row per sample")
    k = int(q.shape[1])
    f = _admix_matrix(f, m, k, "f")
    if int(max_iter) < 0:
        raise ValueError("'max_iter' should be non-negative")
    ll = np.full(int(max_iter) + 1, np.nan, np.float64)
    done = ctypes.c_int(0)
    qo, fo = np.empty((n, k), np.float64), np.empty((m, k), np.float64)
    check(lib().snpgpu_gnrAdmix(k, float(f_min), int(block_snps), _ptr(q), _ptr(f), int(max_iter), float(tol), ADMIX_FIX_F if fix_f else 0,
                                _ptr(ll), ctypes.byref(done), _ptr(qo), _ptr(fo)))
    return qo, fo, ll[:done.value + 1].copy(), done.value
