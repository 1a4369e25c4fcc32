"""The kernel paths an accumulator context can take, as ONE table that both halves of the suite read (no HIP call at import).

csrc/ctx_plan.h decides, from environment switches read when a context is created, which pair-counter and which SYRK kernel a block
without and a block with missing calls takes.  snpgpu_diag_plan (no GPU needed) prints that decision.  This module

  * lists the switches that select a path and the values worth crossing (SWITCH_SPACE),
  * turns a plan into a `signature` -- the kind, its four kernel names, and the plan fields that change what a kernel computes
    without changing its name,
  * enumerates the signatures that are reachable at all (`reachable`),
  * and holds one hand-kept entry per reachable signature (CASES): the smallest environment that produces it, how its result is
    compared with the oracle, and the GPU test that runs it.

tests/test_cpu_kernel_paths.py holds the table against the library (a signature without a case, a case whose environment gives another
signature than its neighbours expect, a switch of ctx_plan.h that is in no table: all errors, found without a GPU);
tests/test_gpu_kernel_paths.py runs every case on the device.  The fixtures of tests/test_gpu_parity.py take their environments from
PAIR_BACKEND_ENVS / SYRK_BACKEND_ENVS below, so a fixture value that selects nothing is found here as well."""
import functools
import itertools
import os

KIND_NAMES = ("IBS", "KING_ROBUST", "KING_HOMO", "GRM_GCTA", "PCA_COV", "EIGMIX", "INDIV_BETA", "DISS")
COUNTER_KINDS = ("IBS", "KING_ROBUST", "INDIV_BETA")                 # results are integers: bit-exact
SYRK_KINDS = ("KING_HOMO", "GRM_GCTA", "PCA_COV", "EIGMIX", "DISS")  # kinds with an fp64 plane (row panels are evaluated for them)

# ---- switches that select a kernel: value None = unset (always one of the values) ----------------------------------------------------
# Presence switches (SNPGPU_I8_NO_NOMISS, SNPGPU_SYRK_MISS3) count once they are set; value switches are "not 0", so "=1" equals unset
# and only "0" is crossed; SNPGPU_SYRK_UV16 is clamped to 0 ... 3 with 3 the default.
SWITCH_SPACE = {
    "SNPGPU_PAIR_BACKEND": (None, "popcount"),
    "SNPGPU_PAIR_FP4": (None, "0"),
    "SNPGPU_PAIR_FP4_GENERAL": (None, "0"),
    "SNPGPU_GCTA_MISS_FP4": (None, "0"),
    "SNPGPU_I8_NO_NOMISS": (None, "1"),
    "SNPGPU_SYRK": (None, "f32", "h3"),
    "SNPGPU_SYRK_X1": (None, "0"),
    "SNPGPU_SYRK_MISS3": (None, "1"),
    "SNPGPU_SYRK_UV": (None, "0"),
    "SNPGPU_HOMO_UV": (None, "0"),
    "SNPGPU_SYRK_UV16": (None, "0", "1", "2"),
}

# ---- switches of Switches::from_env that change geometry, launches or numerics, never a kernel name: one hand-written GPU test each --
# name -> the test of tests/test_gpu_*.py that sets it, compares with the oracle and proves the non-default geometry from a counter
GEOMETRY_SWITCHES = {
    "SNPGPU_ACC_LAYOUT": ("test_gpu_api_golden.py", "test_panel_product_matches_dense_many_vectors"),
    "SNPGPU_EIG_BLAS": ("test_gpu_api_golden.py", "test_panel_product_matches_dense_many_vectors"),
    "SNPGPU_GCTA_SPARSE": ("test_gpu_parity.py", "test_grm_gcta_denominators_sparse_and_dense_routes"),
    "SNPGPU_GCTA_SPARSE_MAX_RATE": ("test_gpu_parity.py", "test_grm_gcta_denominators_sparse_and_dense_routes"),
    "SNPGPU_H3_SUPER": ("test_gpu_kernel_paths.py", "test_super_tile_edges"),
    "SNPGPU_X1_SUPER": ("test_gpu_kernel_paths.py", "test_super_tile_edges"),
    "SNPGPU_SYRK_FAST": ("test_gpu_kernel_paths.py", "test_one_run_one_weight_target"),
    "SNPGPU_H3_PROMOTE": ("test_gpu_parity.py", "test_grm_several_fp32_runs_per_block"),
    "SNPGPU_UV_TARGETS": ("test_gpu_parity.py", "test_grm_weight_targets_per_fp32_run"),
    "SNPGPU_X1_SPARSE": ("test_gpu_parity.py", "test_rare_variants_in_blocks_with_missing_calls"),
    "SNPGPU_X1_SHORT_RUNS": ("test_gpu_kernel_paths.py", "test_short_run_flag_of_the_exact_row_kernel"),
    "SNPGPU_X1_SPARSE_MAC": ("test_gpu_kernel_paths.py", "test_short_run_flag_of_the_exact_row_kernel"),
    "SNPGPU_UVC_PACE": ("test_gpu_parity.py", "test_converted_operand_kernel_whole_tiles_vs_oracle"),
    "SNPGPU_UVC_CARRY_ALL": ("test_gpu_carry_all.py", "test_slot_pools_reuse_and_fallback"),
    "SNPGPU_UVC_CARRY_SLOTS": ("test_gpu_carry_all.py", "_whole_tiles"),
    "SNPGPU_I8_TAIL_PARTS": ("test_gpu_parity.py", "test_ragged_blocks_and_forced_tail_split"),
}

# ---- every environment variable read anywhere under snprelate_amd/csrc: the GPU test file and function that sets it --------------------
# (the path-selecting switches are set by the parametrised test over CASES, from the cases' environments)
_PATH_TEST = ("test_gpu_kernel_paths.py", "test_kernel_path")
SWITCH_TESTS = dict({k: _PATH_TEST for k in SWITCH_SPACE}, **GEOMETRY_SWITCHES)
SWITCH_TESTS.update({
    "SNPGPU_RUN_INNER": ("test_gpu_kernel_paths.py", "test_fp32_runs_as_one_launch_or_one_launch_per_run"),
    "SNPGPU_PREP_TWO_PASS": ("test_gpu_parity.py", "test_counters_from_2bit_rows_one_pass_prepass"),
    "SNPGPU_EIG_FP32": ("test_gpu_eigen_spectra.py", "test_krylov_routes"),
    "SNPGPU_EIG_F32_PANEL": ("test_gpu_eigen_spectra.py", "test_krylov_routes"),
    "SNPGPU_EIG_MIXED": ("test_gpu_api_golden.py", "test_iterative_eigen_matches_dense"),
    "SNPGPU_EIG_KEEP": ("test_gpu_api_golden.py", "test_iterative_eigen_matches_dense"),
    "SNPGPU_EIG_CHOLQR_MIN_N": ("test_gpu_api_golden.py", "test_iterative_eigen_matches_dense"),
    "SNPGPU_EIG_GRAM_CHUNK": ("test_gpu_api_golden.py", "test_iterative_eigen_matches_dense"),
    "SNPGPU_EIG_DENSE_MAX": ("test_gpu_api_golden.py", "test_eigen_solver_never_returns_unconverged_pairs"),
    "SNPGPU_MDS_STAGE_BYTES": ("test_gpu_mds.py", "test_staging_windows"),
    "SNPGPU_MERGE_STAGE_BYTES": ("test_gpu_geno_merge.py", "test_several_windows_give_the_single_window_result"),
    "SNPGPU_MULTI_COMM": ("test_gpu_multi_device.py", "test_multi_pca_and_gcta_eigen"),
    "SNPGPU_MULTI_GATHER_SERIAL": ("test_gpu_multi_device.py", "test_gather_concurrent_per_device_equals_serial"),
    "SNPGPU_PAIR_BLOCK_SNPS": ("test_gpu_pair_score.py", "test_edge_shapes"),
    "SNPGPU_PCR_BLOCK_SNPS": ("test_gpu_pcrelate.py", "test_forced_block_size_takes_several_internal_blocks"),
    "SNPGPU_PCR_STAGE_BYTES": ("test_gpu_pcrelate.py", "test_small_stage_takes_several_internal_blocks"),
    "SNPGPU_POP_BLOCK_SNPS": ("test_gpu_fst.py", "test_pop_counts_unaligned_device_rows_and_blocks"),
    "SNPGPU_QC_BLOCK_SNPS": ("test_gpu_qc.py", "test_counters_bit_exact"),
    "SNPGPU_SELECT_LDS_WORDS": ("test_gpu_geno_select.py", "test_gather_with_rows_in_global_memory_and_small_lds"),
    "SNPGPU_SELECT_STAGE_BYTES": ("test_gpu_geno_select.py", "test_host_source_through_several_staging_windows"),
    "SNPGPU_TEXT_STAGE_BYTES": ("test_gpu_gen.py", "test_text_memory_kinds_and_staging_windows"),
    "SNPGPU_VCF_STAGE_BYTES": ("test_gpu_vcf.py", "test_text_memory_kinds_and_staging_windows"),
})
EXEMPT = {
    "SNPGPU_EIG_VERBOSE": "prints the solver's phase times to stderr; computes nothing",
    "SNPGPU_PLAN_ALPHA": "host-side panel plan of the multi-device object; tests/test_cpu_host.py holds it",
}

# plan fields that change what a kernel computes without changing its name
PLAN_FIELDS = ("syrk_family", "uv_form", "homo_uv", "homo_form", "eigmix_x1", "sparse_missing", "h3_exact_missing", "uv_targets",
               "wt_layout", "gcta_sparse")
KERNEL_FIELDS = ("counter_kernel_nomiss", "counter_kernel_missing", "syrk_kernel_nomiss", "syrk_kernel_missing")
REFUSED = "refused"

# evaluation points: below X1_SPARSE_MIN_N = 384 and above it (three ragged 256-tiles); a row panel for the kinds with a plane
N_SMALL, N_LARGE, PANEL_ROWS = 300, 700, (256, 512)
N_COUNTER = 279                      # the counter kinds' cases (their plan does not depend on n)

# the arithmetic a SYRK kernel does (two kernels of one family may agree bit for bit, two of different families cannot be expected to)
SYRK_ARITHMETIC = {
    "none": "none",
    "syrk_uv_kernel": "single_product", "syrk_uv16_kernel": "single_product", "syrk_uv16c_kernel": "single_product",
    "syrk_x1_kernel": "exact_row", "syrk_h3_kernel<2, true>": "exact_row",
    "syrk_h3_kernel<2, false>": "two_product", "syrk_h3_kernel<3, false>": "three_product",
    "syrk_mfma_kernel": "fp32",
}


def _all_switch_names():
    return list(SWITCH_SPACE) + list(GEOMETRY_SWITCHES)


class SwitchEnv:
    """os.environ with exactly `env` of the plan's switches set (the library reads them with getenv), restored on exit."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in _all_switch_names()}
        for k in self.saved:
            os.environ.pop(k, None)
        for k, v in self.env.items():
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _signature_here(kind, n, rows=None):
    """signature under os.environ as it stands"""
    from snprelate_amd import _lib
    try:
        d = _lib.diag_plan(getattr(_lib, kind), n, rows=rows)
    except _lib.SnpGpuError:
        return (kind, REFUSED)
    return (kind,) + tuple(d[k] for k in KERNEL_FIELDS) + tuple(d.get(k) for k in PLAN_FIELDS)


def signature(kind, env, n, rows=None):
    """(kind, the four kernel names, PLAN_FIELDS) of a context of `kind` (a name of KIND_NAMES) for n samples created under `env`
    (switch -> value, everything else of the plan's switches unset); (kind, "refused") where snpgpu_create refuses.  env=None: the
    process environment as it is (what a test calls after monkeypatch)."""
    if env is None:
        return _signature_here(kind, n, rows)
    with SwitchEnv(env):
        return _signature_here(kind, n, rows)


def syrk_kernels(sig):
    return () if sig[1] == REFUSED else (sig[3], sig[4])


def counter_kernels(sig):
    return () if sig[1] == REFUSED else (sig[1], sig[2])


def environments():
    names = list(SWITCH_SPACE)
    for values in itertools.product(*(SWITCH_SPACE[k] for k in names)):
        yield {k: v for k, v in zip(names, values) if v is not None}


@functools.lru_cache(maxsize=None)
def _enumerate():
    """signature -> (smallest-set environment, n, rows) that produces it; ties go to the environment met first, full before panel,
    N_LARGE before N_SMALL (so n = N_SMALL marks a signature that exists only below X1_SPARSE_MIN_N)"""
    first = {}
    points = [(N_LARGE, None), (N_SMALL, None), (N_LARGE, PANEL_ROWS)]
    for env in sorted(environments(), key=lambda e: (len(e), sorted(e.items()))):
        with SwitchEnv(env):
            for kind in KIND_NAMES:
                for n, rows in points:
                    if rows and kind not in SYRK_KINDS:
                        continue
                    s = _signature_here(kind, n, rows)
                    if s not in first:
                        first[s] = (dict(env), n, rows)
    return first


def reachable():
    """the distinct signatures over SWITCH_SPACE for the eight kinds (refusals included, as (kind, "refused"))"""
    return set(_enumerate())


# ---- the environments of the two parity fixtures (tests/test_gpu_parity.py reads them from here) -----------------------------------
# value -> (environment, kinds that use it; at least one of them must tell this value from every other value of the fixture)
PAIR_BACKEND_ENVS = {
    "mfma_i8": {},                                                             # deliberately the default (the name is historic)
    "mfma_i8_no_fp4": {"SNPGPU_PAIR_FP4": "0", "SNPGPU_GCTA_MISS_FP4": "0"},
    "mfma_fp4_nomiss_only": {"SNPGPU_PAIR_FP4_GENERAL": "0"},                  # int8 general kernels beside the fp4 two-product kernel
    "popcount": {"SNPGPU_PAIR_BACKEND": "popcount"},
}
PAIR_BACKEND_DEFAULT = "mfma_i8"
PAIR_BACKEND_KINDS = ("IBS", "KING_ROBUST", "KING_HOMO", "GRM_GCTA", "INDIV_BETA")
SYRK_BACKEND_ENVS = {
    "f16": {},                                                                 # deliberately the default
    "f16_uvc": {"SNPGPU_SYRK_UV16": "2"},
    "f16_uv16": {"SNPGPU_SYRK_UV16": "1"},
    "f16_uv32": {"SNPGPU_SYRK_UV16": "0"},
    "f16_x1": {"SNPGPU_SYRK_UV": "0"},
    "f16_2w": {"SNPGPU_SYRK_X1": "0"},
    "h3": {"SNPGPU_SYRK": "h3"},
    "f32": {"SNPGPU_SYRK": "f32"},
}
SYRK_BACKEND_DEFAULT = "f16"
SYRK_BACKEND_KINDS = ("KING_HOMO", "GRM_GCTA", "PCA_COV", "EIGMIX")

# ---- comparison classes ---------------------------------------------------------------------------------------------------------------
EXACT = "bit-exact against the oracle and against the default path"          # IBS / KING-robust / individual beta counters
REL_1E5 = "norms.py: contract and off-diagonal figure < 1e-5"                # every SYRK family (test_grm_gcta's bound)
KING_HOMO_TOL = "test_king_homo: k0 rtol 1e-5 atol 1e-7, k1 rtol 1e-5 atol 2e-5"
DISS_TOL = "test_sum_geno_bit_exact: SumGeno exact, SumAFreq rtol 2e-6 atol 1e-9"
REFUSAL = "snpgpu_create refuses with the plan's text"
COMPARE = {"IBS": EXACT, "KING_ROBUST": EXACT, "INDIV_BETA": EXACT, "KING_HOMO": KING_HOMO_TOL, "GRM_GCTA": REL_1E5, "PCA_COV": REL_1E5,
           "EIGMIX": REL_1E5, "DISS": DISS_TOL}
GPU_TEST = ("test_gpu_kernel_paths.py", "test_kernel_path")


def _case(kind, env, n=N_LARGE, rows=None, compare=None):
    return {"kind": kind, "env": env, "n": n, "rows": rows, "compare": compare or COMPARE[kind], "test": GPU_TEST}


def case_signature(c):
    return signature(c["kind"], c["env"], c["n"], c["rows"])


def case_id(c):
    env = ",".join("%s=%s" % (k[len("SNPGPU_"):], v) for k, v in sorted(c["env"].items())) or "default"
    return "%s-%s%s%s" % (c["kind"], env, "" if c["n"] == N_LARGE else "-n%d" % c["n"], "-panel" if c["rows"] else "")


# One entry per reachable signature, smallest environment first (tests/test_cpu_kernel_paths.py: the set of their signatures IS
# reachable()), then one row panel per SYRK kernel name (PANEL_CASES).
CASES = [
    _case("IBS", {}, n=N_COUNTER),
    _case("IBS", {"SNPGPU_I8_NO_NOMISS": "1"}, n=N_COUNTER),
    _case("IBS", {"SNPGPU_PAIR_BACKEND": "popcount"}, n=N_COUNTER),
    _case("IBS", {"SNPGPU_PAIR_FP4": "0"}, n=N_COUNTER),
    _case("IBS", {"SNPGPU_PAIR_FP4_GENERAL": "0"}, n=N_COUNTER),
    _case("KING_ROBUST", {}, n=N_COUNTER),
    _case("KING_ROBUST", {"SNPGPU_I8_NO_NOMISS": "1"}, n=N_COUNTER),
    _case("KING_ROBUST", {"SNPGPU_PAIR_BACKEND": "popcount"}, n=N_COUNTER),
    _case("KING_ROBUST", {"SNPGPU_PAIR_FP4": "0"}, n=N_COUNTER),
    _case("KING_ROBUST", {"SNPGPU_PAIR_FP4_GENERAL": "0"}, n=N_COUNTER),
    _case("KING_HOMO", {}),
    _case("KING_HOMO", {"SNPGPU_HOMO_UV": "0"}),
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_BACKEND": "popcount"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0"}),
    _case("KING_HOMO", {"SNPGPU_SYRK": "f32"}),
    _case("KING_HOMO", {"SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_HOMO_UV": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_HOMO_UV": "0"}),
    _case("KING_HOMO", {"SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0"}),
    _case("KING_HOMO", {"SNPGPU_HOMO_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_I8_NO_NOMISS": "1"}),
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "f32"}),
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "h3"}),
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "f32"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "h3"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_SYRK": "f32"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_SYRK": "f32"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_HOMO_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_HOMO_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "f32"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "h3"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4_GENERAL": "0", "SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("KING_HOMO", {"SNPGPU_PAIR_FP4": "0", "SNPGPU_I8_NO_NOMISS": "1", "SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {}),
    _case("GRM_GCTA", {}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_SYRK": "f32"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK": "h3"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_MISS3": "1"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "0"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "1"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "1"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "2"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "2"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_SYRK_X1": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK": "f32"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK": "h3"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_MISS3": "1"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV16": "0"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV16": "1"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV16": "1"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV16": "2"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV16": "2"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_X1": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "f32"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "h3"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_MISS3": "1"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "0"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "1"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "1"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "2"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV16": "2"}, n=N_SMALL),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_X1": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_MISS3": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_SYRK_X1": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_MISS3": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_GCTA_MISS_FP4": "0", "SNPGPU_SYRK_X1": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_MISS3": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("GRM_GCTA", {"SNPGPU_PAIR_BACKEND": "popcount", "SNPGPU_SYRK_X1": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("PCA_COV", {}),
    _case("PCA_COV", {}, n=N_SMALL),
    _case("PCA_COV", {"SNPGPU_SYRK": "f32"}),
    _case("PCA_COV", {"SNPGPU_SYRK": "h3"}),
    _case("PCA_COV", {"SNPGPU_SYRK_MISS3": "1"}),
    _case("PCA_COV", {"SNPGPU_SYRK_UV": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK_UV16": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK_UV16": "0"}, n=N_SMALL),
    _case("PCA_COV", {"SNPGPU_SYRK_UV16": "1"}),
    _case("PCA_COV", {"SNPGPU_SYRK_UV16": "1"}, n=N_SMALL),
    _case("PCA_COV", {"SNPGPU_SYRK_UV16": "2"}),
    _case("PCA_COV", {"SNPGPU_SYRK_UV16": "2"}, n=N_SMALL),
    _case("PCA_COV", {"SNPGPU_SYRK_X1": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK_MISS3": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK_UV": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("PCA_COV", {"SNPGPU_SYRK_X1": "0", "SNPGPU_SYRK_UV16": "0"}),
    _case("EIGMIX", {}),
    _case("EIGMIX", {"SNPGPU_SYRK": "f32"}),
    _case("EIGMIX", {"SNPGPU_SYRK": "h3"}),
    _case("EIGMIX", {"SNPGPU_SYRK_MISS3": "1"}),
    _case("EIGMIX", {"SNPGPU_SYRK_UV16": "0"}),
    _case("EIGMIX", {"SNPGPU_SYRK": "f32", "SNPGPU_SYRK_UV16": "0"}),
    _case("EIGMIX", {"SNPGPU_SYRK": "h3", "SNPGPU_SYRK_UV16": "0"}),
    _case("EIGMIX", {"SNPGPU_SYRK_MISS3": "1", "SNPGPU_SYRK_UV16": "0"}),
    _case("INDIV_BETA", {}, n=N_COUNTER),
    _case("INDIV_BETA", {"SNPGPU_PAIR_BACKEND": "popcount"}, n=N_COUNTER),
    _case("INDIV_BETA", {"SNPGPU_PAIR_FP4": "0"}, n=N_COUNTER),
    _case("DISS", {}),
    _case("DISS", {"SNPGPU_PAIR_BACKEND": "popcount"}, compare=REFUSAL),
    _case("DISS", {"SNPGPU_SYRK_UV16": "0"}),
]

# one row panel (rows 256 ... 512 of 700) per reachable PAIR of SYRK kernels (block without / with missing calls), which covers every
# SYRK kernel name in either position; their signatures are those of the full contexts above
PANEL_CASES = [
    _case("GRM_GCTA", {}, rows=PANEL_ROWS),                                    # syrk_uv16c_kernel, syrk_x1_kernel
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "1"}, rows=PANEL_ROWS),             # syrk_uv16_kernel, syrk_x1_kernel
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV16": "0"}, rows=PANEL_ROWS),             # syrk_uv_kernel, syrk_x1_kernel
    _case("GRM_GCTA", {"SNPGPU_SYRK_UV": "0"}, rows=PANEL_ROWS),               # syrk_x1_kernel for every block
    _case("GRM_GCTA", {"SNPGPU_SYRK_X1": "0"}, rows=PANEL_ROWS),               # syrk_h3_kernel<2, true> for every block
    _case("GRM_GCTA", {"SNPGPU_SYRK_MISS3": "1"}, rows=PANEL_ROWS),            # syrk_h3_kernel<2, true> + <3, false>, picked by the device flag
    _case("GRM_GCTA", {"SNPGPU_SYRK": "h3"}, rows=PANEL_ROWS),                 # syrk_h3_kernel<3, false>
    _case("GRM_GCTA", {"SNPGPU_SYRK": "f32"}, rows=PANEL_ROWS),                # syrk_mfma_kernel
    _case("KING_HOMO", {}, rows=PANEL_ROWS),                                   # none, syrk_uv16_kernel on KING-homo's binary tables
    _case("KING_HOMO", {"SNPGPU_SYRK_UV16": "0"}, rows=PANEL_ROWS),            # none, syrk_uv_kernel
    _case("KING_HOMO", {"SNPGPU_HOMO_UV": "0"}, rows=PANEL_ROWS),              # none, syrk_h3_kernel<2, false>
    _case("KING_HOMO", {"SNPGPU_SYRK": "h3", "SNPGPU_HOMO_UV": "0"}, rows=PANEL_ROWS),   # none, syrk_h3_kernel<3, false>
    _case("KING_HOMO", {"SNPGPU_SYRK": "f32"}, rows=PANEL_ROWS),               # none, syrk_mfma_kernel
    _case("KING_HOMO", {"SNPGPU_I8_NO_NOMISS": "1"}, rows=PANEL_ROWS),         # syrk_h3_kernel<2, false> for every block
]
CASES += PANEL_CASES
