// Accumulator contexts (ctx_*.hip): the environment switches, and the kernel path they select for a context -- decided ONCE, by a
// function that makes no HIP call and allocates nothing.  snpgpu_create allocates from the plan, the feed reads it
// (DESIGN.md 17a).  Below them: the context itself, the plan next to its runtime state.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "snpgpu_internal.h"

namespace snpgpu {

// ---- switches: every SNPGPU_* variable of snpgpu_create, read when a context is created -----------------------------------------
// Two kinds.  PRESENCE: the variable counts once it is set, whatever its value (even "0").  VALUE: unset = the default, set =
// "not 0" (atoi), so "=0" switches a default-on path off and "=1" equals unset.
inline bool env_present(const char *name) { return getenv(name) != nullptr; }
inline bool env_nonzero(const char *name, bool unset)
{
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : unset;
}
// an integer taken only inside [lo, hi]
inline int env_int_in(const char *name, int lo, int hi, int unset)
{
    const char *e = getenv(name);
    if (!e) return unset;
    const int v = atoi(e);
    return (v >= lo && v <= hi) ? v : unset;
}

enum class SyrkChoice { Default, F32, H3 };      // SNPGPU_SYRK unset / "f32" / "h3"

struct Switches {
    // fp64 planes tile-major (snpgpu_internal.h: acc_off); row-major with SNPGPU_ACC_LAYOUT=row and for the rocBLAS form of
    // the eigen solver's panel product (SNPGPU_EIG_BLAS, presence), which needs a leading dimension
    bool acc_layout_row = false, eig_blas = false;
    // IBS / KING / beta counters: exact MFMA contractions by default; SNPGPU_PAIR_BACKEND=popcount selects the bit-plane
    // kernel (same counters, kept for comparison and for the GCTA missing mask)
    bool pair_popcount = false;
    bool pair_fp4 = true;            // blocks without missing calls on the MX-fp4 MFMA (SNPGPU_PAIR_FP4=0: the int8 two-product kernel)
    bool pair_fp4_general = true;    // ... and the general kernels (blocks with missing calls; SNPGPU_PAIR_FP4_GENERAL=0: int8)
    bool gcta_miss_fp4 = true;       // GCTA both-missing counts on the MX-fp4 MFMA (SNPGPU_GCTA_MISS_FP4=0: the int8 kernel)
    bool i8_no_nomiss = false;       // SNPGPU_I8_NO_NOMISS (presence): no two-product kernel for blocks without missing calls
    // GCTA denominators: blocks with FEW missing calls count the both-missing pairs from SETS of samples (pair_sparse_miss_kernel,
    // work ~ f^2) instead of the dense int8 product (81 ms per 32 768-SNP block at N = 100 000 whatever f).  Measured at
    // N = 100 000 (A/B on one box, bench.py --missing f): f = 0.2 %: 42 ms, 0.5 %: 75 ms, 1 %: 136 ms, 2 %: 285 ms -- the
    // per-thread nested walk over two 256-bit sets diverges badly and the sets themselves are 160 GB of L2 reads per block; the
    // sparse form is therefore taken up to 0.2 % missing calls in a block (well-called array / sequence data; 0.3 % before the dense
    // product moved to the fp4 instruction: 44 ms per 32 768 SNPs), the dense
    // product beyond.  SNPGPU_GCTA_SPARSE=0: always dense; SNPGPU_GCTA_SPARSE_MAX_RATE overrides the threshold (tests: 0.03)
    bool gcta_sparse = true;
    double gcta_sparse_max_rate = 0.002;   // (0.003 while the dense product was the int8 kernel: 81 ms per 32 768 SNPs; fp4: 44)
    // split-fp16 MFMAs for every SYRK table (GRM / PCA / EIGMIX: |z| <= ~1e3, small values only next to O(1)
    // ones; KING-homo: sqrt(p(1-p)) and p(1-p) are multiplied by 2^8 so that p(1-p) ~ 1e-6 stays in fp16's
    // normal range, the finaliser divides the sums by 2^16); SNPGPU_SYRK=f32 keeps the fp32-MFMA kernel, =h3 three products
    SyrkChoice syrk = SyrkChoice::Default;
    int h3_super = H3_SUPER, x1_super = H3_SUPER / 2;   // SNPGPU_H3_SUPER / SNPGPU_X1_SUPER, 1 ... 32 (tuning)
    // the exact-row kernel with one wave per SIMD (syrk_x1_kernel) where it applies (GRM / PCA); SNPGPU_SYRK_X1=0: two waves
    // per SIMD (syrk_h3_kernel<2, true>, the round-2 kernel before it; measurement only)
    bool syrk_x1 = true;
    // SNPGPU_SYRK_MISS3 (presence): three products for blocks with missing calls, as in round 1 (A/B measurements)
    bool syrk_miss3 = false;
    // fp32 run lengths (snpgpu_internal.h: H3_PROMOTE_*): SNPGPU_SYRK_FAST=1 = one 32 768-SNP run per flush and one weight
    // target (round 2's kernels: 1.6e-5 instead of < 1e-5 in the off-diagonal figure); SNPGPU_H3_PROMOTE sets both run
    // lengths (a multiple of 256 in 256 ... 65 536; 0 here = unset; measurements)
    bool syrk_fast = false;
    int h3_promote = 0;
    // blocks WITHOUT missing calls of a GRM / PCA context: the single-product kernel (syrk_uv_kernel: the SNP weight as
    // a product of two fp16 numbers, integer centres); SNPGPU_SYRK_UV=0: the exact-row kernel for every block
    bool syrk_uv = true;
    bool uv_targets = true;          // SNPGPU_UV_TARGETS=0: one weight target for every run (measurement)
    // rare variants of blocks WITH missing calls: their carriers' pairs in fp64 beside the exact-row kernel (GRM / PCA
    // weights only; SNPGPU_X1_SPARSE=0: everything in the dense product, as before)
    bool x1_sparse = true;
    bool x1_short_runs = true;       // ... and such blocks as 4096-SNP fp32 runs of the exact-row kernel (SNPGPU_X1_SHORT_RUNS=0: 8192 as every other block)
    int x1_sparse_mac = X1_SPARSE_MAC;   // SNPGPU_X1_SPARSE_MAC lowers it (clamped to 1 ... X1_SPARSE_MAC)
    // KING-homo, blocks with missing calls: SNPGPU_HOMO_UV=0: the two-product kernels as before round 5
    bool homo_uv = true;
    // the single-product kernel on v_mfma_f32_16x16x32_f16 (round 6: the same products and fp32 runs, half the accumulator traffic per flop
    // under the socket power cap).  SNPGPU_SYRK_UV16: 0 = the 32x32x16 form (syrk_uv_kernel); 1 = syrk_uv16_kernel (operands looked up in
    // LDS tables -- what KING-homo's binary tables and EIGMIX always take); 2 = syrk_uv16c_kernel (GRM / PCA contexts: nibble words, one
    // v_cvt_scalef32_pk_f16_fp4 + one v_pk_fma_f16 per operand dword, no tables); 3 = ... and a work item walks the fp32 runs of its tile
    // itself, half of its sub-tile sums carried in the freed LDS between runs.  Default 3 with the pace-maker fetches on (SNPGPU_UVC_PACE=0:
    // off): -2.4 % per step against the lookup form, panel writes -40 %, word fetches -12 % (profiles/r06_uvc_ab.txt; without the pace-maker
    // the workgroups of an XCD drift apart and fetch 2.4 x the words).  Values outside 0 ... 3 are clamped.
    int syrk_uv16 = 3;
    bool uvc_pace = true;
    // ... form 3: the sub-tile sums LDS cannot hold (29 of a wave's 64) wait in a scratch slot of device memory between runs instead of
    // meeting the fp64 panel after every run: one panel flush per block (3.3 passes of atomics -> 1.0).  SNPGPU_UVC_CARRY_ALL=0: today's
    // per-run atomics for those sub-tiles, exactly.  SNPGPU_UVC_CARRY_SLOTS: slots per XCD pool (0 ... 256, default 64 = twice the
    // workgroups an XCD holds; 0: no slot, every work item takes the per-run atomics; tests).
    // MEASURED (configs[2], one box, profiles/carry_all_ab.json): 436.6 against 439.5 ms per step in alternating rounds of one process (-0.7 %, every
    // round below every round of the old form), 437.4 against 441.6 with bench.py alternated; WRITE_SIZE 133 -> 87.5 GB per step (40 of panel
    // atomics + 47 of scratch stores, which the L2 writes through), FETCH_SIZE raw 173.5 -> 202 GB; no work item without a slot.
    bool uvc_carry_all = true;
    int uvc_carry_slots = UV_CARRY_SLOTS;
    int i8_tail_parts = 0;           // SNPGPU_I8_TAIL_PARTS 1 ... 64: K parts of the last round of a work list (0: chosen per list)

    static Switches from_env()
    {
        Switches s;
        const char *e;
        s.acc_layout_row = (e = getenv("SNPGPU_ACC_LAYOUT")) && std::string(e) == "row";
        s.eig_blas = env_present("SNPGPU_EIG_BLAS");
        s.pair_popcount = (e = getenv("SNPGPU_PAIR_BACKEND")) && std::string(e) == "popcount";
        s.pair_fp4 = env_nonzero("SNPGPU_PAIR_FP4", true);
        s.pair_fp4_general = env_nonzero("SNPGPU_PAIR_FP4_GENERAL", true);
        s.gcta_miss_fp4 = env_nonzero("SNPGPU_GCTA_MISS_FP4", true);
        s.i8_no_nomiss = env_present("SNPGPU_I8_NO_NOMISS");
        s.gcta_sparse = env_nonzero("SNPGPU_GCTA_SPARSE", true);
        if ((e = getenv("SNPGPU_GCTA_SPARSE_MAX_RATE"))) { const double v = atof(e); if (v >= 0 && v <= 1) s.gcta_sparse_max_rate = v; }
        if ((e = getenv("SNPGPU_SYRK"))) s.syrk = std::string(e) == "f32" ? SyrkChoice::F32 : std::string(e) == "h3" ? SyrkChoice::H3 : SyrkChoice::Default;
        s.h3_super = env_int_in("SNPGPU_H3_SUPER", 1, 32, s.h3_super);
        s.x1_super = env_int_in("SNPGPU_X1_SUPER", 1, 32, s.x1_super);
        s.syrk_x1 = env_nonzero("SNPGPU_SYRK_X1", true);
        s.syrk_miss3 = env_present("SNPGPU_SYRK_MISS3");
        s.syrk_fast = env_nonzero("SNPGPU_SYRK_FAST", false);
        s.h3_promote = env_int_in("SNPGPU_H3_PROMOTE", 256, 65536, 0);
        if (s.h3_promote % 256) s.h3_promote = 0;
        s.syrk_uv = env_nonzero("SNPGPU_SYRK_UV", true);
        s.uv_targets = env_nonzero("SNPGPU_UV_TARGETS", true);
        s.x1_sparse = env_nonzero("SNPGPU_X1_SPARSE", true);
        s.x1_short_runs = env_nonzero("SNPGPU_X1_SHORT_RUNS", true);
        if ((e = getenv("SNPGPU_X1_SPARSE_MAC"))) s.x1_sparse_mac = std::max(1, std::min(atoi(e), X1_SPARSE_MAC));
        s.homo_uv = env_nonzero("SNPGPU_HOMO_UV", true);
        if ((e = getenv("SNPGPU_SYRK_UV16"))) s.syrk_uv16 = std::max(0, std::min(atoi(e), 3));
        s.uvc_pace = env_nonzero("SNPGPU_UVC_PACE", true);
        s.uvc_carry_all = env_nonzero("SNPGPU_UVC_CARRY_ALL", true);
        s.uvc_carry_slots = env_int_in("SNPGPU_UVC_CARRY_SLOTS", 0, UV_CARRY_SLOTS_MAX, s.uvc_carry_slots);
        s.i8_tail_parts = env_int_in("SNPGPU_I8_TAIL_PARTS", 1, 64, 0);
        return s;
    }
};

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
struct CtxPlan {
    // what was asked for, and the panel: sample rows [row0, row1) x columns [col0, N) with col0 = row0
    int kind = 0, bayesian = 0;
    int64_t N = 0, row0 = 0, row1 = 0, col0 = 0;
    int64_t rows_pad = 0, ncols_pad = 0, RB = 0, Bmax = 0;
    int KWmax = 0;
    bool full = false;
    int64_t acc_tiles_c = 0;     // fp64 planes tile-major: ncols_pad / 256 (0 = row-major)
    int tail_parts = 0;          // forced K parts of a work list's last round (0: chosen per list)
    // pair counters
    bool use_pc = false;
    int pc_mode = 0, n_u32 = 0;
    bool pc_i8 = false;          // on MFMAs (w2 words) instead of bit planes
    bool miss_fp4 = true, nomiss_fp4 = true, general_fp4 = false;   // which of them on the MX-fp4 MFMA (Switches)
    int pc_tile_r = 0, pc_tile_c = 0, pc_wg_per_cu = 2;             // work list of the general kernel
    bool want_het = false;       // two-product kernel for blocks without missing calls: per-sample het counts + its own work list
    int nm_tile_r = 0, nm_tile_c = 0, nm_wg_per_cu = 2;
    bool gcta_sparse = false;    // GCTA denominators from sets of samples for blocks of at most sp_max_rate missing calls
    double sp_max_rate = 0.0;
    // SYRK tables
    bool use_mm = false;
    int n_lut = 0, n_f64 = 0, lut_mode[2] = {0, 0};
    bool mm_h3 = false;          // split-fp16 MFMAs instead of fp32 MFMAs
    int h3_super = H3_SUPER, x1_super = H3_SUPER / 2;
    bool h3_exact_rows = false;  // table 0: two-product kernel with the exact row operand (g - c_s) 2^shift
    bool h3_exact_missing = false;   // ... also for blocks WITH missing calls (row value of a missing call = fp16(avg - c_s)); else three products there
    // row operand of the two-product kernel per table: -1 none (three products), 0 g - 1 (exact rows),
    // 1 call indicator (KING-homo weights), 2 missing indicator (EIGMIX both-missing weights)
    int h3_a_kind[2] = {-1, -1};
    int h3_w_shift = 0;          // exact-row tables hold w * 2^-shift, the row operand is +-2^shift (fp16 range, |w| <= 4N)
    int h3_promote = 0, uv_promote = 0;   // fp32 runs: exact-row kernel (SNPs), single-product kernel (slots)
    bool want_x1_list = false;   // work list of syrk_x1_kernel / syrk_uv*_kernel (256 x 256 tiles, one workgroup per CU)
    bool uv_enabled = false;     // blocks without missing calls on the single-product kernel (GRM / PCA, EIGMIX)
    bool uv_eigmix = false;      // ... for the EIGMIX numerator (weight 1: exact)
    bool uv_targets = false;     // a weight target per fp32 run (uv_factor_kernel)
    UvForm uv_form = UvForm::Mfma32x32x16;
    bool uvc_pace = false;       // Converted forms: pace-maker fetches on
    bool uvc_carry_all = false;  // ConvertedCarry: every sub-tile sum carried between runs, those beyond LDS in scratch slots ...
    int uvc_carry_slots = 0;     // ... of which each XCD's pool has this many
    bool eigmix_x1 = false;      // EIGMIX numerator of blocks with missing calls on syrk_x1_kernel, from its own 12 * code words
    bool sparse_missing = false; // rare variants of blocks with missing calls: carriers' pairs added in fp64 (uv_sparse_kernel)
    bool x1_short_runs = true;   // ... and such blocks as half-length fp32 runs (device flag)
    int x1_sparse_mac = 0;
    WordLayout wt_layout = WordLayout::Entry8Or16;
    bool wt_block_flag = false;  // the words (and EIGMIX's per-sample pass) read the block's missing-call flag
    // KING-homo / dissimilarity weights
    bool homo_uv = false;        // blocks with missing calls: totals - per-sample missing sums + ONE fp16 product per weight
    UvForm homo_form = UvForm::Mfma32x32x16;   // ... its kernel (binary tables: always a lookup form)
    int homo_weights = 0;        // 2, dissimilarity: the first only

    bool uvc() const { return uv_form == UvForm::Converted || uv_form == UvForm::ConvertedCarry; }
    // padded block of the single-product tables
    int64_t Bpad() const { return std::max<int64_t>((Bmax + 1023) / 1024 * 1024, 2 * UV_CHS); }
};

inline int64_t plan_round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// 0, or 1 with *error set (no prefix)
inline int plan_context(int kind, int64_t n_samp, const snpgpu_opts &o, const Switches &sw, CtxPlan *out, std::string *error)
{
    CtxPlan p;
    if (kind < SNPGPU_IBS || kind > SNPGPU_DISS) { *error = "invalid kind"; return 1; }
    if (n_samp <= 0 || n_samp > 0x7fffffffLL) { *error = "invalid number of samples"; return 1; }
    p.kind = kind; p.bayesian = o.bayesian; p.N = n_samp;
    p.row0 = o.row_begin; p.row1 = o.row_end;
    if (p.row0 == 0 && p.row1 == 0) p.row1 = n_samp;
    if (p.row0 < 0 || p.row1 > n_samp || p.row0 >= p.row1 || (p.row0 % PANEL_ALIGN) != 0) {
        *error = "invalid panel rows (row_begin must be a multiple of 256, < row_end <= n_samp)";
        return 1;
    }
    p.full = (p.row0 == 0 && p.row1 == n_samp);
    p.col0 = p.row0;
    p.rows_pad = plan_round_up(p.row1 - p.row0, PANEL_ALIGN);
    p.ncols_pad = plan_round_up(p.N - p.col0, PANEL_ALIGN);
    p.RB = plan_round_up(p.N, 256) / 4;
    p.Bmax = plan_round_up(o.max_block_snps > 0 ? o.max_block_snps : 32768, 64);       // 32 768: the block bench.py feeds for GRM / PCA
    p.KWmax = (int)(p.Bmax / 32);
    p.acc_tiles_c = (sw.acc_layout_row || sw.eig_blas) ? 0 : p.ncols_pad / ACC_TILE;
    p.tail_parts = sw.i8_tail_parts;

    switch (kind) {
    case SNPGPU_IBS: p.use_pc = true; p.pc_mode = PM_IBS; break;
    case SNPGPU_KING_ROBUST: p.use_pc = true; p.pc_mode = PM_KING_ROBUST; break;
    case SNPGPU_KING_HOMO:
        p.use_pc = true; p.pc_mode = PM_KING_HOMO;
        p.use_mm = true; p.n_lut = 2; p.lut_mode[0] = LUT_HOMO_W1; p.lut_mode[1] = LUT_HOMO_W2;
        break;
    case SNPGPU_GRM_GCTA:
        p.use_pc = true; p.pc_mode = PM_GCTA_MISS;
        p.use_mm = true; p.n_lut = 1; p.lut_mode[0] = LUT_GCTA;
        break;
    case SNPGPU_PCA_COV:
        p.use_mm = true; p.n_lut = 1; p.lut_mode[0] = o.bayesian ? LUT_BAYES : LUT_GCTA;
        break;
    case SNPGPU_EIGMIX:
        p.use_mm = true; p.n_lut = 2; p.lut_mode[0] = LUT_EIGMIX_NUM; p.lut_mode[1] = LUT_EIGMIX_MISSW;
        break;
    case SNPGPU_INDIV_BETA: p.use_pc = true; p.pc_mode = PM_BETA; break;
    case SNPGPU_DISS:      // SumGeno on the MX-fp4 counter kernels, SumAFreq = 8 x KING-homo's first weight sum
        p.use_pc = true; p.pc_mode = PM_DISS;
        p.use_mm = true; p.n_lut = 1; p.lut_mode[0] = LUT_HOMO_W1;
        break;
    }
    p.n_u32 = p.use_pc ? pair_mode_counters(p.pc_mode) : 0;
    p.n_f64 = p.n_lut;

    if (p.use_pc) {
        p.pc_i8 = !sw.pair_popcount;
        if (p.pc_i8) {
            pair_i8_tile(p.pc_mode, &p.pc_tile_r, &p.pc_tile_c, &p.pc_wg_per_cu);
            p.nomiss_fp4 = sw.pair_fp4;
            int ftr = 0, ftc = 0, fw = 1;
            if (p.nomiss_fp4 && sw.pair_fp4_general && pair_fp4_tile(p.pc_mode, &ftr, &ftc, &fw)) {
                p.general_fp4 = true; p.pc_tile_r = ftr; p.pc_tile_c = ftc; p.pc_wg_per_cu = fw;
            }
            p.miss_fp4 = sw.gcta_miss_fp4;
            // blocks without missing calls: binary 3-product kernel (IBS and KING-robust), 128 x 128 tiles
            // (the dissimilarity counter has no other form for such blocks: always)
            p.want_het = ((p.pc_mode == PM_IBS || p.pc_mode == PM_KING_ROBUST || p.pc_mode == PM_KING_HOMO) && !sw.i8_no_nomiss) ||
                         p.pc_mode == PM_DISS;
            if (p.want_het) pair_i8_tile(PM_IBS_NOMISS, &p.nm_tile_r, &p.nm_tile_c, &p.nm_wg_per_cu);
            p.gcta_sparse = p.pc_mode == PM_GCTA_MISS && sw.gcta_sparse;
            if (p.gcta_sparse) p.sp_max_rate = sw.gcta_sparse_max_rate;
        }
    }
    if (p.use_mm) {
        const bool gp = p.lut_mode[0] == LUT_GCTA || p.lut_mode[0] == LUT_BAYES;      // GRM / PCA weights
        const bool eig = p.lut_mode[0] == LUT_EIGMIX_NUM;
        p.mm_h3 = sw.syrk != SyrkChoice::F32;
        p.h3_super = sw.h3_super; p.x1_super = sw.x1_super;
        // exact-row-side kernel for blocks without missing calls (tables of the form y (g - avg) only)
        p.h3_exact_rows = sw.syrk == SyrkChoice::Default && (gp || eig);
        for (int i = 0; i < p.n_lut; i++) {
            const int m = p.lut_mode[i];
            p.h3_a_kind[i] = sw.syrk != SyrkChoice::Default ? -1
                             : (i == 0 && p.h3_exact_rows) ? 0
                             : (m == LUT_HOMO_W1 || m == LUT_HOMO_W2) ? 1 : (m == LUT_EIGMIX_MISSW) ? 2 : -1;
        }
        // |w| = y^2 |g - avg| <= 4N(1 + 1/N) in a block without missing calls (num = N; singleton: p = 1/2N): keep it
        // below 2^15 by moving a power of two to the (exact) row operand.  EIGMIX has y = 1.
        if (p.h3_exact_rows && !eig)
            while (std::ldexp(4.04 * (double)p.N, -p.h3_w_shift) > 32768.0) p.h3_w_shift++;
        // the exact-row kernel also for blocks WITH missing calls (GRM / PCA; EIGMIX shares its words with the 8-byte-entry
        // table of the both-missing weights and keeps three products there)
        p.h3_exact_missing = p.h3_exact_rows && !eig && !sw.syrk_miss3;
        p.h3_promote = sw.syrk_fast ? H3_PROMOTE_FAST : H3_PROMOTE_EXACT;
        p.uv_promote = sw.syrk_fast ? H3_PROMOTE_FAST : H3_PROMOTE_UV;
        if (sw.h3_promote) p.h3_promote = p.uv_promote = sw.h3_promote;
        const bool x1 = p.h3_exact_rows && sw.syrk_x1 && !sw.syrk_miss3;
        const bool uv_gp = x1 && p.h3_exact_missing && gp && sw.syrk_uv;
        // EIGMIX numerator sum (g_i - 2p)(g_j - 2p): weight 1 = 1 x 1, so the single-product form is EXACT there; its words
        // carry 8 * code for every block (the both-missing weight table and the three-product kernel of the blocks with
        // missing calls have 8-byte entries as well)
        p.uv_eigmix = x1 && eig && sw.syrk_uv;
        // (EIGMIX: the list only serves the single-product kernel of its blocks without missing calls)
        p.want_x1_list = x1 && (!eig || p.uv_eigmix);
        p.uv_enabled = uv_gp || p.uv_eigmix;
        p.uv_targets = uv_gp && !sw.syrk_fast && sw.uv_targets;      // (EIGMIX's weight 1 is exact)
        p.sparse_missing = uv_gp && p.N >= X1_SPARSE_MIN_N && sw.x1_sparse;
        p.x1_sparse_mac = sw.x1_sparse_mac;
        p.x1_short_runs = sw.x1_short_runs;
        // EIGMIX blocks WITH missing calls: the numerator on the exact-row kernel as well (round 3; the three-product kernel it
        // took before drops lo lo': 2.3e-5 of the off-diagonal scale at L = 1e6).  Its 12-byte entries need 12 * code words:
        // a second transposition for such blocks (the both-missing weight table keeps its 8 * code words).
        p.eigmix_x1 = p.uv_eigmix && !sw.syrk_miss3;
        p.wt_layout = p.uv_eigmix ? WordLayout::Entry8Or16 : p.uv_enabled ? WordLayout::Entry12Or8
                      : p.want_x1_list ? WordLayout::Entry12 : p.h3_exact_missing ? WordLayout::Entry16 : WordLayout::Entry8Or16;
        p.wt_block_flag = p.h3_exact_rows && !p.uv_eigmix;
    }
    // KING-homo, blocks with missing calls (round 5): masked weight sums = totals - per-sample missing sums + ONE fp16 product of
    // binary operands per weight (homo_uv_tables_kernel, syrk_uv_kernel) instead of two-product SYRKs of an indicator against a
    // hi / lo operand.  Needs the two-scalar form of the blocks without missing calls (the binary counter kernel's contexts)
    p.homo_uv = kind == SNPGPU_KING_HOMO && p.mm_h3 && p.want_het && sw.homo_uv;
    p.homo_weights = 2;
    // individual dissimilarity: the first weight of that path only, and the MX-fp4 counters; no other form exists (no silent fall-back)
    if (kind == SNPGPU_DISS) {
        p.homo_uv = p.mm_h3 && p.want_het;
        p.homo_weights = 1;
        if (!p.homo_uv || !p.pc_i8 || !p.nomiss_fp4 || !p.general_fp4) {
            *error = "the dissimilarity kind needs the MX-fp4 counter kernels and the fp16 weight product (SNPGPU_PAIR_BACKEND, "
                     "SNPGPU_PAIR_FP4, SNPGPU_PAIR_FP4_GENERAL or SNPGPU_SYRK select a form it does not have)";
            return 1;
        }
    }
    const UvForm lookup = sw.syrk_uv16 ? UvForm::Lookup16x16x32 : UvForm::Mfma32x32x16;
    const bool conv = sw.syrk_uv16 >= 2 && p.uv_enabled && !p.uv_eigmix;
    p.uv_form = !conv ? lookup : sw.syrk_uv16 == 3 ? UvForm::ConvertedCarry : UvForm::Converted;
    p.homo_form = lookup;
    p.uvc_pace = conv && sw.uvc_pace;       // on / off (the size is fixed: 16 KiB per wave)
    p.uvc_carry_all = p.uv_form == UvForm::ConvertedCarry && sw.uvc_carry_all;
    p.uvc_carry_slots = p.uvc_carry_all ? sw.uvc_carry_slots : 0;
    *out = p;
    return 0;
}

// ---- a block of n_snp SNPs on the SYRK side -----------------------------------------------------------------------------------
// syrk_x1_kernel walks rounds of eight 16-SNP groups, syrk_uv_kernel of sixteen.
// The single-product kernel runs a block as fp32 runs of `cpr` table chunks (one launch and one fp64 flush each); with
// more than one run every run carries its own weight target and the block's SNPs are dealt to the runs (uv_assign_kernel)
// (at least two runs = two targets: one target leaves the weights at 1.05e-6 rms, 1.1e-5 at worst over the 1.6e8 entries
// of an 18 000-sample panel; a block of a single table chunk is spread over two half-empty ones -- twice the MFMA work
// of a block that is small anyway)
struct BlockRuns {
    int uv_runs = 1, uv_cpr = 1, uv_chunks = 0;
    int uv_q = 1;          // weight targets
    int64_t n_pad = 0;     // padded SNPs = slots of the single-product kernel's K dimension
    int n_q = 0;           // groups of 16 SNPs (= 2 pair-coded dwords per sample)
};
inline BlockRuns plan_block(const CtxPlan &p, int64_t n_snp)
{
    BlockRuns b;
    const bool targets = p.uv_targets && !p.uv_eigmix;
    if (p.uv_enabled) {
        const int64_t run0 = std::max<int64_t>(UV_CHS, (int64_t)p.uv_promote / UV_CHS * UV_CHS);
        b.uv_chunks = std::max((int)(plan_round_up(n_snp, UV_CHS) / UV_CHS), targets ? 2 : 1);
        if (n_snp > run0 || targets) {
            const int runs0 = std::max(targets ? 2 : 1, (int)((b.uv_chunks * (int64_t)UV_CHS + run0 - 1) / run0));
            b.uv_cpr = (b.uv_chunks + runs0 - 1) / runs0;                  // balanced: 32 chunks at <= 11 per run = 11 + 11 + 10
            b.uv_runs = (b.uv_chunks + b.uv_cpr - 1) / b.uv_cpr;
        }
    }
    b.uv_q = (targets && b.uv_runs > 1) ? std::min(b.uv_runs, UV_QMAX) : 1;
    b.n_pad = (p.uv_enabled && b.uv_runs > 1) ? (int64_t)b.uv_chunks * UV_CHS
                                              : plan_round_up(n_snp, (p.uv_enabled || p.homo_uv) ? 256 : p.want_x1_list ? 128 : 64);
    b.n_q = (int)(b.n_pad / 16);
    return b;
}

}  // namespace snpgpu

struct snpgpu_ctx {
    // What the context computes and with which kernels: decided once at creation (ctx_plan.h), read-only afterwards.  Everything
    // below it is runtime state: streams, buffers, the block counts of the work lists, what is pending.
    snpgpu::CtxPlan plan;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n_snp_total = 0;
    // asynchronous host feeds: second stream + double-buffered raw block + events
    hipStream_t copy_stream = nullptr;
    snpgpu::DevBuf raw2[2];
    hipEvent_t ev_copied[2] = {nullptr, nullptr};    // H2D of raw2[k] finished
    hipEvent_t ev_consumed[2] = {nullptr, nullptr};  // repack of raw2[k] finished (buffer reusable)
    const void *host_src[2] = {nullptr, nullptr};
    int raw_turn = 0;
    int diag_mirrored = 0;        // eigen solver: 1 = diagonal 64 x 64 tiles mirrored, 2 = whole diagonal square
    bool frozen = false;          // snpgpu_finalize_inplace: plane 0 of acc_f64 holds the FINAL matrix (upper trapezoid of the
    int frozen_diagadj = 0;       //   panel rectangle); no feeds may follow, the kind's finaliser copies it out
    double frozen_scale = 1.0;
    void *blas = nullptr;         // rocblas_handle, created on first use
    bool timing = false;
    int64_t syrk_launches = 0;    // kernel launches of launch_syrk / launch_syrk_h3 / launch_syrk_uv since creation (snpgpu_diag_syrk_launches)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];  // [0] pair popcount, [1] SYRK

    // feed-block scratch
    snpgpu::DevBuf raw, packed, sum, num, lut[2], rowp, colp, wt, w2, scalars, family, miss_diag, dvals, samp_het, samp_dmiss, samp_dsq;
    snpgpu::DevBuf eig_qt;        // eigen solver: sample-major copy of the current vector block, double [N][48]
    snpgpu::DevBuf acc_f32;       // eigen solver: fp32 copy of plane 0 for the fp32 products (made on first use where memory allows)
    bool acc_f32_valid = false;   //     ... and whether it still mirrors the plane (a feed invalidates it)
    snpgpu::DevBuf het_blk;       // per-block het counts of the one-pass pre-pass (committed to `het` when the block's flag is final)
    snpgpu::DevBuf het, i8_work_nm;   // binary pair kernel for blocks without missing calls: per-sample het counts, its work list
    int i8_blocks_nm = 0;
    bool het_pending = false;
    snpgpu::DevBuf ccoef, tcorr;   // exact-row-side SYRK: per-SNP {u, v} and per-chunk column terms [Bmax / H3_LUTCH + 1][ncols_pad]
    snpgpu::DevBuf colterm;        // ... their running total per column (fp64 [ncols_pad]), subtracted from every row of the
    bool colterm_pending = false;  //     panel once, before a result is read (ctx_settle, ctx_results.hip)
    snpgpu::DevBuf wt12;           // EIGMIX: 12 * code words of a block with missing calls (exact-row kernel of the numerator)
    snpgpu::DevBuf uvpace;         // syrk_uv16c_kernel: 64 KiB per table chunk that every workgroup fetches (zeros; see the kernel)
    snpgpu::DevBuf uvcarry, uvcarry_flags;   // ... its carry scratch (plan.uvc_carry_all: slots of 116 KiB) and the slots' flag words
    snpgpu::DevBuf uvlut, uvslot;  // single-product SYRK: its own tables (8-byte entries, per SLOT) and the slot -> SNP map of the current block
    snpgpu::DevBuf uvcand;         // ... per SNP and weight target: {relative error, u | v << 16}, {t, avg}, SNP -> slot
    snpgpu::DevBuf uvcoef, uvterm, uvkpart, uvsp;   // ... (blocks without missing calls): per-SNP {d_b uv, c_a, d_a uv, c_b},
                                   //     the running row / column terms {R[ncols_pad], Q[ncols_pad], K} and per-chunk parts of K
    snpgpu::DevBuf homo_lut[2], homo_wts, homo_tc, homo_msum, homo_work;   // KING-homo blocks with missing calls: tables, effective weights, per-chunk partials, M[2][ncols_pad], work list
    int homo_blocks = 0;
    snpgpu::DevBuf nosh;         // dissimilarity, KING-homo: which pairs share no call at an SNP of nonzero weight (kernels_final.hip, nosh_*)
    snpgpu::DevBuf diss_called;  // dissimilarity, KING-homo: per column sample, 1 once it is called at an SNP of nonzero weight (exact zero denominators)
    // accumulators
    snpgpu::DevBuf acc_u32, acc_f64;
    snpgpu::TileGrid tg_pc{}, tg_mm{};
    snpgpu::DevBuf tg_pc_tab, tg_mm_tab;
    int i8_blocks = 0;         // work items (= workgroups) of the MFMA pair kernel, see build_worklist (worklist.h)
    snpgpu::DevBuf i8_work;    // int4 {tile row, tile col, K part, K parts} per workgroup, XCD-interleaved
    snpgpu::DevBuf mm256, sp_work;   // GCTA denominators, sparse form: per (256-sample group, SNP) set of missing calls; its 256 x 256 work list
    int sp_blocks = 0;
    int h3_blocks = 0;
    snpgpu::DevBuf h3_work;
    int x1_blocks = 0;          // work list of syrk_x1_kernel (256 x 256 tiles, one workgroup per CU); 0: not used
    snpgpu::DevBuf x1_work;

    snpgpu_ctx() = default;
    ~snpgpu_ctx();              // ctx_life.hip: events, streams and the rocBLAS handle on the context's device; the buffers follow

    // scalars layout: SCALAR_SLOTS slots of 8 bytes (unsigned long long / double) -- the allocation in snpgpu_create is exactly
    // this many, a ninth scalar needs SCALAR_SLOTS raised with it:
    // [0] missing cells of the current block, [1] nLocus, [2] trace (double), [3] EIGMIX SumDenominator (double),
    // [4..5] KING-homo weight sums of the blocks without missing calls, [6..7] route of this block's both-missing counts
    // [8] this block holds rare variants on the fp64 sparse path next to missing calls: the exact-row kernel runs it as 4096-SNP fp32 runs
    static constexpr int SCALAR_SLOTS = 16;
    unsigned long long *d_missing() { return (unsigned long long *)scalars.p; }
    unsigned long long *d_nlocus() { return (unsigned long long *)scalars.p + 1; }
    double *d_trace() { return (double *)scalars.p + 2; }
    double *d_sumden() { return (double *)scalars.p + 3; }
    double *d_homo_w() { return (double *)scalars.p + 4; }   // [2]: sum p(1-p), sum (p(1-p))^2 over the blocks without missing calls (KING-homo)
    unsigned long long *d_short_runs() { return (unsigned long long *)scalars.p + 8; }
    unsigned long long *d_miss_route() { return (unsigned long long *)scalars.p + 6; }   // [2]: this block's both-missing counts take the sparse / the dense form

    snpgpu::PanelGeom geom() const
    {
        return snpgpu::PanelGeom{plan.N, plan.row0, plan.row1, plan.col0, plan.rows_pad, plan.ncols_pad, plan.acc_tiles_c};
    }
    int64_t plane() const { return plan.rows_pad * plan.ncols_pad; }
    double *plane_f64(int i) { return (double *)acc_f64.p + (size_t)i * (size_t)plane(); }
    // the plane every SYRK launch of table i adds to
    snpgpu::SyrkPanel syrk_panel(const snpgpu::DevBuf &words, int i)
    {
        return snpgpu::SyrkPanel{(const uint32_t *)words.p, plan.ncols_pad, plane_f64(i), plan.ncols_pad, plan.acc_tiles_c, plan.N - plan.row0};
    }
};
