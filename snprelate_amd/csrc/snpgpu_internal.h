// Internal declarations shared by the HIP translation units of libsnpgpu.
// Device data layout (all per context, see DESIGN.md 3, "Data layout in HBM"):
//
//   packed   uint8  [B][RB]            2-bit genotypes of the current feed block, SNP-major,
//                                      RB = round_up(N,256)/4 bytes per SNP, samples >= N are 3
//   sum,num  int32  [B]                per-SNP genotype sum / non-missing count over all N
//   lut      float2 [nlut][Bpad/2][16] per-SNP-pair decode table: entry c0 + 4*c1 = (z_2p(c0), z_2p+1(c1))
//   wt       uint32 [Bpad/8][ncols_pad] sample-major pair-coded words (byte p = 8*(c0+4*c1) of SNPs 8d+2p, 8d+2p+1)
//   w2       uint32 [Bpad/16][ncols_pad] sample-major 2-bit words (code of SNP 16d+m at bits 2m), int8-MFMA pair kernel
//   rowp     PV     [rows_pad/8][KW][8] bit planes of the panel's row samples, 8 rows of one word adjacent
//   colp     PV     [KW][ncols_pad]    word-major bit planes of the panel's column samples
//   acc_u32  uint32 [C][rows_pad][ld]  pair counters,   rectangular panel, ld = ncols_pad
//   acc_f64  double [S][rows_pad][ld]  pair fp64 sums,  rectangular panel
//
// A panel covers sample rows [row0,row1) and columns [col0,N) with col0 = row0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

#include "../../include/snpgpu.h"

struct snpgpu_ctx;

namespace snpgpu {

constexpr int PANEL_ALIGN = 256;   // row0 / padded extents are multiples of this
// Layout of the fp64 accumulator planes (round 3): TILE-MAJOR, 256 x 256 tiles of 512 KB, rows of a tile 2 KB apart -- the
// fp64 flush of a SYRK wave (128 rows x 32-column pieces) and the eigen solver's panel product (64-row strips) then work
// inside a few hundred KB instead of striding through rows 8 * ncols_pad bytes (800 KB at N = 100 000, 4 MB at 500 000)
// apart.  tiles_c = ncols_pad / 256 (0: row-major with leading dimension ld -- SNPGPU_ACC_LAYOUT=row, and the rocBLAS form
// of the panel product).  Panel-relative (r, c) -> element offset:
constexpr int ACC_TILE = 256;
__host__ __device__ __forceinline__ int64_t acc_off(int64_t ld, int64_t tiles_c, int64_t r, int64_t c)
{
    return tiles_c ? ((((r >> 8) * tiles_c + (c >> 8)) << 16) + ((r & 255) << 8) + (c & 255)) : (r * ld + c);
}
constexpr int PC_ROWS_PER_WAVE = 8;
constexpr int PC_WAVES = 4;
constexpr int PC_TILE_R = PC_ROWS_PER_WAVE * PC_WAVES;  // 32 rows per workgroup
constexpr int PC_COLS_PER_LANE = 2;
constexpr int PC_TILE_C = 64 * PC_COLS_PER_LANE;         // 128 columns per workgroup
constexpr int PC_SUPER = 8;                              // 8x8 workgroup tiles per XCD super-tile
constexpr int MM_TILE_R = 128;                           // SYRK workgroup tile: 128 rows x 128 columns
constexpr int MM_TILE_C = 128;                           //   (4 waves as 2x2, each 64 x 64 = 2x2 MFMA 32x32 tiles)
constexpr int MM_PROMOTE = 1024;                         // SNPs accumulated in fp32 (one rounding per 2 SNPs) before the fp64 flush
constexpr int MM_LUTCH = 256;                            // SNPs per LDS-resident decode-table chunk (128 pairs x 128 B)
constexpr int MM_SUPER = 4;                              // 4x4 tiles per XCD super-tile
constexpr int H3_TILE_R = 256;                           // split-fp16 SYRK: 256 x 128 workgroup tile
constexpr int H3_TILE_C = 128;                           //   (4 waves as 2x2, each 128 x 64 = 4x2 MFMA 32x32 tiles)
#ifndef X1_CHS_SNPS
#define X1_CHS_SNPS 512
#endif
constexpr int X1_CHS = X1_CHS_SNPS;                       // ... SNPs per LDS table chunk (12-byte entries: 96 bytes per SNP)
constexpr int UV_CHS = 1024;                             // single-product SYRK (syrk_uv_kernel): SNPs per LDS table chunk (8-byte entries: 64 bytes per SNP)
constexpr int UV_SPARSE_MAC = 128;                       // ... SNPs with at most this many copies of the minor allele are added sparsely in fp64 (uv_sparse_kernel)
constexpr int X1_SPARSE_MAC = 128;                       // ... blocks WITH missing calls: up to this many copies (512: 8.2e-6 instead of 9.3e-6 on the
                                                         // rare-variant spectrum for +10 % of its step; SNPGPU_X1_SPARSE_MAC lowers it),
constexpr int X1_SPARSE_MIN_N = 384;                     // in contexts of at least this many samples (smaller data sets: bit-reproducible runs),
constexpr double X1_SPARSE_MIN_W = 64.0;                  // blocks WITH missing calls: ... and only where the weight 1 / (p (1 - p)) is at least this
constexpr int UV_CHUNK = 64;                             // ... slots per centre-balancing chunk (uv_tables_kernel)
constexpr int X1_TILE = 256;                             // single-wave-per-SIMD exact-row SYRK: 256 x 256 workgroup tile (4 waves of 128 x 128)
constexpr int H3_SUPER = 8;                              // 8 x 8 tiles per XCD super-tile: the 64 workgroups resident on an XCD share rows / columns (L2 word fetches -17 % against 4 x 4)
constexpr int H3_PROMOTE = 4096;                          // SNPs accumulated in fp32 before the fp64 flush (split-fp16 SYRK, three products)
// fp32 run lengths of the exact-row / single-product kernels (one launch and one fp64 flush per run; a flush = 5e9 fp64 atomics
// at N = 100 000: 7.7 ms, bound by the L2 atomic rate -- flat vs global address space, fp32 instead of fp64 operands and the
// order of the 256 instructions of a wave make no difference, tools/scratch A/B of round 4).  The accumulation error grows with
// sqrt(run): measured over ALL 3.7e8 entries of an 8192-row panel at configs[2]'s size 32 768-SNP runs put the maximum of the
// off-diagonal figure at 1.2e-5 (exact-row) / 1.6e-5 (single product, one weight target), 16 384 at 7e-6 / 1.2e-5 -- hence 8192 SNPs
// for the exact-row kernel.  The single-product kernel's runs also set its number of weight targets (kernels_tables.hip,
// uv_factor_kernel): a 32 768-SNP block = 3 runs of <= 11 264 slots, weight error 0.37e-6 rms, no refinement slots.
// SNPGPU_H3_PROMOTE overrides both; SNPGPU_SYRK_FAST=1 restores one 32 768-SNP run (one target).
constexpr int H3_PROMOTE_EXACT = 8192;          // (16 384: 29 of 3.7e8 entries above 1e-5, maximum 1.17e-5, on GCTA with 2 % missing calls)
constexpr int H3_PROMOTE_UV = 11264;            // slots per run of the single-product kernel (11 table chunks)
constexpr int H3_PROMOTE_FAST = 32768;
constexpr int UV_QMAX = 8;                      // runs of a block that may carry their own weight target (more runs: one target)
// carry scratch of syrk_uv16c_kernel (ConvertedCarry): the sub-tiles of a wave that LDS cannot hold between runs (64 - 35), as f32x4 per
// lane; a slot serves the four waves of a workgroup (116 KiB).  Flag words: [0] work items that found no free slot (diagnostic),
// [UV_CARRY_FLAG0 + xcd * slots + s] 1 while slot s of XCD xcd's pool is taken.  UV_GETREG_XCC_ID: s_getreg operand of bits 3:0 of
// hardware register 20 (XCC_ID)
constexpr int UV_CARRY_REST = 29;
constexpr int UV_CARRY_SLOT_BYTES = 4 * UV_CARRY_REST * 64 * 16;
constexpr int UV_CARRY_FLAG0 = 16;
constexpr int UV_CARRY_XCDS = 8;
constexpr int UV_CARRY_SLOTS = 64;              // per XCD: twice the 32 workgroups an XCD holds at one per CU (58 MiB in all)
constexpr int UV_CARRY_SLOTS_MAX = 256;
constexpr int UV_GETREG_XCC_ID = ((4 - 1) << 11) | 20;
inline size_t uv_carry_flag_bytes(int slots) { return sizeof(unsigned int) * (size_t)(UV_CARRY_FLAG0 + UV_CARRY_XCDS * slots); }
inline size_t uv_carry_scratch_bytes(int slots) { return (size_t)UV_CARRY_XCDS * (size_t)slots * (size_t)UV_CARRY_SLOT_BYTES; }
__host__ __device__ __forceinline__ double uv_run_factor(int q) { return 1.0 - (double)q * (1.0 / 4096.0); }   // flush factor of run q
constexpr int H3_HOMO_SHIFT = 8;                          // KING-homo tables are multiplied by 2^8 for the fp16 split
constexpr int H3_LUTCH = 512;                            // SNPs per LDS table chunk of the split-fp16 SYRK (2 x 32 KiB)
constexpr int I8_SUPER = 4;                              // int8-MFMA pair kernel: 4x4 tiles per XCD super-tile

void set_error(const std::string &msg);

#define SNPGPU_HIP_CHECK(expr)                                                             \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            ::snpgpu::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e)); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

// counter sets of the bit-plane pair kernel
enum PairMode { PM_IBS = 0, PM_KING_ROBUST = 1, PM_KING_HOMO = 2, PM_GCTA_MISS = 3, PM_BETA = 4,
                PM_IBS_NOMISS = 5 /* int8 kernel only: IBS / KING-robust for blocks without missing calls */,
                PM_HOMO_NOMISS = 6 /* ... KING-homo for such blocks: the same two products into its two planes */,
                PM_DISS = 7 /* individual dissimilarity: one plane, sum g (2 - g') + (2 - g) g' over the SNPs both samples are called at */ };
constexpr int pair_mode_counters(int m) { return (m == PM_IBS || m == PM_BETA) ? 3 : m == PM_KING_ROBUST ? 5 : m == PM_KING_HOMO ? 2 : 1; }

// decode-table flavours of the SYRK kernel (what z(g) is)
enum LutMode {
    LUT_GCTA = 0,      // (g - 2p)/sqrt(p(1-p)), 0 unless 0<p<1        (genPCA.cpp:98-181)
    LUT_BAYES = 1,     // (g - 2p)/sqrt(s(1-s)), s=(sum+1)/(2num+2)    (genPCA.cpp:441-453)
    LUT_HOMO_W1 = 2,   // sqrt(p(1-p))          -> sum_mask p(1-p)      (genKING.cpp:236-248)
    LUT_HOMO_W2 = 3,   // p(1-p)                -> sum_mask (p(1-p))^2
    LUT_EIGMIX_NUM = 4,  // g - 2p (no scaling; missing -> 0)                 (genEIGMIX.cpp:104-110)
    LUT_EIGMIX_MISSW = 5 // sqrt(4p(1-p)) for MISSING calls, 0 otherwise -> weighted both-missing sums
};

void pair_i8_tile(int mode, int *tile_r, int *tile_c, int *wg_per_cu = nullptr);
bool pair_fp4_tile(int mode, int *tile_r, int *tile_c, int *wg_per_cu);

// form of the single-product SYRK (syrk_uv*_kernel)
enum class UvForm {
    Mfma32x32x16 = 0,      // syrk_uv_kernel
    Lookup16x16x32 = 1,    // syrk_uv16_kernel: operands looked up in LDS tables (tables with swapped odd quarters)
    Converted = 2,         // syrk_uv16c_kernel: operands CONVERTED from nibble words (`uvlut` holds the slots' factors, `wt` bytes
                           // c0 | c1 << 4 in blocks without missing calls); GRM / PCA contexts only
    ConvertedCarry = 3     // ... and a work item walks its tile's runs itself, half the sub-tile sums carried in LDS as fp32
};
// what a byte of the pair-coded words holds (transpose8_kernel): the table offset of the pair's entry
enum class WordLayout {
    Entry8Or16 = 0,        // 8 * code; 16 * code in a block without missing calls when the block flag is passed
    Entry16 = 1,           // 16 * code in every block
    Entry12 = 2,           // 12 * code in every block
    Entry12Or8 = 3,        // 12 * code, 8 * code in a block without missing calls (single-product kernel: 8-byte entries)
    Entry12Missing = 4     // 12 * code, written only for a block WITH missing calls (EIGMIX: a second word array)
};

// which blocks a launch of colcorr_kernel / colterm_add_kernel serves, by the block's missing-call flag
enum class ColcorrBlocks { WithoutMissing = 0, Every = 1, WithMissing = 2 };

struct TileGrid {      // upper-trapezoid tile enumeration with XCD super-tiles
    int tile_r, tile_c;        // tile extents in samples
    int super;                 // super-tile edge in tiles
    int n_tr, n_tc;            // tiles per panel (rows / cols)
    int n_sr;                  // super-tile rows
    int n_super;               // valid super-tiles
    int grid;                  // workgroups to launch
    int *d_prefix;             // [n_sr+1] prefix count of valid super-tiles per super-row
    int *d_first;              // [n_sr]   first valid super-col per super-row
};

// ---- launchers (defined in the .hip files) --------------------------------
int launch_sym_panel_matmul(hipStream_t st, const double *P, int64_t ld, int64_t tiles_c, int64_t nI, int64_t nJ, int64_t col0,
                            int64_t N, double scale, const double *Q, int m, double *Y, double *qt_scratch, bool fp32_products = false,
                            const float *P32 = nullptr);
int launch_panel_to_f32(hipStream_t st, const double *src, float *dst, size_t n_elems);
// linkage disequilibrium (kernels_ld.hip): staging rows of rbp bytes (a multiple of 32), 64-row tiles read whole
int launch_ld_stage(hipStream_t st, const void *src, int format, int64_t n, int64_t n_samp, int64_t rbp, uint8_t *dst);
int launch_ld_count_rect(hipStream_t st, const uint8_t *A, int n_a, const uint8_t *B, int n_b, int64_t rbp, int32_t *tab);
int launch_ld_count_band(hipStream_t st, const uint8_t *rows, int i_lo, int n_i, int n_rows, int slide, int64_t rbp, int32_t *tab);
int launch_ld_final_band(hipStream_t st, const int32_t *tab, int64_t n_i, int slide, int64_t i0, int64_t n_snp, int method, double *out);
int launch_ld_final_rect(hipStream_t st, const int32_t *tab, int64_t n_i, int64_t n_j, int64_t i0, int method, double *out);
// LD pruning: threshold bits of band tables [n_i][w][9] -> uint64 [n_i][ceil(w / 64)] (pairs with i0 + t < start transposed)
int launch_ld_prune_bits(hipStream_t st, const int32_t *tab, int64_t n_i, int w, int64_t i0, int64_t n_snp, int64_t start, int method,
                         double threshold, uint64_t *bits);
// LD scores (kernels_ld_score.hip): band tables [n_i][w][9] of rows i0 ... -> terms vals[(k - 1) n_i + (i - i0)] (NaN: not valid or
// outside the window hi[]) and the number of valid ones added to the LD_SCORE_COUNT_SLOTS counters at n_valid (their sum counts);
// then the ordered fold into acc / nv [n_snp]
constexpr int LD_SCORE_COUNT_SLOTS = 256;
int launch_ld_score_init(hipStream_t st, double *acc, int32_t *nv, int64_t n, double self);
int launch_ld_score_terms(hipStream_t st, const int32_t *tab, int64_t n_i, int w, int64_t i0, const int32_t *hi, int method, int adjust,
                          double *vals, uint64_t *n_valid);
int launch_ld_score_fold(hipStream_t st, const double *vals, int64_t n_i, int w, int64_t i0, int64_t n_snp, const int32_t *lo,
                         const int32_t *hi, double *acc, int32_t *nv);
// staging a feed block (kernels_prep.hip)
int launch_repack_stats(hipStream_t st, const void *src, int format, int64_t n_snp, int64_t n_samp, uint8_t *packed,
                        int64_t RB, int32_t *sum, int32_t *num, unsigned long long *d_missing);
int launch_repack(hipStream_t st, const void *src, int format, int64_t n_snp, int64_t n_samp,
                  uint8_t *packed, int64_t RB);
int launch_snp_stats(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                     int32_t *sum, int32_t *num, unsigned long long *d_missing_cells, int32_t *nhet = nullptr);
// per-SNP tables (kernels_tables.hip)
// table pass of one SYRK table (build_lut_kernel); the named fields are the kernel's arguments of the same names
struct BuildLutOpts {
    int lut_mode = 0;
    bool split16 = false;
    float2 *lut = nullptr;
    unsigned long long *d_nlocus = nullptr;
    double *d_sumden = nullptr, *dvals = nullptr;
    const unsigned long long *d_missing = nullptr;
    double2 *ccoef = nullptr;
    bool exact_rows_always = false;
    int w_shift = 0;
    bool exact_with_missing = false, entry12 = false;
    double *homo_const = nullptr;
    double4 *uvsp_miss = nullptr;
    int x1_sparse_mac = 0;
    unsigned long long *d_short_runs = nullptr;
};
int launch_build_lut(hipStream_t st, const int32_t *sum, const int32_t *num, int64_t n_snp, int64_t n_snp_pad, const BuildLutOpts &o);
struct BuildUvOpts {
    int lut_mode = 0;
    uint2 *lut = nullptr;
    double4 *uvcoef = nullptr, *uvsp = nullptr;
    double *kpart = nullptr;
    float *cand_err = nullptr;
    uint32_t *cand_uv = nullptr;
    double2 *snp_tavg = nullptr;
    int32_t *slot_of = nullptr, *slot_src = nullptr;
    int n_target = 1, cpr = 1;
    const unsigned long long *d_missing = nullptr;
    UvForm form = UvForm::Mfma32x32x16;          // table layout of the kernel that reads them
};
int launch_build_uv(hipStream_t st, const int32_t *sum, const int32_t *num, int64_t n_snp, int64_t n_snp_pad, const BuildUvOpts &o);
int launch_homo_tables(hipStream_t st, const int32_t *sum, const int32_t *num, int64_t n_snp, int64_t n_snp_pad, uint2 *lut1, uint2 *lut2,
                       double2 *wts, double *totals, const unsigned long long *d_missing, int swap_odd = 0, int n_w = 2);
// per-sample terms beside the SYRKs (kernels_terms.hip)
int launch_colcorr(hipStream_t st, const uint32_t *w8, int64_t ncols_pad, int n_d, const double2 *ccoef, double *tc,
                   double *colterm, const unsigned long long *d_missing, ColcorrBlocks blocks = ColcorrBlocks::WithoutMissing,
                   int entry12 = 0);
int launch_uvcorr(hipStream_t st, const uint32_t *w8, int64_t ncols_pad, int n_d, const double4 *uvcoef, const double *kpart,
                  int n_kpart, double2 *tc, double *uvterm, const unsigned long long *d_missing, int nibble = 0);
int launch_uv_sparse(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t N, int64_t row0, int64_t row1,
                     int64_t col0, const double4 *uvsp, double *acc, int64_t ld, int64_t tiles_c, int64_t ncols_pad, double *uvterm,
                     const unsigned long long *d_missing, int missing_blocks = 0);
int launch_homo_miss_sums(hipStream_t st, const uint32_t *w8, int64_t ncols_pad, int n_d, const double2 *wts, double2 *tc, double *msum,
                          const unsigned long long *d_missing);
int launch_eigmix_samples(hipStream_t st, const uint32_t *w8, int n_d, int64_t ncols_pad, int64_t col0,
                          const double *dvals, uint32_t *het, double *dmiss, double *dsq,
                          const unsigned long long *d_wide16 = nullptr);
// SNP-major to sample-major words (kernels_transpose.hip)
struct Transpose8Opts {
    int n_d = 0;
    uint32_t *w8 = nullptr;
    const unsigned long long *d_block_flag = nullptr;   // the block's missing-call flag (the kernel's d_wide16)
    WordLayout layout = WordLayout::Entry8Or16;
    const int32_t *slot_src = nullptr;
    bool nibble_nomiss = false;
};
int launch_transpose8(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t col0, int64_t ncols_pad,
                      const Transpose8Opts &o);
// (sample-major 2-bit words of the MFMA pair counters: IBS / KING / beta)
int launch_transpose2(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t col0,
                      int64_t ncols_pad, int n_d, uint32_t *w2, uint32_t *het = nullptr,
                      const unsigned long long *d_missing = nullptr, bool classic = false);
int launch_transpose2_missmask(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                               const int32_t *sum, const int32_t *num, int64_t col0, int64_t ncols_pad, int n_d,
                               uint32_t *w2, uint32_t *diag, const unsigned long long *d_skip_if_zero);
int launch_missmask256(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t N, const int32_t *sum,
                       const int32_t *num, int64_t col0, int n_groups, int64_t snp_stride, uint4 *mm,
                       unsigned long long max_cells, unsigned long long *flags);
int launch_transpose2_direct(hipStream_t st, const uint8_t *src, int64_t n_samp, int64_t n_snp, int64_t col0,
                             int64_t ncols_pad, int n_d, uint32_t *w2, uint32_t *het, uint32_t *het_blk,
                             unsigned long long *d_missing);
int launch_bitplanes4(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                      int64_t col0, int64_t ncols_pad, int64_t rows_pad, int KW, uint4 *rowp, uint4 *colp);
int launch_bitplanes_miss(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                          const int32_t *sum, const int32_t *num, int64_t col0, int64_t ncols_pad,
                          int64_t rows_pad, int KW, uint2 *rowp, uint2 *colp,
                          const unsigned long long *d_missing_cells);
// synthetic genotypes (kernels_synth.hip)
int launch_synth_block(hipStream_t st, uint8_t *dst, int64_t n_samp, int64_t snp_begin, int64_t n_snp, uint32_t seed,
                       uint32_t miss32, int spectrum, int special);
// PCA projections (kernels_proj.hip)
int launch_proj_snp(hipStream_t st, int corr, const uint32_t *w2, int64_t ncols_pad, int64_t N, int64_t n_snp,
                    const double *et, int kp, int k, const int32_t *sum, const int32_t *num, int bayesian, double *out,
                    double *part, int *cnt, double *out_avg, double *out_scale, const double *ext_avg = nullptr,
                    const double *ext_scale = nullptr);
int launch_proj_samp(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t N, int64_t n_snp, const double *sl,
                     int kp, int k, const double *af, const double *sc, double *out);
int launch_proj_transpose(hipStream_t st, const double *src, int64_t N, int k, double *dst, int64_t n_pad, int kp);
// settling the per-sample terms into the panel (kernels_final.hip), pair counters (kernels_pair.hip)
int launch_colterm_settle(hipStream_t st, double *acc, int64_t ld, int64_t tiles_c, int64_t n_rows_real, int64_t ncols_pad, int64_t n_cols_real,
                          double *colterm, double *uvterm = nullptr);
int launch_pair_popcount(hipStream_t st, int mode, const TileGrid &tg, const void *rowp, const void *colp,
                         int KW, int64_t ncols_pad, uint32_t *acc, int64_t acc_plane,
                         const unsigned long long *d_skip_if_zero);
int launch_pair_sparse_miss(hipStream_t st, const uint4 *mm, int64_t snp_stride, int n_snp, uint32_t *acc, int64_t ncols_pad,
                            const int4 *work, int n_blocks, const unsigned long long *d_run);
int launch_pair_fp4_miss(hipStream_t st, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad, int n_s,
                         uint32_t *acc, const unsigned long long *d_missing);
int launch_pair_i8(hipStream_t st, int mode, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad,
                   int n_q, int n_snp, uint32_t *acc, int64_t acc_plane, const unsigned long long *d_missing,
                   const int4 *work_nm = nullptr, int n_blocks_nm = 0, bool fp4_nomiss = false, bool fp4_general = false);
int launch_het_settle(hipStream_t st, uint32_t *acc, int64_t plane, int64_t rows_pad, int64_t ncols_pad, uint32_t *het,
                      int king, int plane_ibs1 = 1, int plane_ibs0x2 = 2);
// what every SYRK launch shares: the pair-coded words and the fp64 plane they add to
struct SyrkPanel { const uint32_t *w8; int64_t ncols_pad; double *acc; int64_t ld, tiles_c, n_rows_real; };
struct SyrkH3Opts {
    const int4 *work = nullptr, *work_x1 = nullptr;
    int n_blocks = 0, n_blocks_x1 = 0;
    const uint2 *lut = nullptr;
    int n_q = 0, a_kind = -1, promote_snps = 0;
    const unsigned long long *d_skip_if_zero = nullptr, *d_missing = nullptr, *d_short_runs = nullptr;
    int64_t *n_launched = nullptr;               // where given: raised by one per kernel launch (snpgpu_diag_syrk_launches)
};
int launch_syrk_h3(hipStream_t st, const SyrkPanel &p, const SyrkH3Opts &o);
struct SyrkUvOpts {
    const int4 *work_x1 = nullptr;
    int n_blocks_x1 = 0;
    const uint2 *lut = nullptr;                  // Converted forms: the slots' factor arrays
    int n_q = 0;
    const unsigned long long *d_missing = nullptr;
    int run_chunks = 0, n_target = 1;
    bool run_if_missing = false;
    int64_t copy_lut_bytes = 0, copy_acc_elems = 0;   // table / plane stride between the copies of a work list (KING-homo's weights)
    UvForm form = UvForm::Mfma32x32x16;
    const void *pace_src = nullptr;              // Converted forms: the pace-maker (16 x 1 KiB per wave and chunk) and its switch
    bool pace = false;
    void *carry_scr = nullptr;                   // ConvertedCarry: the carry scratch (nullptr: off), its flag words, slots per XCD
    unsigned int *carry_flags = nullptr;
    int carry_slots = 0;
    int64_t *n_launched = nullptr;               // as SyrkH3Opts::n_launched
};
int launch_syrk_uv(hipStream_t st, const SyrkPanel &p, const SyrkUvOpts &o);
int launch_syrk(hipStream_t st, const TileGrid &tg, const uint32_t *w8, int64_t ncols_pad, const float2 *lut,
                int n_q, double *acc, int64_t ld, int64_t tiles_c, const unsigned long long *d_skip_if_zero = nullptr);

// finalisers: panel accumulators -> caller layout (device buffers)
struct PanelGeom {
    int64_t N, row0, row1, col0, rows_pad, ncols_pad;
    int64_t f64_tiles_c;       // fp64 planes: 0 = row-major [rows_pad][ncols_pad], else tile-major with this many 256-column tiles per row
};
int launch_fin_ibs_num(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int32_t *o0, int32_t *o1,
                       int32_t *o2, int packed);
int launch_fin_ibs_ave(hipStream_t st, const PanelGeom &g, const uint32_t *acc, double *out, int packed);
int launch_fin_king_counts(hipStream_t st, const PanelGeom &g, const uint32_t *acc, uint32_t *out5);
int launch_fin_king_robust(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const int32_t *family,
                           double *ibs0, double *kin, int packed);
int launch_fin_king_homo(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *facc, double fscale,
                         double *k0, double *k1, int packed, const double *w_const = nullptr, const double *msum = nullptr,
                         const uint32_t *called = nullptr, const uint32_t *nosh = nullptr);
// individual dissimilarity: out = SumGeno / SumAFreq (x 2 on the diagonal), or (out == nullptr) the packed sums themselves
int launch_fin_diss(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *facc, double fscale, const double *w_const,
                    const double *msum, const uint32_t *called, double *out, uint32_t *geno_sum, double *wsum, int packed,
                    const uint32_t *nosh = nullptr);
// rank-one terms of the dissimilarity counter of blocks without missing calls: SumGeno += 2 (S_r + S_c), S = H + 2 T; then het = 0
int launch_diss_settle(hipStream_t st, uint32_t *acc, int64_t rows_pad, int64_t ncols_pad, uint32_t *het);
// called[j] = 1 once column sample j is called at an SNP of this block with 0 < p < 1 (packed rows [n_snp][RB])
int launch_diss_called(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, const int32_t *sum, const int32_t *num,
                       int64_t col0, int64_t ncols, uint32_t *called);
// Pairs without a shared call (KING-homo, dissimilarity; see kernels_final.hip): the words of the tracking buffer for ncols_pad columns,
// and the per-block update (packed rows [n_snp][RB], the block's per-SNP sum / num)
constexpr int NOSH_HEAVY = 64;         // samples that may be missing at half the SNPs of a block or more, over the whole stream
constexpr int64_t nosh_words(int64_t ncols_pad) { return 8 + 3 * ncols_pad + NOSH_HEAVY + (int64_t)NOSH_HEAVY * ncols_pad; }
int launch_nosh_block(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, const int32_t *sum, const int32_t *num,
                      int64_t col0, int64_t ncols, int64_t ncols_pad, uint32_t *nosh);
int launch_fin_gcta(hipStream_t st, const PanelGeom &g, const double *num, const uint32_t *miss,
                    const uint32_t *diag, const unsigned long long *d_nlocus, double *out, int packed,
                    const double *colterm = nullptr, const double *uvterm = nullptr);
int launch_miss_diag(hipStream_t st, const uint2 *colp, int KWv, int64_t ncols_pad, int64_t col0, uint32_t *diag,
                     const unsigned long long *skip);
int launch_fin_cov(hipStream_t st, const PanelGeom &g, const double *num, double scale, double *out, int packed);
int launch_trace(hipStream_t st, const PanelGeom &g, const double *num, double *d_trace);
int launch_fin_mom(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *e, int constraint,
                   double *k0, double *k1, int packed);
int launch_fin_eigmix(hipStream_t st, const PanelGeom &g, const double *num, const double *dd, const uint32_t *het,
                      const double *dmiss, const double *dsq, const double *d_sumden, int diagadj, double scale, double *out, int packed);
int launch_beta_reduce(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int diag_inbreeding, double *partial_min,
                       double *partial_sum, int nblocks);
int launch_fin_beta(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int mode, double avg, double mn, double *out,
                    int packed);
int launch_mirror_diag(hipStream_t st, const PanelGeom &g, double *num);

// selection of related pairs (kernels_select.hip): the pairs row0 <= i < row1, i < j < N of the panel with sel[i] && sel[j] (absolute
// samples; nullptr: all) and kinship >= cutoff (non-finite cutoff: every pair), in the order i ascending, j ascending.  write == false
// fills counts[select_segments(g)]; launch_select_scan turns them into offsets[segments + 1] (the last one = the total); write == true
// stores the first `capacity` pairs (any output may be nullptr).  The kinds take the arguments of their finalisers.
constexpr int64_t SELECT_MAX_GRID = 1 << 20;   // workgroups of a pass (one row each, stride loop beyond)
struct SelectArgs {
    const uint8_t *sel; double cutoff;
    uint32_t *counts; int64_t *offsets;
    int64_t capacity; int32_t *idx1, *idx2; double *v0, *v1, *kin;
    double *v2 = nullptr;      // the fourth value of a kind that has one (launch_select_pcr: nsnp)
};
// the context kind a selection's `what` accumulates on
inline int select_kind(int what) { return what == SNPGPU_SEL_KING_ROBUST ? SNPGPU_KING_ROBUST : what == SNPGPU_SEL_KING_HOMO ? SNPGPU_KING_HOMO : SNPGPU_IBS; }
int64_t select_segments(const PanelGeom &g);
int launch_select_scan(hipStream_t st, const uint32_t *counts, int64_t n_seg, int64_t *offsets);
int launch_select_king_robust(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const int32_t *family, const SelectArgs &s, bool write);
int launch_select_king_homo(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *facc, double fscale, const double *w_const,
                            const double *msum, const uint32_t *called, const uint32_t *nosh, const SelectArgs &s, bool write);
int launch_select_mom(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *e, int constraint, const SelectArgs &s, bool write);
// The GRM kinds (one value per pair, stored in s.kin; s.v0 / s.v1 are not used): the arguments of launch_fin_gcta / _cov / _eigmix /
// _beta.  pass: the count pass, the write pass, or the diagonal -- diag[k] = the entry (row0 + k, row0 + k) for the panel's real rows
// k < min(row1, N) - row0, by the same value function, whatever s.sel says.
enum SelPass { SEL_COUNT = 0, SEL_WRITE = 1, SEL_DIAG = 2 };
int launch_select_gcta(hipStream_t st, const PanelGeom &g, const double *num, const uint32_t *miss, const uint32_t *miss_diag,
                       const unsigned long long *d_nlocus, const double *colterm, const double *uvterm, const SelectArgs &s, SelPass pass,
                       double *diag);
int launch_select_cov(hipStream_t st, const PanelGeom &g, const double *num, double scale, const SelectArgs &s, SelPass pass, double *diag);
int launch_select_eigmix(hipStream_t st, const PanelGeom &g, const double *num, const double *dd, const uint32_t *het, const double *dmiss,
                         const double *dsq, const double *d_sumden, int diagadj, double scale, const SelectArgs &s, SelPass pass, double *diag);
int launch_select_beta(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int mode, double avg, double mn, const SelectArgs &s,
                       SelPass pass, double *diag);
int launch_mirror_diag_tiles(hipStream_t st, const PanelGeom &g, double *num, int T);

// context-level pieces shared between the ctx_*.hip files, eigen.hip and multi.hip
int ctx_settle(snpgpu_ctx *c);                                   // pending column / row terms of the fp16 SYRK -> panel (ctx_results.hip)
int ctx_panel_matmul_enqueue(snpgpu_ctx *c, double scale, const double *Q, int m, double *Y, bool fp32_products = false);   // no host synchronisation
// what every result call starts with (ctx_results.hip): the context is of kind_a or kind_b, a full matrix comes from a full context,
// the pending terms are in the panel (`settle`: the column / row terms too), the context's device is current; `fn`: the public name
int check_out(snpgpu_ctx *c, int kind_a, int kind_b, int packed, const char *fn, bool settle = true);
int finish(snpgpu_ctx *c);                                       // waits for the context's stream
// KING-robust family codes [N] of the caller in the context's `family` buffer: *dfam, nullptr without codes
int upload_family(snpgpu_ctx *c, const int32_t *family, const int32_t **dfam);
// what the KING-homo values take beside the counters and the fp64 sums (launch_fin_king_homo, launch_select_king_homo)
struct HomoTerms { double fscale; const double *w_const, *msum; const uint32_t *called, *nosh; };
HomoTerms homo_terms(snpgpu_ctx *c);
// the refusals of a selection that need neither a context nor a device (ctx_select.hip); `fn`: the public name
int select_check_opts(const char *fn, const snpgpu_sel_opts *o, int64_t capacity, const void *const *outs, int n_outs);
int select_grm_check_opts(const char *fn, const snpgpu_grm_sel_opts *o, int64_t capacity, const void *const *outs, int n_outs);
// the context kind a GRM selection's `what` accumulates on
inline int select_grm_kind(int what)
{
    return what == SNPGPU_SEL_GRM_GCTA ? SNPGPU_GRM_GCTA : what == SNPGPU_SEL_GRM_EIGENSTRAT ? SNPGPU_PCA_COV : what == SNPGPU_SEL_GRM_EIGMIX ? SNPGPU_EIGMIX
                                                                                                                                         : SNPGPU_INDIV_BETA;
}
// individual beta (ctx_results.hip): the minimum of all raw values and the mean of the off-diagonal ones (launch_beta_reduce), as
// snpgpu_indiv_beta(mode) takes them; `fn`: the public name
int beta_terms(snpgpu_ctx *c, int mode, double *avg, double *mn, const char *fn);

struct DevBuf {            // owns its device memory: released with the object, movable, not copyable
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int alloc(size_t n)
    {
        if (n == 0) n = 16;
        SNPGPU_HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// output staging: finalisers write device buffers; host destinations go through a temporary
struct OutBuf {
    hipStream_t st;
    void *user;
    void *dev = nullptr;
    size_t bytes;
    int mem;
    bool temp = false;
    OutBuf(hipStream_t st_, void *user_, size_t bytes_, int mem_) : st(st_), user(user_), bytes(bytes_), mem(mem_) {}
    int prepare()
    {
        if (mem == SNPGPU_DEVICE) { dev = user; return 0; }
        SNPGPU_HIP_CHECK(hipMalloc(&dev, bytes ? bytes : 16));
        temp = true;
        return 0;
    }
    int commit()
    {
        if (temp) SNPGPU_HIP_CHECK(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, st));
        return 0;
    }
    ~OutBuf()
    {
        if (temp && dev) {
            (void)hipStreamSynchronize(st);
            (void)hipFree(dev);
        }
    }
};

// The one sequence of every result, after its check_out: the temporaries in the order of `outs`, ONE launch (launch() returns
// nonzero with the error set), the copies to the host in that order, one wait for the stream.  The temporaries go with the OutBufs.
template <class Launch> int stage_out(snpgpu_ctx *c, const std::vector<OutBuf *> &outs, Launch &&launch)
{
    for (OutBuf *b : outs) if (b->prepare()) return 1;
    if (launch()) return 1;
    for (OutBuf *b : outs) if (b->commit()) return 1;
    return finish(c);
}

}  // namespace snpgpu

struct snpgpu_proj {       // PCA projector (proj.hip)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t N = 0, RB = 0, ncols_pad = 0, Bmax = 0, n_pad = 0;
    int k = 0, kp = 0;
    bool have_eig = false;
    int64_t staged_snps = 0;   // SNPs of the block currently held in `packed` (0: none)
    bool staged_words = false; // ... and whether w2 holds its sample-major words
    snpgpu::DevBuf raw, packed, sum, num, w2, et, eig_in, out, part, cnt, avg, scale, sl, af, sc, acc, flag;
};
