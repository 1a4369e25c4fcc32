// The single-product SYRK of GRM / PCA blocks without missing calls (and KING-homo's / EIGMIX's weight sums), three generations:
//
//  syrk_uv_kernel        centred / scaled genotype outer products on fp16 MFMAs, ONE product per SNP: integer-centred
//      genotypes x the two fp16 factors of the SNP weight, one wave per SIMD (default for GRM / PCA blocks WITHOUT missing
//      calls; with syrk_x1_kernel it replaces CProdMat_AlgArith::MulAdd src/genPCA.cpp:229-312 and the TransposeGenotype /
//      GenoSub / GenoMul preparation src/genPCA.h:93-108, genPCA.cpp:315-368)
//  syrk_uv16_kernel      the same arithmetic on v_mfma_f32_16x16x32_f16 (SNPGPU_SYRK_UV16=1; KING-homo and EIGMIX run on it)
//  syrk_uv16c_kernel     the same with the operands converted instead of looked up, the runs of a tile walked inside (the headline
//      kernel: default for GRM / PCA)
#include <algorithm>
#include "snpgpu_internal.h"
#include "syrk_device.h"

namespace snpgpu {

// ---------------------------------------------------------------------------
// syrk_uv_kernel: ONE fp16 product per SNP for blocks without missing calls.  The per-SNP weight y^2 = 1 / (p (1 - p)) is
// factorised as u v with u, v BOTH fp16 (uv_factor_kernel searches the 1024 mantissas of u for the one whose quotient rounds
// best: |u v / y^2 - 1| ~ 1e-6 rms, <= 4.2e-6) and the genotypes are centred at INTEGERS c_a, c_b in {0, 1, 2}:
//     row operand  (g_i - c_a) u   and   column operand  (g_j - c_b) v   are exact fp16 numbers (+-u, +-2u, 0),
// their products exact in fp32, and      u v (g_i - avg)(g_j - avg)
//     = [(g_i - c_a) u] [(g_j - c_b) v]  -  d_b u v (g_i - c_a)  -  d_a u v (g_j - c_b)  +  d_a d_b u v,   d = avg - c,
// where the last three terms are a per-row sum, a per-column sum and a constant (uvcorr_kernel, fp64; settled with the
// column term of the exact-row kernel).  The centres are picked per SNP so that the running mean of the products,
// sum d_a d_b u v, stays near zero (c_a = c_b = nearest integer gives + d^2, nearest / other neighbour gives - |d_a d_b|):
// the fp32 accumulators then carry a centred random walk as with exactly centred operands.
// Same skeleton as syrk_x1_kernel (one wave per SIMD, 4 x 4 accumulators in AGPRs, two operand sets, lookups of group g + 1
// behind the MFMAs of group g) with 8-byte table entries {row pair, column pair} (banks 2 c, 2 c + 1: conflict-free
// ds_read_b32), 16 MFMAs and 32 lookups per 16-SNP group, table chunks of 1024 SNPs (2 x 64 KiB) and two banks of EIGHT
// word sets: the groups take half the time, so the word loads run twice as many groups ahead.
// (the lookup macros index operand arrays in BOTH arms of a constant conditional; inside a template clang warns about the arm that
// is never evaluated)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Warray-bounds"
__global__ __launch_bounds__(256, 1) void syrk_uv_kernel(
    const uint32_t *__restrict__ w8, int64_t ncols_pad, const uint2 *__restrict__ lut, int n_q,
    double *__restrict__ acc, int64_t ld, int64_t tiles_c, const int4 *__restrict__ work,
    const unsigned long long *__restrict__ d_missing, int64_t n_rows_real, int chunk_lo, int chunk_hi, double fscale,
    int n_runs, int run_chunks, int n_target, int run_group, int n_items8, int run_if_missing, int64_t copy_lut_bytes,
    int64_t copy_acc_elems)
{
    // GRM / PCA: blocks WITHOUT missing calls (the others take syrk_x1_kernel).  run_if_missing: KING-homo's both-missing weight
    // sums (binary operands x the two fp16 factors of the weight, homo_uv_tables_kernel) -- blocks WITH missing calls only
    if ((*d_missing != 0ull) != (run_if_missing != 0)) return;
    constexpr int TM = 4, TN = 4, D = 8;
    constexpr int CHS = UV_CHS;                    // SNPs per table chunk
    constexpr int PST = 128;                       // bytes of table per SNP pair: 16 entries of 8 bytes
    constexpr int CHE = (CHS / 2) * PST / 8;       // 8-byte units per chunk: 64 KiB
    constexpr int QCH = CHS / 16;                  // 16-SNP groups per chunk
    static_assert(QCH % (2 * D) == 0, "whole double rounds of the word banks per chunk");
    __shared__ uint2 slut[2][CHE];

    // n_runs > 1: ONE launch for all fp32 runs of the block, work items = (tile, run) with the run index fastest inside an
    // XCD's queue (workgroup b: XCD b & 7, position b >> 3 = item * n_runs + run) -- the runs of a tile execute side by side
    // on one XCD and their fp64 flushes meet the tile's 512 KB in the Infinity Cache instead of sweeping the whole panel
    // through HBM once per run (round 5).  chunk_lo / chunk_hi / fscale then come from the run index.
    int wi = blockIdx.x;
    if (n_runs > 1) {
        const FusedItem f = fused_item(n_runs, run_group, n_items8);
        if (!f.valid) return;
        wi = f.wi;
        chunk_lo = f.run * run_chunks;
        chunk_hi = (chunk_lo + run_chunks < chunk_hi) ? (chunk_lo + run_chunks) : chunk_hi;
        fscale = (n_target > 1) ? uv_run_factor(f.run % n_target) : 1.0;
    }
    int4 item = work[wi];
    if (item.w == 0) return;
    {
        // work lists with several copies of every tile (worklist.h: build_worklist, `copies`): the copy index picks its own tables and plane
        // (written out here and in syrk_uv16_kernel: as a shared function it changes the code of both)
        const int copy = item.w >> 16;
        item.w &= 0xFFFF;
        lut = reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(lut) + (int64_t)copy * copy_lut_bytes);
        acc += (int64_t)copy * copy_acc_elems;
    }
    const auto [c_beg, c_end] = k_part(chunk_lo, chunk_hi, item.z, item.w);
    if (c_beg >= c_end) return;

    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int64_t row_w = (int64_t)item.x * X1_TILE + wr * (32 * TM), col_w = (int64_t)item.y * X1_TILE + wc * (32 * TN);
    const uint32_t *__restrict__ pa = w8 + (int64_t)kh * ncols_pad + row_w + li;
    const uint32_t *__restrict__ pb = w8 + (int64_t)kh * ncols_pad + col_w + li;
    double *__restrict__ pacc = acc + acc_off(ld, tiles_c, row_w + 4 * kh, col_w + li);
    const int64_t rs = tiles_c ? ACC_TILE : ld;    // row stride inside this wave's part of the accumulator

    f32x16 c32[TM][TN];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) c32[i][j][r] = 0.f;

    u32x4 Av[2][TM], Bv[2][TN];                    // two operand sets: MFMAs read one, the lookups fill the other
    uint32_t W0a[D][TM], W0b[D][TN], W1a[D][TM], W1b[D][TN];   // two banks of eight word sets

    // lookup L (0..31) of a group, in the order the MFMAs (row-major over the 4 x 4 tiles) first need the operands:
    // A0, B0, B1, B2, B3, A1, A2, A3 -- four dwords (SNP pairs) each
#define UV_ISROW(L) ((((L) >> 2) == 0) || (((L) >> 2) >= 5))
#define UV_RI(L) ((((L) >> 2) >= 5) ? ((L) >> 2) - 4 : 0)
#define UV_CI(L) (((((L) >> 2) >= 1) && (((L) >> 2) <= 4)) ? ((L) >> 2) - 1 : 0)
#define UV_AD(LA_, LB_, NS_, L, tb)                                                                        \
    (UV_ISROW(L) ? (tb) + ((LA_[NS_][UV_RI(L)] >> (8 * ((L) & 3))) & 0xFFu)                                \
                 : (tb) + ((LB_[NS_][UV_CI(L)] >> (8 * ((L) & 3))) & 0xFFu))
#define UV_RD(T_, L, a)                                                                                    \
    do {                                                                                                   \
        if (UV_ISROW(L)) Av[T_][UV_RI(L)][(L) & 3] = x1_lds32((a) + PST * ((L) & 3));                       \
        else Bv[T_][UV_CI(L)][(L) & 3] = x1_lds32((a) + PST * ((L) & 3) + 4);                               \
    } while (0)
#define UV_TABLE_ASYNC(chunk, buf)                                                                             \
    do {                                                                                                       \
        const char *src_ = reinterpret_cast<const char *>(lut) + (int64_t)(chunk) * (CHE * 8) + wave * (CHE * 2) + lane * 16; \
        char *dst_ = reinterpret_cast<char *>(&slut[buf][0]) + wave * (CHE * 2);                              \
        _Pragma("unroll") for (int t_ = 0; t_ < CHE * 2 / 1024; t_++)                                          \
            x1_lds_dma16(src_ + 1024 * t_, x1_lds_off(dst_ + 1024 * t_));                                      \
    } while (0)
    // word load number m (0..63) of a round: set m >> 3, sample group m & 7 (four row groups, four column groups)
#define UV_LOAD(YA_, YB_, g_first, m)                                                         \
    do {                                                                                      \
        const int64_t off_ = (int64_t)((g_first) + ((m) >> 3)) * 2 * ncols_pad;               \
        if (((m) & 7) < TM) YA_[(m) >> 3][((m) & 7) < TM ? ((m) & 7) : 0] = pa[off_ + 32 * ((m) & 7)]; \
        else YB_[(m) >> 3][((m) & 7) >= TM ? ((m) & 7) - TM : 0] = pb[off_ + 32 * (((m) & 7) - TM)];  \
    } while (0)
    // one group: 16 MFMAs out of operand set S_; behind each, two lookups of the NEXT group (word set NS_ of bank LA_ / LB_,
    // into operand set T_), their addresses computed one slot earlier.  LOAD_ 1 / 2: behind every MFMA two word loads of
    // the next round (bank YA_ / YB_), numbers 2 m, 2 m + 1 (+ 32 for LOAD_ == 2): all 64 go out during the first two
    // groups of a round and are first looked up in its last one.
#define UV_STEP(m, S_, T_, LA_, LB_, NS_, LOAD_, YA_, YB_, g_load, tb)                                              \
    do {                                                                                                            \
        c32[(m) >> 2][(m) & 3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(                                             \
            (f16x8)Av[S_][(m) >> 2], (f16x8)Bv[S_][(m) & 3], c32[(m) >> 2][(m) & 3], 0, 0, 0);                       \
        UV_RD(T_, 2 * (m), a0_); UV_RD(T_, 2 * (m) + 1, a1_);                                                        \
        if ((m) < 15) { a0_ = UV_AD(LA_, LB_, NS_, 2 * (m) + 2, tb); a1_ = UV_AD(LA_, LB_, NS_, 2 * (m) + 3, tb);    \
                        asm volatile("" : "+v"(a0_), "+v"(a1_)); }   /* pins the additions HERE, not next to their reads */ \
        if (LOAD_) { UV_LOAD(YA_, YB_, g_load, 2 * (m) + 32 * ((LOAD_) - 1)); UV_LOAD(YA_, YB_, g_load, 2 * (m) + 1 + 32 * ((LOAD_) - 1)); } \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
    } while (0)
#define UV_STEP4(m, ...) UV_STEP(m, __VA_ARGS__); UV_STEP((m) + 1, __VA_ARGS__); UV_STEP((m) + 2, __VA_ARGS__); UV_STEP((m) + 3, __VA_ARGS__)
#define UV_GROUP_ADDR0(S_, T_, LA_, LB_, NS_, LOAD_, YA_, YB_, g_load, tb)                                           \
    uint32_t a0_ = UV_AD(LA_, LB_, NS_, 0, tb), a1_ = UV_AD(LA_, LB_, NS_, 1, tb)
#define UV_GROUP(...)                                                                                               \
    do {                                                                                                            \
        UV_GROUP_ADDR0(__VA_ARGS__);                                                                                \
        UV_STEP4(0, __VA_ARGS__); UV_STEP4(4, __VA_ARGS__); UV_STEP4(8, __VA_ARGS__); UV_STEP4(12, __VA_ARGS__);    \
    } while (0)

    // prologue: table of the first chunk, the words of the first round, the lookups of group 0
    UV_TABLE_ASYNC(c_beg, c_beg & 1);
#define UV_L8(m) UV_LOAD(W0a, W0b, c_beg * QCH, m); UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 1); UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 2); UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 3); \
                 UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 4); UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 5); UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 6); UV_LOAD(W0a, W0b, c_beg * QCH, (m) + 7)
    UV_L8(0); UV_L8(8); UV_L8(16); UV_L8(24); UV_L8(32); UV_L8(40); UV_L8(48); UV_L8(56);
#undef UV_L8
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();
    uint32_t tbn = x1_lds_off(&slut[c_beg & 1][0]) + 4 * PST * kh;
    {
        uint32_t a0_, a1_;
#define UV_LK2(L) a0_ = UV_AD(W0a, W0b, 0, L, tbn); a1_ = UV_AD(W0a, W0b, 0, (L) + 1, tbn); UV_RD(0, L, a0_); UV_RD(0, (L) + 1, a1_)
#define UV_LK8(L) UV_LK2(L); UV_LK2((L) + 2); UV_LK2((L) + 4); UV_LK2((L) + 6)
        UV_LK8(0); UV_LK8(8); UV_LK8(16); UV_LK8(24);
#undef UV_LK8
#undef UV_LK2
    }
    tbn += 8 * PST;

    for (int c = c_beg; c < c_end; c++) {
        const int cur = c & 1;
        const int q0 = c * QCH;
        const int q_cnt = (q0 + QCH <= n_q) ? QCH : (n_q - q0);      // multiple of 16 (blocks are padded to 256 SNPs)
        const bool more = (c + 1 < c_end);
        if (more) UV_TABLE_ASYNC(c + 1, cur ^ 1);   // every wave is past the barrier that freed this buffer
        for (int q = 0; q < q_cnt; q += 2 * D) {
            const int g = q0 + q;
            // round A: words of bank 0, loads into bank 1
            UV_GROUP(0, 1, W0a, W0b, 1, 1, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W0a, W0b, 2, 2, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(0, 1, W0a, W0b, 3, 0, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W0a, W0b, 4, 0, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(0, 1, W0a, W0b, 5, 0, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W0a, W0b, 6, 0, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(0, 1, W0a, W0b, 7, 0, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W1a, W1b, 0, 0, W1a, W1b, g + 8, tbn); tbn += 8 * PST;
            // round B: words of bank 1, loads into bank 0
            UV_GROUP(0, 1, W1a, W1b, 1, 1, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W1a, W1b, 2, 2, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            UV_GROUP(0, 1, W1a, W1b, 3, 0, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W1a, W1b, 4, 0, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            UV_GROUP(0, 1, W1a, W1b, 5, 0, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            UV_GROUP(1, 0, W1a, W1b, 6, 0, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            UV_GROUP(0, 1, W1a, W1b, 7, 0, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
            // the chunk's last group looks up the NEXT chunk's table (or, at the very end, harmlessly re-reads this one);
            // one straight-line body, as in syrk_x1_kernel
            if (q + 2 * D >= q_cnt) {
                if (more) {
                    // vmcnt is in-order: the table copy went out at the start of this (full) chunk, behind it eight rounds of
                    // 64 word loads, the last of them seven groups ago -- all but the newest 62 requests covers it (63 is
                    // the counter's ceiling and waits for nothing)
                    __builtin_amdgcn_s_waitcnt(0xCF7E); // vmcnt(62)
                    __syncthreads();
                    tbn = x1_lds_off(&slut[cur ^ 1][0]) + 4 * PST * kh;
                } else {
                    tbn = x1_lds_off(&slut[cur][0]) + 4 * PST * kh;
                }
            }
            UV_GROUP(1, 0, W0a, W0b, 0, 0, W0a, W0b, g + 16, tbn); tbn += 8 * PST;
        }
    }
    flush_tiles32<true>(pacc, rs, flush_rows_left(n_rows_real, row_w + 4 * kh), c32, fscale);
#undef UV_GROUP
#undef UV_GROUP_ADDR0
#undef UV_STEP4
#undef UV_STEP
#undef UV_LOAD
#undef UV_TABLE_ASYNC
#undef UV_RD
#undef UV_AD
#undef UV_CI
#undef UV_RI
#undef UV_ISROW
}
#pragma clang diagnostic pop

// ---------------------------------------------------------------------------
// syrk_uv16_kernel (round 6): syrk_uv_kernel's arithmetic -- the same tables, words, work list, fp32 runs and fp64 flush -- on
// v_mfma_f32_16x16x32_f16.  Why: the kernel runs against the socket power cap, and what a matrix instruction costs in power is
// dominated by its accumulator traffic.  32x32x16 reads and writes 16 accumulator registers per lane for 32 768 flops, 16x16x32 four
// for 16 384: half the traffic per flop.  A register-only stream with this kernel's operand classes sustains 2100 TFLOP/s through
// 16x16x32 against 1790 through 32x32x16 on the same box (snpgpu_diag_mfma_rate, profiles/r06_probe_shapes.txt); results are
// bit-identical (the same products summed in the same order: tools/ubench/r06_kloop_ubench.hip -- so the hoped-for "one rounding
// per 32 SNPs" does not exist, the power does).
// A wave's 128 x 128 tile is 8 x 8 sub-tiles of 16 x 16 (64 x 4 = the same 256 AGPRs).  Lane l: sample l & 15 of a sub-tile, SNP
// quarter l >> 4 of a 32-SNP group = word row 4 G + (l >> 4).  Per group: 64 MFMAs, 64 lookups (one behind every MFMA), 16 words.
// Registers: sixteen 4-dword operands per group would need 128 VGPRs double-buffered; the ROW operands are therefore refilled
// in place -- row r of the 8 x 8 MFMA order is the last reader of row operand r, so row operand r - 1 of the NEXT group is looked up
// behind the MFMAs of row r (operand 7 behind row 0 of the group that uses it) -- and only the column operands have two sets:
// 96 VGPRs of operands + a ring of four word sets (64): the words of group g + 4 are requested behind the first 16 MFMAs of group g,
// into the set group g has just finished with (its one remaining use, the word of row operand 7, is copied out first), and are
// first looked up in group g + 3.
// LDS banks: a 32-lane pass of a lookup now spans TWO quarters, i.e. two pair tables with the same bank mapping (entry c of
// every table sits in banks 2 c, 2 c + 1).  The table builders therefore swap the halves of the entries of odd quarters
// ({column pair, row pair}; uv_tables_kernel / homo_uv_tables_kernel, `swap_odd`): a row lookup reads bank 2 c in even quarters
// and 2 c + 1 in odd ones, a column lookup the other way round -- conflict-free again.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Warray-bounds"
__global__ __launch_bounds__(256, 1) void syrk_uv16_kernel(
    const uint32_t *__restrict__ w8, int64_t ncols_pad, const uint2 *__restrict__ lut, int n_q,
    double *__restrict__ acc, int64_t ld, int64_t tiles_c, const int4 *__restrict__ work,
    const unsigned long long *__restrict__ d_missing, int64_t n_rows_real, int chunk_lo, int chunk_hi, double fscale,
    int n_runs, int run_chunks, int n_target, int run_group, int n_items8, int run_if_missing, int64_t copy_lut_bytes,
    int64_t copy_acc_elems)
{
    if ((*d_missing != 0ull) != (run_if_missing != 0)) return;
    constexpr int TS = 8, D = 4;
    constexpr int CHS = UV_CHS;                    // SNPs per table chunk
    constexpr int PST = 128;                       // bytes of table per SNP pair: 16 entries of 8 bytes
    constexpr int CHE = (CHS / 2) * PST / 8;       // 8-byte units per chunk: 64 KiB
    constexpr int GCH = CHS / 32;                  // 32-SNP groups per chunk
    constexpr int GST = 16 * PST;                  // bytes of table per group
    static_assert(GCH % (2 * D) == 0, "whole double rounds of the word banks per chunk");
    __shared__ uint2 slut[2][CHE];

    int wi = blockIdx.x;
    if (n_runs > 1) {                              // fused (tile, run) launch: see syrk_uv_kernel
        const FusedItem f = fused_item(n_runs, run_group, n_items8);
        if (!f.valid) return;
        wi = f.wi;
        chunk_lo = f.run * run_chunks;
        chunk_hi = (chunk_lo + run_chunks < chunk_hi) ? (chunk_lo + run_chunks) : chunk_hi;
        fscale = (n_target > 1) ? uv_run_factor(f.run % n_target) : 1.0;
    }
    int4 item = work[wi];
    if (item.w == 0) return;
    {
        const int copy = item.w >> 16;
        item.w &= 0xFFFF;
        lut = reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(lut) + (int64_t)copy * copy_lut_bytes);
        acc += (int64_t)copy * copy_acc_elems;
    }
    const auto [c_beg, c_end] = k_part(chunk_lo, chunk_hi, item.z, item.w);
    if (c_beg >= c_end) return;

    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int64_t row_w = (int64_t)item.x * X1_TILE + wr * (16 * TS), col_w = (int64_t)item.y * X1_TILE + wc * (16 * TS);
    // word loads: uniform row base (SGPRs, per group) + a 32-bit lane offset + an immediate -- no address arithmetic on the VALU
    const int la = (int)((int64_t)kq * ncols_pad + row_w + l16), lb = (int)((int64_t)kq * ncols_pad + col_w + l16);
    double *__restrict__ pacc = acc + acc_off(ld, tiles_c, row_w + 4 * kq, col_w + l16);
    const int64_t rs = tiles_c ? ACC_TILE : ld;

    f32x4 c16[TS][TS];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) c16[i][j][r] = 0.f;

    u32x4 Av[TS], Bv[2][TS];                       // row operands: ONE set, refilled in place; column operands: two sets
    uint32_t Wa[D][TS], Wb[D][TS];                 // ring of four word sets (8 row + 8 column words each): group g lives in set g & 3
    uint32_t wa7;                                  // this group's word of row operand 7 (its set is being refilled for group g + 4)
    uint32_t tc_row, tn_row, tn_col;               // table positions: this group's (row half), the next group's (row / column half)

    // lookup L (0..63) of a group, issued behind MFMA L (row r = L >> 3 of the 8 x 8 order, t = L & 7):
    //   t < 4:  dword t of row operand (r == 0 ? 7 of THIS group : r - 1 of the NEXT group)
    //   t >= 4: dword t - 4 of column operand r of the next group (set T_)
#define U16_R(L) ((L) >> 3)
#define U16_ISA(L) (((L) & 7) < 4)
#define U16_AI(L) (U16_R(L) == 0 ? 7 : U16_R(L) - 1)
#define U16_D(L) ((L) & 3)
#define U16_AD(NS_, L)                                                                                       \
    (U16_ISA(L) ? (U16_R(L) == 0 ? tc_row + ((wa7 >> (8 * U16_D(L))) & 0xFFu)                                 \
                                 : tn_row + ((Wa[NS_][U16_AI(L)] >> (8 * U16_D(L))) & 0xFFu))                 \
                : tn_col + ((Wb[NS_][U16_R(L)] >> (8 * U16_D(L))) & 0xFFu))
#define U16_RD(T_, L, a)                                                                                     \
    do {                                                                                                     \
        if (U16_ISA(L)) Av[U16_AI(L)][U16_D(L)] = x1_lds32((a) + PST * U16_D(L));                             \
        else Bv[T_][U16_R(L)][U16_D(L)] = x1_lds32((a) + PST * U16_D(L));                                     \
    } while (0)
#define U16_TABLE_ASYNC(chunk, buf)                                                                            \
    do {                                                                                                       \
        const char *src_ = reinterpret_cast<const char *>(lut) + (int64_t)(chunk) * (CHE * 8) + wave * (CHE * 2) + lane * 16; \
        char *dst_ = reinterpret_cast<char *>(&slut[buf][0]) + wave * (CHE * 2);                              \
        _Pragma("unroll") for (int t_ = 0; t_ < CHE * 2 / 1024; t_++)                                          \
            x1_lds_dma16(src_ + 1024 * t_, x1_lds_off(dst_ + 1024 * t_));                                      \
    } while (0)
    // word load number m (0..15) of a group into set CS_: eight row sub-tiles, eight column sub-tiles
#define U16_LOAD(CS_, g_abs, m)                                                               \
    do {                                                                                      \
        const uint32_t *__restrict__ bs_ = w8 + (int64_t)(g_abs) * 4 * ncols_pad;              \
        if ((m) < TS) Wa[CS_][(m) < TS ? (m) : 0] = bs_[la + 16 * (m)];                        \
        else Wb[CS_][(m) >= TS ? (m) - TS : 0] = bs_[lb + 16 * ((m) - TS)];                    \
    } while (0)
#define U16_MFMA(m, S_)                                                                                             \
        c16[(m) >> 3][(m) & 7] = __builtin_amdgcn_mfma_f32_16x16x32_f16(                                             \
            (f16x8)Av[(m) >> 3], (f16x8)Bv[S_][(m) & 7], c16[(m) >> 3][(m) & 7], 0, 0, 0)
    // Issue pattern (measured, profiles/r06_uv16_patterns.txt; ms per 65 536-SNP step at N = 100 000 on one box, the 32x32x16 kernel 456):
    // one lookup + one address op behind every MFMA 489; MFMAs in runs of 4 / 8 with their lookups behind 486 / 540; exactly TWO
    // companions of ONE kind behind every MFMA -- [M dd][M aa] 430, [M aa][M dd] a little better again: a lone wave pays for every
    // switch between the matrix pipe, the LDS and the VALU, and a 16-clock MFMA hides two instructions, not three.  The addresses of
    // a batch of four lookups are computed one batch ahead into the other half of eight address registers.
#define U16_SB() __builtin_amdgcn_sched_barrier(0)
#define U16_M(m, S_) do { U16_MFMA(m, S_); U16_SB(); } while (0)
#define U16_A2(NS_, m, k)      /* addresses of lookups m + 4 + k, + 1 (the NEXT batch) into the other register half */              \
    do {                                                                                                                            \
        if ((m) + 4 + (k) < 64) {                                                                                                   \
            a_[4 * ((((m) >> 2) + 1) & 1) + (k)] = U16_AD(NS_, ((m) + 4 + (k)) & 63);                                               \
            a_[4 * ((((m) >> 2) + 1) & 1) + (k) + 1] = U16_AD(NS_, ((m) + 5 + (k)) & 63);                                           \
            asm volatile("" : "+v"(a_[4 * ((((m) >> 2) + 1) & 1) + (k)]), "+v"(a_[4 * ((((m) >> 2) + 1) & 1) + (k) + 1]));           \
        }                                                                                                                           \
        U16_SB();                                                                                                                   \
    } while (0)
#define U16_D2(T_, m, k)       /* lookups m + k, + 1 of THIS batch */                                                               \
    do {                                                                                                                            \
        U16_RD(T_, (m) + (k), a_[4 * (((m) >> 2) & 1) + (k)]); U16_RD(T_, (m) + (k) + 1, a_[4 * (((m) >> 2) & 1) + (k) + 1]);        \
        U16_SB();                                                                                                                   \
    } while (0)
#define U16_STEP4(m, S_, T_, CS_, NS_, g_abs)                                                                       \
    do {                                                                                                            \
        U16_M(m, S_);       U16_A2(NS_, m, 0);                                                                      \
        U16_M((m) + 1, S_); U16_D2(T_, m, 0);                                                                       \
        U16_M((m) + 2, S_); U16_A2(NS_, m, 2);                                                                      \
        U16_M((m) + 3, S_); U16_D2(T_, m, 2);                                                                       \
        if ((m) < 16) {     /* the words of group g + 4 into this group's set, four behind each of the first four batches */ \
            U16_LOAD(CS_, (g_abs) + D, m); U16_LOAD(CS_, (g_abs) + D, (m) + 1); U16_LOAD(CS_, (g_abs) + D, (m) + 2); U16_LOAD(CS_, (g_abs) + D, (m) + 3); \
            U16_SB();                                                                                               \
        }                                                                                                           \
    } while (0)
#define U16_STEP8(m, ...) U16_STEP4(m, __VA_ARGS__); U16_STEP4((m) + 4, __VA_ARGS__)
    // one 32-SNP group (absolute index g_abs, word set CS_ = g_abs & 3, the next group's NS_); afterwards the table positions move on
#define U16_GROUP(S_, T_, CS_, NS_, g_abs)                                                                          \
    do {                                                                                                            \
        wa7 = Wa[CS_][7];                                                                                           \
        asm volatile("" : "+v"(wa7));                                                                               \
        uint32_t a_[8];                                                                                             \
        a_[0] = U16_AD(NS_, 0); a_[1] = U16_AD(NS_, 1); a_[2] = U16_AD(NS_, 2); a_[3] = U16_AD(NS_, 3);             \
        U16_STEP8(0, S_, T_, CS_, NS_, g_abs);  U16_STEP8(8, S_, T_, CS_, NS_, g_abs);                               \
        U16_STEP8(16, S_, T_, CS_, NS_, g_abs); U16_STEP8(24, S_, T_, CS_, NS_, g_abs);                              \
        U16_STEP8(32, S_, T_, CS_, NS_, g_abs); U16_STEP8(40, S_, T_, CS_, NS_, g_abs);                              \
        U16_STEP8(48, S_, T_, CS_, NS_, g_abs); U16_STEP8(56, S_, T_, CS_, NS_, g_abs);                              \
        tc_row = tn_row; tn_row += GST; tn_col += GST;                                                              \
    } while (0)

    // prologue: table of the first chunk, the words of the first four groups, the lookups of group 0 (row operand 7 comes with row 0)
    U16_TABLE_ASYNC(c_beg, c_beg & 1);
#define U16_L16(S) U16_LOAD(S, c_beg * GCH + S, 0); U16_LOAD(S, c_beg * GCH + S, 1); U16_LOAD(S, c_beg * GCH + S, 2); U16_LOAD(S, c_beg * GCH + S, 3);     \
                   U16_LOAD(S, c_beg * GCH + S, 4); U16_LOAD(S, c_beg * GCH + S, 5); U16_LOAD(S, c_beg * GCH + S, 6); U16_LOAD(S, c_beg * GCH + S, 7);     \
                   U16_LOAD(S, c_beg * GCH + S, 8); U16_LOAD(S, c_beg * GCH + S, 9); U16_LOAD(S, c_beg * GCH + S, 10); U16_LOAD(S, c_beg * GCH + S, 11);   \
                   U16_LOAD(S, c_beg * GCH + S, 12); U16_LOAD(S, c_beg * GCH + S, 13); U16_LOAD(S, c_beg * GCH + S, 14); U16_LOAD(S, c_beg * GCH + S, 15)
    U16_L16(0); U16_L16(1); U16_L16(2); U16_L16(3);
#undef U16_L16
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();
    {
        // odd quarters read the row half of an entry at + 4 and the column half at + 0 (swapped entries, see the header)
        const uint32_t base = x1_lds_off(&slut[c_beg & 1][0]) + 4 * PST * kq;
        tn_row = base + 4 * (kq & 1);
        tn_col = base + 4 - 4 * (kq & 1);
        tc_row = tn_row;
    }
    {
        uint32_t a_;
        // group 0: row operands 0..6 and the eight column operands (set 0) from word set 0
#define U16_PA(i, d) a_ = tn_row + ((Wa[0][i] >> (8 * (d))) & 0xFFu); Av[i][d] = x1_lds32(a_ + PST * (d))
#define U16_PB(j, d) a_ = tn_col + ((Wb[0][j] >> (8 * (d))) & 0xFFu); Bv[0][j][d] = x1_lds32(a_ + PST * (d))
#define U16_P4(M, i) M(i, 0); M(i, 1); M(i, 2); M(i, 3)
        U16_P4(U16_PA, 0); U16_P4(U16_PA, 1); U16_P4(U16_PA, 2); U16_P4(U16_PA, 3); U16_P4(U16_PA, 4); U16_P4(U16_PA, 5); U16_P4(U16_PA, 6);
        U16_P4(U16_PB, 0); U16_P4(U16_PB, 1); U16_P4(U16_PB, 2); U16_P4(U16_PB, 3); U16_P4(U16_PB, 4); U16_P4(U16_PB, 5); U16_P4(U16_PB, 6); U16_P4(U16_PB, 7);
#undef U16_P4
#undef U16_PB
#undef U16_PA
    }
    tn_row += GST; tn_col += GST;                  // (tc_row stays on group 0: its row operand 7 is looked up behind row 0)

    for (int c = c_beg; c < c_end; c++) {
        const int cur = c & 1;
        const int q_cnt = (c * (CHS / 16) + CHS / 16 <= n_q) ? GCH : (n_q - c * (CHS / 16)) / 2;   // 32-SNP groups: a multiple of 8
        const bool more = (c + 1 < c_end);
        if (more) U16_TABLE_ASYNC(c + 1, cur ^ 1);  // every wave is past the barrier that freed this buffer
        for (int q = 0; q < q_cnt; q += 2 * D) {
            const int g = c * GCH + q;
            U16_GROUP(0, 1, 0, 1, g);
            U16_GROUP(1, 0, 1, 2, g + 1);
            U16_GROUP(0, 1, 2, 3, g + 2);
            U16_GROUP(1, 0, 3, 0, g + 3);
            U16_GROUP(0, 1, 0, 1, g + 4);
            U16_GROUP(1, 0, 1, 2, g + 5);
            U16_GROUP(0, 1, 2, 3, g + 6);
            // the chunk's last group looks up the NEXT chunk's first group (or, at the very end, harmlessly re-reads this chunk);
            // its own row operand 7 still comes from this chunk (tc_row)
            if (q + 2 * D >= q_cnt) {
                uint32_t base;
                if (more) {
                    // vmcnt is in-order: the table copy went out at the start of this (full) chunk, behind it 31 groups of 16 word
                    // loads -- all but the newest 62 requests covers it
                    __builtin_amdgcn_s_waitcnt(0xCF7E); // vmcnt(62)
                    __syncthreads();
                    base = x1_lds_off(&slut[cur ^ 1][0]) + 4 * PST * kq;
                } else {
                    base = x1_lds_off(&slut[cur][0]) + 4 * PST * kq;
                }
                tn_row = base + 4 * (kq & 1);
                tn_col = base + 4 - 4 * (kq & 1);
            }
            U16_GROUP(1, 0, 3, 0, g + 7);
        }
    }
    {
        double *pflush = flush_ptr(pacc);
        const int64_t rows_left = flush_rows_left(n_rows_real, row_w + 4 * kq);
#pragma unroll
        for (int i = 0; i < TS; i++) flush_row16(pflush, rs, rows_left, c16, i, fscale, 0, false);
    }
#undef U16_GROUP
#undef U16_STEP8
#undef U16_STEP4
#undef U16_D2
#undef U16_A2
#undef U16_M
#undef U16_SB
#undef U16_MFMA
#undef U16_LOAD
#undef U16_TABLE_ASYNC
#undef U16_RD
#undef U16_AD
#undef U16_D
#undef U16_AI
#undef U16_ISA
#undef U16_R
}
#pragma clang diagnostic pop

// ---------------------------------------------------------------------------
// syrk_uv16c_kernel (round 6, SNPGPU_SYRK_UV16=2): syrk_uv16_kernel with the operands CONVERTED instead of looked up.  The pair bytes
// of a block without missing calls hold two e2m1 nibbles c0 | c1 << 4 (value c / 2; transpose8_kernel, nibble_nomiss), ONE
// v_cvt_scalef32_pk_f16_fp4 (byte select by op_sel) turns a byte into the fp16 pair (c0 / 2, c1 / 2) and ONE v_pk_fma_f16 with the
// lane's factor pairs makes (c / 2)(2 u) - c_a u = (c - c_a) u: exact at every step, the same operand values as the tables'.  Per
// operand dword two vector ops instead of an address op + a ds_read_b32; per 32-SNP group four ds_read_b128 of factors (256 bytes per
// group: uv_tables_kernel, swap_odd == 2) instead of 64 table reads; LDS 16 KiB instead of 128.  K-loop model
// (tools/ubench/r06_kloop_ubench.hip, E against F): 20.5 against 22.6 us per 1024 SNPs of a wave tile.
// Same MFMA order, register plan (row operands refilled in place, two column sets, ring of four word sets), work list, runs, flush.
// MEASURED (configs[2], interleaved on one box, profiles/r06_uvc_ab.txt): the kernel is bound by the socket power cap, not by issue slots --
// the converted operands alone (SNPGPU_SYRK_UV16=2) need 5 % fewer cycles and run at a 5 % lower clock: 432 against 431 ms per step.  With the
// runs walked inside and 35 of a wave's 64 sub-tile sums carried in LDS (=3) the panel writes fall from 242 to 131 GB per step (32: 144).
// THE PACE-MAKER.  L2 -> fabric reads (TCC_EA0_RDREQ x 128 B; the fp64 atomics leave as EA atomic writes and fetch nothing) are all genotype
// word lines: the workgroups demand 1.28 TB of them per step from their L2s, and what they fetch depends on whether the 32 workgroups of an
// XCD stream the word rows they share IN STEP.  The lookup kernel's do (391 GB: a line serves ~3.3 workgroups, the 4 x 4 super-tiles'
// sharing); this kernel's, left alone, drift apart (727 GB, 947 GB with the runs walked inside).  What keeps the lookup kernel's in step is
// its table: every workgroup fetches the same 64 KiB per chunk; the first to arrive misses, and because vmcnt counts in order its word loads
// wait behind that fetch, while the followers' fetches hit -- the leader is held back one memory latency per chunk.  This kernel therefore
// issues the same fetch as a PACE-MAKER: 16 x 1 KiB per wave and chunk (= the table's size) from a zero-filled region common to all
// workgroups (uvpace), into an LDS slot nobody reads.  That brings the reads to 345 - 407 GB; 4 or 1 KiB per wave do nothing (1030 / 946 GB).
// With it this form takes 414 - 416 against 424 - 426 ms of kernel time per step (-2.4 %, at 2158 against 2136 MHz under the same 1370 W;
// -2.0 ... -2.8 % on a second box) and moves 489 instead of 633 GB: the default since the end of round 6 (SNPGPU_SYRK_UV16=1: the lookup
// kernel; SNPGPU_UVC_PACE=0: no pace-maker).
// THE K LOOP'S BUDGET.  One wave per SIMD pays an issue turn for EVERY instruction of its stream (about 4 clocks, an MFMA 8; a gap runs
// max(16, sum)): an MFMA hides its two companions, the conversion pair or the fma pair of an operand dword, and whatever else a 32-SNP
// group of 64 MFMAs holds is time.  What has to be there: 16 word loads, 4 factor reads, 3 waits, 2 scalar adds = 25 (tools/isa_mix.py
// counts 25.7 with the loop's own branch; tests/test_cpu_kloop_isa.py holds it below 30).  Until this budget was written down the group
// held 44: the 64-bit product (group index) x 4 ncols_pad and the base add redone for every group (12 scalar), two v_lshl_add_u64 for
// the sides' 64-bit address pairs, and a tighter vmcnt in front of nearly every first use of a word (9.7 waits).  Now a group's words are
// addressed as (uniform 64-bit base in scalar registers) + (the lane's 32-bit byte offset, one per side) + 64 m as the instruction's
// immediate; the base is made once per run in the prologue, from c_beg, and moves on by the constant 16 ncols_pad bytes behind MFMA 60,
// which has no conversions behind it; and ONE vmcnt(32) behind a group's first MFMA covers the next group's sixteen words (requested
// three groups earlier; vmcnt counts in order).  Same loads, same order, same conversions and MFMAs: results are bit-identical.
// MEASURED (profiles/kloop_diet_ab.json, bench.py alternated with the parent commit on one device): 408.5 - 409.1 against 416.8 - 418.0 ms
// per step, kernel 402.0 - 402.6 against 410.4 - 411.5 (-2.1 %); wave cycles per MFMA 21.2 against 22.2.  (SQ_WAIT_INST_ANY, a quarter
// of the wave cycles before and after, counts issue stall -- cycles in which the wave had an instruction and could not issue it -- not
// time parked at an s_waitcnt.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Warray-bounds"
__global__ __launch_bounds__(256, 1) void syrk_uv16c_kernel(
    const uint32_t *__restrict__ w8, int64_t ncols_pad, const uint2 *__restrict__ lut, int n_q,
    double *__restrict__ acc, int64_t ld, int64_t tiles_c, const int4 *__restrict__ work,
    const unsigned long long *__restrict__ d_missing, int64_t n_rows_real, int chunk_lo, int chunk_hi, double fscale,
    int n_runs, int run_chunks, int n_target, int run_group, int n_items8, int run_if_missing, const char *__restrict__ pace_src, int pace,
    f32x4 *__restrict__ carry_scr, unsigned int *__restrict__ carry_flags, int carry_slots)
{
    if ((*d_missing != 0ull) != (run_if_missing != 0)) return;
    constexpr int TS = 8, D = 4;
    constexpr int CHS = UV_CHS;                    // slots per factor chunk
    constexpr int GCH = CHS / 32;                  // 32-SNP groups per chunk
    constexpr int GST = 256;                       // bytes of factors per group: {row 2u, row -c u, column 2v, column -c v} x 4 quarters x 4 pairs
    constexpr int CHB = GCH * GST;                 // 8 KiB per chunk
    static_assert(GCH % (2 * D) == 0, "whole double rounds of the word banks per chunk");
    __shared__ u32x4 sfac[2][CHB / 16];
    // run_group == 0 with n_runs > 1 (SNPGPU_SYRK_UV16=3): a work item is a TILE and walks its fp32 runs itself.  With the tables gone
    // 144 KiB of LDS are free: the sums of CARRY_SUB of a wave's 64 sub-tiles stay there between runs as fp32 (carry += f_q x partial;
    // six additions of 24-bit numbers: 3e-7 of a run's scale against the 5e-6 of the run itself) and meet the fp64 panel ONCE per block;
    // the other sub-tiles flush after every run as before.  Half the fp64 read-modify-writes of the 40 GB panel per run go away.
    constexpr int CARRY_SUB = 35;                  // sub-tiles 0 .. 34 in (i, j) order: 35 KiB per wave = all the LDS there is (16 + 4 + 140 KiB)
    __shared__ f32x4 scar[4][CARRY_SUB * 64];
    // THE CARRY SCRATCH (carry_scr != nullptr): the other UV_CARRY_REST sub-tiles are carried the same way, their sums waiting in a SLOT of
    // device memory (116 KiB per workgroup: [wave][sub-tile - CARRY_SUB][lane] f32x4, 1 KiB contiguous per wave instruction) instead of
    // meeting the panel after every run.  After a run's K loop the operand, word and factor registers are dead: all 29 loads of a wave go
    // out first, then the LDS part, then the adds and stores -- ONE round trip per run boundary, to lines this workgroup wrote a run
    // earlier.  Slots come from a pool PER XCD (the hardware XCC id, never blockIdx): a slot is only ever read and written through one
    // L2, so no dirty line of an earlier owner in another L2 can be written back over newer sums.  One lane takes a slot with a single
    // pass of compare-and-swap over the pool's flags and frees it once every wave's last read has returned; the first run only writes,
    // so nothing is cleared between owners.  A pass that finds no free slot waits for nothing: the item flushes sub-tiles >= CARRY_SUB
    // after every run as before (the two schemes differ only in where the partial sums wait) and counts itself in carry_flags[0].
    constexpr int CARRY_REST = UV_CARRY_REST;
    static_assert(CARRY_SUB + CARRY_REST == TS * TS, "every sub-tile is carried in LDS or in the slot");
    __shared__ u32x4 space[4][64];                 // 1 KiB per wave: where the pace-maker fetches land (never read)
    const bool inner = (n_runs > 1 && run_group == 0);

    int wi = blockIdx.x;
    if (n_runs > 1 && !inner) {                    // fused (tile, run) launch: see syrk_uv_kernel
        const FusedItem f = fused_item(n_runs, run_group, n_items8);
        if (!f.valid) return;
        wi = f.wi;
        chunk_lo = f.run * run_chunks;
        chunk_hi = (chunk_lo + run_chunks < chunk_hi) ? (chunk_lo + run_chunks) : chunk_hi;
        fscale = (n_target > 1) ? uv_run_factor(f.run % n_target) : 1.0;
    }
    int4 item = work[wi];
    if (item.w == 0) return;
    item.w &= 0xFFFF;                              // (no table copies in this form: GRM / PCA contexts only)
    const int runs_here = inner ? n_runs : 1;
    const bool carry_on = inner && item.w == 1;    // (a tile whose K range is split over several workgroups flushes every run)
    const int all_lo = chunk_lo, all_hi = chunk_hi;

    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int64_t row_w = (int64_t)item.x * X1_TILE + wr * (16 * TS), col_w = (int64_t)item.y * X1_TILE + wc * (16 * TS);
    // word addresses: a uniform 64-bit base per 32-SNP group (scalar registers, advanced by the constant stride of a group's four word
    // rows) + this lane's 32-bit BYTE offset into those rows, once for the row side and once for the column side (at most 16 ncols_pad
    // bytes: 8 MB at N = 500 000, whatever the size of the word array) + 64 m as the instruction's immediate
    uint32_t la = (uint32_t)(4 * ((int64_t)kq * ncols_pad + row_w + l16)), lb = (uint32_t)(4 * ((int64_t)kq * ncols_pad + col_w + l16));
    const int64_t wstride = 16 * ncols_pad;        // bytes from one group's words to the next group's
    double *__restrict__ pacc = acc + acc_off(ld, tiles_c, row_w + 4 * kq, col_w + l16);
    const int64_t rs = tiles_c ? ACC_TILE : ld;

    // a slot of the carry scratch for this work item (see above); the id travels through the pace-maker's landing area, which no
    // fetch of this workgroup has touched yet (all of the LDS is spoken for)
    int slot = -1;
    unsigned int *slot_flag = nullptr;
    if (carry_on && carry_scr) {                   // (uniform over the workgroup)
        volatile int *mail = reinterpret_cast<volatile int *>(&space[0][0]);
        if (tid == 0) {
            const int xcd = (int)(__builtin_amdgcn_s_getreg(UV_GETREG_XCC_ID) & 7u);
            unsigned int *fl = carry_flags + UV_CARRY_FLAG0 + xcd * carry_slots;
            int got = -1, s = carry_slots > 0 ? (int)((blockIdx.x >> 3) % (unsigned)carry_slots) : 0;
            for (int k = 0; k < carry_slots && got < 0; k++, s = (s + 1 < carry_slots) ? s + 1 : 0) {   // ONE pass, no waiting
                unsigned int free_ = 0u;
                if (__hip_atomic_compare_exchange_strong(fl + s, &free_, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    got = xcd * carry_slots + s;
            }
            if (got < 0) (void)__hip_atomic_fetch_add(carry_flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *mail = got;
        }
        __syncthreads();
        slot = __builtin_amdgcn_readfirstlane(*mail);
        __syncthreads();                           // (wave 0's first pace-maker fetch lands where the id was)
        if (slot >= 0) slot_flag = carry_flags + UV_CARRY_FLAG0 + slot;
    }
    f32x4 *scr = carry_scr + ((int64_t)(slot < 0 ? 0 : slot) * 4 + wave) * (CARRY_REST * 64) + lane;

    f32x4 c16[TS][TS];
    zero_acc(c16);

    for (int run = 0; run < runs_here; run++) {
    if (inner) {
        chunk_lo = run * run_chunks;
        chunk_hi = (chunk_lo + run_chunks < all_hi) ? (chunk_lo + run_chunks) : all_hi;
        fscale = (n_target > 1) ? uv_run_factor(run % n_target) : 1.0;
    } else { chunk_lo = all_lo; chunk_hi = all_hi; }
    const int per = (chunk_hi - chunk_lo + item.w - 1) / item.w;   // (inline: k_part changes this kernel's code)
    const int c_beg = chunk_lo + item.z * per;
    const int c_end = (c_beg + per < chunk_hi) ? (c_beg + per) : chunk_hi;
    if (c_beg >= c_end) continue;                  // (uniform over the workgroup; never with carry_on)

    u32x4 Av[TS], Bv[2][TS];                       // row operands: ONE set, refilled in place; column operands: two sets
    uint32_t Wa[D][TS], Wb[D][TS];                 // ring of four word sets (8 row + 8 column words each): group g lives in set g & 3
    uint32_t wa7;                                  // this group's word of row operand 7 (its set is being refilled for group g + 4)
    u32x4 RF1[2], RF0[2];                          // row factors {2 u}, {-c_a u} of the lane's four pairs: group parity g & 1
    u32x4 CF1, CF0;                                // column factors of the NEXT group
    uint32_t fn;                                   // LDS position of the next group's factors (this lane's quarter)
    __attribute__((address_space(1))) const char *wnext;   // the words of the group FOUR ahead of the loop's current one (uniform)

    // conversion L (0..63) of a group, issued around MFMA L (row r = L >> 3 of the 8 x 8 order, t = L & 7):
    //   t < 4:  dword t of row operand (r == 0 ? 7 of THIS group : r - 1 of the NEXT group)
    //   t >= 4: dword t - 4 of column operand r of the next group (set T_)
#define C16_R(L) ((L) >> 3)
#define C16_ISA(L) (((L) & 7) < 4)
#define C16_AI(L) (C16_R(L) == 0 ? 7 : C16_R(L) - 1)
#define C16_D(L) ((L) & 3)
#define C16_WORD(NS_, L) (C16_ISA(L) ? (C16_R(L) == 0 ? wa7 : Wa[NS_][C16_AI(L)]) : Wb[NS_][C16_R(L)])
#define C16_CVT(NS_, L) __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(C16_WORD(NS_, L), 1.0f, C16_D(L)))
    // P_ = parity of THIS group: its own row factors RF[P_] serve operand 7, the next group's RF[P_ ^ 1] operands 0..6
#define C16_F1(P_, L) (C16_ISA(L) ? RF1[C16_R(L) == 0 ? (P_) : (P_) ^ 1][C16_D(L)] : CF1[C16_D(L)])
#define C16_F0(P_, L) (C16_ISA(L) ? RF0[C16_R(L) == 0 ? (P_) : (P_) ^ 1][C16_D(L)] : CF0[C16_D(L)])
#define C16_FMA(T_, P_, L, x)                                                                                \
    do {                                                                                                     \
        const f16x2 y_ = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, (uint32_t)(x)), __builtin_bit_cast(f16x2, (uint32_t)(C16_F1(P_, L))), \
                                                   __builtin_bit_cast(f16x2, (uint32_t)(C16_F0(P_, L))));     \
        if (C16_ISA(L)) Av[C16_AI(L)][C16_D(L)] = __builtin_bit_cast(uint32_t, y_);                           \
        else Bv[T_][C16_R(L)][C16_D(L)] = __builtin_bit_cast(uint32_t, y_);                                   \
    } while (0)
#define C16_TABLE_ASYNC(chunk, buf)                                                                            \
    do {                                                                                                       \
        const char *src_ = reinterpret_cast<const char *>(lut) + (int64_t)(chunk) * CHB + wave * (CHB / 4) + lane * 16; \
        char *dst_ = reinterpret_cast<char *>(&sfac[buf][0]) + wave * (CHB / 4);                              \
        _Pragma("unroll") for (int t_ = 0; t_ < CHB / 4 / 1024; t_++)                                          \
            x1_lds_dma16(src_ + 1024 * t_, x1_lds_off(dst_ + 1024 * t_));                                      \
        /* the pace-maker: 16 more KiB per wave from a region every workgroup reads for this chunk.  (Unrolled on purpose: as a loop  \
           with a run-time count the compiler drains vmcnt at its back edge, every iteration waits for all word loads in flight, and  \
           the workgroups drift as if there were no pace-maker: 1043 against 407 GB of word fetches, + 2 % instead of - 2 %.) */    \
        if (pace) {                                                                                            \
            const char *ps_ = pace_src + (int64_t)(chunk) * 65536 + wave * 16384 + lane * 16;                 \
            _Pragma("unroll") for (int t_ = 0; t_ < 16; t_++) x1_lds_dma16(ps_ + 1024 * t_, x1_lds_off(&space[wave][0])); \
        }                                                                                                      \
    } while (0)
#define C16_LOAD(CS_, wp_, m)                                                                 \
    do {                                                                                      \
        if ((m) < TS) Wa[CS_][(m) < TS ? (m) : 0] = *(__attribute__((address_space(1))) const uint32_t *)((wp_) + la + 64 * (m));          \
        else Wb[CS_][(m) >= TS ? (m) - TS : 0] = *(__attribute__((address_space(1))) const uint32_t *)((wp_) + lb + 64 * ((m) - TS));      \
    } while (0)
    // the words' ONE wait of a group: vmcnt counts in order, the next group's sixteen words were requested three groups ago and the 32
    // requests of the two groups since are all that may still be under way (a chunk's factor copy and pace-maker pieces, where they lie
    // in between, only make the true number larger: the loop body is shared by a chunk's four rounds, so it takes the count that holds
    // in all of them)
#define C16_WAIT_WORDS() __builtin_amdgcn_s_waitcnt(0x8F70)      /* vmcnt(32) */
#define C16_MFMA(m, S_)                                                                                             \
        c16[(m) >> 3][(m) & 7] = __builtin_amdgcn_mfma_f32_16x16x32_f16(                                             \
            (f16x8)Av[(m) >> 3], (f16x8)Bv[S_][(m) & 7], c16[(m) >> 3][(m) & 7], 0, 0, 0)
    // issue pattern: as syrk_uv16_kernel's -- two companions of ONE kind behind every MFMA: [M cc][M ff], the conversions of a batch of
    // four one batch ahead of their fmas
#define C16_SB() __builtin_amdgcn_sched_barrier(0)
#define C16_M(m, S_) do { C16_MFMA(m, S_); C16_SB(); } while (0)
#define C16_C2(NS_, m, k)      /* conversions m + 4 + k, + 1 (the NEXT batch) into the other register half */                       \
    do {                                                                                                                            \
        if ((m) == 0 && (k) == 0) { C16_WAIT_WORDS(); C16_SB(); }   /* behind MFMA 0: the first touch of the next group's words */ \
        if ((m) == 60 && (k) == 0) {                     /* MFMA 60 has no conversions behind it: the word base moves on here */  \
            wnext += wstride;                                                                                                       \
            asm volatile("" : "+s"(wnext));              /* (a running base: no product of the group index) */                     \
        }                                                                                                                           \
        if ((m) + 4 + (k) < 64) {                                                                                                   \
            x_[4 * ((((m) >> 2) + 1) & 1) + (k)] = C16_CVT(NS_, ((m) + 4 + (k)) & 63);                                              \
            x_[4 * ((((m) >> 2) + 1) & 1) + (k) + 1] = C16_CVT(NS_, ((m) + 5 + (k)) & 63);                                          \
            asm volatile("" : "+v"(x_[4 * ((((m) >> 2) + 1) & 1) + (k)]), "+v"(x_[4 * ((((m) >> 2) + 1) & 1) + (k) + 1]));           \
        }                                                                                                                           \
        C16_SB();                                                                                                                   \
    } while (0)
#define C16_F2(T_, P_, m, k)   /* fmas m + k, + 1 of THIS batch */                                                                  \
    do {                                                                                                                            \
        C16_FMA(T_, P_, (m) + (k), x_[4 * (((m) >> 2) & 1) + (k)]); C16_FMA(T_, P_, (m) + (k) + 1, x_[4 * (((m) >> 2) & 1) + (k) + 1]); \
        C16_SB();                                                                                                                   \
    } while (0)
#define C16_STEP4(m, S_, T_, CS_, NS_, P_)                                                                          \
    do {                                                                                                            \
        C16_M(m, S_);       C16_C2(NS_, m, 0);                                                                      \
        C16_M((m) + 1, S_); C16_F2(T_, P_, m, 0);                                                                   \
        C16_M((m) + 2, S_); C16_C2(NS_, m, 2);                                                                      \
        C16_M((m) + 3, S_); C16_F2(T_, P_, m, 2);                                                                   \
        if ((m) < 16) {     /* the words of group g + 4 into this group's set, four behind each of the first four batches */ \
            C16_LOAD(CS_, wnext, m); C16_LOAD(CS_, wnext, (m) + 1); C16_LOAD(CS_, wnext, (m) + 2); C16_LOAD(CS_, wnext, (m) + 3); \
            C16_SB();                                                                                               \
        }                                                                                                           \
    } while (0)
#define C16_STEP8(m, ...) C16_STEP4(m, __VA_ARGS__); C16_STEP4((m) + 4, __VA_ARGS__)
    // one 32-SNP group g (parity P_, word set CS_ = g & 3, the next group's NS_; wnext = the words of group g + 4): the next group's
    // factors are requested first (row pairs first used behind MFMA 8, column pairs behind MFMA 4)
#define C16_GROUP(S_, T_, CS_, NS_, P_)                                                                             \
    do {                                                                                                            \
        wa7 = Wa[CS_][7];                                                                                           \
        asm volatile("" : "+v"(wa7));                                                                               \
        asm volatile("" : "+v"(la), "+v"(lb));   /* (32-bit lane offsets where the loads are: hoisted as 64-bit pairs they cost an add each) */ \
        CF1 = x1_lds128(fn + 128); CF0 = x1_lds128(fn + 192);                                                       \
        RF1[(P_) ^ 1] = x1_lds128(fn); RF0[(P_) ^ 1] = x1_lds128(fn + 64);                                          \
        uint32_t x_[8];                                                                                             \
        x_[0] = C16_CVT(NS_, 0); x_[1] = C16_CVT(NS_, 1); x_[2] = C16_CVT(NS_, 2); x_[3] = C16_CVT(NS_, 3);         \
        C16_STEP8(0, S_, T_, CS_, NS_, P_);  C16_STEP8(8, S_, T_, CS_, NS_, P_);                                     \
        C16_STEP8(16, S_, T_, CS_, NS_, P_); C16_STEP8(24, S_, T_, CS_, NS_, P_);                                    \
        C16_STEP8(32, S_, T_, CS_, NS_, P_); C16_STEP8(40, S_, T_, CS_, NS_, P_);                                    \
        C16_STEP8(48, S_, T_, CS_, NS_, P_); C16_STEP8(56, S_, T_, CS_, NS_, P_);                                    \
        fn += GST;                                                                                                  \
    } while (0)

    // prologue: factors of the first chunk, the words of the first four groups, the operands of group 0 (row operand 7 comes with row 0)
    C16_TABLE_ASYNC(c_beg, c_beg & 1);
    // (the run's first group may lie anywhere in the block -- c_beg of a tile split along K, of a fused (tile, run) item, of a later
    // run -- and anywhere in a word array of many GiB: the base is a 64-bit product, made here once per run)
    wnext = (__attribute__((address_space(1))) const char *)w8 + (int64_t)c_beg * GCH * wstride;
#define C16_L16(S) C16_LOAD(S, wnext, 0); C16_LOAD(S, wnext, 1); C16_LOAD(S, wnext, 2); C16_LOAD(S, wnext, 3);       \
                   C16_LOAD(S, wnext, 4); C16_LOAD(S, wnext, 5); C16_LOAD(S, wnext, 6); C16_LOAD(S, wnext, 7);       \
                   C16_LOAD(S, wnext, 8); C16_LOAD(S, wnext, 9); C16_LOAD(S, wnext, 10); C16_LOAD(S, wnext, 11);     \
                   C16_LOAD(S, wnext, 12); C16_LOAD(S, wnext, 13); C16_LOAD(S, wnext, 14); C16_LOAD(S, wnext, 15);   \
                   wnext += wstride
    C16_L16(0); C16_L16(1); C16_L16(2); C16_L16(3);
#undef C16_L16
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();
    fn = x1_lds_off(&sfac[c_beg & 1][0]) + 16 * kq;
    {
        // group 0: row operands 0..6 and the eight column operands (set 0) from word set 0 with group 0's factors
        RF1[0] = x1_lds128(fn); RF0[0] = x1_lds128(fn + 64);
        CF1 = x1_lds128(fn + 128); CF0 = x1_lds128(fn + 192);      // (group 0's columns: the loop's first group replaces them with group 1's)
#define C16_PO(W, d, F1_, F0_) __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(__builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(W, 1.0f, d)), \
                                   __builtin_bit_cast(f16x2, (uint32_t)F1_[d]), __builtin_bit_cast(f16x2, (uint32_t)F0_[d])))      /* (the casts matter: __builtin_bit_cast of a vector-ELEMENT lvalue reads element 0) */
#define C16_PA(i) Av[i][0] = C16_PO(Wa[0][i], 0, RF1[0], RF0[0]); Av[i][1] = C16_PO(Wa[0][i], 1, RF1[0], RF0[0]); \
                  Av[i][2] = C16_PO(Wa[0][i], 2, RF1[0], RF0[0]); Av[i][3] = C16_PO(Wa[0][i], 3, RF1[0], RF0[0])
#define C16_PB(j) Bv[0][j][0] = C16_PO(Wb[0][j], 0, CF1, CF0); Bv[0][j][1] = C16_PO(Wb[0][j], 1, CF1, CF0); \
                  Bv[0][j][2] = C16_PO(Wb[0][j], 2, CF1, CF0); Bv[0][j][3] = C16_PO(Wb[0][j], 3, CF1, CF0)
        C16_PA(0); C16_PA(1); C16_PA(2); C16_PA(3); C16_PA(4); C16_PA(5); C16_PA(6);
        C16_PB(0); C16_PB(1); C16_PB(2); C16_PB(3); C16_PB(4); C16_PB(5); C16_PB(6); C16_PB(7);
#undef C16_PB
#undef C16_PA
#undef C16_PO
    }
    fn += GST;                                     // (RF[0] stays group 0's: its row operand 7 is made behind row 0)

    for (int c = c_beg; c < c_end; c++) {
        const int cur = c & 1;
        const int q_cnt = (c * (CHS / 16) + CHS / 16 <= n_q) ? GCH : (n_q - c * (CHS / 16)) / 2;   // 32-SNP groups: a multiple of 8
        const bool more = (c + 1 < c_end);
        if (more) C16_TABLE_ASYNC(c + 1, cur ^ 1);  // every wave is past the barrier that freed this buffer
        for (int q = 0; q < q_cnt; q += 2 * D) {
            C16_GROUP(0, 1, 0, 1, 0);
            C16_GROUP(1, 0, 1, 2, 1);
            C16_GROUP(0, 1, 2, 3, 0);
            C16_GROUP(1, 0, 3, 0, 1);
            C16_GROUP(0, 1, 0, 1, 0);
            C16_GROUP(1, 0, 1, 2, 1);
            C16_GROUP(0, 1, 2, 3, 0);
            // the chunk's last group prepares the NEXT chunk's first group (or, at the very end, harmlessly re-reads this chunk)
            if (q + 2 * D >= q_cnt) {
                if (more) {
                    // vmcnt is in-order: the factor copy went out at the start of this chunk, behind it at least seven groups of 16 word
                    // loads -- all but the newest 62 requests covers it
                    __builtin_amdgcn_s_waitcnt(0xCF7E); // vmcnt(62)
                    __syncthreads();
                    fn = x1_lds_off(&sfac[cur ^ 1][0]) + 16 * kq;
                } else {
                    fn = x1_lds_off(&sfac[cur][0]) + 16 * kq;
                }
            }
            C16_GROUP(1, 0, 3, 0, 1);
        }
    }
    {
        double *pflush = flush_ptr(pacc);
        const int64_t rows_left = flush_rows_left(n_rows_real, row_w + 4 * kq);
        const bool first_run = (run == 0), last_run = (run + 1 == runs_here);
        const float fs32 = (float)fscale;          // 1 - q / 4096: exact in fp32
        // carried sub-tile (i, j) of the LDS part: fp32 sums in LDS until the block's last run
#define C16_LDS_CARRY(i, j)                                                                                        \
        do {                                                                                                       \
            f32x4 *cp = &scar[wave][((i) * TS + (j)) * 64 + lane];                                                 \
            f32x4 t = c16[i][j] * fs32;                                                                            \
            if (!first_run) t += *cp;                                                                              \
            if (!last_run) *cp = t;                                                                                \
            c16[i][j] = t;                 /* (what the last run flushes below; every other run clears it) */      \
        } while (0)
        if (slot >= 0) {
            // every sub-tile carried: 0 .. CARRY_SUB - 1 in LDS, the others in the slot.  The slot's loads first, all of them, into
            // the registers the K loop has left; the LDS part runs while they are under way.
            f32x4 sv[CARRY_REST];
            f32x4 *sp_ = scr;                      // (opaque, as pflush: 29 addresses kept across the K loop would be spilled)
            asm volatile("" : "+v"(sp_));
            __attribute__((address_space(1))) f32x4 *sp = (__attribute__((address_space(1))) f32x4 *)sp_;
            if (first_run) {
#pragma unroll
                for (int k = 0; k < CARRY_REST; k++) sv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int k = 0; k < CARRY_REST; k++) sv[k] = sp[k * 64];
            }
#pragma unroll
            for (int s = 0; s < CARRY_SUB; s++) C16_LDS_CARRY(s / TS, s % TS);
#pragma unroll
            for (int k = 0; k < CARRY_REST; k++) {
                const int i = (CARRY_SUB + k) / TS, j = (CARRY_SUB + k) % TS;
                const f32x4 t = c16[i][j] * fs32 + sv[k];
                if (!last_run) sp[k * 64] = t;
                c16[i][j] = t;
            }
            if (last_run) {
                // the slot is free once the last reads of all four waves have returned (they have: the sums above used them)
                __syncthreads();
                if (tid == 0) __hip_atomic_store(slot_flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int i = 0; i < TS; i++) flush_row16(pflush, rs, rows_left, c16, i, fscale, TS, true);   // (the sums carry their factors already)
            }
        } else {
#pragma unroll
        for (int i = 0; i < TS; i++) {
            const int nc = carry_on ? ((CARRY_SUB - i * TS) < 0 ? 0 : (CARRY_SUB - i * TS) > TS ? TS : (CARRY_SUB - i * TS)) : 0;   // carried: j < nc
#pragma unroll
            for (int j = 0; j < TS; j++)
                if (j < nc) C16_LDS_CARRY(i, j);
            if (nc == TS && !last_run) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {       // (inline: flush_row16 with a run-time nc changes this kernel's code)
                const int row = i * 16 + r;
                double *__restrict__ pr = pflush + (int64_t)row * rs;
                if (row < rows_left) {
#pragma unroll
                    for (int j = 0; j < TS; j++)      // f_q x fp32 partial: exact in fp64 (13 + 24 bits); carried sums carry their factors already
                        if (j >= nc || last_run)
                            (void)__builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double *)(pr + 16 * j),
                                                                          (double)c16[i][j][r] * (j < nc ? 1.0 : fscale));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        }
#undef C16_LDS_CARRY
        zero_acc(c16);
    }
    }   // run
#undef C16_GROUP
#undef C16_STEP8
#undef C16_STEP4
#undef C16_F2
#undef C16_C2
#undef C16_M
#undef C16_SB
#undef C16_MFMA
#undef C16_WAIT_WORDS
#undef C16_LOAD
#undef C16_TABLE_ASYNC
#undef C16_FMA
#undef C16_F0
#undef C16_F1
#undef C16_CVT
#undef C16_WORD
#undef C16_D
#undef C16_AI
#undef C16_ISA
#undef C16_R
}
#pragma clang diagnostic pop

// run_chunks: table chunks per fp32 run (0: the whole block is one run); n_target > 1: run q's sums are multiplied by
// uv_run_factor(q) at its flush (the run's SNPs were factorised for the weight target t / f_q, uv_factor_kernel)
int launch_syrk_uv(hipStream_t st, const SyrkPanel &p, const SyrkUvOpts &o)
{
    const int run_if_missing = o.run_if_missing ? 1 : 0, pace = o.pace ? 1 : 0, uv16 = (int)o.form;    // the kernels' integer codes
    if (o.n_q <= 0 || o.n_blocks_x1 <= 0) return 0;
    const int n_chunk = (o.n_q + (UV_CHS / 16) - 1) / (UV_CHS / 16);           // table chunks of the block; one launch per fp32 run
    const int run = o.run_chunks > 0 ? o.run_chunks : n_chunk;
    const int n_runs = (n_chunk + run - 1) / run;
    // (round 6: a non-atomic read-modify-write flush for tiles with one owner per launch was measured -- 465.8 against 456.8 ms per
    // step in the one-launch-per-run form, profiles/r06_flush_rmw_ab.txt -- and removed)
    // One launch geometry for the three kernels (uv16: the 16x16x32 form, its tables carry swapped odd quarters; uv16 >= 2:
    // syrk_uv16c_kernel, `o.lut` = the slots' factor arrays, pace-maker and carry arguments instead of table copies).
    // uv16 == 3: work items = tiles, the runs walked inside, the sub-tile sums carried in LDS and in the carry scratch.
    const bool inner = (uv16 == 3 && n_runs > 1);
    const RunLaunches g{o.n_blocks_x1, n_chunk, run, n_runs, inner ? -1 : n_runs > 1 ? run_inner_launch() : 0};
    const auto kern = uv16 ? syrk_uv16_kernel : syrk_uv_kernel;
    for (int k = 0; k < g.count(); k++) {
        const RunLaunch L = g.at(k);
        // a launch of ONE run takes the run's flush factor as an argument; the others find it from the run index and n_target
        const double fscale = (!g.group && o.n_target > 1) ? uv_run_factor(k % o.n_target) : 1.0;
        const int n_target = g.group ? o.n_target : 1;
        if (o.n_launched) ++*o.n_launched;
        if (uv16 >= 2)
            hipLaunchKernelGGL(syrk_uv16c_kernel, dim3(L.grid), dim3(256), 0, st, p.w8, p.ncols_pad, o.lut, o.n_q, p.acc, p.ld, p.tiles_c, o.work_x1,
                               o.d_missing, p.n_rows_real, L.chunk_lo, L.chunk_hi, fscale, L.n_runs, L.run_chunks, n_target, L.run_group, L.n_items8,
                               run_if_missing, (const char *)o.pace_src, pace, inner ? (f32x4 *)o.carry_scr : (f32x4 *)nullptr,
                               inner ? o.carry_flags : (unsigned int *)nullptr, inner && o.carry_scr ? o.carry_slots : 0);
        else
            hipLaunchKernelGGL(kern, dim3(L.grid), dim3(256), 0, st, p.w8, p.ncols_pad, o.lut, o.n_q, p.acc, p.ld, p.tiles_c, o.work_x1, o.d_missing,
                               p.n_rows_real, L.chunk_lo, L.chunk_hi, fscale, L.n_runs, L.run_chunks, n_target, L.run_group, L.n_items8, run_if_missing,
                               o.copy_lut_bytes, o.copy_acc_elems);
    }
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
