// The N x N pair counters (the SYRK half of the hot path: kernels_syrk.hip, kernels_syrk_uv.hip):
//
//  pair_mfma_i8_kernel   IBS / KING / beta counters and the GCTA both-missing counts as exact int8 MFMA contractions
//      (default; replaces CIBSCount::thread_ibs_num src/genIBS.cpp:154-273, CKINGRobust::thread_ibs_num
//       src/genKING.cpp:292-426, the integer half of CKINGHomo::thread_ibs_num src/genKING.cpp:66-200, CIndivBeta
//       src/genBeta.cpp:65-183 and the serial missing-denominator loop of CGCTA_AlgArith::Run src/genPCA.cpp:1201-1224)
//  pair_popcount_kernel  the same counters as wavefront bit-ops (SNPGPU_PAIR_BACKEND=popcount)
//  pair_sparse_miss_kernel      the GCTA both-missing counts from the sets of samples with a missing call
//  pair_mfma_fp4_miss_kernel, pair_mfma_fp4_nomiss_kernel, pair_mfma_fp4_kernel   the same counters on the MX-fp4 MFMA
#include <algorithm>
#include "snpgpu_internal.h"
#include "syrk_device.h"
#include <utility>

namespace snpgpu {

// ---------------------------------------------------------------------------
// bit-plane pair counters.  One wave = 8 rows x 128 columns: the row samples' plane words are
// wave-uniform (scalar loads, SGPR operands), each lane owns two column samples.
// Instruction costs measured on MI355X (tools/ubench/valu_asm_ubench.hip): v_and/v_xor/v_bitop3
// 2.4 cycles per wave64 instruction, v_bcnt_u32_b32 and v_and_or_b32 4.2 -> popcounts dominate and
// 3-input logic goes through v_bitop3_b32.
template <int MODE> struct PairOps;

// f(a,b,c) truth tables for v_bitop3_b32 (a=0xF0, b=0xCC, c=0xAA)
#define BITOP3_A_OR_BC 0xF8     /* a | (b & c)  */
#define BITOP3_AXB_AND_C 0x28   /* (a ^ b) & c  */

template <> struct PairOps<PM_IBS> {   // 4 logic + 3 popcount ops / 32 SNP pairs
    typedef uint4 PV;
    static constexpr int C = 3;       // {nvalid, ibs1, ibs0}
    static __device__ __forceinline__ void run(const uint4 &r, const uint4 &c, uint32_t *cnt)
    {
        const uint32_t t0 = r.x & c.x;                     // both called
        cnt[0] += __popc(t0);
        cnt[1] += __popc(__builtin_amdgcn_bitop3_b32(c.y, r.y, t0, BITOP3_AXB_AND_C));   // one het -> IBS1
        cnt[2] += __popc(__builtin_amdgcn_bitop3_b32(r.z & c.w, r.w, c.z, BITOP3_A_OR_BC));  // opposite hom -> IBS0
    }
};
template <> struct PairOps<PM_KING_ROBUST> {   // 6 logic + 5 popcount ops / 32 SNP pairs
    typedef uint4 PV;
    static constexpr int C = 5;       // {nLoci, ibs1, ibs0, N1_Aa, N2_Aa}
    static __device__ __forceinline__ void run(const uint4 &r, const uint4 &c, uint32_t *cnt)
    {
        cnt[0] += __popc(r.x & c.x);
        const uint32_t a = r.y & c.x;                      // row het, column called
        const uint32_t b = r.x & c.y;                      // column het, row called
        cnt[3] += __popc(a);
        cnt[4] += __popc(b);
        cnt[1] += __popc(a ^ b);
        cnt[2] += __popc(__builtin_amdgcn_bitop3_b32(r.z & c.w, r.w, c.z, BITOP3_A_OR_BC));
    }
};
template <> struct PairOps<PM_KING_HOMO> {
    typedef uint4 PV;
    static constexpr int C = 2;       // {ibs1, ibs0}
    static __device__ __forceinline__ void run(const uint4 &r, const uint4 &c, uint32_t *cnt)
    {
        cnt[0] += __popc(__builtin_amdgcn_bitop3_b32(c.y, r.y, r.x & c.x, BITOP3_AXB_AND_C));
        cnt[1] += __popc(__builtin_amdgcn_bitop3_b32(r.z & c.w, r.w, c.z, BITOP3_A_OR_BC));
    }
};
template <> struct PairOps<PM_BETA> {          // CIndivBeta::thread_ibs_num, src/genBeta.cpp:65-183
    typedef uint4 PV;
    static constexpr int C = 3;       // {num, at least one het (both called), both homozygous and equal}
    static __device__ __forceinline__ void run(const uint4 &r, const uint4 &c, uint32_t *cnt)
    {
        const uint32_t t0 = r.x & c.x;
        cnt[0] += __popc(t0);
        cnt[1] += __popc(__builtin_amdgcn_bitop3_b32(c.y, r.y, t0, 0xA8));                   // (Hi | Hj) & t0
        cnt[2] += __popc(__builtin_amdgcn_bitop3_b32(r.z & c.z, r.w, c.w, BITOP3_A_OR_BC));  // (Oi&Oj) | (Ti&Tj)
    }
};
template <> struct PairOps<PM_GCTA_MISS> {     // uint2 = 64 SNPs
    typedef uint2 PV;
    static constexpr int C = 1;       // {both missing at a polymorphic SNP}
    static __device__ __forceinline__ void run(const uint2 &r, const uint2 &c, uint32_t *cnt)
    {
        cnt[0] += __popc(r.x & c.x);
        cnt[0] += __popc(r.y & c.y);
    }
};

// Row operands are stored [row group of 8][word][8 rows] so that the 8 rows of a wave for one
// word are 8*sizeof(PV) consecutive bytes (two s_load_dwordx16 for uint4 planes).
template <int MODE>
__global__ __launch_bounds__(256) void pair_popcount_kernel(
    const typename PairOps<MODE>::PV *__restrict__ rowp, const typename PairOps<MODE>::PV *__restrict__ colp,
    int KWv /* plane vectors per sample */, int64_t ncols_pad, uint32_t *__restrict__ acc, int64_t acc_plane,
    const int *__restrict__ prefix, const int *__restrict__ first, int n_sr, int n_super, int n_tr, int n_tc,
    const unsigned long long *__restrict__ d_skip_if_zero)
{
    typedef typename PairOps<MODE>::PV PV;
    constexpr int C = PairOps<MODE>::C;
    constexpr int A = PC_ROWS_PER_WAVE, BC = PC_COLS_PER_LANE;
    if (d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    const TileCoord t = map_tile(prefix, first, n_sr, n_super, TileShape{PC_SUPER, PC_TILE_R, PC_TILE_C}, n_tr, n_tc);
    if (!t.valid) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int row_base = t.tr * PC_TILE_R + wave * A;          // wave-uniform, multiple of 8
    const int64_t col_base = (int64_t)t.tc * PC_TILE_C + lane;

    uint32_t cnt[A][BC][C];
#pragma unroll
    for (int a = 0; a < A; a++)
#pragma unroll
        for (int b = 0; b < BC; b++)
#pragma unroll
            for (int c = 0; c < C; c++) cnt[a][b][c] = 0;

    const PV *__restrict__ rp = rowp + (int64_t)(row_base / A) * KWv * A;   // [word][8 rows]
    const PV *__restrict__ cp = colp + col_base;

    // One word per iteration, loads at the top: with 5-7 resident waves per SIMD the other waves'
    // VALU work covers the load latency (measured faster than explicit ping-pong prefetching, which
    // costs registers and therefore occupancy -- tools/ubench/pc_ubench.hip).
    for (int kw = 0; kw < KWv; kw++) {
        PV r[A], c[BC];
#pragma unroll
        for (int a = 0; a < A; a++) r[a] = rp[(int64_t)kw * A + a];
#pragma unroll
        for (int b = 0; b < BC; b++) c[b] = cp[(int64_t)kw * ncols_pad + b * 64];
#pragma unroll
        for (int a = 0; a < A; a++)
#pragma unroll
            for (int b = 0; b < BC; b++) PairOps<MODE>::run(r[a], c[b], cnt[a][b]);
    }
    // accumulate into the panel's counters.  Each element has exactly one owner per launch, so the
    // atomics never contend: they are used as fire-and-forget adds (no load -> wait -> store chain).
#pragma unroll
    for (int a = 0; a < A; a++)
#pragma unroll
        for (int b = 0; b < BC; b++) {
            uint32_t *p = acc + (int64_t)(row_base + a) * ncols_pad + col_base + b * 64;
#pragma unroll
            for (int c = 0; c < C; c++)   // the ibs0 plane of the IBS / KING counters holds 2 * ibs0 (I8Scheme<PM_IBS_NOMISS>)
                atomicAdd(p + (int64_t)c * acc_plane, (((MODE == PM_IBS || MODE == PM_KING_ROBUST) && c == 2) ||
                                                       (MODE == PM_KING_HOMO && c == 1)) ? 2u * cnt[a][b][c] : cnt[a][b][c]);
        }
}

template <int MODE>
static int launch_pc(hipStream_t st, const TileGrid &tg, const void *rowp, const void *colp, int KW,
                     int64_t ncols_pad, uint32_t *acc, int64_t acc_plane, const unsigned long long *skip)
{
    typedef typename PairOps<MODE>::PV PV;
    const int KWv = (sizeof(PV) == 16) ? KW : KW / 2;
    hipLaunchKernelGGL(pair_popcount_kernel<MODE>, dim3((unsigned)tg.grid), dim3(256), 0, st, (const PV *)rowp,
                       (const PV *)colp, KWv, ncols_pad, acc, acc_plane, tg.d_prefix, tg.d_first, tg.n_sr,
                       tg.n_super, tg.n_tr, tg.n_tc, skip);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_pair_popcount(hipStream_t st, int mode, const TileGrid &tg, const void *rowp, const void *colp, int KW,
                         int64_t ncols_pad, uint32_t *acc, int64_t acc_plane,
                         const unsigned long long *d_skip_if_zero)
{
    switch (mode) {
    case PM_IBS: return launch_pc<PM_IBS>(st, tg, rowp, colp, KW, ncols_pad, acc, acc_plane, d_skip_if_zero);
    case PM_KING_ROBUST: return launch_pc<PM_KING_ROBUST>(st, tg, rowp, colp, KW, ncols_pad, acc, acc_plane, d_skip_if_zero);
    case PM_KING_HOMO: return launch_pc<PM_KING_HOMO>(st, tg, rowp, colp, KW, ncols_pad, acc, acc_plane, d_skip_if_zero);
    case PM_GCTA_MISS: return launch_pc<PM_GCTA_MISS>(st, tg, rowp, colp, KW, ncols_pad, acc, acc_plane, d_skip_if_zero);
    case PM_BETA: return launch_pc<PM_BETA>(st, tg, rowp, colp, KW, ncols_pad, acc, acc_plane, d_skip_if_zero);
    }
    set_error("launch_pair_popcount: bad mode");
    return 1;
}

// ---------------------------------------------------------------------------
// pair_sparse_miss_kernel: the GCTA both-missing counts of a 256 x 256 tile from the SETS of samples with a missing call
// (missmask256_kernel: MM[group][snp] = 256 bits).  One workgroup of 1024 threads per work item {tile row, tile column, K part,
// K parts}; the tile's 65 536 counters sit in LDS as 16-bit halves of 32 768 dwords (counter (r, c) = half c & 1 of dword
// 128 r + c / 2; at most 32 768 SNPs between two flushes, so a half cannot overflow).  A thread takes one SNP at a time: the two
// sets (2 x 32 bytes, consecutive SNPs adjacent), and for every pair (bit of the row set, bit of the column set) one LDS atomic
// add.  Work ~ f^2 N^2 B / 2 for a missing rate f against N^2 B / 2 int8 products of the dense form: 1 / 2500 of the products at
// f = 2 %.  The flush adds the non-zero dwords to the counter panel (atomic: parts share a tile).
__global__ __launch_bounds__(1024) void pair_sparse_miss_kernel(const uint4 *__restrict__ mm, int64_t snp_stride, int n_snp,
                                                                uint32_t *__restrict__ acc, int64_t ncols_pad,
                                                                const int4 *__restrict__ work,
                                                                const unsigned long long *__restrict__ d_run)
{
    if (*d_run == 0ull) return;
    __shared__ uint32_t cnt[256 * 128];
    const int4 item = work[blockIdx.x];
    if (item.w == 0) return;
    const int per = (((n_snp + item.w - 1) / item.w) + 1023) / 1024 * 1024;
    const int s_beg = item.z * per, s_end = (s_beg + per < n_snp) ? (s_beg + per) : n_snp;
    if (s_beg >= s_end) return;
    const int tid = threadIdx.x;
    const uint4 *__restrict__ mi = mm + (int64_t)item.x * snp_stride * 2;
    const uint4 *__restrict__ mj = mm + (int64_t)item.y * snp_stride * 2;
    for (int sb = s_beg; sb < s_end; sb += 32768) {
        const int se = (sb + 32768 < s_end) ? (sb + 32768) : s_end;
        for (int e = tid; e < 256 * 128; e += 1024) cnt[e] = 0u;
        __syncthreads();
        for (int s = sb + tid; s < se; s += 1024) {
            const uint4 a0 = mi[2 * (int64_t)s], a1 = mi[2 * (int64_t)s + 1];
            if ((a0.x | a0.y | a0.z | a0.w | a1.x | a1.y | a1.z | a1.w) == 0u) continue;
            const uint4 b0 = mj[2 * (int64_t)s], b1 = mj[2 * (int64_t)s + 1];
            const uint32_t ra[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const uint32_t cb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            if ((b0.x | b0.y | b0.z | b0.w | b1.x | b1.y | b1.z | b1.w) == 0u) continue;
            for (int a = 0; a < 8; a++) {
                uint32_t x = ra[a];
                while (x) {
                    const int r = 32 * a + __builtin_ctz(x);
                    x &= x - 1u;
                    uint32_t *row = cnt + r * 128;
                    for (int b = 0; b < 8; b++) {
                        uint32_t y = cb[b];
                        while (y) {
                            const int c = __builtin_ctz(y);
                            y &= y - 1u;
                            atomicAdd(row + 16 * b + (c >> 1), 1u << (16 * (c & 1)));
                        }
                    }
                }
            }
        }
        __syncthreads();
        uint32_t *__restrict__ dst = acc + (int64_t)item.x * 256 * ncols_pad + (int64_t)item.y * 256;
        for (int e = tid; e < 256 * 128; e += 1024) {
            const uint32_t v = cnt[e];
            if (v) {
                uint32_t *p = dst + (int64_t)(e >> 7) * ncols_pad + 2 * (e & 127);
                if (v & 0xFFFFu) atomicAdd(p, v & 0xFFFFu);
                if (v >> 16) atomicAdd(p + 1, v >> 16);
            }
        }
        __syncthreads();
    }
}

int launch_pair_sparse_miss(hipStream_t st, const uint4 *mm, int64_t snp_stride, int n_snp, uint32_t *acc, int64_t ncols_pad,
                            const int4 *work, int n_blocks, const unsigned long long *d_run)
{
    if (n_snp <= 0 || n_blocks <= 0) return 0;
    hipLaunchKernelGGL(pair_sparse_miss_kernel, dim3((unsigned)n_blocks), dim3(1024), 0, st, mm, snp_stride, n_snp, acc, ncols_pad, work, d_run);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// The same counters as exact int8 contractions on the matrix cores.
// Per genotype code (0,1,2 = allele count, 3 = missing) define int8 values
//     v = called   h = het   y = hom   s = v - 2h   x = [g==0] - [g==2]      (all 0 for missing)
// then for a pair of samples, summed over SNPs,
//     v.v' = both called            s.s' = both called - 2 * (exactly one het)
//     h.v' = row het & col called   h.h' = both het      y.y' - x.x' = 2 * (opposite homozygotes)
//     y.y' + x.x' = 2 * (equal homozygotes)             h.y' + y.h' = exactly one het
// i.e. every counter of PairOps<> is an exact integer combination of a few int8 dot products, which
// v_mfma_i32_32x32x32_i8 evaluates 32 SNPs x 1024 pairs at a time with int32 accumulation (bit-exact).
// Measured on MI355X (tools/ubench/i8_ubench.hip): SIMD time = 36 cycles per MFMA + ~4 cycles per
// VALU op (they do not overlap), so the operand decode is kept to shift/and (four clean codes per
// dword: (w >> 2u) & 0x03030303) plus ONE v_perm_b32 per operand dword (the code bytes select from a
// 4-byte value table).  Lane l holds sample (l & 31) and 16 of the 32 SNPs of a k-step in one dword
// of the sample-major 2-bit words W2[d][sample] (d = 16-SNP group, half h = l >> 5 reads d = 2q + h);
// any SNP order inside a k-step is legal because both operands use the same one.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

#define I8T_V 0x00010101u     /* byte c of the table = value for code c */
#define I8T_H 0x00000100u
#define I8T_NH 0x0000FF00u
#define I8T_S 0x0001FF01u
#define I8T_Y 0x00010001u
#define I8T_X 0x00FF0001u
#define I8T_NX 0x000100FFu
#define I8T_M 0x01000000u     /* code 3 only */
#define I8T_E0 0x00000001u    /* g == 0 */
#define I8T_E2 0x00010000u    /* g == 2 */
#define I8T_G 0x00020100u     /* g itself (0 for missing) */
#define I8T_G2 0x00000102u    /* 2 - g (0 for missing) */
#define I8T_CODE 0xFFFFFFFFu  /* the code byte itself as operand (0, 1, 2; 3 for missing / padding): no table lookup */

template <int MODE> struct I8Scheme;
template <> struct I8Scheme<PM_IBS> {            // 4 MFMA slots, 3 accumulators, 64 x 64 per wave
    static constexpr int NS = 4, NA = 3, TM = 2, TN = 2, C = 3, WPS = 2;
    // ibs0 as e0.e2' + e2.e0' (binary operands) rather than (y.y' - x.x') / 2 (x = +-1): same four products and
    // value types, fewer toggling multiplier bits -- the kernel runs at the socket power cap (HISTORY.md 4.5)
    static __device__ __forceinline__ constexpr uint32_t ta(int s) { return s == 0 ? I8T_V : s == 1 ? I8T_S : s == 2 ? I8T_E0 : I8T_E2; }
    static __device__ __forceinline__ constexpr uint32_t tb(int s) { return s == 0 ? I8T_V : s == 1 ? I8T_S : s == 2 ? I8T_E2 : I8T_E0; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s == 0 ? 0 : s == 1 ? 1 : 2; }
    static __device__ __forceinline__ void emit(const int *a, int, uint32_t *cnt)   // {nvalid, ibs1, 2 ibs0}
    {
        cnt[0] = (uint32_t)a[0]; cnt[1] = (uint32_t)(a[0] - a[1]) >> 1; cnt[2] = 2u * (uint32_t)a[2];
    }
};
// IBS / KING-robust for blocks WITHOUT missing calls (imputed data): TWO products, h.h' and g.g' (h = het, g = the
// genotype itself).  With the per-sample counts H = #het and T = #(g == 2) of the block:
//     ibs1 = H_i + H_j - 2 h.h'                (exactly one het)
//     sum (g - g')^2 = ibs1 + 4 ibs0 = (H_i + 4 T_i) + (H_j + 4 T_j) - 2 g.g'      =>      2 ibs0 = 2 (T_i + T_j) + h.h' - g.g'
//     KING: N1_Aa = H_i, N2_Aa = H_j
// (with the per-sample margins known, ibs0 and ibs1 span two dimensions modulo separable terms: two products is the
// minimum; the three-product binary form h.h', e0.e2', e2.e0' was 1.5x the MFMA work).  g.g' needs no operand table at all:
// the extracted code bytes ARE g (padding SNPs hold code 3 for every sample: 9 per padding SNP and pair, a constant the
// flush puts back) -- 24 fewer v_perm_b32 per k-step, 4.3 instead of 5.8 decode instructions per MFMA.  Operands {0, 1} and
// {0, 1, 2, (3)}: the first two-product form used x = [g==0] - [g==2], whose -1 bytes put the kernel back at the power cap
// (2.2 GHz, 1364 W).  The kernel adds {n, -2 h.h', h.h' - g.g'}; the rank-one terms H_i + H_j, 2 (T_i + T_j) (and N1, N2)
// are added once, when a result is asked for (counts from the transposition kernel per block, het_settle_kernel at the
// end).  Plane 2 of the IBS / KING-robust counters therefore carries 2 ibs0 for EVERY block and backend (the halves do not
// separate per block); the finalisers shift.  Selected per block on the device (missing-call flag).
// Per-wave tile 128 x 64 with ONE wave per SIMD: the 2 x 8 x 16 = 256 accumulators live in AGPRs, 203 VGPRs hold the
// pipeline.  Against 64 x 64 at two waves per SIMD the decode drops from 6.3 to 4.75 VALU per MFMA (114 per 24 MFMAs), and
// with four word sets in flight (I8PipeSpread::D) the lone wave never waits for its loads: 5.19 -> 4.70 ms per 65 536-SNP
// block at N = 10 000 (A/B on one box; the same tile with two word sets: 5.05 ms).
#ifndef I8_NOMISS_TM
#define I8_NOMISS_TM 4
#define I8_NOMISS_WPS 1
#endif
// GCTA both-missing product: 128 x 128 per wave, one wave per SIMD (256 AGPR accumulators), operands straight from the
// masked words (I8ExtractMask): 7 VALU per operand dword, 3.5 per MFMA.  54 -> 37 ms per 16 384-SNP block at N = 100 000
// with 2 % missing calls (A/B on one box; the 128 x 64 / two-waves form with the same extraction: 70 ms -- its single code set
// aliases the operand registers the queued MFMAs still read).
#ifndef I8_GCTA_TN
#define I8_GCTA_TN 4
#define I8_GCTA_WPS 1
#endif
#ifndef I8_KING_TN
#define I8_KING_TN 2
#define I8_KING_WPS 2
#endif
template <> struct I8Scheme<PM_IBS_NOMISS> {
    static constexpr int NS = 2, NA = 2, TM = I8_NOMISS_TM, TN = 2, C = 3, WPS = I8_NOMISS_WPS;
    // slot 0: g.g' straight from the code bytes (no v_perm_b32: a block without missing calls holds the codes 0, 1, 2, and
    // 3 only as SNP / sample padding); slot 1: h.h'.  The code product comes FIRST: its MFMAs read the code registers of this
    // k-step, which the extraction of the k-step after next overwrites a whole product later
    static __device__ __forceinline__ constexpr uint32_t ta(int s) { return s == 0 ? I8T_CODE : I8T_H; }
    static __device__ __forceinline__ constexpr uint32_t tb(int s) { return s == 0 ? I8T_CODE : I8T_H; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    // a[0] = g.g' + 9 (padding SNPs of this K part), a[1] = h.h'.  {nvalid, ibs1 - H_i - H_j}; plane 2 gets h.h' + 9 pad
    // (atomic add) and - a[0] (global_atomic_sub) from the flush -- any arithmetic on the first accumulator there (a sum of
    // both, a negation) tipped the register allocator into spilling 85 registers, some inside the K loop
    static __device__ __forceinline__ void emit(const int *a, int nv, uint32_t *cnt)
    {
        cnt[0] = (uint32_t)nv; cnt[1] = 0u - 2u * (uint32_t)a[1]; cnt[2] = 0u;
    }
};
// GCTA denominators: both-missing counts over the masked words (code 3 = missing call at a polymorphic SNP
// of a real sample, launch_transpose2_missmask) -- one product, one accumulator.
template <> struct I8Scheme<PM_GCTA_MISS> {
    static constexpr int NS = 1, NA = 1, TM = 4, TN = I8_GCTA_TN, C = 1, WPS = I8_GCTA_WPS;
    static __device__ __forceinline__ constexpr uint32_t ta(int) { return I8T_M; }
    static __device__ __forceinline__ constexpr uint32_t tb(int) { return I8T_M; }
    static __device__ __forceinline__ constexpr int acc(int) { return 0; }
    static __device__ __forceinline__ void emit(const int *a, int, uint32_t *cnt) { cnt[0] = (uint32_t)a[0]; }
};
// KING-robust in the basis {y, h, x} (v = y + h): five products / five accumulators / three value types
//   a0 = y.y'  a1 = x.x'  a2 = y.h'  a3 = h.y'  a4 = h.h'
//   nLoci = a0 + a2 + a3 + a4   N1_Aa (row het, column called) = a3 + a4   N2_Aa = a2 + a4
//   ibs1 = a2 + a3   ibs0 = (a0 - a1) / 2
// (the direct form {v.v', h.v', v.h', h.h', y.y' - x.x'} needs six products and four value types)
template <> struct I8Scheme<PM_KING_ROBUST> {
    static constexpr int NS = 5, NA = 5, TM = 1, TN = I8_KING_TN, C = 5, WPS = I8_KING_WPS;
    static __device__ __forceinline__ constexpr uint32_t ta(int s) { return s == 0 ? I8T_Y : s == 1 ? I8T_X : s == 2 ? I8T_Y : I8T_H; }
    static __device__ __forceinline__ constexpr uint32_t tb(int s) { return s == 0 ? I8T_Y : s == 1 ? I8T_X : s == 2 ? I8T_H : s == 3 ? I8T_Y : I8T_H; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    static __device__ __forceinline__ void emit(const int *a, int, uint32_t *cnt)   // {nLoci, ibs1, 2 ibs0, N1_Aa, N2_Aa}
    {
        cnt[0] = (uint32_t)(a[0] + a[2] + a[3] + a[4]); cnt[1] = (uint32_t)(a[2] + a[3]);
        cnt[2] = (uint32_t)(a[0] - a[1]) /* 2 ibs0 */; cnt[3] = (uint32_t)(a[3] + a[4]); cnt[4] = (uint32_t)(a[2] + a[4]);
    }
};
template <> struct I8Scheme<PM_KING_HOMO> {      // 4 slots, 2 accumulators: 128 x 64 per wave at one wave per SIMD, as the binary kernel
    static constexpr int NS = 4, NA = 2, TM = 4, TN = 2, C = 2, WPS = 1;
    // ibs0 = e0.e2' + e2.e0' (binary operands, as in I8Scheme<PM_IBS>)
    static __device__ __forceinline__ constexpr uint32_t ta(int s) { return s == 0 ? I8T_H : s == 1 ? I8T_Y : s == 2 ? I8T_E0 : I8T_E2; }
    static __device__ __forceinline__ constexpr uint32_t tb(int s) { return s == 0 ? I8T_Y : s == 1 ? I8T_H : s == 2 ? I8T_E2 : I8T_E0; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s < 2 ? 0 : 1; }
    static __device__ __forceinline__ void emit(const int *a, int, uint32_t *cnt)   // {ibs1, 2 ibs0}
    {
        cnt[0] = (uint32_t)a[0]; cnt[1] = 2u * (uint32_t)a[1];
    }
};
// KING-homo, blocks without missing calls: the two products of I8Scheme<PM_IBS_NOMISS> into the planes {ibs1, 2 ibs0}
template <> struct I8Scheme<PM_HOMO_NOMISS> {
    static constexpr int NS = 2, NA = 2, TM = I8_NOMISS_TM, TN = 2, C = 2, WPS = I8_NOMISS_WPS;
    static __device__ __forceinline__ constexpr uint32_t ta(int s) { return s == 0 ? I8T_CODE : I8T_H; }
    static __device__ __forceinline__ constexpr uint32_t tb(int s) { return s == 0 ? I8T_CODE : I8T_H; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    static __device__ __forceinline__ void emit(const int *a, int, uint32_t *cnt)   // {ibs1 - H_i - H_j, 0} (+ h.h' + 9 pad - a[0] in the flush)
    {
        cnt[0] = 0u - 2u * (uint32_t)a[1]; cnt[1] = 0u;
    }
};
// individual beta: the three counters lie in the span of three symmetric rank-one products,
//   a0 = y.y' (both homozygous)   a1 = x.x' (equal - opposite homozygotes)   a2 = v.v' (both called)
//   num = a2   at least one het (both called) = a2 - a0   equal homozygotes = (a0 + a1) / 2
// (round 1 built the middle one from y.h' + h.y' + h.h': five products)
template <> struct I8Scheme<PM_BETA> {
    static constexpr int NS = 3, NA = 3, TM = 2, TN = 2, C = 3, WPS = 1;
    static __device__ __forceinline__ constexpr uint32_t ta(int s) { return s == 0 ? I8T_Y : s == 1 ? I8T_X : I8T_V; }
    static __device__ __forceinline__ constexpr uint32_t tb(int s) { return s == 0 ? I8T_Y : s == 1 ? I8T_X : I8T_V; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    static __device__ __forceinline__ void emit(const int *a, int, uint32_t *cnt)   // {num, >= one het, equal homozygotes}
    {
        cnt[0] = (uint32_t)a[2]; cnt[1] = (uint32_t)(a[2] - a[0]); cnt[2] = (uint32_t)(a[0] + a[1]) >> 1;
    }
};

__device__ __forceinline__ i32x4 i8_decode(uint32_t tbl, const uint32_t *e)
{
    i32x4 r;
#pragma unroll
    for (int u = 0; u < 4; u++) r[u] = (int)__builtin_amdgcn_perm(0u, tbl, e[u]);
    return r;
}

// The masked words of the GCTA denominators hold only the codes 0 and 3 ("missing call at a polymorphic SNP"): bit 0 of a
// code IS the int8 operand, so (w >> 2u) & 0x01010101 delivers four operand bytes and the v_perm_b32 table lookup falls
// away -- 7 instead of 11 VALU instructions per 16 SNPs (the kernel is VALU-issue-bound: 9.85 VALU per MFMA measured).
template <int MODE> struct I8ExtractMask { static constexpr uint32_t value = 0x03030303u; };
template <> struct I8ExtractMask<PM_GCTA_MISS> { static constexpr uint32_t value = 0x01010101u; };
template <int MODE> __device__ __forceinline__ i32x4 i8_decode_mode(uint32_t tbl, const uint32_t *e)
{
    if (MODE == PM_GCTA_MISS || tbl == I8T_CODE) {
        i32x4 r;
#pragma unroll
        for (int u = 0; u < 4; u++) r[u] = (int)e[u];
        return r;
    }
    return i8_decode(tbl, e);
}

// Software pipeline of one wave.  int8 MFMAs and VALU ops overlap on gfx950 (about 6 VALU ops hide
// behind one 32x32x32 MFMA, tools/ubench/coissue_ubench.hip), but only if the decode of the NEXT slot
// writes other registers than the queued MFMAs read: two operand register sets; slot s+1 is decoded
// while the MFMAs of slot s run, and the last slot of a k-step extracts the next k-step's codes.
// W2 has spare rows, so the words two k-steps ahead are loaded unconditionally.
template <int MODE> struct I8Pipe {
    typedef I8Scheme<MODE> S;
    static constexpr int TM = S::TM, TN = S::TN, NA = S::NA;
    // the operand register sets alternate per slot: an odd number of products is walked two k-steps at a time
    static constexpr int STEPS = (S::NS % 2 == 0) ? 1 : 2;
    const uint32_t *pa, *pb;
    int64_t kstride;
    uint32_t cw[TM + TN], e[TM + TN][4];
    i32x4 A[2][TM], B[2][TN];

    __device__ __forceinline__ void load_words()
    {
#pragma unroll
        for (int i = 0; i < TM; i++) cw[i] = pa[64 * i];
#pragma unroll
        for (int j = 0; j < TN; j++) cw[TM + j] = pb[64 * j];
        pa += kstride; pb += kstride;
    }
    __device__ __forceinline__ void extract()
    {
#pragma unroll
        for (int g = 0; g < TM + TN; g++)
#pragma unroll
            for (int u = 0; u < 4; u++) e[g][u] = (cw[g] >> (2 * u)) & I8ExtractMask<MODE>::value;
    }
    template <int SLOT, int SET> __device__ __forceinline__ void decode()
    {
#pragma unroll
        for (int i = 0; i < TM; i++) A[SET][i] = i8_decode_mode<MODE>(S::ta(SLOT), e[i]);
#pragma unroll
        for (int j = 0; j < TN; j++) B[SET][j] = i8_decode_mode<MODE>(S::tb(SLOT), e[TM + j]);
    }
    template <int P> __device__ __forceinline__ void phase(i32x16 (&c)[NA][TM][TN])
    {
        constexpr int s = P % S::NS;                     // product of this phase
        constexpr int cur = P & 1, nxt = cur ^ 1;
        constexpr bool last = (s == S::NS - 1);          // last product of a k-step
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
                c[S::acc(s)][i][j] =
                    __builtin_amdgcn_mfma_i32_32x32x32_i8(A[cur][i], B[cur][j], c[S::acc(s)][i][j], 0, 0, 0);
        if (last) {
            extract();
            load_words();
            decode<0, nxt>();
        } else {
            decode<last ? 0 : s + 1, nxt>();
        }
        // one MFMA, then a share of this phase's VALU work
        constexpr int dv = (MODE == PM_GCTA_MISS) ? 0 : 4;         // VALU ops per operand dword of a decode
        constexpr int nv = last ? (7 + dv) * (TM + TN) : dv * (TM + TN);
        constexpr int per = (nv + TM * TN - 1) / (TM * TN);
#pragma unroll
        for (int m = 0; m < TM * TN; m++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, per, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int... Is> __device__ __forceinline__ void kstep(i32x16 (&c)[NA][TM][TN], std::integer_sequence<int, Is...>)
    {
        (phase<Is>(c), ...);
    }
    __device__ __forceinline__ void prologue()
    {
        load_words();
        extract();
        load_words();
        decode<0, 0>();
    }
};

// The same pipeline with the code extraction of the NEXT k-step spread over the phases (row group g in phase g)
// instead of sitting in the last one: needs a second set of words and codes (4 (TM + TN) + (TM + TN) VGPRs) and
// at least TM + TN products.  Used where the register budget allows (KING-robust: 5 products, 3 row groups).
template <int MODE> struct I8PipeSpread {
    typedef I8Scheme<MODE> S;
    static constexpr int TM = S::TM, TN = S::TN, NA = S::NA, R = TM + TN;
    // D word sets: the words of k-step j + D are requested at the start of k-step j and first used (extracted) during
    // k-step j + D - 1.  Four sets: a wave that has its SIMD to itself (WPS == 1) must never wait for its loads (binary kernel
    // 5.05 -> 4.70 ms against two sets); with a second wave on the SIMD they still bought 1.6 % (KING-robust 9.11 -> 8.96 ms).
#ifndef I8_D2
#define I8_D2 4
#endif
    static constexpr int D = (S::WPS == 1) ? 4 : I8_D2;
    static constexpr int STEPS = D;                 // k-steps per loop round (even: the code sets alternate per k-step)
    // row group g is extracted in phase (g * NS) / R of the previous k-step
    const uint32_t *pa, *pb;
    int64_t kstride;
    uint32_t cw[D][R], e[2][R][4];
    i32x4 A[2][TM], B[2][TN];

    template <int K> __device__ __forceinline__ void load_words()
    {
#pragma unroll
        for (int i = 0; i < TM; i++) cw[K][i] = pa[64 * i];
#pragma unroll
        for (int j = 0; j < TN; j++) cw[K][TM + j] = pb[64 * j];
        pa += kstride; pb += kstride;
    }
    template <int W, int K, int G> __device__ __forceinline__ void extract_group()      // word set W -> code set K
    {
#pragma unroll
        for (int u = 0; u < 4; u++) e[K][G][u] = (cw[W][G] >> (2 * u)) & I8ExtractMask<MODE>::value;
    }
    template <int K, int SLOT, int SET> __device__ __forceinline__ void decode()
    {
#pragma unroll
        for (int i = 0; i < TM; i++) A[SET][i] = i8_decode_mode<MODE>(S::ta(SLOT), e[K][i]);
#pragma unroll
        for (int j = 0; j < TN; j++) B[SET][j] = i8_decode_mode<MODE>(S::tb(SLOT), e[K][TM + j]);
    }
    static constexpr int groups_in_phase(int s)
    {
        int n = 0;
        for (int g = 0; g < R; g++) n += ((g * S::NS) / R == s);
        return n;
    }
    template <int W, int K, int G, int PH> __device__ __forceinline__ void extract_if()
    {
        if ((G * S::NS) / R == PH) extract_group<W, K, G>();
    }
    template <int W, int K, int PH, int... Gs> __device__ __forceinline__ void extract_for_phase(std::integer_sequence<int, Gs...>)
    {
        (extract_if<W, K, Gs, PH>(), ...);
    }
    template <int P> __device__ __forceinline__ void phase(i32x16 (&c)[NA][TM][TN])
    {
        constexpr int s = P % S::NS, kj = P / S::NS;            // product, k-step of this loop round
        constexpr int kp = kj & 1, ws = kj % D;                 // code set / word set of this k-step
        constexpr int cur = P & 1, nxt = cur ^ 1;
        constexpr bool last = (s == S::NS - 1);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
                c[S::acc(s)][i][j] =
                    __builtin_amdgcn_mfma_i32_32x32x32_i8(A[cur][i], B[cur][j], c[S::acc(s)][i][j], 0, 0, 0);
        if (s == 0) load_words<ws>();                           // words D k-steps ahead (this k-step's are consumed)
        extract_for_phase<(ws + 1) % D, kp ^ 1, s>(std::make_integer_sequence<int, R>{});   // codes of the next k-step
        if (last) decode<kp ^ 1, 0, nxt>();
        else decode<kp, last ? 0 : s + 1, nxt>();
        constexpr int n_ext = groups_in_phase(s);
        constexpr int nv = 4 * R + 7 * n_ext;
        constexpr int per = (nv + TM * TN - 1) / (TM * TN);
#pragma unroll
        for (int m = 0; m < TM * TN; m++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, per, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int... Is> __device__ __forceinline__ void kstep(i32x16 (&c)[NA][TM][TN], std::integer_sequence<int, Is...>)
    {
        (phase<Is>(c), ...);
    }
    template <int... Gs> __device__ __forceinline__ void extract_all0(std::integer_sequence<int, Gs...>)
    {
        (extract_group<0, 0, Gs>(), ...);
    }
    template <int... Ks> __device__ __forceinline__ void load_rest(std::integer_sequence<int, Ks...>)
    {
        (load_words<Ks + 1>(), ...);
    }
    __device__ __forceinline__ void prologue()
    {
        load_words<0>();
        extract_all0(std::make_integer_sequence<int, R>{});
        load_rest(std::make_integer_sequence<int, D - 1>{});
        decode<0, 0, 0>();
    }
};
template <int MODE, bool SPREAD> struct I8PipeSel { typedef I8Pipe<MODE> type; };
template <int MODE> struct I8PipeSel<MODE, true> { typedef I8PipeSpread<MODE> type; };

// Workgroup = 4 waves as 2 x 2, tile (64 TM) x (64 TN).  Workgroup b executes work item b of a host-built
// list (worklist.h: build_worklist): {tile row, tile col, K part, K parts}; the list is interleaved so
// that the items of one XCD (b % 8) walk neighbouring tiles, and its tail holds K-split items so that the
// last, partially filled round of workgroups is short.  The flush is atomic, parts may share a tile.
template <int MODE>
__global__ __launch_bounds__(256, I8Scheme<MODE>::WPS) void pair_mfma_i8_kernel(
    const uint32_t *__restrict__ w2, int64_t ncols_pad, int n_q, int n_snp, uint32_t *__restrict__ acc, int64_t acc_plane,
    const int4 *__restrict__ work, const unsigned long long *__restrict__ d_missing, int run_if_missing)
{
    typedef I8Scheme<MODE> S;
    constexpr int TM = S::TM, TN = S::TN, NA = S::NA;
    if (d_missing && ((*d_missing != 0ull) != (run_if_missing != 0))) return;   // the other variant handles this block
    const int4 item = work[blockIdx.x];
    if (item.w == 0) return;
    struct { int tr, tc; } t = {item.x, item.y};
    typedef typename I8PipeSel<MODE, (MODE == PM_KING_ROBUST || MODE == PM_KING_HOMO || MODE == PM_IBS_NOMISS || MODE == PM_HOMO_NOMISS || MODE == PM_BETA ||
                                      (MODE == PM_GCTA_MISS && I8Scheme<MODE>::WPS == 1))>::type Pipe;
    constexpr int KR = Pipe::STEPS > 2 ? Pipe::STEPS : 2;            // k-steps per loop round (n_q is a multiple of 4: blocks are padded to 128 SNPs)
    const int per = (((n_q + item.w - 1) / item.w) + KR - 1) / KR * KR;   // (inline: k_part changes the code of <PM_IBS>)
    const int q_beg = item.z * per;
    const int q_end = (q_beg + per < n_q) ? (q_beg + per) : n_q;
    if (q_beg >= q_end) return;

    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int row_base = t.tr * (64 * TM) + wr * (32 * TM);
    const int64_t col_base = (int64_t)t.tc * (64 * TN) + wc * (32 * TN);
    // W2 = uint2[row pair = k-step][sample]: the halves of a k-step lie side by side (lane half kh takes element kh)
    const uint32_t *__restrict__ pa = w2 + 2 * ((int64_t)q_beg * ncols_pad + row_base + li) + kh;
    const uint32_t *__restrict__ pb = w2 + 2 * ((int64_t)q_beg * ncols_pad + col_base + li) + kh;
    const int64_t kstride = 2 * ncols_pad;

    i32x16 c[NA][TM][TN];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) c[a][i][j][r] = 0;

    // Software pipeline (I8Pipe): slot s+1 is decoded while the MFMAs of slot s run.
    Pipe pipe;
    pipe.pa = pa; pipe.pb = pb; pipe.kstride = kstride;
    pipe.prologue();
    for (int q = q_beg; q < q_end; q += Pipe::STEPS)                // q_end - q_beg is a multiple of KR
        pipe.kstep(c, std::make_integer_sequence<int, S::NS * Pipe::STEPS>{});
    // real SNPs of this K part (both-called count of a block without missing calls)
    const int nv_lo = 32 * q_beg, nv_hi = (32 * q_end < n_snp) ? 32 * q_end : n_snp;
    const int nv = (nv_hi > nv_lo) ? (nv_hi - nv_lo) : 0;
    const int pad9 = 9 * (32 * (q_end - q_beg) - nv);      // code product of the padding SNPs of this K part (code 3 x code 3)
    (void)pad9;
    // C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    // One owner per element and K slice: fire-and-forget atomic adds (measured against streaming
    // load/add/store updates of the HBM-resident counters, tools/ubench/i8_ubench.hip: atomics cost 4.5 %
    // of an IBS launch at N = 10 000, B = 16 384, the load/store form 6.5 %).
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
            uint32_t *p0 = tile32_counter0(acc, ncols_pad, row_base, col_base, i, j, li, kh);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int a[NA];
                uint32_t cnt[S::C];
#pragma unroll
                for (int k = 0; k < NA; k++) a[k] = c[k][i][j][r];
                S::emit(a, nv, cnt);
                uint32_t *p = tile32_counter(p0, ncols_pad, r);
#pragma unroll
                for (int k = 0; k < S::C; k++) {
                    if ((MODE == PM_IBS_NOMISS && k == 2) || (MODE == PM_HOMO_NOMISS && k == 1)) continue;   // below
                    atomicAdd(p + (int64_t)k * acc_plane, cnt[k]);
                }
                if (MODE == PM_IBS_NOMISS || MODE == PM_HOMO_NOMISS) {    // 2 ibs0 += h.h' - g.g' (+ the rank-one terms at settle time)
                    uint32_t *p0 = p + (MODE == PM_IBS_NOMISS ? 2 : 1) * acc_plane;
                    atomicAdd(p0, (uint32_t)(a[1] + pad9));
                    asm volatile("global_atomic_sub %0, %1, off" : : "v"(p0), "v"(a[0]) : "memory");
                }
            }
        }
}

template <int MODE>
static int launch_i8(hipStream_t st, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad, int n_q,
                     int n_snp, uint32_t *acc, int64_t acc_plane, const unsigned long long *d_missing, int run_if_missing)
{
    hipLaunchKernelGGL(pair_mfma_i8_kernel<MODE>, dim3((unsigned)n_blocks), dim3(256), 0, st, w2, ncols_pad, n_q, n_snp,
                       acc, acc_plane, work, d_missing, run_if_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// GCTA both-missing counts on the MX-fp4 matrix instruction (round 4).  The masked words hold only the codes 0 and 3, so bit 1 of
// a code, left where it is, IS an e2m1 nibble: 0b0010 = 1.0 (0b0000 = 0).  One 16-code word gives two operand dwords of eight
// nibbles -- w & 0x22222222 (even SNPs) and (w >> 2) & 0x22222222 (odd SNPs); any SNP order inside a k-step is legal, both
// operands use the same one -- three VALU per two dwords.  v_mfma_scale_f32_32x32x64_f8f6f4 with both formats fp4 (cbsz = blgp = 4)
// and unit E8M0 scales (0x7F) takes 64 SNPs x 1024 pairs per instruction at twice the int8 rate (MI355X_MICROARCH.md: 9099 TF against
// 4404 TOP/s); the products are 0 or 1 and the fp32 sums exact (a launch holds <= 2^16 SNPs < 2^24).  Same tile, work list
// and flush as pair_mfma_i8_kernel<PM_GCTA_MISS>: 128 x 128 per wave in AGPRs, one wave per SIMD, four word sets in flight.
// Lane l: sample l & 31, SNPs 32 (l >> 5) ... + 32 of the k-step = the word rows 4 s + 2 (l >> 5) + {0, 1}.
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// The genotype words of the three MX-fp4 pipes: D sets in flight for TM row and TN column groups of a wave.
template <int TM, int TN> struct Fp4Words {
    static constexpr int R = TM + TN, D = 4;
    // the word PAIRS of a sample lie side by side (launch_transpose2_missmask, paired): one 8-byte load per 32 SNPs, 32 loads in
    // flight with four sets (64 single-word loads overran the 6-bit vmcnt counter: the compiler then waited for loads it had just
    // issued).  Uniform base (SGPRs, advanced per k-step) + one constant byte offset per lane and operand.
    const char *base;
    uint32_t offa, offb;
    int64_t kstride;
    uint2 cw[D][R];

    // an operand of the MX-fp4 MFMA: the instruction reads eight dwords, fp4 data fill the first four
    static __device__ __forceinline__ i32x8 wide(const i32x4 v) { return __builtin_shufflevector(v, v, 0, 1, 2, 3, -1, -1, -1, -1); }
    template <int K> __device__ __forceinline__ void load_words()
    {
        // raw buffer loads: descriptor = the uniform row address (SGPRs, rebuilt per k-step with scalar adds), lane offset in ONE
        // VGPR.  (Flat loads from base + offset kept 64-bit lane addresses alive across the loop; the allocator spilled them and
        // every reload -- scratch counts in vmcnt -- drained the four word sets in flight.)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, 0x7FFFFFFF, 0x00020000);
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(offa + 256 * i), 0, 0);
            cw[K][i] = make_uint2(v[0], v[1]);
        }
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(offb + 256 * j), 0, 0);
            cw[K][TM + j] = make_uint2(v[0], v[1]);
        }
        base += kstride;
    }
};

struct Fp4MissPipe : Fp4Words<4, 4> {
    static constexpr int TM = 4, TN = 4;
    i32x4 A[2][TM], B[2][TN];

    static __device__ __forceinline__ i32x4 nibbles(const uint2 w)
    {
        i32x4 r;
        r[0] = (int)(w.x & 0x22222222u); r[1] = (int)((w.x >> 2) & 0x22222222u);
        r[2] = (int)(w.y & 0x22222222u); r[3] = (int)((w.y >> 2) & 0x22222222u);
        return r;
    }
    template <int K, int SET> __device__ __forceinline__ void decode()
    {
#pragma unroll
        for (int i = 0; i < TM; i++) A[SET][i] = nibbles(cw[K][i]);
#pragma unroll
        for (int j = 0; j < TN; j++) B[SET][j] = nibbles(cw[K][TM + j]);
    }
    template <int J> __device__ __forceinline__ void step(f32x16 (&c)[TM][TN])
    {
        constexpr int cur = J & 1, nxt = cur ^ 1;
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++) {
                c[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(A[cur][i]), wide(B[cur][j]), c[i][j], 4, 4, 0, 0, 0, 0);   // scale operands 0: the unscaled, single instruction
            }
        decode<(J + 1) % D, nxt>();        // the next k-step's operands while this one's MFMAs run
        load_words<J % D>();               // words D k-steps ahead (this k-step's were decoded a step ago)
#pragma unroll
        for (int m = 0; m < TM * TN; m++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
            if (m % 2 == 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void prologue()
    {
        load_words<0>(); load_words<1>(); load_words<2>(); load_words<3>();
        decode<0, 0>();
    }
};

__global__ __launch_bounds__(256, 1) void pair_mfma_fp4_miss_kernel(
    const uint32_t *__restrict__ w2, int64_t ncols_pad, int n_s, uint32_t *__restrict__ acc, const int4 *__restrict__ work,
    const unsigned long long *__restrict__ d_missing, int run_if_missing)
{
    typedef Fp4MissPipe P;
    if (d_missing && ((*d_missing != 0ull) != (run_if_missing != 0))) return;
    const int4 item = work[blockIdx.x];
    if (item.w == 0) return;
    const auto [s_beg, s_end] = k_part<true>(0, n_s, item.z, item.w, P::D);    // n_s is a multiple of D (blocks padded to 256 SNPs)
    if (s_beg >= s_end) return;
    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int row_base = item.x * (64 * P::TM) + wr * (32 * P::TM);
    const int64_t col_base = (int64_t)item.y * (64 * P::TN) + wc * (32 * P::TN);
    P pipe;
    // pair row 2 s + kh of k-step s; a row of pairs is 8 ncols_pad bytes (< 2^31 for every panel that fits a GPU)
    pipe.base = reinterpret_cast<const char *>(w2) + (int64_t)(2 * s_beg) * ncols_pad * 8;
    pipe.offa = (uint32_t)(((int64_t)kh * ncols_pad + row_base + li) * 8);
    pipe.offb = (uint32_t)(((int64_t)kh * ncols_pad + col_base + li) * 8);
    pipe.kstride = 2 * ncols_pad * 8;
    f32x16 c[P::TM][P::TN];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) c[i][j][r] = 0.f;
    pipe.prologue();
    for (int s = s_beg; s < s_end; s += P::D) {
        pipe.step<0>(c); pipe.step<1>(c); pipe.step<2>(c); pipe.step<3>(c);
    }
    // the sums leave the loop IN the accumulation registers: without this the allocator split their live ranges at the loop
    // latch and copied 85 of them to scratch in every round
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++) asm volatile("" : "+a"(c[i][j]));
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++) {
            uint32_t *p0 = tile32_counter0(acc, ncols_pad, row_base, col_base, i, j, li, kh);
#pragma unroll
            for (int r = 0; r < 16; r++)
                atomicAdd(tile32_counter(p0, ncols_pad, r), (uint32_t)c[i][j][r]);
        }
}

// ---------------------------------------------------------------------------
// IBS / KING counters of blocks WITHOUT missing calls on the MX-fp4 MFMA (round 4): the two products of I8Scheme<PM_IBS_NOMISS>,
// g.g' and h.h', with e2m1 operands.  A 2-bit code, left where it is, IS the nibble of g / 2 (0b0000 = 0, 0b0001 = 0.5,
// 0b0010 = 1, 0b0011 = 1.5), and in a block without missing calls bit 0 of a code is the het indicator (codes 0, 1, 2; 3 only as
// SNP / sample padding), i.e. the nibble 0.5 h.  Round 6: the UNSCALED instruction (scale operands 0: one issue slot instead of the v_mfma_ld_scale + v_mfma
// pair; +2 ... 5 % on every fp4 kernel) sums g g' / 4 and h h' / 4 -- multiples of 1/4 below 2^18, exact in fp32 -- and the flush multiplies by 4.
// Decode per 16-code word: w & 0x33333333, (w >> 2) & 0x33333333 (g, even / odd SNPs), w & 0x11111111, (w >> 2) & 0x11111111
// (h) -- five VALU per word for both products, 3.75 per MFMA (int8 form: 4.75), and every MFMA takes 64 SNPs instead of 32.
// Padding SNPs (code 3 for every sample) add 9 to g.g' (as in the int8 form) and 1 to h.h': constants of the K part, put
// back by the flush.  Sums exact in fp32 (<= 9 x 2^16 per launch).  Tile, work list, planes and rank-one terms as I8Scheme<PM_IBS_NOMISS>.
struct Fp4NomissPipe : Fp4Words<4, 2> {
    static constexpr int TM = 4, TN = 2;
    i32x4 G[2][R], H[2][R];

    template <int K, int SET> __device__ __forceinline__ void decode()
    {
#pragma unroll
        for (int g = 0; g < R; g++) {
            const uint32_t x = cw[K][g].x, y = cw[K][g].y, xs = x >> 2, ys = y >> 2;
            G[SET][g][0] = (int)(x & 0x33333333u); G[SET][g][1] = (int)(xs & 0x33333333u);
            G[SET][g][2] = (int)(y & 0x33333333u); G[SET][g][3] = (int)(ys & 0x33333333u);
            H[SET][g][0] = (int)(x & 0x11111111u); H[SET][g][1] = (int)(xs & 0x11111111u);
            H[SET][g][2] = (int)(y & 0x11111111u); H[SET][g][3] = (int)(ys & 0x11111111u);
        }
    }
    template <int J> __device__ __forceinline__ void step(f32x16 (&cg)[TM][TN], f32x16 (&ch)[TM][TN])
    {
        constexpr int cur = J & 1, nxt = cur ^ 1;
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
                cg[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(G[cur][i]), wide(G[cur][TM + j]), cg[i][j], 4, 4, 0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
                ch[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(H[cur][i]), wide(H[cur][TM + j]), ch[i][j], 4, 4, 0, 0, 0, 0);
        decode<(J + 1) % D, nxt>();
        load_words<J % D>();
#pragma unroll
        for (int m = 0; m < 2 * TM * TN; m++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            if (m % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void prologue()
    {
        load_words<0>(); load_words<1>(); load_words<2>(); load_words<3>();
        decode<0, 0>();
    }
};

template <int MODE>
__global__ __launch_bounds__(256, 1) void pair_mfma_fp4_nomiss_kernel(
    const uint32_t *__restrict__ w2, int64_t ncols_pad, int n_s, int n_snp, uint32_t *__restrict__ acc, int64_t acc_plane,
    const int4 *__restrict__ work, const unsigned long long *__restrict__ d_missing)
{
    typedef Fp4NomissPipe P;
    if (*d_missing != 0ull) return;                    // the general kernel takes blocks with missing calls
    const int4 item = work[blockIdx.x];
    if (item.w == 0) return;
    const auto [s_beg, s_end] = k_part<true>(0, n_s, item.z, item.w, P::D);    // n_s is a multiple of D (blocks padded to 256 SNPs)
    if (s_beg >= s_end) return;
    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int row_base = item.x * (64 * P::TM) + wr * (32 * P::TM);
    const int64_t col_base = (int64_t)item.y * (64 * P::TN) + wc * (32 * P::TN);
    P pipe;
    pipe.base = reinterpret_cast<const char *>(w2) + (int64_t)(2 * s_beg) * ncols_pad * 8;
    pipe.offa = (uint32_t)(((int64_t)kh * ncols_pad + row_base + li) * 8);
    pipe.offb = (uint32_t)(((int64_t)kh * ncols_pad + col_base + li) * 8);
    pipe.kstride = 2 * ncols_pad * 8;
    f32x16 cg[P::TM][P::TN], ch[P::TM][P::TN];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) { cg[i][j][r] = 0.f; ch[i][j][r] = 0.f; }
    pipe.prologue();
    for (int s = s_beg; s < s_end; s += P::D) {
        pipe.step<0>(cg, ch); pipe.step<1>(cg, ch); pipe.step<2>(cg, ch); pipe.step<3>(cg, ch);
    }
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++) { asm volatile("" : "+a"(cg[i][j])); asm volatile("" : "+a"(ch[i][j])); }
    const int nv_lo = 64 * s_beg, nv_hi = (64 * s_end < n_snp) ? 64 * s_end : n_snp;
    const int nv = (nv_hi > nv_lo) ? (nv_hi - nv_lo) : 0;         // real SNPs of this K part = both-called count of every pair
    const int npad = 64 * (s_end - s_beg) - nv;                   // padding SNPs: 9 each in g.g', 1 each in h.h'
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++) {
            uint32_t *p0 = tile32_counter0(acc, ncols_pad, row_base, col_base, i, j, li, kh);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                uint32_t *p = tile32_counter(p0, ncols_pad, r);
                const int gg = (int)(4.0f * cg[i][j][r]);         // g.g' + 9 npad  (unscaled products of g / 2, h / 2: x 4, exact)
                const int hh = (int)(4.0f * ch[i][j][r]) - npad;  // h.h'
                if (MODE == PM_IBS_NOMISS) {                      // {n, ibs1 - H_i - H_j, 2 ibs0 - 2 (T_i + T_j)} (+ rank-one terms at settle time)
                    atomicAdd(p, (uint32_t)nv);
                    atomicAdd(p + acc_plane, 0u - 2u * (uint32_t)hh);
                    atomicAdd(p + 2 * acc_plane, (uint32_t)(hh + 9 * npad - gg));
                } else if (MODE == PM_DISS) {                     // {SumGeno - 2 (S_i + S_j)}: - 2 g.g' (+ the rank-one terms at settle time)
                    atomicAdd(p, 0u - 2u * (uint32_t)(gg - 9 * npad));
                } else {                                          // PM_HOMO_NOMISS: {ibs1 - H_i - H_j, 2 ibs0 - ...}
                    atomicAdd(p, 0u - 2u * (uint32_t)hh);
                    atomicAdd(p + acc_plane, (uint32_t)(hh + 9 * npad - gg));
                }
            }
        }
}

template <int MODE>
static int launch_fp4_nomiss(hipStream_t st, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad, int n_s, int n_snp,
                             uint32_t *acc, int64_t acc_plane, const unsigned long long *d_missing)
{
    if (n_s <= 0 || n_blocks <= 0) return 0;
    // (round 6: a 16x16x128 form of this kernel -- 8 x 4 sub-tiles, het operands made in place, two VALU behind every MFMA -- was built,
    // bit-exact, and measured: K loop 1.70 ms per 65 536-SNP block at N = 10 000 against 1.68, and a flush of 4 x 64-byte pieces per
    // atomic instruction that costs 0.56 ms against 0.23; not kept -- profiles/r06_fp4_16x16x128_ab.txt)
    hipLaunchKernelGGL(pair_mfma_fp4_nomiss_kernel<MODE>, dim3((unsigned)n_blocks), dim3(256), 0, st, w2, ncols_pad, n_s, n_snp, acc,
                       acc_plane, work, d_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// The general IBS / KING-robust counters (blocks WITH missing calls) on the MX-fp4 MFMA (round 4): the products of
// I8Scheme<PM_IBS> / <PM_KING_ROBUST> with e2m1 operands built by bit logic instead of v_perm_b32 table lookups.  Per nibble (one
// SNP; code bits b1 b0, x = the word or the word >> 2, t = x >> 1, M = 0x11111111):
//     P = x & M (b0)    m = P & t (missing)    v = M ^ m (called)    h = P ^ m (het)    y = M ^ P (homozygous, called)
//     e2 = t & y (g == 2)     s = v | h << 3  (= +-1/2: v - 2 h)      x = y | e2 << 3  (= +-1/2: [g == 0] - [g == 2])
// (bit 0 of a nibble = 1/2, bit 3 = the sign; unscaled instruction, the flush multiplies the sums of quarter products by 4), 7 / 9 VALU per eight SNPs for KING's three /
// IBS's four value types.  One wave per SIMD, operand sets double-buffered, four word sets in flight; every MFMA takes 64 SNPs.
//   IBS   64 x 64 per wave: v.v', s.s', y.y', x.x' -> {nvalid, ibs1 = (nvalid - s.s') / 2, 2 ibs0 = y.y' - x.x'}
//   KING  32 x 64 per wave: y.y', x.x', y.h', h.y', h.h' -> the five counters as I8Scheme<PM_KING_ROBUST>::emit
// Sums exact in fp32 (|sum| <= 2^16 per launch).
template <int MODE> struct Fp4Scheme;
// types(x, t, x2, x3, o): x = the word or the word >> 2 (code bits b1 b0 at the nibble's bits 1 0), t = x >> 1 (b1 at bit 0),
// x2 = x << 2 (b1 at bit 3), x3 = x << 3 (b0 at bit 3); M = bit 0, M8 = bit 3 of every nibble.  The sign bit of a nibble whose
// magnitude is 0 is free (-0 = 0), so s takes b0 and x takes b1 as sign without masking them by "called" / "homozygous":
// every value type is ONE three-input boolean instruction (v_bitop3_b32) on top of the shifts.
template <> struct Fp4Scheme<PM_IBS> {
    static constexpr int NS = 4, NA = 4, NT = 4, TM = 2, TN = 2, C = 3, WPS = 1;
    static constexpr bool NEED_X3 = true;
    static __device__ __forceinline__ constexpr int ta(int s) { return s; }
    static __device__ __forceinline__ constexpr int tb(int s) { return s; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    static __device__ __forceinline__ void types(uint32_t x, uint32_t t, uint32_t x2, uint32_t x3, int (&o)[NT])   // {v, s, y, x}
    {
        const uint32_t M = 0x11111111u, M8 = 0x88888888u, v = M & ~(x & t), y = M & ~x;
        o[0] = (int)v; o[1] = (int)(v | (x3 & M8)); o[2] = (int)y; o[3] = (int)(y | (x2 & M8));
    }
    static __device__ __forceinline__ void emit(const int *a, uint32_t *cnt)         // {nvalid, ibs1, 2 ibs0}
    {
        cnt[0] = (uint32_t)a[0]; cnt[1] = (uint32_t)(a[0] - a[1]) >> 1; cnt[2] = (uint32_t)(a[2] - a[3]);
    }
};
template <> struct Fp4Scheme<PM_KING_ROBUST> {
    static constexpr int NS = 5, NA = 5, NT = 3, TM = 1, TN = 2, C = 5;
#ifndef FP4_KING_WPS
#define FP4_KING_WPS 1     /* 2: 128 + 128 registers, 296 bytes of scratch, 62 instead of 5.5 ms */
#endif
    static constexpr int WPS = FP4_KING_WPS;
    static constexpr bool NEED_X3 = false;
    static __device__ __forceinline__ constexpr int ta(int s) { return s == 0 ? 0 : s == 1 ? 1 : s == 2 ? 0 : 2; }   // y x y h h
    static __device__ __forceinline__ constexpr int tb(int s) { return s == 0 ? 0 : s == 1 ? 1 : s == 2 ? 2 : s == 3 ? 0 : 2; }   // y x h y h
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    static __device__ __forceinline__ void types(uint32_t x, uint32_t t, uint32_t x2, uint32_t, int (&o)[NT])        // {y, x, h}
    {
        const uint32_t M = 0x11111111u, M8 = 0x88888888u, y = M & ~x;
        o[0] = (int)y; o[1] = (int)(y | (x2 & M8)); o[2] = (int)(M & x & ~t);
    }
    static __device__ __forceinline__ void emit(const int *a, uint32_t *cnt)         // {nLoci, ibs1, 2 ibs0, N1_Aa, N2_Aa}
    {
        cnt[0] = (uint32_t)(a[0] + a[2] + a[3] + a[4]); cnt[1] = (uint32_t)(a[2] + a[3]);
        cnt[2] = (uint32_t)(a[0] - a[1]); cnt[3] = (uint32_t)(a[3] + a[4]); cnt[4] = (uint32_t)(a[2] + a[4]);
    }
};

// individual beta: y.y', x.x', v.v' -> {num = v.v', at least one het = v.v' - y.y', equal homozygotes = (y.y' + x.x') / 2}
template <> struct Fp4Scheme<PM_BETA> {
    static constexpr int NS = 3, NA = 3, NT = 3, TM = 2, TN = 2, C = 3, WPS = 1;
    static constexpr bool NEED_X3 = false;
    static __device__ __forceinline__ constexpr int ta(int s) { return s; }
    static __device__ __forceinline__ constexpr int tb(int s) { return s; }
    static __device__ __forceinline__ constexpr int acc(int s) { return s; }
    static __device__ __forceinline__ void types(uint32_t x, uint32_t t, uint32_t x2, uint32_t, int (&o)[NT])        // {y, x, v}
    {
        const uint32_t M = 0x11111111u, M8 = 0x88888888u, y = M & ~x;
        o[0] = (int)y; o[1] = (int)(y | (x2 & M8)); o[2] = (int)(M & ~(x & t));
    }
    static __device__ __forceinline__ void emit(const int *a, uint32_t *cnt)
    {
        cnt[0] = (uint32_t)a[2]; cnt[1] = (uint32_t)(a[2] - a[0]); cnt[2] = (uint32_t)(a[0] + a[1]) >> 1;
    }
};

// KING-homo (blocks with missing calls): h.y' + y.h' = ibs1 in ONE accumulator, y.y' and x.x' -> 2 ibs0 = y.y' - x.x'
template <> struct Fp4Scheme<PM_KING_HOMO> {
    static constexpr int NS = 4, NA = 3, NT = 3, TM = 2, TN = 2, C = 2, WPS = 1;
    static constexpr bool NEED_X3 = false;
    static __device__ __forceinline__ constexpr int ta(int s) { return s == 0 ? 2 : s == 1 ? 0 : s == 2 ? 0 : 1; }   // h y y x
    static __device__ __forceinline__ constexpr int tb(int s) { return s == 0 ? 0 : s == 1 ? 2 : s == 2 ? 0 : 1; }   // y h y x
    static __device__ __forceinline__ constexpr int acc(int s) { return s < 2 ? 0 : s - 1; }
    static __device__ __forceinline__ void types(uint32_t x, uint32_t t, uint32_t x2, uint32_t, int (&o)[NT])        // {y, x, h}
    {
        const uint32_t M = 0x11111111u, M8 = 0x88888888u, y = M & ~x;
        o[0] = (int)y; o[1] = (int)(y | (x2 & M8)); o[2] = (int)(M & x & ~t);
    }
    static __device__ __forceinline__ void emit(const int *a, uint32_t *cnt)         // {ibs1, 2 ibs0}
    {
        cnt[0] = (uint32_t)a[0]; cnt[1] = (uint32_t)(a[1] - a[2]);
    }
};

// individual dissimilarity (blocks with missing calls): a = g / 2 and b = (2 - g) / 2, both 0 where the call is missing, and the two
// products a.b' + b.a' into ONE accumulator: the sum of g (2 - g') + (2 - g) g' / 4 over the SNPs both samples are called at, so the
// flush's x 4 gives SumGeno itself (terms <= 1 per SNP and pair in quarters: < 2^18 per launch, exact in fp32).  With the het
// indicator h (bit 0 = 1/2), e2 = [g == 2] and e0 = [g == 0] at bit 0: a = h | e2 << 1 (1/2 or 1), b = h | e0 << 1; h, e2, e0 are
// one v_bitop3_b32 each, the two ORs one v_lshl_or_b32 each.  2 MFMAs per 64 SNPs (the KING-robust counters: 5); 128 x 128 per wave
// in AGPRs (one accumulator), so that the decode of the two value types is shared by twice the MFMAs of a 128 x 64 tile.
template <> struct Fp4Scheme<PM_DISS> {
#ifndef FP4_DISS_TN
#define FP4_DISS_TN 4
#endif
    static constexpr int NS = 2, NA = 1, NT = 2, TM = 4, TN = FP4_DISS_TN, C = 1, WPS = 1;
    static constexpr bool NEED_X3 = false;
    static __device__ __forceinline__ constexpr int ta(int s) { return s; }         // a b
    static __device__ __forceinline__ constexpr int tb(int s) { return 1 - s; }     // b a
    static __device__ __forceinline__ constexpr int acc(int) { return 0; }
    static __device__ __forceinline__ void types(uint32_t x, uint32_t t, uint32_t, uint32_t, int (&o)[NT])         // {a, b}
    {
        const uint32_t M = 0x11111111u, h = M & x & ~t, e2 = M & t & ~x, e0 = M & ~(x | t);
        o[0] = (int)(h | (e2 << 1)); o[1] = (int)(h | (e0 << 1));
    }
    static __device__ __forceinline__ void emit(const int *a, uint32_t *cnt) { cnt[0] = (uint32_t)a[0]; }     // {SumGeno}
};

template <int MODE> struct Fp4GenPipe : Fp4Words<Fp4Scheme<MODE>::TM, Fp4Scheme<MODE>::TN> {
    typedef Fp4Scheme<MODE> S;
    typedef Fp4Words<S::TM, S::TN> W;
    using W::cw; using W::R; using W::D; using W::wide;
    static constexpr int TM = S::TM, TN = S::TN, NT = S::NT, NS = S::NS, NA = S::NA;
    i32x4 V[2][R][NT];

    // decode unit U = (row group U / 2, word U % 2): 16 SNPs -> dwords 2 (U % 2) and 2 (U % 2) + 1 of every value type
    template <int K, int SET, int U> __device__ __forceinline__ void decode_unit()
    {
        constexpr int g = U / 2, hw = U % 2;
        const uint32_t w = hw ? cw[K][g].y : cw[K][g].x;
        int o[NT];
        S::types(w, w >> 1, w << 2, S::NEED_X3 ? (w << 3) : 0u, o);            // even SNPs of the word
#pragma unroll
        for (int t = 0; t < NT; t++) V[SET][g][t][2 * hw] = o[t];
        S::types(w >> 2, w >> 3, w, S::NEED_X3 ? (w << 1) : 0u, o);            // odd SNPs
#pragma unroll
        for (int t = 0; t < NT; t++) V[SET][g][t][2 * hw + 1] = o[t];
    }
    template <int K, int SET, int U0, int U1> __device__ __forceinline__ void decode_units()
    {
        if constexpr (U0 < U1) { decode_unit<K, SET, U0>(); decode_units<K, SET, U0 + 1, U1>(); }
    }
    template <int K, int SET> __device__ __forceinline__ void decode() { decode_units<K, SET, 0, 2 * R>(); }
    // phase PH of k-step J: the MFMAs of product PH, a share of the next k-step's decode units (and, in phase 0, the word loads
    // D k-steps ahead); a scheduling barrier per phase keeps the VALU work spread under the MFMAs
    template <int J, int PH> __device__ __forceinline__ void phase(f32x16 (&c)[NA][TM][TN])
    {
        constexpr int cur = J & 1, nxt = cur ^ 1;
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
                c[S::acc(PH)][i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(V[cur][i][S::ta(PH)]), wide(V[cur][TM + j][S::tb(PH)]),
                                                                                     c[S::acc(PH)][i][j], 4, 4, 0, 0, 0, 0);
        constexpr int u0 = PH * 2 * R / NS, u1 = (PH + 1) * 2 * R / NS;
        decode_units<(J + 1) % D, nxt, u0, u1>();
        if (PH == 0) this->template load_words<J % D>();
        constexpr int n_valu = (u1 - u0) * (S::NEED_X3 ? 14 : 10);
        constexpr int per = (n_valu + TM * TN - 1) / (TM * TN);
#pragma unroll
        for (int m = 0; m < TM * TN; m++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, per, 0);
            if (PH == 0) __builtin_amdgcn_sched_group_barrier(0x020, (R + TM * TN - 1) / (TM * TN), 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int J, int PH> __device__ __forceinline__ void phases(f32x16 (&c)[NA][TM][TN])
    {
        if constexpr (PH < NS) { phase<J, PH>(c); phases<J, PH + 1>(c); }
    }
    template <int J> __device__ __forceinline__ void step(f32x16 (&c)[NA][TM][TN]) { phases<J, 0>(c); }
    __device__ __forceinline__ void prologue()
    {
        this->template load_words<0>(); this->template load_words<1>(); this->template load_words<2>(); this->template load_words<3>();
        decode<0, 0>();
    }
};

template <int MODE>
__global__ __launch_bounds__(256, Fp4Scheme<MODE>::WPS) void pair_mfma_fp4_kernel(
    const uint32_t *__restrict__ w2, int64_t ncols_pad, int n_s, uint32_t *__restrict__ acc, int64_t acc_plane,
    const int4 *__restrict__ work, const unsigned long long *__restrict__ d_missing)
{
    typedef Fp4GenPipe<MODE> P;
    typedef Fp4Scheme<MODE> S;
    if (d_missing && *d_missing == 0ull) return;       // the two-product kernel takes blocks without missing calls
    const int4 item = work[blockIdx.x];
    if (item.w == 0) return;
    const auto [s_beg, s_end] = k_part<true>(0, n_s, item.z, item.w, P::D);    // n_s is a multiple of D (blocks padded to 256 SNPs)
    if (s_beg >= s_end) return;
    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const int row_base = item.x * (64 * P::TM) + wr * (32 * P::TM);
    const int64_t col_base = (int64_t)item.y * (64 * P::TN) + wc * (32 * P::TN);
    P pipe;
    pipe.base = reinterpret_cast<const char *>(w2) + (int64_t)(2 * s_beg) * ncols_pad * 8;
    pipe.offa = (uint32_t)(((int64_t)kh * ncols_pad + row_base + li) * 8);
    pipe.offb = (uint32_t)(((int64_t)kh * ncols_pad + col_base + li) * 8);
    pipe.kstride = 2 * ncols_pad * 8;
    f32x16 c[P::NA][P::TM][P::TN];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int a = 0; a < P::NA; a++)
#pragma unroll
        for (int i = 0; i < P::TM; i++)
#pragma unroll
            for (int j = 0; j < P::TN; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) c[a][i][j][r] = 0.f;
    pipe.prologue();
    for (int s = s_beg; s < s_end; s += P::D) {
        pipe.template step<0>(c); pipe.template step<1>(c); pipe.template step<2>(c); pipe.template step<3>(c);
    }
#pragma unroll
    for (int a = 0; a < P::NA; a++)
#pragma unroll
        for (int i = 0; i < P::TM; i++)
#pragma unroll
            for (int j = 0; j < P::TN; j++) asm volatile("" : "+a"(c[a][i][j]));
#pragma unroll
    for (int i = 0; i < P::TM; i++)
#pragma unroll
        for (int j = 0; j < P::TN; j++) {
            // (inline: tile32_counter0 / tile32_counter change the code of <PM_KING_ROBUST>)
            uint32_t *p0 = acc + (int64_t)(row_base + 32 * i + 4 * kh) * ncols_pad + col_base + 32 * j + li;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int a[P::NA];
                uint32_t cnt[S::C];
#pragma unroll
                for (int k = 0; k < P::NA; k++) a[k] = (int)(4.0f * c[k][i][j][r]);   // unscaled products of halves: x 4, exact
                S::emit(a, cnt);
                uint32_t *p = p0 + (int64_t)((r & 3) + 8 * (r >> 2)) * ncols_pad;
#pragma unroll
                for (int k = 0; k < S::C; k++) atomicAdd(p + (int64_t)k * acc_plane, cnt[k]);
            }
        }
}

template <int MODE>
static int launch_fp4_gen(hipStream_t st, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad, int n_s, uint32_t *acc,
                          int64_t acc_plane, const unsigned long long *d_missing)
{
    if (n_s <= 0 || n_blocks <= 0) return 0;
    hipLaunchKernelGGL(pair_mfma_fp4_kernel<MODE>, dim3((unsigned)n_blocks), dim3(256), 0, st, w2, ncols_pad, n_s, acc, acc_plane, work,
                       d_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// tile and workgroups per CU of the fp4 form of a kind's general kernel (0: the kind has none)
bool pair_fp4_tile(int mode, int *tile_r, int *tile_c, int *wg_per_cu)
{
    if (mode == PM_IBS) { *tile_r = 64 * Fp4Scheme<PM_IBS>::TM; *tile_c = 64 * Fp4Scheme<PM_IBS>::TN; }
    else if (mode == PM_KING_ROBUST) { *tile_r = 64 * Fp4Scheme<PM_KING_ROBUST>::TM; *tile_c = 64 * Fp4Scheme<PM_KING_ROBUST>::TN; }
    else if (mode == PM_BETA) { *tile_r = 64 * Fp4Scheme<PM_BETA>::TM; *tile_c = 64 * Fp4Scheme<PM_BETA>::TN; }
    else if (mode == PM_KING_HOMO) { *tile_r = 64 * Fp4Scheme<PM_KING_HOMO>::TM; *tile_c = 64 * Fp4Scheme<PM_KING_HOMO>::TN; }
    else if (mode == PM_DISS) { *tile_r = 64 * Fp4Scheme<PM_DISS>::TM; *tile_c = 64 * Fp4Scheme<PM_DISS>::TN; }
    else return false;
    if (wg_per_cu) *wg_per_cu = (mode == PM_KING_ROBUST) ? Fp4Scheme<PM_KING_ROBUST>::WPS : 1;
    return true;
}

int launch_pair_fp4_miss(hipStream_t st, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad, int n_s,
                         uint32_t *acc, const unsigned long long *d_missing)
{
    if (n_s <= 0 || n_blocks <= 0) return 0;
    hipLaunchKernelGGL(pair_mfma_fp4_miss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, w2, ncols_pad, n_s, acc, work,
                       d_missing, 1);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int MODE> static void i8_tile_of(int *tile_r, int *tile_c, int *wg_per_cu)
{
    *tile_r = 64 * I8Scheme<MODE>::TM; *tile_c = 64 * I8Scheme<MODE>::TN;
    if (wg_per_cu) *wg_per_cu = I8Scheme<MODE>::WPS;
}

void pair_i8_tile(int mode, int *tile_r, int *tile_c, int *wg_per_cu)
{
    switch (mode) {
    case PM_IBS: return i8_tile_of<PM_IBS>(tile_r, tile_c, wg_per_cu);
    case PM_KING_ROBUST: return i8_tile_of<PM_KING_ROBUST>(tile_r, tile_c, wg_per_cu);
    case PM_KING_HOMO: return i8_tile_of<PM_KING_HOMO>(tile_r, tile_c, wg_per_cu);
    case PM_GCTA_MISS: return i8_tile_of<PM_GCTA_MISS>(tile_r, tile_c, wg_per_cu);
    case PM_BETA: return i8_tile_of<PM_BETA>(tile_r, tile_c, wg_per_cu);
    default: return i8_tile_of<PM_IBS_NOMISS>(tile_r, tile_c, wg_per_cu);
    }
}

// d_missing != nullptr (IBS, KING-robust): two launches, one of them exits at once -- blocks without missing calls
// take the binary 3-product form on its own work list (128 x 128 tiles).
int launch_pair_i8(hipStream_t st, int mode, const int4 *work, int n_blocks, const uint32_t *w2, int64_t ncols_pad,
                   int n_q, int n_snp, uint32_t *acc, int64_t acc_plane, const unsigned long long *d_missing,
                   const int4 *work_nm, int n_blocks_nm, bool fp4_nomiss, bool fp4_general)
{
    // fp4_nomiss: blocks without missing calls take the MX-fp4 form of the two-product kernel (n_q is a multiple of 8 then)
    if (n_q <= 0 || n_blocks <= 0) return 0;
    const unsigned long long *nf = nullptr;
    // IBS / KING-robust: the kind's general kernel, then (d_missing) the two-product kernel for the blocks without missing calls
    const auto general_then_nomiss = [&](auto kind) {
        constexpr int M = decltype(kind)::value;
        if (fp4_general ? launch_fp4_gen<M>(st, work, n_blocks, w2, ncols_pad, n_q / 2, acc, acc_plane, d_missing)
                        : launch_i8<M>(st, work, n_blocks, w2, ncols_pad, n_q, n_snp, acc, acc_plane, d_missing, 1)) return 1;
        if (d_missing && fp4_nomiss) return launch_fp4_nomiss<PM_IBS_NOMISS>(st, work_nm, n_blocks_nm, w2, ncols_pad, n_q / 2, n_snp, acc, acc_plane, d_missing);
        return d_missing ? launch_i8<PM_IBS_NOMISS>(st, work_nm, n_blocks_nm, w2, ncols_pad, n_q, n_snp, acc, acc_plane, d_missing, 0) : 0;
    };
    switch (mode) {
    case PM_IBS: return general_then_nomiss(std::integral_constant<int, PM_IBS>{});
    case PM_KING_ROBUST: return general_then_nomiss(std::integral_constant<int, PM_KING_ROBUST>{});
    case PM_KING_HOMO:
        if (!d_missing)
            return fp4_general ? launch_fp4_gen<PM_KING_HOMO>(st, work, n_blocks, w2, ncols_pad, n_q / 2, acc, acc_plane, nf)
                               : launch_i8<PM_KING_HOMO>(st, work, n_blocks, w2, ncols_pad, n_q, n_snp, acc, acc_plane, nf, 0);
        if (fp4_general ? launch_fp4_gen<PM_KING_HOMO>(st, work, n_blocks, w2, ncols_pad, n_q / 2, acc, acc_plane, d_missing)
                        : launch_i8<PM_KING_HOMO>(st, work, n_blocks, w2, ncols_pad, n_q, n_snp, acc, acc_plane, d_missing, 1)) return 1;
        if (fp4_nomiss) return launch_fp4_nomiss<PM_HOMO_NOMISS>(st, work_nm, n_blocks_nm, w2, ncols_pad, n_q / 2, n_snp, acc, acc_plane, d_missing);
        return launch_i8<PM_HOMO_NOMISS>(st, work_nm, n_blocks_nm, w2, ncols_pad, n_q, n_snp, acc, acc_plane, d_missing, 0);
    case PM_BETA:
        if (fp4_general) return launch_fp4_gen<PM_BETA>(st, work, n_blocks, w2, ncols_pad, n_q / 2, acc, acc_plane, nf);
        return launch_i8<PM_BETA>(st, work, n_blocks, w2, ncols_pad, n_q, n_snp, acc, acc_plane, nf, 0);
    case PM_GCTA_MISS:   // only for blocks that hold missing calls
        return launch_i8<PM_GCTA_MISS>(st, work, n_blocks, w2, ncols_pad, n_q, n_snp, acc, acc_plane, d_missing, 1);
    case PM_DISS:        // MX-fp4 only: the general kernel for blocks with missing calls, g.g' of the two-product kernel for the others
        if (!fp4_general || !fp4_nomiss || !d_missing) { set_error("launch_pair_i8: the dissimilarity counters need the MX-fp4 kernels"); return 1; }
        if (launch_fp4_gen<PM_DISS>(st, work, n_blocks, w2, ncols_pad, n_q / 2, acc, acc_plane, d_missing)) return 1;
        return launch_fp4_nomiss<PM_DISS>(st, work_nm, n_blocks_nm, w2, ncols_pad, n_q / 2, n_snp, acc, acc_plane, d_missing);
    }
    set_error("launch_pair_i8: bad mode");
    return 1;
}

}  // namespace snpgpu
