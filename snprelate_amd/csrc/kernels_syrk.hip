// SYRK kernels of the GRM / PCA / KING-homo / EIGMIX panels other than the single-product family (kernels_syrk_uv.hip):
//
//  syrk_x1_kernel        syrk_uv_kernel's sums (with it: CProdMat_AlgArith::MulAdd src/genPCA.cpp:229-312) from an exact row operand x
//      hi / lo-split column operand (two products), one wave per SIMD (GRM / PCA blocks WITH missing calls; every block with SNPGPU_SYRK_UV=0)
//  syrk_h3_kernel        <2, true>: the same product at two waves per SIMD; <2, false>: constant row table (the masked
//      p(1-p) sums of KING-homo src/genKING.cpp:115-154, EIGMIX's both-missing weights); <3, false>: three-product split
//  syrk_mfma_kernel      the same sums on fp32 MFMAs (SNPGPU_SYRK=f32; the tile north_star names)
#include <algorithm>
#include "snpgpu_internal.h"
#include "syrk_device.h"

namespace snpgpu {

// ---------------------------------------------------------------------------
// SYRK on fp32 MFMA, barrier-free main loop.
// Measured on MI355X (tools/ubench/syrk_ubench.hip): fp32 MFMA shares the SIMD datapath with VALU
// and LDS returns -- every VALU op or lane-divergent ds_read next to f32 MFMAs costs ~4-5 SIMD
// cycles -- so the decode work per MFMA is what separates this kernel from the 98.7 % pure-MFMA
// loop.  Hence PAIR-coded genotype words and a 16-entry float2 table per SNP pair in LDS: TWO
// operand values cost ONE VALU op (v_add_u32_sdwa: table address = base + byte) plus ONE
// conflict-free ds_read_b64, i.e. 0.5 decode events per MFMA with a 64 x 64 tile per wave
// (2 x 2 v_mfma_f32_32x32x2_f32 accumulators; micro-benchmark: 90 % of peak.  A 64 x 128 tile per
// wave measures the same at N = 100 000 and 8 % less at N = 20 000: more tail, fewer waves).
// Workgroup = 4 waves (2x2), tile 128 x 128.  Lane l of a wave needs Z[sample = l&31][snp] for the
// MFMA steps of 16-SNP group q with snp = 16q + 8h + 2p + e (h = l>>5, pair p = 0..3, e = 0/1; any K
// order is legal as long as both operands use it): half h reads dword 2q+h of ITS sample
// (coalesced 128-byte rows of W8) and walks its 4 bytes.  No operand tile lives in LDS, waves never
// wait for each other inside the K loop; the only barrier is the table swap every MM_LUTCH SNPs.
// Accumulation is fp32 for at most MM_PROMOTE = 1024 SNPs (relative rounding error ~1.5e-6 on the
// diagonal, less elsewhere), then the partial is added to the fp64 panel accumulator in HBM with
// fire-and-forget global_atomic_add_f64 (one owner per element and launch: no contention).

__global__ __launch_bounds__(256, 4) void syrk_mfma_kernel(
    const uint32_t *__restrict__ w8, int64_t ncols_pad, const float2 *__restrict__ lut, int n_q,
    double *__restrict__ acc, int64_t ld, int64_t tiles_c, const int *__restrict__ prefix, const int *__restrict__ first, int n_sr,
    int n_super, int n_tr, int n_tc, const unsigned long long *__restrict__ d_skip_if_zero)
{
    if (d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    const TileCoord t = map_tile(prefix, first, n_sr, n_super, TileShape{MM_SUPER, MM_TILE_R, MM_TILE_C}, n_tr, n_tc);
    if (!t.valid) return;
    constexpr int CHE = (MM_LUTCH / 2) * 16;      // float2 entries per table chunk (128 B per SNP pair)
    __shared__ float2 slut[2][CHE];               // 2 x 16 KiB decode tables

    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    constexpr int TM = 2, TN = 2;

    const uint32_t *__restrict__ pa = w8 + (int64_t)kh * ncols_pad + (int64_t)t.tr * MM_TILE_R + wr * 64 + li;
    const uint32_t *__restrict__ pb = w8 + (int64_t)kh * ncols_pad + (int64_t)t.tc * MM_TILE_C + wc * 64 + li;

    f32x16 c32[TM][TN];   // (inline: zero_acc changes this kernel's code)
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) c32[i][j][r] = 0.f;
    // C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    double *__restrict__ pacc = acc + acc_off(ld, tiles_c, (int64_t)t.tr * MM_TILE_R + wr * 64 + 4 * kh,
                                              (int64_t)t.tc * MM_TILE_C + wc * 64 + li);
    const int64_t rs = tiles_c ? ACC_TILE : ld;    // row stride inside this wave's part of the accumulator

    constexpr int QCH = MM_LUTCH / 16;             // 16-SNP groups per table chunk
    const int n_chunk = (n_q + QCH - 1) / QCH;
    const int n_ent = n_q * 8 * 16;                // float2 entries of the whole block's table

    for (int e = tid; e < CHE; e += 256) slut[0][e] = (e < n_ent) ? lut[e] : make_float2(0.f, 0.f);
    uint32_t wa[TM], wb[TN];
#pragma unroll
    for (int i = 0; i < TM; i++) wa[i] = pa[32 * i];
#pragma unroll
    for (int j = 0; j < TN; j++) wb[j] = pb[32 * j];
    __syncthreads();

    for (int c = 0; c < n_chunk; c++) {
        const int cur = c & 1;
        const int q_beg = c * QCH;
        const int q_end = (q_beg + QCH < n_q) ? (q_beg + QCH) : n_q;
        const bool more = (c + 1 < n_chunk);
        // byte address of the table of this lane-half's first SNP pair of the chunk (4 pairs per half)
        const char *tb = reinterpret_cast<const char *>(&slut[cur][0]) + 512 * kh;
        for (int q = q_beg; q < q_end; q++) {
            uint32_t a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; i++) a[i] = wa[i];
#pragma unroll
            for (int j = 0; j < TN; j++) b[j] = wb[j];
            if (q + 1 < n_q) {                     // prefetch the next 16 SNPs
                const int64_t off = (int64_t)(q + 1) * 2 * ncols_pad;
#pragma unroll
                for (int i = 0; i < TM; i++) wa[i] = pa[off + 32 * i];
#pragma unroll
                for (int j = 0; j < TN; j++) wb[j] = pb[off + 32 * j];
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                float2 za[TM], zb[TN];
#pragma unroll
                for (int i = 0; i < TM; i++)
                    za[i] = *reinterpret_cast<const float2 *>(tb + ((a[i] >> (8 * p)) & 0xFFu) + 128 * p);
#pragma unroll
                for (int j = 0; j < TN; j++)
                    zb[j] = *reinterpret_cast<const float2 *>(tb + ((b[j] >> (8 * p)) & 0xFFu) + 128 * p);
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++)
                        c32[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[i].x, zb[j].x, c32[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++)
                        c32[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[i].y, zb[j].y, c32[i][j], 0, 0, 0);
            }
            tb += 1024;                            // 8 SNP pairs x 128 B
        }
        // every MM_PROMOTE SNPs (and at the end) flush the fp32 partial into the fp64 panel accumulator
        if (!more || ((c + 1) % (MM_PROMOTE / MM_LUTCH)) == 0) {
            // (the flush address is opaque: without that the row addresses are hoisted out of the K loop and kept in scratch: 27 spills)
            flush_tiles32<false, true>(pacc, rs, INT64_MAX, c32, 1.0);
        }
        if (more) {                                // next chunk's table into the other buffer
            const float2 *__restrict__ src = lut + (int64_t)(c + 1) * CHE;
            for (int e = tid; e < CHE; e += 256)
                slut[cur ^ 1][e] = ((c + 1) * CHE + e < n_ent) ? src[e] : make_float2(0.f, 0.f);
            __syncthreads();
        }
    }
}

int launch_syrk(hipStream_t st, const TileGrid &tg, const uint32_t *w8, int64_t ncols_pad, const float2 *lut,
                int n_q, double *acc, int64_t ld, int64_t tiles_c, const unsigned long long *d_skip_if_zero)
{
    if (n_q <= 0) return 0;
    hipLaunchKernelGGL(syrk_mfma_kernel, dim3((unsigned)tg.grid), dim3(256), 0, st, w8, ncols_pad, lut, n_q, acc, ld, tiles_c,
                       tg.d_prefix, tg.d_first, tg.n_sr, tg.n_super, tg.n_tr, tg.n_tc, d_skip_if_zero);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// SYRK on fp16 MFMAs with split operands: z = hi + lo, hi = fp16(z), lo = fp16(z - hi) (22 significant
// bits, built from the fp64 table values), and
//     z z' = hi hi' + hi lo' + lo hi'  (+ lo lo' ~ 2^-22 z z', dropped)
// Products of two fp16 numbers are exact in fp32, the accumulation is fp32 inside the MFMA and fp64
// across MM_PROMOTE SNPs exactly as in syrk_mfma_kernel, so the result carries the same rounding
// budget as the fp32-MFMA form (measured against the fp64 oracle in tests/test_gpu_parity.py) while
// three v_mfma_f32_32x32x16_f16 (96 matrix-pipe cycles) replace eight v_mfma_f32_32x32x2_f32 (512) per
// 16 SNPs and 32 x 32 pairs.  Operand decode as above: pair-coded words, one v_add_u32_sdwa + one
// ds_read_b64 per SNP pair; the 8-byte table entry is {hi0 | hi1 << 16, lo0 | lo1 << 16}, so the four
// lookups of a lane ARE its 8-SNP operand registers (hi: dword 0 of each, lo: dword 1).
// Workgroup = 4 waves (2 x 2), tile 256 x 128, each wave 128 x 64 = 4 x 2 accumulators; two operand
// register sets: group q+1 is decoded while the 24 MFMAs of group q run (fp16 MFMAs overlap with
// VALU/LDS work, unlike fp32 MFMAs).  Work items as in the int8 pair kernel ({tile, K part}); the
// flush is an fp64 atomic add, so K parts may share a tile.

//
// NP = 2 ("exact row side", blocks WITHOUT missing calls): with z = y (g - avg) per SNP and a centre c close to avg
// that has only a few binary digits,
//     z_i z_j = (g_i - c) * [y z_j]  -  (avg - c) * [y z_j]
// the row operand g - c is exact in fp16, so only the column operand w = y z needs the hi/lo split: TWO MFMAs per
// 32 x 32 x 16 instead of three, and a row operand that toggles few multiplier bits (the kernel runs against the
// socket power cap, HISTORY.md 4.5).  The second term does not depend on i: the kernel leaves it out, colcorr_kernel sums
// it per column over all blocks (fp64, ctx->colterm) and colterm_settle_kernel subtracts it from every row of the panel
// once, before a result is read (kernels_final.hip).
// The table builder writes w instead of z when the block has no missing call; with one, a missing row
// genotype would need the real-valued centre avg and the three-product kernel runs instead (the two launches
// are gated on the block's missing flag, as in the int8 pair kernel).
// The masked sums of KING-homo and EIGMIX are exact-row-side products by nature, for every block and without a
// column term: sum_s v_i v_j c_s = v_i * [c v_j] with the call indicator v (a_kind 1), and the weighted
// both-missing sums m_i * [d m_j] with the missing indicator m (a_kind 2).
// E16 (NP == 2, a_kind 0): 16-byte table entries {hi pair, lo pair, ROW pair, -} -- the row operand is per SNP,
// (g - c_s) 2^shift with c_s = avg_s rounded to a few binary digits (build_lut_kernel), so that the products have
// the variance of the centred form whatever the allele frequency (a fixed centre 1 costs a factor 1/(2p) in
// variance, i.e. accuracy, on rare variants); the words carry code * 16 and a chunk holds 256 SNPs.
// Row pair of a 16-byte table entry (bytes 8..15 hold it twice) as an EIGHT-byte LDS read.  ds_read_b32 banks are
// (a/4) mod 32, so the dword at 16 c + 8 of entry c shares its bank with entry c + 8 -- the second genotype of the pair
// being 0 or 2 -- and nearly every 32-lane group paid a two-way conflict (SQ_LDS_BANK_CONFLICT = 33 % of SQ_LDS_IDX_ACTIVE
// in round 1).  ds_read_b64 banks are (a/4) mod 64: the 16 entries sit on 16 different bank pairs, and the instruction
// costs the same two LDS cycles as a conflict-free ds_read_b32 (MI355X_MICROARCH.md, LDS).
__device__ __forceinline__ uint32_t h3_row_pair(const char *p)
{
    // volatile: the compiler must not narrow the access to the one dword that is used
    typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
    const u32x2_t v = *(const volatile __attribute__((address_space(3))) u32x2_t *)(p);
    return v.x;
}

template <int NP, bool E16>
__global__ __launch_bounds__(256, 2) void syrk_h3_kernel(
    const uint32_t *__restrict__ w8, int64_t ncols_pad, const uint2 *__restrict__ lut, int n_q,
    double *__restrict__ acc, int64_t ld, int64_t tiles_c, const int4 *__restrict__ work,
    const unsigned long long *__restrict__ d_skip_if_zero, const unsigned long long *__restrict__ d_missing,
    int64_t n_rows_real, int a_kind, int promote_chunks)
{
    if (d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    if (d_missing && ((*d_missing != 0ull) != (NP == 3))) return;
    constexpr int TM = 4, TN = 2;    // the exact / cheaper-to-decode row side gets the four 32-sample groups
    constexpr int CHS = E16 ? H3_LUTCH / 2 : H3_LUTCH;   // SNPs per table chunk
    constexpr int PST = E16 ? 256 : 128;                 // bytes of table per SNP pair (16 entries)
    constexpr int CHE = (H3_LUTCH / 2) * 16;       // 8-byte units per chunk: 32 KiB either way
    constexpr int QCH = CHS / 16;                  // 16-SNP groups per chunk
    __shared__ uint2 slut[2][CHE];                 // 2 x 32 KiB
    __shared__ uint2 sgt[16];                      // NP == 2, !E16: pair code -> {fp16(a0) | fp16(a1) << 16} of the indicator, 8-byte stride

    const int4 item = work[blockIdx.x];
    if (item.w == 0) return;
    const int n_chunk_all = (n_q + QCH - 1) / QCH;
    const auto [c_beg, c_end] = k_part(0, n_chunk_all, item.z, item.w);
    if (c_beg >= c_end) return;

    const auto [tid, lane, wave, wr, wc, li, kh, l16, kq] = wave_coord();
    const uint32_t *__restrict__ pa = w8 + (int64_t)kh * ncols_pad + (int64_t)item.x * H3_TILE_R + wr * (32 * TM) + li;
    const uint32_t *__restrict__ pb = w8 + (int64_t)kh * ncols_pad + (int64_t)item.y * H3_TILE_C + wc * (32 * TN) + li;
    double *__restrict__ pacc = acc + acc_off(ld, tiles_c, (int64_t)item.x * H3_TILE_R + wr * (32 * TM) + 4 * kh,
                                              (int64_t)item.y * H3_TILE_C + wc * (32 * TN) + li);
    const int64_t rs = tiles_c ? ACC_TILE : ld;    // row stride inside this wave's part of the accumulator

    f32x16 c32[TM][TN];
    zero_acc(c32);

    if (NP == 2 && !E16 && threadIdx.x < 16) {
        // constant row operand per genotype code 0, 1, 2, 3:  a_kind 1: called, a_kind 2: missing
        const uint32_t one = 0x3C00u;
        const uint32_t c0 = threadIdx.x & 3, c1 = threadIdx.x >> 2;
        const uint32_t h0 = (a_kind == 1) ? (c0 != 3 ? one : 0u) : (c0 == 3 ? one : 0u);
        const uint32_t h1 = (a_kind == 1) ? (c1 != 3 ? one : 0u) : (c1 == 3 ? one : 0u);
        sgt[threadIdx.x] = make_uint2(h0 | (h1 << 16), 0u);
    }
    u32x4 Ah[1][TM], Al[1][NP == 3 ? TM : 1], Bh[1][TN], Bl[1][TN];
    uint32_t wa[TM], wb[TN], wa2[TM], wb2[TN];     // words of the current and of the next group
    const char *gt = reinterpret_cast<const char *>(&sgt[0]);
#define H3_LOAD_WORDS(q, A_, B_)                                                          \
    do {                                                                                  \
        const int64_t off_ = (int64_t)(q) * 2 * ncols_pad;                                \
        _Pragma("unroll") for (int i = 0; i < TM; i++) A_[i] = pa[off_ + 32 * i];         \
        _Pragma("unroll") for (int j = 0; j < TN; j++) B_[j] = pb[off_ + 32 * j];         \
    } while (0)
#define H3_DECODE(set, tb, wa, wb)                                                                \
    do {                                                                                  \
        _Pragma("unroll") for (int p = 0; p < 4; p++) {                                   \
            _Pragma("unroll") for (int i = 0; i < TM; i++) {                              \
                if (NP == 3) {                                                            \
                    const uint2 t_ = *reinterpret_cast<const uint2 *>((tb) + ((wa[i] >> (8 * p)) & 0xFFu) + PST * p); \
                    Ah[set][i][p] = t_.x; Al[set][NP == 3 ? i : 0][p] = t_.y;             \
                } else if (E16) {                                                         \
                    Ah[set][i][p] = h3_row_pair((tb) + ((wa[i] >> (8 * p)) & 0xFFu) + PST * p + 8); \
                } else {                                                                  \
                    Ah[set][i][p] = *reinterpret_cast<const uint32_t *>(gt + ((wa[i] >> (8 * p)) & 0xFFu)); \
                }                                                                         \
            }                                                                             \
            _Pragma("unroll") for (int j = 0; j < TN; j++) {                              \
                const uint2 t_ = *reinterpret_cast<const uint2 *>((tb) + ((wb[j] >> (8 * p)) & 0xFFu) + PST * p); \
                Bh[set][j][p] = t_.x; Bl[set][j][p] = t_.y;                               \
            }                                                                             \
        }                                                                                 \
    } while (0)
#define H3_MFMAS(set)  /* product-major: MFMAs on the same accumulator are TM*TN instructions apart */ \
    do {                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; i++)                                    \
            _Pragma("unroll") for (int j = 0; j < TN; j++)                                \
                c32[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16((f16x8)Ah[set][i], (f16x8)Bh[set][j], c32[i][j], 0, 0, 0); \
        _Pragma("unroll") for (int i = 0; i < TM; i++)                                    \
            _Pragma("unroll") for (int j = 0; j < TN; j++)                                \
                c32[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16((f16x8)Ah[set][i], (f16x8)Bl[set][j], c32[i][j], 0, 0, 0); \
        if (NP == 3) {                                                                    \
            _Pragma("unroll") for (int i = 0; i < TM; i++)                                \
                _Pragma("unroll") for (int j = 0; j < TN; j++)                            \
                    c32[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16((f16x8)Al[set][NP == 3 ? i : 0], (f16x8)Bh[set][j], c32[i][j], 0, 0, 0); \
        }                                                                                 \
    } while (0)

    // Table chunks (32 KiB) travel HBM/L2 -> LDS without passing through VGPRs (global_load_lds_dwordx4,
    // 1 KiB per instruction and wave): the copy of chunk c+1 is issued at the start of chunk c and is
    // complete long before the barrier at its end (vmcnt is in-order and the loop waits for younger loads).
#define H3_TABLE_ASYNC(chunk, buf)                                                                             \
    do {                                                                                                       \
        const char *src_ = reinterpret_cast<const char *>(lut) + (int64_t)(chunk) * (CHE * 8) + wave * (CHE * 2) + lane * 16; \
        char *dst_ = reinterpret_cast<char *>(&slut[buf][0]) + wave * (CHE * 2);                              \
        _Pragma("unroll") for (int t_ = 0; t_ < CHE * 2 / 1024; t_++)                                                       \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src_ + 1024 * t_), \
                                             (__attribute__((address_space(3))) void *)(dst_ + 1024 * t_), 16, 0, 0); \
    } while (0)
    H3_TABLE_ASYNC(c_beg, c_beg & 1);
    H3_LOAD_WORDS(c_beg * QCH, wa, wb);
    H3_LOAD_WORDS(c_beg * QCH + 1, wa2, wb2);
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();

    // fp32 partial sums go to the fp64 panel every promote_chunks table chunks (launch_syrk_h3: 4096 SNPs for the
    // three-product kernel, one whole 16 384-SNP feed block for the exact-row kernel)
    for (int c = c_beg; c < c_end; c++) {
        const int cur = c & 1;
        const int q0 = c * QCH;
        const int q_cnt = (q0 + QCH <= n_q) ? QCH : (n_q - q0);      // multiple of 4 (blocks are padded to 64 SNPs)
        const bool more = (c + 1 < c_end);
        // byte address of the tables of this lane-half's 4 SNP pairs of group 0 of the chunk
        const char *tb = reinterpret_cast<const char *>(&slut[cur][0]) + 4 * PST * kh;
        for (int q = 0; q < q_cnt; q += 2) {        // q_cnt is even; words are loaded two groups ahead
            H3_DECODE(0, tb, wa, wb);
            tb += 8 * PST;
            H3_LOAD_WORDS(q0 + q + 2, wa, wb);      // W8 has spare rows: reading ahead is always legal
            // next chunk's table: issued together with a word load (same latency, in-order return), so the
            // vmcnt wait of a later decode does not stall on it
            if (q == 0 && more) H3_TABLE_ASYNC(c + 1, cur ^ 1);
            H3_MFMAS(0);
            H3_DECODE(0, tb, wa2, wb2);
            tb += 8 * PST;
            H3_LOAD_WORDS(q0 + q + 3, wa2, wb2);
            H3_MFMAS(0);
        }
        // every MM_PROMOTE SNPs (and at the end of the part) flush the fp32 partial into the fp64 panel
        if (!more || ((c + 1) % promote_chunks) == 0) {
            double *pflush = flush_ptr(pacc);       // opaque: keeps the 32 row addresses out of the main loop's live ranges
            // (inline: flush_tiles32 changes this kernel's code)
            const int64_t rows_left = flush_rows_left(n_rows_real, (int64_t)item.x * H3_TILE_R + wr * (32 * TM) + 4 * kh);
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = i * 32 + (r & 3) + 8 * (r >> 2);
                    double *__restrict__ pr = pflush + (int64_t)row * rs;
                    const bool real_row = (row < rows_left);
#pragma unroll
                    for (int j = 0; j < TN; j++) {
                        // fp32 partials, exactly representable in fp64: the panel sums do not depend on the order in
                        // which the K parts of a tile arrive
                        if (real_row) unsafeAtomicAdd(pr + 32 * j, (double)c32[i][j][r]);
                        c32[i][j][r] = 0.f;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        if (more) {                                 // the next chunk's table is in place for every wave
            // vmcnt is in-order: the table copy was issued in the chunk's first iteration, the only loads that may
            // still be in flight behind it are the words of the next two groups (2 (TM + TN) = 12; a chunk that is
            // followed by another one is full, so at least that many were issued after the copy) -- wait for
            // everything older, not for them
            static_assert(2 * (TM + TN) == 12, "s_waitcnt immediate below");
            __builtin_amdgcn_s_waitcnt(0x0F7C);     // vmcnt(12)
            __syncthreads();
        }
    }
#undef H3_TABLE_ASYNC
#undef H3_LOAD_WORDS
#undef H3_DECODE
#undef H3_MFMAS
}

// ---------------------------------------------------------------------------
// syrk_x1_kernel: the exact-row SYRK (syrk_h3_kernel<2, true>: same tables, same words, same arithmetic) with ONE wave
// per SIMD.  Each wave owns 128 x 128 = 4 x 4 accumulators (256 AGPRs), the workgroup (2 x 2 waves) a 256 x 256 tile: 32
// table lookups per 32 MFMAs instead of 24 per 16, and a third fewer sample words per flop.  With the SIMD to itself the
// wave hides its own latencies: two operand register sets -- the lookups of group g + 1 are interleaved one by one with the
// MFMAs of group g (source order pinned by sched_barrier) -- and a ring of four word sets (the words of group g + 4 are
// requested during group g and first used during group g + 3).  Table chunks as in syrk_h3_kernel (256 SNPs, 32 KiB, double
// buffered, HBM/L2 -> LDS without VGPRs); the barrier of a chunk boundary sits before the chunk's LAST group, whose MFMAs
// then cover the first lookups out of the next chunk's table.  Table entries are 12 bytes {hi pair, lo pair, row pair}: the
// dword banks 3 c + {0, 1, 2} (mod 32) of the 16 entries of a pair are distinct, so every lookup is a conflict-free
// ds_read_b32 straight into its slot of an MFMA operand (an 8-byte read needs a v_mov -- and a wait -- per value).

__global__ __launch_bounds__(256, 1) void syrk_x1_kernel(
    const uint32_t *__restrict__ w8, int64_t ncols_pad, const uint2 *__restrict__ lut, int n_q,
    double *__restrict__ acc, int64_t ld, int64_t tiles_c, const int4 *__restrict__ work,
    const unsigned long long *__restrict__ d_skip_if_zero, int64_t n_rows_real, int chunk_lo, int chunk_hi, int n_runs, int run_chunks,
    int run_group, int n_items8, const unsigned long long *__restrict__ d_short_runs, int short_div)
{
    if (d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    constexpr int TM = 4, TN = 4, D = 4;
    constexpr int CHS = X1_CHS;                    // SNPs per table chunk
    constexpr int PST = 192;                       // bytes of table per SNP pair: 16 entries of 12 bytes {hi pair, lo pair, row pair}
    constexpr int CHE = (CHS / 2) * PST / 8;       // 8-byte units per chunk: 24 KiB
    constexpr int QCH = CHS / 16;                  // 16-SNP groups per chunk
    static_assert(QCH % (2 * D) == 0, "whole double rounds of the word banks per chunk");
    __shared__ uint2 slut[2][CHE];

    // n_runs > 1: one launch for all fp32 runs of the block, work items (tile, run), run fastest per XCD (see syrk_uv_kernel)
    int wi = blockIdx.x;
    if (n_runs > 1) {
        const FusedItem f = fused_item(n_runs, run_group, n_items8);
        if (!f.valid) return;
        wi = f.wi;
        // the launch is laid out for the SHORT runs (run_chunks / short_div table chunks each: blocks that hold rare variants next
        // to missing calls, flag set by build_lut_kernel); any other block uses the first runs of it at the full length
        const int rc = (d_short_runs && *d_short_runs != 0ull) ? run_chunks / short_div : run_chunks;
        chunk_lo = f.run * rc;
        if (chunk_lo >= chunk_hi) return;
        chunk_hi = (chunk_lo + rc < chunk_hi) ? (chunk_lo + rc) : chunk_hi;
    } else if (d_short_runs) {
        // one launch per run (SNPGPU_RUN_INNER=0), two launches per full-length run [chunk_lo, chunk_hi): `run_group` = which half.
        // A flagged block runs both halves as fp32 runs of their own -- the same numerics as the fused launch (this
        // A/B switch used to change the accuracy as well) --, any other block does the whole run in launch 0 and launch 1 exits
        if (*d_short_runs != 0ull) {
            chunk_lo += run_group * (run_chunks / short_div);
            if (chunk_lo >= chunk_hi) return;
            if (run_group == 0) chunk_hi = (chunk_lo + run_chunks / short_div < chunk_hi) ? (chunk_lo + run_chunks / short_div) : chunk_hi;
        } else if (run_group != 0) return;
    }
    const int4 item = work[wi];
    if (item.w == 0) return;
    // this launch covers the table chunks [chunk_lo, chunk_hi) -- one fp32 run: the accumulators are flushed ONCE, after the
    // K loop (a flush inside the loop writes them with VALU instructions and the compiler then keeps all 256 in VGPRs,
    // shuttling each through AGPRs around its MFMA: 1140 bytes of scratch per lane)
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

    u32x4 Ah[2][TM], Bh[2][TN], Bl[2][TN];        // two operand sets: MFMAs read one, the lookups fill the other
    // two banks of four word sets: a round of four groups looks its words up in one bank while ALL 32 word loads of the
    // next round go out during its first group into the other bank -- whatever s_waitcnt vmcnt the compiler places later in
    // the round (it is conservative across the loop edge) then finds them three groups old
    uint32_t W0a[D][TM], W0b[D][TN], W1a[D][TM], W1b[D][TN];

#define X1_LOOKUP(t, WA_, WB_, wset, m, tb)  /* lookup number m of a group: 16 row lookups, then 16 column lookups */ \
    do {                                                                                     \
        if ((m) < 16) {                                                                      \
            constexpr int i_ = ((m) < 16 ? (m) : 0) >> 2, p_ = (m) & 3;                       \
            Ah[t][i_][p_] = x1_lds32((tb) + ((WA_[wset][i_] >> (8 * p_)) & 0xFFu) + PST * p_ + 8); \
        } else {                                                                             \
            constexpr int j_ = ((m) >= 16 ? (m) - 16 : 0) >> 2, p_ = (m) & 3;                 \
            const uint32_t e_ = (tb) + ((WB_[wset][j_] >> (8 * p_)) & 0xFFu) + PST * p_;      \
            Bh[t][j_][p_] = x1_lds32(e_);      /* volatile: not to be merged into ds_read2_b32 (pair result + moves) */ \
            Bl[t][j_][p_] = x1_lds32(e_ + 4);                                                \
        }                                                                                    \
    } while (0)
#define X1_TABLE_ASYNC(chunk, buf)                                                                             \
    do {                                                                                                       \
        const char *src_ = reinterpret_cast<const char *>(lut) + (int64_t)(chunk) * (CHE * 8) + wave * (CHE * 2) + lane * 16; \
        char *dst_ = reinterpret_cast<char *>(&slut[buf][0]) + wave * (CHE * 2);                              \
        _Pragma("unroll") for (int t_ = 0; t_ < CHE * 2 / 1024; t_++)                                          \
            x1_lds_dma16(src_ + 1024 * t_, x1_lds_off(dst_ + 1024 * t_));                                      \
    } while (0)
    // word load number m (0..31) of a round: set m >> 3, sample group m & 7 (four row groups, four column groups)
#define X1_LOAD(YA_, YB_, g_first, m)                                                         \
    do {                                                                                      \
        const int64_t off_ = (int64_t)((g_first) + ((m) >> 3)) * 2 * ncols_pad;               \
        if (((m) & 7) < TM) YA_[(m) >> 3][((m) & 7) < TM ? ((m) & 7) : 0] = pa[off_ + 32 * ((m) & 7)]; \
        else YB_[(m) >> 3][((m) & 7) >= TM ? ((m) & 7) - TM : 0] = pb[off_ + 32 * (((m) & 7) - TM)];  \
    } while (0)
    // one group: 32 MFMAs out of operand set S_.  The 48 LDS reads of the NEXT group's lookups (word set NS_ of bank LA_ / LB_,
    // into operand set T_) ride behind the first 24 MFMAs, two lookups behind each of the first 8 and one behind the next 16, so
    // that the last returns while the final eight MFMAs run; LOAD_ != 0 (first group of a round): behind every MFMA one word
    // load of the next round (bank YA_ / YB_).  Plain macros: every register index is a literal.
    // address of lookup L of the next group / its LDS read(s), split so that an address is computed one MFMA slot before it is used
    // (a ds_read right behind its v_add_u32_sdwa waits for the VALU result: two such pairs filled a 32-cycle MFMA slot)
#define X1_AD(LA_, LB_, NS_, L, tb)   /* table base + the pair's byte; the constant part of the address stays an immediate of the read */ \
    ((L) < 16 ? (tb) + ((LA_[NS_][((L) < 16 ? (L) : 0) >> 2] >> (8 * ((L) & 3))) & 0xFFu)                            \
              : (tb) + ((LB_[NS_][((L) >= 16 ? (L) - 16 : 0) >> 2] >> (8 * ((L) & 3))) & 0xFFu))
#define X1_RD(T_, L, a)                                                                                              \
    do {                                                                                                            \
        if ((L) < 16) Ah[T_][((L) < 16 ? (L) : 0) >> 2][(L) & 3] = x1_lds32((a) + PST * ((L) & 3) + 8);              \
        else { Bh[T_][((L) >= 16 ? (L) - 16 : 0) >> 2][(L) & 3] = x1_lds32((a) + PST * ((L) & 3));                   \
               Bl[T_][((L) >= 16 ? (L) - 16 : 0) >> 2][(L) & 3] = x1_lds32((a) + PST * ((L) & 3) + 4); }             \
    } while (0)
#define X1_STEP(m, S_, T_, LA_, LB_, NS_, LOAD_, YA_, YB_, g_load, tb)                                              \
    do {                                                                                                            \
        c32[((m) & 15) >> 2][(m) & 3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(                                      \
            (f16x8)Ah[S_][((m) & 15) >> 2], (f16x8)(((m) >> 4) ? Bl[S_][(m) & 3] : Bh[S_][(m) & 3]),                 \
            c32[((m) & 15) >> 2][(m) & 3], 0, 0, 0);                                                                \
        if ((m) < 8) {                                                                                              \
            X1_RD(T_, 2 * (m), a0_); X1_RD(T_, 2 * (m) + 1, a1_);                                                    \
            if ((m) < 7) { a0_ = X1_AD(LA_, LB_, NS_, 2 * (m) + 2, tb); a1_ = X1_AD(LA_, LB_, NS_, 2 * (m) + 3, tb); \
                           asm volatile("" : "+v"(a0_), "+v"(a1_)); }   /* pins the additions HERE, not next to their reads */ \
            else { a0_ = X1_AD(LA_, LB_, NS_, 16, tb); asm volatile("" : "+v"(a0_)); }                              \
        } else if ((m) < 24) {                                                                                      \
            X1_RD(T_, (m) + 8, a0_);                                                                                \
            if ((m) < 23) { a0_ = X1_AD(LA_, LB_, NS_, (m) + 9, tb); asm volatile("" : "+v"(a0_)); }                 \
        }                                                                                                           \
        if (LOAD_) X1_LOAD(YA_, YB_, g_load, m);                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
    } while (0)
#define X1_STEP4(m, ...) X1_STEP(m, __VA_ARGS__); X1_STEP((m) + 1, __VA_ARGS__); X1_STEP((m) + 2, __VA_ARGS__); X1_STEP((m) + 3, __VA_ARGS__)
#define X1_GROUP_ADDR0(S_, T_, LA_, LB_, NS_, LOAD_, YA_, YB_, g_load, tb)                                           \
    uint32_t a0_ = X1_AD(LA_, LB_, NS_, 0, tb), a1_ = X1_AD(LA_, LB_, NS_, 1, tb)
#define X1_GROUP(...)                                                                                               \
    do {                                                                                                            \
        X1_GROUP_ADDR0(__VA_ARGS__);                                                                                \
        X1_STEP4(0, __VA_ARGS__); X1_STEP4(4, __VA_ARGS__); X1_STEP4(8, __VA_ARGS__); X1_STEP4(12, __VA_ARGS__);    \
        X1_STEP4(16, __VA_ARGS__); X1_STEP4(20, __VA_ARGS__); X1_STEP4(24, __VA_ARGS__); X1_STEP4(28, __VA_ARGS__); \
    } while (0)

    // prologue: table of the first chunk, the words of the first round, the lookups of group 0
    X1_TABLE_ASYNC(c_beg, c_beg & 1);
#define X1_L8(m) X1_LOAD(W0a, W0b, c_beg * QCH, m); X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 1); X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 2); X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 3); \
                 X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 4); X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 5); X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 6); X1_LOAD(W0a, W0b, c_beg * QCH, (m) + 7)
    X1_L8(0); X1_L8(8); X1_L8(16); X1_L8(24);
#undef X1_L8
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();
    uint32_t tbn = x1_lds_off(&slut[c_beg & 1][0]) + 4 * PST * kh;
#define X1_L4(m) X1_LOOKUP(0, W0a, W0b, 0, m, tbn); X1_LOOKUP(0, W0a, W0b, 0, (m) + 1, tbn); X1_LOOKUP(0, W0a, W0b, 0, (m) + 2, tbn); X1_LOOKUP(0, W0a, W0b, 0, (m) + 3, tbn)
    X1_L4(0); X1_L4(4); X1_L4(8); X1_L4(12); X1_L4(16); X1_L4(20); X1_L4(24); X1_L4(28);
#undef X1_L4
    tbn += 8 * PST;

    for (int c = c_beg; c < c_end; c++) {
        const int cur = c & 1;
        const int q0 = c * QCH;
        const int q_cnt = (q0 + QCH <= n_q) ? QCH : (n_q - q0);      // multiple of 8 (blocks are padded to 128 SNPs)
        const bool more = (c + 1 < c_end);
        if (more) X1_TABLE_ASYNC(c + 1, cur ^ 1);   // every wave is past the barrier that freed this buffer
        for (int q = 0; q < q_cnt; q += 2 * D) {
            const int g = q0 + q;
            // round A: words of bank 0, loads into bank 1
            X1_GROUP(0, 1, W0a, W0b, 1, 1, W1a, W1b, g + 4, tbn); tbn += 8 * PST;
            X1_GROUP(1, 0, W0a, W0b, 2, 0, W1a, W1b, g + 4, tbn); tbn += 8 * PST;
            X1_GROUP(0, 1, W0a, W0b, 3, 0, W1a, W1b, g + 4, tbn); tbn += 8 * PST;
            X1_GROUP(1, 0, W1a, W1b, 0, 0, W1a, W1b, g + 4, tbn); tbn += 8 * PST;
            // round B: words of bank 1, loads into bank 0
            X1_GROUP(0, 1, W1a, W1b, 1, 1, W0a, W0b, g + 8, tbn); tbn += 8 * PST;
            X1_GROUP(1, 0, W1a, W1b, 2, 0, W0a, W0b, g + 8, tbn); tbn += 8 * PST;
            X1_GROUP(0, 1, W1a, W1b, 3, 0, W0a, W0b, g + 8, tbn); tbn += 8 * PST;
            // the chunk's last group looks up the NEXT chunk's table (or, at the very end, harmlessly re-reads this one:
            // ONE straight-line body -- a second variant without lookups made the register allocator give the sixteen
            // accumulator tiles different AGPRs on the two paths and shuffle them through scratch every round)
            if (q + 2 * D >= q_cnt) {
                if (more) {
                    // vmcnt is in-order: the table copy was issued at the start of this (full) chunk, behind it 64 word
                    // loads, the last 32 of them a whole round ago -- wait for everything older than those
                    __builtin_amdgcn_s_waitcnt(0x8F70); // vmcnt(32)
                    __syncthreads();
                    tbn = x1_lds_off(&slut[cur ^ 1][0]) + 4 * PST * kh;
                } else {
                    tbn = x1_lds_off(&slut[cur][0]) + 4 * PST * kh;
                }
            }
            X1_GROUP(1, 0, W0a, W0b, 0, 0, W0a, W0b, g + 8, tbn); tbn += 8 * PST;
        }
    }
    flush_tiles32<false>(pacc, rs, flush_rows_left(n_rows_real, row_w + 4 * kh), c32, 1.0);
#undef X1_GROUP
#undef X1_GROUP_ADDR0
#undef X1_STEP4
#undef X1_STEP
#undef X1_RD
#undef X1_AD
#undef X1_LOAD
#undef X1_LOOKUP
#undef X1_TABLE_ASYNC
}

// a_kind < 0: three-product kernel for every block.  a_kind 0: exact-row kernel (16-byte table entries); with
// d_missing != nullptr the table was built for the block's missing flag (build_lut_kernel) and exactly one of the two
// launches does the work (blocks with missing calls: three products), with d_missing == nullptr the exact-row kernel
// takes every block (the row value of a missing call is the fp16 residual avg - c_s).  a_kind 1 / 2: two-product kernel
// with a constant row table, always.  promote_snps: fp32 run length of the exact-row kernel (0 = default).
int launch_syrk_h3(hipStream_t st, const SyrkPanel &p, const SyrkH3Opts &o)
{
    if (o.n_q <= 0 || o.n_blocks <= 0) return 0;
    const int p3 = H3_PROMOTE / H3_LUTCH;                                    // three products: 512-SNP chunks
    const int p2e = (o.promote_snps > 0 ? o.promote_snps : H3_PROMOTE_EXACT) / (H3_LUTCH / 2);   // exact rows: 256-SNP chunks
    const int p2c = H3_PROMOTE / H3_LUTCH;                                   // constant row table: 512-SNP chunks
    int64_t launched = 0;
    if (o.a_kind < 0 || (o.a_kind == 0 && o.d_missing)) {
        launched++;
        hipLaunchKernelGGL((syrk_h3_kernel<3, false>), dim3((unsigned)o.n_blocks), dim3(256), 0, st, p.w8, p.ncols_pad, o.lut, o.n_q, p.acc, p.ld, p.tiles_c, o.work,
                           o.d_skip_if_zero, o.a_kind == 0 ? o.d_missing : nullptr, p.n_rows_real, 0, p3);
    }
    if (o.a_kind == 0 && o.work_x1 && !o.d_missing) {
        const int n_chunk = (o.n_q + (X1_CHS / 16) - 1) / (X1_CHS / 16);       // table chunks of the block; one launch per fp32 run
        const int run = std::max(1, (o.promote_snps > 0 ? o.promote_snps : H3_PROMOTE_EXACT) / X1_CHS);
        // (fused launch only) blocks flagged by build_lut_kernel run as half-length fp32 runs: the grid is laid out for those
        const int short_div = (o.d_short_runs && run >= 2 && (run % 2) == 0) ? 2 : 1;
        const int n_runs = (n_chunk + run / short_div - 1) / (run / short_div);
        // (round 6: a 16x16x32 form of this kernel -- syrk_uv16_kernel's skeleton, column operands looked up just in time, a padded
        // table layout against the bank conflicts of two quarters per LDS pass -- was built, passed every parity test and ran configs[2]
        // with 2 % missing calls in 883 - 902 ms per step against 896 here, depending on the issue pattern: not kept,
        // profiles/r06_x116_patterns.txt)
        const RunLaunches g{o.n_blocks_x1, n_chunk, run, n_runs, n_runs > 1 ? run_inner_launch() : 0};
        for (int k = 0; k < g.count(); k++)
            for (int half = 0; half < (g.group ? 1 : short_div); half++) {   // (one launch per run, short_div = 2: see the kernel's branch for it)
                const RunLaunch L = g.at(k);
                launched++;
                hipLaunchKernelGGL(syrk_x1_kernel, dim3(L.grid), dim3(256), 0, st, p.w8, p.ncols_pad, o.lut, o.n_q, p.acc, p.ld, p.tiles_c, o.work_x1,
                                   o.d_skip_if_zero, p.n_rows_real, L.chunk_lo, L.chunk_hi, L.n_runs, run, g.group ? L.run_group : half, L.n_items8,
                                   short_div > 1 ? o.d_short_runs : nullptr, short_div);
            }
    } else if (o.a_kind == 0) {
        launched++;
        hipLaunchKernelGGL((syrk_h3_kernel<2, true>), dim3((unsigned)o.n_blocks), dim3(256), 0, st, p.w8, p.ncols_pad, o.lut, o.n_q, p.acc, p.ld, p.tiles_c,
                           o.work, o.d_skip_if_zero, o.d_missing, p.n_rows_real, o.a_kind, p2e > 0 ? p2e : 1);
    } else if (o.a_kind > 0) {
        launched++;
        hipLaunchKernelGGL((syrk_h3_kernel<2, false>), dim3((unsigned)o.n_blocks), dim3(256), 0, st, p.w8, p.ncols_pad, o.lut, o.n_q, p.acc, p.ld, p.tiles_c,
                           o.work, o.d_skip_if_zero, nullptr, p.n_rows_real, o.a_kind, p2c);
    }
    if (o.n_launched) *o.n_launched += launched;
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
