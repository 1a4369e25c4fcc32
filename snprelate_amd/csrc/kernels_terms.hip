// Per-sample terms that travel beside the SYRK products of a feed block (fp64, from the pair-coded words or the packed rows;
// launched by feed_syrk, ctx_feed.hip, after the tables of kernels_tables.hip and the words of kernels_transpose.hip):
//   colcorr / colterm_add           column term of the exact-row SYRK
//   uvcorr / uvterm_add             row / column terms of the single-product SYRK
//   homo_miss_sums / homo_miss_add  KING-homo per-sample missing sums (launch_homo_miss_sums)
//   eigmix_samples                  EIGMIX per-sample sums
//   uv_sparse                       rare variants in fp64
#include "snpgpu_internal.h"
#include "prep_device.h"

namespace snpgpu {

// The three column-sum pairs (colcorr / colterm_add, uvcorr / uvterm_add, homo_miss_sums / homo_miss_add) share one skeleton: one
// thread per column, blockIdx.y = a chunk of COL_CHUNK_WORDS words (H3_LUTCH / 2 SNPs) whose partial sums go to tc[chunk][col]; the
// second kernel adds the partials in chunk order, so the sums do not depend on the launch geometry.
constexpr int COL_CHUNK_WORDS = H3_LUTCH / 16;
struct ChunkRange { int d0, d1; };
__device__ __forceinline__ ChunkRange col_chunk_range(int n_d)
{
    const int d0 = blockIdx.y * COL_CHUNK_WORDS;
    return {d0, (d0 + COL_CHUNK_WORDS < n_d) ? (d0 + COL_CHUNK_WORDS) : n_d};
}
__device__ __forceinline__ void add_chunk_partials(const double *tc, int n_chunk, int64_t ncols_pad, int64_t col,
                                                   double *dst)
{
    double s = dst[col];
    for (int k = 0; k < n_chunk; k++) s += tc[(int64_t)k * ncols_pad + col];
    dst[col] = s;
}
// partials of two sums: dst[col] and dst[ncols_pad + col]
__device__ __forceinline__ void add_chunk_partials(const double2 *tc, int n_chunk, int64_t ncols_pad, int64_t col,
                                                   double *dst)
{
    double s1 = dst[col], s2 = dst[ncols_pad + col];
    for (int k = 0; k < n_chunk; k++) { const double2 t = tc[(int64_t)k * ncols_pad + col]; s1 += t.x; s2 += t.y; }
    dst[col] = s1; dst[ncols_pad + col] = s2;
}
struct ColChunks {      // launch geometry of a pair: grid of the partial-sum kernel; the adder takes grid.x workgroups
    int n_chunk;
    dim3 grid;
    ColChunks(int64_t ncols_pad, int n_d)
        : n_chunk((n_d + COL_CHUNK_WORDS - 1) / COL_CHUNK_WORDS), grid((unsigned)((ncols_pad + 255) / 256), (unsigned)n_chunk) {}
};
// true where the block's missing-call flag takes the block away from a colcorr launch that serves `blocks`
// (if / return: as one return expression it changes colcorr_kernel's code)
__device__ __forceinline__ bool colcorr_skips(int blocks, const unsigned long long *d_missing)
{
    if (blocks == (int)ColcorrBlocks::WithMissing ? (*d_missing == 0ull)
                                                  : (blocks == (int)ColcorrBlocks::WithoutMissing && *d_missing != 0ull))
        return true;
    return false;
}

// Column term of the exact-row-side SYRK: T[j] += sum over the block's SNPs of (avg_s - c_s) w_s(g_js) = u_s + v_s g_js
// (fp64; g_js from the pair-coded words W8, byte = 16 * (c0 + 4 * c1)).  Cells with code 3 (missing calls, SNP / sample
// padding) have w = 0 and contribute nothing.  One thread per column walks the block in SNP order, so the sum does not
// depend on the launch geometry.  blocks == WithoutMissing: only for blocks without missing calls (the others take the three-product
// kernel).  The term is the same for every row of the panel: it is subtracted once, by colterm_settle_kernel.
__global__ __launch_bounds__(256) void colcorr_kernel(const uint32_t *__restrict__ w8, int64_t ncols_pad, int n_d,
                                                      const double2 *__restrict__ ccoef, double *__restrict__ tc,
                                                      const unsigned long long *__restrict__ d_missing, int blocks,
                                                      int entry12)
{
    // blocks: a ColcorrBlocks (WithMissing: the blocks without take the single-product kernel and uvcorr_kernel)
    if (colcorr_skips(blocks, d_missing)) return;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols_pad) return;
    const ChunkRange ch = col_chunk_range(n_d);
    double s = 0.0;
    for (int d = ch.d0; d < ch.d1; d++) {
        const uint32_t w = w8[(int64_t)d * ncols_pad + col];
        const double2 *__restrict__ cf = ccoef + (int64_t)d * 8;     // wave-uniform: scalar loads
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const uint32_t by = (w >> (8 * p)) & 0xFFu;
            const uint32_t b = entry12 ? (by * 171u) >> 11 : by >> 4, c0 = b & 3u, c1 = b >> 2;   // bytes carry 12 / 16 * code here
            const double2 f0 = cf[2 * p], f1 = cf[2 * p + 1];
            s += (c0 == 3u) ? 0.0 : (f0.x + f0.y * (double)c0);
            s += (c1 == 3u) ? 0.0 : (f1.x + f1.y * (double)c1);
        }
    }
    tc[(int64_t)blockIdx.y * ncols_pad + col] = s;
}

// colterm[j] += the chunk sums of this block, in chunk order
__global__ __launch_bounds__(256) void colterm_add_kernel(const double *__restrict__ tc, int n_chunk, int64_t ncols_pad,
                                                          double *__restrict__ colterm,
                                                          const unsigned long long *__restrict__ d_missing, int blocks)
{
    if (colcorr_skips(blocks, d_missing)) return;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols_pad) return;
    add_chunk_partials(tc, n_chunk, ncols_pad, col, colterm);
}

int launch_colcorr(hipStream_t st, const uint32_t *w8, int64_t ncols_pad, int n_d, const double2 *ccoef, double *tc,
                   double *colterm, const unsigned long long *d_missing, ColcorrBlocks blocks, int entry12)
{
    if (n_d <= 0) return 0;
    const ColChunks g(ncols_pad, n_d);
    hipLaunchKernelGGL(colcorr_kernel, g.grid, dim3(256), 0, st, w8, ncols_pad, n_d, ccoef, tc, d_missing, (int)blocks, entry12);
    hipLaunchKernelGGL(colterm_add_kernel, dim3(g.grid.x), dim3(256), 0, st, tc, g.n_chunk, ncols_pad, colterm, d_missing, (int)blocks);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// Rare variants of a block without missing calls, in fp64 and with the exact weight y^2.  With g' the count of the MINOR
// allele (g or 2 - g; (g - avg) = -(g' - avg') so the products are the same) and C the carriers (g' > 0; at most
// UV_SPARSE_MAC of them):   y^2 (g'_i - avg')(g'_j - avg') = y^2 g'_i g'_j - y^2 avg' g'_i - y^2 avg' g'_j + y^2 avg'^2,
// i.e. |C|(|C| + 1) / 2 entries of the accumulator plus sparse additions to the row / column / constant terms that
// colterm_settle_kernel applies (acc[i][j] -= R[i] + Q[j] - K).  One wave per SNP: the lanes scan the SNP's packed row
// (16 bytes = 64 samples a time), collect the carriers in LDS and share out the pairs.
__global__ __launch_bounds__(256) void uv_sparse_kernel(const uint8_t *__restrict__ packed, int64_t RB, int64_t n_snp,
                                                        int64_t N, int64_t row0, int64_t row1, int64_t col0,
                                                        const double4 *__restrict__ uvsp, double *__restrict__ acc,
                                                        int64_t ld, int64_t tiles_c, int64_t ncols_pad, double *__restrict__ uvterm,
                                                        const unsigned long long *__restrict__ d_missing, int missing_blocks)
{
    // missing_blocks = 0: blocks without missing calls, the SNP has left the dense product altogether (weight 0 there).
    // missing_blocks = 1: blocks WITH missing calls (build_lut_kernel's `rare`): the dense product (exact-row kernel) still
    // holds the SNP with every called genotype replaced by the non-carrier's, i.e. y^2 avg'^2 m_i m_j; what is added here is the
    // rest of y^2 (g'_i - avg')(g'_j - avg') m_i m_j: the carrier pairs' y^2 g'_i g'_j, the carriers' row / column terms
    // y^2 avg' g'_i -- which colterm_settle_kernel subtracts from EVERY entry of the carrier's row and column, so they are
    // given back at the cells (carrier, sample with a missing call), whose pair does not count -- and no constant.
    if (missing_blocks ? (*d_missing == 0ull) : (*d_missing != 0ull)) return;
    constexpr int MAXC = X1_SPARSE_MAC > UV_SPARSE_MAC ? X1_SPARSE_MAC : UV_SPARSE_MAC;
    __shared__ int s_idx[4][MAXC];
    __shared__ int s_g[4][MAXC];
    __shared__ int s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    if (k >= n_snp) return;
    const double4 sp = uvsp[k];
    if (sp.w == 0.0) return;                       // wave-uniform
    if (lane == 0) s_cnt[wave] = 0;
    __builtin_amdgcn_wave_barrier();
    const bool flip = (sp.z != 0.0);
    const uint8_t *__restrict__ row = packed + k * RB;
    for (int64_t b0 = (int64_t)lane * 16; b0 < RB; b0 += 64 * 16) {
        const uint4 q = *reinterpret_cast<const uint4 *>(row + b0);     // RB is a multiple of 64 bytes (samples padded with code 3)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int ws = 0; ws < 4; ws++) {
            if ((flip ? (w[ws] != 0xAAAAAAAAu) : (w[ws] != 0u))) {   // sixteen samples without a copy of the minor allele
                for (int j = 0; j < 16; j++) {
                    const uint32_t code = (w[ws] >> (2 * j)) & 3u;
                    const int64_t smp = b0 * 4 + ws * 16 + j;
                    if (code == 3u || smp >= N) continue;
                    const int gp = flip ? 2 - (int)code : (int)code;
                    if (gp > 0) {
                        const int slot = atomicAdd(&s_cnt[wave], 1);
                        if (slot < MAXC) { s_idx[wave][slot] = (int)smp; s_g[wave][slot] = gp; }
                    }
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    const int cnt = s_cnt[wave] < MAXC ? s_cnt[wave] : MAXC;   // <= the mode's copy limit by construction
    const double y2 = sp.x, ya = sp.x * sp.y;
    for (int a = lane; a < cnt; a += 64) {
        const int64_t c = (int64_t)s_idx[wave][a] - col0;
        if (c >= 0) {
            const double t = ya * (double)s_g[wave][a];
            unsafeAtomicAdd(uvterm + c, t);
            unsafeAtomicAdd(uvterm + ncols_pad + c, t);
        }
    }
    if (lane == 0 && !missing_blocks) unsafeAtomicAdd(uvterm + 2 * ncols_pad, ya * sp.y);
    if (missing_blocks && cnt > 0) {
        for (int64_t b0 = (int64_t)lane * 16; b0 < RB; b0 += 64 * 16) {
            const uint4 q = *reinterpret_cast<const uint4 *>(row + b0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int ws = 0; ws < 4; ws++) {
                uint32_t miss = code3_mask(w[ws]);
                while (miss) {
                    const int bit = __ffs((int)miss) - 1;
                    miss &= miss - 1;
                    const int64_t smp = b0 * 4 + ws * 16 + (bit >> 1);
                    if (smp >= N) break;                                  // sample padding
                    for (int a = 0; a < cnt; a++) {
                        const int64_t ca = s_idx[wave][a];
                        const int64_t i = ca < smp ? ca : smp, j = ca < smp ? smp : ca;
                        if (i >= row0 && i < row1)
                            unsafeAtomicAdd(acc + acc_off(ld, tiles_c, i - col0, j - col0), ya * (double)s_g[wave][a]);
                    }
                }
            }
        }
    }
    const int n_pair = cnt * (cnt + 1) / 2;
    for (int pi = lane; pi < n_pair; pi += 64) {
        // pair number pi -> (a <= b): row b of the lower triangle
        int b = (int)((sqrt(8.0 * pi + 1.0) - 1.0) * 0.5);
        while (b * (b + 1) / 2 > pi) b--;
        while ((b + 1) * (b + 2) / 2 <= pi) b++;
        const int a = pi - b * (b + 1) / 2;
        const int sa = s_idx[wave][a], sb = s_idx[wave][b];
        const int64_t i = sa < sb ? sa : sb, j = sa < sb ? sb : sa;
        if (i >= row0 && i < row1)
            unsafeAtomicAdd(acc + acc_off(ld, tiles_c, i - col0, j - col0), y2 * (double)(s_g[wave][a] * s_g[wave][b]));
    }
}

int launch_uv_sparse(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t N, int64_t row0, int64_t row1,
                     int64_t col0, const double4 *uvsp, double *acc, int64_t ld, int64_t tiles_c, int64_t ncols_pad, double *uvterm,
                     const unsigned long long *d_missing, int missing_blocks)
{
    if (n_snp <= 0) return 0;
    hipLaunchKernelGGL(uv_sparse_kernel, dim3((unsigned)((n_snp + 3) / 4)), dim3(256), 0, st, packed, RB, n_snp, N, row0, row1, col0,
                       uvsp, acc, ld, tiles_c, ncols_pad, uvterm, d_missing, missing_blocks);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// Row / column terms of the single-product SYRK: per sample j, over the block's SNPs,
//   R[j] += sum d_b u v g_js      Q[j] += sum d_a u v g_js       (fp64; bytes of W8 = 8 * (c0 + 4 * c1))
// in per-chunk partial sums added in chunk order (independent of the launch geometry); the centre parts
// sum d_b u v c_a + sum d_a u v c_b are the same for every sample and sit in K with sum d_a d_b u v (uv_tables_kernel).
// Code 3 occurs only as SNP padding (coefficients 0) and sample padding (terms never read): no special case.
__global__ __launch_bounds__(256) void uvcorr_kernel(const uint32_t *__restrict__ w8, int64_t ncols_pad, int n_d,
                                                     const double4 *__restrict__ uvcoef, double2 *__restrict__ tc,
                                                     const unsigned long long *__restrict__ d_missing, int nibble)
{
    if (*d_missing != 0ull) return;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols_pad) return;
    const ChunkRange ch = col_chunk_range(n_d);
    double sr = 0.0, sq = 0.0;
    for (int d = ch.d0; d < ch.d1; d++) {
        const uint32_t w = w8[(int64_t)d * ncols_pad + col];
        const double4 *__restrict__ cf = uvcoef + (int64_t)d * 8;    // wave-uniform: scalar loads
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const uint32_t by = (w >> (8 * p)) & 0xFFu, b = by >> 3;    // 8 * (c0 + 4 c1), or the nibble form c0 | c1 << 4
            const double g0 = nibble ? (double)(by & 3u) : (double)(b & 3u), g1 = nibble ? (double)(by >> 4) : (double)(b >> 2);
            const double4 f0 = cf[2 * p], f1 = cf[2 * p + 1];
            sr = fma(f0.x, g0, sr); sq = fma(f0.z, g0, sq);
            sr = fma(f1.x, g1, sr); sq = fma(f1.z, g1, sq);
        }
    }
    tc[(int64_t)blockIdx.y * ncols_pad + col] = make_double2(sr, sq);
}

__global__ __launch_bounds__(256) void uvterm_add_kernel(const double2 *__restrict__ tc, int n_chunk, int64_t ncols_pad,
                                                         const double *__restrict__ kpart, int n_kpart,
                                                         double *__restrict__ uvterm,
                                                         const unsigned long long *__restrict__ d_missing)
{
    if (*d_missing != 0ull) return;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col == 0) {
        double ks = uvterm[2 * ncols_pad];
        for (int i = 0; i < n_kpart; i++) ks += kpart[i];
        uvterm[2 * ncols_pad] = ks;
    }
    if (col >= ncols_pad) return;
    add_chunk_partials(tc, n_chunk, ncols_pad, col, uvterm);
}

int launch_uvcorr(hipStream_t st, const uint32_t *w8, int64_t ncols_pad, int n_d, const double4 *uvcoef, const double *kpart,
                  int n_kpart, double2 *tc, double *uvterm, const unsigned long long *d_missing, int nibble)
{
    if (n_d <= 0) return 0;
    const ColChunks g(ncols_pad, n_d);
    hipLaunchKernelGGL(uvcorr_kernel, g.grid, dim3(256), 0, st, w8, ncols_pad, n_d, uvcoef, tc, d_missing, nibble);
    hipLaunchKernelGGL(uvterm_add_kernel, dim3(g.grid.x), dim3(256), 0, st, tc, g.n_chunk, ncols_pad, kpart, n_kpart, uvterm, d_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// per-sample sums M1[j] += sum_s w1_s mu_js, M2 likewise, from the pair-coded words (byte = 8 (c0 + 4 c1)): per-chunk partials
// added in chunk order (independent of the launch geometry), as uvcorr_kernel / uvterm_add_kernel
__global__ __launch_bounds__(256) void homo_miss_sums_kernel(const uint32_t *__restrict__ w8, int64_t ncols_pad, int n_d,
                                                             const double2 *__restrict__ wts, double2 *__restrict__ tc,
                                                             const unsigned long long *__restrict__ d_missing)
{
    if (*d_missing == 0ull) return;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols_pad) return;
    const ChunkRange ch = col_chunk_range(n_d);
    double s1 = 0.0, s2 = 0.0;
    for (int d = ch.d0; d < ch.d1; d++) {
        const uint32_t w = w8[(int64_t)d * ncols_pad + col];
        const double2 *__restrict__ cf = wts + (int64_t)d * 8;       // wave-uniform: scalar loads
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const uint32_t b = ((w >> (8 * p)) & 0xFFu) >> 3;
            if ((b & 3u) == 3u) { s1 += cf[2 * p].x; s2 += cf[2 * p].y; }
            if ((b >> 2) == 3u) { s1 += cf[2 * p + 1].x; s2 += cf[2 * p + 1].y; }
        }
    }
    tc[(int64_t)blockIdx.y * ncols_pad + col] = make_double2(s1, s2);
}

__global__ __launch_bounds__(256) void homo_miss_add_kernel(const double2 *__restrict__ tc, int n_chunk, int64_t ncols_pad,
                                                            double *__restrict__ msum,
                                                            const unsigned long long *__restrict__ d_missing)
{
    if (*d_missing == 0ull) return;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols_pad) return;
    add_chunk_partials(tc, n_chunk, ncols_pad, col, msum);
}

int launch_homo_miss_sums(hipStream_t st, const uint32_t *w8, int64_t ncols_pad, int n_d, const double2 *wts, double2 *tc, double *msum,
                          const unsigned long long *d_missing)
{
    if (n_d <= 0) return 0;
    const ColChunks g(ncols_pad, n_d);
    hipLaunchKernelGGL(homo_miss_sums_kernel, g.grid, dim3(256), 0, st, w8, ncols_pad, n_d, wts, tc, d_missing);
    hipLaunchKernelGGL(homo_miss_add_kernel, dim3(g.grid.x), dim3(256), 0, st, tc, g.n_chunk, ncols_pad, msum, d_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

constexpr int EIGMIX_SAMPLES_CHUNK = 128;    // words (of 8 SNPs) per thread of eigmix_samples_kernel
// per-sample sums of EIGMIX over one block (pair-coded words, see transpose8): number of
// heterozygous calls (DiagAdjVal, genEIGMIX.cpp:125-128) and sum of 4p(1-p) over the SNPs where the
// sample is missing (row/column totals of the missing-union denominator, :129-136)
__global__ __launch_bounds__(256) void eigmix_samples_kernel(const uint32_t *__restrict__ w8, int n_d,
                                                             int64_t ncols_pad, int64_t col0,
                                                             const double *__restrict__ dvals,
                                                             uint32_t *__restrict__ het, double *__restrict__ dmiss,
                                                             double *__restrict__ dsq,
                                                             const unsigned long long *__restrict__ d_wide16)
{
    const int64_t sc = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sc >= ncols_pad) return;
    const int sh = (d_wide16 && *d_wide16 == 0ull) ? 4 : 3;     // same rule as transpose8_kernel
    uint32_t h = 0;
    double dm = 0, sq = 0;
    // blockIdx.y: a chunk of EIGMIX_SAMPLES_CHUNK words (one thread per sample over the whole block left a 10 000-sample
    // panel with 157 waves for 65 536 SNPs: 11 ms of a 18 ms step); the chunk sums are added atomically
    const int d_lo = blockIdx.y * EIGMIX_SAMPLES_CHUNK;
    const int d_hi = (d_lo + EIGMIX_SAMPLES_CHUNK < n_d) ? (d_lo + EIGMIX_SAMPLES_CHUNK) : n_d;
    for (int d = d_lo; d < d_hi; d++) {
        const uint32_t w = w8[(int64_t)d * ncols_pad + sc];
#pragma unroll
        for (int t = 0; t < 8; t++) {       // byte p = (8 or 16) * (c0 + 4*c1)
            const uint32_t idx = ((w >> (8 * (t >> 1))) & 0xFFu) >> sh;
            const uint32_t code = (t & 1) ? (idx >> 2) : (idx & 3u);
            const int k = 8 * d + t;
            h += (code == 1u);
            if (code == 3u) dm += dvals[2 * k];
            else { const double z = (double)code - dvals[2 * k + 1]; sq += z * z; }
        }
    }
    if (h) atomicAdd(het + col0 + sc, h);
    if (dm != 0.0) unsafeAtomicAdd(dmiss + col0 + sc, dm);
    unsafeAtomicAdd(dsq + col0 + sc, sq);     // fp64 diagonal numerator: (diag - #het) cancels to ~2 % of its terms
}

int launch_eigmix_samples(hipStream_t st, const uint32_t *w8, int n_d, int64_t ncols_pad, int64_t col0,
                          const double *dvals, uint32_t *het, double *dmiss, double *dsq,
                          const unsigned long long *d_wide16)
{
    if (n_d <= 0) return 0;
    hipLaunchKernelGGL(eigmix_samples_kernel,
                       dim3((unsigned)((ncols_pad + 255) / 256), (unsigned)((n_d + EIGMIX_SAMPLES_CHUNK - 1) / EIGMIX_SAMPLES_CHUNK)),
                       dim3(256), 0, st, w8, n_d,
                       ncols_pad, col0, dvals, het, dmiss, dsq, d_wide16);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
