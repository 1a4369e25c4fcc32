// Kernels behind snpgdsPairScore: genotype scores of listed sample pairs from exact integer tables.
//   pair_snp_table   per SNP the 4 x 4 table of the listed pairs' codes (a, b) and the allele flip of flap_allele (gsum < n)
//   pair_flip_words  the flips of 16 SNPs as one mask of high-plane bits
//   pair_words       the listed samples of a block of rows as word-major 2-bit words (16 SNPs per word)
//   pair_count       per pair the 3 x 3 table of the SNPs with codes (a, b), after the flip: bit planes and popcounts
//   pair_matrix      the score of every (SNP, pair), SNP-major
// None of them knows a method or `dosage`: the tables count codes, and the host applies the 4 x 4 score map (pairscore.hip).
// The matrix kernel gets the map as 2-bit fields, which hold the values -1 ... 2 as a bit2 node would.
//
// Rows are read where the caller put them (rb bytes per SNP, any byte address).  A workgroup that gathers the codes of the pairs
// from one row first stages that row in LDS when it fits (PS_LDS_ROW_BYTES), word by word from the aligned words that hold it.
// Only listed sample indices are looked up, so the padding codes of a row's last byte are never read as genotypes.
#include "snpgpu_internal.h"
#include "prep_device.h"

#include <climits>

namespace snpgpu {

constexpr int PS_THREADS = 256;
constexpr int64_t PS_LDS_ROW_BYTES = 60 << 10;      // a longer row is gathered from global memory
constexpr int PS_HEAD_WORDS = 64;                   // dynamic LDS: [4 waves][16] partial counters, then the row
constexpr int PS_WORD_CHUNK = 256;                  // words (4 096 SNPs) per workgroup of the per-pair counter

// bytes [4 j, 4 j + 4) of the row; only aligned words that hold a byte of the row are read, bytes past the row are undefined
__device__ __forceinline__ uint32_t ps_row_word(const uint8_t *row, int64_t rb, int64_t j)
{
    const uintptr_t a = (uintptr_t)(row + 4 * j);
    const int64_t left = rb - 4 * j;
    const int nb = left < 4 ? (int)left : 4;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const int sh = (int)(a & 3);
    uint32_t v = w[0] >> (8 * sh);
    if (sh + nb > 4) v |= w[1] << (32 - 8 * sh);
    return v;
}

// the row of this workgroup as bytes: its copy in LDS (after a barrier), or the row itself
template <bool LDS> __device__ __forceinline__ const uint8_t *ps_stage(uint32_t *lds_row, const uint8_t *row, int64_t rb)
{
    if (!LDS) return row;
    const int64_t nwd = (rb + 3) / 4;
    for (int64_t j = threadIdx.x; j < nwd; j += PS_THREADS) lds_row[j] = ps_row_word(row, rb, j);
    __syncthreads();
    return reinterpret_cast<const uint8_t *>(lds_row);
}

__device__ __forceinline__ unsigned ps_code(const uint8_t *r, int32_t i) { return (r[i >> 2] >> (2 * (i & 3))) & 3u; }

// One workgroup per SNP; lanes run over the pairs.  A wave counts the 16 cells of its 64 pairs with ballots (wave-uniform sums),
// the four waves are added through LDS, and the workgroup stores its SNP's table: no global atomic is needed.
// snp_tab [n_snp][16] (cell 4 a + b) and flip [n_snp] may each be NULL.  flip: n = called genotypes over both lists, gsum their
// sum, from the marginals of the table (a sample counts once per appearance); 1 when gsum < n.
template <bool LDS>
__global__ __launch_bounds__(PS_THREADS) void pair_snp_table_kernel(const uint8_t *__restrict__ geno, int64_t rb, const int32_t *__restrict__ idx1,
                                                                    const int32_t *__restrict__ idx2, int64_t n_pair,
                                                                    int32_t *__restrict__ snp_tab, uint8_t *__restrict__ flip)
{
    extern __shared__ uint32_t ps_lds[];
    int *part = reinterpret_cast<int *>(ps_lds);
    const int64_t s = blockIdx.x;
    const uint8_t *r = ps_stage<LDS>(ps_lds + PS_HEAD_WORDS, geno + s * rb, rb);
    int cnt[16];
#pragma unroll
    for (int k = 0; k < 16; k++) cnt[k] = 0;
    const int64_t n_round = (n_pair + 63) / 64 * 64;             // whole waves take part in every ballot
    for (int64_t p = threadIdx.x; p < n_round; p += PS_THREADS) {
        unsigned cell = 16u;
        if (p < n_pair) cell = 4u * ps_code(r, idx1[p]) + ps_code(r, idx2[p]);
#pragma unroll
        for (int k = 0; k < 16; k++) cnt[k] += __popcll(__ballot(cell == (unsigned)k));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) part[16 * wave + k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int k = threadIdx.x;
        const int tot = part[k] + part[16 + k] + part[32 + k] + part[48 + k];
        if (snp_tab) snp_tab[16 * s + k] = tot;
        part[k] = tot;                                           // only this thread reads or writes column k
    }
    __syncthreads();
    if (flip && threadIdx.x == 0) {
        int64_t n = 0, gsum = 0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 4; b++) {
                n += part[4 * a + b] + part[4 * b + a];          // first member called (a), second member called (a)
                gsum += (int64_t)a * (part[4 * a + b] + part[4 * b + a]);
            }
        flip[s] = gsum < n ? 1 : 0;
    }
}

int launch_pair_snp_table(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, const int32_t *idx1, const int32_t *idx2,
                          int64_t n_pair, int32_t *snp_tab, uint8_t *flip)
{
    if (n_snp <= 0) return 0;
    const dim3 grid((unsigned)n_snp);
    if (rb <= PS_LDS_ROW_BYTES) {
        const size_t lds = sizeof(uint32_t) * (size_t)(PS_HEAD_WORDS + (rb + 3) / 4);
        hipLaunchKernelGGL(pair_snp_table_kernel<true>, grid, dim3(PS_THREADS), lds, st, geno, rb, idx1, idx2, n_pair, snp_tab, flip);
    } else {
        hipLaunchKernelGGL(pair_snp_table_kernel<false>, grid, dim3(PS_THREADS), sizeof(uint32_t) * PS_HEAD_WORDS, st, geno, rb, idx1, idx2,
                           n_pair, snp_tab, flip);
    }
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// fw[w]: bit 2 m + 1 set when SNP 16 w + m of the block is flipped
__global__ __launch_bounds__(PS_THREADS) void pair_flip_words_kernel(const uint8_t *__restrict__ flip, int64_t n_snp, int64_t nw,
                                                                     uint32_t *__restrict__ fw)
{
    const int64_t w = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (w >= nw) return;
    uint32_t v = 0;
    for (int m = 0; m < 16; m++) {
        const int64_t l = 16 * w + m;
        if (l < n_snp && flip[l]) v |= 2u << (2 * m);
    }
    fw[w] = v;
}

int launch_pair_flip_words(hipStream_t st, const uint8_t *flip, int64_t n_snp, uint32_t *fw)
{
    if (n_snp <= 0) return 0;
    const int64_t nw = (n_snp + 15) / 16;
    hipLaunchKernelGGL(pair_flip_words_kernel, dim3((unsigned)((nw + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, st, flip, n_snp, nw, fw);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// words [nw][2 n_pair]: word w of slot t holds SNPs 16 w ... 16 w + 15 of the block at bits 2 m for sample idx1[t] (t < n_pair)
// or idx2[t - n_pair]; SNPs past the block's end are 3.  Word-major, so that the lanes of the counter read neighbouring words.
__global__ __launch_bounds__(PS_THREADS) void pair_words_kernel(const uint8_t *__restrict__ rows, int64_t rb, int64_t n_snp,
                                                                const int32_t *__restrict__ idx, int64_t n_slot, uint32_t *__restrict__ words)
{
    const int64_t t = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x, w = blockIdx.y;
    if (t >= n_slot) return;
    const int32_t i = idx[t];
    uint32_t v = 0;
    for (int m = 0; m < 16; m++) {
        const int64_t l = 16 * w + m;
        unsigned code = 3u;
        if (l < n_snp) code = ps_code(rows + l * rb, i);
        v |= code << (2 * m);
    }
    words[w * n_slot + t] = v;
}

// idx: [2 n_pair], the first list and then the second
int launch_pair_words(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, const int32_t *idx, int64_t n_pair, uint32_t *words)
{
    if (n_snp <= 0) return 0;
    const dim3 grid((unsigned)((2 * n_pair + PS_THREADS - 1) / PS_THREADS), (unsigned)((n_snp + 15) / 16));
    hipLaunchKernelGGL(pair_words_kernel, grid, dim3(PS_THREADS), 0, st, rows, rb, n_snp, idx, 2 * n_pair, words);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// One pair per lane over a chunk of words (grid.y); cell 3 a + b counts the SNPs with codes (a, b), a, b < 3, in 32 bits and is
// added to tab [n_pair][9] with 64-bit integer atomics (zeroed by the caller, carried across the streamed blocks).  fw (or NULL):
// the flip of word w, the same for every lane: it toggles the high plane where the low plane is 0 (0 <-> 2; 1 and 3 stay).
__global__ __launch_bounds__(PS_THREADS) void pair_count_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ fw, int64_t nw,
                                                                int64_t n_pair, unsigned long long *__restrict__ tab)
{
    const int64_t p = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (p >= n_pair) return;
    const int64_t w0 = (int64_t)blockIdx.y * PS_WORD_CHUNK;
    const int64_t w1 = w0 + PS_WORD_CHUNK < nw ? w0 + PS_WORD_CHUNK : nw;
    const uint32_t m55 = GENO_LO_BITS;
    int c[9];
#pragma unroll
    for (int k = 0; k < 9; k++) c[k] = 0;
    for (int64_t w = w0; w < w1; w++) {
        uint32_t x = words[w * 2 * n_pair + p], y = words[w * 2 * n_pair + n_pair + p];
        if (fw) {
            const uint32_t f = fw[w];
            x ^= f & ~((x & m55) << 1);
            y ^= f & ~((y & m55) << 1);
        }
        const uint32_t xl = x & m55, xh = (x >> 1) & m55, yl = y & m55, yh = (y >> 1) & m55;   // (geno_lo / geno_hi as calls change this kernel)
        const uint32_t xe[3] = {~(xl | xh) & m55, xl & ~xh, xh & ~xl};
        const uint32_t ye[3] = {~(yl | yh) & m55, yl & ~yh, yh & ~yl};
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) c[3 * a + b] += __popc(xe[a] & ye[b]);
    }
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (c[k]) atomicAdd(tab + 9 * p + k, (unsigned long long)c[k]);
}

int launch_pair_count(hipStream_t st, const uint32_t *words, const uint32_t *fw, int64_t n_snp, int64_t n_pair, unsigned long long *tab)
{
    if (n_snp <= 0) return 0;
    const int64_t nw = (n_snp + 15) / 16;
    const dim3 grid((unsigned)((n_pair + PS_THREADS - 1) / PS_THREADS), (unsigned)((nw + PS_WORD_CHUNK - 1) / PS_WORD_CHUNK));
    hipLaunchKernelGGL(pair_count_kernel, grid, dim3(PS_THREADS), 0, st, words, fw, nw, n_pair, tab);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// One workgroup per SNP; out [n_snp][n_pair], lanes on neighbouring pairs.  map2: field 4 a + b (2 bits) = map[a][b] & 3, where
// every cell with a missing genotype holds -1.  T = uint8_t stores the field (what a bit2 node keeps: 3 for missing, and for a
// score of -1); T = int32_t stores the value, INT_MIN for a missing genotype.
template <bool LDS, class T>
__global__ __launch_bounds__(PS_THREADS) void pair_matrix_kernel(const uint8_t *__restrict__ geno, int64_t rb, const int32_t *__restrict__ idx1,
                                                                 const int32_t *__restrict__ idx2, int64_t n_pair,
                                                                 const uint8_t *__restrict__ flip, uint32_t map2, T *__restrict__ out)
{
    extern __shared__ uint32_t ps_lds[];
    const int64_t s = blockIdx.x;
    const uint8_t *r = ps_stage<LDS>(ps_lds + PS_HEAD_WORDS, geno + s * rb, rb);
    const bool f = flip && flip[s];
    T *o = out + s * n_pair;
    for (int64_t p = threadIdx.x; p < n_pair; p += PS_THREADS) {
        unsigned a = ps_code(r, idx1[p]), b = ps_code(r, idx2[p]);
        if (f) {
            a = (a & 1u) ? a : a ^ 2u;
            b = (b & 1u) ? b : b ^ 2u;
        }
        const unsigned v = (map2 >> (2 * (4 * a + b))) & 3u;
        if (sizeof(T) == 1)
            o[p] = (T)v;
        else
            o[p] = (a == 3u || b == 3u) ? (T)INT_MIN : (v == 3u ? (T)-1 : (T)v);
    }
}

// elem_size 4: int32 out, 1: uint8 out
int launch_pair_matrix(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, const int32_t *idx1, const int32_t *idx2,
                       int64_t n_pair, const uint8_t *flip, uint32_t map2, int elem_size, void *out)
{
    if (n_snp <= 0) return 0;
    const dim3 grid((unsigned)n_snp), block(PS_THREADS);
    const bool lds = rb <= PS_LDS_ROW_BYTES;
    const size_t bytes = sizeof(uint32_t) * (size_t)(PS_HEAD_WORDS + (lds ? (rb + 3) / 4 : 0));
    if (elem_size == 4) {
        if (lds) hipLaunchKernelGGL((pair_matrix_kernel<true, int32_t>), grid, block, bytes, st, geno, rb, idx1, idx2, n_pair, flip, map2, (int32_t *)out);
        else hipLaunchKernelGGL((pair_matrix_kernel<false, int32_t>), grid, block, bytes, st, geno, rb, idx1, idx2, n_pair, flip, map2, (int32_t *)out);
    } else {
        if (lds) hipLaunchKernelGGL((pair_matrix_kernel<true, uint8_t>), grid, block, bytes, st, geno, rb, idx1, idx2, n_pair, flip, map2, (uint8_t *)out);
        else hipLaunchKernelGGL((pair_matrix_kernel<false, uint8_t>), grid, block, bytes, st, geno, rb, idx1, idx2, n_pair, flip, map2, (uint8_t *)out);
    }
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
