// Linkage disequilibrium between SNP pairs (snpgdsLDMat, src/genLD.cpp:957-1010): the 3 x 3 genotype table of every pair
// on the MX-fp4 MFMA, then one fp64 thread per pair for the LD value.
//
// Every LD method of the reference is a function of ONE table per SNP pair (i, j): n_ab = number of samples with genotype a at
// SNP i and b at SNP j, over the samples called at both (the Num_* / Sum_* lookup tables of src/genLD.cpp:103-168 are linear in
// those nine cells).  n_ab = P_a(i) . P_b(j) with P_a the one-hot plane "genotype == a" over the samples: nine binary
// contractions, run as v_mfma_scale_f32_32x32x64_f8f6f4 with both operands e2m1 (cbsz = blgp = 4, unit scales).  A plane bit is
// the nibble 0b0010 = 1.0, so products are 0 / 1 and the fp32 sums exact while N < 2^24.
//
// Operand form.  Rows are SNPs in the staging layout of csrc/ld.hip: 2-bit codes, 4 samples per byte LSB first, `rbp` bytes per
// row (a multiple of 32), every code of a sample >= n_samp forced to 3 (missing) by ld_stage_kernel, whatever the caller's
// padding held.  Lane l of a wave takes SNP row (l & 31) and, per 128-sample step, the 16 bytes at 32 s + 16 (l >> 5): two
// k-steps of 32 samples.  A dword of 16 codes splits into two nibble dwords (even / odd samples) with shifts, and each plane is
// ONE v_bitop3_b32 of (bit 0 of the code, bit 1 of the code, 0x22222222).  The sample order inside K differs from file order;
// both operands use the same one, which is all a contraction needs.
#include "snpgpu_internal.h"
#include "ld_device.h"

#include <cmath>
#include <cfloat>

namespace snpgpu {

namespace {

typedef float ld_f32x16 __attribute__((ext_vector_type(16)));
typedef int ld_i32x4 __attribute__((ext_vector_type(4)));
typedef int ld_i32x8 __attribute__((ext_vector_type(8)));

constexpr uint32_t LD_NIB = 0x22222222u;   // bit 1 of every nibble: e2m1 1.0
// v_bitop3_b32 truth tables over (a = code bit 0, b = code bit 1, c = LD_NIB); a = 0xF0, b = 0xCC, c = 0xAA
constexpr int LD_P0 = 0x02;   // ~a & ~b & c : code 0
constexpr int LD_P1 = 0x20;   //  a & ~b & c : code 1
constexpr int LD_P2 = 0x08;   // ~a &  b & c : code 2   (code 3 = missing sets no plane)

struct Planes { ld_i32x4 p[3]; };

// 32 samples (two dwords of codes) -> the three one-hot operand registers of one k-step
__device__ __forceinline__ Planes ld_planes(uint32_t w0, uint32_t w1)
{
    Planes r;
    const uint32_t e0a = w0 << 1, e0b = w0, o0a = w0 >> 1, o0b = w0 >> 2;   // even samples: bits 4k, 4k+1 -> 4k+1; odd: 4k+2, 4k+3
    const uint32_t e1a = w1 << 1, e1b = w1, o1a = w1 >> 1, o1b = w1 >> 2;
#define LD_PLANE(P, T)                                                                  \
    r.p[P][0] = (int)__builtin_amdgcn_bitop3_b32(e0a, e0b, LD_NIB, T);                 \
    r.p[P][1] = (int)__builtin_amdgcn_bitop3_b32(o0a, o0b, LD_NIB, T);                 \
    r.p[P][2] = (int)__builtin_amdgcn_bitop3_b32(e1a, e1b, LD_NIB, T);                 \
    r.p[P][3] = (int)__builtin_amdgcn_bitop3_b32(o1a, o1b, LD_NIB, T);
    LD_PLANE(0, LD_P0)
    LD_PLANE(1, LD_P1)
    LD_PLANE(2, LD_P2)
#undef LD_PLANE
    return r;
}

__device__ __forceinline__ void ld_mfma9(ld_f32x16 (&c)[9], const Planes &a, const Planes &b)
{
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) {
            const ld_i32x8 av = __builtin_shufflevector(a.p[x], a.p[x], 0, 1, 2, 3, -1, -1, -1, -1);
            const ld_i32x8 bv = __builtin_shufflevector(b.p[y], b.p[y], 0, 1, 2, 3, -1, -1, -1, -1);
            c[3 * x + y] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c[3 * x + y], 4, 4, 0, 0, 0, 0);
        }
}

// One workgroup = a 64 x 64 tile of SNP pairs, four waves of 32 x 32.  BAND = false: rows A [0, n_a) x rows B [0, n_b), tile
// (blockIdx.x, blockIdx.y), tab[(i n_b + j) 9 + 3 a + b].  BAND = true: A = B = the resident rows, i in [i_lo, i_lo + n_a),
// partners j = i + k, k = 1 ... slide, j < n_b; row tile blockIdx.x, column tile = row tile + blockIdx.y (tiles wholly outside
// the band return at once), tab[((i - i_lo) slide + k - 1) 9 + 3 a + b].  Both buffers hold whole 64-row tiles (rows past n_a /
// n_b are read, never written).
template <bool BAND>
__global__ __launch_bounds__(256, 2) void ld_count_kernel(const uint8_t *__restrict__ A, const uint8_t *__restrict__ B, int64_t rbp,
                                                          int n_a, int n_b, int slide, int32_t *__restrict__ tab)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int ti0 = blockIdx.x * 64;                 // first A row of the tile (relative to A)
    int tj0;                                         // first B row of the tile
    if (BAND) {
        tj0 = ti0 + blockIdx.y * 64;                 // B row index of A row ti0 is ti0 (A = B + i_lo rows, see launcher)
        if ((int)blockIdx.y * 64 - 63 > slide || tj0 >= n_b) return;
    } else {
        tj0 = blockIdx.y * 64;
    }
    const uint8_t *pa = A + (int64_t)(ti0 + 32 * wr + li) * rbp + 16 * kh;
    const uint8_t *pb = B + (int64_t)(tj0 + 32 * wc + li) * rbp + 16 * kh;
    ld_f32x16 c[9];
#pragma unroll
    for (int q = 0; q < 9; q++)
#pragma unroll
        for (int r = 0; r < 16; r++) c[q][r] = 0.f;
    const int steps = (int)(rbp / 32);
    uint4 va = *reinterpret_cast<const uint4 *>(pa), vb = *reinterpret_cast<const uint4 *>(pb);
    for (int s = 0; s < steps; s++) {
        const uint4 ca = va, cb = vb;
        if (s + 1 < steps) {                          // next step's words while this one's MFMAs run
            va = *reinterpret_cast<const uint4 *>(pa + 32 * (s + 1));
            vb = *reinterpret_cast<const uint4 *>(pb + 32 * (s + 1));
        }
        ld_mfma9(c, ld_planes(ca.x, ca.y), ld_planes(cb.x, cb.y));
        ld_mfma9(c, ld_planes(ca.z, ca.w), ld_planes(cb.z, cb.w));
    }
    // c[q][r]: A row 32 wr + 4 kh + (r & 3) + 8 (r >> 2) of the tile, B row 32 wc + li
    const int j = tj0 + 32 * wc + li;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int i = ti0 + 32 * wr + 4 * kh + (r & 3) + 8 * (r >> 2);
        int32_t *dst;
        if (BAND) {
            // A row i sits at B row i (+ i_lo, folded into both pointers by the launcher)
            const int k = j - i;
            if (i >= n_a || j >= n_b || k < 1 || k > slide) continue;
            dst = tab + ((int64_t)i * slide + (k - 1)) * 9;
        } else {
            if (i >= n_a || j >= n_b) continue;
            dst = tab + ((int64_t)i * n_b + j) * 9;
        }
#pragma unroll
        for (int q = 0; q < 9; q++) dst[q] = (int32_t)c[q][r];
    }
}

// Copy `n` caller rows (SNPGPU_GENO_PACKED2 rows of `rb` bytes, or SNPGPU_GENO_U8 rows of n_samp bytes) into staging rows of `rbp`
// bytes: codes of samples >= n_samp and every byte past the row become 3, U8 values > 2 become 3.  One thread per output byte.
__global__ void ld_stage_kernel(const uint8_t *__restrict__ src, int format, int64_t n, int64_t n_samp, int64_t rb, int64_t rbp,
                                uint8_t *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * rbp) return;
    const int64_t row = t / rbp, b = t - row * rbp;
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t s = 4 * b + q;
        uint32_t code = 3;
        if (s < n_samp) {
            if (format == SNPGPU_GENO_U8) {
                const uint32_t g = src[row * n_samp + s];
                code = g > 2 ? 3u : g;
            } else {
                code = (src[row * rb + b] >> (2 * q)) & 3u;
            }
        }
        v |= code << (2 * q);
    }
    dst[t] = (uint8_t)v;
}

// Band finaliser: tables [n_i][slide][9] of rows i = i0 ... (global SNP index i0 + t) -> out[t slide + k - 1]; partners past the last
// SNP (global index >= n_snp) give NaN.
__global__ void ld_final_band_kernel(const int32_t *__restrict__ tab, int64_t n_i, int slide, int64_t i0, int64_t n_snp, int method,
                                     double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_i * slide) return;
    const int64_t i = i0 + t / slide, j = i + (t % slide) + 1;
    if (j >= n_snp) { out[t] = __builtin_nan(""); return; }
    long n[9];
#pragma unroll
    for (int q = 0; q < 9; q++) n[q] = tab[t * 9 + q];
    out[t] = ld_value(method, n);
}

// Rectangle finaliser of a full-matrix row panel: tables [n_i][n_j][9] of rows i0 + t x columns 0 ... n_j - 1 -> out[t n_j + j].
// A pair below the diagonal is evaluated on the transposed table, i.e. exactly as the pair (j, i): the matrix is symmetric bit
// for bit, as the reference's (it computes each unordered pair once).
__global__ void ld_final_rect_kernel(const int32_t *__restrict__ tab, int64_t n_i, int64_t n_j, int64_t i0, int method,
                                     double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_i * n_j) return;
    const int64_t i = i0 + t / n_j, j = t % n_j;
    long n[9];
    if (i <= j) {
#pragma unroll
        for (int q = 0; q < 9; q++) n[q] = tab[t * 9 + q];
    } else {
#pragma unroll
        for (int q = 0; q < 9; q++) n[3 * (q % 3) + q / 3] = tab[t * 9 + q];
    }
    out[t] = ld_value(method, n);
}

// Pruning finaliser (snpgpu_ld_prune, csrc/ld_prune.hip): band tables [n_i][w][9] of rows i = i0 + t (chromosome indices) -> one
// threshold bit per pair, bits[t wpr + (k - 1) / 64] bit (k - 1) % 64 = |LD(pair (i, i + k))| > threshold, 0 when k > w or
// i + k >= n_snp (the band kernel wrote no table there) and when the value is NaN.  The kept SNP is the first argument of the
// reference's _CalcLD: i itself in the forward pass (i >= start), the later SNP i + k in the backward pass (i < start), whose
// table is the transpose -- the same orientation rule as ld_final_rect_kernel's, so r / dprime see the EM in the same order.
// One wave per output word: lane l takes k = 64 word + l + 1, and the word is the wave's ballot.
__global__ __launch_bounds__(256) void ld_prune_bits_kernel(const int32_t *__restrict__ tab, int64_t n_i, int w, int64_t wpr, int64_t i0,
                                                            int64_t n_snp, int64_t start, int method, double threshold,
                                                            unsigned long long *__restrict__ bits)
{
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;   // output word (uniform across the wave)
    const int lane = threadIdx.x & 63;
    if (g >= n_i * wpr) return;
    const int64_t t = g / wpr, i = i0 + t;
    const int64_t k = (g - t * wpr) * 64 + lane + 1;
    bool bit = false;
    if (k <= w && i + k < n_snp) {
        const int32_t *c = tab + (t * w + (k - 1)) * 9;
        long n[9];
        if (i >= start) {
#pragma unroll
            for (int q = 0; q < 9; q++) n[q] = c[q];
        } else {
#pragma unroll
            for (int q = 0; q < 9; q++) n[3 * (q % 3) + q / 3] = c[q];
        }
        bit = fabs(ld_value(method, n)) > threshold;      // NaN: false, as `fabs(NaN) > LD_threshold` in the reference
    }
    const unsigned long long word = __ballot(bit);
    if (lane == 0) bits[g] = word;
}

constexpr int FIN_THREADS = 256;

}  // namespace

int launch_ld_stage(hipStream_t st, const void *src, int format, int64_t n, int64_t n_samp, int64_t rbp, uint8_t *dst)
{
    const int64_t total = n * rbp;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(ld_stage_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint8_t *)src, format, n,
                       n_samp, (n_samp + 3) / 4, rbp, dst);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_count_rect(hipStream_t st, const uint8_t *A, int n_a, const uint8_t *B, int n_b, int64_t rbp, int32_t *tab)
{
    if (n_a <= 0 || n_b <= 0) return 0;
    hipLaunchKernelGGL(ld_count_kernel<false>, dim3((unsigned)((n_a + 63) / 64), (unsigned)((n_b + 63) / 64)), dim3(256), 0, st, A,
                       B, rbp, n_a, n_b, 0, tab);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_count_band(hipStream_t st, const uint8_t *rows, int i_lo, int n_i, int n_rows, int slide, int64_t rbp, int32_t *tab)
{
    if (n_i <= 0) return 0;
    // A = B = rows shifted by i_lo: row indices inside the kernel are relative to i_lo on both sides
    const uint8_t *base = rows + (int64_t)i_lo * rbp;
    hipLaunchKernelGGL(ld_count_kernel<true>, dim3((unsigned)((n_i + 63) / 64), (unsigned)((63 + slide) / 64 + 1)), dim3(256), 0, st,
                       base, base, rbp, n_i, n_rows - i_lo, slide, tab);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_final_band(hipStream_t st, const int32_t *tab, int64_t n_i, int slide, int64_t i0, int64_t n_snp, int method, double *out)
{
    const int64_t total = n_i * slide;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(ld_final_band_kernel, dim3((unsigned)((total + FIN_THREADS - 1) / FIN_THREADS)), dim3(FIN_THREADS), 0, st, tab,
                       n_i, slide, i0, n_snp, method, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_final_rect(hipStream_t st, const int32_t *tab, int64_t n_i, int64_t n_j, int64_t i0, int method, double *out)
{
    const int64_t total = n_i * n_j;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(ld_final_rect_kernel, dim3((unsigned)((total + FIN_THREADS - 1) / FIN_THREADS)), dim3(FIN_THREADS), 0, st, tab,
                       n_i, n_j, i0, method, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_prune_bits(hipStream_t st, const int32_t *tab, int64_t n_i, int w, int64_t i0, int64_t n_snp, int64_t start, int method,
                         double threshold, uint64_t *bits)
{
    const int64_t wpr = (w + 63) / 64;
    const int64_t threads = n_i * wpr * 64;
    if (threads <= 0) return 0;
    hipLaunchKernelGGL(ld_prune_bits_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, tab, n_i, w, wpr, i0, n_snp,
                       start, method, threshold, (unsigned long long *)bits);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
