// Population kernels behind snpgdsFst / snpgdsSlidingWindow:
//   pop_mask     K population masks in the rows' own bit layout (0b01 at the code position of every member sample)
//   pop_count    one pass over the 2-bit rows -> exact per-SNP, per-population counters ACnt (sum of called genotypes) and
//                Cnt (2 x called samples) of WC84 / WH02 (src/genFst.cpp:56-74, :103-120); integer arithmetic only
//   fst_terms    per SNP: W&C84 numerator / denominator / ratio, or the W&H02 ratio, in the reference's operation order
//   fst_sum_*    sums over SNP sets (CSR windows) in ascending SNP order, sequentially in fp64, one lane per output
//
// Rows are read where the caller put them: rb = ceil(N / 4) bytes per SNP, so a row starts anywhere inside a 16-byte line.
// The kernel loads the aligned lines that cover a row (bytes of the neighbouring rows included) and the masks are built
// once per distinct offset h of a row's first byte inside its line (16 / gcd(rb, 16) variants, zero outside the row), so
// neither the neighbours nor the padding codes of the last byte count.
#include "snpgpu_internal.h"
#include "prep_device.h"

namespace snpgpu {

constexpr int POP_SNPS = 4;       // SNPs per workgroup; they share the line offset, hence every mask load

__global__ __launch_bounds__(256) void pop_mask_kernel(const int32_t *__restrict__ pop, int64_t N, int64_t rb, int K, int h0, int g,
                                                       int64_t mbytes, uint8_t *__restrict__ mask)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= mbytes) return;
    const int k = blockIdx.y, s = blockIdx.z;
    const int h = (h0 + s * g) & 15;
    const int64_t i = j - h;                       // byte of the row
    unsigned out = 0;
    if (i >= 0 && i < rb) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int64_t smp = 4 * i + t;
            if (smp < N && pop[smp] == k) out |= 1u << (2 * t);
        }
    }
    mask[((int64_t)s * K + k) * mbytes + j] = (uint8_t)out;
}

// plane algebra of count_word (prep_device.h) under a population mask
template <int KG>
__device__ __forceinline__ void pop_word(uint32_t w, const uint32_t (&m)[KG], int (&n1)[KG], int (&n2)[KG], int (&nc)[KG])
{
    const uint32_t lo = w & GENO_LO_BITS, hi = (w >> 1) & GENO_LO_BITS;   // (geno_lo / geno_hi as calls change pop_count_kernel: inline copy)
    const uint32_t one = lo & ~hi, two = hi & ~lo, called = GENO_LO_BITS & ~(lo & hi);
#pragma unroll
    for (int k = 0; k < KG; k++) {
        n1[k] += __popc(one & m[k]);
        n2[k] += __popc(two & m[k]);
        nc[k] += __popc(called & m[k]);
    }
}

// One workgroup per POP_SNPS SNPs of one line offset; populations in register groups of KG.  mask: [n_var][K][mvec] uint4.
template <int KG>
__global__ __launch_bounds__(256) void pop_count_kernel(const uint8_t *__restrict__ geno, int64_t rb, int64_t n_snp, int K, int n_var,
                                                        int h0, int g, int64_t mvec, const uint4 *__restrict__ mask,
                                                        int32_t *__restrict__ acnt, int32_t *__restrict__ cnt)
{
    const int c = (int)(blockIdx.x % (unsigned)n_var);
    const int64_t q = blockIdx.x / (unsigned)n_var;
    int64_t snp[POP_SNPS];
    const uint4 *row[POP_SNPS];
    const int s = (int)((((int64_t)c * (rb & 15)) & 15) / g);          // mask variant of these rows
    const int h = (h0 + s * g) & 15;
#pragma unroll
    for (int i = 0; i < POP_SNPS; i++) {
        snp[i] = (q * POP_SNPS + i) * n_var + c;
        const int64_t r = snp[i] < n_snp ? snp[i] : c;                 // c < n_var <= n_snp: a row that exists
        row[i] = reinterpret_cast<const uint4 *>(geno + r * rb - h);
    }
    const int nv = (int)((h + rb + 15) >> 4);                          // lines that cover a row (<= mvec)
    const uint4 *mk = mask + (int64_t)s * K * mvec;
    __shared__ int red[4][POP_SNPS][KG][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

    for (int k0 = 0; k0 < K; k0 += KG) {
        int n1[POP_SNPS][KG], n2[POP_SNPS][KG], nc[POP_SNPS][KG];
#pragma unroll
        for (int i = 0; i < POP_SNPS; i++)
#pragma unroll
            for (int k = 0; k < KG; k++) n1[i][k] = n2[i][k] = nc[i][k] = 0;
        for (int v = threadIdx.x; v < nv; v += 256) {
            uint32_t mx[KG], my[KG], mz[KG], mw[KG];
#pragma unroll
            for (int k = 0; k < KG; k++) {
                uint4 m = make_uint4(0, 0, 0, 0);
                if (k0 + k < K) m = mk[(int64_t)(k0 + k) * mvec + v];
                mx[k] = m.x; my[k] = m.y; mz[k] = m.z; mw[k] = m.w;
            }
#pragma unroll
            for (int i = 0; i < POP_SNPS; i++) {
                const uint4 d = row[i][v];
                pop_word<KG>(d.x, mx, n1[i], n2[i], nc[i]);
                pop_word<KG>(d.y, my, n1[i], n2[i], nc[i]);
                pop_word<KG>(d.z, mz, n1[i], n2[i], nc[i]);
                pop_word<KG>(d.w, mw, n1[i], n2[i], nc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < POP_SNPS; i++)
#pragma unroll
            for (int k = 0; k < KG; k++) {
                int a = n1[i][k], b = n2[i][k], d = nc[i][k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    a += __shfl_down(a, off);
                    b += __shfl_down(b, off);
                    d += __shfl_down(d, off);
                }
                if (lane == 0) { red[wave][i][k][0] = a; red[wave][i][k][1] = b; red[wave][i][k][2] = d; }
            }
        __syncthreads();
        if (threadIdx.x < POP_SNPS * KG) {
            const int i = threadIdx.x / KG, k = threadIdx.x % KG;
            if (snp[i] < n_snp && k0 + k < K) {
                int t[3];
#pragma unroll
                for (int x = 0; x < 3; x++) t[x] = red[0][i][k][x] + red[1][i][k][x] + red[2][i][k][x] + red[3][i][k][x];
                acnt[snp[i] * K + k0 + k] = t[0] + 2 * t[1];
                cnt[snp[i] * K + k0 + k] = 2 * t[2];
            }
        }
        __syncthreads();
    }
}

int launch_pop_mask(hipStream_t st, const int32_t *pop, int64_t n_samp, int64_t rb, int K, int n_var, int h0, int g, int64_t mbytes,
                    uint8_t *mask)
{
    dim3 grid((unsigned)((mbytes + 255) / 256), (unsigned)K, (unsigned)n_var);
    hipLaunchKernelGGL(pop_mask_kernel, grid, dim3(256), 0, st, pop, n_samp, rb, K, h0, g, mbytes, mask);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// geno: n_snp rows of rb bytes; (uintptr_t)geno & 15 == h0; acnt / cnt: [n_snp][K] of these rows
int launch_pop_count(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, int K, int n_var, int h0, int g, int64_t mvec,
                     const void *mask, int32_t *acnt, int32_t *cnt)
{
    if (n_snp <= 0) return 0;
    if (n_snp < n_var) n_var = (int)n_snp;      // rows 0 ... n_snp - 1 use the variants 0 ... n_snp - 1 of the same table
    const int64_t per = (n_snp + n_var - 1) / n_var, groups = (per + POP_SNPS - 1) / POP_SNPS;
    const dim3 grid((unsigned)(groups * n_var)), block(256);
    // the fewest register slots for K populations, the larger group on a tie
    int kg = 4;
    if (K <= 4) kg = K < 2 ? 2 : K;
    else if ((K + 2) / 3 * 3 < (K + 3) / 4 * 4) kg = 3;
    const uint4 *m = (const uint4 *)mask;
    if (kg == 2) hipLaunchKernelGGL(pop_count_kernel<2>, grid, block, 0, st, geno, rb, n_snp, K, n_var, h0, g, mvec, m, acnt, cnt);
    else if (kg == 3) hipLaunchKernelGGL(pop_count_kernel<3>, grid, block, 0, st, geno, rb, n_snp, K, n_var, h0, g, mvec, m, acnt, cnt);
    else hipLaunchKernelGGL(pop_count_kernel<4>, grid, block, 0, st, geno, rb, n_snp, K, n_var, h0, g, mvec, m, acnt, cnt);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// fp64 part: every expression in the reference's order, no contraction into FMAs
#pragma clang fp contract(off)

__device__ __forceinline__ double pop_freq(const int32_t *a, const int32_t *c, int k) { return (double)a[k] / c[k]; }

// H[k1][k2] of WH02 (src/genFst.cpp:131-139), k1 <= k2
__device__ __forceinline__ double wh02_h(const int32_t *a, const int32_t *c, int k1, int k2)
{
    const double p1 = pop_freq(a, c, k1);
    if (k1 == k2) return 2.0 * c[k1] / (c[k1] - 1) * p1 * (1 - p1);
    const double p2 = pop_freq(a, c, k2);
    return p1 + p2 - 2 * p1 * p2;
}

// method 1: num / den / ratio of WC84 (:76-98); method 2: ratio = WH02_beta of the SNP's own H (:143-166).
// valid = 0 (ratio NaN) when a population has no called sample.  n_c sums Cnt^2 exactly (the reference's int product
// overflows beyond 23 170 called samples in a population).
__global__ __launch_bounds__(256) void fst_terms_kernel(int method, const int32_t *__restrict__ acnt, const int32_t *__restrict__ cnt,
                                                        int64_t n_snp, int K, double *__restrict__ num, double *__restrict__ den,
                                                        double *__restrict__ ratio, uint8_t *__restrict__ valid)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_snp) return;
    const int32_t *a = acnt + s * K, *c = cnt + s * K;
    int64_t at = 0, ct = 0;
    bool ok = true;
    for (int k = 0; k < K; k++) { at += a[k]; ct += c[k]; ok = ok && c[k] > 0; }
    valid[s] = ok ? 1 : 0;
    if (!ok) {
        ratio[s] = __builtin_nan("");
        if (method == 1) { num[s] = 0; den[s] = 0; }
        return;
    }
    if (method == 1) {
        const double p_all = (double)at / (double)ct;
        double msb = 0, msw = 0, n_c = 0;
        for (int k = 0; k < K; k++) {
            const double p = pop_freq(a, c, k);
            msb += c[k] * (p - p_all) * (p - p_all);
            msw += c[k] * p * (1 - p);
            n_c += (double)((int64_t)c[k] * c[k]);
        }
        msb /= (double)(K - 1);
        msw /= (double)(ct - K);
        n_c = ((double)ct - n_c / (double)ct) / (double)(K - 1);
        const double nu = msb - msw, de = msb + (n_c - 1) * msw;
        num[s] = nu; den[s] = de;
        ratio[s] = nu / de;
    } else {
        double hw = 0, hb = 0;
        for (int k1 = 0; k1 < K; k1++) {
            hw += wh02_h(a, c, k1, k1);
            for (int k2 = k1 + 1; k2 < K; k2++) hb += wh02_h(a, c, k1, k2);
        }
        hw /= (double)K;
        hb /= (double)((int64_t)K * (K - 1) / 2);
        ratio[s] = 1 - hw / hb;
    }
}

// W&C84: one lane per window, Numerator / Denominator over its valid SNPs in ascending order (gnrFst :192-207)
__global__ __launch_bounds__(64) void fst_sum_wc84_kernel(const double *__restrict__ num, const double *__restrict__ den,
                                                          const int64_t *__restrict__ offsets,
                                                          const int32_t *__restrict__ snp_index, int64_t n_win, double *__restrict__ out)
{
    const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (w >= n_win) return;
    // an invalid SNP carries num = den = +0, and x + 0 = x: no branch, so that the loads of several SNPs are in flight while the
    // additions stay in order
    double sn = 0, sd = 0;
#pragma unroll 8
    for (int64_t i = offsets[w]; i < offsets[w + 1]; i++) {
        const int64_t s = snp_index ? snp_index[i] : i;
        sn += num[s];
        sd += den[s];
    }
    out[w] = sn / sd;
}

// W&H02: one lane per (window, k1 <= k2): SumH over the window's valid SNPs, H recomputed from the counters (:219-229)
__global__ __launch_bounds__(64) void fst_sum_wh02_kernel(const int32_t *__restrict__ acnt, const int32_t *__restrict__ cnt,
                                                          const uint8_t *__restrict__ valid, int K, const int64_t *__restrict__ offsets,
                                                          const int32_t *__restrict__ snp_index, int64_t w0, int64_t n_w,
                                                          double *__restrict__ sum_h)
{
    const int64_t n_pair = (int64_t)K * (K + 1) / 2;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= n_w * n_pair) return;
    const int64_t w = t / n_pair;
    int64_t p = t - w * n_pair;
    int k1 = 0;
    while (p >= K - k1) { p -= K - k1; k1++; }
    const int k2 = k1 + (int)p;
    double sh = 0;
#pragma unroll 4
    for (int64_t i = offsets[w0 + w]; i < offsets[w0 + w + 1]; i++) {
        const int64_t s = snp_index ? snp_index[i] : i;
        const double h = wh02_h(acnt + s * K, cnt + s * K, k1, k2);      // NaN / Inf for an invalid SNP: selected away, x + 0 = x
        sh += valid[s] ? h : 0.0;
    }
    sum_h[(w * K + k1) * K + k2] = sh;
}

// WH02_beta on each window's SumH (upper triangle), in place: beta is written over both triangles
__global__ __launch_bounds__(64) void fst_beta_kernel(double *__restrict__ h, int K, int64_t n_w, double *__restrict__ out)
{
    const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (w >= n_w) return;
    double *H = h + w * K * K;
    double hw = 0, hb = 0;
    for (int k1 = 0; k1 < K; k1++) {
        hw += H[k1 * K + k1];
        for (int k2 = k1 + 1; k2 < K; k2++) hb += H[k1 * K + k2];
    }
    hw /= (double)K;
    hb /= (double)((int64_t)K * (K - 1) / 2);
    for (int k1 = 0; k1 < K; k1++)
        for (int k2 = k1; k2 < K; k2++) {
            const double b = 1 - H[k1 * K + k2] / hb;
            H[k1 * K + k2] = b;
            H[k2 * K + k1] = b;
        }
    out[w] = 1 - hw / hb;
}

int launch_fst_terms(hipStream_t st, int method, const int32_t *acnt, const int32_t *cnt, int64_t n_snp, int K, double *num, double *den,
                     double *ratio, uint8_t *valid)
{
    hipLaunchKernelGGL(fst_terms_kernel, dim3((unsigned)((n_snp + 255) / 256)), dim3(256), 0, st, method, acnt, cnt, n_snp, K, num, den,
                       ratio, valid);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_fst_sum_wc84(hipStream_t st, const double *num, const double *den, const int64_t *offsets, const int32_t *snp_index,
                        int64_t n_win, double *out)
{
    hipLaunchKernelGGL(fst_sum_wc84_kernel, dim3((unsigned)((n_win + 63) / 64)), dim3(64), 0, st, num, den, offsets, snp_index, n_win,
                       out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// windows [w0, w0 + n_w): sum_h [n_w][K][K] receives beta, out [n_w] the windows' Fst
int launch_fst_sum_wh02(hipStream_t st, const int32_t *acnt, const int32_t *cnt, const uint8_t *valid, int K, const int64_t *offsets,
                        const int32_t *snp_index, int64_t w0, int64_t n_w, double *sum_h, double *out)
{
    const int64_t n = n_w * ((int64_t)K * (K + 1) / 2);
    hipLaunchKernelGGL(fst_sum_wh02_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, acnt, cnt, valid, K, offsets, snp_index, w0,
                       n_w, sum_h);
    SNPGPU_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(fst_beta_kernel, dim3((unsigned)((n_w + 63) / 64)), dim3(64), 0, st, sum_h, K, n_w, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
