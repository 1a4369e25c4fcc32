// Quality-control kernels behind snpgdsSampMissRate / snpgdsHWE / snpgdsIndInb:
//   qc_count     one pass over the 2-bit rows -> exact genotype counts per SNP (g = 0, 1, 2) and missing calls per sample
//   qc_freq      allele frequency of a SNP from its counts (calc_afreq's sum / num * 0.5, or GetAlleleFreqs' sum / (2 num))
//   qc_table     per SNP the three values a moment method adds for g = 0, 1, 2 (src/genIBD.cpp:1910-2000), reference order
//   qc_mom       one lane per sample walks the SNPs in ascending order: the reference's sequential fp64 sums, bit for bit
//   qc_words     sample-major 2-bit words of resident rows (as ibd_words_kernel, without its usable-SNP mask)
//   qc_mle       _inb_mle (src/genIBD.cpp:1393-1438): one wave per sample, lanes stride over the SNP words of every sweep
//   qc_hwe       SNPHWE_pValue (src/genHWE.cpp:46-113): one lane per SNP, the recurrence run twice (sum, then p-value)
//
// Rows are read where the caller put them (rb bytes per SNP, any byte address): a lane owns the 16 samples of one 32-bit word
// column of the row and assembles that word from the one or two aligned words that hold it.
#include "snpgpu_internal.h"
#include "prep_device.h"

#include <cmath>

namespace snpgpu {

// every fp64 expression below is written in the reference's order and must not be contracted into FMAs
#pragma clang fp contract(off)

constexpr int QC_CHUNK = 255;     // SNPs per workgroup of the counter kernel: the per-sample byte counters cannot overflow

// bytes [4 j, 4 j + 4) of the row; only aligned words that hold a byte of the row are read, bytes past the row are undefined
__device__ __forceinline__ uint32_t qc_row_word(const uint8_t *row, int64_t rb, int64_t j)
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

// grid.x: 256 word columns (4096 samples) each, grid.y: chunks of QC_CHUNK SNPs.  snp_cnt [n_snp][3] and samp_miss [n_samp] are
// added to with integer atomics (zeroed by the caller), so the result does not depend on the order.  Either may be NULL.
__global__ __launch_bounds__(256) void qc_count_kernel(const uint8_t *__restrict__ geno, int64_t rb, int64_t n_snp, int64_t n_samp,
                                                       int32_t *__restrict__ snp_cnt, int32_t *__restrict__ samp_miss)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_words = (n_samp + 15) / 16;
    const bool live = j < n_words;
    int nv = 0;
    if (live) nv = n_samp - 16 * j < 16 ? (int)(n_samp - 16 * j) : 16;          // samples of this word: the rest is padding
    const uint32_t m55 = nv >= 16 ? GENO_LO_BITS : (GENO_LO_BITS & ((1u << (2 * nv)) - 1u));
    const int64_t s0 = (int64_t)blockIdx.y * QC_CHUNK;
    const int64_t s1 = s0 + QC_CHUNK < n_snp ? s0 + QC_CHUNK : n_snp;
    const int lane = threadIdx.x & 63;
    uint32_t acc[4] = {0, 0, 0, 0};                 // byte t + 4 b of the lane: missing calls of sample 16 j + t + 4 b
    for (int64_t s = s0; s < s1; s++) {
        const uint32_t w = live ? qc_row_word(geno + s * rb, rb, j) : 0u;
        const uint32_t lo = geno_lo(w), hi = geno_hi(w);
        const uint32_t miss = lo & hi & m55;
        if (snp_cnt) {
            const uint32_t zero = ~(lo | hi) & m55, one = lo & ~hi & m55, two = hi & ~lo & m55;
            int c01 = __popc(zero) | (__popc(one) << 16), c2 = __popc(two);     // <= 16 x 64 per field after the wave sum
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                c01 += __shfl_down(c01, off);
                c2 += __shfl_down(c2, off);
            }
            if (lane == 0) {
                if (c01 & 0xFFFF) atomicAdd(snp_cnt + 3 * s, c01 & 0xFFFF);
                if (c01 >> 16) atomicAdd(snp_cnt + 3 * s + 1, c01 >> 16);
                if (c2) atomicAdd(snp_cnt + 3 * s + 2, c2);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] += (miss >> (2 * t)) & 0x01010101u;
    }
    if (samp_miss && live) {
        for (int k = 0; k < nv; k++) {
            const int c = (int)((acc[k & 3] >> (8 * (k >> 2))) & 255u);
            if (c) atomicAdd(samp_miss + 16 * j + k, c);
        }
    }
}

int launch_qc_count(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, int64_t n_samp, int32_t *snp_cnt, int32_t *samp_miss)
{
    if (n_snp <= 0) return 0;
    const int64_t n_words = (n_samp + 15) / 16;
    const dim3 grid((unsigned)((n_words + 255) / 256), (unsigned)((n_snp + QC_CHUNK - 1) / QC_CHUNK));
    hipLaunchKernelGGL(qc_count_kernel, grid, dim3(256), 0, st, geno, rb, n_snp, n_samp, snp_cnt, samp_miss);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// mode 0: calc_afreq (src/genIBD.cpp:1831-1844), sum / num * 0.5; mode 1: GetAlleleFreqs (src/dGenGWAS.cpp:250-302), sum / (2 num).
// No call gives 0 / 0 = NaN in both.
__global__ __launch_bounds__(256) void qc_freq_kernel(const int32_t *__restrict__ cnt, int64_t n_snp, int mode, double *__restrict__ af)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_snp) return;
    const int n0 = cnt[3 * s], n1 = cnt[3 * s + 1], n2 = cnt[3 * s + 2];
    const double sum = (double)(n1 + 2 * (int64_t)n2);
    const int64_t num = (int64_t)n0 + n1 + n2;
    af[s] = mode == 0 ? sum / (double)num * 0.5 : sum / (double)(2 * num);
}

int launch_qc_freq(hipStream_t st, const int32_t *cnt, int64_t n_snp, int mode, double *af)
{
    if (n_snp <= 0) return 0;
    hipLaunchKernelGGL(qc_freq_kernel, dim3((unsigned)((n_snp + 255) / 256)), dim3(256), 0, st, cnt, n_snp, mode, af);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// tab[s] = {value for g = 0, 1, 2, h}; flag[s]: bit g = the value is finite (it is added and counted).  mom.weir adds its
// numerator and h for every called genotype whatever they are, so its flags are not read.
__global__ __launch_bounds__(256) void qc_table_kernel(int method, const double *__restrict__ af, int64_t n_snp, double4 *__restrict__ tab,
                                                       uint8_t *__restrict__ flag)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_snp) return;
    const double p = af[s];
    const double h = 2 * p * (1 - p);
    const double p1 = 1 + 2 * p, p2 = 2 * p * p;
    double v[3];
    unsigned f = 0;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        double x;
        if (method == SNPGPU_INB_GCTA1) {
            const double d = g - 2 * p;
            x = d * d / h - 1;
        } else if (method == SNPGPU_INB_GCTA2) {
            x = 1 - g * (2 - g) / h;
        } else if (method == SNPGPU_INB_MOM_WEIR) {
            x = g * g - g * p1 + p2;
        } else {
            x = (g * g - g * p1 + p2) / h;
        }
        v[g] = x;
        if (isfinite(x)) f |= 1u << g;
    }
    tab[s] = make_double4(v[0], v[1], v[2], h);
    flag[s] = (uint8_t)f;
}

int launch_qc_table(hipStream_t st, int method, const double *af, int64_t n_snp, void *tab, uint8_t *flag)
{
    if (n_snp <= 0) return 0;
    hipLaunchKernelGGL(qc_table_kernel, dim3((unsigned)((n_snp + 255) / 256)), dim3(256), 0, st, method, af, n_snp, (double4 *)tab, flag);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// One lane per sample over the n_snp rows of a block in ascending order; acc / den / cnt carry the sums across blocks.  The SNP
// index is wave-uniform, so the table entries are scalar loads.
template <bool WEIR>
__global__ __launch_bounds__(256) void qc_mom_kernel(const uint8_t *__restrict__ geno, int64_t rb, int64_t n_snp, int64_t n_samp,
                                                     const double4 *__restrict__ tab, const uint8_t *__restrict__ flag,
                                                     double *__restrict__ acc, double *__restrict__ den, int32_t *__restrict__ cnt)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_samp) return;
    const uint8_t *col = geno + (s >> 2);
    const int sh = 2 * (int)(s & 3);
    double a = acc[s], d = WEIR ? den[s] : 0.0;
    int c = WEIR ? 0 : cnt[s];
#pragma unroll 8
    for (int64_t l = 0; l < n_snp; l++) {
        const unsigned g = (col[l * rb] >> sh) & 3u;
        const double4 t = tab[l];
        const double v = g == 0u ? t.x : g == 1u ? t.y : t.z;
        if (WEIR) {
            if (g < 3u) { a += v; d += t.w; }
        } else {
            const bool ok = g < 3u && ((flag[l] >> g) & 1u);
            a = ok ? a + v : a;
            c += ok ? 1 : 0;
        }
    }
    acc[s] = a;
    if (WEIR) den[s] = d; else cnt[s] = c;
}

int launch_qc_mom(hipStream_t st, int weir, const uint8_t *geno, int64_t rb, int64_t n_snp, int64_t n_samp, const void *tab,
                  const uint8_t *flag, double *acc, double *den, int32_t *cnt)
{
    if (n_snp <= 0) return 0;
    const dim3 grid((unsigned)((n_samp + 255) / 256));
    if (weir)
        hipLaunchKernelGGL(qc_mom_kernel<true>, grid, dim3(256), 0, st, geno, rb, n_snp, n_samp, (const double4 *)tab, flag, acc, den, cnt);
    else
        hipLaunchKernelGGL(qc_mom_kernel<false>, grid, dim3(256), 0, st, geno, rb, n_snp, n_samp, (const double4 *)tab, flag, acc, den, cnt);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// vec_f64_div (src/dVect.cpp:460-469): by the int count, or for mom.weir by the fp64 denominator
__global__ __launch_bounds__(256) void qc_mom_final_kernel(int weir, int64_t n_samp, const double *__restrict__ acc,
                                                           const double *__restrict__ den, const int32_t *__restrict__ cnt,
                                                           double *__restrict__ out)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_samp) return;
    out[s] = weir ? acc[s] / den[s] : acc[s] / (double)cnt[s];
}

int launch_qc_mom_final(hipStream_t st, int weir, int64_t n_samp, const double *acc, const double *den, const int32_t *cnt, double *out)
{
    hipLaunchKernelGGL(qc_mom_final_kernel, dim3((unsigned)((n_samp + 255) / 256)), dim3(256), 0, st, weir, n_samp, acc, den, cnt, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// word w0 + blockIdx.y of sample s: SNPs 16 w .. 16 w + 15 of the block's rows at bits 2 m; SNPs past the block's end are 3
__global__ __launch_bounds__(256) void qc_words_kernel(const uint8_t *__restrict__ rows, int64_t rb, int64_t n_snp, int64_t n_samp,
                                                       int64_t w0, int64_t nw, uint32_t *__restrict__ gt)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (s >= n_samp) return;
    uint32_t v = 0;
    for (int m = 0; m < 16; m++) {
        const int64_t l = 16 * w + m;
        unsigned code = 3u;
        if (l < n_snp) code = (rows[l * rb + (s >> 2)] >> (2 * (s & 3))) & 3u;
        v |= code << (2 * m);
    }
    gt[s * nw + w0 + w] = v;
}

// rows: n_snp rows of a block that starts at SNP 16 w0 of the data set; gt: [n_samp][nw]
int launch_qc_words(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, int64_t n_samp, int64_t w0, int64_t nw, uint32_t *gt)
{
    if (n_snp <= 0) return 0;
    const dim3 grid((unsigned)((n_samp + 255) / 256), (unsigned)((n_snp + 15) / 16));
    hipLaunchKernelGGL(qc_words_kernel, grid, dim3(256), 0, st, rows, rb, n_snp, n_samp, w0, nw, gt);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

__device__ __forceinline__ double qc_wave_sum(double v)
{
    // butterfly: both lanes of a pair add the same two numbers, so every lane ends with the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int qc_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

constexpr int QC_MLE_MAX_ITER = 10000;
constexpr double QC_LN2 = 0.69314718055994530942;

// One wave (= one workgroup) per sample.  Sweep k evaluates, at F_k, both the log-likelihood L_k and the update sum that gives F_{k + 1}; the
// reference's iteration `iter` stops on |L_iter - L_{iter - 1}| <= contol and returns F_iter, so sweep k decides iteration k.
// The log-likelihood is a product of the terms' mantissas with their exponents summed as integers, one log per lane and sweep.
// af: [16 nw] (entries past n_snp are never used: their codes are 3).  stats: [0] lane-steps that held a word, [1] issued: their
// ratio is the fill of the last 64-word stride, nw / round_up(nw, 64) -- geometry, not a measurement; no wave waits for another.
__global__ __launch_bounds__(64) void qc_mle_kernel(const uint32_t *__restrict__ gt, int64_t nw, const double *__restrict__ af,
                                                     int64_t n_samp, double reltol, double *__restrict__ out_f,
                                                     int32_t *__restrict__ out_niter, unsigned long long *__restrict__ stats)
{
    const int lane = threadIdx.x;
    const int64_t s = blockIdx.x;                              // a workgroup is one wave: it retires when its sample stops
    const uint32_t *g = gt + s * nw;

    // start value: _inb_mom_ratio (:1354-1370), every called SNP whatever its frequency
    double num = 0, den = 0;
    for (int64_t w = lane; w < nw; w += 64) {
        const uint32_t word = g[w];
#pragma unroll 4
        for (int m = 0; m < 16; m++) {
            const int code = (int)((word >> (2 * m)) & 3u);
            const double p = af[16 * w + m];
            const double a = code * code - (1 + 2 * p) * code + 2 * p * p, b = 2 * p * (1 - p);
            if (code < 3) { num += a; den += b; }
        }
    }
    num = qc_wave_sum(num);
    den = qc_wave_sum(den);
    double F = num / den;
    int niter = -1;
    unsigned long long sweeps = 0;
    if (isfinite(F)) {
        if (F < 0.001) F = 0.001;
        if (F > 1 - 0.001) F = 1 - 0.001;
        double old = 0, contol = 0;
        for (int k = 0;; k++) {
            const double omF = 1 - F;
            double sum = 0, prod = 1;
            int cnt = 0, ex = 0;
            for (int64_t w = lane; w < nw; w += 64) {
                const uint32_t word = g[w];
#pragma unroll 4
                for (int m = 0; m < 16; m++) {
                    const unsigned code = (word >> (2 * m)) & 3u;
                    const double p = af[16 * w + m], q = 1 - p;
                    const bool het = code == 1u, hom = (code & 1u) == 0u;        // code 3: neither
                    const double x = code == 0u ? q : p;
                    const double tmp = F / (F + x * omF);
                    const bool ok = hom && isfinite(tmp);
                    sum = ok ? sum + tmp : sum;
                    cnt += (ok || het) ? 1 : 0;
                    const double arg = het ? omF * 2 * p * q : omF * x * x + F * x;
                    const bool use = (hom || het) && arg > 0 && arg < INFINITY;  // log(arg) is finite
                    int e1;
                    const double mant = frexp(arg, &e1);
                    prod *= use ? mant : 1.0;
                    ex += use ? e1 : 0;
                }
                int e;
                prod = frexp(prod, &e);
                ex += e;
            }
            sweeps++;
            const double L = qc_wave_sum(log(prod) + ex * QC_LN2);
            sum = qc_wave_sum(sum);
            cnt = qc_wave_sum(cnt);
            if (k == 0) {
                contol = fabs(L) * reltol;
            } else {
                if (fabs(L - old) <= contol) { niter = k; break; }
                if (k == QC_MLE_MAX_ITER) { niter = QC_MLE_MAX_ITER + 1; break; }
            }
            old = L;
            F = sum / cnt;
        }
    }
    if (lane == 0) {
        out_f[s] = F;
        if (out_niter) out_niter[s] = niter;
        if (stats) {
            atomicAdd(stats, sweeps * (unsigned long long)nw);
            atomicAdd(stats + 1, sweeps * (unsigned long long)((nw + 63) / 64 * 64));
        }
    }
}

int launch_qc_mle(hipStream_t st, const uint32_t *gt, int64_t nw, const double *af, int64_t n_samp, double reltol, double *out_f,
                  int32_t *out_niter, unsigned long long *stats)
{
    hipLaunchKernelGGL(qc_mle_kernel, dim3((unsigned)n_samp), dim3(64), 0, st, gt, nw, af, n_samp, reltol, out_f, out_niter,
                       stats);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// One lane per SNP; lane i takes SNP perm[i] (the host sorts the SNPs by the number of rare-allele copies, so the lanes of a
// wave run loops of nearly the same length).  The recurrence from the midpoint down and then up gives the unnormalised terms and
// their sum in the reference's order; it is then run again (the same operations: the same bits) for the p-value, which adds
// term / sum over the terms not greater than the observed one in that generation order.  The products rare x (2 n - rare) are
// taken in 64 bits (the reference's int overflows beyond 32 767 samples).
__global__ __launch_bounds__(64) void qc_hwe_kernel(const int32_t *__restrict__ cnt, const int32_t *__restrict__ perm, int64_t n_snp,
                                                    double *__restrict__ pv)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_snp) return;
    const int64_t s = perm ? perm[i] : i;
    const int64_t hom2 = cnt[3 * s], het = cnt[3 * s + 1], hom1 = cnt[3 * s + 2];
    const int64_t homc = hom1 < hom2 ? hom2 : hom1, homr = hom1 < hom2 ? hom1 : hom2;
    const int64_t rare = 2 * homr + het, gen = het + homc + homr;
    if (gen <= 0) { pv[s] = __builtin_nan(""); return; }
    int64_t mid = rare * (2 * gen - rare) / (2 * gen);
    if ((rare & 1) ^ (mid & 1)) mid++;
    const double r0 = (double)((rare - mid) / 2), c0 = (double)(gen - mid - (rare - mid) / 2);

    double sum = 1.0, tobs = mid == het ? 1.0 : 0.0;
    {
        double t = 1.0, r = r0, c = c0;
        for (int64_t h = mid; h > 1; h -= 2) {
            const double dh = (double)h;
            t = t * dh * (dh - 1.0) / (4.0 * (r + 1.0) * (c + 1.0));
            sum += t;
            if (h - 2 == het) tobs = t;
            r += 1.0; c += 1.0;
        }
        t = 1.0; r = r0; c = c0;
        for (int64_t h = mid; h <= rare - 2; h += 2) {
            const double dh = (double)h;
            t = t * 4.0 * r * c / ((dh + 2.0) * (dh + 1.0));
            sum += t;
            if (h + 2 == het) tobs = t;
            r -= 1.0; c -= 1.0;
        }
    }
    const double qobs = tobs / sum;
    double p = 0.0;
    {
        double t = 1.0, r = r0, c = c0;
        double q = t / sum;
        p += q > qobs ? 0.0 : q;
        for (int64_t h = mid; h > 1; h -= 2) {
            const double dh = (double)h;
            t = t * dh * (dh - 1.0) / (4.0 * (r + 1.0) * (c + 1.0));
            q = t / sum;
            p += q > qobs ? 0.0 : q;
            r += 1.0; c += 1.0;
        }
        t = 1.0; r = r0; c = c0;
        for (int64_t h = mid; h <= rare - 2; h += 2) {
            const double dh = (double)h;
            t = t * 4.0 * r * c / ((dh + 2.0) * (dh + 1.0));
            q = t / sum;
            p += q > qobs ? 0.0 : q;
            r -= 1.0; c -= 1.0;
        }
    }
    pv[s] = p > 1.0 ? 1.0 : p;
}

int launch_qc_hwe(hipStream_t st, const int32_t *cnt, const int32_t *perm, int64_t n_snp, double *pv)
{
    if (n_snp <= 0) return 0;
    hipLaunchKernelGGL(qc_hwe_kernel, dim3((unsigned)((n_snp + 63) / 64)), dim3(64), 0, st, cnt, perm, n_snp, pv);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
