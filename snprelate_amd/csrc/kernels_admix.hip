// Ancestry proportions by EM (include/snpgpu.h section 1s): g_ij ~ Binomial(2, sum_k q_ik f_kj) over the called
// genotypes.  fp64 throughout, correctly rounded divisions and the library logarithm, no atomics: every sum has one owner and a
// fixed order that depends neither on the feeds nor on the internal block (admix_device.h).
//   admix_snp_kernel        thread = SNP, f_j in registers, Q through LDS: the SNP's sums over one segment of samples -- sum_i w1 q_ik,
//                           sum_i w0 q_ik and the SNP's part of L -- in ascending sample order
//   admix_samp_kernel       thread = sample, q_i in registers, F and the genotype words through LDS: a_ik over one segment of SNPs in
//                           ascending SNP order, carried across internal blocks
//   admix_fold_snp_kernel   the segments of a SNP in ascending order, then u, v and F'
//   admix_fold_samp_kernel  the segments of a sample in ascending order, then Q'
//   admix_loglik_kernel     L = the sum of the SNPs' parts: one workgroup, strided partial sums and a fixed tree
// Both owners recompute h1 = sum_k q f and h0 = sum_k q (1 - f) from Q and F, which are small and stay in the caches, instead of
// exchanging n x B operand planes.  Every expression is written with explicit fma() under contract(off), so that the instantiations
// (with / without u and v, every padded K) round alike: a padded population has q = 0 and adds exact zeros.
#include <cmath>

#include "admix_device.h"
#include "snpgpu_internal.h"

namespace snpgpu {

namespace {

constexpr int SNP_CHUNK = 64;       // samples of one step of admix_snp_kernel: one 16-byte load of a row
constexpr int SAMP_CHUNK = 32;      // SNPs of one step of admix_samp_kernel

// h1, h0 and the weights of one genotype; code 3 (missing, or a sample / SNP beyond the data) gives w1 = w0 = 0
template <int KP>
__device__ __forceinline__ void admix_weights(const double (&q)[KP], const double (&f)[KP], const double (&g)[KP], uint32_t code, double &h1,
                                              double &h0, double &w1, double &w0)
{
#pragma clang fp contract(off)
    h1 = 0.0; h0 = 0.0;
#pragma unroll
    for (int k = 0; k < KP; k++) {
        h1 = fma(q[k], f[k], h1);
        h0 = fma(q[k], g[k], h0);
    }
    const bool called = code != 3u;
    w1 = called ? (double)code / h1 : 0.0;
    w0 = called ? (double)(2u - code) / h0 : 0.0;
}

template <int KP, bool UV>
__global__ __launch_bounds__(256) void admix_snp_kernel(AdmixState s, int64_t j0, int64_t j1, double *__restrict__ upart,
                                                        double *__restrict__ vpart, double *__restrict__ lpart)
{
#pragma clang fp contract(off)
    __shared__ double qs[SNP_CHUNK][KP];
    const int tid = (int)threadIdx.x, K = s.K;
    const int64_t j = j0 + (int64_t)blockIdx.x * 256 + tid;
    const int64_t jr = j < j1 ? j : j1 - 1;                     // threads past the block repeat its last SNP and store nothing
    const int64_t seg = blockIdx.y, i0 = seg * ADMIX_SSEG, i1 = i0 + ADMIX_SSEG < s.n ? i0 + ADMIX_SSEG : s.n;
    const uint8_t *__restrict__ row = s.rows + jr * s.rbr;
    double f[KP], g[KP], s1[KP], s0[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) {
        f[k] = k < K ? s.F[jr * K + k] : 0.5;
        g[k] = 1.0 - f[k];
        s1[k] = 0.0; s0[k] = 0.0;
    }
    double L = 0.0;
    for (int64_t ic = i0; ic < i1; ic += SNP_CHUNK) {
        __syncthreads();
        for (int idx = tid; idx < SNP_CHUNK * KP; idx += 256) {
            const int ii = idx / KP, k = idx - ii * KP;
            const int64_t i = ic + ii;
            qs[ii][k] = (i < i1 && k < K) ? s.Q[i * K + k] : 0.0;
        }
        __syncthreads();
        // ic is a multiple of 64 below n: the 16 bytes at ic / 4 lie inside the row's rbr (a multiple of 16) bytes
        const uint4 w4 = *reinterpret_cast<const uint4 *>(row + (ic >> 2));
#pragma unroll 1
        for (int ii = 0; ii < SNP_CHUNK; ii++) {
            const int t = ii >> 4;
            const uint32_t wt = t == 0 ? w4.x : t == 1 ? w4.y : t == 2 ? w4.z : w4.w;
            uint32_t code = (wt >> (2 * (ii & 15))) & 3u;
            if (ic + ii >= i1) code = 3u;
            double q[KP];
#pragma unroll
            for (int k = 0; k < KP; k++) q[k] = qs[ii][k];
            double h1, h0, w1, w0;
            admix_weights<KP>(q, f, g, code, h1, h0, w1, w0);
            if (code != 3u) L = L + fma((double)(2u - code), log(h0), (double)code * log(h1));
            if (UV) {
#pragma unroll
                for (int k = 0; k < KP; k++) {
                    s1[k] = fma(w1, q[k], s1[k]);
                    s0[k] = fma(w0, q[k], s0[k]);
                }
            }
        }
    }
    if (j >= j1) return;
    lpart[seg * s.m + j] = L;
    if (UV) {
        for (int k = 0; k < K && k < KP; k++) {
            upart[(seg * s.m + j) * K + k] = s1[k];
            vpart[(seg * s.m + j) * K + k] = s0[k];
        }
    }
}

template <int KP>
__global__ __launch_bounds__(256) void admix_samp_kernel(AdmixState s, int64_t j0, int64_t j1, double *__restrict__ apart)
{
#pragma clang fp contract(off)
    __shared__ double fs[SAMP_CHUNK][KP][2];
    __shared__ uint32_t gs[SAMP_CHUNK][16];
    const int tid = (int)threadIdx.x, K = s.K;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const int64_t seg = j0 / ADMIX_JSEG + blockIdx.y, seg0 = seg * ADMIX_JSEG;
    const int64_t ja = j0 > seg0 ? j0 : seg0, jb = j1 < seg0 + ADMIX_JSEG ? j1 : seg0 + ADMIX_JSEG;
    const bool live = i < s.n;
    double *__restrict__ mine = apart + (seg * s.n + (live ? i : 0)) * K;
    double q[KP], a[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) {
        q[k] = (live && k < K) ? s.Q[i * K + k] : 0.0;
        a[k] = (live && k < K && ja > seg0) ? mine[k] : 0.0;   // the segment was begun by an earlier internal block
    }
    const int64_t byte0 = (int64_t)blockIdx.x * 64;             // this workgroup's 256 samples of a row
    for (int64_t jc = ja; jc < jb; jc += SAMP_CHUNK) {
        const int nj = (int)(jb - jc < SAMP_CHUNK ? jb - jc : SAMP_CHUNK);
        __syncthreads();
        for (int idx = tid; idx < nj * KP; idx += 256) {
            const int jj = idx / KP, k = idx - jj * KP;
            const double fv = k < K ? s.F[(jc + jj) * K + k] : 0.5;
            fs[jj][k][0] = fv;
            fs[jj][k][1] = 1.0 - fv;
        }
        for (int idx = tid; idx < nj * 16; idx += 256) {
            const int jj = idx >> 4, wd = idx & 15;
            const int64_t off = byte0 + 4 * wd;                 // rbr is a multiple of 16: a word lies inside the row or wholly past it
            gs[jj][wd] = off < s.rbr ? *reinterpret_cast<const uint32_t *>(s.rows + (jc + jj) * s.rbr + off) : 0xFFFFFFFFu;
        }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < nj; jj++) {
            const uint32_t code = live ? (gs[jj][tid >> 4] >> (2 * (tid & 15))) & 3u : 3u;
            double f[KP], g[KP];
#pragma unroll
            for (int k = 0; k < KP; k++) { f[k] = fs[jj][k][0]; g[k] = fs[jj][k][1]; }
            double h1, h0, w1, w0;
            admix_weights<KP>(q, f, g, code, h1, h0, w1, w0);
#pragma unroll
            for (int k = 0; k < KP; k++) a[k] = a[k] + fma(w1, f[k], w0 * g[k]);
        }
    }
    if (!live) return;
    for (int k = 0; k < K && k < KP; k++) mine[k] = a[k];
}

__global__ __launch_bounds__(256) void admix_fold_snp_kernel(AdmixState s, const double *__restrict__ upart, const double *__restrict__ vpart,
                                                             const double *__restrict__ lpart, double f_min, double *__restrict__ Fnew,
                                                             double *__restrict__ lsnp)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= s.m) return;
    const int64_t n_seg = (s.n + ADMIX_SSEG - 1) / ADMIX_SSEG;
    double L = 0.0;
    for (int64_t r = 0; r < n_seg; r++) L = L + lpart[r * s.m + j];
    lsnp[j] = L;
    if (!Fnew) return;
    for (int k = 0; k < s.K; k++) {
        double s1 = 0.0, s0 = 0.0;
        for (int64_t r = 0; r < n_seg; r++) {
            s1 = s1 + upart[(r * s.m + j) * s.K + k];
            s0 = s0 + vpart[(r * s.m + j) * s.K + k];
        }
        const double f = s.F[j * s.K + k];
        const double u = f * s1, v = (1.0 - f) * s0, d = u + v;
        double fn = f;
        if (d > 0.0) {
            fn = u / d;
            fn = fn < f_min ? f_min : fn;
            fn = fn > 1.0 - f_min ? 1.0 - f_min : fn;
        }
        Fnew[j * s.K + k] = fn;
    }
}

__global__ __launch_bounds__(256) void admix_fold_samp_kernel(AdmixState s, const double *__restrict__ apart, double *__restrict__ Qnew)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n) return;
    const int64_t n_seg = (s.m + ADMIX_JSEG - 1) / ADMIX_JSEG;
    const int K = s.K;
    // x_k = q_k a_k is made twice, by the same operations, rather than kept in a dynamically indexed array (scratch)
    auto x_of = [&](int k) {
        double a = 0.0;
        for (int64_t r = 0; r < n_seg; r++) a = a + apart[(r * s.n + i) * K + k];
        return s.Q[i * K + k] * a;
    };
    double sum = 0.0;
    for (int k = 0; k < K; k++) sum = sum + x_of(k);
    // a sample without a called SNP keeps its row
    for (int k = 0; k < K; k++) Qnew[i * K + k] = sum > 0.0 ? x_of(k) / sum : s.Q[i * K + k];
}

__global__ __launch_bounds__(1024) void admix_loglik_kernel(const double *__restrict__ lsnp, int64_t m, double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double red[1024];
    const int tid = (int)threadIdx.x;
    double acc = 0.0;
    for (int64_t j = tid; j < m; j += 1024) acc = acc + lsnp[j];
    red[tid] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    if (tid == 0) *out = red[0];
}

// the instantiation that holds K populations: the next of 2, 3, 4, 6, 8, 12, 16, 24, 32 (the padding adds exact zeros)
template <class Fn> int with_kp(int K, Fn &&fn)
{
    if (K <= 2) return fn(std::integral_constant<int, 2>());
    if (K <= 3) return fn(std::integral_constant<int, 3>());
    if (K <= 4) return fn(std::integral_constant<int, 4>());
    if (K <= 6) return fn(std::integral_constant<int, 6>());
    if (K <= 8) return fn(std::integral_constant<int, 8>());
    if (K <= 12) return fn(std::integral_constant<int, 12>());
    if (K <= 16) return fn(std::integral_constant<int, 16>());
    if (K <= 24) return fn(std::integral_constant<int, 24>());
    return fn(std::integral_constant<int, 32>());
}

}  // namespace

int launch_admix_snp(hipStream_t st, const AdmixState &s, int64_t j0, int64_t j1, bool uv, double *upart, double *vpart, double *lpart)
{
    if (j1 <= j0 || s.n <= 0) return 0;
    const dim3 grid((unsigned)((j1 - j0 + 255) / 256), (unsigned)((s.n + ADMIX_SSEG - 1) / ADMIX_SSEG));
    with_kp(s.K, [&](auto kp) {
        constexpr int KP = decltype(kp)::value;
        if (uv) hipLaunchKernelGGL((admix_snp_kernel<KP, true>), grid, dim3(256), 0, st, s, j0, j1, upart, vpart, lpart);
        else hipLaunchKernelGGL((admix_snp_kernel<KP, false>), grid, dim3(256), 0, st, s, j0, j1, upart, vpart, lpart);
        return 0;
    });
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_admix_samp(hipStream_t st, const AdmixState &s, int64_t j0, int64_t j1, double *apart)
{
    if (j1 <= j0 || s.n <= 0) return 0;
    const int64_t seg_a = j0 / ADMIX_JSEG, seg_b = (j1 - 1) / ADMIX_JSEG;
    const dim3 grid((unsigned)((s.n + 255) / 256), (unsigned)(seg_b - seg_a + 1));
    with_kp(s.K, [&](auto kp) {
        constexpr int KP = decltype(kp)::value;
        hipLaunchKernelGGL((admix_samp_kernel<KP>), grid, dim3(256), 0, st, s, j0, j1, apart);
        return 0;
    });
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_admix_fold_snp(hipStream_t st, const AdmixState &s, const double *upart, const double *vpart, const double *lpart, double f_min,
                          double *Fnew, double *lsnp)
{
    if (s.m <= 0) return 0;
    hipLaunchKernelGGL(admix_fold_snp_kernel, dim3((unsigned)((s.m + 255) / 256)), dim3(256), 0, st, s, upart, vpart, lpart, f_min, Fnew, lsnp);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_admix_fold_samp(hipStream_t st, const AdmixState &s, const double *apart, double *Qnew)
{
    hipLaunchKernelGGL(admix_fold_samp_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, st, s, apart, Qnew);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_admix_loglik(hipStream_t st, const double *lsnp, int64_t m, double *out)
{
    hipLaunchKernelGGL(admix_loglik_kernel, dim3(1), dim3(1024), 0, st, lsnp, m, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
