// LD scores (snpgdsLDScore, csrc/ld_score.hip): score[i] = sum over the window partners j of i of the squared LD value of the
// pair, from the band tables [n_i][W][9] of one launch of rows i0 ... i0 + n_i - 1 (kernels_ld.hip, ld_band.h).
//
// Two kernels per launch.  ld_score_terms_kernel evaluates every pair (i, i + k) of the band inside the window ONCE (for r /
// dprime that is one EM per pair) and writes its term t, NaN when the pair is not valid or not in the window.  ld_score_fold_kernel
// then has one thread per SNP j of [i0, i0 + n_i + W): it continues j's running sum with the launch's rows i < j inside j's
// window in ascending i (pair (i, j), read at row i, distance j - i), and, when j is itself a row of the launch, with its own
// partners j + 1 ... hi[j].  Launches are stream-ordered in ascending i0, so every score is ONE left fold over its partners in
// ascending order whatever the block partition: bit-identical to a plain fp64 loop, without atomics.
//
// Layout of the terms: distance-major, vals[(k - 1) n_i + (i - i0)].  A fold thread walks the distance; its neighbour j + 1 reads
// the neighbouring row at the same distance in both directions, so every fold load of a wave is one run of consecutive doubles.
// The price is paid by the terms kernel, whose tables are row-major: it works in 16 x 16 (row, distance) tiles and turns each
// through LDS, so that table reads are runs of 16 tables and term writes runs of 16 doubles (one 128-byte line).
#include "snpgpu_internal.h"
#include "ld_device.h"

#include <algorithm>

namespace snpgpu {

namespace {

constexpr int LS_TILE = 16;       // rows and distances per workgroup of the terms kernel
constexpr int LS_UNROLL = 8;      // loads a fold thread has in flight ahead of its (sequential) adds
constexpr int LS_SLOTS = LD_SCORE_COUNT_SLOTS;
static_assert((LS_SLOTS & (LS_SLOTS - 1)) == 0, "the slot of a workgroup is its index modulo a power of two");

__global__ void ld_score_init_kernel(double *__restrict__ acc, int32_t *__restrict__ nv, int64_t n, double self)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    acc[t] = self;
    nv[t] = 0;
}

// hi[i]: the last window partner of SNP i (chromosome index, i itself when it has none above it); n_valid: LS_SLOTS counters whose
// sum grows by the number of valid pairs
__global__ __launch_bounds__(LS_TILE *LS_TILE) void ld_score_terms_kernel(const int32_t *__restrict__ tab, int64_t n_i, int w, int64_t i0,
                                                                          const int32_t *__restrict__ hi, int method, int adjust,
                                                                          double *__restrict__ vals,
                                                                          unsigned long long *__restrict__ n_valid)
{
#pragma clang fp contract(off)
    __shared__ double tile[LS_TILE][LS_TILE + 1];
    const int64_t tiles_k = (w + LS_TILE - 1) / LS_TILE;
    const int64_t r0 = (int64_t)blockIdx.x / tiles_k * LS_TILE;
    const int k0 = (int)((int64_t)blockIdx.x % tiles_k) * LS_TILE;       // distance - 1 of the tile's first column
    const int tx = threadIdx.x & (LS_TILE - 1), ty = threadIdx.x >> 4;
    {
        const int64_t r = r0 + ty;
        const int k = k0 + tx;                                             // distance - 1
        double t = __builtin_nan("");
        if (r < n_i && k < w && i0 + r + k + 1 <= hi[i0 + r]) {
            const int32_t *c = tab + (r * w + k) * 9;
            long n[9];
            long tot = 0;
#pragma unroll
            for (int q = 0; q < 9; q++) { n[q] = c[q]; tot += n[q]; }
            const double v = ld_value(method, n);
            if (v == v && (!adjust || tot > 2)) {
                t = v * v;
                if (adjust) t = t - (1 - t) / (double)(tot - 2);
            }
        }
        tile[ty][tx] = t;
        // the barrier of the tile is also the workgroup's count of valid pairs: one atomic per workgroup, spread over LS_SLOTS
        // counters (a single address would serialise a quarter of a million atomics per launch)
        const int valid = __syncthreads_count(t == t);
        if (threadIdx.x == 0 && valid) atomicAdd(n_valid + (blockIdx.x & (LS_SLOTS - 1)), (unsigned long long)valid);
    }
    const int64_t r = r0 + tx;
    const int k = k0 + ty;
    if (r < n_i && k < w) vals[(int64_t)k * n_i + r] = tile[tx][ty];
}

// lo[j] / hi[j]: the first / last window partner of SNP j.  acc / nv: the running sum and valid count of every SNP.
__global__ __launch_bounds__(256) void ld_score_fold_kernel(const double *__restrict__ vals, int64_t n_i, int w, int64_t i0, int64_t n_snp,
                                                            const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,
                                                            double *__restrict__ acc, int32_t *__restrict__ nv)
{
#pragma clang fp contract(off)
    const int64_t j = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row_end = i0 + n_i;
    if (j >= n_snp || j >= row_end + w) return;
    double a = acc[j];
    int32_t c = nv[j];
    const double NaN = __builtin_nan("");
    // Both loops run over the whole band in step across the wave (that is what makes the loads consecutive); a lane outside its
    // own range loads element 0 and drops it -- a select, not a branch around the load, so the LS_UNROLL loads issue together.
    {
        // rows i < j of this launch inside j's window, ascending i: distance d = j - i descending
        const int64_t ib = lo[j] > i0 ? (int64_t)lo[j] : i0, ie = j - 1 < row_end - 1 ? j - 1 : row_end - 1;
        const int64_t d_hi = j - ib, d_lo = j - ie;
        for (int64_t d0 = w; d0 >= 1; d0 -= LS_UNROLL) {
            double v[LS_UNROLL];
#pragma unroll
            for (int u = 0; u < LS_UNROLL; u++) {
                const int64_t d = d0 - u;
                const bool ok = d >= d_lo && d <= d_hi;
                const double x = vals[ok ? (d - 1) * n_i + (j - d - i0) : 0];
                v[u] = ok ? x : NaN;
            }
#pragma unroll
            for (int u = 0; u < LS_UNROLL; u++)
                if (v[u] == v[u]) { a += v[u]; c++; }
        }
    }
    if (j < row_end) {
        // j's own partners j + k, ascending
        const int64_t k_hi = hi[j] - j, col = j - i0;
        for (int64_t k0 = 1; k0 <= w; k0 += LS_UNROLL) {
            double v[LS_UNROLL];
#pragma unroll
            for (int u = 0; u < LS_UNROLL; u++) {
                const int64_t k = k0 + u;
                const bool ok = k <= k_hi;
                const double x = vals[ok ? (k - 1) * n_i + col : 0];
                v[u] = ok ? x : NaN;
            }
#pragma unroll
            for (int u = 0; u < LS_UNROLL; u++)
                if (v[u] == v[u]) { a += v[u]; c++; }
        }
    }
    acc[j] = a;
    nv[j] = c;
}

}  // namespace

int launch_ld_score_init(hipStream_t st, double *acc, int32_t *nv, int64_t n, double self)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ld_score_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc, nv, n, self);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_score_terms(hipStream_t st, const int32_t *tab, int64_t n_i, int w, int64_t i0, const int32_t *hi, int method, int adjust,
                          double *vals, uint64_t *n_valid)
{
    if (n_i <= 0 || w <= 0) return 0;
    const int64_t blocks = ((n_i + LS_TILE - 1) / LS_TILE) * (((int64_t)w + LS_TILE - 1) / LS_TILE);
    if (blocks > 0x7fffffffLL) { set_error("ld_score: too many pairs in one table launch"); return 1; }
    hipLaunchKernelGGL(ld_score_terms_kernel, dim3((unsigned)blocks), dim3(LS_TILE * LS_TILE), 0, st, tab, n_i, w, i0, hi, method, adjust,
                       vals, (unsigned long long *)n_valid);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ld_score_fold(hipStream_t st, const double *vals, int64_t n_i, int w, int64_t i0, int64_t n_snp, const int32_t *lo,
                         const int32_t *hi, double *acc, int32_t *nv)
{
    const int64_t n = std::min(n_snp, i0 + n_i + w) - i0;
    if (n_i <= 0 || w <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(ld_score_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, vals, n_i, w, i0, n_snp, lo, hi, acc, nv);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
