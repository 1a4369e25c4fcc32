// Kernels of the permutation test of snpgdsCutTree (gnrDistPerm, src/SNPRelate.cpp:502-677); host side: tree.hip, design:
// DESIGN.md 18.
//
//   P      double [n][n]   the dissimilarity matrix with rows and columns in LEAF ORDER (first column of every merge to the left):
//                          the members of merge m are the rows / columns [start, start + n1 + n2), first n1 then n2 of them
//   R      double [sum N]  per merge m and member x (relative to start): the sum of row start + x of P over the merge's columns
//   Inc    double [sum n1] per merge m and member x < n1: the sum of that row over the columns of the SECOND child (-> obs)
//   d      double [n_perm][n - 1]  the value of every permutation of every merge
//
// A permutation of merge m draws S = the first NSub1 slots of the reference's partial shuffle and needs the mean of D[i][j] over
// i in S, j in the merge but not in S.  That sum is  sum_{i in S} R(i) - sum_{i, j in S} D[i][j]  (exact for a non-symmetric matrix
// too): NSub1^2 gathers instead of NSub1 x NSub2.  Every sum below has an order that depends on the tree alone (lane-strided
// partial sums, then a butterfly over the 64 lanes), so a result does not depend on the launch geometry.
#include "snpgpu_internal.h"

namespace snpgpu {

struct TreeMerge {            // 32 bytes, tree.hip builds them
    int32_t start, n1, n2, parent;      // parent: the merge this one is a child of, -1 for the root
    int64_t roff, ioff;                 // offsets into R and Inc
};

namespace {

constexpr int TREE_THREADS = 256, TREE_WAVES = TREE_THREADS / 64;

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o));
    return v;
}

// Philox4x32-10 (Salmon et al. 2011), key = the call's seed, counter (draw >> 2, permutation, merge, 0); returns word draw & 3
__device__ __forceinline__ void philox_block(uint2 key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t out[4])
{
    uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = 0, k0 = key.x, k1 = key.y;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = __umulhi(0xD2511F53u, x0), l0 = 0xD2511F53u * x0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, x2), l1 = 0xCD9E8D57u * x2;
        const uint32_t y0 = h1 ^ x1 ^ k0, y2 = h0 ^ x3 ^ k1;
        x0 = y0; x1 = l1; x2 = y2; x3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}

// the reference's _RandomNum(Range) on u = (x + 0.5) 2^-32: (int)(u (Range - 1) + 0.5), product and sum rounded separately
__device__ __forceinline__ int draw_step(uint32_t x, int range)
{
    const double u = __dmul_rn(__dadd_rn((double)x, 0.5), 0x1p-32);
    const int rv = (int)__dadd_rn(__dmul_rn(u, (double)(range - 1)), 0.5);
    return rv >= range ? range - 1 : rv;
}

// the offset by which a permutation rotates the member order before its shuffle: floor(u N) from word 0 of the block with
// counter (2^32 - 1, permutation, merge, 0), which no draw of the shuffle uses
__device__ __forceinline__ int draw_rotation(uint2 key, int p, int m, int N)
{
    uint32_t w[4];
    philox_block(key, 0xFFFFFFFFu, (uint32_t)p, (uint32_t)m, w);
    const int c = (int)__dmul_rn(__dmul_rn(__dadd_rn((double)w[0], 0.5), 0x1p-32), (double)N);
    return c >= N ? N - 1 : c;
}

// P[inv[r]][b] = src[r - r0][leaf[b]] for the caller's rows [r0, r0 + rows)
__global__ __launch_bounds__(TREE_THREADS) void tree_gather_kernel(const double *__restrict__ src, int64_t r0, int64_t rows, int64_t n,
                                                                   const int32_t *__restrict__ leaf, const int32_t *__restrict__ inv,
                                                                   double *__restrict__ P)
{
    const int64_t idx = (int64_t)blockIdx.x * TREE_THREADS + threadIdx.x;
    if (idx >= rows * n) return;
    const int64_t r = idx / n, b = idx - r * n;
    P[(int64_t)inv[r0 + r] * n + b] = src[r * n + leaf[b]];
}

// One wave per row a of P: the row is its diagonal entry and, for every ancestor merge of leaf a, the columns of the sibling --
// walking up adds one segment per merge: R of that merge, and Inc where the leaf is in the first child.
__global__ __launch_bounds__(TREE_THREADS) void tree_rows_kernel(const double *__restrict__ P, int64_t n, const TreeMerge *__restrict__ mg,
                                                                 const int32_t *__restrict__ leaf_parent, double *__restrict__ R,
                                                                 double *__restrict__ Inc)
{
    const int lane = threadIdx.x & 63;
    const int64_t a = (int64_t)blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (a >= n) return;
    const double *row = P + a * n;
    double r = row[a];
    for (int m = leaf_parent[a]; m >= 0;) {
        const TreeMerge t = mg[m];
        const int x = (int)a - t.start;
        const int lo = x < t.n1 ? t.start + t.n1 : t.start, len = x < t.n1 ? t.n2 : t.n1;
        double s = 0.0;
        for (int j = lane; j < len; j += 64) s = __dadd_rn(s, row[lo + j]);
        s = wave_sum(s);
        r = __dadd_rn(r, s);
        if (lane == 0) {
            R[t.roff + x] = r;
            if (x < t.n1) Inc[t.ioff + x] = s;
        }
        m = t.parent;
    }
}

// obs[m] = sum of Inc over the first child / (n1 n2): one wave per merge
__global__ __launch_bounds__(TREE_THREADS) void tree_obs_kernel(const TreeMerge *__restrict__ mg, int64_t n_merge, const double *__restrict__ Inc,
                                                                double *__restrict__ obs)
{
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (m >= n_merge) return;
    const TreeMerge t = mg[m];
    double s = 0.0;
    for (int j = lane; j < t.n1; j += 64) s = __dadd_rn(s, Inc[t.ioff + j]);
    s = wave_sum(s);
    if (lane == 0) obs[m] = s / ((double)t.n1 * (double)t.n2);
}

// merges with NSub1 = 1: the drawn member is slot k of the first draw, rotated; one lane per (merge of the list, permutation)
__global__ __launch_bounds__(TREE_THREADS) void tree_perm_light_kernel(const double *__restrict__ P, int64_t n, const TreeMerge *__restrict__ mg,
                                                                       const double *__restrict__ R, const int32_t *__restrict__ list,
                                                                       int64_t n_list, int n_perm, uint2 key, double *__restrict__ d,
                                                                       int64_t n_merge)
{
    const int64_t idx = (int64_t)blockIdx.x * TREE_THREADS + threadIdx.x;
    if (idx >= n_list * n_perm) return;
    const int64_t li = idx / n_perm;
    const int p = (int)(idx - li * n_perm), m = list[li];
    const TreeMerge t = mg[m];
    const int N = t.n1 + t.n2;
    uint32_t w[4];
    philox_block(key, 0u, (uint32_t)p, (uint32_t)m, w);
    int xs = draw_step(w[0], N) + draw_rotation(key, p, m, N);
    if (xs >= N) xs -= N;
    const int64_t x = xs, g = t.start + x;
    d[(int64_t)p * n_merge + m] = __dadd_rn(R[t.roff + x], -P[g * n + g]) / (double)(N - 1);
}

__global__ __launch_bounds__(TREE_THREADS) void tree_iota_kernel(int32_t *arr, int64_t stride, int64_t n_arr)
{
    const int64_t idx = (int64_t)blockIdx.x * TREE_THREADS + threadIdx.x;
    if (idx < stride * n_arr) arr[idx] = (int32_t)(idx % stride);
}

// One wave per permutation.  items[k] = {merge, first permutation, end permutation, 0}; a wave takes the items wave, wave + W, ...
// Its arrangement (stride ints of `scratch`, the identity between permutations) is shuffled by lane 0 as the reference does it,
// read by all lanes -- slot value x stands for member (x + c) mod N, c the permutation's rotation -- and put back by all lanes from
// the same draws.
__global__ __launch_bounds__(TREE_THREADS) void tree_perm_kernel(const double *__restrict__ P, int64_t n, const TreeMerge *__restrict__ mg,
                                                                 const double *__restrict__ R, const int4 *__restrict__ items, int64_t n_items,
                                                                 uint2 key, int32_t *__restrict__ scratch, int64_t stride,
                                                                 double *__restrict__ d, int64_t n_merge)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * TREE_WAVES + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * TREE_WAVES;
    int32_t *arr = scratch + wave * stride;
    for (int64_t it = wave; it < n_items; it += n_waves) {
        const int4 item = items[it];
        const int m = item.x;
        const TreeMerge t = mg[m];
        const int N = t.n1 + t.n2, ns1 = t.n1 < t.n2 ? t.n1 : t.n2;
        const double *Rm = R + t.roff, *Pm = P + (int64_t)t.start * n + t.start;
        const double denom = (double)ns1 * (double)(N - ns1);
        for (int p = item.y; p < item.z; p++) {
            if (lane == 0) {
                uint32_t w[4];
                for (int i = 0; i < ns1; i++) {
                    if ((i & 3) == 0) philox_block(key, (uint32_t)(i >> 2), (uint32_t)p, (uint32_t)m, w);
                    const int j = i + draw_step(w[i & 3], N - i);
                    const int32_t vi = arr[i], vj = arr[j];
                    arr[i] = vj; arr[j] = vi;
                }
            }
            __threadfence_block();
            const int c = draw_rotation(key, p, m, N);
            auto member = [&](int slot) { const int x = arr[slot] + c; return x >= N ? x - N : x; };
            double sr = 0.0, ss = 0.0;
            for (int i = lane; i < ns1; i += 64) sr = __dadd_rn(sr, Rm[member(i)]);
            if (ns1 < 64) {
                for (int q = lane; q < ns1 * ns1; q += 64) {
                    const int i = q / ns1, j = q - i * ns1;
                    ss = __dadd_rn(ss, Pm[(int64_t)member(i) * n + member(j)]);
                }
            } else {
                for (int i = 0; i < ns1; i++) {
                    const double *row = Pm + (int64_t)member(i) * n;
                    for (int j = lane; j < ns1; j += 64) ss = __dadd_rn(ss, row[member(j)]);
                }
            }
            sr = wave_sum(sr);
            ss = wave_sum(ss);
            if (lane == 0) d[(int64_t)p * n_merge + m] = __dadd_rn(sr, -ss) / denom;
            __threadfence_block();                      // every read of the arrangement is done
            for (int i = lane; i < ns1; i += 64) {
                uint32_t w[4];
                philox_block(key, (uint32_t)(i >> 2), (uint32_t)p, (uint32_t)m, w);
                const int j = i + draw_step(w[i & 3], N - i);
                arr[i] = i; arr[j] = j;
            }
            __threadfence_block();
        }
    }
}

// per merge: mean and variance over the n_perm values in index order (two passes, the reference's operations), then z
__global__ __launch_bounds__(TREE_THREADS) void tree_stats_kernel(const TreeMerge *__restrict__ mg, int64_t n_merge, const double *__restrict__ d,
                                                                  int n_perm, const double *__restrict__ obs, double *__restrict__ z,
                                                                  double *__restrict__ mean_out, double *__restrict__ sd_out)
{
    const int64_t m = (int64_t)blockIdx.x * TREE_THREADS + threadIdx.x;
    if (m >= n_merge) return;
    const TreeMerge t = mg[m];
    if (t.n1 <= 1 && t.n2 <= 1) {
        z[m] = 0.0; mean_out[m] = __builtin_nan(""); sd_out[m] = __builtin_nan("");
        return;
    }
    double mean = 0.0;
    for (int p = 0; p < n_perm; p++) mean = __dadd_rn(mean, d[(int64_t)p * n_merge + m]);
    mean /= (double)n_perm;
    double var = 0.0;
    for (int p = 0; p < n_perm; p++) {
        const double e = __dadd_rn(d[(int64_t)p * n_merge + m], -mean);
        var = __dadd_rn(var, __dmul_rn(e, e));
    }
    var /= (double)(n_perm - 1);
    const double sd = sqrt(var);
    z[m] = (var > 0.0) ? __dadd_rn(obs[m], -mean) / sd : 0.0;
    mean_out[m] = mean; sd_out[m] = sd;
}

inline unsigned blocks_for(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

int launch_tree_gather(hipStream_t st, const double *src, int64_t r0, int64_t rows, int64_t n, const int32_t *leaf, const int32_t *inv, double *P)
{
    hipLaunchKernelGGL(tree_gather_kernel, dim3(blocks_for(rows * n, TREE_THREADS)), dim3(TREE_THREADS), 0, st, src, r0, rows, n, leaf, inv, P);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_tree_rows(hipStream_t st, const double *P, int64_t n, const TreeMerge *mg, const int32_t *leaf_parent, double *R, double *Inc,
                     double *obs)
{
    hipLaunchKernelGGL(tree_rows_kernel, dim3(blocks_for(n, TREE_WAVES)), dim3(TREE_THREADS), 0, st, P, n, mg, leaf_parent, R, Inc);
    SNPGPU_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tree_obs_kernel, dim3(blocks_for(n - 1, TREE_WAVES)), dim3(TREE_THREADS), 0, st, mg, n - 1, Inc, obs);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_tree_perm_light(hipStream_t st, const double *P, int64_t n, const TreeMerge *mg, const double *R, const int32_t *list,
                           int64_t n_list, int n_perm, uint64_t seed, double *d)
{
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    hipLaunchKernelGGL(tree_perm_light_kernel, dim3(blocks_for(n_list * n_perm, TREE_THREADS)), dim3(TREE_THREADS), 0, st, P, n, mg, R, list,
                       n_list, n_perm, key, d, n - 1);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_tree_iota(hipStream_t st, int32_t *arr, int64_t stride, int64_t n_arr)
{
    hipLaunchKernelGGL(tree_iota_kernel, dim3(blocks_for(stride * n_arr, TREE_THREADS)), dim3(TREE_THREADS), 0, st, arr, stride, n_arr);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// n_blocks workgroups of TREE_WAVES waves; scratch holds n_blocks * TREE_WAVES arrangements of `stride` ints
int launch_tree_perm(hipStream_t st, int n_blocks, const double *P, int64_t n, const TreeMerge *mg, const double *R, const int4 *items,
                     int64_t n_items, uint64_t seed, int32_t *scratch, int64_t stride, double *d)
{
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    hipLaunchKernelGGL(tree_perm_kernel, dim3(n_blocks), dim3(TREE_THREADS), 0, st, P, n, mg, R, items, n_items, key, scratch, stride, d, n - 1);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_tree_stats(hipStream_t st, const TreeMerge *mg, int64_t n_merge, const double *d, int n_perm, const double *obs, double *z,
                      double *mean, double *sd)
{
    hipLaunchKernelGGL(tree_stats_kernel, dim3(blocks_for(n_merge, TREE_THREADS)), dim3(TREE_THREADS), 0, st, mg, n_merge, d, n_perm, obs, z,
                       mean, sd);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
