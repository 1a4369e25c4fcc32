// Finalisers: rectangular panel accumulators -> the reference's output layouts
// (packed upper triangle slab, CdMatTri src/dGenGWAS.h:511-583, or the full symmetric matrix that
// gnrIBSNum / gnrIBSAve / grm_output build, src/genIBS.cpp:463-543, src/genPCA.cpp:1586-1602).
#include "fin_values.h"

#include <math.h>

namespace snpgpu {

struct OutPos {
    int64_t a, b;  // primary index and mirror index (-1 = none)
};

__device__ __forceinline__ int64_t tri_idx(int64_t N, int64_t i, int64_t j) { return j + i * (2 * N - i - 1) / 2; }

// grid: (ceil((N-col0)/256), groups of FIN_ROWS panel rows); F::apply(rel, relf, i, j, pos): element offsets in the uint32 / fp64 planes.
// A workgroup walks FIN_ROWS consecutive rows of its 256 columns (round 4: one row per workgroup left the finaliser latency-bound --
// 25 million workgroups of one or two elements per thread at N = 100 000: 30 ms for the 100 GB of a GCTA panel).
constexpr int FIN_ROWS = 32;
template <class F>
__global__ __launch_bounds__(256) void fin_kernel(PanelGeom g, int packed, F f)
{
    const int64_t j = g.col0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= g.N) return;
    for (int64_t ib = g.row0 + (int64_t)blockIdx.y * FIN_ROWS; ib < g.row1; ib += (int64_t)gridDim.y * FIN_ROWS) {   // grid.y is capped at 65535
        const int64_t ie = (ib + FIN_ROWS < g.row1) ? (ib + FIN_ROWS) : g.row1;
        if (j < ib) continue;                                   // (the whole group lies right of this column only from row j on)
#pragma unroll 4
        for (int64_t i = ib; i < ie; i++) {
            if (j < i) break;
            const int64_t rel = (i - g.row0) * g.ncols_pad + (j - g.col0);                         // uint32 planes: row-major
            const int64_t relf = acc_off(g.ncols_pad, g.f64_tiles_c, i - g.row0, j - g.col0);      // fp64 planes
            OutPos pos;
            if (packed == 2) {          // the panel rectangle itself (in-place finalisation: out == the fp64 accumulator plane)
                pos.a = relf;
                pos.b = -1;
            } else if (packed) {
                pos.a = tri_idx(g.N, i, j) - tri_idx(g.N, g.row0, g.row0);
                pos.b = -1;
            } else {
                pos.a = i * g.N + j;
                pos.b = (i == j) ? -1 : (j * g.N + i);
            }
            f.apply(rel, relf, i, j, pos);
        }
    }
}

template <class F>
static int run_fin(hipStream_t st, const PanelGeom &g, int packed, const F &f)
{
    const int64_t nrows = g.row1 - g.row0;
    if (nrows <= 0) return 0;
    const int64_t ngrp = (nrows + FIN_ROWS - 1) / FIN_ROWS;
    dim3 grid((unsigned)((g.N - g.col0 + 255) / 256), (unsigned)(ngrp < 65535 ? ngrp : 65535));
    hipLaunchKernelGGL(fin_kernel<F>, grid, dim3(256), 0, st, g, packed, f);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- IBS -------------------------------------------------------------------
struct FinIbsNum {
    const uint32_t *acc; int64_t plane; int32_t *o0, *o1, *o2;
    __device__ void apply(int64_t rel, int64_t relf, int64_t, int64_t, OutPos p) const
    {
        const uint32_t n = acc[rel], c1 = acc[plane + rel], c0 = acc[2 * plane + rel] >> 1;   // the plane holds 2 ibs0
        const int32_t v0 = (int32_t)c0, v1 = (int32_t)c1, v2 = (int32_t)(n - c0 - c1);
        o0[p.a] = v0; o1[p.a] = v1; o2[p.a] = v2;
        if (p.b >= 0) { o0[p.b] = v0; o1[p.b] = v1; o2[p.b] = v2; }
    }
};
int launch_fin_ibs_num(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int32_t *o0, int32_t *o1,
                       int32_t *o2, int packed)
{
    FinIbsNum f{acc, g.rows_pad * g.ncols_pad, o0, o1, o2};
    return run_fin(st, g, packed, f);
}

struct FinIbsAve {
    const uint32_t *acc; int64_t plane; double *out;
    __device__ void apply(int64_t rel, int64_t relf, int64_t, int64_t, OutPos p) const
    {
        const uint32_t n = acc[rel], c1 = acc[plane + rel], c0 = acc[2 * plane + rel] >> 1;   // the plane holds 2 ibs0
        const uint32_t c2 = n - c0 - c1;
        // (0.5*IBS1 + IBS2) / (IBS0+IBS1+IBS2) with the reference's uint32 sum, genIBS.cpp:475
        const double v = (0.5 * c1 + c2) / (double)(uint32_t)(c0 + c1 + c2);
        out[p.a] = v;
        if (p.b >= 0) out[p.b] = v;
    }
};
int launch_fin_ibs_ave(hipStream_t st, const PanelGeom &g, const uint32_t *acc, double *out, int packed)
{
    FinIbsAve f{acc, g.rows_pad * g.ncols_pad, out};
    return run_fin(st, g, packed, f);
}

// ---- KING robust -------------------------------------------------------------
// kernel counters {nLoci, ibs1, ibs0, N1, N2} -> TS_KINGRobust {IBS0, nLoci, SumSq, N1_Aa, N2_Aa}
struct FinKingCounts {
    const uint32_t *acc; int64_t plane; uint32_t *out;
    __device__ void apply(int64_t rel, int64_t relf, int64_t, int64_t, OutPos p) const
    {
        const uint32_t n = acc[rel], c1 = acc[plane + rel], c0 = acc[2 * plane + rel] >> 1;   // the plane holds 2 ibs0
        uint32_t *o = out + 5 * p.a;
        o[0] = c0; o[1] = n; o[2] = c1 + 4u * c0; o[3] = acc[3 * plane + rel]; o[4] = acc[4 * plane + rel];
    }
};
int launch_fin_king_counts(hipStream_t st, const PanelGeom &g, const uint32_t *acc, uint32_t *out5)
{
    FinKingCounts f{acc, g.rows_pad * g.ncols_pad, out5};
    return run_fin(st, g, 1, f);
}

struct FinKingRobust {
    KingRobustArgs v; double *ibs0, *kin;
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        double vi, vk;
        if (i == j) {           // genKING.cpp:623
            vi = 0; vk = 0.5;
        } else {
            king_robust_value(v, rel, i, j, vi, vk);
        }
        ibs0[p.a] = vi; kin[p.a] = vk;
        if (p.b >= 0) { ibs0[p.b] = vi; kin[p.b] = vk; }
    }
};
int launch_fin_king_robust(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const int32_t *family,
                           double *ibs0, double *kin, int packed)
{
    FinKingRobust f{KingRobustArgs{acc, g.rows_pad * g.ncols_pad, family}, ibs0, kin};
    return run_fin(st, g, packed, f);
}

// ---- pairs without a shared call (KING-homo, dissimilarity) ---------------------------------------------------------------------------
// Both finalisers divide by weight sums over the SNPs a pair is called at TOGETHER, formed as C - M_i - M_j + B_ij: not exactly 0
// where the true sum is, and the reference has 0 / 0 = NaN there.  Which pairs share no call at an SNP of nonzero weight (0 < p < 1) is
// decided exactly, in integers, block by block.  In a block with Lw such SNPs a pair shares none only if the two samples' missing counts
// there add up to Lw or more, so at least one of them is HEAVY in that block (2 x missing >= Lw).  Per sample: hb = the number of blocks
// it was heavy in, and a slot once it was heavy.  Per slot h and column sample j one word: bit 31 = h and j shared a call in a block
// where h was heavy, bits 0..30 = the number of blocks BOTH were heavy in.  With nb the number of blocks (Lw > 0), the pair (i, j) never
// shared a call  <=>  hb_i + hb_j - both_ij == nb (one of them heavy in every block) and neither word has bit 31.  Ordinary data has no
// heavy sample: one pass over the block counts the missing calls, nothing else runs.  More than NOSH_HEAVY heavy samples: the flag in
// word 2 is set and the finalisers go without (a rounding residue decides those pairs then, as before this existed).
// words: {nb, slots, overflow, heavy in this block, Lw of this block, -, -, -}, cnt[nc], hb[nc], slot[nc] (0: none), list[NOSH_HEAVY], T[NOSH_HEAVY][nc]
__device__ __forceinline__ bool nosh_weighted(const int32_t *sum, const int32_t *num, int64_t k) { return sum[k] > 0 && sum[k] < 2 * num[k]; }

__global__ __launch_bounds__(256) void nosh_count_kernel(const uint8_t *__restrict__ packed, int64_t RB, int64_t n_snp, const int32_t *__restrict__ sum,
                                                         const int32_t *__restrict__ num, int64_t col0, int64_t ncols, uint32_t *__restrict__ ns)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.y * 256, k1 = (k0 + 256 < n_snp) ? (k0 + 256) : n_snp;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t lw = 0;
        for (int64_t k = k0; k < k1; k++) lw += nosh_weighted(sum, num, k) ? 1u : 0u;
        if (lw) atomicAdd(&ns[4], lw);
    }
    if (j >= ncols) return;
    const int64_t s = col0 + j, b = s >> 2;
    const int sh = 2 * (int)(s & 3);
    uint32_t c = 0;
    for (int64_t k = k0; k < k1; k++)
        if (((packed[k * RB + b] >> sh) & 3) == 3 && nosh_weighted(sum, num, k)) c++;
    if (c) atomicAdd(&ns[8 + j], c);
}

__global__ __launch_bounds__(256) void nosh_classify_kernel(int64_t ncols, int64_t nc, uint32_t *__restrict__ ns)
{
    const uint32_t lw = ns[4];
    if (lw == 0) return;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j == 0) ns[0] += 1;                                    // (nobody reads it in this launch)
    if (j >= ncols || 2u * ns[8 + j] < lw) return;
    ns[8 + nc + j] += 1;
    if (!ns[8 + 2 * nc + j]) {
        const uint32_t sl = atomicAdd(&ns[1], 1u);
        if (sl < (uint32_t)NOSH_HEAVY) ns[8 + 2 * nc + j] = sl + 1;
        else ns[2] = 1;
    }
    const uint32_t pos = atomicAdd(&ns[3], 1u);
    if (pos < (uint32_t)NOSH_HEAVY) ns[8 + 3 * nc + pos] = (uint32_t)j;
    else ns[2] = 1;
}

// grid.y = NOSH_HEAVY: the heavy samples of this block, each against every column sample
__global__ __launch_bounds__(256) void nosh_update_kernel(const uint8_t *__restrict__ packed, int64_t RB, int64_t n_snp, const int32_t *__restrict__ sum,
                                                          const int32_t *__restrict__ num, int64_t col0, int64_t ncols, int64_t nc, uint32_t *__restrict__ ns)
{
    const uint32_t lw = ns[4], nh = ns[3] < (uint32_t)NOSH_HEAVY ? ns[3] : (uint32_t)NOSH_HEAVY;
    if (lw == 0 || blockIdx.y >= nh) return;
    const int64_t h = ns[8 + 3 * nc + blockIdx.y];
    const uint32_t sl = ns[8 + 2 * nc + h];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sl == 0 || j >= ncols) return;                         // (no slot: more heavy samples than slots, the flag is set)
    uint32_t *w = ns + 8 + 3 * nc + NOSH_HEAVY + (int64_t)(sl - 1) * nc + j;
    uint32_t v = *w;
    if (2u * ns[8 + j] >= lw) v += 1;
    if (!(v >> 31)) {
        const int64_t sh_ = col0 + h, sj = col0 + j;
        const int64_t bh = sh_ >> 2, bj = sj >> 2;
        const int th = 2 * (int)(sh_ & 3), tj = 2 * (int)(sj & 3);
        for (int64_t k = 0; k < n_snp; k++)
            if (((packed[k * RB + bh] >> th) & 3) != 3 && ((packed[k * RB + bj] >> tj) & 3) != 3 && nosh_weighted(sum, num, k)) { v |= 0x80000000u; break; }
    }
    *w = v;
}

int launch_nosh_block(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, const int32_t *sum, const int32_t *num,
                      int64_t col0, int64_t ncols, int64_t ncols_pad, uint32_t *nosh)
{
    if (n_snp <= 0 || ncols <= 0) return 0;
    const unsigned gx = (unsigned)((ncols + 255) / 256);
    hipLaunchKernelGGL(nosh_count_kernel, dim3(gx, (unsigned)((n_snp + 255) / 256)), dim3(256), 0, st, packed, RB, n_snp, sum, num, col0, ncols, nosh);
    hipLaunchKernelGGL(nosh_classify_kernel, dim3(gx), dim3(256), 0, st, ncols, ncols_pad, nosh);
    hipLaunchKernelGGL(nosh_update_kernel, dim3(gx, NOSH_HEAVY), dim3(256), 0, st, packed, RB, n_snp, sum, num, col0, ncols, ncols_pad, nosh);
    SNPGPU_HIP_CHECK(hipGetLastError());
    SNPGPU_HIP_CHECK(hipMemsetAsync(nosh + 3, 0, sizeof(uint32_t) * 2, st));                       // this block's heavy count and Lw
    SNPGPU_HIP_CHECK(hipMemsetAsync(nosh + 8, 0, sizeof(uint32_t) * (size_t)ncols_pad, st));       // and its missing counts
    return 0;
}

// nosh_never_shared(words, ncols_pad, ri, rj), the read side of these words, is in fin_values.h (the selection kernels share it)

// ---- KING homo ---------------------------------------------------------------
struct FinKingHomo {
    KingHomoArgs v; double *k0, *k1;       // (what the arguments are: fin_values.h)
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        double a = 0, b = 0;
        if (i != j) king_homo_value(v, rel, relf, i, j, a, b);           // genKING.cpp:526-537
        k0[p.a] = a; k1[p.a] = b;
        if (p.b >= 0) { k0[p.b] = a; k1[p.b] = b; }
    }
};
int launch_fin_king_homo(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *facc, double fscale,
                         double *k0, double *k1, int packed, const double *w_const, const double *msum, const uint32_t *called, const uint32_t *nosh)
{
    FinKingHomo f{KingHomoArgs{acc, facc, g.rows_pad * g.ncols_pad, fscale, w_const, msum, g.col0, g.ncols_pad, called, nosh}, k0, k1};
    return run_fin(st, g, packed, f);
}

// ---- individual dissimilarity -------------------------------------------------
// gnrDiss, src/genIBS.cpp:652-683: SumGeno / SumAFreq, twice that on the diagonal; IEEE division, no guard (0/0 = NaN, x/0 = Inf).
// SumAFreq = 8 x KING-homo's first weight sum, the sum of p (1 - p) over the SNPs both samples are called at (the same p,
// genIBS.cpp:353-362), in the same form: C - M_i - M_j + B_ij with B in the fp64 plane (tables x 2^16: fscale) for blocks with missing
// calls, C in w_const (the totals of all blocks).  That difference of sums is not exactly 0 where the true sum is: a sample never
// called at an SNP of nonzero weight (called[] == 0) has SumAFreq = 0 exactly with every sample, so 0 / 0 = NaN as in the reference.
// out == nullptr: the packed sums {SumGeno, SumAFreq} (diagnostics).
struct FinDiss {
    const uint32_t *acc; const double *facc; double fscale; const double *wc, *msum; const uint32_t *called; int64_t col0;
    double *out; uint32_t *gsum; double *wsum; const uint32_t *nosh; int64_t ncols_pad;
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        const uint32_t sg = acc[rel];
        double saf = facc[relf] * fscale + (wc ? wc[0] : 0.0);
        if (msum) saf -= msum[i - col0] + msum[j - col0];
        saf *= 8.0;                                                     // exact: a power of two
        if (!called[i - col0] || !called[j - col0]) saf = 0.0;
        if (nosh && nosh_never_shared(nosh, ncols_pad, i - col0, j - col0)) saf = 0.0;
        if (!out) { gsum[p.a] = sg; wsum[p.a] = saf; return; }
        const double v = (i == j) ? 2 * ((double)sg / saf) : (double)sg / saf;
        out[p.a] = v;
        if (p.b >= 0) out[p.b] = v;
    }
};
int launch_fin_diss(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *facc, double fscale, const double *w_const,
                    const double *msum, const uint32_t *called, double *out, uint32_t *geno_sum, double *wsum, int packed, const uint32_t *nosh)
{
    FinDiss f{acc, facc, fscale, w_const, msum, called, g.col0, out, geno_sum, wsum, nosh, g.ncols_pad};
    return run_fin(st, g, out ? packed : 1, f);
}

// ---- GCTA / covariance ---------------------------------------------------------
// gcta_value, cov_value: fin_values.h
struct FinGcta {
    GctaArgs v; double *out;
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        const double x = gcta_value(v, rel, relf, i, j);
        out[p.a] = x;
        if (p.b >= 0) out[p.b] = x;
    }
};

struct FinCov {
    CovArgs v; double *out;
    __device__ void apply(int64_t rel, int64_t relf, int64_t, int64_t, OutPos p) const
    {
        const double x = cov_value(v, relf);
        out[p.a] = x;
        if (p.b >= 0) out[p.b] = x;
    }
};
int launch_fin_cov(hipStream_t st, const PanelGeom &g, const double *num, double scale, double *out, int packed)
{
    FinCov f{CovArgs{num, scale}, out};
    return run_fin(st, g, packed, f);
}

// ---- PLINK method of moments ------------------------------------------------------
// Est_PLINK_Kinship, src/genIBD.cpp:341-390; kernel counters {n, ibs1, ibs0}
struct FinMom {
    MomArgs v; double *k0, *k1;
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        double a = 0, b = 0;
        if (i != j) mom_value(v, rel, a, b);
        k0[p.a] = a; k1[p.a] = b;
        if (p.b >= 0) { k0[p.b] = a; k1[p.b] = b; }
    }
};
int launch_fin_mom(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *e, int constraint,
                   double *k0, double *k1, int packed)
{
    FinMom f{MomArgs{acc, g.rows_pad * g.ncols_pad, e[0], e[1], e[2], e[3], e[4], constraint}, k0, k1};
    return run_fin(st, g, packed, f);
}

// ---- EIGMIX -------------------------------------------------------------------------
// eigmix_value, fin_values.h
struct FinEigmix {
    EigmixArgs v; double *out;
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        const double x = eigmix_value(v, relf, i, j);
        out[p.a] = x;
        if (p.b >= 0) out[p.b] = x;
    }
};
int launch_fin_eigmix(hipStream_t st, const PanelGeom &g, const double *num, const double *dd, const uint32_t *het,
                      const double *dmiss, const double *dsq, const double *d_sumden, int diagadj, double scale,
                      double *out, int packed)
{
    FinEigmix f{EigmixArgs{num, dd, het, dmiss, dsq, d_sumden, diagadj, scale}, out};
    return run_fin(st, g, packed, f);
}

// ---- individual beta ------------------------------------------------------------------
// beta_raw, beta_value: fin_values.h

// min over all entries and sum over the off-diagonal entries of the raw values
__global__ __launch_bounds__(256) void beta_reduce_kernel(PanelGeom g, const uint32_t *__restrict__ acc,
                                                          int diag_inbreeding, double *__restrict__ pmin,
                                                          double *__restrict__ psum)
{
    const int64_t plane = g.rows_pad * g.ncols_pad;
    double mn = 1e300, sm = 0;
    for (int64_t i = g.row0 + blockIdx.x; i < g.row1; i += gridDim.x)
        for (int64_t j = i + threadIdx.x; j < g.N; j += 256) {
            const int64_t rel = (i - g.row0) * g.ncols_pad + (j - g.col0);
            const double v = beta_raw(acc, plane, rel, (i == j) && diag_inbreeding);
            if (v < mn) mn = v;
            if (i != j) sm += v;
        }
    __shared__ double rmin[256], rsum[256];
    rmin[threadIdx.x] = mn; rsum[threadIdx.x] = sm;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            rsum[threadIdx.x] += rsum[threadIdx.x + off];
            if (rmin[threadIdx.x + off] < rmin[threadIdx.x]) rmin[threadIdx.x] = rmin[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { pmin[blockIdx.x] = rmin[0]; psum[blockIdx.x] = rsum[0]; }
}
int launch_beta_reduce(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int diag_inbreeding, double *partial_min,
                       double *partial_sum, int nblocks)
{
    hipLaunchKernelGGL(beta_reduce_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, g, acc, diag_inbreeding,
                       partial_min, partial_sum);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

struct FinBeta {
    BetaArgs v; double *out;
    __device__ void apply(int64_t rel, int64_t relf, int64_t i, int64_t j, OutPos p) const
    {
        const double x = beta_value(v, rel, i, j);
        out[p.a] = x;
        if (p.b >= 0) out[p.b] = x;
    }
};
int launch_fin_beta(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int mode, double avg, double mn, double *out,
                    int packed)
{
    FinBeta f{BetaArgs{acc, g.rows_pad * g.ncols_pad, mode, avg, mn}, out};
    return run_fin(st, g, packed, f);
}

__global__ __launch_bounds__(256) void trace_kernel(PanelGeom g, const double *__restrict__ num,
                                                    double *__restrict__ d_trace)
{
    double s = 0;
    for (int64_t i = g.row0 + threadIdx.x; i < g.row1; i += 256)
        s += num[acc_off(g.ncols_pad, g.f64_tiles_c, i - g.row0, i - g.col0)];
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_trace = red[0];
}
int launch_trace(hipStream_t st, const PanelGeom &g, const double *num, double *d_trace)
{
    hipLaunchKernelGGL(trace_kernel, dim3(1), dim3(256), 0, st, g, num, d_trace);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// copy the upper triangle of the panel's diagonal block (rows I x columns I) onto its lower
// triangle, so that the block can be used as a dense symmetric operand
__global__ __launch_bounds__(256) void mirror_diag_kernel(PanelGeom g, double *__restrict__ num)
{
    const int64_t nI = g.row1 - g.row0;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;      // column within the block
    for (int64_t i = blockIdx.y; i < nI; i += gridDim.y)            // row within the block
        if (j < i) num[acc_off(g.ncols_pad, g.f64_tiles_c, i, j)] = num[acc_off(g.ncols_pad, g.f64_tiles_c, j, i)];
}
// the same inside the T x T tiles on the diagonal only (all the one-pass symmetric panel product reads below
// the diagonal)
__global__ __launch_bounds__(256) void mirror_diag_tiles_kernel(PanelGeom g, double *__restrict__ num, int T)
{
    const int64_t nI = g.row1 - g.row0;
    const int64_t t0 = (int64_t)blockIdx.x * T;
    for (int e = threadIdx.x; e < T * T; e += 256) {
        const int64_t i = t0 + e / T, j = t0 + e % T;
        if (j < i && i < nI) num[acc_off(g.ncols_pad, g.f64_tiles_c, i, j)] = num[acc_off(g.ncols_pad, g.f64_tiles_c, j, i)];
    }
}
int launch_mirror_diag_tiles(hipStream_t st, const PanelGeom &g, double *num, int T)
{
    const int64_t nI = g.row1 - g.row0;
    if (nI <= 1) return 0;
    hipLaunchKernelGGL(mirror_diag_tiles_kernel, dim3((unsigned)((nI + T - 1) / T)), dim3(256), 0, st, g, num, T);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mirror_diag(hipStream_t st, const PanelGeom &g, double *num)
{
    const int64_t nI = g.row1 - g.row0;
    if (nI <= 1) return 0;
    dim3 grid((unsigned)((nI + 255) / 256), (unsigned)(nI < 65535 ? nI : 65535));
    hipLaunchKernelGGL(mirror_diag_kernel, grid, dim3(256), 0, st, g, num);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// GCTA needs M(s,s) for every column sample, which lies outside a non-full panel's rows: a
// per-sample count vector `diag` (absolute sample index) is accumulated by miss_diag_kernel below.
int launch_fin_gcta(hipStream_t st, const PanelGeom &g, const double *num, const uint32_t *miss,
                    const uint32_t *diag, const unsigned long long *d_nlocus, double *out, int packed,
                    const double *colterm, const double *uvterm)
{
    FinGcta f{GctaArgs{num, miss, d_nlocus, diag, colterm, uvterm, g.row0, g.col0, g.ncols_pad}, out};
    return run_fin(st, g, packed, f);
}

// Rank-one terms of the two-product pair kernel (blocks without missing calls): ibs1 += H_r + H_c, 2 ibs0 += 2 (T_r + T_c), and for KING-robust
// N1_Aa += H_r, N2_Aa += H_c, over the whole panel rectangle; then the counts start over.
__global__ __launch_bounds__(256) void het_settle_kernel(uint32_t *__restrict__ acc, int64_t plane, int64_t rows_pad,
                                                         int64_t ncols_pad, const uint32_t *__restrict__ het, int king,
                                                         int p1, int p0)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols_pad) return;
    const uint32_t hc = het[c];
    for (int64_t r = blockIdx.y; r < rows_pad; r += gridDim.y) {
        const uint32_t hr = het[r];           // panel-relative rows and columns start at the same sample
        const int64_t e = r * ncols_pad + c;
        const uint32_t tr = het[ncols_pad + r], tc = het[ncols_pad + c];                    // #(g == 2) of row and column sample
        if (hr + hc) acc[p1 * plane + e] += hr + hc;                                         // ibs1 += H_r + H_c
        if (tr + tc) acc[p0 * plane + e] += 2u * (tr + tc);                                  // 2 ibs0 += 2 (T_r + T_c)
        if (king) {
            if (hr) acc[3 * plane + e] += hr;
            if (hc) acc[4 * plane + e] += hc;
        }
    }
}

// The same for the dissimilarity counter (one plane): SumGeno = 2 S_r + 2 S_c - 2 g.g' in a block without missing calls, S = H + 2 T the
// sample's genotype sum over those blocks; the pair kernel added - 2 g.g'.
__global__ __launch_bounds__(256) void diss_settle_kernel(uint32_t *__restrict__ acc, int64_t rows_pad, int64_t ncols_pad,
                                                          const uint32_t *__restrict__ het)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols_pad) return;
    const uint32_t sc = het[c] + 2u * het[ncols_pad + c];
    for (int64_t r = blockIdx.y; r < rows_pad; r += gridDim.y) {
        const uint32_t sr = het[r] + 2u * het[ncols_pad + r];     // panel-relative rows and columns start at the same sample
        if (sr + sc) acc[r * ncols_pad + c] += 2u * (sr + sc);
    }
}

// a column sample is flagged at its first call at an SNP with 0 < p < 1 (sum, num over all samples); flagged samples skip the block
__global__ __launch_bounds__(256) void diss_called_kernel(const uint8_t *__restrict__ packed, int64_t RB, int64_t n_snp,
                                                          const int32_t *__restrict__ sum, const int32_t *__restrict__ num, int64_t col0,
                                                          int64_t ncols, uint32_t *__restrict__ called)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncols || called[j]) return;
    const int64_t s = col0 + j, b = s >> 2;
    const int sh = 2 * (int)(s & 3);
    for (int64_t k = 0; k < n_snp; k++) {
        const int32_t sk = sum[k], nk = num[k];
        if (sk > 0 && sk < 2 * nk && ((packed[k * RB + b] >> sh) & 3) != 3) { called[j] = 1u; return; }
    }
}

int launch_diss_called(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, const int32_t *sum, const int32_t *num,
                       int64_t col0, int64_t ncols, uint32_t *called)
{
    if (n_snp <= 0 || ncols <= 0) return 0;
    hipLaunchKernelGGL(diss_called_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, st, packed, RB, n_snp, sum, num, col0, ncols,
                       called);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_diss_settle(hipStream_t st, uint32_t *acc, int64_t rows_pad, int64_t ncols_pad, uint32_t *het)
{
    dim3 grid((unsigned)((ncols_pad + 255) / 256), (unsigned)std::min<int64_t>(rows_pad, 4096));
    hipLaunchKernelGGL(diss_settle_kernel, grid, dim3(256), 0, st, acc, rows_pad, ncols_pad, het);
    SNPGPU_HIP_CHECK(hipGetLastError());
    SNPGPU_HIP_CHECK(hipMemsetAsync(het, 0, sizeof(uint32_t) * (size_t)(2 * ncols_pad), st));
    return 0;
}

int launch_het_settle(hipStream_t st, uint32_t *acc, int64_t plane, int64_t rows_pad, int64_t ncols_pad, uint32_t *het,
                      int king, int plane_ibs1, int plane_ibs0x2)
{
    dim3 grid((unsigned)((ncols_pad + 255) / 256), (unsigned)std::min<int64_t>(rows_pad, 4096));
    hipLaunchKernelGGL(het_settle_kernel, grid, dim3(256), 0, st, acc, plane, rows_pad, ncols_pad, het, king, plane_ibs1,
                       plane_ibs0x2);
    SNPGPU_HIP_CHECK(hipGetLastError());
    SNPGPU_HIP_CHECK(hipMemsetAsync(het, 0, sizeof(uint32_t) * (size_t)(2 * ncols_pad), st));
    return 0;
}

// per-sample popcount of the missing plane (uint2 words, word-major colp layout) added to diag[s]
__global__ __launch_bounds__(256) void miss_diag_kernel(const uint2 *__restrict__ colp, int KWv, int64_t ncols_pad,
                                                        int64_t col0, uint32_t *__restrict__ diag,
                                                        const unsigned long long *__restrict__ skip)
{
    if (skip && *skip == 0ull) return;
    const int64_t sc = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sc >= ncols_pad) return;
    uint32_t c = 0;
    for (int k = 0; k < KWv; k++) {
        const uint2 v = colp[(int64_t)k * ncols_pad + sc];
        c += __popc(v.x) + __popc(v.y);
    }
    diag[col0 + sc] += c;
}
int launch_miss_diag(hipStream_t st, const uint2 *colp, int KWv, int64_t ncols_pad, int64_t col0, uint32_t *diag,
                     const unsigned long long *skip)
{
    hipLaunchKernelGGL(miss_diag_kernel, dim3((unsigned)((ncols_pad + 255) / 256)), dim3(256), 0, st, colp, KWv,
                       ncols_pad, col0, diag, skip);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// Exact-row SYRK: the kernel accumulates sum_s (g_is - c_s) w_js; the part - sum_s (avg_s - c_s) w_js = - T[j] is the same
// for every row i and is applied here, once per result request: acc[i][j] -= T[j] for the real rows i and the stored
// columns j >= 256 floor(i / 256) (the tiles that touch the upper trapezoid), then T is cleared.
__global__ __launch_bounds__(256) void colterm_settle_kernel(double *__restrict__ acc, int64_t ld, int64_t tiles_c,
                                                             int64_t n_rows_real, int64_t ncols_pad, int64_t n_cols_real,
                                                             const double *__restrict__ colterm,
                                                             const double *__restrict__ uvterm)
{
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // (the padding columns stay zero: the row terms R[i] are not zero there, and the eigen solver's panel product reads the
    // columns up to the next multiple of 16)
    if (col >= n_cols_real) return;
    // single-product blocks (syrk_uv_kernel): acc[i][j] -= R[i] + Q[j] - K, uvterm = {R[ncols_pad], Q[ncols_pad], K}
    const double t = colterm[col] + (uvterm ? uvterm[ncols_pad + col] - uvterm[2 * ncols_pad] : 0.0);
    if (!uvterm && t == 0.0) return;
    const int64_t r_end_all = (col / 256 + 1) * 256;                 // rows whose tile row starts at or left of this column
    const int64_t r_end = r_end_all < n_rows_real ? r_end_all : n_rows_real;
    const int64_t per = (r_end + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = (r0 + per < r_end) ? (r0 + per) : r_end;
    if (uvterm) for (int64_t r = r0; r < r1; r++) acc[acc_off(ld, tiles_c, r, col)] -= t + uvterm[r];
    else for (int64_t r = r0; r < r1; r++) acc[acc_off(ld, tiles_c, r, col)] -= t;
}

int launch_colterm_settle(hipStream_t st, double *acc, int64_t ld, int64_t tiles_c, int64_t n_rows_real, int64_t ncols_pad,
                          int64_t n_cols_real, double *colterm, double *uvterm)
{
    if (n_rows_real <= 0) return 0;
    int gy = (int)((n_rows_real + 255) / 256);
    if (gy > 256) gy = 256;
    hipLaunchKernelGGL(colterm_settle_kernel, dim3((unsigned)((ncols_pad + 255) / 256), (unsigned)gy), dim3(256), 0, st, acc, ld,
                       tiles_c, n_rows_real, ncols_pad, n_cols_real, colterm, uvterm);
    SNPGPU_HIP_CHECK(hipGetLastError());
    SNPGPU_HIP_CHECK(hipMemsetAsync(colterm, 0, sizeof(double) * (size_t)ncols_pad, st));
    if (uvterm) SNPGPU_HIP_CHECK(hipMemsetAsync(uvterm, 0, sizeof(double) * (size_t)(2 * ncols_pad + 2), st));
    return 0;
}

}  // namespace snpgpu
