// The VALUE part of the relatedness and GRM finalisers, shared by the finaliser functors (kernels_final.hip), which write every pair of
// a panel, and the selection kernels (kernels_select.hip), which write the pairs at or above a cutoff (and, for the GRM kinds, the
// diagonal): one source of each expression, so that a selected pair carries the bits the finaliser would have written for it.
// Index conventions, as in the functors: `rel` / `relf` are element offsets in the uint32 / fp64 accumulator planes (panel-relative),
// msum, called and nosh are indexed relative to the panel's first column (i - col0), fam by ABSOLUTE sample.
#pragma once
#include "snpgpu_internal.h"

#include <math.h>

namespace snpgpu {

// ri, rj: the samples relative to the panel's first column (see "pairs without a shared call", kernels_final.hip)
__device__ __forceinline__ bool nosh_never_shared(const uint32_t *ns, int64_t nc, int64_t ri, int64_t rj)
{
    const uint32_t nb = ns[0];
    if (nb == 0 || ns[2]) return false;
    const uint32_t hi = ns[8 + nc + ri], hj = ns[8 + nc + rj];
    if (hi + hj < nb) return false;
    const uint32_t si = ns[8 + 2 * nc + ri], sj = ns[8 + 2 * nc + rj];
    const uint32_t *T = ns + 8 + 3 * nc + NOSH_HEAVY;
    const uint32_t wi = si ? T[(int64_t)(si - 1) * nc + rj] : 0u, wj = sj ? T[(int64_t)(sj - 1) * nc + ri] : 0u;
    if ((wi | wj) >> 31) return false;
    const uint32_t both = (si ? wi : wj) & 0x7fffffffu;
    return hi + hj - both == nb;
}

// ---- KING robust: off-diagonal pair (i != j); kernel counters {nLoci, ibs1, 2 ibs0, N1, N2}, genKING.cpp:604-650 -----------------------
struct KingRobustArgs {
    const uint32_t *acc; int64_t plane; const int32_t *fam;
};
__device__ __forceinline__ void king_robust_value(const KingRobustArgs &a, int64_t rel, int64_t i, int64_t j, double &vi, double &vk)
{
    const uint32_t n = a.acc[rel], c1 = a.acc[a.plane + rel], c0 = a.acc[2 * a.plane + rel] >> 1;   // the plane holds 2 ibs0
    const uint32_t n1 = a.acc[3 * a.plane + rel], n2 = a.acc[4 * a.plane + rel];
    const uint32_t sumsq = c1 + 4u * c0;
    vi = (n > 0) ? ((double)c0 / n) : (double)NAN;
    const int f1 = a.fam ? a.fam[i] : -1, f2 = a.fam ? a.fam[j] : -1;
    double v = (f1 == f2 && f1 >= 0) ? (0.5 - sumsq / (2.0 * (uint32_t)(n1 + n2)))
                                     : (0.5 - sumsq / (4.0 * (n1 < n2 ? n1 : n2)));
    if (!isfinite(v)) v = (double)NAN;
    vk = v;
}

// ---- KING homo: off-diagonal pair, genKING.cpp:526-537 ------------------------------------------------------------------------------------
struct KingHomoArgs {
    const uint32_t *acc; const double *facc; int64_t plane; double fscale; const double *wc;
    // round 5: blocks with missing calls leave B_ij = sum c mu_i mu_j in the planes and per-sample sums M in msum[2][ncols_pad]:
    // masked sum = C - M_i - M_j + B_ij with C in wc (the totals of ALL blocks then); msum == nullptr: the planes hold the masked sums
    const double *msum; int64_t col0, ncols_pad;
    // that difference of sums is not exactly 0 where the true sum is: a sample never called at an SNP of nonzero weight (called[] == 0, as
    // FinDiss) has both weight sums 0 exactly with every sample, so 0 / 0 = NaN as in the reference.  Two samples that are both
    // called somewhere and share no call: nosh (kernels_final.hip), here and in FinDiss
    const uint32_t *called;
    const uint32_t *nosh;
};
__device__ __forceinline__ void king_homo_value(const KingHomoArgs &h, int64_t rel, int64_t relf, int64_t i, int64_t j, double &a, double &b)
{
    const uint32_t c1 = h.acc[rel], c0 = h.acc[h.plane + rel] >> 1;   // the plane holds 2 ibs0
    const uint32_t sumsq = c1 + 4u * c0;
    // tables may be pre-scaled; blocks without missing calls contribute the same sum to every pair (wc)
    double saf = h.facc[relf] * h.fscale + (h.wc ? h.wc[0] : 0.0), saf2 = h.facc[h.plane + relf] * h.fscale + (h.wc ? h.wc[1] : 0.0);
    if (h.msum) {
        saf -= h.msum[i - h.col0] + h.msum[j - h.col0];
        saf2 -= h.msum[h.ncols_pad + i - h.col0] + h.msum[h.ncols_pad + j - h.col0];
    }
    if (h.called && (!h.called[i - h.col0] || !h.called[j - h.col0])) saf = saf2 = 0.0;
    if (h.nosh && nosh_never_shared(h.nosh, h.ncols_pad, i - h.col0, j - h.col0)) saf = saf2 = 0.0;
    const double theta = 0.5 - sumsq / (8 * saf);
    const double v0 = c0 / (2 * saf2);
    const double v1 = 2 - 2 * v0 - 4 * theta;
    a = isfinite(v0) ? v0 : (double)NAN;
    b = isfinite(v1) ? v1 : (double)NAN;
}

// ---- PLINK method of moments: off-diagonal pair; Est_PLINK_Kinship, src/genIBD.cpp:341-390; kernel counters {n, ibs1, 2 ibs0} -------------
struct MomArgs {
    const uint32_t *acc; int64_t plane; double e00, e01, e02, e11, e12; int constraint;
};
// the same from the three counts of a pair (the listed-pairs EM of kernels_ibd.hip counts them itself)
__device__ __forceinline__ void mom_from_counts(double e00, double e01, double e02, double e11, double e12, int constraint, int n012,
                                                int IBS1, int IBS0, double &a, double &b)
{
    const int IBS2 = n012 - IBS0 - IBS1;
    const double f00 = e00 * n012, f01 = e01 * n012, f11 = e11 * n012, f02 = e02 * n012, f12 = e12 * n012,
                 f22 = 1.0 * n012;
    double v0 = IBS0 / f00;
    double v1 = (IBS1 - v0 * f01) / f11;
    double v2 = (IBS2 - v0 * f02 - v1 * f12) / f22;
    if (v0 > 1) { v0 = 1; v1 = v2 = 0; }
    if (v1 > 1) { v1 = 1; v0 = v2 = 0; }
    if (v2 > 1) { v2 = 1; v0 = v1 = 0; }
    if (v0 < 0) { const double S = v1 + v2; v1 /= S; v2 /= S; v0 = 0; }
    if (v1 < 0) { const double S = v0 + v2; v0 /= S; v2 /= S; v1 = 0; }
    if (v2 < 0) { const double S = v0 + v1; v0 /= S; v1 /= S; v2 = 0; }
    if (constraint) {
        v2 = 1 - v0 - v1;
        const double pihat = v1 / 2 + v2;
        if (pihat * pihat < v2) { v0 = (1 - pihat) * (1 - pihat); v1 = 2 * pihat * (1 - pihat); }
    }
    a = v0; b = v1;
}
__device__ __forceinline__ void mom_value(const MomArgs &m, int64_t rel, double &a, double &b)
{
    const int n012 = (int)m.acc[rel], IBS1 = (int)m.acc[m.plane + rel], IBS0 = (int)(m.acc[2 * m.plane + rel] >> 1);
    mom_from_counts(m.e00, m.e01, m.e02, m.e11, m.e12, m.constraint, n012, IBS1, IBS0, a, b);
}

// kinship of a pair from its k0 / k1 (snpgdsIBDSelection, R/IBD.R:487).  0.5 and 0.25 are powers of two: both products are exact, the
// sum rounds once with or without a fused multiply-add
__device__ __forceinline__ double kinship_k0k1(double k0, double k1) { return (1 - k0 - k1) * 0.5 + k1 * 0.25; }

// ---- the GRM kinds: ANY entry i <= j of the panel, the diagonal included (FinGcta / FinCov / FinEigmix / FinBeta, the GRM selection and its
// diagonal kernel).  diag, het, dmiss, dsq are indexed by ABSOLUTE sample, colterm / uvterm relative to the panel ------------------------------

// GCTA: Denom(i,j) = #polymorphic SNPs where i or j is missing = M(i,i) + M(j,j) - M(i,j) with M = both-missing counts;
// result = num / (2 (nLocus - Denom)), no guard (genPCA.cpp:1232-1236)
struct GctaArgs {
    const double *num; const uint32_t *miss; const unsigned long long *nlocus;
    const uint32_t *diag;  // M(s,s) for every sample s (absolute index)
    // the pending column / row / constant terms of the fp16 SYRK kernels (colterm_settle_kernel's job, folded in here: the
    // sums stay as they are, so further blocks may follow): num - (T[c] + Q[c] + R[r] - K), panel-relative r, c
    const double *colterm, *uvterm; int64_t row0, col0, ncols_pad;
};
__device__ __forceinline__ double gcta_value(const GctaArgs &a, int64_t rel, int64_t relf, int64_t i, int64_t j)
{
    const long long nl = (long long)*a.nlocus;
    const long long den = (long long)a.diag[i] + (long long)a.diag[j] - (long long)a.miss[rel];
    double s = a.num[relf];
    if (a.colterm) {
        const int64_t r = i - a.row0, c = j - a.col0;
        s -= a.colterm[c] + (a.uvterm ? a.uvterm[a.ncols_pad + c] + a.uvterm[r] - a.uvterm[2 * a.ncols_pad] : 0.0);
    }
    return s / (double)(2 * (nl - den));
}

// a plane times a factor: the trace-normalised covariance, and a panel finalised in place (snpgpu_finalize_inplace)
struct CovArgs {
    const double *num; double scale;
};
__device__ __forceinline__ double cov_value(const CovArgs &a, int64_t relf) { return a.num[relf] * a.scale; }

// EIGMIX: ibd = (num - diagadj*het_i [i==j]) / (SumDenominator - Denom),  Denom(i,j) = sum of 4p(1-p) over the SNPs where i or j is
// missing = dmiss[i] + dmiss[j] - dd(i,j)   (src/genEIGMIX.cpp:113-155)
struct EigmixArgs {
    const double *num, *dd; const uint32_t *het; const double *dmiss, *dsq; const double *sumden; int diagadj; double scale;
};
__device__ __forceinline__ double eigmix_value(const EigmixArgs &a, int64_t relf, int64_t i, int64_t j)
{
    double v = (i == j) ? a.dsq[i] : a.num[relf];     // diagonal numerator from the fp64 per-sample sums
    if (i == j && a.diagadj) v -= (double)a.het[i];
    return v / (*a.sumden - (a.dmiss[i] + a.dmiss[j] - a.dd[relf])) * a.scale;
}

// individual beta: kernel counters {num, x1, x2}: ibscnt = x1 + 2*x2 (src/genBeta.cpp:170-176)
__device__ __forceinline__ double beta_raw(const uint32_t *acc, int64_t plane, int64_t rel, bool diag_m1)
{
    const uint32_t num = acc[rel], ibscnt = acc[plane + rel] + 2u * acc[2 * plane + rel];
    return diag_m1 ? ((double)ibscnt / num - 1) : ((0.5 * ibscnt) / num);
}
// mn, avg: the minimum of all raw values and the mean of the off-diagonal ones (beta_reduce_kernel)
struct BetaArgs {
    const uint32_t *acc; int64_t plane; int mode; double avg, mn;
};
__device__ __forceinline__ double beta_value(const BetaArgs &a, int64_t rel, int64_t i, int64_t j)
{
    if (a.mode == 2) {                   // CalcIndivBetaGRM, src/genBeta.cpp:263-357
        const double r = beta_raw(a.acc, a.plane, rel, i == j);
        const double scale = 2.0 / (1 - a.mn);
        return (i == j) ? ((r - a.mn) * scale * 0.5 + 1) : ((r - a.mn) * scale);
    }
    // gnrIBD_Beta, src/genBeta.cpp:384-452
    const double r = beta_raw(a.acc, a.plane, rel, (i == j) && a.mode == 1);
    return (r - a.avg) * (1.0 / (1 - a.avg));
}

}  // namespace snpgpu
