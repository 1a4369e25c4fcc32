// Device code that both IBD-MLE translation units need: kernels_ibd.hip (EM, matrix and listed pairs) and
// kernels_ibd_methods.hip (downhill simplex and Jacquard's nine coefficients of listed pairs).  The per-SNP likelihood table,
// the running-product helpers, the wave reductions, and the three pieces every one-wave-per-pair kernel starts with: the queue
// take, the integer pre-sweep for the IBS counts with Est_PLINK_Kinship, and the 0.005 clamp of the start values.
#pragma once
#include "snpgpu_internal.h"
#include "fin_values.h"

#include <cmath>

namespace snpgpu {

constexpr double LN2 = 0.69314718055994530942;

// per-SNP constants (wave-uniform in the lane-per-pair kernels): {q, p, p q, 4 p q}
struct IbdSnp { double q, p, pq, pq4; };

// E[IBS | IBD] of Init_EPrIBD_IBS: {E00, E01, E02, E11, E12}
struct IbdE { double e00, e01, e02, e11, e12; };

// The usable-SNP table of codes (a, b) for allele frequency (q, p): factor c and the three coefficients.
__device__ inline void ibd_terms(unsigned a, unsigned b, const IbdSnp &s, double &c, double &a0, double &a1, double &a2)
{
    const bool same = a == b, hh = (a & b) == 1u && same, het = (a == 1u) | (b == 1u);
    const unsigned hom = same ? a : a + b - 1u;          // the homozygote of a hom/het pair
    const double x = hom == 0u ? s.q : s.p;
    const double xx = x * x;
    // selects, not branches: the lanes of a wave hold different classes
    const double pqx = s.pq * x, pq2 = s.pq * s.pq, x2 = x + x;
    a0 = hh ? s.pq4 : same ? xx : het ? x2 : 1.0;
    a1 = hh ? 1.0 : same ? x : het ? 1.0 : 0.0;
    a2 = hh ? 2.0 : same ? 1.0 : 0.0;
    c = hh ? s.pq : same ? xx : het ? pqx : pq2;
}

__device__ inline void renorm(double &prod, int &ex)
{
    int e;
    prod = frexp(prod, &e);
    ex += e;
}

__device__ inline double recip(double s)
{
    double r = __builtin_amdgcn_rcp(s);
    double e = fma(-s, r, 1.0);
    r = fma(r, e, r);
    e = fma(-s, r, 1.0);
    return fma(r, e, r);
}

// sums over the 64 lanes by an xor butterfly (32, 16, .. 1): every lane ends with the same bits
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline IbdSnp snp_of_p(double p)
{
    IbdSnp t;
    const double q = 1 - p;
    t.q = q; t.p = p; t.pq = p * q; t.pq4 = 4 * p * q;
    return t;
}

// ---- one wave per pair: what every kernel of that mapping starts with ----------------------------------------------------------
// the next pair of the queue (queue[0]); lane 0 takes it, every lane gets it
__device__ inline int64_t take_pair(unsigned long long *__restrict__ queue, int lane)
{
    unsigned long long next = 0;
    if (lane == 0) next = atomicAdd(queue, 1ull);
    return (int64_t)__shfl(next, 0);
}

// the pair's IBS counts from the unmasked codes (exact; nb steps of 64 words), then Est_PLINK_Kinship: (a, b) = (k0, k1) before the clamp
__device__ inline void pair_mom_start(const uint32_t *__restrict__ ga, const uint32_t *__restrict__ gb, int64_t nb, int lane,
                                      const IbdE &e, int constraint, double &a, double &b)
{
    int cn = 0, c1 = 0, c0 = 0;
    for (int64_t bk = 0; bk < nb; bk++) {
        const uint32_t wa = ga[bk * 64 + lane], wb = gb[bk * 64 + lane];
        const uint32_t both = ~(wa & (wa >> 1)) & ~(wb & (wb >> 1)) & 0x55555555u;
        const uint32_t x = wa ^ wb, lo = x & both, hi = (x >> 1) & both;     // |a - b| = 1: x = 01 or 11; 2: x = 10
        cn += __popc(both); c1 += __popc(lo); c0 += __popc(hi & ~lo);
    }
    cn = wave_sum(cn); c1 = wave_sum(c1); c0 = wave_sum(c0);
    mom_from_counts(e.e00, e.e01, e.e02, e.e11, e.e12, constraint, cn, c1, c0, a, b);
}

// each of k0, k1, k2 >= 0.005 and renormalised (src/genIBD.cpp:824-832)
__device__ inline void clamp_start(double a, double b, double &k0, double &k1)
{
    double c = 1 - a - b;
    if (a < 0.005) a = 0.005;
    if (b < 0.005) b = 0.005;
    if (c < 0.005) c = 0.005;
    const double s = a + b + c;
    k0 = a / s; k1 = b / s;
}

}  // namespace snpgpu
