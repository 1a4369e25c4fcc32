// Device code that both LD translation units need: kernels_ld.hip (snpgdsLDMat's finalisers, the pruning bits) and
// kernels_ld_score.hip (the LD-score terms): the LD value of one 3 x 3 genotype table.
#pragma once
#include "snpgpu_internal.h"

#include <cmath>
#include <cfloat>

namespace snpgpu {

// ---- LD value of one table (fp64, the reference's formulas and NaN rules) -------------------------------------------------------
// The reference's operations in its order, and no contraction into FMAs (the pragma in each body), so that the value matches a
// plain fp64 evaluation of the same formulas.

__device__ __forceinline__ double ld_plog(double v) { return log(v + DBL_EPSILON); }

// haplotype proportions by EM, src/genLD.cpp:254-331
__device__ inline void ld_haplo(long nAA, long nAB, long nBA, long nBB, long nDH2, double &pAA, double &pAB, double &pBA, double &pBB)
{
#pragma clang fp contract(off)
    const double f = 0.01;
    const double tol_rel = sqrt(DBL_EPSILON);
    const double tot = (double)(nAA + nAB + nBA + nBB + nDH2);
    if (tot > 0 && nDH2 > 0) {
        const double div = nAA + nAB + nBA + nBB + 4.0 * f;
        pAA = (nAA + f) / div; pAB = (nAB + f) / div; pBA = (nBA + f) / div; pBB = (nBB + f) / div;
        const long nDH = nDH2 / 2;
        double old = nAA * ld_plog(pAA) + nAB * ld_plog(pAB) + nBA * ld_plog(pBA) + nBB * ld_plog(pBB) +
                     nDH * ld_plog(pAA * pBB + pAB * pBA);
        double tol = fabs(tol_rel * old);
        if (tol < DBL_EPSILON) tol = DBL_EPSILON;
        for (int it = 1; it <= 1000; it++) {
            const double x = pAA * pBB, y = pAB * pBA;
            const double dAA = x / (x + y) * nDH;
            const double dAB = nDH - dAA;
            pAA = (nAA + dAA) / tot; pAB = (nAB + dAB) / tot; pBA = (nBA + dAB) / tot; pBB = (nBB + dAA) / tot;
            const double ll = nAA * ld_plog(pAA) + nAB * ld_plog(pAB) + nBA * ld_plog(pBA) + nBB * ld_plog(pBB) +
                              nDH * ld_plog(pAA * pBB + pAB * pBA);
            if (fabs(ll - old) <= tol) break;
            old = ll;
        }
    } else {
        pAA = nAA / tot; pAB = nAB / tot; pBA = nBA / tot; pBB = nBB / tot;
    }
}

// n[3 a + b]: a = genotype of the first SNP, b = of the second
__device__ inline double ld_value(int method, const long (&n)[9])
{
#pragma clang fp contract(off)
    const long r0 = n[0] + n[1] + n[2], r1 = n[3] + n[4] + n[5], r2 = n[6] + n[7] + n[8];   // first SNP's genotype counts
    const long c0 = n[0] + n[3] + n[6], c1 = n[1] + n[4] + n[7], c2 = n[2] + n[5] + n[8];   // second SNP's
    const long tot = r0 + r1 + r2;
    const double NaN = __builtin_nan("");
    switch (method) {
    case SNPGPU_LD_COMPOSITE: {                        // src/genLD.cpp:177-213
        if (tot <= 0) return NaN;
        const double delta = double(n[8] + n[0] - n[2] - n[6]) / (2 * tot) - double(r0 - r2) * double(c0 - c2) / (2.0 * tot * tot);
        const double pa = double(2 * r0 + r1) / (2 * tot);
        const double pA = 1 - pa, pAA = double(r2) / tot;
        const double pb = double(2 * c0 + c1) / (2 * tot);
        const double pB = 1 - pb, pBB = double(c2) / tot;
        const double DA = pAA - pA * pA, DB = pBB - pB * pB;
        const double t = (pA * pa + DA) * (pB * pb + DB);
        return t > 0 ? delta / sqrt(t) : NaN;
    }
    case SNPGPU_LD_R:
    case SNPGPU_LD_DPRIME: {                           // src/genLD.cpp:334-446
        const long hAA = 2 * n[8] + n[7] + n[5], hAB = n[3] + 2 * n[6] + n[7];
        const long hBA = n[1] + 2 * n[2] + n[5], hBB = 2 * n[0] + n[1] + n[3];
        double pAA, pAB, pBA, pBB;
        ld_haplo(hAA, hAB, hBA, hBB, 2 * n[4], pAA, pAB, pBA, pBB);
        const double pA = pAA + pAB, p_A = pAA + pBA, pB = pBA + pBB, p_B = pAB + pBB;
        const double D = pAA - pA * p_A;
        if (method == SNPGPU_LD_R) return D / sqrt(pA * p_A * pB * p_B);
        double den;
        if (D >= 0) { const double u = pA * p_B, v = pB * p_A; den = (v < u) ? v : u; }          // std::min
        else { const double u = -pA * p_A, v = -pB * p_B; den = (u < v) ? v : u; }                // std::max
        return D / den;
    }
    case SNPGPU_LD_CORR: {                             // src/genLD.cpp:449-506
        if (tot <= 0) return NaN;
        const long X = r1 + 2 * r2, XX = r1 + 4 * r2, Y = c1 + 2 * c2, YY = c1 + 4 * c2;
        const long XY = n[4] + 2 * n[5] + 2 * n[7] + 4 * n[8];
        const double d1 = XX - double(X) * X / tot, d2 = YY - double(Y) * Y / tot;
        const double v = d1 * d2;
        return v > 0 ? (XY - double(X) * Y / tot) / sqrt(v) : NaN;
    }
    case SNPGPU_LD_COV: {                              // src/genLD.cpp:509-525
        if (tot <= 1) return NaN;
        const long X = r1 + 2 * r2, Y = c1 + 2 * c2, XY = n[4] + 2 * n[5] + 2 * n[7] + 4 * n[8];
        return (XY - double(X) * Y / tot) / (tot - 1);
    }
    default: return NaN;
    }
}

}  // namespace snpgpu
