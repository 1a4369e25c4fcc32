// IBD by maximum likelihood of listed pairs, the two methods beside "EM": the downhill simplex (the reference's Simplex /
// SimplexMin<double, 2> / NM_LogLik, src/genIBD.cpp:60-189 and :661-779) and Jacquard's nine condensed coefficients
// (PrIBDTabJacq / EM_Jacq_Alg, :864-1072).  Both use the one-wave-per-pair mapping of ibd_em_pairs_kernel (kernels_ibd.hip): a wave
// owns one pair at a time, lane l sweeps the 16-SNP words w = 64 b + l of both samples, the per-SNP constant is the transposed p
// table, SNPs without 0 < p < 1 are masked by um, and every per-sweep sum goes through the xor butterfly so that all lanes hold
// the same bits.  Every decision below is therefore wave-uniform, and a pair's result depends on its own words only.
//
// Downhill simplex.  A Nelder-Mead step is a chain of decisions that need 1, 2 or 4 values of the objective
//     f(k0, k1) = - sum over usable SNPs of log(d0 k0 + d1 k1 + t2),   d0 = t0 - t2, d1 = t1 - t2   (NM_Prepare, NM_LogLik)
// which is 1e30 outside {k0 >= 0, k1 >= 0, k0 + k1 <= 1} and where a usable SNP with d0 > 0 has a sum that is not > 0.  With
// (t0, t1, t2) = c (a0, a1, a2) of ibd_terms, d0 > 0 exactly for the classes with a2 = 0 (opposite homozygotes, hom/het), whose
// sum is c (a0 k0 + a1 k1): it is 0 exactly when the reference's is, so a point is penalised here when it is there.  One sweep
// evaluates the points the reference evaluates independently of each other (the three start vertices; the two shrunken vertices;
// the six LOGLIK_ADJUST candidates); reflection, expansion and contraction are one sweep each.  The geometry (trial point, psum,
// shrink, start simplex, convtol) is plain fp64 in the reference's order without contraction, redundantly on every lane, so the
// vertices are a function of the start vertices and the decision sequence alone.  The three vertices live in named registers
// behind selects: a runtime-indexed array would go to scratch.
//
// Jacquard.  PrIBDTabJacq's nine probabilities of codes (a, b) are a factor c times
//     (mm, mm)               c = q     (1, q, q, q^2, q, q^2, q, q^2, q^3)
//     (hom x, het)           c = p q   Pr3 = 1, Pr4 = 2x, Pr8 = x, Pr9 = 2 x^2
//     (het, hom x)           c = p q   Pr5 = 1, Pr6 = 2x, Pr8 = x, Pr9 = 2 x^2
//     (hom x_a, hom x_b)     c = p q   Pr2 = 1, Pr4 = x_b, Pr6 = x_a, Pr9 = p q          x_a != x_b
//     (het, het)             c = p q   Pr7 = 2, Pr8 = 1, Pr9 = 4 p q
// (x = q for genotype 0, p for genotype 2), so the table is NOT symmetric in the two samples: listing a pair as (j, i) exchanges
// D3 with D5 and D4 with D6.  (MM, MM): the reference's `case 2` / `case 2` entry has no `break` and falls through to `default`,
// which zeroes all nine; EM_Jacq_Alg then skips those SNPs.  That is reproduced: an SNP at which both samples are MM is not
// usable here.  The posteriors do not depend on c, one reciprocal serves the nine sums, and the log-likelihood is the running
// product of c s as in em_sweep_lane.  The stop rule is EMAlg's.
#include "ibd_device.h"

#include <cfloat>

namespace snpgpu {

namespace {

// one pair's words and the tables every sweep reads
struct PairWords {
    const uint32_t *ga, *gb, *um;
    const double *pt;
    int64_t nb;
    int lane;
};

constexpr double NM_PENALTY = 1e30;

// ---- the simplex geometry: fp64 in the reference's order, no contraction ------------------------------------------------------------
__device__ inline double nm_get(const double (&v)[3], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : v[2]; }
__device__ inline void nm_set(double (&v)[3], int i, double x)
{
    v[0] = i == 0 ? x : v[0];
    v[1] = i == 1 ? x : v[1];
    v[2] = i == 2 ? x : v[2];
}
__device__ inline double nm_max(double a, double b) { return a < b ? b : a; }            // std::max

__device__ inline bool nm_outside(double k0, double k1)
{
#pragma clang fp contract(off)
    return (k0 < 0) || (k1 < 0) || (k0 + k1 > 1);
}

// Simplex's three start vertices (:745-757); the second vertex's else branch has no "/ 2", the third's has
__device__ inline void nm_start_simplex(double k0, double k1, double (&px)[3], double (&py)[3])
{
#pragma clang fp contract(off)
    px[0] = k0; py[0] = k1;
    px[1] = k0;
    double f = (1 - k0) / 2;
    py[1] = (k1 <= f) ? (k1 + nm_max(k1, f - k1) / 2) : (k1 - nm_max(k1 - f, 1 - k0 - k1));
    py[2] = k1;
    f = (1 - k1) / 2;
    px[2] = (k0 <= f) ? (k0 + nm_max(k0, f - k0) / 2) : (k0 - nm_max(k0 - f, 1 - k1 - k0) / 2);
}

__device__ inline double nm_convtol(double reltol, double y0)
{
#pragma clang fp contract(off)
    double convtol = reltol * (fabs(y0) + fabs(reltol));
    if (convtol < DBL_EPSILON) convtol = DBL_EPSILON;
    return convtol;
}

__device__ inline void nm_psum(const double (&px)[3], const double (&py)[3], double &ps0, double &ps1)
{
#pragma clang fp contract(off)
    double sum = 0;
    sum += px[0]; sum += px[1]; sum += px[2];
    ps0 = sum;
    sum = 0;
    sum += py[0]; sum += py[1]; sum += py[2];
    ps1 = sum;
}

// Simplex_Point_Try's trial point (:67-70)
__device__ inline void nm_trial_point(const double (&px)[3], const double (&py)[3], double ps0, double ps1, int ihi, double fac,
                                      double &t0, double &t1)
{
#pragma clang fp contract(off)
    const double fac1 = (1.0 - fac) / 2, fac2 = fac1 - fac;
    t0 = ps0 * fac1 - nm_get(px, ihi) * fac2;
    t1 = ps1 * fac1 - nm_get(py, ihi) * fac2;
}

// the trial point replaces the high point (:76-81)
__device__ inline void nm_accept(double (&px)[3], double (&py)[3], double &ps0, double &ps1, int ihi, double t0, double t1)
{
#pragma clang fp contract(off)
    ps0 += t0 - nm_get(px, ihi);
    nm_set(px, ihi, t0);
    ps1 += t1 - nm_get(py, ihi);
    nm_set(py, ihi, t1);
}

__device__ inline double nm_half_way(double a, double b)
{
#pragma clang fp contract(off)
    return 0.5 * (a + b);
}

__device__ inline bool nm_converged(double yhi, double ylo, double convtol)
{
#pragma clang fp contract(off)
    return (yhi - ylo) <= convtol;
}

// ---- the objective ------------------------------------------------------------------------------------------------------------------
// this lane's share of one sweep at NP points: per point the log of the running product and whether a usable SNP with d0 > 0
// had a sum that is not > 0
template <int NP>
__device__ inline void nm_sweep_lane(const PairWords &A, const double (&k0)[NP], const double (&k1)[NP], double (&L)[NP],
                                     bool (&bad)[NP])
{
    double prod[NP];
    int ex[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) { prod[q] = 1; ex[q] = 0; bad[q] = false; }
    for (int64_t b = 0; b < A.nb; b++) {
        const int64_t w = b * 64 + A.lane;
        const uint32_t wa = A.ga[w] | A.um[w], wb = A.gb[w];
        const double *pp = A.pt + b * 1024 + A.lane;
#pragma unroll 1
        for (int h = 0; h < 16; h += 8) {
#pragma unroll
            for (int m = 0; m < 8; m += 2) {
                // two SNPs per step.  With one or two points their factors are multiplied first, which halves the dependent
                // chain on prod; with more points the points themselves are independent chains (and the registers are needed)
                double f[2][NP];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const unsigned ca = (wa >> (2 * (h + m + u))) & 3u, cb = (wb >> (2 * (h + m + u))) & 3u;
                    const bool use = (ca != 3u) & (cb != 3u);
                    double cf, a0, a1, a2;
                    ibd_terms(ca, cb, snp_of_p(pp[(h + m + u) * 64]), cf, a0, a1, a2);
                    const double d0 = a0 - a2, d1 = a1 - a2;
                    const bool d0pos = d0 > 0;
#pragma unroll
                    for (int q = 0; q < NP; q++) {
                        const double s = d0 * k0[q] + d1 * k1[q] + a2;
                        const bool pos = s > 0;
                        bad[q] = bad[q] | (use & !pos & d0pos);
                        f[u][q] = (use & pos) ? cf * s : 1.0;
                        if (NP > 2) prod[q] *= f[u][q];
                    }
                }
                if (NP <= 2) {
#pragma unroll
                    for (int q = 0; q < NP; q++) prod[q] *= f[0][q] * f[1][q];
                }
            }
#pragma unroll
            for (int q = 0; q < NP; q++) renorm(prod[q], ex[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < NP; q++) L[q] = log(prod[q]) + ex[q] * LN2;
}

// _optim at NP independent points in one sweep: y = -NM_LogLik, 1e30 where that is not finite.  fin: NM_LogLik is finite.
// A sweep all of whose points lie outside the triangle is not run (and not counted).
template <int NP>
__device__ inline void nm_eval(const PairWords &A, const double (&k0)[NP], const double (&k1)[NP], double (&y)[NP], bool (&fin)[NP],
                               unsigned long long &sweeps)
{
    bool out[NP], any_in = false;
#pragma unroll
    for (int q = 0; q < NP; q++) {
        out[q] = nm_outside(k0[q], k1[q]);
        any_in = any_in | !out[q];
        y[q] = NM_PENALTY;
        fin[q] = false;
    }
    if (!any_in) return;
    double L[NP];
    bool bad[NP];
    nm_sweep_lane<NP>(A, k0, k1, L, bad);
    sweeps++;
#pragma unroll
    for (int q = 0; q < NP; q++) {
        const double Lq = wave_sum(L[q]);
        const bool any_bad = __ballot(bad[q]) != 0ull;
        if (!out[q] && !any_bad && isfinite(Lq)) { y[q] = -Lq; fin[q] = true; }
    }
}

// queue: [0] next pair, [1] wave-sweeps (function-evaluation sweeps of one pair by one wave)
__global__ __launch_bounds__(256) void ibd_nm_pairs_kernel(const uint32_t *__restrict__ gt, int64_t wpad,
                                                           const uint32_t *__restrict__ um, const double *__restrict__ pt,
                                                           const int32_t *__restrict__ slot1, const int32_t *__restrict__ slot2,
                                                           int64_t n_pairs, IbdE e, int constraint, int max_niter, double reltol,
                                                           int coeff_correct, unsigned long long *__restrict__ queue,
                                                           double *__restrict__ ok0, double *__restrict__ ok1,
                                                           double *__restrict__ oll, int32_t *__restrict__ onit)
{
    const int lane = threadIdx.x & 63;
    const int64_t nb = wpad / 64;
    unsigned long long sweeps = 0;
    while (true) {
        const int64_t pair = take_pair(queue, lane);
        if (pair >= n_pairs) break;
        const uint32_t *ga = gt + (int64_t)slot1[pair] * wpad, *gb = gt + (int64_t)slot2[pair] * wpad;
        const PairWords A = {ga, gb, um, pt, nb, lane};

        double a, b, s0, s1;
        pair_mom_start(ga, gb, nb, lane, e, constraint, a, b);
        clamp_start(a, b, s0, s1);

        // SimplexMin<double, 2> (:97-189), statement for statement
        double px[3], py[3], y[3], ps0, ps1;
        bool fin3[3];
        nm_start_simplex(s0, s1, px, py);
        nm_eval<3>(A, px, py, y, fin3, sweeps);
        int nfunk = 2;
        const double convtol = nm_convtol(reltol, y[0]);
        nm_psum(px, py, ps0, ps1);
        int ilo, ihi, inhi;
        while (true) {
            ilo = 0;
            if (y[0] > y[1]) { inhi = 1; ihi = 0; } else { inhi = 0; ihi = 1; }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (y[i] <= nm_get(y, ilo)) ilo = i;
                if (y[i] > nm_get(y, ihi)) { inhi = ihi; ihi = i; }
                else if ((y[i] > nm_get(y, inhi)) && (i != ihi)) inhi = i;
            }
            if (nm_converged(nm_get(y, ihi), nm_get(y, ilo), convtol) || (nfunk >= max_niter)) break;
            nfunk += 2;
            // reflection, then expansion or one-dimensional contraction: one call site of the one-point sweep
            double fac = -1.0, ysave = 0;
            bool contraction = false, shrink = false;
#pragma unroll 1
            for (int step = 0; step < 2; step++) {
                double t0[1], t1[1], yt[1];
                bool ft[1];
                nm_trial_point(px, py, ps0, ps1, ihi, fac, t0[0], t1[0]);
                nm_eval<1>(A, t0, t1, yt, ft, sweeps);
                const double ytry = yt[0];
                if (ytry < nm_get(y, ihi)) {
                    nm_set(y, ihi, ytry);
                    nm_accept(px, py, ps0, ps1, ihi, t0[0], t1[0]);
                }
                if (step == 0) {
                    if (ytry <= nm_get(y, ilo)) {
                        fac = 2.0;
                    } else if (ytry >= nm_get(y, inhi)) {
                        ysave = nm_get(y, ihi);
                        fac = 0.5;
                        contraction = true;
                    } else {
                        --nfunk;
                        break;
                    }
                } else if (contraction && ytry >= ysave) {
                    shrink = true;
                }
            }
            if (shrink) {
                // contract around the lowest point: the two other vertices, evaluated in one sweep
                const double lx = nm_get(px, ilo), ly = nm_get(py, ilo);
                const int i0 = ilo == 0 ? 1 : 0, i1 = ilo == 2 ? 1 : 2;               // the vertices i != ilo in ascending order
                double sx[2], sy[2], ys[2];
                bool fs[2];
                sx[0] = nm_half_way(nm_get(px, i0), lx); sy[0] = nm_half_way(nm_get(py, i0), ly);
                sx[1] = nm_half_way(nm_get(px, i1), lx); sy[1] = nm_half_way(nm_get(py, i1), ly);
                nm_eval<2>(A, sx, sy, ys, fs, sweeps);
                nm_set(px, i0, sx[0]); nm_set(py, i0, sy[0]); nm_set(y, i0, ys[0]);
                nm_set(px, i1, sx[1]); nm_set(py, i1, sy[1]); nm_set(y, i1, ys[1]);
                nfunk += 2;
                nm_psum(px, py, ps0, ps1);
            }
        }
        double fk0 = nm_get(px, ilo), fk1 = nm_get(py, ilo), fL = -nm_get(y, ilo);
        if (coeff_correct) {
            // LOGLIK_ADJUST through NM_LogLik: the six candidates in one sweep, in the reference's order against -y[ilo]
            const double c0k[6] = {0, 0.25, 0, 0.5, 0.75, 1}, c1k[6] = {0, 0.5, 1, 0.5, 0.25, 0};
            double yc[6];
            bool fc[6];
            nm_eval<6>(A, c0k, c1k, yc, fc, sweeps);
#pragma unroll
            for (int q = 0; q < 6; q++)
                if (fc[q] && fL < -yc[q]) { fL = -yc[q]; fk0 = c0k[q]; fk1 = c1k[q]; }
        }
        if (lane == 0) {
            ok0[pair] = fk0; ok1[pair] = fk1;
            if (oll) oll[pair] = fL;
            if (onit) onit[pair] = nfunk;
        }
    }
    if (lane == 0) atomicAdd(queue + 1, sweeps);
}

// ---- Jacquard ------------------------------------------------------------------------------------------------------------------------
// PrIBDTabJacq of codes (a, b), neither missing and not both 2, at 0 < p < 1: factor c and the nine coefficients
__device__ inline void jacq_terms(unsigned a, unsigned b, double p, double &c, double (&t)[9])
{
    const double q = 1 - p, pq = p * q, pq4 = 4 * pq;
    const double xa = a == 0u ? q : p, xb = b == 0u ? q : p;
    const bool ahet = a == 1u, bhet = b == 1u;
    const bool S = (a == b) & !ahet, H = ahet & bhet, A = !ahet & bhet, B = ahet & !bhet, AB = A | B;
    const bool O = !(S | H | AB);
    const double x = ahet ? xb : xa;                       // the homozygote's allele frequency
    const double x2 = x + x, xx = x * x, xx2 = xx + xx, xxx = xx * x;
    // selects, not branches: the lanes of a wave hold different classes
    t[0] = S ? 1.0 : 0.0;
    t[1] = S ? x : O ? 1.0 : 0.0;
    t[2] = S ? x : A ? 1.0 : 0.0;
    t[3] = S ? xx : A ? x2 : O ? xb : 0.0;
    t[4] = S ? x : B ? 1.0 : 0.0;
    t[5] = S ? xx : B ? x2 : O ? xa : 0.0;
    t[6] = S ? x : H ? 2.0 : 0.0;
    t[7] = S ? xx : AB ? x : H ? 1.0 : 0.0;
    t[8] = S ? xxx : AB ? xx2 : O ? pq : pq4;
    c = S ? x : pq;
}

// this lane's share of one EM sweep at D[0..8]: the nine posterior sums, the usable count, the log-likelihood
__device__ inline void jacq_sweep_lane(const PairWords &A, const double (&D)[9], double (&S)[9], int &nS, double &L)
{
    double prod = 1;
    int ex = 0;
    nS = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) S[i] = 0;
    for (int64_t b = 0; b < A.nb; b++) {
        const int64_t w = b * 64 + A.lane;
        const uint32_t wa = A.ga[w] | A.um[w], wb = A.gb[w];
        const double *pp = A.pt + b * 1024 + A.lane;
#pragma unroll 1
        for (int h = 0; h < 16; h += 2) {
            // 2 SNPs per step (4 would not fit the 128 registers of four waves per SIMD without scratch), a renormalisation every 4
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const unsigned ca = (wa >> (2 * (h + m))) & 3u, cb = (wb >> (2 * (h + m))) & 3u;
                // (MM, MM) is not usable: the reference's table falls through to its default there
                const bool use = (ca != 3u) & (cb != 3u) & !((ca == 2u) & (cb == 2u));
                double c, t[9], mm[9];
                jacq_terms(ca, cb, pp[(h + m) * 64], c, t);
#pragma unroll
                for (int i = 0; i < 9; i++) mm[i] = t[i] * D[i];
                double s = mm[0] + mm[1] + mm[2] + mm[3] + mm[4] + mm[5] + mm[6] + mm[7] + mm[8];
                s = use ? s : 1.0;
                const double r = recip(s);
#pragma unroll
                for (int i = 0; i < 9; i++) S[i] = use ? fma(mm[i], r, S[i]) : S[i];
                prod *= use ? c * s : 1.0;
                nS += use ? 1 : 0;
            }
            if (h & 2) renorm(prod, ex);
        }
    }
    L = log(prod) + ex * LN2;
}

// queue as above; od: eight planes [8][n_pairs] (D1 .. D8).  Bounded to the 128 registers of four waves per SIMD, which the grid rule
// assumes: with 2 SNPs per step the sweep fits them without scratch (unbounded the compiler takes 165 and three waves fit)
__global__ __launch_bounds__(256, 4) void ibd_jacq_pairs_kernel(const uint32_t *__restrict__ gt, int64_t wpad,
                                                             const uint32_t *__restrict__ um, const double *__restrict__ pt,
                                                             const int32_t *__restrict__ slot1, const int32_t *__restrict__ slot2,
                                                             int64_t n_pairs, int max_niter, double reltol,
                                                             unsigned long long *__restrict__ queue, double *__restrict__ od,
                                                             double *__restrict__ oll, int32_t *__restrict__ onit)
{
    const int lane = threadIdx.x & 63;
    const int64_t nb = wpad / 64;
    unsigned long long sweeps = 0;
    while (true) {
        const int64_t pair = take_pair(queue, lane);
        if (pair >= n_pairs) break;
        const PairWords A = {gt + (int64_t)slot1[pair] * wpad, gt + (int64_t)slot2[pair] * wpad, um, pt, nb, lane};

        // IBD_Jacq_InitVal (:1074): D1 .. D8 = 0.01, D9 the left-to-right chain
        double D[9], fD[9], fL, old = 0, tol = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) D[i] = 0.01;
        D[8] = 1 - D[0] - D[1] - D[2] - D[3] - D[4] - D[5] - D[6] - D[7];
        int it = 0, fit;
        while (true) {                                        // the decisions of ibd_em_pairs_kernel
            double S[9], L;
            int nS;
            jacq_sweep_lane(A, D, S, nS, L);
#pragma unroll
            for (int i = 0; i < 9; i++) S[i] = wave_sum(S[i]);
            L = wave_sum(L); nS = wave_sum(nS);
            sweeps++;
            bool done = false;
#pragma unroll
            for (int i = 0; i < 9; i++) fD[i] = D[i];
            fL = L; fit = it;
            if (it == 0) {
                tol = isfinite(L) ? reltol * (fabs(L) + fabs(reltol)) : reltol;
                if (tol < 0) tol = 0;
                if (max_niter < 0) { done = true; fit = max_niter; fL = isfinite(L) ? L : 1e8; }
            }
            if (!done) {
                if (fabs(L - old) <= tol) {
                    done = true;                               // converged: the previous iterate, niter = iIter
                } else {
                    old = L;
#pragma unroll
                    for (int i = 0; i < 9; i++) D[i] = S[i] / nS;
                    if (it >= max_niter) {
                        done = true; fit = max_niter;
#pragma unroll
                        for (int i = 0; i < 9; i++) fD[i] = D[i];
                    } else {
                        it++;
                    }
                }
            }
            if (done) break;
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) od[(int64_t)i * n_pairs + pair] = fD[i];
            if (oll) oll[pair] = fL;
            if (onit) onit[pair] = fit;
        }
    }
    if (lane == 0) atomicAdd(queue + 1, sweeps);
}

inline void waves_to_grid(int n_waves, dim3 &grid, dim3 &block)
{
    const int per = std::min(n_waves, 4);
    grid = dim3((unsigned)(n_waves / per));
    block = dim3(64 * per);
}

}  // namespace

// n_waves <= n_pairs; whole blocks of 4 waves (fewer than 4 waves: one smaller block), as launch_ibd_em_pairs
int launch_ibd_nm_pairs(hipStream_t st, int n_waves, const uint32_t *gt, int64_t wpad, const uint32_t *um, const double *pt,
                        const int32_t *slot1, const int32_t *slot2, int64_t n_pairs, const double *e, int constraint, int max_niter,
                        double reltol, int coeff_correct, unsigned long long *queue, double *k0, double *k1, double *loglik,
                        int32_t *niter)
{
    if (n_pairs <= 0 || n_waves <= 0) return 0;
    dim3 grid, block;
    waves_to_grid(n_waves, grid, block);
    const IbdE ee = {e[0], e[1], e[2], e[3], e[4]};
    hipLaunchKernelGGL(ibd_nm_pairs_kernel, grid, block, 0, st, gt, wpad, um, pt, slot1, slot2, n_pairs, ee, constraint, max_niter,
                       reltol, coeff_correct, queue, k0, k1, loglik, niter);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ibd_jacq_pairs(hipStream_t st, int n_waves, const uint32_t *gt, int64_t wpad, const uint32_t *um, const double *pt,
                          const int32_t *slot1, const int32_t *slot2, int64_t n_pairs, int max_niter, double reltol,
                          unsigned long long *queue, double *d, double *loglik, int32_t *niter)
{
    if (n_pairs <= 0 || n_waves <= 0) return 0;
    dim3 grid, block;
    waves_to_grid(n_waves, grid, block);
    hipLaunchKernelGGL(ibd_jacq_pairs_kernel, grid, block, 0, st, gt, wpad, um, pt, slot1, slot2, n_pairs, max_niter, reltol, queue,
                       d, loglik, niter);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
