// IBD by maximum likelihood (snpgdsIBDMLE, method "EM"): the per-pair EM iteration of the reference's EMAlg
// (src/genIBD.cpp:582-656) and the log-likelihood sweep of EM_LogLik (:538-575), fp64 throughout.
//
// Mapping.  One sample pair per lane; the 64 lanes of a wave sweep the SNPs in lockstep, so the SNP index is wave-uniform and
// the per-SNP values derived from p (ibd_snp_t) are scalar loads shared by 64 pairs.  Each lane reads the 2-bit codes of its
// two samples from sample-major words (16 SNPs per 4-byte load).  A lane whose pair stops at the end of a sweep writes the
// pair's result and takes the next pair from a global queue (one vector atomic per wave and sweep), which it starts on the
// next sweep; the wave ends when the queue is empty and its last pair has stopped.
//
// Arithmetic.  PrIBDTable's (t0, t1, t2) for a usable SNP (both called, 0 < p < 1) is a pair-constant factor c times
//     hom/hom same  (x^2, x, 1)    c = x^2      x = q for genotype 0, p for genotype 2
//     hom/het       (2x, 1, 0)     c = p q x    x from the homozygote
//     het/het       (4pq, 1, 2)    c = p q
//     opposite hom  (1, 0, 0)      c = p^2 q^2
// The posteriors t_i k_i / sum do not depend on c; one reciprocal of s = a0 k0 + a1 k1 + a2 k2 serves both sums.  The
// log-likelihood sum of log(c s) is kept as a running product renormalised by exponent every 4 (EM) or 8 (log-likelihood
// sweep) SNPs and turned into a log once
// per sweep.  SNPs that are not usable are written as missing codes when the words are built, so they contribute nothing.
//
// Listed pairs (snpgdsIBDMLEPairs): the second half of this file maps one pair to a WAVE, see "one wave per pair" below.
#include "ibd_device.h"

namespace snpgpu {

namespace {

__device__ inline void row_of_pair(const int64_t *__restrict__ rowoff, int64_t n_rows, int64_t r0, int64_t idx, int diag,
                                   int64_t &i, int64_t &j)
{
    int64_t lo = 0, hi = n_rows;           // largest r with rowoff[r] <= idx
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowoff[mid] <= idx) lo = mid; else hi = mid;
    }
    i = r0 + lo;
    j = i + (diag ? 0 : 1) + (idx - rowoff[lo]);
}

// One sweep over the SNPs for one pair (codes from words ga / gb) at (k0, k1, k2): the posterior sums, the number of usable
// SNPs, and the log-likelihood as a product (times 2^ex).  Lanes without a pair sweep sample 0 and discard the result.
__device__ inline void em_sweep(const uint32_t *__restrict__ ga, const uint32_t *__restrict__ gb, int64_t nw,
                                const IbdSnp *__restrict__ snp, double k0, double k1, double k2, double &S0, double &S1,
                                int &nS, double &prod, int &ex)
{
    S0 = 0; S1 = 0; prod = 1; ex = 0; nS = 0;
    for (int64_t w = 0; w < nw; w++) {
        const uint32_t wa = ga[w], wb = gb[w];
        const IbdSnp *tab = snp + w * 16;
        // 4 SNPs per step: their 4 x 4 doubles of constants fit the scalar registers (with 8 per step, 54 SGPRs spilled to
        // VGPR lanes and the loop paid v_writelane / v_readlane for them)
#pragma unroll 1
        for (int h = 0; h < 16; h += 4) {
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const unsigned a = (wa >> (2 * (h + m))) & 3u, b = (wb >> (2 * (h + m))) & 3u;
                const bool use = (a != 3u) & (b != 3u);
                double c, a0, a1, a2;
                ibd_terms(a, b, tab[h + m], c, a0, a1, a2);
                const double m0 = a0 * k0, m1 = a1 * k1;
                double s = m0 + m1 + a2 * k2;
                s = use ? s : 1.0;
                const double r = recip(s);
                S0 = use ? fma(m0, r, S0) : S0;
                S1 = use ? fma(m1, r, S1) : S1;
                prod *= use ? c * s : 1.0;
                nS += use ? 1 : 0;
            }
            renorm(prod, ex);
        }
    }
}

// queue: [0] next pair, [1] useful lane-sweeps, [2] issued lane-sweeps; outputs per pair of the range
__global__ __launch_bounds__(256) void ibd_em_kernel(const uint32_t *__restrict__ gt, int64_t nw, const IbdSnp *__restrict__ snp,
                                                     const double *__restrict__ mom_k0, const double *__restrict__ mom_k1,
                                                     const int64_t *__restrict__ rowoff, int64_t n_rows, int64_t r0,
                                                     int64_t n_samp, int64_t n_pairs, int max_niter, double reltol,
                                                     unsigned long long *__restrict__ queue, double *__restrict__ ok0,
                                                     double *__restrict__ ok1, double *__restrict__ oll,
                                                     int32_t *__restrict__ onit)
{
    const int lane = threadIdx.x & 63;
    int64_t pair = -1, si = 0, sj = 0;
    double k0 = 0, k1 = 0, k2 = 0, old = 0, tol = 0;
    int it = 0;
    bool exhausted = false;
    unsigned long long useful = 0, issued = 0;
    while (true) {
        // refill the lanes without a pair from the queue
        const unsigned long long need = __ballot(pair < 0 && !exhausted);
        if (need) {
            const int leader = __ffsll((long long)need) - 1, cnt = __popcll(need);
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(queue, (unsigned long long)cnt);
            base = __shfl(base, leader);
            if (base + cnt >= (unsigned long long)n_pairs) exhausted = true;
            const int64_t idx = (int64_t)(base + __popcll(need & ((1ull << lane) - 1ull)));
            if (((need >> lane) & 1ull) && idx < n_pairs) {
                pair = idx;
                row_of_pair(rowoff, n_rows, r0, idx, 0, si, sj);
                const int64_t t = sj + si * (2 * n_samp - si - 1) / 2;
                // start values: Est_PLINK_Kinship, then each of k0, k1, k2 >= 0.005 and renormalised (:824-832)
                double a = mom_k0[t], b = mom_k1[t], c = 1 - a - b;
                if (a < 0.005) a = 0.005;
                if (b < 0.005) b = 0.005;
                if (c < 0.005) c = 0.005;
                const double s = a + b + c;
                k0 = a / s; k1 = b / s; k2 = 1 - k0 - k1;
                old = 0; it = 0;
            }
        }
        if (!__ballot(pair >= 0)) break;
        useful += (pair >= 0) ? 1 : 0;
        issued += 1;

        double S0, S1, prod;
        int nS, ex;
        em_sweep(gt + (pair >= 0 ? si : 0) * nw, gt + (pair >= 0 ? sj : 0) * nw, nw, snp, k0, k1, k2, S0, S1, nS, prod, ex);
        if (pair < 0) continue;
        const double L = log(prod) + ex * LN2;
        bool done = false;
        double fk0 = k0, fk1 = k1, fL = L;
        int fit = it;
        if (it == 0) {
            // ConvTol from the log-likelihood at the start values (:590-600)
            tol = isfinite(L) ? reltol * (fabs(L) + fabs(reltol)) : reltol;
            if (tol < 0) tol = 0;
            if (max_niter < 0) { done = true; fit = max_niter; fL = isfinite(L) ? L : 1e8; }
        }
        if (!done) {
            const double n0 = S0 / nS, n1 = S1 / nS;
            if (fabs(L - old) <= tol) {
                done = true;                                   // converged: the previous iterate, niter = iIter
            } else {
                old = L;
                k0 = n0; k1 = n1; k2 = 1 - n0 - n1;
                if (it >= max_niter) { done = true; fk0 = k0; fk1 = k1; fit = max_niter; }
                else it++;
            }
        }
        if (done) {
            ok0[pair] = fk0; ok1[pair] = fk1; oll[pair] = fL; onit[pair] = fit;
            pair = -1;
        }
    }
    atomicAdd(queue + 1, useful);                  // this lane's sweeps that advanced a pair
    if (lane == 0) atomicAdd(queue + 2, issued * 64ull);
}

// Log-likelihood sweep of NC parameter pairs per lane (EM_LogLik): NC = 6 applies coeff.correct's candidates (LOGLIK_ADJUST,
// in the reference's order) to the EM results of the pairs; NC = 1 evaluates one (k0, k1) per pair, from per-pair matrices or
// one global pair, into a full n x n matrix (Do_MLE_LogLik / _k01, diagonal included).
template <int NC>
__global__ __launch_bounds__(256) void ibd_loglik_kernel(const uint32_t *__restrict__ gt, int64_t nw,
                                                         const IbdSnp *__restrict__ snp, const int64_t *__restrict__ rowoff,
                                                         int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs, int diag,
                                                         const double *__restrict__ km0, const double *__restrict__ km1,
                                                         double ks0, double ks1, double *__restrict__ out,
                                                         double *__restrict__ pk0, double *__restrict__ pk1,
                                                         const double *__restrict__ pll)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < n_pairs;
    int64_t si = 0, sj = 0;
    if (live) row_of_pair(rowoff, n_rows, r0, idx, diag, si, sj);
    double kk0[NC], kk1[NC], kk2[NC];
    if constexpr (NC == 6) {
        const double c0[6] = {0, 0.25, 0, 0.5, 0.75, 1}, c1[6] = {0, 0.5, 1, 0.5, 0.25, 0};
        for (int c = 0; c < 6; c++) { kk0[c] = c0[c]; kk1[c] = c1[c]; kk2[c] = 1 - c0[c] - c1[c]; }
    } else {
        const double a = km0 ? (live ? km0[si * n_samp + sj] : 0) : ks0;
        const double b = km1 ? (live ? km1[si * n_samp + sj] : 0) : ks1;
        kk0[0] = a; kk1[0] = b; kk2[0] = 1 - a - b;
    }
    const uint32_t *ga = gt + si * nw, *gb = gt + sj * nw;
    double prod[NC];
    int ex[NC];
    bool bad[NC];
    for (int c = 0; c < NC; c++) { prod[c] = 1; ex[c] = 0; bad[c] = false; }
    for (int64_t w = 0; w < nw; w++) {
        const uint32_t wa = ga[w], wb = gb[w];
        const IbdSnp *tab = snp + w * 16;
#pragma unroll 1
        for (int h = 0; h < 16; h += 8) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const unsigned a = (wa >> (2 * (h + m))) & 3u, b = (wb >> (2 * (h + m))) & 3u;
                const bool use = (a != 3u) & (b != 3u);
                double cf, a0, a1, a2;
                ibd_terms(a, b, tab[h + m], cf, a0, a1, a2);
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const double s = a0 * kk0[c] + a1 * kk1[c] + a2 * kk2[c];
                    // sum <= 0 (or NaN) on a usable SNP: -Inf, as EM_LogLik's early return
                    bad[c] = bad[c] | (use & !(s > 0));
                    prod[c] *= (use & (s > 0)) ? cf * s : 1.0;
                }
            }
            for (int c = 0; c < NC; c++) renorm(prod[c], ex[c]);
        }
    }
    if (!live) return;
    double L[NC];
    for (int c = 0; c < NC; c++) L[c] = bad[c] ? -INFINITY : log(prod[c]) + ex[c] * LN2;
    if constexpr (NC == 6) {
        // LOGLIK_ADJUST in the reference's order: self, full sibs, offspring, half sibs, cousins, unrelated
        double best = pll[idx], b0 = pk0[idx], b1 = pk1[idx];
        for (int c = 0; c < 6; c++)
            if (isfinite(L[c]) && best < L[c]) { best = L[c]; b0 = kk0[c]; b1 = kk1[c]; }
        pk0[idx] = b0; pk1[idx] = b1;
    } else {
        out[si * n_samp + sj] = L[0];
        out[sj * n_samp + si] = L[0];
    }
}

// sample-major words: word w of sample s holds SNPs 16 w .. 16 w + 15 at bits 2 m; SNPs past n_snp or flagged unusable are 3
__global__ void ibd_words_kernel(const uint8_t *__restrict__ rows, int64_t rb, int64_t n_snp, int64_t n_samp,
                                 const uint8_t *__restrict__ usable, int64_t wpad, uint32_t *__restrict__ gt)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (s >= n_samp) return;
    uint32_t v = 0;
    for (int m = 0; m < 16; m++) {
        const int64_t l = 16 * w + m;
        unsigned code = 3u;
        if (l < n_snp && usable[l]) code = (rows[l * rb + (s >> 2)] >> (2 * (s & 3))) & 3u;
        v |= code << (2 * m);
    }
    gt[s * wpad + w] = v;
}

// per SNP: sum of the called genotypes and number of calls (InitAFreq's estimate, :1135-1160); one wave per SNP
__global__ void ibd_freq_kernel(const uint8_t *__restrict__ rows, int64_t rb, int64_t n_samp, double *__restrict__ af)
{
    const int64_t l = blockIdx.x;
    const uint8_t *r = rows + l * rb;
    int sum = 0, num = 0;
    for (int64_t s = threadIdx.x; s < n_samp; s += 64) {
        const unsigned g = (r[s >> 2] >> (2 * (s & 3))) & 3u;
        if (g < 3u) { sum += (int)g; num += 2; }
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); num += __shfl_xor(num, o); }
    if (threadIdx.x == 0) af[l] = num > 0 ? (double)sum / num : -1.0;
}

__global__ void ibd_snp_table_kernel(const double *__restrict__ af, int64_t n_snp, int64_t n_pad, IbdSnp *__restrict__ tab,
                                     uint8_t *__restrict__ usable)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= n_pad) return;
    const double p = l < n_snp ? af[l] : -1.0;
    const bool ok = (0 < p) && (p < 1);
    IbdSnp t;
    if (ok) { const double q = 1 - p; t.q = q; t.p = p; t.pq = p * q; t.pq4 = 4 * p * q; }
    else { t.q = 0.5; t.p = 0.5; t.pq = 0.25; t.pq4 = 1.0; }
    tab[l] = t;
    if (l < n_snp) usable[l] = ok ? 1 : 0;
}

// compact per-pair values (pairs i < j of rows [r0, r1)) -> full n x n, mirrored; the rows' diagonal entries are 0
__global__ void ibd_expand_kernel(const int64_t *__restrict__ rowoff, int64_t n_rows, int64_t r0, int64_t n_samp,
                                  int64_t n_pairs, const double *__restrict__ k0, const double *__restrict__ k1,
                                  const int32_t *__restrict__ nit, double *__restrict__ o0, double *__restrict__ o1,
                                  int32_t *__restrict__ on)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n_rows) {
        const int64_t d = (r0 + idx) * (n_samp + 1);
        o0[d] = 0; o1[d] = 0;
        if (on) on[d] = 0;
    }
    if (idx >= n_pairs) return;
    int64_t i, j;
    row_of_pair(rowoff, n_rows, r0, idx, 0, i, j);
    o0[i * n_samp + j] = o0[j * n_samp + i] = k0[idx];
    o1[i * n_samp + j] = o1[j * n_samp + i] = k1[idx];
    if (on) on[i * n_samp + j] = on[j * n_samp + i] = nit[idx];
}

// ---- one wave per pair (snpgpu_ibd_mle_pairs) ------------------------------------------------------------------------------------
// A short list of pairs leaves most lanes of the lane-per-pair kernel idle and every wave waiting for its slowest pair.  Here a
// wave owns one pair at a time and its 64 lanes split the SNPs: lane l sweeps the 16-SNP words w = 64 b + l of both samples
// (one coalesced 256-byte load per sample and step b).  Nothing is wave-uniform per SNP, so the constants are vector loads: p
// alone (8 bytes per SNP; q, pq and 4pq are three register operations, against 32 bytes of IbdSnp), stored transposed so that
// the 64 lanes' values of SNP m of their words are one 512-byte line: pt[(16 b + m) * 64 + l] = p of SNP 16 (64 b + l) + m.
// The words hold the samples' codes as they are; SNPs without 0 < p < 1 are masked by OR-ing um[w] (11 at their positions),
// while the start values' IBS counts use the unmasked words, as the IBS context of the matrix path counts every SNP.
// After each sweep S0, S1, the log-likelihood and the usable-SNP count are summed over the lanes by an xor butterfly
// (32, 16, .. 1): every lane ends with the same bits, so the stop decision is wave-uniform, and a pair's result depends on
// nothing but its own words.  When its pair stops, lane 0 takes the next one from the queue.
// this lane's share of one EM sweep; nb steps of 64 words
__device__ inline void em_sweep_lane(const uint32_t *__restrict__ ga, const uint32_t *__restrict__ gb,
                                     const uint32_t *__restrict__ um, const double *__restrict__ pt, int64_t nb, int lane,
                                     double k0, double k1, double k2, double &S0, double &S1, int &nS, double &L)
{
    double prod = 1;
    int ex = 0;
    S0 = 0; S1 = 0; nS = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int64_t w = b * 64 + lane;
        const uint32_t wa = ga[w] | um[w], wb = gb[w];
        const double *pp = pt + b * 1024 + lane;
#pragma unroll 1
        for (int h = 0; h < 16; h += 4) {
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const unsigned a = (wa >> (2 * (h + m))) & 3u, bb = (wb >> (2 * (h + m))) & 3u;
                const bool use = (a != 3u) & (bb != 3u);
                double c, a0, a1, a2;
                ibd_terms(a, bb, snp_of_p(pp[(h + m) * 64]), c, a0, a1, a2);
                const double m0 = a0 * k0, m1 = a1 * k1;
                double s = m0 + m1 + a2 * k2;
                s = use ? s : 1.0;
                const double r = recip(s);
                S0 = use ? fma(m0, r, S0) : S0;
                S1 = use ? fma(m1, r, S1) : S1;
                prod *= use ? c * s : 1.0;
                nS += use ? 1 : 0;
            }
            renorm(prod, ex);
        }
    }
    L = log(prod) + ex * LN2;
}

// queue: [0] next pair, [1] wave-sweeps (EM and candidate sweeps; the integer pre-sweep is not counted)
__global__ __launch_bounds__(256) void ibd_em_pairs_kernel(const uint32_t *__restrict__ gt, int64_t wpad,
                                                           const uint32_t *__restrict__ um, const double *__restrict__ pt,
                                                           const int32_t *__restrict__ slot1, const int32_t *__restrict__ slot2,
                                                           int64_t n_pairs, IbdE e, int constraint, int mode, int max_niter,
                                                           double reltol, int coeff_correct, unsigned long long *__restrict__ queue,
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

        // start values: the pair's IBS counts from the unmasked codes (exact), then Est_PLINK_Kinship
        double a, b;
        pair_mom_start(ga, gb, nb, lane, e, constraint, a, b);
        if (mode == 1) {
            if (lane == 0) {
                ok0[pair] = a; ok1[pair] = b;
                if (oll) oll[pair] = (double)NAN;
                if (onit) onit[pair] = 0;
            }
            continue;
        }
        double k0, k1;
        clamp_start(a, b, k0, k1);
        double k2 = 1 - k0 - k1, old = 0, tol = 0;
        double fk0, fk1, fL;
        int it = 0, fit;
        while (true) {                                        // the decisions of ibd_em_kernel, wave-uniform here
            double S0, S1, L;
            int nS;
            em_sweep_lane(ga, gb, um, pt, nb, lane, k0, k1, k2, S0, S1, nS, L);
            S0 = wave_sum(S0); S1 = wave_sum(S1); L = wave_sum(L); nS = wave_sum(nS);
            sweeps++;
            bool done = false;
            fk0 = k0; fk1 = k1; fL = L; fit = it;
            if (it == 0) {
                tol = isfinite(L) ? reltol * (fabs(L) + fabs(reltol)) : reltol;
                if (tol < 0) tol = 0;
                if (max_niter < 0) { done = true; fit = max_niter; fL = isfinite(L) ? L : 1e8; }
            }
            if (!done) {
                const double n0 = S0 / nS, n1 = S1 / nS;
                if (fabs(L - old) <= tol) {
                    done = true;
                } else {
                    old = L;
                    k0 = n0; k1 = n1; k2 = 1 - n0 - n1;
                    if (it >= max_niter) { done = true; fk0 = k0; fk1 = k1; fit = max_niter; }
                    else it++;
                }
            }
            if (done) break;
        }
        if (coeff_correct) {
            // LOGLIK_ADJUST: the six candidates in one more sweep, in the reference's order against the final log-likelihood
            const double c0k[6] = {0, 0.25, 0, 0.5, 0.75, 1}, c1k[6] = {0, 0.5, 1, 0.5, 0.25, 0};
            double prod[6];
            int ex[6];
            bool bad[6];
#pragma unroll
            for (int q = 0; q < 6; q++) { prod[q] = 1; ex[q] = 0; bad[q] = false; }
            for (int64_t bk = 0; bk < nb; bk++) {
                const int64_t w = bk * 64 + lane;
                const uint32_t wa = ga[w] | um[w], wb = gb[w];
                const double *pp = pt + bk * 1024 + lane;
#pragma unroll 1
                for (int h = 0; h < 16; h += 8) {
#pragma unroll
                    for (int m = 0; m < 8; m++) {
                        const unsigned ca = (wa >> (2 * (h + m))) & 3u, cb = (wb >> (2 * (h + m))) & 3u;
                        const bool use = (ca != 3u) & (cb != 3u);
                        double cf, a0, a1, a2;
                        ibd_terms(ca, cb, snp_of_p(pp[(h + m) * 64]), cf, a0, a1, a2);
#pragma unroll
                        for (int q = 0; q < 6; q++) {
                            const double sq = a0 * c0k[q] + a1 * c1k[q] + a2 * (1 - c0k[q] - c1k[q]);
                            bad[q] = bad[q] | (use & !(sq > 0));
                            prod[q] *= (use & (sq > 0)) ? cf * sq : 1.0;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 6; q++) renorm(prod[q], ex[q]);
                }
            }
            sweeps++;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const double Lq = wave_sum(log(prod[q]) + ex[q] * LN2);
                const bool any_bad = __ballot(bad[q]) != 0ull;
                if (!any_bad && isfinite(Lq) && fL < Lq) { fL = Lq; fk0 = c0k[q]; fk1 = c1k[q]; }
            }
        }
        if (lane == 0) {
            ok0[pair] = fk0; ok1[pair] = fk1;
            if (oll) oll[pair] = fL;
            if (onit) onit[pair] = fit;
        }
    }
    if (lane == 0) atomicAdd(queue + 1, sweeps);
}

// words of the listed samples only: word w of slot t holds the codes of sample list[t] as they are (3 past n_snp)
__global__ void ibd_words_listed_kernel(const uint8_t *__restrict__ rows, int64_t rb, int64_t n_snp,
                                        const int32_t *__restrict__ list, int64_t n_list, int64_t wpad, uint32_t *__restrict__ gt)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (t >= n_list) return;
    const int64_t s = list[t];
    uint32_t v = 0;
    for (int m = 0; m < 16; m++) {
        const int64_t l = 16 * w + m;
        unsigned code = 3u;
        if (l < n_snp) code = (rows[l * rb + (s >> 2)] >> (2 * (s & 3))) & 3u;
        v |= code << (2 * m);
    }
    gt[t * wpad + w] = v;
}

// per word: the transposed p of its 16 SNPs (0.5 where the SNP is not usable or past n_snp) and the mask of those SNPs
__global__ void ibd_pairs_table_kernel(const double *__restrict__ af, int64_t n_snp, int64_t wpad, double *__restrict__ pt,
                                       uint32_t *__restrict__ um)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= wpad) return;
    const int64_t b = w >> 6, lane = w & 63;
    uint32_t mask = 0;
    for (int m = 0; m < 16; m++) {
        const int64_t l = 16 * w + m;
        const double p = l < n_snp ? af[l] : -1.0;
        const bool ok = (0 < p) && (p < 1);
        pt[(b * 16 + m) * 64 + lane] = ok ? p : 0.5;
        if (!ok) mask |= 3u << (2 * m);
    }
    um[w] = mask;
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

size_t ibd_snp_bytes() { return sizeof(IbdSnp); }

int launch_ibd_freq(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, int64_t n_samp, double *af)
{
    if (n_snp <= 0) return 0;
    hipLaunchKernelGGL(ibd_freq_kernel, dim3((unsigned)n_snp), dim3(64), 0, st, rows, rb, n_samp, af);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ibd_prepare(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, int64_t n_samp, const double *af,
                       int64_t w4, void *tab, uint8_t *usable, uint32_t *gt)
{
    const int64_t n_pad = w4 * 64;
    hipLaunchKernelGGL(ibd_snp_table_kernel, dim3(grid_of(n_pad)), dim3(256), 0, st, af, n_snp, n_pad, (IbdSnp *)tab, usable);
    SNPGPU_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ibd_words_kernel, dim3(grid_of(n_samp), (unsigned)(w4 * 4)), dim3(256), 0, st, rows, rb, n_snp, n_samp,
                       (const uint8_t *)usable, w4 * 4, gt);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ibd_em(hipStream_t st, int n_waves, const uint32_t *gt, int64_t w4, const void *tab, const double *mom_k0,
                  const double *mom_k1, const int64_t *rowoff, int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs,
                  int max_niter, double reltol, unsigned long long *queue, double *k0, double *k1, double *loglik,
                  int32_t *niter)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(ibd_em_kernel, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, st, gt, w4 * 4, (const IbdSnp *)tab,
                       mom_k0, mom_k1, rowoff, n_rows, r0, n_samp, n_pairs, max_niter, reltol, queue, k0, k1, loglik, niter);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ibd_candidates(hipStream_t st, const uint32_t *gt, int64_t w4, const void *tab, const int64_t *rowoff,
                          int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs, const double *loglik, double *k0,
                          double *k1)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(ibd_loglik_kernel<6>, dim3(grid_of(n_pairs)), dim3(256), 0, st, gt, w4 * 4, (const IbdSnp *)tab, rowoff,
                       n_rows, r0, n_samp, n_pairs, 0, (const double *)nullptr, (const double *)nullptr, 0.0, 0.0,
                       (double *)nullptr, k0, k1, loglik);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ibd_loglik(hipStream_t st, const uint32_t *gt, int64_t w4, const void *tab, const int64_t *rowoff, int64_t n_rows,
                      int64_t n_samp, int64_t n_pairs, const double *km0, const double *km1, double ks0, double ks1,
                      double *out)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(ibd_loglik_kernel<1>, dim3(grid_of(n_pairs)), dim3(256), 0, st, gt, w4 * 4, (const IbdSnp *)tab, rowoff,
                       n_rows, (int64_t)0, n_samp, n_pairs, 1, km0, km1, ks0, ks1, out, (double *)nullptr, (double *)nullptr,
                       (const double *)nullptr);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// wpad: words per sample, a multiple of 64; pt: wpad * 16 doubles; um: wpad words; gt: n_list * wpad words
int launch_ibd_pairs_prepare(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, const double *af, const int32_t *list,
                             int64_t n_list, int64_t wpad, double *pt, uint32_t *um, uint32_t *gt)
{
    hipLaunchKernelGGL(ibd_pairs_table_kernel, dim3(grid_of(wpad)), dim3(256), 0, st, af, n_snp, wpad, pt, um);
    SNPGPU_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ibd_words_listed_kernel, dim3(grid_of(n_list), (unsigned)wpad), dim3(256), 0, st, rows, rb, n_snp, list,
                       n_list, wpad, gt);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// n_waves <= n_pairs; whole blocks of 4 waves (fewer than 4 waves: one smaller block), so never more waves than asked for
int launch_ibd_em_pairs(hipStream_t st, int n_waves, const uint32_t *gt, int64_t wpad, const uint32_t *um, const double *pt,
                        const int32_t *slot1, const int32_t *slot2, int64_t n_pairs, const double *e, int constraint, int mode,
                        int max_niter, double reltol, int coeff_correct, unsigned long long *queue, double *k0, double *k1,
                        double *loglik, int32_t *niter)
{
    if (n_pairs <= 0 || n_waves <= 0) return 0;
    const int per = std::min(n_waves, 4);
    const IbdE ee = {e[0], e[1], e[2], e[3], e[4]};
    hipLaunchKernelGGL(ibd_em_pairs_kernel, dim3((unsigned)(n_waves / per)), dim3(64 * per), 0, st, gt, wpad, um, pt, slot1, slot2,
                       n_pairs, ee, constraint, mode, max_niter, reltol, coeff_correct, queue, k0, k1, loglik, niter);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ibd_expand(hipStream_t st, const int64_t *rowoff, int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs,
                      const double *k0, const double *k1, const int32_t *niter, double *o0, double *o1, int32_t *on)
{
    const int64_t n = std::max(n_pairs, n_rows);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ibd_expand_kernel, dim3(grid_of(n)), dim3(256), 0, st, rowoff, n_rows, r0, n_samp, n_pairs, k0, k1,
                       niter, o0, o1, on);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
