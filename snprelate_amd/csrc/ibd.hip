// C ABI of libsnpgpu: IBD coefficients by maximum likelihood (snpgdsIBDMLE, method "EM") and the log-likelihood of given
// coefficients (snpgdsIBDMLELogLik), on resident 2-bit rows.  Kernels: kernels_ibd.hip.
//
// gnrIBD_MLE (src/genIBD.cpp:1465-1548) step by step:
//   InitAFreq (:1122-1165)             caller's frequencies (non-finite -> -1) or sum / 2n over the calls (ibd_freq_kernel)
//   Init_EPrIBD_IBS(afreq, , false)    E[IBS | IBD] from plain monomials over the SNPs with 0 <= p <= 1 (host, SNP order)
//   Est_PLINK_Kinship(.., false)       the IBS counters of an SNPGPU_IBS context + launch_fin_mom with constraint 0
//   EMAlg + LOGLIK_ADJUST              ibd_em_kernel, then ibd_loglik_kernel<6> when coeff_correct
// Output: full n x n k0 / k1 / niter, 0 on the diagonal.
//
// snpgpu_ibd_mle_pairs does the same for a list of pairs without any n x n object: only the listed samples are transposed to
// words, and ibd_em_pairs_kernel (one wave per pair) counts the IBS states, applies Est_PLINK_Kinship, runs the EM and the
// candidates, and reports the log-likelihood after LOGLIK_ADJUST (gnrPairIBD's third output).  Its mode 2 runs the downhill simplex
// (ibd_nm_pairs_kernel) and snpgpu_ibd_jacquard_pairs Jacquard's nine coefficients (ibd_jacq_pairs_kernel) on the same words and
// tables with the same grid rule; both kernels are in kernels_ibd_methods.hip.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_util.h"

namespace snpgpu {
size_t ibd_snp_bytes();
int launch_ibd_freq(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, int64_t n_samp, double *af);
int launch_ibd_prepare(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, int64_t n_samp, const double *af,
                       int64_t w4, void *tab, uint8_t *usable, uint32_t *gt);
int launch_ibd_em(hipStream_t st, int n_waves, const uint32_t *gt, int64_t w4, const void *tab, const double *mom_k0,
                  const double *mom_k1, const int64_t *rowoff, int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs,
                  int max_niter, double reltol, unsigned long long *queue, double *k0, double *k1, double *loglik,
                  int32_t *niter);
int launch_ibd_candidates(hipStream_t st, const uint32_t *gt, int64_t w4, const void *tab, const int64_t *rowoff,
                          int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs, const double *loglik, double *k0,
                          double *k1);
int launch_ibd_loglik(hipStream_t st, const uint32_t *gt, int64_t w4, const void *tab, const int64_t *rowoff, int64_t n_rows,
                      int64_t n_samp, int64_t n_pairs, const double *km0, const double *km1, double ks0, double ks1,
                      double *out);
int launch_ibd_pairs_prepare(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, const double *af, const int32_t *list,
                             int64_t n_list, int64_t wpad, double *pt, uint32_t *um, uint32_t *gt);
int launch_ibd_em_pairs(hipStream_t st, int n_waves, const uint32_t *gt, int64_t wpad, const uint32_t *um, const double *pt,
                        const int32_t *slot1, const int32_t *slot2, int64_t n_pairs, const double *e, int constraint, int mode,
                        int max_niter, double reltol, int coeff_correct, unsigned long long *queue, double *k0, double *k1,
                        double *loglik, int32_t *niter);
int launch_ibd_expand(hipStream_t st, const int64_t *rowoff, int64_t n_rows, int64_t r0, int64_t n_samp, int64_t n_pairs,
                      const double *k0, const double *k1, const int32_t *niter, double *o0, double *o1, int32_t *on);
int launch_ibd_nm_pairs(hipStream_t st, int n_waves, const uint32_t *gt, int64_t wpad, const uint32_t *um, const double *pt,
                        const int32_t *slot1, const int32_t *slot2, int64_t n_pairs, const double *e, int constraint, int max_niter,
                        double reltol, int coeff_correct, unsigned long long *queue, double *k0, double *k1, double *loglik,
                        int32_t *niter);
int launch_ibd_jacq_pairs(hipStream_t st, int n_waves, const uint32_t *gt, int64_t wpad, const uint32_t *um, const double *pt,
                          const int32_t *slot1, const int32_t *slot2, int64_t n_pairs, int max_niter, double reltol,
                          unsigned long long *queue, double *d, double *loglik, int32_t *niter);
}  // namespace snpgpu

using namespace snpgpu;

namespace {

thread_local double g_stats[4] = {0, 0, 0, 0};   // EM kernel ms, all kernels ms, useful / issued lane-sweeps
thread_local double g_pair_stats[4] = {0, 0, 0, 0};   // the last listed-pairs call: its kernel's ms, all kernels ms, wave-sweeps, pairs

constexpr GenoLimits IBD_GENO = {2, NO_LIMIT, NO_LIMIT, true, "at least two samples are needed"};
enum { T_EM = 0, T_REST = 1 };   // snpgpu_ibd_mle's EventLog: the EM kernel; candidates and expansion, back to back with it

// the genotype words and per-SNP tables both sweeps read, and the frequencies of InitAFreq
struct Prep {
    int64_t n_snp = 0, n_samp = 0, rb = 0, w4 = 0;
    const uint8_t *rows = nullptr;     // device
    DevBuf *gt = nullptr, *tab = nullptr;
    std::vector<double> af;            // MLEAlleleFreq (host)
};

// the rows in device memory and InitAFreq's frequencies, on the device (*daf) and, once the stream is synchronised, in P.af
int rows_and_freq(CallStream &st, DevArena &bufs, const void *geno, int64_t n_snp, int64_t n_samp, int mem,
                  const double *allele_freq, Prep &P, DevBuf *&daf)
{
    int rc = 0;
    P.n_snp = n_snp; P.n_samp = n_samp; P.rb = (n_samp + 3) / 4;
    P.w4 = (n_snp + 63) / 64;
    const size_t row_bytes = (size_t)n_snp * (size_t)P.rb;
    if (mem == SNPGPU_HOST) {
        DevBuf *r = bufs.get(row_bytes, rc);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(r->p, geno, row_bytes, hipMemcpyHostToDevice, st.s));
        P.rows = (const uint8_t *)r->p;
    } else {
        P.rows = (const uint8_t *)geno;
    }
    daf = bufs.get(sizeof(double) * n_snp, rc);
    if (rc) return 1;
    P.af.assign((size_t)n_snp, -1.0);
    if (allele_freq) {
        for (int64_t l = 0; l < n_snp; l++)
            if (std::isfinite(allele_freq[l])) P.af[l] = allele_freq[l];
        SNPGPU_HIP_CHECK(hipMemcpyAsync(daf->p, P.af.data(), sizeof(double) * n_snp, hipMemcpyHostToDevice, st.s));
    } else {
        if (launch_ibd_freq(st.s, P.rows, P.rb, n_snp, n_samp, (double *)daf->p)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(P.af.data(), daf->p, sizeof(double) * n_snp, hipMemcpyDeviceToHost, st.s));
    }
    return 0;
}

int prepare(CallStream &st, DevArena &bufs, const void *geno, int64_t n_snp, int64_t n_samp, int mem,
            const double *allele_freq, Prep &P)
{
    int rc = 0;
    DevBuf *daf = nullptr;
    if (rows_and_freq(st, bufs, geno, n_snp, n_samp, mem, allele_freq, P, daf)) return 1;
    DevBuf *usable = bufs.get((size_t)n_snp, rc);
    P.tab = bufs.get(ibd_snp_bytes() * (size_t)P.w4 * 64, rc);
    P.gt = bufs.get((size_t)n_samp * (size_t)P.w4 * 16, rc);
    if (rc) return 1;
    if (launch_ibd_prepare(st.s, P.rows, P.rb, n_snp, n_samp, (const double *)daf->p, P.w4, P.tab->p,
                           (uint8_t *)usable->p, (uint32_t *)P.gt->p))
        return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    return 0;
}

// Init_EPrIBD_IBS(afreq, NULL, false), src/genIBD.cpp:253-338: plain monomials, SNPs with a finite p in [0, 1]
void e_prib(const std::vector<double> &af, double e[5])
{
    double e00 = 0, e01 = 0, e02 = 0, e11 = 0, e12 = 0;
    long n_valid = 0;
    for (const double p : af) {
        if (!(p >= 0 && p <= 1)) continue;
        const double q = 1 - p;
        e00 += 2 * p * p * q * q;
        e01 += 4 * p * p * p * q + 4 * p * q * q * q;
        e02 += q * q * q * q + p * p * p * p + 4 * p * p * q * q;
        e11 += 2 * p * p * q + 2 * p * q * q;
        e12 += p * p * p + q * q * q + p * p * q + p * q * q;
        n_valid++;
    }
    e[0] = e00 / n_valid; e[1] = e01 / n_valid; e[2] = e02 / n_valid; e[3] = e11 / n_valid; e[4] = e12 / n_valid;
}

// rowoff[k] = index of the first pair of row r0 + k (pairs i < j, or i <= j with the diagonal)
std::vector<int64_t> row_offsets(int64_t n, int64_t r0, int64_t r1, bool diag)
{
    std::vector<int64_t> off((size_t)(r1 - r0 + 1), 0);
    for (int64_t r = r0; r < r1; r++) off[(size_t)(r - r0 + 1)] = off[(size_t)(r - r0)] + (n - r - (diag ? 0 : 1));
    return off;
}

// the argument checks every listed-pairs call makes before a device is touched, after its own NULL checks
int check_pairs(const char *fn, const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int64_t n_snp, int64_t n_samp, int out_mem)
{
    if (!idx1 || !idx2) return fail(fn, "idx1 / idx2 is NULL");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (int64_t t = 0; t < n_pairs; t++)
        for (const int32_t v : {idx1[t], idx2[t]})
            if (v < 0 || v >= n_samp)
                return fail(fn, "sample index " + std::to_string(v) + " of pair " + std::to_string(t) + " is out of range (0 ... " +
                                    std::to_string(n_samp - 1) + ")");
    if (n_snp > int64_t(65535) * 16) return fail(fn, "invalid number of SNPs: too many SNPs (<= 1 048 560)");    // grid.y = words per sample
    return 0;
}

enum { K_EM = 0, K_NM = 1, K_JACQ = 2 };   // the kernel of a listed-pairs call

// The listed-pairs call after its checks: words of the distinct listed samples, the p table, then one wave per pair in `kernel`.
// o0 / o1: k0 / k1 [n_pairs], or for K_JACQ o0 = the eight planes [8][n_pairs] and o1 unused.
int run_pairs(const char *fn, const void *geno, int64_t n_snp, int64_t n_samp, int mem, const double *allele_freq, const int32_t *idx1,
              const int32_t *idx2, int64_t n_pairs, int kernel, int mode, int kinship_constraint, int max_niter, double reltol,
              int coeff_correct, double *k0, double *k1, double *loglik, int32_t *niter, double *afreq_out, int out_mem, int device)
{
    for (double &s : g_pair_stats) s = 0;

    // the distinct listed samples in ascending order, and each pair's two slots among them
    std::vector<int32_t> list(idx1, idx1 + n_pairs);
    list.insert(list.end(), idx2, idx2 + n_pairs);
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    std::vector<int32_t> slots((size_t)(2 * n_pairs));
    for (int64_t t = 0; t < n_pairs; t++) {
        slots[(size_t)t] = (int32_t)(std::lower_bound(list.begin(), list.end(), idx1[t]) - list.begin());
        slots[(size_t)(n_pairs + t)] = (int32_t)(std::lower_bound(list.begin(), list.end(), idx2[t]) - list.begin());
    }
    const int64_t n_list = (int64_t)list.size(), wpad = (n_snp + 1023) / 1024 * 64;

    Call c;
    if (c.open(fn, device, true)) return 1;
    CallStream &st = c.st;
    DevBuf *daf = nullptr;
    Prep P;
    if (rows_and_freq(st, c.bufs, geno, n_snp, n_samp, mem, allele_freq, P, daf)) return 1;
    int rc = 0;
    DevBuf *dlist = c.bufs.get(sizeof(int32_t) * list.size(), rc), *dslot = c.bufs.get(sizeof(int32_t) * slots.size(), rc);
    DevBuf *pt = c.bufs.get(sizeof(double) * (size_t)wpad * 16, rc), *um = c.bufs.get(sizeof(uint32_t) * (size_t)wpad, rc);
    DevBuf *gt = c.bufs.get(sizeof(uint32_t) * (size_t)n_list * (size_t)wpad, rc);
    DevBuf *queue = c.bufs.get(2 * sizeof(unsigned long long), rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dlist->p, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, st.s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dslot->p, slots.data(), sizeof(int32_t) * slots.size(), hipMemcpyHostToDevice, st.s));
    SNPGPU_HIP_CHECK(hipMemsetAsync(queue->p, 0, 2 * sizeof(unsigned long long), st.s));
    if (c.log.begin(T_REST, st.s)) return 1;
    if (launch_ibd_pairs_prepare(st.s, P.rows, P.rb, n_snp, (const double *)daf->p, (const int32_t *)dlist->p, n_list, wpad,
                                 (double *)pt->p, (uint32_t *)um->p, (uint32_t *)gt->p))
        return 1;
    if (c.log.end(st.s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));          // P.af is complete
    if (afreq_out) std::copy(P.af.begin(), P.af.end(), afreq_out);
    double e[5];
    e_prib(P.af, e);

    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const int n_waves = (int)std::min<int64_t>(n_pairs, (int64_t)cus * 16);

    HostOut o0, o1, ol, on;
    if (o0.open(c.bufs, k0, sizeof(double) * n_pairs * (kernel == K_JACQ ? 8 : 1), out_mem, false, st.s) ||
        (kernel != K_JACQ && o1.open(c.bufs, k1, sizeof(double) * n_pairs, out_mem, false, st.s)) ||
        ol.open(c.bufs, loglik, sizeof(double) * n_pairs, out_mem, false, st.s) ||
        on.open(c.bufs, niter, sizeof(int32_t) * n_pairs, out_mem, false, st.s))
        return 1;
    if (c.log.begin(T_EM, st.s)) return 1;
    const uint32_t *dgt = (const uint32_t *)gt->p, *dum = (const uint32_t *)um->p;
    const int32_t *s1 = (const int32_t *)dslot->p, *s2 = s1 + n_pairs;
    unsigned long long *dq = (unsigned long long *)queue->p;
    if (kernel == K_EM)
        rc = launch_ibd_em_pairs(st.s, n_waves, dgt, wpad, dum, (const double *)pt->p, s1, s2, n_pairs, e, kinship_constraint ? 1 : 0,
                                 mode, max_niter, reltol, coeff_correct ? 1 : 0, dq, (double *)o0.dev, (double *)o1.dev,
                                 (double *)ol.dev, (int32_t *)on.dev);
    else if (kernel == K_NM)
        rc = launch_ibd_nm_pairs(st.s, n_waves, dgt, wpad, dum, (const double *)pt->p, s1, s2, n_pairs, e, kinship_constraint ? 1 : 0,
                                 max_niter, reltol, coeff_correct ? 1 : 0, dq, (double *)o0.dev, (double *)o1.dev, (double *)ol.dev,
                                 (int32_t *)on.dev);
    else
        rc = launch_ibd_jacq_pairs(st.s, n_waves, dgt, wpad, dum, (const double *)pt->p, s1, s2, n_pairs, max_niter, reltol, dq,
                                   (double *)o0.dev, (double *)ol.dev, (int32_t *)on.dev);
    if (rc) return 1;
    if (c.log.end(st.s)) return 1;
    if (o0.close(st.s) || (kernel != K_JACQ && o1.close(st.s)) || ol.close(st.s) || on.close(st.s)) return 1;
    unsigned long long q[2] = {0, 0};
    SNPGPU_HIP_CHECK(hipMemcpyAsync(q, queue->p, sizeof(q), hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    double ms_rest = 0;
    if (c.log.sum_ms(T_EM, &g_pair_stats[0]) || c.log.sum_ms(T_REST, &ms_rest)) return 1;
    g_pair_stats[1] = g_pair_stats[0] + ms_rest; g_pair_stats[2] = (double)q[1]; g_pair_stats[3] = (double)n_pairs;
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_ibd_mle(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                   int max_niter, double reltol, int coeff_correct, int64_t row_begin, int64_t row_end, double *k0, double *k1,
                   int32_t *niter, double *afreq_out, int out_mem, int device)
{
    const char *fn = "snpgpu_ibd_mle";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, IBD_GENO)) return 1;
    if (!k0 || !k1) { set_error("snpgpu_ibd_mle: k0 / k1 is NULL"); return 1; }
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) { set_error("snpgpu_ibd_mle: invalid out_mem"); return 1; }
    int64_t r0 = row_begin, r1 = row_end;
    const bool whole = (r0 == 0 && r1 == 0) || (r0 == 0 && r1 == n_samp);
    if (r0 == 0 && r1 == 0) r1 = n_samp;
    if (r0 < 0 || r1 > n_samp || r0 >= r1) { set_error("snpgpu_ibd_mle: invalid row range"); return 1; }
    for (double &s : g_stats) s = 0;

    Call c;
    if (c.open(fn, device, true)) return 1;
    CallStream &st = c.st;
    DevArena &bufs = c.bufs;
    Prep P;
    if (prepare(st, bufs, geno, n_snp, n_samp, mem, allele_freq, P)) return 1;
    if (afreq_out) std::copy(P.af.begin(), P.af.end(), afreq_out);

    double e[5];
    e_prib(P.af, e);

    // PLINK start values on the IBS counters (Est_PLINK_Kinship with constraint = false, :823)
    int rc = 0;
    const size_t tri = (size_t)n_samp * (size_t)(n_samp + 1) / 2;
    DevBuf *mk0 = bufs.get(sizeof(double) * tri, rc), *mk1 = bufs.get(sizeof(double) * tri, rc);
    if (rc) return 1;
    {
        snpgpu_opts o{};
        o.device = device;
        o.max_block_snps = 32768;
        snpgpu_ctx *c = nullptr;
        if (snpgpu_create(SNPGPU_IBS, n_samp, &o, &c)) return 1;
        for (int64_t i0 = 0; i0 < n_snp && !rc; i0 += 32768)
            rc = snpgpu_feed(c, P.rows + (size_t)i0 * P.rb, std::min<int64_t>(32768, n_snp - i0), SNPGPU_GENO_PACKED2,
                             SNPGPU_DEVICE);
        if (!rc) rc = snpgpu_ibd_mom(c, e, 0, (double *)mk0->p, (double *)mk1->p, 1, SNPGPU_DEVICE);
        if (!rc) rc = snpgpu_sync(c);
        snpgpu_destroy(c);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipSetDevice(device));
    }

    const std::vector<int64_t> off = row_offsets(n_samp, r0, r1, false);
    const int64_t n_rows = r1 - r0, n_pairs = off.back();
    DevBuf *drow = bufs.get(sizeof(int64_t) * off.size(), rc), *queue = bufs.get(3 * sizeof(unsigned long long), rc);
    DevBuf *pk0 = bufs.get(sizeof(double) * n_pairs, rc), *pk1 = bufs.get(sizeof(double) * n_pairs, rc);
    DevBuf *pl = bufs.get(sizeof(double) * n_pairs, rc), *pn = bufs.get(sizeof(int32_t) * n_pairs, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(drow->p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, st.s));
    SNPGPU_HIP_CHECK(hipMemsetAsync(queue->p, 0, 3 * sizeof(unsigned long long), st.s));

    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const int64_t want = (n_pairs + 63) / 64;
    const int n_waves = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * 16));

    if (c.log.begin(T_EM, st.s)) return 1;
    if (launch_ibd_em(st.s, n_waves, (const uint32_t *)P.gt->p, P.w4, P.tab->p, (const double *)mk0->p,
                      (const double *)mk1->p, (const int64_t *)drow->p, n_rows, r0, n_samp, n_pairs, max_niter, reltol,
                      (unsigned long long *)queue->p, (double *)pk0->p, (double *)pk1->p, (double *)pl->p,
                      (int32_t *)pn->p))
        return 1;
    if (c.log.end(st.s) || c.log.begin(T_REST, st.s)) return 1;
    if (coeff_correct &&
        launch_ibd_candidates(st.s, (const uint32_t *)P.gt->p, P.w4, P.tab->p, (const int64_t *)drow->p, n_rows, r0, n_samp,
                              n_pairs, (const double *)pl->p, (double *)pk0->p, (double *)pk1->p))
        return 1;

    const size_t nn = (size_t)n_samp * (size_t)n_samp;
    HostOut o0, o1, on;
    if (o0.open(bufs, k0, nn * sizeof(double), out_mem, !whole, st.s) ||
        o1.open(bufs, k1, nn * sizeof(double), out_mem, !whole, st.s) ||
        on.open(bufs, niter, nn * sizeof(int32_t), out_mem, !whole, st.s))
        return 1;
    if (launch_ibd_expand(st.s, (const int64_t *)drow->p, n_rows, r0, n_samp, n_pairs, (const double *)pk0->p,
                          (const double *)pk1->p, (const int32_t *)pn->p, (double *)o0.dev, (double *)o1.dev,
                          (int32_t *)on.dev))
        return 1;
    if (c.log.end(st.s)) return 1;
    if (o0.close(st.s) || o1.close(st.s) || on.close(st.s)) return 1;
    unsigned long long q[3] = {0, 0, 0};
    SNPGPU_HIP_CHECK(hipMemcpyAsync(q, queue->p, sizeof(q), hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    double ms_rest = 0;
    if (c.log.sum_ms(T_EM, &g_stats[0]) || c.log.sum_ms(T_REST, &ms_rest)) return 1;
    g_stats[1] = g_stats[0] + ms_rest; g_stats[2] = (double)q[1]; g_stats[3] = (double)q[2];
    return 0;
}

int snpgpu_ibd_mle_pairs(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                         const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int mode, int kinship_constraint, int max_niter,
                         double reltol, int coeff_correct, double *k0, double *k1, double *loglik, int32_t *niter,
                         double *afreq_out, int out_mem, int device)
{
    const char *fn = "snpgpu_ibd_mle_pairs";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, IBD_GENO)) return 1;
    if (n_pairs < 1) return fail(fn, "no pair is listed (n_pairs < 1)");
    if (!k0 || !k1) return fail(fn, "k0 / k1 is NULL");
    if (mode != 0 && mode != 1 && mode != 2)
        return fail(fn, "invalid mode " + std::to_string(mode) + " (0 = EM, 1 = start values, 2 = downhill simplex)");
    if (check_pairs(fn, idx1, idx2, n_pairs, n_snp, n_samp, out_mem)) return 1;
    return run_pairs(fn, geno, n_snp, n_samp, mem, allele_freq, idx1, idx2, n_pairs, mode == 2 ? K_NM : K_EM, mode,
                     kinship_constraint, max_niter, reltol, coeff_correct, k0, k1, loglik, niter, afreq_out, out_mem, device);
}

int snpgpu_ibd_jacquard_pairs(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                              const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int max_niter, double reltol, double *d,
                              double *loglik, int32_t *niter, double *afreq_out, int out_mem, int device)
{
    const char *fn = "snpgpu_ibd_jacquard_pairs";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, IBD_GENO)) return 1;
    if (n_pairs < 1) return fail(fn, "no pair is listed (n_pairs < 1)");
    if (!d) return fail(fn, "d is NULL");
    if (check_pairs(fn, idx1, idx2, n_pairs, n_snp, n_samp, out_mem)) return 1;
    return run_pairs(fn, geno, n_snp, n_samp, mem, allele_freq, idx1, idx2, n_pairs, K_JACQ, 0, 0, max_niter, reltol, 0, d, nullptr,
                     loglik, niter, afreq_out, out_mem, device);
}

int snpgpu_ibd_mle_pairs_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_ibd_mle_pairs_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 4; k++) stats[k] = g_pair_stats[k];
    return 0;
}

int snpgpu_ibd_loglik(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                      const double *k0, const double *k1, double k0_all, double k1_all, double *out, double *afreq_out,
                      int out_mem, int device)
{
    const char *fn = "snpgpu_ibd_loglik";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, IBD_GENO)) return 1;
    if (!out) { set_error("snpgpu_ibd_loglik: out is NULL"); return 1; }
    if ((k0 == nullptr) != (k1 == nullptr)) { set_error("snpgpu_ibd_loglik: give both k0 and k1 matrices, or neither"); return 1; }
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) { set_error("snpgpu_ibd_loglik: invalid out_mem"); return 1; }
    Call c;
    if (c.open(fn, device, false)) return 1;
    CallStream &st = c.st;
    DevArena &bufs = c.bufs;
    Prep P;
    if (prepare(st, bufs, geno, n_snp, n_samp, mem, allele_freq, P)) return 1;
    if (afreq_out) std::copy(P.af.begin(), P.af.end(), afreq_out);
    int rc = 0;
    const std::vector<int64_t> off = row_offsets(n_samp, 0, n_samp, true);
    DevBuf *drow = bufs.get(sizeof(int64_t) * off.size(), rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(drow->p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, st.s));
    const size_t nn = (size_t)n_samp * (size_t)n_samp;
    HostOut m0, m1, o;
    if (k0) {
        if (m0.open(bufs, (void *)k0, nn * sizeof(double), out_mem, true, st.s) ||
            m1.open(bufs, (void *)k1, nn * sizeof(double), out_mem, true, st.s))
            return 1;
    }
    if (o.open(bufs, out, nn * sizeof(double), out_mem, false, st.s)) return 1;
    if (launch_ibd_loglik(st.s, (const uint32_t *)P.gt->p, P.w4, P.tab->p, (const int64_t *)drow->p, n_samp, n_samp,
                          off.back(), (const double *)m0.dev, (const double *)m1.dev, k0_all, k1_all, (double *)o.dev))
        return 1;
    if (o.close(st.s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    return 0;
}

int snpgpu_ibd_mle_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_ibd_mle_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 4; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
