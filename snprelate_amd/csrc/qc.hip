// C ABI of libsnpgpu, quality-control statistics (include/snpgpu.h section 1g): genotype counts per SNP and missing calls per
// sample (gnrSampFreq, src/SNPRelate.cpp:275-283), the exact test of Hardy-Weinberg equilibrium (gnrHWE, src/genHWE.cpp:46-137)
// and individual inbreeding coefficients (gnrIndInb, src/genIBD.cpp:1847-2006).  Kernels: kernels_qc.hip.
//
// The genotypes are read once, block by block: 2-bit rows in device memory where they lie, host rows through one staging buffer,
// one-byte genotypes through the existing repack.  Every block runs the counter kernel and whatever the statistic adds per block
// (the moment kernel, or the transposition to the resident sample-major words of the MLE).  All argument errors are found before
// any device is touched.
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_util.h"

namespace snpgpu {
int launch_qc_count(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, int64_t n_samp, int32_t *snp_cnt, int32_t *samp_miss);
int launch_qc_freq(hipStream_t st, const int32_t *cnt, int64_t n_snp, int mode, double *af);
int launch_qc_table(hipStream_t st, int method, const double *af, int64_t n_snp, void *tab, uint8_t *flag);
int launch_qc_mom(hipStream_t st, int weir, const uint8_t *geno, int64_t rb, int64_t n_snp, int64_t n_samp, const void *tab,
                  const uint8_t *flag, double *acc, double *den, int32_t *cnt);
int launch_qc_mom_final(hipStream_t st, int weir, int64_t n_samp, const double *acc, const double *den, const int32_t *cnt, double *out);
int launch_qc_words(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, int64_t n_samp, int64_t w0, int64_t nw, uint32_t *gt);
int launch_qc_mle(hipStream_t st, const uint32_t *gt, int64_t nw, const double *af, int64_t n_samp, double reltol, double *out_f,
                  int32_t *out_niter, unsigned long long *stats);
int launch_qc_hwe(hipStream_t st, const int32_t *cnt, const int32_t *perm, int64_t n_snp, double *pv);
}  // namespace snpgpu

using namespace snpgpu;

namespace {

// counter ms, its launches, genotype bytes it read, moment ms, MLE ms, MLE useful / issued lane-steps, HWE ms
thread_local double g_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

constexpr size_t QC_STAGE_BYTES = size_t(256) << 20;     // genotype bytes per streamed block
constexpr int64_t QC_MAX_BLOCK_SNPS = 65535 * 16;         // SNPs per block of any input kind: 65 535 words of 16 SNPs

constexpr GenoLimits QC_GENO = {1, int64_t(1) << 30, int64_t(1) << 31, false, "invalid number of samples (1 ... 2^30 - 1)"};
enum { T_COUNT = 0, T_MOM = 1, T_MLE = 2, T_HWE = 3 };   // phases of a call's EventLog (always on: snpgpu_qc_stats reports every call)

// the rows in blocks (RowBlocks; SNPGPU_QC_BLOCK_SNPS forces a block size): fn(src, rb, i0, nb) per block
template <class F> int for_blocks(Call &c, const void *geno, int64_t n_snp, int64_t N, int format, int mem, F &&fn)
{
    RowBlocks blocks;
    if (blocks.open(c.bufs, geno, n_snp, N, format, mem, QC_STAGE_BYTES, QC_MAX_BLOCK_SNPS, "SNPGPU_QC_BLOCK_SNPS")) return 1;
    return blocks.for_each(c.st.s, fn);
}

// the counter kernel on one block, timed; snp_cnt: the block's [nb][3] (zeroed here) or NULL; samp_miss: zeroed by the caller
int count_block(Call &c, const uint8_t *src, int64_t rb, int64_t nb, int64_t N, int32_t *snp_cnt, int32_t *samp_miss)
{
    hipStream_t s = c.st.s;
    if (snp_cnt) SNPGPU_HIP_CHECK(hipMemsetAsync(snp_cnt, 0, sizeof(int32_t) * 3 * (size_t)nb, s));
    if (c.log.begin(T_COUNT, s) || launch_qc_count(s, src, rb, nb, N, snp_cnt, samp_miss) || c.log.end(s)) return 1;
    if (c.log.wait_last(&g_stats[0])) return 1;
    g_stats[1] += 1; g_stats[2] += (double)nb * (double)((N + 3) / 4);
    return 0;
}

// the exact test on device counters [n_snp][3] -> device p-values; the SNPs go to the lanes in descending order of rare copies
int hwe_core(Call &c, const int32_t *dcnt, int64_t n_snp, double *dpv)
{
    hipStream_t s = c.st.s;
    std::vector<int32_t> cnt(3 * (size_t)n_snp), perm((size_t)n_snp);
    SNPGPU_HIP_CHECK(hipMemcpyAsync(cnt.data(), dcnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int64_t> rare((size_t)n_snp);
    for (int64_t i = 0; i < n_snp; i++) {
        const int64_t a = cnt[3 * i], b = cnt[3 * i + 2];
        rare[(size_t)i] = 2 * std::min(a, b) + cnt[3 * i + 1];
        perm[(size_t)i] = (int32_t)i;
    }
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return rare[(size_t)x] > rare[(size_t)y]; });
    int rc = 0;
    DevBuf *dperm = c.bufs.get(sizeof(int32_t) * (size_t)n_snp, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dperm->p, perm.data(), sizeof(int32_t) * (size_t)n_snp, hipMemcpyHostToDevice, s));
    if (c.log.begin(T_HWE, s) || launch_qc_hwe(s, dcnt, (const int32_t *)dperm->p, n_snp, dpv) || c.log.end(s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return c.log.wait_last(&g_stats[7]);
}

}  // namespace

extern "C" {

int snpgpu_geno_counts(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int32_t *snp_cnt,
                       int32_t *samp_missing, int out_mem, int device)
{
    const char *fn = "snpgpu_geno_counts";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, QC_GENO)) return 1;
    if (!snp_cnt && !samp_missing) return fail(fn, "snp_cnt and samp_missing are both NULL");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    hipStream_t s = c.st.s;
    HostOut oc, om;
    if (oc.open(c.bufs, snp_cnt, sizeof(int32_t) * 3 * (size_t)n_snp, out_mem, false, s) ||
        om.open(c.bufs, samp_missing, sizeof(int32_t) * (size_t)n_samp, out_mem, false, s))
        return 1;
    int32_t *dc = (int32_t *)oc.dev, *dm = (int32_t *)om.dev;
    if (dm) SNPGPU_HIP_CHECK(hipMemsetAsync(dm, 0, om.bytes, s));
    if (for_blocks(c, geno, n_snp, n_samp, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
            return count_block(c, src, rb, nb, n_samp, dc ? dc + 3 * i0 : nullptr, dm);
        }))
        return 1;
    if (oc.close(s) || om.close(s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int snpgpu_hwe(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, double *pvalue, int device)
{
    const char *fn = "snpgpu_hwe";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, QC_GENO)) return 1;
    if (!pvalue) return fail(fn, "pvalue is NULL");
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    int rc = 0;
    DevBuf *dc = c.bufs.get(sizeof(int32_t) * 3 * (size_t)n_snp, rc), *dp = c.bufs.get(sizeof(double) * (size_t)n_snp, rc);
    if (rc) return 1;
    if (for_blocks(c, geno, n_snp, n_samp, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
            return count_block(c, src, rb, nb, n_samp, (int32_t *)dc->p + 3 * i0, nullptr);
        }))
        return 1;
    if (hwe_core(c, (const int32_t *)dc->p, n_snp, (double *)dp->p)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(pvalue, dp->p, sizeof(double) * (size_t)n_snp, hipMemcpyDeviceToHost, c.st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c.st.s));
    return 0;
}

int snpgpu_hwe_counts(const int32_t *snp_cnt, int64_t n_snp, double *pvalue, int mem, int device)
{
    const char *fn = "snpgpu_hwe_counts";
    if (!snp_cnt || !pvalue) return fail(fn, "snp_cnt / pvalue is NULL");
    if (n_snp < 1 || n_snp >= (int64_t(1) << 31)) return fail(fn, "invalid number of SNPs");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) return fail(fn, "invalid memory kind");
    if (mem == SNPGPU_HOST)
        for (int64_t i = 0; i < 3 * n_snp; i++)
            if (snp_cnt[i] < 0) return fail(fn, "a count is negative");
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    HostOut in, out;                                  // `in` is only read: never closed
    if (in.open(c.bufs, (void *)snp_cnt, sizeof(int32_t) * 3 * (size_t)n_snp, mem, true, c.st.s) ||
        out.open(c.bufs, pvalue, sizeof(double) * (size_t)n_snp, mem, false, c.st.s))
        return 1;
    if (hwe_core(c, (const int32_t *)in.dev, n_snp, (double *)out.dev) || out.close(c.st.s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c.st.s));
    return 0;
}

// coeff / niter are copied out of buffers of the call (niter may be NULL, and the kernels write both), so they are no HostOut
int snpgpu_ind_inb(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq, int method,
                   double reltol, double *coeff, int32_t *niter, double *afreq_out, int out_mem, int device)
{
    const char *fn = "snpgpu_ind_inb";
    if (method < SNPGPU_INB_MOM_WEIR || method > SNPGPU_INB_GCTA3) return fail(fn, "invalid method (1 ... 6)");
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, QC_GENO)) return 1;
    if (!coeff) return fail(fn, "coeff is NULL");
    if (method == SNPGPU_INB_MLE && !std::isfinite(reltol)) return fail(fn, "`reltol' should a real number.");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    hipStream_t s = c.st.s;
    DevArena &bufs = c.bufs;

    const bool mle = method == SNPGPU_INB_MLE, weir = method == SNPGPU_INB_MOM_WEIR;
    const int64_t N = n_samp, nw = (n_snp + 15) / 16;
    int rc = 0;
    DevBuf *daf = bufs.get(sizeof(double) * (size_t)(16 * nw), rc);            // the frequencies used, all SNPs
    DevBuf *dcnt = allele_freq ? nullptr : bufs.get(sizeof(int32_t) * 3 * (size_t)n_snp, rc);
    DevBuf *dout = bufs.get(sizeof(double) * (size_t)N, rc);
    DevBuf *dnit = bufs.get(sizeof(int32_t) * (size_t)N, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemsetAsync(daf->p, 0, sizeof(double) * (size_t)(16 * nw), s));
    if (allele_freq)
        SNPGPU_HIP_CHECK(hipMemcpyAsync(daf->p, allele_freq, sizeof(double) * (size_t)n_snp, hipMemcpyHostToDevice, s));
    double *af = (double *)daf->p;
    int32_t *cnt = dcnt ? (int32_t *)dcnt->p : nullptr;

    if (!mle) {
        const int64_t bmax = (n_snp + 15) / 16 * 16;                             // no block of for_blocks is larger
        DevBuf *tab = bufs.get(sizeof(double) * 4 * (size_t)bmax, rc), *flag = bufs.get((size_t)bmax, rc);
        DevBuf *acc = bufs.get(sizeof(double) * (size_t)N, rc), *den = bufs.get(sizeof(double) * (size_t)N, rc);
        DevBuf *scnt = bufs.get(sizeof(int32_t) * (size_t)N, rc);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(acc->p, 0, sizeof(double) * (size_t)N, s));
        SNPGPU_HIP_CHECK(hipMemsetAsync(den->p, 0, sizeof(double) * (size_t)N, s));
        SNPGPU_HIP_CHECK(hipMemsetAsync(scnt->p, 0, sizeof(int32_t) * (size_t)N, s));
        if (for_blocks(c, geno, n_snp, N, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
                if (cnt) {
                    if (count_block(c, src, rb, nb, N, cnt + 3 * i0, nullptr)) return 1;
                    if (launch_qc_freq(s, cnt + 3 * i0, nb, 0, af + i0)) return 1;
                }
                if (c.log.begin(T_MOM, s) || launch_qc_table(s, method, af + i0, nb, tab->p, (uint8_t *)flag->p) ||
                    launch_qc_mom(s, weir, src, rb, nb, N, tab->p, (const uint8_t *)flag->p, (double *)acc->p, (double *)den->p,
                                  (int32_t *)scnt->p) ||
                    c.log.end(s))
                    return 1;
                return c.log.wait_last(&g_stats[3]);
            }))
            return 1;
        if (launch_qc_mom_final(s, weir, N, (const double *)acc->p, (const double *)den->p, (const int32_t *)scnt->p,
                                (double *)dout->p))
            return 1;
    } else {
        DevBuf *gt = bufs.get(sizeof(uint32_t) * (size_t)N * (size_t)nw, rc), *dst = bufs.get(2 * sizeof(unsigned long long), rc);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(dst->p, 0, 2 * sizeof(unsigned long long), s));
        if (for_blocks(c, geno, n_snp, N, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
                if (cnt) {
                    if (count_block(c, src, rb, nb, N, cnt + 3 * i0, nullptr)) return 1;
                    if (launch_qc_freq(s, cnt + 3 * i0, nb, 1, af + i0)) return 1;
                }
                return launch_qc_words(s, src, rb, nb, N, i0 / 16, nw, (uint32_t *)gt->p);      // blocks start at multiples of 16
            }))
            return 1;
        if (c.log.begin(T_MLE, s) ||
            launch_qc_mle(s, (const uint32_t *)gt->p, nw, af, N, reltol, (double *)dout->p, (int32_t *)dnit->p,
                          (unsigned long long *)dst->p) ||
            c.log.end(s))
            return 1;
        unsigned long long q[2] = {0, 0};
        SNPGPU_HIP_CHECK(hipMemcpyAsync(q, dst->p, sizeof(q), hipMemcpyDeviceToHost, s));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
        if (c.log.sum_ms(T_MLE, &g_stats[4])) return 1;
        g_stats[5] = (double)q[0]; g_stats[6] = (double)q[1];
    }
    const hipMemcpyKind kind = out_mem == SNPGPU_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(coeff, dout->p, sizeof(double) * (size_t)N, kind, s));
    if (mle && niter) SNPGPU_HIP_CHECK(hipMemcpyAsync(niter, dnit->p, sizeof(int32_t) * (size_t)N, kind, s));
    if (afreq_out) SNPGPU_HIP_CHECK(hipMemcpyAsync(afreq_out, af, sizeof(double) * (size_t)n_snp, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int snpgpu_qc_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_qc_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 8; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
