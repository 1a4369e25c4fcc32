// C ABI of libsnpgpu, population statistics (include/snpgpu.h section 1f): per-SNP, per-population allele counters and the
// fixation index on them -- gnrFst (src/genFst.cpp:170-242) and the Fst scan of gnrSlidingWindow (src/genSlideWin.cpp:101-327).
// Kernels: kernels_pop.hip.
//
// Everything gnrFst needs from a SNP is 2 K integers, so the genotypes are read ONCE (streamed in SNP blocks; host rows through
// one staging buffer), the counters of the whole selection stay on the device (8 K bytes per SNP), and every window of a scan is a
// sum over them.  2-bit rows are counted where they lie (no re-layout); one-byte genotypes go through the existing repack first.
// All argument errors are found before any device is touched.
#include <algorithm>
#include <vector>

#include "host_util.h"

namespace snpgpu {
int launch_pop_mask(hipStream_t st, const int32_t *pop, int64_t n_samp, int64_t rb, int K, int n_var, int h0, int g, int64_t mbytes,
                    uint8_t *mask);
int launch_pop_count(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, int K, int n_var, int h0, int g, int64_t mvec,
                     const void *mask, int32_t *acnt, int32_t *cnt);
int launch_fst_terms(hipStream_t st, int method, const int32_t *acnt, const int32_t *cnt, int64_t n_snp, int K, double *num, double *den,
                     double *ratio, uint8_t *valid);
int launch_fst_sum_wc84(hipStream_t st, const double *num, const double *den, const int64_t *offsets, const int32_t *snp_index,
                        int64_t n_win, double *out);
int launch_fst_sum_wh02(hipStream_t st, const int32_t *acnt, const int32_t *cnt, const uint8_t *valid, int K, const int64_t *offsets,
                        const int32_t *snp_index, int64_t w0, int64_t n_w, double *sum_h, double *out);
}  // namespace snpgpu

using namespace snpgpu;

namespace {

// counter kernel ms, its launches, Fst kernels ms, genotype bytes the counter kernel read, launches of the W&H02 window sums
thread_local double g_stats[5] = {0, 0, 0, 0, 0};

constexpr size_t POP_STAGE_BYTES = size_t(256) << 20;    // genotype bytes per streamed block
constexpr size_t POP_SUMH_BYTES = size_t(64) << 20;      // W&H02 window sums per launch

constexpr GenoLimits POP_GENO = {1, int64_t(1) << 30, NO_LIMIT, false, "invalid number of samples (1 ... 2^30 - 1)"};
enum { T_COUNT = 0, T_FST = 1 };   // phases of a call's EventLog (always on: snpgpu_pop_stats reports every call)

int check_pop(const char *fn, const int32_t *pop, int64_t n_samp, int n_pop)
{
    if (n_pop < 2) return fail(fn, "There should be at least two populations!");
    if (!pop) return fail(fn, "pop is NULL");
    std::vector<int64_t> size((size_t)n_pop, 0);
    for (int64_t i = 0; i < n_samp; i++) {
        if (pop[i] < 0 || pop[i] >= n_pop) return fail(fn, "a population index lies outside the populations");
        size[(size_t)pop[i]]++;
    }
    for (int k = 0; k < n_pop; k++)
        if (size[(size_t)k] < 1) return fail(fn, "Each population should have at least one individual.");
    return 0;
}

int check_method(const char *fn, int method)
{
    if (method != SNPGPU_FST_WC84 && method != SNPGPU_FST_WH02) return fail(fn, "invalid Fst method (1 = W&C84, 2 = W&H02)");
    return 0;
}

int check_windows(const char *fn, const int64_t *offsets, const int32_t *snp_index, int64_t n_win, int64_t n_snp)
{
    if (n_win < 1) return fail(fn, "no window");
    if (!offsets) return fail(fn, "offsets is NULL");
    if (offsets[0] != 0) return fail(fn, "offsets[0] should be 0");
    for (int64_t w = 0; w < n_win; w++)
        if (offsets[w + 1] < offsets[w]) return fail(fn, "window offsets should not decrease");
    if (offsets[n_win] > 0 && !snp_index) return fail(fn, "snp_index is NULL");
    for (int64_t w = 0; w < n_win; w++)
        for (int64_t i = offsets[w]; i < offsets[w + 1]; i++) {
            if (snp_index[i] < 0 || snp_index[i] >= n_snp) return fail(fn, "a window holds a SNP index outside the genotype rows");
            if (i > offsets[w] && snp_index[i] <= snp_index[i - 1]) return fail(fn, "the SNP indices of a window should ascend");
        }
    return 0;
}

// the counters of all n_snp rows into device arrays [n_snp][K]; pop: host, 0-based
int count_all(Call &c, const void *geno, int64_t n_snp, int64_t N, int format, int mem, const int32_t *pop, int K, int32_t *dacnt,
              int32_t *dcnt)
{
    hipStream_t s = c.st.s;
    // 2-bit rows in device memory need no staging buffer: one launch over all of them.  Everything else goes through buffers of
    // the staging budget, block by block (SNPGPU_POP_BLOCK_SNPS: a block size for either case, e.g. to test the streaming)
    RowBlocks blocks;
    if (blocks.open(c.bufs, geno, n_snp, N, format, mem, POP_STAGE_BYTES, NO_LIMIT, "SNPGPU_POP_BLOCK_SNPS")) return 1;
    const int64_t rb = blocks.rb;                                    // bytes per row the counter kernel reads
    const int h0 = (int)((uintptr_t)blocks.first() & 15);
    int g = 16;
    while (rb % g) g >>= 1;                                          // gcd(rb, 16)
    const int n_var = 16 / g;
    const int64_t mbytes = (rb + 15 + 15) / 16 * 16, mvec = mbytes / 16;
    int rc = 0;
    DevBuf *mask = c.bufs.get((size_t)n_var * (size_t)K * (size_t)mbytes, rc);
    DevBuf *dpop = c.bufs.get(sizeof(int32_t) * (size_t)N, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dpop->p, pop, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, s));
    if (launch_pop_mask(s, (const int32_t *)dpop->p, N, rb, K, n_var, h0, g, mbytes, (uint8_t *)mask->p)) return 1;

    return blocks.for_each(s, [&](const uint8_t *src, int64_t, int64_t i0, int64_t nb) {
        if (c.log.begin(T_COUNT, s) ||
            launch_pop_count(s, src, rb, nb, K, n_var, h0, g, mvec, mask->p, dacnt + i0 * K, dcnt + i0 * K) || c.log.end(s))
            return 1;
        g_stats[1] += 1; g_stats[3] += (double)nb * (double)rb;
        return c.log.wait_last(&g_stats[0]);
    });
}

// Fst of the windows (CSR, host arrays; offsets == NULL: one window of all SNPs) from the device counters
int fst_core(Call &c, const int32_t *dacnt, const int32_t *dcnt, int64_t n_snp, int K, int method, const int64_t *offsets,
             const int32_t *snp_index, int64_t n_win, double *fst_win, double *beta_win, double *fst_snp)
{
    CallStream &st = c.st;
    DevArena &bufs = c.bufs;
    int rc = 0;
    const int64_t whole[2] = {0, n_snp};
    if (!offsets) { offsets = whole; snp_index = nullptr; n_win = 1; }
    const int64_t n_idx = snp_index ? offsets[n_win] : 0;
    DevBuf *dnum = bufs.get(method == SNPGPU_FST_WC84 ? sizeof(double) * (size_t)n_snp : 0, rc);
    DevBuf *dden = bufs.get(method == SNPGPU_FST_WC84 ? sizeof(double) * (size_t)n_snp : 0, rc);
    DevBuf *dratio = bufs.get(sizeof(double) * (size_t)n_snp, rc), *dvalid = bufs.get((size_t)n_snp, rc);
    DevBuf *doff = bufs.get(sizeof(int64_t) * (size_t)(n_win + 1), rc), *didx = bufs.get(sizeof(int32_t) * (size_t)n_idx, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(doff->p, offsets, sizeof(int64_t) * (size_t)(n_win + 1), hipMemcpyHostToDevice, st.s));
    if (n_idx > 0)
        SNPGPU_HIP_CHECK(hipMemcpyAsync(didx->p, snp_index, sizeof(int32_t) * (size_t)n_idx, hipMemcpyHostToDevice, st.s));
    const int32_t *idx = snp_index ? (const int32_t *)didx->p : nullptr;
    if (c.log.begin(T_FST, st.s)) return 1;
    if (launch_fst_terms(st.s, method, dacnt, dcnt, n_snp, K, (double *)dnum->p, (double *)dden->p, (double *)dratio->p,
                         (uint8_t *)dvalid->p))
        return 1;
    if (method == SNPGPU_FST_WC84) {
        DevBuf *dout = bufs.get(sizeof(double) * (size_t)n_win, rc);
        if (rc) return 1;
        if (launch_fst_sum_wc84(st.s, (const double *)dnum->p, (const double *)dden->p, (const int64_t *)doff->p, idx, n_win,
                                (double *)dout->p))
            return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(fst_win, dout->p, sizeof(double) * (size_t)n_win, hipMemcpyDeviceToHost, st.s));
    } else {
        const size_t kk = (size_t)K * (size_t)K;
        const int64_t W = std::max<int64_t>(1, std::min<int64_t>(n_win, (int64_t)(POP_SUMH_BYTES / (kk * 8))));
        DevBuf *dsum = bufs.get(sizeof(double) * kk * (size_t)W, rc), *dout = bufs.get(sizeof(double) * (size_t)W, rc);
        if (rc) return 1;
        for (int64_t w0 = 0; w0 < n_win; w0 += W) {
            const int64_t nw = std::min(W, n_win - w0);
            if (launch_fst_sum_wh02(st.s, dacnt, dcnt, (const uint8_t *)dvalid->p, K, (const int64_t *)doff->p, idx, w0, nw,
                                    (double *)dsum->p, (double *)dout->p))
                return 1;
            g_stats[4] += 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(fst_win + w0, dout->p, sizeof(double) * (size_t)nw, hipMemcpyDeviceToHost, st.s));
            if (beta_win)
                SNPGPU_HIP_CHECK(hipMemcpyAsync(beta_win + (size_t)w0 * kk, dsum->p, sizeof(double) * kk * (size_t)nw,
                                                hipMemcpyDeviceToHost, st.s));
        }
    }
    if (c.log.end(st.s)) return 1;
    if (fst_snp) SNPGPU_HIP_CHECK(hipMemcpyAsync(fst_snp, dratio->p, sizeof(double) * (size_t)n_snp, hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    return c.log.sum_ms(T_FST, &g_stats[2]);
}

// counters of the whole input on the device, then the windows' Fst (offsets == NULL: all SNPs as one window)
int fst_run(const char *fn, const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop, int method,
            const int64_t *offsets, const int32_t *snp_index, int64_t n_win, double *fst_win, double *beta_win, double *fst_snp, int device)
{
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    int rc = 0;
    const size_t bytes = sizeof(int32_t) * (size_t)n_snp * (size_t)n_pop;
    DevBuf *da = c.bufs.get(bytes, rc), *dc = c.bufs.get(bytes, rc);
    if (rc) return 1;
    if (count_all(c, geno, n_snp, n_samp, format, mem, pop, n_pop, (int32_t *)da->p, (int32_t *)dc->p)) return 1;
    return fst_core(c, (const int32_t *)da->p, (const int32_t *)dc->p, n_snp, n_pop, method, offsets, snp_index, n_win, fst_win,
                    beta_win, fst_snp);
}

}  // namespace

extern "C" {

int snpgpu_pop_counts(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop,
                      int32_t *acnt, int32_t *cnt, int out_mem, int device)
{
    const char *fn = "snpgpu_pop_counts";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, POP_GENO) || check_pop(fn, pop, n_samp, n_pop)) return 1;
    if (!acnt || !cnt) return fail(fn, "acnt / cnt is NULL");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    const size_t bytes = sizeof(int32_t) * (size_t)n_snp * (size_t)n_pop;
    HostOut oa, oc;
    if (oa.open(c.bufs, acnt, bytes, out_mem, false, c.st.s) || oc.open(c.bufs, cnt, bytes, out_mem, false, c.st.s)) return 1;
    if (count_all(c, geno, n_snp, n_samp, format, mem, pop, n_pop, (int32_t *)oa.dev, (int32_t *)oc.dev)) return 1;
    if (oa.close(c.st.s) || oc.close(c.st.s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c.st.s));
    return 0;
}

int snpgpu_fst_windows(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop, int method,
                       const int64_t *offsets, const int32_t *snp_index, int64_t n_win, double *fst_win, double *beta_win,
                       double *fst_snp, int device)
{
    const char *fn = "snpgpu_fst_windows";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, POP_GENO) || check_pop(fn, pop, n_samp, n_pop) || check_method(fn, method) ||
        check_windows(fn, offsets, snp_index, n_win, n_snp))
        return 1;
    if (!fst_win) return fail(fn, "fst_win is NULL");
    return fst_run(fn, geno, n_snp, n_samp, format, mem, pop, n_pop, method, offsets, snp_index, n_win, fst_win, beta_win, fst_snp, device);
}

int snpgpu_fst(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop, int method,
               double *fst, double *fst_snp, double *beta, int device)
{
    const char *fn = "snpgpu_fst";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, POP_GENO) || check_pop(fn, pop, n_samp, n_pop) || check_method(fn, method)) return 1;
    if (!fst) return fail(fn, "fst is NULL");
    return fst_run(fn, geno, n_snp, n_samp, format, mem, pop, n_pop, method, nullptr, nullptr, 1, fst, beta, fst_snp, device);
}

int snpgpu_pop_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_pop_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 5; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
