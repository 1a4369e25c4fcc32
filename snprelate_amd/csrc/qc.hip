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
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "snpgpu_internal.h"

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

struct Bufs {
    std::vector<DevBuf *> all;
    ~Bufs() { for (DevBuf *b : all) { b->release(); delete b; } }
    DevBuf *get(size_t bytes, int &rc)
    {
        DevBuf *b = new DevBuf;
        all.push_back(b);
        if (!rc) rc = b->alloc(bytes);
        return b;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~Stream()
    {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
    }
    int open(const char *fn, int device)
    {
        int ndev = 0;
        SNPGPU_HIP_CHECK(hipGetDeviceCount(&ndev));
        if (ndev <= 0) { set_error(std::string(fn) + ": no HIP device (the GPU path has no CPU fallback)"); return 1; }
        if (device < 0 || device >= ndev) { set_error(std::string(fn) + ": invalid device ordinal"); return 1; }
        SNPGPU_HIP_CHECK(hipSetDevice(device));
        SNPGPU_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        for (auto &e : ev) SNPGPU_HIP_CHECK(hipEventCreate(&e));
        return 0;
    }
};

int fail(const char *fn, const char *msg) { set_error(std::string(fn) + ": " + msg); return 1; }

int check_geno(const char *fn, const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem)
{
    if (!geno) return fail(fn, "geno is NULL");
    if (n_snp < 1) return fail(fn, "no SNP in the working dataset");
    if (n_snp >= (int64_t(1) << 31)) return fail(fn, "too many SNPs (< 2^31)");
    if (n_samp < 1 || n_samp >= (int64_t(1) << 30)) return fail(fn, "invalid number of samples (1 ... 2^30 - 1)");
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) return fail(fn, "invalid genotype format");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) return fail(fn, "invalid memory kind");
    return 0;
}

// per block: rows of rb bytes in device memory, the block's first SNP and its number of SNPs; the block is complete on the stream
using BlockFn = std::function<int(const uint8_t *src, int64_t rb, int64_t i0, int64_t nb)>;

// SNPGPU_QC_BLOCK_SNPS: a block size for every input kind (e.g. to test the streaming); blocks are multiples of 16 SNPs
int for_blocks(Stream &st, Bufs &bufs, const void *geno, int64_t n_snp, int64_t N, int format, int mem, const BlockFn &fn)
{
    const bool repack = format == SNPGPU_GENO_U8;
    const int64_t rb_in = repack ? N : (N + 3) / 4;
    const int64_t rb = repack ? (N + 255) / 256 * 64 : rb_in;
    int64_t B = (mem == SNPGPU_DEVICE && !repack) ? (n_snp + 15) / 16 * 16 : (int64_t)(QC_STAGE_BYTES / (size_t)rb_in);
    if (const char *e = getenv("SNPGPU_QC_BLOCK_SNPS")) { if (atoll(e) > 0) B = atoll(e); }
    B = std::min<int64_t>(B, QC_MAX_BLOCK_SNPS);                     // the kernels put SNP chunks / words into grid.y (<= 65 535)
    B = std::max<int64_t>(16, B / 16 * 16);
    B = std::min(B, (n_snp + 15) / 16 * 16);
    int rc = 0;
    DevBuf *raw = mem == SNPGPU_HOST ? bufs.get((size_t)(B * rb_in) + 32, rc) : nullptr;
    DevBuf *packed = repack ? bufs.get((size_t)(B * rb) + 32, rc) : nullptr;
    if (rc) return 1;
    for (int64_t i0 = 0; i0 < n_snp; i0 += B) {
        const int64_t nb = std::min(B, n_snp - i0);
        const uint8_t *src = (const uint8_t *)geno + i0 * rb_in;
        if (raw) {
            SNPGPU_HIP_CHECK(hipMemcpyAsync(raw->p, src, (size_t)(nb * rb_in), hipMemcpyHostToDevice, st.s));
            src = (const uint8_t *)raw->p;
        }
        if (repack) {
            if (launch_repack(st.s, src, format, nb, N, (uint8_t *)packed->p, rb)) return 1;
            src = (const uint8_t *)packed->p;
        }
        if (fn(src, rb, i0, nb)) return 1;
        SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));                // the staging buffers are reused by the next block
    }
    return 0;
}

// the counter kernel on one block, timed; snp_cnt: the block's [nb][3] (zeroed here) or NULL; samp_miss: zeroed by the caller
int count_block(Stream &st, const uint8_t *src, int64_t rb, int64_t nb, int64_t N, int32_t *snp_cnt, int32_t *samp_miss)
{
    if (snp_cnt) SNPGPU_HIP_CHECK(hipMemsetAsync(snp_cnt, 0, sizeof(int32_t) * 3 * (size_t)nb, st.s));
    SNPGPU_HIP_CHECK(hipEventRecord(st.ev[0], st.s));
    if (launch_qc_count(st.s, src, rb, nb, N, snp_cnt, samp_miss)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(st.ev[1], st.s));
    SNPGPU_HIP_CHECK(hipEventSynchronize(st.ev[1]));
    float ms = 0;
    SNPGPU_HIP_CHECK(hipEventElapsedTime(&ms, st.ev[0], st.ev[1]));
    g_stats[0] += ms; g_stats[1] += 1; g_stats[2] += (double)nb * (double)((N + 3) / 4);
    return 0;
}

// the exact test on device counters [n_snp][3] -> device p-values; the SNPs go to the lanes in descending order of rare copies
int hwe_core(Stream &st, Bufs &bufs, const int32_t *dcnt, int64_t n_snp, double *dpv)
{
    std::vector<int32_t> cnt(3 * (size_t)n_snp), perm((size_t)n_snp);
    SNPGPU_HIP_CHECK(hipMemcpyAsync(cnt.data(), dcnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    std::vector<int64_t> rare((size_t)n_snp);
    for (int64_t s = 0; s < n_snp; s++) {
        const int64_t a = cnt[3 * s], b = cnt[3 * s + 2];
        rare[(size_t)s] = 2 * std::min(a, b) + cnt[3 * s + 1];
        perm[(size_t)s] = (int32_t)s;
    }
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return rare[(size_t)x] > rare[(size_t)y]; });
    int rc = 0;
    DevBuf *dperm = bufs.get(sizeof(int32_t) * (size_t)n_snp, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dperm->p, perm.data(), sizeof(int32_t) * (size_t)n_snp, hipMemcpyHostToDevice, st.s));
    SNPGPU_HIP_CHECK(hipEventRecord(st.ev[0], st.s));
    if (launch_qc_hwe(st.s, dcnt, (const int32_t *)dperm->p, n_snp, dpv)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(st.ev[1], st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    float ms = 0;
    SNPGPU_HIP_CHECK(hipEventElapsedTime(&ms, st.ev[0], st.ev[1]));
    g_stats[7] += ms;
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_geno_counts(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int32_t *snp_cnt,
                       int32_t *samp_missing, int out_mem, int device)
{
    const char *fn = "snpgpu_geno_counts";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem)) return 1;
    if (!snp_cnt && !samp_missing) return fail(fn, "snp_cnt and samp_missing are both NULL");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (double &s : g_stats) s = 0;
    Stream st;
    Bufs bufs;
    if (st.open(fn, device)) return 1;
    const size_t cb = sizeof(int32_t) * 3 * (size_t)n_snp, mb = sizeof(int32_t) * (size_t)n_samp;
    int32_t *dc = snp_cnt, *dm = samp_missing;
    if (out_mem == SNPGPU_HOST) {
        int rc = 0;
        if (snp_cnt) dc = (int32_t *)bufs.get(cb, rc)->p;
        if (samp_missing) dm = (int32_t *)bufs.get(mb, rc)->p;
        if (rc) return 1;
    }
    if (dm) SNPGPU_HIP_CHECK(hipMemsetAsync(dm, 0, mb, st.s));
    if (for_blocks(st, bufs, geno, n_snp, n_samp, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
            return count_block(st, src, rb, nb, n_samp, dc ? dc + 3 * i0 : nullptr, dm);
        }))
        return 1;
    if (out_mem == SNPGPU_HOST) {
        if (snp_cnt) SNPGPU_HIP_CHECK(hipMemcpyAsync(snp_cnt, dc, cb, hipMemcpyDeviceToHost, st.s));
        if (samp_missing) SNPGPU_HIP_CHECK(hipMemcpyAsync(samp_missing, dm, mb, hipMemcpyDeviceToHost, st.s));
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    return 0;
}

int snpgpu_hwe(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, double *pvalue, int device)
{
    const char *fn = "snpgpu_hwe";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem)) return 1;
    if (!pvalue) return fail(fn, "pvalue is NULL");
    for (double &s : g_stats) s = 0;
    Stream st;
    Bufs bufs;
    if (st.open(fn, device)) return 1;
    int rc = 0;
    DevBuf *dc = bufs.get(sizeof(int32_t) * 3 * (size_t)n_snp, rc), *dp = bufs.get(sizeof(double) * (size_t)n_snp, rc);
    if (rc) return 1;
    if (for_blocks(st, bufs, geno, n_snp, n_samp, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
            return count_block(st, src, rb, nb, n_samp, (int32_t *)dc->p + 3 * i0, nullptr);
        }))
        return 1;
    if (hwe_core(st, bufs, (const int32_t *)dc->p, n_snp, (double *)dp->p)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(pvalue, dp->p, sizeof(double) * (size_t)n_snp, hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
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
    Stream st;
    Bufs bufs;
    if (st.open(fn, device)) return 1;
    const int32_t *dc = snp_cnt;
    double *dp = pvalue;
    if (mem == SNPGPU_HOST) {
        int rc = 0;
        DevBuf *c = bufs.get(sizeof(int32_t) * 3 * (size_t)n_snp, rc), *p = bufs.get(sizeof(double) * (size_t)n_snp, rc);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->p, snp_cnt, sizeof(int32_t) * 3 * (size_t)n_snp, hipMemcpyHostToDevice, st.s));
        dc = (const int32_t *)c->p;
        dp = (double *)p->p;
    }
    if (hwe_core(st, bufs, dc, n_snp, dp)) return 1;
    if (mem == SNPGPU_HOST) SNPGPU_HIP_CHECK(hipMemcpyAsync(pvalue, dp, sizeof(double) * (size_t)n_snp, hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    return 0;
}

int snpgpu_ind_inb(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq, int method,
                   double reltol, double *coeff, int32_t *niter, double *afreq_out, int out_mem, int device)
{
    const char *fn = "snpgpu_ind_inb";
    if (method < SNPGPU_INB_MOM_WEIR || method > SNPGPU_INB_GCTA3) return fail(fn, "invalid method (1 ... 6)");
    if (check_geno(fn, geno, n_snp, n_samp, format, mem)) return 1;
    if (!coeff) return fail(fn, "coeff is NULL");
    if (method == SNPGPU_INB_MLE && !std::isfinite(reltol)) return fail(fn, "`reltol' should a real number.");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (double &s : g_stats) s = 0;
    Stream st;
    Bufs bufs;
    if (st.open(fn, device)) return 1;

    const bool mle = method == SNPGPU_INB_MLE, weir = method == SNPGPU_INB_MOM_WEIR;
    const int64_t N = n_samp, nw = (n_snp + 15) / 16;
    int rc = 0;
    DevBuf *daf = bufs.get(sizeof(double) * (size_t)(16 * nw), rc);            // the frequencies used, all SNPs
    DevBuf *dcnt = allele_freq ? nullptr : bufs.get(sizeof(int32_t) * 3 * (size_t)n_snp, rc);
    DevBuf *dout = bufs.get(sizeof(double) * (size_t)N, rc);
    DevBuf *dnit = bufs.get(sizeof(int32_t) * (size_t)N, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemsetAsync(daf->p, 0, sizeof(double) * (size_t)(16 * nw), st.s));
    if (allele_freq)
        SNPGPU_HIP_CHECK(hipMemcpyAsync(daf->p, allele_freq, sizeof(double) * (size_t)n_snp, hipMemcpyHostToDevice, st.s));
    double *af = (double *)daf->p;
    int32_t *cnt = dcnt ? (int32_t *)dcnt->p : nullptr;

    if (!mle) {
        const int64_t bmax = (n_snp + 15) / 16 * 16;                             // no block of for_blocks is larger
        DevBuf *tab = bufs.get(sizeof(double) * 4 * (size_t)bmax, rc), *flag = bufs.get((size_t)bmax, rc);
        DevBuf *acc = bufs.get(sizeof(double) * (size_t)N, rc), *den = bufs.get(sizeof(double) * (size_t)N, rc);
        DevBuf *scnt = bufs.get(sizeof(int32_t) * (size_t)N, rc);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(acc->p, 0, sizeof(double) * (size_t)N, st.s));
        SNPGPU_HIP_CHECK(hipMemsetAsync(den->p, 0, sizeof(double) * (size_t)N, st.s));
        SNPGPU_HIP_CHECK(hipMemsetAsync(scnt->p, 0, sizeof(int32_t) * (size_t)N, st.s));
        if (for_blocks(st, bufs, geno, n_snp, N, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
                if (cnt) {
                    if (count_block(st, src, rb, nb, N, cnt + 3 * i0, nullptr)) return 1;
                    if (launch_qc_freq(st.s, cnt + 3 * i0, nb, 0, af + i0)) return 1;
                }
                SNPGPU_HIP_CHECK(hipEventRecord(st.ev[0], st.s));
                if (launch_qc_table(st.s, method, af + i0, nb, tab->p, (uint8_t *)flag->p)) return 1;
                if (launch_qc_mom(st.s, weir, src, rb, nb, N, tab->p, (const uint8_t *)flag->p, (double *)acc->p, (double *)den->p,
                                  (int32_t *)scnt->p))
                    return 1;
                SNPGPU_HIP_CHECK(hipEventRecord(st.ev[2], st.s));
                SNPGPU_HIP_CHECK(hipEventSynchronize(st.ev[2]));
                float ms = 0;
                SNPGPU_HIP_CHECK(hipEventElapsedTime(&ms, st.ev[0], st.ev[2]));
                g_stats[3] += ms;
                return 0;
            }))
            return 1;
        if (launch_qc_mom_final(st.s, weir, N, (const double *)acc->p, (const double *)den->p, (const int32_t *)scnt->p,
                                (double *)dout->p))
            return 1;
    } else {
        DevBuf *gt = bufs.get(sizeof(uint32_t) * (size_t)N * (size_t)nw, rc), *dst = bufs.get(2 * sizeof(unsigned long long), rc);
        if (rc) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(dst->p, 0, 2 * sizeof(unsigned long long), st.s));
        if (for_blocks(st, bufs, geno, n_snp, N, format, mem, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
                if (cnt) {
                    if (count_block(st, src, rb, nb, N, cnt + 3 * i0, nullptr)) return 1;
                    if (launch_qc_freq(st.s, cnt + 3 * i0, nb, 1, af + i0)) return 1;
                }
                return launch_qc_words(st.s, src, rb, nb, N, i0 / 16, nw, (uint32_t *)gt->p);      // blocks start at multiples of 16
            }))
            return 1;
        SNPGPU_HIP_CHECK(hipEventRecord(st.ev[0], st.s));
        if (launch_qc_mle(st.s, (const uint32_t *)gt->p, nw, af, N, reltol, (double *)dout->p, (int32_t *)dnit->p,
                          (unsigned long long *)dst->p))
            return 1;
        SNPGPU_HIP_CHECK(hipEventRecord(st.ev[1], st.s));
        unsigned long long q[2] = {0, 0};
        SNPGPU_HIP_CHECK(hipMemcpyAsync(q, dst->p, sizeof(q), hipMemcpyDeviceToHost, st.s));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
        float ms = 0;
        SNPGPU_HIP_CHECK(hipEventElapsedTime(&ms, st.ev[0], st.ev[1]));
        g_stats[4] = ms; g_stats[5] = (double)q[0]; g_stats[6] = (double)q[1];
    }
    const hipMemcpyKind kind = out_mem == SNPGPU_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(coeff, dout->p, sizeof(double) * (size_t)N, kind, st.s));
    if (mle && niter) SNPGPU_HIP_CHECK(hipMemcpyAsync(niter, dnit->p, sizeof(int32_t) * (size_t)N, kind, st.s));
    if (afreq_out) SNPGPU_HIP_CHECK(hipMemcpyAsync(afreq_out, af, sizeof(double) * (size_t)n_snp, hipMemcpyDeviceToHost, st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
    return 0;
}

int snpgpu_qc_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_qc_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 8; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
