// C ABI of libsnpgpu, ancestry proportions by EM (include/snpgpu.h section 1s): the object behind snpgdsAdmix.  Kernels:
// kernels_admix.hip; the definitions: DESIGN.md 32.
//
// snpgpu_admix_create checks and records its arguments and makes no HIP call, and neither do a feed of host rows into an object
// whose device is not open yet (the rows are copied and wait) or snpgpu_admix_set (the checked values wait): the first run, get or
// feed of device rows opens the device, checks the memory, allocates and takes what waits, in the order it came.  So every
// refusal that depends on the arguments or on the object's state alone is made before any HIP call.
// The 2-bit rows stay resident ([max_snps][rbr], rbr = the row bytes rounded up to 16, the padding 0xFF = missing).  A pass walks
// the fed SNPs in internal blocks of block_snps: the per-SNP owner and the per-sample owner of each block, then the folds of the
// segments, Q', F' and L.  The internal block bounds a launch and nothing else -- the rows are resident and no operand plane is
// staged -- so the sums are cut at fixed absolute indices (admix_device.h) and the bits do not depend on it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "admix_device.h"
#include "host_util.h"
#include "workspace.h"

using namespace snpgpu;

namespace {

constexpr size_t ADMIX_STAGE_BYTES = size_t(64) << 20;      // host rows and one-byte genotypes on their way to the resident rows
constexpr size_t ADMIX_RESERVE_BYTES = size_t(64) << 20;    // left free on the device beside an object
constexpr int64_t ADMIX_SAMP_END = int64_t(1) << 23;
constexpr int64_t ADMIX_SNP_END = int64_t(1) << 30;
constexpr int64_t ADMIX_BLOCK_MAX = int64_t(1) << 20;       // SNPs of an internal block when none is asked for

inline int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

}  // namespace

struct snpgpu_admix {
    int device = 0;
    void *user_stream = nullptr;
    CallStream st;
    bool open = false;
    int64_t n = 0, max_snps = 0, rbr = 0, block = 0, n_fed = 0, f_rows = -1;
    int K = 0;
    double f_min = 0;
    bool have_q = false;
    // what waits for the device: host feeds in their order, the checked values of snpgpu_admix_set
    struct Waiting { std::vector<uint8_t> bytes; int64_t n_snp; int format; };
    std::vector<Waiting> waiting;
    std::vector<double> q_host, f_host;
    bool q_waits = false, f_waits = false;
    DevBuf rows, Q[2], F[2], apart, upart, vpart, lpart, lsnp, lout;
    int cur_q = 0, cur_f = 0;
    EventLog log;
    double pass_ms = 0;
    int64_t blocks_per_pass = 0, launches = 0, iterations = 0;
    size_t resident = 0;
};

namespace {

int64_t n_sseg(const snpgpu_admix *a) { return (a->n + ADMIX_SSEG - 1) / ADMIX_SSEG; }
int64_t n_jseg(const snpgpu_admix *a) { return (a->max_snps + ADMIX_JSEG - 1) / ADMIX_JSEG; }

int check_create(const char *fn, int64_t n_samp, int n_pop, int64_t max_snps, double f_min, int64_t block_snps)
{
    if (n_samp < 1 || n_samp >= ADMIX_SAMP_END) return fail(fn, "invalid number of samples (1 ... 2^23 - 1)");
    if (n_pop < 2 || n_pop > ADMIX_MAX_POP) return fail(fn, "invalid number of populations: n_pop must be in 2 ... 32");
    if (max_snps < 1 || max_snps >= ADMIX_SNP_END) return fail(fn, "invalid max_snps (1 ... 2^30 - 1)");
    if (!(f_min > 0.0 && f_min < 0.5)) return fail(fn, "f_min must be inside (0, 0.5)");
    if (block_snps < 0 || block_snps % 16 || block_snps > ADMIX_BLOCK_MAX)
        return fail(fn, "block_snps must be 0 or a positive multiple of 16, at most 2^20");
    return 0;
}

// the first use of the device: stream, memory check, buffers
int open_device(const char *fn, snpgpu_admix *a)
{
    if (a->open) { SNPGPU_HIP_CHECK(hipSetDevice(a->device)); return 0; }
    if (a->st.open(fn, a->device, a->user_stream)) return 1;
    const size_t nk = sizeof(double) * (size_t)a->n * (size_t)a->K, mk = sizeof(double) * (size_t)a->max_snps * (size_t)a->K;
    const size_t rows = (size_t)a->max_snps * (size_t)a->rbr;
    const size_t ap = nk * (size_t)n_jseg(a), up_ = mk * (size_t)n_sseg(a), lp = sizeof(double) * (size_t)a->max_snps * (size_t)n_sseg(a);
    const size_t state = rows + 2 * nk + 2 * mk, work = ap + 2 * up_ + lp + sizeof(double) * (size_t)a->max_snps + ADMIX_STAGE_BYTES;
    size_t free_b = 0, total_b = 0;
    SNPGPU_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (state + work + ADMIX_RESERVE_BYTES > free_b)
        return fail(fn, "the device cannot hold this object: its genotype rows, Q and F take " + std::to_string(state >> 20) +
                            " MiB and the segment sums " + std::to_string(work >> 20) + " MiB, " + std::to_string(free_b >> 20) +
                            " MiB are free (there is no CPU fallback)");
    if (a->rows.alloc(rows) || a->Q[0].alloc(nk) || a->Q[1].alloc(nk) || a->F[0].alloc(mk) || a->F[1].alloc(mk) || a->apart.alloc(ap) ||
        a->upart.alloc(up_) || a->vpart.alloc(up_) || a->lpart.alloc(lp) || a->lsnp.alloc(sizeof(double) * (size_t)a->max_snps) ||
        a->lout.alloc(sizeof(double)))
        return 1;
    SNPGPU_HIP_CHECK(hipMemsetAsync(a->rows.p, 0xFF, rows, a->st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(a->st.s));
    a->resident = state + ap + 2 * up_ + lp + sizeof(double) * (size_t)a->max_snps;
    a->log.on = true;
    a->open = true;
    return 0;
}

AdmixState state_of(const snpgpu_admix *a)
{
    return AdmixState{(const uint8_t *)a->rows.p, a->rbr, a->n, a->n_fed, a->K, (const double *)a->Q[a->cur_q].p, (const double *)a->F[a->cur_f].p};
}

// One pass over the fed genotypes from the current (Q, F): *loglik = L(Q, F); move_q / move_f: Q' / F' become current
int pass(snpgpu_admix *a, bool move_q, bool move_f, double *loglik)
{
    hipStream_t s = a->st.s;
    const AdmixState S = state_of(a);
    if (a->log.begin(0, s)) return 1;
    int64_t blocks = 0;
    for (int64_t j0 = 0; j0 < a->n_fed; j0 += a->block, blocks++) {
        const int64_t j1 = std::min(a->n_fed, j0 + a->block);
        if (launch_admix_snp(s, S, j0, j1, move_f, (double *)a->upart.p, (double *)a->vpart.p, (double *)a->lpart.p)) return 1;
        a->launches++;
        if (move_q) {
            if (launch_admix_samp(s, S, j0, j1, (double *)a->apart.p)) return 1;
            a->launches++;
        }
    }
    a->blocks_per_pass = blocks;
    if (launch_admix_fold_snp(s, S, (const double *)a->upart.p, (const double *)a->vpart.p, (const double *)a->lpart.p, a->f_min,
                              move_f ? (double *)a->F[a->cur_f ^ 1].p : nullptr, (double *)a->lsnp.p))
        return 1;
    if (move_q && launch_admix_fold_samp(s, S, (const double *)a->apart.p, (double *)a->Q[a->cur_q ^ 1].p)) return 1;
    if (launch_admix_loglik(s, (const double *)a->lsnp.p, a->n_fed, (double *)a->lout.p)) return 1;
    a->launches += 2 + (move_q ? 1 : 0);
    if (a->log.end(s)) return 1;
    // the scalar the stopping rule needs: the only host traffic of a pass
    SNPGPU_HIP_CHECK(hipMemcpyAsync(loglik, a->lout.p, sizeof(double), hipMemcpyDeviceToHost, s));
    if (hipStreamSynchronize(s) != hipSuccess) return fail("snpgpu_admix_run", "a kernel failed");
    if (move_q) a->cur_q ^= 1;
    if (move_f) a->cur_f ^= 1;
    return 0;
}

// n_snp caller rows into the resident rows from row `at` on
int feed_rows(const char *fn, snpgpu_admix *ad, const void *geno, int64_t n_snp, int format, int mem, int64_t at)
{
    hipStream_t s = ad->st.s;
    DevArena arena;
    RowBlocks rows;
    const int64_t rb_in = format == SNPGPU_GENO_U8 ? ad->n : (ad->n + 3) / 4;
    // (no forced block size from the environment: how the rows are cut on their way changes nothing that is kept)
    if (rows.open(arena, geno, n_snp, ad->n, format, mem, std::max(ADMIX_STAGE_BYTES / 2, (size_t)(16 * rb_in)), ADMIX_BLOCK_MAX, "")) return 1;
    const size_t width = (size_t)((ad->n + 3) / 4);
    uint8_t *dst = (uint8_t *)ad->rows.p + at * ad->rbr;
    const int rc = rows.for_each(s, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
        SNPGPU_HIP_CHECK(hipMemcpy2DAsync(dst + i0 * ad->rbr, (size_t)ad->rbr, src, (size_t)rb, width, (size_t)nb, hipMemcpyDeviceToDevice, s));
        return 0;
    });
    if (hipStreamSynchronize(s) != hipSuccess) return fail(fn, "a copy failed");
    return rc;
}

// opens the device and takes what waits: the host feeds in their order, then the values of snpgpu_admix_set
int flush(const char *fn, snpgpu_admix *ad)
{
    if (open_device(fn, ad)) return 1;
    if (!ad->waiting.empty()) {
        int64_t total = 0;
        for (const auto &w : ad->waiting) total += w.n_snp;
        int64_t at = ad->n_fed - total;
        for (const auto &w : ad->waiting) {
            if (feed_rows(fn, ad, w.bytes.data(), w.n_snp, w.format, SNPGPU_HOST, at)) return 1;
            at += w.n_snp;
        }
        ad->waiting.clear();
        ad->waiting.shrink_to_fit();
    }
    hipStream_t s = ad->st.s;
    if (ad->q_waits) SNPGPU_HIP_CHECK(hipMemcpyAsync(ad->Q[ad->cur_q].p, ad->q_host.data(), sizeof(double) * ad->q_host.size(), hipMemcpyHostToDevice, s));
    if (ad->f_waits) SNPGPU_HIP_CHECK(hipMemcpyAsync(ad->F[ad->cur_f].p, ad->f_host.data(), sizeof(double) * ad->f_host.size(), hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    ad->q_waits = ad->f_waits = false;
    std::vector<double>().swap(ad->q_host);
    std::vector<double>().swap(ad->f_host);
    return 0;
}

int fold_log(snpgpu_admix *a)
{
    SNPGPU_HIP_CHECK(hipStreamSynchronize(a->st.s));
    double t = 0;
    if (a->log.sum_ms(0, &t)) return 1;
    a->pass_ms += t;
    a->log.clear();
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_admix_create(int64_t n_samp, int n_pop, int64_t max_snps, double f_min, int64_t block_snps, const snpgpu_opts *opts,
                        snpgpu_admix **out)
{
    const char *fn = "snpgpu_admix_create";
    if (!out) return fail(fn, "NULL argument: out is NULL");
    *out = nullptr;
    if (check_create(fn, n_samp, n_pop, max_snps, f_min, block_snps)) return 1;
    snpgpu_admix *a = new snpgpu_admix();
    if (opts) { a->device = opts->device; a->user_stream = opts->stream; }
    a->n = n_samp; a->K = n_pop; a->max_snps = max_snps; a->f_min = f_min;
    a->rbr = up((n_samp + 3) / 4, 16);
    a->block = block_snps > 0 ? block_snps : std::min(up(max_snps, 16), ADMIX_BLOCK_MAX);
    *out = a;
    return 0;
}

int snpgpu_admix_destroy(snpgpu_admix *ad)
{
    if (!ad) return 0;
    if (ad->open && ad->st.s) {
        (void)hipSetDevice(ad->device);
        (void)hipStreamSynchronize(ad->st.s);
    }
    delete ad;
    return 0;
}

int snpgpu_admix_feed(snpgpu_admix *ad, const void *geno, int64_t n_snp, int format, int mem)
{
    const char *fn = "snpgpu_admix_feed";
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) return fail(fn, "invalid genotype format");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) return fail(fn, "invalid memory kind");
    if (n_snp < 0 || n_snp >= ADMIX_SNP_END) return fail(fn, "invalid number of SNPs");
    if (!ad) return fail(fn, "NULL argument: ad is NULL");
    if (!geno && n_snp > 0) return fail(fn, "NULL argument: geno is NULL");
    if (ad->n_fed + n_snp > ad->max_snps)
        return fail(fn, "more rows than max_snps: " + std::to_string(ad->n_fed) + " fed, " + std::to_string(n_snp) + " more, max_snps " +
                            std::to_string(ad->max_snps));
    if (n_snp == 0) return 0;
    if (!ad->open && mem == SNPGPU_HOST) {
        const size_t bytes = (size_t)n_snp * (size_t)(format == SNPGPU_GENO_U8 ? ad->n : (ad->n + 3) / 4);
        ad->waiting.push_back({std::vector<uint8_t>((const uint8_t *)geno, (const uint8_t *)geno + bytes), n_snp, format});
        ad->n_fed += n_snp;
        return 0;
    }
    if (flush(fn, ad)) return 1;
    if (feed_rows(fn, ad, geno, n_snp, format, mem, ad->n_fed)) return 1;
    ad->n_fed += n_snp;
    return 0;
}

int snpgpu_admix_set(snpgpu_admix *ad, const double *q, const double *f)
{
    const char *fn = "snpgpu_admix_set";
    if (!ad) return fail(fn, "NULL argument: ad is NULL");
    const int K = ad->K;
    std::vector<double> qn, fc;
    if (q) {
        qn.assign(q, q + (size_t)ad->n * K);
        for (int64_t i = 0; i < ad->n; i++) {
            double sum = 0.0;
            for (int k = 0; k < K; k++) {
                const double v = q[i * K + k];
                if (!std::isfinite(v) || v < 0.0) return fail(fn, "q must be finite and non-negative (sample " + std::to_string(i) + ")");
                sum += v;
            }
            if (!(sum > 0.0) || !std::isfinite(sum)) return fail(fn, "a row of q has no positive sum (sample " + std::to_string(i) + ")");
            for (int k = 0; k < K; k++) qn[i * K + k] = q[i * K + k] / sum;
        }
    }
    if (f) {
        if (ad->n_fed == 0) return fail(fn, "f before any row was fed: it holds one row per fed SNP");
        fc.assign(f, f + (size_t)ad->n_fed * K);
        for (double &v : fc) {
            if (!std::isfinite(v)) return fail(fn, "f must be finite");
            v = std::min(std::max(v, ad->f_min), 1.0 - ad->f_min);
        }
    }
    // the values wait for the next run or get (no HIP call here)
    if (q) { ad->q_host.swap(qn); ad->q_waits = true; ad->have_q = true; }
    if (f) { ad->f_host.swap(fc); ad->f_waits = true; ad->f_rows = ad->n_fed; }
    return 0;
}

int snpgpu_admix_run(snpgpu_admix *ad, int max_iter, double tol, int flags, double *loglik, int *n_done)
{
    const char *fn = "snpgpu_admix_run";
    if (!ad) return fail(fn, "NULL argument: ad is NULL");
    if (!loglik) return fail(fn, "NULL argument: loglik is NULL");
    if (max_iter < 0) return fail(fn, "negative max_iter");
    if (flags & ~SNPGPU_ADMIX_FIX_F) return fail(fn, "unknown flags");
    if (std::isnan(tol)) return fail(fn, "tol is NaN");
    if (!ad->have_q || ad->f_rows < 0) return fail(fn, "run before set: Q and F have no values (snpgpu_admix_set)");
    if (ad->f_rows != ad->n_fed)
        return fail(fn, "rows were fed after F was set: F holds " + std::to_string(ad->f_rows) + " of " + std::to_string(ad->n_fed) + " SNPs");
    if (flush(fn, ad)) return 1;
    const bool move_f = !(flags & SNPGPU_ADMIX_FIX_F);
    int done = 0;
    for (int t = 0; t < max_iter; t++) {
        if (pass(ad, true, move_f, &loglik[t])) return 1;
        done = t + 1;
        ad->iterations++;
        if (t >= 1 && loglik[t] - loglik[t - 1] < tol) break;
    }
    // the likelihood of the state that is kept
    if (pass(ad, false, false, &loglik[done])) return 1;
    if (n_done) *n_done = done;
    return fold_log(ad);
}

int snpgpu_admix_get(snpgpu_admix *ad, double *q, double *f)
{
    const char *fn = "snpgpu_admix_get";
    if (!ad) return fail(fn, "NULL argument: ad is NULL");
    if (q && !ad->have_q) return fail(fn, "Q has no values (snpgpu_admix_set)");
    if (f && ad->f_rows < 0) return fail(fn, "F has no values (snpgpu_admix_set)");
    if (!q && !f) return 0;
    if (flush(fn, ad)) return 1;
    hipStream_t s = ad->st.s;
    if (q) SNPGPU_HIP_CHECK(hipMemcpyAsync(q, ad->Q[ad->cur_q].p, sizeof(double) * (size_t)ad->n * (size_t)ad->K, hipMemcpyDeviceToHost, s));
    if (f) SNPGPU_HIP_CHECK(hipMemcpyAsync(f, ad->F[ad->cur_f].p, sizeof(double) * (size_t)ad->f_rows * (size_t)ad->K, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int snpgpu_admix_stats(snpgpu_admix *ad, double *stats)
{
    const char *fn = "snpgpu_admix_stats";
    if (!ad || !stats) return fail(fn, "NULL argument");
    stats[0] = (double)ad->blocks_per_pass; stats[1] = (double)ad->launches; stats[2] = ad->pass_ms; stats[3] = (double)ad->resident;
    stats[4] = (double)ad->block; stats[5] = (double)ad->iterations;
    return 0;
}

int snpgpu_gnrAdmix(int n_pop, double f_min, int64_t block_snps, const double *q, const double *f, int max_iter, double tol, int flags,
                    double *loglik, int *n_done, double *q_res, double *f_res)
{
    const char *fn = "snpgpu_gnrAdmix";
    if (!q || !f) return fail(fn, "NULL argument: the starting values q and f");
    if (need_ws(fn)) return 1;
    if (ws_n_snp() < 1) return fail(fn, "no SNP in the working dataset");
    snpgpu_opts o{};
    o.device = ws_device();
    struct Guard { snpgpu_admix *p = nullptr; ~Guard() { if (p) snpgpu_admix_destroy(p); } } g;
    if (snpgpu_admix_create(ws_n_samp(), n_pop, ws_n_snp(), f_min, block_snps, &o, &g.p)) return 1;
    // the device is opened before the feeds, so that the working space's blocks go straight to the resident rows (no second host copy)
    if (flush(fn, g.p)) return 1;
    if (ws_for_each_block([&](const uint8_t *rows, int64_t, int64_t nb) {
            return snpgpu_admix_feed(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST);
        }))
        return 1;
    if (snpgpu_admix_set(g.p, q, f) || snpgpu_admix_run(g.p, max_iter, tol, flags, loglik, n_done)) return 1;
    return snpgpu_admix_get(g.p, q_res, f_res);
}

}  // extern "C"
