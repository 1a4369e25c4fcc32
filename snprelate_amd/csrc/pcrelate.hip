// C ABI of libsnpgpu, PC-Relate (include/snpgpu.h section 1r): the streaming object behind snpgdsPCRelate.  Kernels:
// kernels_pcrelate.hip; the definitions: DESIGN.md 31.
//
// At creation the host makes W = V_T (V_T^T V_T)^-1 by Cholesky (V = [1, pcs]) and uploads W, V and the training flags; the n x n
// result planes are allocated and zeroed -- three without SNPGPU_PCR_IBD, eight with it.  A feed walks its rows in internal blocks
// of at most `cap` SNPs (nine operand planes of cap x n_pad doubles within SNPGPU_PCR_STAGE_BYTES; the same cap whatever the flags,
// the format and the memory kind, so that the same feeds give the same bits): beta kernel, operand kernel, then the product
// launches, which add the block's sums to the planes.  Everything is on one stream; a feed returns when its rows have been read.
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"
#include "pcrelate_device.h"
#include "workspace.h"

using namespace snpgpu;

namespace {

constexpr size_t PCR_STAGE_BYTES = size_t(1) << 30;     // the nine operand planes of one internal block
constexpr size_t PCR_OUT_BYTES = size_t(64) << 20;      // one result of one row window on its way to the host
constexpr int64_t PCR_SAMP_END = int64_t(1) << 23;
enum { T_BETA = 0, T_OPS = 1, T_PROD = 2, T_FINAL = 3, N_PHASE = 4 };

inline int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// planes that hold the tiles I <= J only (all but DC)
inline bool plane_sym(int which) { return which != PCR_DC; }

}  // namespace

struct snpgpu_pcr {
    int device = 0;
    CallStream st;
    int64_t n = 0, n_pad = 0, cap = 0;
    int D = 0, d1 = 0, d1p = 0, flags = 0, n_range = 1;
    int64_t range_bytes = 0;
    double lo = 0, hi = 0;
    DevBuf W, Vt, train, beta, num, part, cnt, ops, e, inbreed;
    DevBuf planes[PCR_N_PLANES];
    EventLog log;
    double ms[N_PHASE] = {0, 0, 0, 0};
    int64_t blocks = 0, launches = 0, n_fed = 0;
    size_t plane_bytes = 0;
};

namespace {

bool has_ibd(const snpgpu_pcr *p) { return (p->flags & SNPGPU_PCR_IBD) != 0; }

PcrPlanes plane_ptrs(const snpgpu_pcr *p)
{
    PcrPlanes P;
    for (int k = 0; k < PCR_N_PLANES; k++) P.p[k] = (const double *)p->planes[k].p;
    return P;
}

// W = V_T (V_T^T V_T)^-1 as [n][d1p] with zero rows outside T and zero columns >= d1.  A pivot that is not above 2^-40 of its
// diagonal entry counts as non-positive: what rounding leaves of an exactly dependent column.  Every operation is rounded on its
// own and the sums run in index order, so that a restatement of these loops (tests/pcrelate_ref.py) gives the same bits.
int regression_matrix(const char *fn, int64_t n, int D, const double *pcs, const uint8_t *training, int d1p, std::vector<double> &W)
{
#pragma clang fp contract(off)
    const int d1 = D + 1;
    std::vector<double> G((size_t)d1 * d1, 0.0), v((size_t)d1);
    for (int64_t i = 0; i < n; i++) {
        if (training && !training[i]) continue;
        v[0] = 1.0;
        for (int d = 0; d < D; d++) v[d + 1] = pcs[i * D + d];
        for (int a = 0; a < d1; a++)
            for (int b = 0; b <= a; b++) G[(size_t)a * d1 + b] += v[a] * v[b];
    }
    std::vector<double> Lc((size_t)d1 * d1, 0.0);
    for (int a = 0; a < d1; a++) {
        for (int b = 0; b <= a; b++) {
            double s = G[(size_t)a * d1 + b];
            for (int k = 0; k < b; k++) s -= Lc[(size_t)a * d1 + k] * Lc[(size_t)b * d1 + k];
            if (a == b) {
                if (!(s > std::ldexp(G[(size_t)a * d1 + a], -40))) return fail(fn, "the principal components are collinear in the training set");
                Lc[(size_t)a * d1 + a] = std::sqrt(s);
            } else {
                Lc[(size_t)a * d1 + b] = s / Lc[(size_t)b * d1 + b];
            }
        }
    }
    W.assign((size_t)n * d1p, 0.0);
    for (int64_t i = 0; i < n; i++) {
        if (training && !training[i]) continue;
        v[0] = 1.0;
        for (int d = 0; d < D; d++) v[d + 1] = pcs[i * D + d];
        for (int a = 0; a < d1; a++) {                          // L y = v
            double s = v[a];
            for (int k = 0; k < a; k++) s -= Lc[(size_t)a * d1 + k] * v[k];
            v[a] = s / Lc[(size_t)a * d1 + a];
        }
        for (int a = d1 - 1; a >= 0; a--) {                     // L^T w = y
            double s = v[a];
            for (int k = a + 1; k < d1; k++) s -= Lc[(size_t)k * d1 + a] * v[k];
            v[a] = s / Lc[(size_t)a * d1 + a];
        }
        for (int a = 0; a < d1; a++) W[(size_t)i * d1p + a] = v[a];
    }
    return 0;
}

int check_create(const char *fn, int64_t n, int D, const double *pcs, const uint8_t *training, double maf_thresh, int flags)
{
    if (n < 1 || n >= PCR_SAMP_END) return fail(fn, "invalid number of samples (1 ... 2^23 - 1)");
    if (D < 0 || D > PCR_MAX_PC) return fail(fn, "invalid number of principal components: n_pc must be in 0 ... 32");
    if (D > 0 && !pcs) return fail(fn, "NULL argument: pcs is NULL");
    if (flags & ~SNPGPU_PCR_IBD) return fail(fn, "unknown flags");
    if (!(maf_thresh > 0.0 && maf_thresh < 0.5)) return fail(fn, "maf_thresh must be inside (0, 0.5)");
    int64_t nt = 0;
    for (int64_t i = 0; i < n; i++) nt += !training || training[i];
    if (nt < D + 2) return fail(fn, "too few training samples: " + std::to_string(nt) + " for " + std::to_string(D) + " principal components (at least n_pc + 2)");
    for (int64_t i = 0; i < n * D; i++)
        if (!std::isfinite(pcs[i])) return fail(fn, "a principal component is not finite");
    return 0;
}

int fold_log(snpgpu_pcr *p)
{
    SNPGPU_HIP_CHECK(hipStreamSynchronize(p->st.s));
    for (int k = 0; k < N_PHASE; k++) {
        double t = 0;
        if (p->log.sum_ms(k, &t)) return 1;
        p->ms[k] += t;
    }
    p->log.clear();
    return 0;
}

// one internal block: nb 2-bit rows of rb bytes at src (device)
int feed_block(snpgpu_pcr *p, const uint8_t *src, int64_t rb, int64_t nb, double *beta_out)
{
    hipStream_t s = p->st.s;
    const int m = (int)nb;
    double *beta = (double *)p->beta.p, *ops = (double *)p->ops.p;
    const int64_t stride = p->cap * p->n_pad;
    if (p->log.begin(T_BETA, s) ||
        launch_pcr_beta(s, src, rb, m, p->n, (const uint8_t *)p->train.p, (const double *)p->W.p, p->d1p, p->d1, p->n_range, p->range_bytes,
                        (double *)p->part.p, (int32_t *)p->cnt.p, beta, (int32_t *)p->num.p) ||
        p->log.end(s))
        return 1;
    if (beta_out) SNPGPU_HIP_CHECK(hipMemcpyAsync(beta_out, beta, sizeof(double) * (size_t)m * (size_t)p->d1, hipMemcpyDeviceToHost, s));
    const int n_ops = has_ibd(p) ? PCR_N_OPS : PCR_N_OPS_KIN;
    if (p->log.begin(T_OPS, s) ||
        launch_pcr_operands(s, src, rb, m, p->n, p->n_pad, beta, (const int32_t *)p->num.p, p->d1, (const double *)p->Vt.p, p->lo, p->hi, n_ops,
                            ops, stride) ||
        p->log.end(s))
        return 1;
    auto op = [&](int k) { return (const double *)(ops + (int64_t)k * stride); };
    auto pl = [&](int k) { return (double *)p->planes[k].p; };
    if (p->log.begin(T_PROD, s)) return 1;
    PcrJobs a{};
    int na = 0;
    a.j[na++] = {op(PCR_OP_R), op(PCR_OP_R), pl(PCR_RR)};
    a.j[na++] = {op(PCR_OP_S), op(PCR_OP_S), pl(PCR_SS)};
    a.j[na++] = {op(PCR_OP_O), op(PCR_OP_O), pl(PCR_NS)};
    if (has_ibd(p)) {
        a.j[na++] = {op(PCR_OP_GD), op(PCR_OP_GD), pl(PCR_DD)};
        a.j[na++] = {op(PCR_OP_C), op(PCR_OP_C), pl(PCR_CC)};
        a.j[na++] = {op(PCR_OP_I0), op(PCR_OP_I2), pl(PCR_IBS0)};
        a.j[na++] = {op(PCR_OP_A), op(PCR_OP_B), pl(PCR_K0D)};
    }
    if (launch_pcr_products(s, a, na, p->n, p->n_pad, m, true)) return 1;
    p->launches++;
    if (has_ibd(p)) {
        // the second halves of IBS0 and K0D go into the same planes: a launch of their own, after the first
        PcrJobs b{};
        b.j[0] = {op(PCR_OP_I2), op(PCR_OP_I0), pl(PCR_IBS0)};
        b.j[1] = {op(PCR_OP_B), op(PCR_OP_A), pl(PCR_K0D)};
        PcrJobs c{};
        c.j[0] = {op(PCR_OP_GD), op(PCR_OP_C), pl(PCR_DC)};
        if (launch_pcr_products(s, b, 2, p->n, p->n_pad, m, true) || launch_pcr_products(s, c, 1, p->n, p->n_pad, m, false)) return 1;
        p->launches += 2;
    }
    if (p->log.end(s)) return 1;
    p->blocks++;
    return 0;
}

// a result that leaves in row windows: make(r0, rows, dev) fills dev[rows][n], which is copied to host + r0 * n
template <class F> int windowed(snpgpu_pcr *p, int n_out, double *const *host, F &&make)
{
    const int64_t n = p->n;
    const int64_t rows_max = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(PCR_OUT_BYTES / (sizeof(double) * (size_t)n))));
    DevBuf tmp;
    if (tmp.alloc(sizeof(double) * (size_t)rows_max * (size_t)n * (size_t)n_out)) return 1;
    hipStream_t s = p->st.s;
    for (int64_t r0 = 0; r0 < n; r0 += rows_max) {
        const int64_t rows = std::min(rows_max, n - r0);
        double *dev[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0, at = 0; k < n_out; k++)
            if (host[k]) dev[k] = (double *)tmp.p + (int64_t)(at++) * rows_max * n;
        if (p->log.begin(T_FINAL, s) || make(r0, rows, dev) || p->log.end(s)) return 1;
        for (int k = 0; k < n_out; k++)
            if (host[k]) SNPGPU_HIP_CHECK(hipMemcpyAsync(host[k] + r0 * n, dev[k], sizeof(double) * (size_t)rows * (size_t)n, hipMemcpyDeviceToHost, s));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_pcr_create(int64_t n_samp, int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags,
                      const snpgpu_opts *opts, snpgpu_pcr **out)
{
    const char *fn = "snpgpu_pcr_create";
    if (!out) return fail(fn, "NULL argument: out is NULL");
    *out = nullptr;
    if (check_create(fn, n_samp, n_pc, pcs, training, maf_thresh, flags)) return 1;
    const int d1 = n_pc + 1, d1p = (int)up(d1, PCR_KC);
    std::vector<double> W;
    if (regression_matrix(fn, n_samp, n_pc, pcs, training, d1p, W)) return 1;
    snpgpu_opts o{};
    if (opts) o = *opts;
    snpgpu_pcr *p = new snpgpu_pcr();
    struct Guard { snpgpu_pcr *p; ~Guard() { if (p) snpgpu_pcr_destroy(p); } } guard{p};
    if (p->st.open(fn, o.device, o.stream)) return 1;
    p->device = o.device; p->n = n_samp; p->n_pad = up(n_samp, PCR_TILE); p->D = n_pc; p->d1 = d1; p->d1p = d1p; p->flags = flags;
    p->lo = maf_thresh; p->hi = 1.0 - maf_thresh;
    const size_t per_snp = sizeof(double) * (size_t)PCR_N_OPS * (size_t)p->n_pad;
    p->cap = std::max<int64_t>(16, (int64_t)(env_bytes("SNPGPU_PCR_STAGE_BYTES", PCR_STAGE_BYTES) / per_snp) / 16 * 16);
    p->cap = std::min<int64_t>(p->cap, int64_t(1) << 20);
    // the beta kernel's sample ranges: at least 64 row bytes (256 samples) each, at most 32 of them
    const int64_t row_bytes = (n_samp + 3) / 4;
    p->n_range = (int)std::max<int64_t>(1, std::min<int64_t>(32, row_bytes / 64));
    p->range_bytes = (row_bytes + p->n_range - 1) / p->n_range;
    const size_t part_bytes = sizeof(double) * (size_t)p->n_range * (size_t)p->cap * 2 * (size_t)d1p;
    const int n_planes = has_ibd(p) ? PCR_N_PLANES : 3, n_ops = has_ibd(p) ? PCR_N_OPS : PCR_N_OPS_KIN;
    const size_t nn = sizeof(double) * (size_t)n_samp * (size_t)n_samp;
    p->plane_bytes = nn * (size_t)n_planes;
    const size_t work = sizeof(double) * (size_t)n_ops * (size_t)p->cap * (size_t)p->n_pad + sizeof(double) * (size_t)p->cap * (size_t)d1 +
                        part_bytes + sizeof(double) * (size_t)n_samp * (size_t)(d1p + n_pc + 2) + 4 * std::min(nn, PCR_OUT_BYTES);
    size_t free_b = 0, total_b = 0;
    SNPGPU_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (p->plane_bytes + work + (size_t(64) << 20) > free_b)
        return fail(fn, "the device cannot hold this object: its " + std::to_string(n_planes) + " result planes take " +
                            std::to_string(p->plane_bytes >> 20) + " MiB and its work buffers " + std::to_string(work >> 20) + " MiB, " +
                            std::to_string(free_b >> 20) + " MiB are free (there is no CPU fallback)");
    hipStream_t s = p->st.s;
    // V transposed and padded, sample fastest; the training flags
    std::vector<double> Vt((size_t)std::max(1, n_pc) * (size_t)p->n_pad, 0.0);
    for (int64_t i = 0; i < n_samp; i++)
        for (int d = 0; d < n_pc; d++) Vt[(size_t)d * p->n_pad + i] = pcs[i * n_pc + d];
    std::vector<uint8_t> tr((size_t)n_samp, 1);
    if (training)
        for (int64_t i = 0; i < n_samp; i++) tr[i] = training[i] ? 1 : 0;
    if (p->W.alloc(sizeof(double) * W.size()) || p->Vt.alloc(sizeof(double) * Vt.size()) || p->train.alloc(tr.size()) ||
        p->beta.alloc(sizeof(double) * (size_t)p->cap * (size_t)d1) || p->num.alloc(sizeof(int32_t) * (size_t)p->cap) ||
        p->part.alloc(part_bytes) || p->cnt.alloc(sizeof(int32_t) * (size_t)p->n_range * (size_t)p->cap * 2) ||
        p->ops.alloc(sizeof(double) * (size_t)n_ops * (size_t)p->cap * (size_t)p->n_pad) || p->e.alloc(sizeof(double) * (size_t)n_samp) ||
        p->inbreed.alloc(sizeof(double) * (size_t)n_samp))
        return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(p->W.p, W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(p->Vt.p, Vt.data(), sizeof(double) * Vt.size(), hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(p->train.p, tr.data(), tr.size(), hipMemcpyHostToDevice, s));
    const int held[PCR_N_PLANES] = {PCR_RR, PCR_SS, PCR_NS, PCR_DD, PCR_DC, PCR_CC, PCR_IBS0, PCR_K0D};
    for (int k = 0; k < n_planes; k++) {
        DevBuf &b = p->planes[held[k]];
        if (b.alloc(nn)) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(b.p, 0, nn, s));
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));                  // the host arrays of this call go out of scope
    p->log.on = true;
    guard.p = nullptr;
    *out = p;
    return 0;
}

int snpgpu_pcr_destroy(snpgpu_pcr *pcr)
{
    if (!pcr) return 0;
    if (pcr->st.s) {
        (void)hipSetDevice(pcr->device);
        (void)hipStreamSynchronize(pcr->st.s);
    }
    delete pcr;
    return 0;
}

int snpgpu_pcr_feed(snpgpu_pcr *pcr, const void *geno, int64_t n_snp, int format, int mem, double *beta)
{
    const char *fn = "snpgpu_pcr_feed";
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) return fail(fn, "invalid genotype format");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) return fail(fn, "invalid memory kind");
    if (n_snp < 0 || n_snp >= (int64_t(1) << 30)) return fail(fn, "invalid number of SNPs");
    if (!pcr) return fail(fn, "NULL argument: pcr is NULL");
    if (!geno && n_snp > 0) return fail(fn, "NULL argument: geno is NULL");
    if (n_snp == 0) return 0;
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    DevArena arena;
    RowBlocks rows;
    const int64_t rb_in = format == SNPGPU_GENO_U8 ? pcr->n : (pcr->n + 3) / 4;
    // the staging window holds exactly one internal block: every input form is cut at the same SNPs
    if (rows.open(arena, geno, n_snp, pcr->n, format, mem, (size_t)(pcr->cap * rb_in), pcr->cap, "SNPGPU_PCR_BLOCK_SNPS")) return 1;
    const int d1 = pcr->d1;
    const int rc = rows.for_each(s, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
        return feed_block(pcr, src, rb, nb, beta ? beta + i0 * d1 : nullptr);
    });
    if (hipStreamSynchronize(s) != hipSuccess) return fail(fn, "a kernel failed");
    if (rc) return 1;
    pcr->n_fed += n_snp;
    return fold_log(pcr);
}

int snpgpu_pcr_result(snpgpu_pcr *pcr, double *kinship, double *inbreed, double *k0, double *k2, double *nsnp)
{
    const char *fn = "snpgpu_pcr_result";
    if (!pcr) return fail(fn, "NULL argument: pcr is NULL");
    if ((k0 || k2) && !has_ibd(pcr)) return fail(fn, "k0 and k2 need a handle created with SNPGPU_PCR_IBD");
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    const PcrPlanes P = plane_ptrs(pcr);
    if (pcr->log.begin(T_FINAL, s) || launch_pcr_diag(s, P, pcr->n, (double *)pcr->inbreed.p, (double *)pcr->e.p) || pcr->log.end(s)) return 1;
    if (inbreed) SNPGPU_HIP_CHECK(hipMemcpyAsync(inbreed, pcr->inbreed.p, sizeof(double) * (size_t)pcr->n, hipMemcpyDeviceToHost, s));
    double *host[4] = {kinship, k0, k2, nsnp};
    if (kinship || k0 || k2 || nsnp) {
        const int rc = windowed(pcr, 4, host, [&](int64_t r0, int64_t rows, double **dev) {
            return launch_pcr_final(s, P, pcr->n, r0, rows, (const double *)pcr->e.p, dev[0], dev[1], dev[2], dev[3]);
        });
        if (rc) return 1;
    }
    return fold_log(pcr);
}

int snpgpu_pcr_sums(snpgpu_pcr *pcr, int which, double *plane)
{
    const char *fn = "snpgpu_pcr_sums";
    if (!pcr || !plane) return fail(fn, "NULL argument");
    if (which < 0 || which >= PCR_N_PLANES) return fail(fn, "invalid plane: 0 ... 7 (RR, SS, DD, DC, CC, IBS0, K0D, NS)");
    if (!pcr->planes[which].p) return fail(fn, "this plane needs a handle created with SNPGPU_PCR_IBD");
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    double *host[1] = {plane};
    const int rc = windowed(pcr, 1, host, [&](int64_t r0, int64_t rows, double **dev) {
        return launch_pcr_plane(s, (const double *)pcr->planes[which].p, pcr->n, plane_sym(which), r0, rows, dev[0]);
    });
    if (rc) return 1;
    return fold_log(pcr);
}

int snpgpu_pcr_stats(snpgpu_pcr *pcr, double *stats)
{
    const char *fn = "snpgpu_pcr_stats";
    if (!pcr || !stats) return fail(fn, "NULL argument");
    stats[0] = (double)pcr->blocks; stats[1] = (double)pcr->launches;
    for (int k = 0; k < N_PHASE; k++) stats[2 + k] = pcr->ms[k];
    stats[6] = (double)pcr->plane_bytes; stats[7] = (double)pcr->cap;
    return 0;
}

int snpgpu_gnrPCRelate(int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags, double *kinship, double *inbreed,
                       double *k0, double *k2, double *nsnp)
{
    const char *fn = "snpgpu_gnrPCRelate";
    if (need_ws(fn)) return 1;
    if ((k0 || k2) && !(flags & SNPGPU_PCR_IBD)) return fail(fn, "k0 and k2 need SNPGPU_PCR_IBD");
    snpgpu_opts o{};
    o.device = ws_device();
    struct Guard { snpgpu_pcr *p = nullptr; ~Guard() { if (p) snpgpu_pcr_destroy(p); } } g;
    if (snpgpu_pcr_create(ws_n_samp(), n_pc, pcs, training, maf_thresh, flags, &o, &g.p)) return 1;
    if (ws_for_each_block([&](const uint8_t *rows, int64_t, int64_t nb) {
            return snpgpu_pcr_feed(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST, nullptr);
        }))
        return 1;
    return snpgpu_pcr_result(g.p, kinship, inbreed, k0, k2, nsnp);
}

}  // extern "C"
