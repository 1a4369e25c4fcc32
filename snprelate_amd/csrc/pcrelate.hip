// C ABI of libsnpgpu, PC-Relate (include/snpgpu.h section 1r): the streaming object behind snpgdsPCRelate.  Kernels:
// kernels_pcrelate.hip; the definitions: DESIGN.md 31.
//
// At creation the host makes W = V_T (V_T^T V_T)^-1 by Cholesky (V = [1, pcs]) and uploads W, V and the training flags; the n x n
// result planes are allocated and zeroed -- three without SNPGPU_PCR_IBD, eight with it.  A feed walks its rows in internal blocks
// of at most `cap` SNPs (nine operand planes of cap x n_pad doubles within SNPGPU_PCR_STAGE_BYTES; the same cap whatever the flags,
// the format and the memory kind, so that the same feeds give the same bits): beta kernel, operand kernel, then the product
// launches, which add the block's sums to the planes.  Everything is on one stream; a feed returns when its rows have been read.
//
// A row panel (snpgpu_pcr_create_panel) is the same object with slabs [row_end - row_begin][n - row_begin] in place of
// the n x n planes, a ninth slab CD = DC transposed, and two strips of the diagonal tiles of RR and SS for every sample's
// inbreeding.  Its internal blocks, operands and tiles are the full object's, so its sums are the full object's bits.  Results and
// the selection of related pairs read either layout through a PcrView.
#include <algorithm>
#include <chrono>
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
constexpr size_t PCR_RESERVE_BYTES = size_t(64) << 20;  // left free on the device beside an object
constexpr int64_t PCR_SAMP_END = int64_t(1) << 23;
// (a panel's CD job and its strips are timed on their own and counted into the product phase of snpgpu_pcr_stats as well)
enum { T_BETA = 0, T_OPS = 1, T_PROD = 2, T_FINAL = 3, T_CD = 4, T_STRIP = 5, N_PHASE = 6 };

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
    DevBuf planes[PCR_N_SLABS];
    // a row panel: rows [row0, row1) x columns [row0, n) of every plane, and the diagonal tiles of RR and SS as [n_pad][PCR_TILE]
    bool panel = false;
    int64_t row0 = 0, row1 = 0;
    DevBuf strip_rr, strip_ss;
    EventLog log;
    double ms[N_PHASE] = {0, 0, 0, 0, 0, 0};
    int64_t blocks = 0, launches = 0, n_fed = 0;
    size_t plane_bytes = 0;
};

namespace {

// the selection kept by snpgpu_gnrPCRelatePairs for snpgpu_gnrPCRelatePairs_get, until the next call or snpgpu_ws_clear
struct PcrPairs {
    std::vector<int32_t> idx1, idx2;
    std::vector<double> kin, k0, k2, nsnp, inbreed;
};
PcrPairs g_pairs;

thread_local double g_pcr_sel_ms[4] = {0, 0, 0, 0};     // count pass, scan, write pass (device), whole call (host clock)

bool has_ibd(const snpgpu_pcr *p) { return (p->flags & SNPGPU_PCR_IBD) != 0; }

PcrPlanes plane_ptrs(const snpgpu_pcr *p)
{
    PcrPlanes P;
    for (int k = 0; k < PCR_N_PLANES; k++) P.p[k] = (const double *)p->planes[k].p;
    return P;
}

// the resident sums of either layout: a full object is the panel [0, n) without a CD slab
PcrView view_of(const snpgpu_pcr *p)
{
    PcrView v;
    for (int k = 0; k < PCR_N_SLABS; k++) v.p[k] = (const double *)p->planes[k].p;
    v.ld = p->n - p->row0; v.row0 = p->row0; v.row1 = p->row1; v.col0 = p->row0;
    return v;
}

// inbreed and e = 1 + inbreed of every sample, from the full planes or from the panel's strips
int diag_of(snpgpu_pcr *p)
{
    hipStream_t s = p->st.s;
    if (p->log.begin(T_FINAL, s)) return 1;
    if (p->panel) {
        if (launch_pcr_diag(s, (const double *)p->strip_rr.p, (const double *)p->strip_ss.p, p->n, PCR_TILE, PCR_TILE, (double *)p->inbreed.p,
                            (double *)p->e.p))
            return 1;
    } else if (launch_pcr_diag(s, (const double *)p->planes[PCR_RR].p, (const double *)p->planes[PCR_SS].p, p->n, p->n, 0,
                               (double *)p->inbreed.p, (double *)p->e.p)) {
        return 1;
    }
    return p->log.end(s);
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
    // the plane or slab k of this object as a job's destination: rows [row0, row1) x columns [row0, n)
    auto job = [&](int x, int y, int k, int mode = PCR_JOB_PLAIN) {
        return PcrJob{op(x), op(y), (double *)p->planes[k].p, p->n - p->row0, p->row0, p->row0, p->row1, mode};
    };
    const int tile0 = (int)(p->row0 / PCR_TILE), nt_rows = (int)(up(p->row1, PCR_TILE) / PCR_TILE) - tile0, nt_cols = (int)(p->n_pad / PCR_TILE) - tile0;
    auto launch = [&](const PcrJobs &jobs, int n_jobs, bool tri) {
        p->launches++;
        return launch_pcr_products(s, jobs, n_jobs, p->n, p->n_pad, m, tri, tile0, nt_rows, tile0, nt_cols);
    };
    if (p->log.begin(T_PROD, s)) return 1;
    PcrJobs a{};
    int na = 0;
    a.j[na++] = job(PCR_OP_R, PCR_OP_R, PCR_RR);
    a.j[na++] = job(PCR_OP_S, PCR_OP_S, PCR_SS);
    a.j[na++] = job(PCR_OP_O, PCR_OP_O, PCR_NS);
    if (has_ibd(p)) {
        a.j[na++] = job(PCR_OP_GD, PCR_OP_GD, PCR_DD);
        a.j[na++] = job(PCR_OP_C, PCR_OP_C, PCR_CC);
        a.j[na++] = job(PCR_OP_I0, PCR_OP_I2, PCR_IBS0);
        a.j[na++] = job(PCR_OP_A, PCR_OP_B, PCR_K0D);
    }
    if (launch(a, na, true)) return 1;
    if (has_ibd(p)) {
        // the second halves of IBS0 and K0D go into the same planes: a launch of their own, after the first
        PcrJobs b{};
        b.j[0] = job(PCR_OP_I2, PCR_OP_I0, PCR_IBS0);
        b.j[1] = job(PCR_OP_B, PCR_OP_A, PCR_K0D);
        PcrJobs c{};
        c.j[0] = job(PCR_OP_GD, PCR_OP_C, PCR_DC);
        if (launch(b, 2, true) || launch(c, 1, false)) return 1;
    }
    if (p->log.end(s)) return 1;
    const int cd_cols = nt_cols - nt_rows;          // tile columns right of the panel's diagonal block
    if (p->panel && has_ibd(p) && cd_cols > 0) {
        // DC's other half: the SAME job (gD, c) at the mirrored tile, stored transposed.  Inside the diagonal block DC itself holds
        // both halves (PcrView::dc), so only the columns >= row1 are computed; the block's part of the slab stays zero and unread.
        PcrJobs c{};
        c.j[0] = job(PCR_OP_GD, PCR_OP_C, PCR_CD, PCR_JOB_TRANSPOSED);
        p->launches++;
        if (p->log.begin(T_CD, s) || launch_pcr_products(s, c, 1, p->n, p->n_pad, m, false, tile0, nt_rows, tile0 + nt_rows, cd_cols) ||
            p->log.end(s))
            return 1;
    }
    if (p->panel) {
        // the diagonal tiles (J, J) of RR and SS for every J: the inbreeding of all n samples
        PcrJobs d{};
        d.j[0] = PcrJob{op(PCR_OP_R), op(PCR_OP_R), (double *)p->strip_rr.p, PCR_TILE, 0, 0, p->n, PCR_JOB_DIAG};
        d.j[1] = PcrJob{op(PCR_OP_S), op(PCR_OP_S), (double *)p->strip_ss.p, PCR_TILE, 0, 0, p->n, PCR_JOB_DIAG};
        p->launches++;
        if (p->log.begin(T_STRIP, s) || launch_pcr_products(s, d, 2, p->n, p->n_pad, m, false, 0, 1, 0, (int)(p->n_pad / PCR_TILE)) || p->log.end(s))
            return 1;
    }
    p->blocks++;
    return 0;
}

// a result that leaves in row windows: make(r0, rows, dev) fills dev[rows][n] for the rows r0 ... of `n_rows`, which is copied to
// host + r0 * n (n: the columns of the result, all samples unless said otherwise)
template <class F> int windowed(snpgpu_pcr *p, int n_out, double *const *host, F &&make, int64_t n_rows = -1, int64_t n_cols = -1)
{
    const int64_t n = n_cols < 0 ? p->n : n_cols, nr = n_rows < 0 ? p->n : n_rows;
    const int64_t rows_max = std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)(PCR_OUT_BYTES / (sizeof(double) * (size_t)n))));
    DevBuf tmp;
    if (tmp.alloc(sizeof(double) * (size_t)rows_max * (size_t)n * (size_t)n_out)) return 1;
    hipStream_t s = p->st.s;
    for (int64_t r0 = 0; r0 < nr; r0 += rows_max) {
        const int64_t rows = std::min(rows_max, nr - r0);
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

// what a panel of rows [r0, r1) keeps resident, the work buffers beside it and the SNPs of an internal block: the figures
// create() checks against the free memory, and snpgpu_gnrPCRelatePairs sizes its panels by
struct PcrBytes { size_t resident, work; int64_t cap; int n_slabs; };
PcrBytes pcr_bytes(int64_t n, int n_pc, int flags, bool panel, int64_t r0, int64_t r1)
{
    PcrBytes b{};
    const bool ibd = (flags & SNPGPU_PCR_IBD) != 0;
    const int d1 = n_pc + 1, d1p = (int)up(d1, PCR_KC);
    const int64_t n_pad = up(n, PCR_TILE);
    const size_t per_snp = sizeof(double) * (size_t)PCR_N_OPS * (size_t)n_pad;
    b.cap = std::max<int64_t>(16, (int64_t)(env_bytes("SNPGPU_PCR_STAGE_BYTES", PCR_STAGE_BYTES) / per_snp) / 16 * 16);
    b.cap = std::min<int64_t>(b.cap, int64_t(1) << 20);
    const int64_t row_bytes = (n + 3) / 4;
    const int n_range = (int)std::max<int64_t>(1, std::min<int64_t>(32, row_bytes / 64));
    const size_t part_bytes = sizeof(double) * (size_t)n_range * (size_t)b.cap * 2 * (size_t)d1p;
    const int n_ops = ibd ? PCR_N_OPS : PCR_N_OPS_KIN;
    b.n_slabs = ibd ? (panel ? PCR_N_SLABS : PCR_N_PLANES) : 3;
    const size_t nn = sizeof(double) * (size_t)(r1 - r0) * (size_t)(n - r0);
    b.resident = nn * (size_t)b.n_slabs + (panel ? 2 * sizeof(double) * (size_t)n_pad * PCR_TILE : 0);
    b.work = sizeof(double) * (size_t)n_ops * (size_t)b.cap * (size_t)n_pad + sizeof(double) * (size_t)b.cap * (size_t)d1 + part_bytes +
             sizeof(double) * (size_t)n * (size_t)(d1p + n_pc + 2) + 4 * std::min(nn, PCR_OUT_BYTES);
    return b;
}

// what snpgpu_pcr_select allocates on the device at most, for a panel of `rows` rows that starts at row 0: the outputs of every pair,
// the sample mask, the segment counts and offsets
size_t select_bytes(int64_t n, int64_t rows, bool ibd)
{
    const size_t pairs = (size_t)rows * (size_t)n, per_pair = 2 * sizeof(int32_t) + (ibd ? 4 : 2) * sizeof(double);
    return pairs * per_pair + (size_t)n + (size_t)rows * 4 * (sizeof(uint32_t) + sizeof(int64_t)) + 64;
}

int create(const char *fn, int64_t n_samp, int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags, bool panel,
           int64_t row_begin, int64_t row_end, const snpgpu_opts *opts, snpgpu_pcr **out)
{
    if (!out) return fail(fn, "NULL argument: out is NULL");
    *out = nullptr;
    if (check_create(fn, n_samp, n_pc, pcs, training, maf_thresh, flags)) return 1;
    if (panel) {
        if (row_begin < 0 || row_begin % PCR_TILE) return fail(fn, "row_begin must be a non-negative multiple of 128");
        if (row_end <= row_begin) return fail(fn, "the panel is empty: row_end <= row_begin");
        if (row_end > n_samp) return fail(fn, "row_end is beyond the samples");
        if (row_end % PCR_TILE && row_end != n_samp) return fail(fn, "row_end must be a multiple of 128 or the number of samples");
    }
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
    p->panel = panel; p->row0 = row_begin; p->row1 = row_end;
    const PcrBytes by = pcr_bytes(n_samp, n_pc, flags, panel, row_begin, row_end);
    p->cap = by.cap;
    // the beta kernel's sample ranges: at least 64 row bytes (256 samples) each, at most 32 of them
    const int64_t row_bytes = (n_samp + 3) / 4;
    p->n_range = (int)std::max<int64_t>(1, std::min<int64_t>(32, row_bytes / 64));
    p->range_bytes = (row_bytes + p->n_range - 1) / p->n_range;
    const size_t part_bytes = sizeof(double) * (size_t)p->n_range * (size_t)p->cap * 2 * (size_t)d1p;
    const int n_planes = by.n_slabs, n_ops = has_ibd(p) ? PCR_N_OPS : PCR_N_OPS_KIN;
    const size_t nn = sizeof(double) * (size_t)(row_end - row_begin) * (size_t)(n_samp - row_begin);
    p->plane_bytes = by.resident;
    const size_t work = by.work;
    size_t free_b = 0, total_b = 0;
    SNPGPU_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (panel && p->plane_bytes + work + PCR_RESERVE_BYTES > free_b)
        return fail(fn, "the device cannot hold this panel: its " + std::to_string(n_planes) + " slabs and two strips take " +
                            std::to_string(p->plane_bytes >> 20) + " MiB and its work buffers " + std::to_string(work >> 20) + " MiB, " +
                            std::to_string(free_b >> 20) + " MiB are free (there is no CPU fallback)");
    if (p->plane_bytes + work + PCR_RESERVE_BYTES > free_b)
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
    const int held[PCR_N_SLABS] = {PCR_RR, PCR_SS, PCR_NS, PCR_DD, PCR_DC, PCR_CC, PCR_IBS0, PCR_K0D, PCR_CD};
    for (int k = 0; k < n_planes; k++) {
        DevBuf &b = p->planes[held[k]];
        if (b.alloc(nn)) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(b.p, 0, nn, s));
    }
    if (panel) {
        const size_t strip = sizeof(double) * (size_t)p->n_pad * PCR_TILE;
        if (p->strip_rr.alloc(strip) || p->strip_ss.alloc(strip)) return 1;
        SNPGPU_HIP_CHECK(hipMemsetAsync(p->strip_rr.p, 0, strip, s));
        SNPGPU_HIP_CHECK(hipMemsetAsync(p->strip_ss.p, 0, strip, s));
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));                  // the host arrays of this call go out of scope
    p->log.on = true;
    guard.p = nullptr;
    *out = p;
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_pcr_create(int64_t n_samp, int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags,
                      const snpgpu_opts *opts, snpgpu_pcr **out)
{
    return create("snpgpu_pcr_create", n_samp, n_pc, pcs, training, maf_thresh, flags, false, 0, n_samp, opts, out);
}

int snpgpu_pcr_create_panel(int64_t n_samp, int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags,
                            int64_t row_begin, int64_t row_end, const snpgpu_opts *opts, snpgpu_pcr **out)
{
    return create("snpgpu_pcr_create_panel", n_samp, n_pc, pcs, training, maf_thresh, flags, true, row_begin, row_end, opts, out);
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
    if (pcr->panel) return fail(fn, "this handle is a row panel: its results are not n x n (snpgpu_pcr_panel_result, snpgpu_pcr_select)");
    if ((k0 || k2) && !has_ibd(pcr)) return fail(fn, "k0 and k2 need a handle created with SNPGPU_PCR_IBD");
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    const PcrPlanes P = plane_ptrs(pcr);
    if (diag_of(pcr)) return 1;
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
    if (pcr->panel) return fail(fn, "this handle is a row panel: its planes are not n x n (snpgpu_pcr_panel_sums)");
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

int snpgpu_pcr_panel_result(snpgpu_pcr *pcr, double *kinship, double *inbreed, double *k0, double *k2, double *nsnp)
{
    const char *fn = "snpgpu_pcr_panel_result";
    if (!pcr) return fail(fn, "NULL argument: pcr is NULL");
    if ((k0 || k2) && !has_ibd(pcr)) return fail(fn, "k0 and k2 need a handle created with SNPGPU_PCR_IBD");
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    const PcrView v = view_of(pcr);
    if (diag_of(pcr)) return 1;
    if (inbreed) SNPGPU_HIP_CHECK(hipMemcpyAsync(inbreed, pcr->inbreed.p, sizeof(double) * (size_t)pcr->n, hipMemcpyDeviceToHost, s));
    double *host[4] = {kinship, k0, k2, nsnp};
    if (kinship || k0 || k2 || nsnp) {
        const int rc = windowed(pcr, 4, host, [&](int64_t r0, int64_t rows, double **dev) {
            return launch_pcr_view_final(s, v, pcr->n, v.row0 + r0, rows, (const double *)pcr->e.p, dev[0], dev[1], dev[2], dev[3]);
        }, v.row1 - v.row0, pcr->n - v.col0);
        if (rc) return 1;
    }
    return fold_log(pcr);
}

int snpgpu_pcr_panel_sums(snpgpu_pcr *pcr, int which, double *plane)
{
    const char *fn = "snpgpu_pcr_panel_sums";
    if (!pcr || !plane) return fail(fn, "NULL argument");
    if (which < 0 || which >= PCR_N_SLABS) return fail(fn, "invalid plane: 0 ... 8 (RR, SS, DD, DC, CC, IBS0, K0D, NS, CD)");
    // (a full handle has no CD slab: its DC holds both halves)
    if (!pcr->planes[which == PCR_CD ? PCR_DC : which].p) return fail(fn, "this plane needs a handle created with SNPGPU_PCR_IBD");
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    const PcrView v = view_of(pcr);
    double *host[1] = {plane};
    const int rc = windowed(pcr, 1, host, [&](int64_t r0, int64_t rows, double **dev) {
        return launch_pcr_view_plane(s, v, which, pcr->n, v.row0 + r0, rows, dev[0]);
    }, v.row1 - v.row0, pcr->n - v.col0);
    if (rc) return 1;
    return fold_log(pcr);
}

int snpgpu_pcr_select(snpgpu_pcr *pcr, const snpgpu_pcr_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2, double *kinship, double *k0,
                      double *k2, double *nsnp, double *inbreed, int64_t *n_found)
{
    const char *fn = "snpgpu_pcr_select";
    if (!pcr) return fail(fn, "NULL argument: pcr is NULL");
    if (!o) return fail(fn, "NULL argument: the options are NULL");
    if (!n_found) return fail(fn, "NULL argument: n_found is NULL");
    if (capacity < 0) return fail(fn, "negative capacity");
    if (capacity == 0 && (idx1 || idx2 || kinship || k0 || k2 || nsnp))
        return fail(fn, "capacity 0 with a non-NULL output (count only: every pair output NULL)");
    if ((k0 || k2) && !has_ibd(pcr)) return fail(fn, "k0 and k2 need a handle created with SNPGPU_PCR_IBD");
    const auto t0 = std::chrono::steady_clock::now();
    SNPGPU_HIP_CHECK(hipSetDevice(pcr->device));
    hipStream_t s = pcr->st.s;
    const int64_t n = pcr->n;
    const PcrView v = view_of(pcr);
    if (diag_of(pcr)) return 1;
    if (inbreed) SNPGPU_HIP_CHECK(hipMemcpyAsync(inbreed, pcr->inbreed.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    // scratch of this call: the sample mask, the segment counts and their offsets
    const PanelGeom g{n, v.row0, v.row1, v.col0, v.row1 - v.row0, v.ld, 0};
    const int64_t n_seg = select_segments(g);
    DevBuf dsel, dcnt, doff;
    if (o->samp_sel) {
        if (dsel.alloc((size_t)n)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(dsel.p, o->samp_sel, (size_t)n, hipMemcpyHostToDevice, s));
    }
    if (dcnt.alloc(sizeof(uint32_t) * (size_t)n_seg) || doff.alloc(sizeof(int64_t) * (size_t)(n_seg + 1))) return 1;
    struct Ev {
        hipEvent_t a = nullptr, b = nullptr;
        ~Ev() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
        double ms() const { float t = 0; return (a && b && hipEventElapsedTime(&t, a, b) == hipSuccess) ? (double)t : 0.0; }
    } ev[3];
    for (Ev &e : ev) { SNPGPU_HIP_CHECK(hipEventCreate(&e.a)); SNPGPU_HIP_CHECK(hipEventCreate(&e.b)); }
    SelectArgs a{(const uint8_t *)(o->samp_sel ? dsel.p : nullptr), o->kinship_cutoff, (uint32_t *)dcnt.p, (int64_t *)doff.p, 0,
                 nullptr, nullptr, nullptr, nullptr, nullptr};
    const double *e = (const double *)pcr->e.p;
    int64_t total = 0;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[0].a, s));
    if (launch_select_pcr(s, v, n, e, false, a, false)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[0].b, s));
    SNPGPU_HIP_CHECK(hipEventRecord(ev[1].a, s));
    if (launch_select_scan(s, (const uint32_t *)dcnt.p, n_seg, (int64_t *)doff.p)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[1].b, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(&total, (const int64_t *)doff.p + n_seg, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    *n_found = total;
    g_pcr_sel_ms[0] = ev[0].ms(); g_pcr_sel_ms[1] = ev[1].ms(); g_pcr_sel_ms[2] = 0.0;
    const int64_t nw = std::min(capacity, total);
    if (nw > 0 && (idx1 || idx2 || kinship || k0 || k2 || nsnp)) {
        // the outputs that are present, of the stored length, on the device; then to the host
        const size_t ni = sizeof(int32_t) * (size_t)nw, nd = sizeof(double) * (size_t)nw;
        void *host[6] = {idx1, idx2, k0, k2, kinship, nsnp};
        DevBuf dev[6];
        for (int k = 0; k < 6; k++)
            if (host[k] && dev[k].alloc(k < 2 ? ni : nd)) return 1;
        a.capacity = nw;
        a.idx1 = (int32_t *)dev[0].p; a.idx2 = (int32_t *)dev[1].p; a.v0 = (double *)dev[2].p; a.v1 = (double *)dev[3].p;
        a.kin = (double *)dev[4].p; a.v2 = (double *)dev[5].p;
        SNPGPU_HIP_CHECK(hipEventRecord(ev[2].a, s));
        if (launch_select_pcr(s, v, n, e, k0 || k2, a, true)) return 1;
        SNPGPU_HIP_CHECK(hipEventRecord(ev[2].b, s));
        for (int k = 0; k < 6; k++)
            if (host[k]) SNPGPU_HIP_CHECK(hipMemcpyAsync(host[k], dev[k].p, k < 2 ? ni : nd, hipMemcpyDeviceToHost, s));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
        g_pcr_sel_ms[2] = ev[2].ms();
    }
    if (fold_log(pcr)) return 1;
    g_pcr_sel_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

/* diagnostics of the last snpgpu_pcr_select of this thread: ms of {count pass, scan, write pass} on the device and of the whole call */
int snpgpu_pcr_select_stats(double *ms4)
{
    if (!ms4) return fail("snpgpu_pcr_select_stats", "NULL output");
    for (int k = 0; k < 4; k++) ms4[k] = g_pcr_sel_ms[k];
    return 0;
}

int snpgpu_pcr_stats(snpgpu_pcr *pcr, double *stats)
{
    const char *fn = "snpgpu_pcr_stats";
    if (!pcr || !stats) return fail(fn, "NULL argument");
    stats[0] = (double)pcr->blocks; stats[1] = (double)pcr->launches;
    for (int k = 0; k <= T_FINAL; k++) stats[2 + k] = pcr->ms[k];
    stats[2 + T_PROD] += pcr->ms[T_CD] + pcr->ms[T_STRIP];
    stats[6] = (double)pcr->plane_bytes; stats[7] = (double)pcr->cap;
    return 0;
}

int snpgpu_pcr_panel_stats(snpgpu_pcr *pcr, double *ms2)
{
    const char *fn = "snpgpu_pcr_panel_stats";
    if (!pcr || !ms2) return fail(fn, "NULL argument");
    ms2[0] = pcr->ms[T_CD]; ms2[1] = pcr->ms[T_STRIP];
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

// The related pairs of the working space without an n x n plane: one panel at a time is created, fed every block as
// snpgpu_gnrPCRelate feeds them, selected from and released; the panels' selections in ascending row order are the global order.
int snpgpu_gnrPCRelatePairs(int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags, int64_t panel_rows,
                            double kinship_cutoff, const uint8_t *samp_sel, int verbose, int64_t *n_found, int64_t *n_panels)
{
    const char *fn = "snpgpu_gnrPCRelatePairs";
    const char *bad_rows = "panel_rows must be a positive multiple of 128, at least the number of samples (one panel), or 0 (as many rows as fit)";
    if (panel_rows < 0) return fail(fn, bad_rows);
    if (need_ws(fn)) return 1;
    const int64_t n = ws_n_samp();
    if (panel_rows > 0 && panel_rows < n && panel_rows % PCR_TILE) return fail(fn, bad_rows);
    if (check_create(fn, n, n_pc, pcs, training, maf_thresh, flags)) return 1;
    g_pairs = PcrPairs();
    snpgpu_opts o{};
    o.device = ws_device();
    const bool ibd = (flags & SNPGPU_PCR_IBD) != 0;
    if (panel_rows == 0) {
        // the largest multiple of 128 whose first (widest) panel fits the free memory together with what snpgpu_pcr_select allocates
        // beside it when every pair of the panel is selected (a non-finite or low cutoff): the selection never fails for memory
        if (use_device(fn, o.device)) return 1;
        size_t free_b = 0, total_b = 0;
        SNPGPU_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        auto fits = [&](int64_t rows) {
            const PcrBytes b = pcr_bytes(n, n_pc, flags, true, 0, std::min(rows, n));
            return b.resident + b.work + select_bytes(n, std::min(rows, n), ibd) + PCR_RESERVE_BYTES <= free_b;
        };
        int64_t lo = 1, hi = up(n, PCR_TILE) / PCR_TILE;            // in tiles; lo is tried whatever the memory (create refuses)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (fits(mid * PCR_TILE)) lo = mid; else hi = mid - 1;
        }
        panel_rows = lo * PCR_TILE;
    }
    const size_t n_s = (size_t)n;
    g_pairs.inbreed.assign(n_s, 0.0);
    int64_t panels = 0;
    for (int64_t r0 = 0; r0 < n; r0 += panel_rows, panels++) {
        const int64_t r1 = std::min(n, r0 + panel_rows);
        struct Guard { snpgpu_pcr *p = nullptr; ~Guard() { if (p) snpgpu_pcr_destroy(p); } } g;
        if (snpgpu_pcr_create_panel(n, n_pc, pcs, training, maf_thresh, flags, r0, r1, &o, &g.p)) return 1;
        if (ws_for_each_block([&](const uint8_t *rows, int64_t, int64_t nb) {
                return snpgpu_pcr_feed(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST, nullptr);
            }))
            return 1;
        snpgpu_pcr_sel_opts so{kinship_cutoff, samp_sel};
        int64_t found = 0, again = 0;
        if (snpgpu_pcr_select(g.p, &so, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, g_pairs.inbreed.data(), &found)) return 1;
        if (verbose) fprintf(stderr, "[snpgpu pcrelate] panel %lld: rows %lld ... %lld, %lld pairs\n", (long long)panels, (long long)r0,
                             (long long)r1, (long long)found);
        if (found == 0) continue;
        const size_t at = g_pairs.idx1.size(), m = at + (size_t)found;
        g_pairs.idx1.resize(m); g_pairs.idx2.resize(m); g_pairs.kin.resize(m); g_pairs.nsnp.resize(m);
        if (ibd) { g_pairs.k0.resize(m); g_pairs.k2.resize(m); }
        if (snpgpu_pcr_select(g.p, &so, found, g_pairs.idx1.data() + at, g_pairs.idx2.data() + at, g_pairs.kin.data() + at,
                              ibd ? g_pairs.k0.data() + at : nullptr, ibd ? g_pairs.k2.data() + at : nullptr, g_pairs.nsnp.data() + at, nullptr,
                              &again))
            return 1;
        if (again != found) return fail(fn, "the selection changed between the count and the fetch");
    }
    if (n_found) *n_found = (int64_t)g_pairs.idx1.size();
    if (n_panels) *n_panels = panels;
    return 0;
}

int snpgpu_gnrPCRelatePairs_get(int32_t *idx1, int32_t *idx2, double *kinship, double *k0, double *k2, double *nsnp, double *inbreed)
{
    const size_t m = g_pairs.idx1.size();
    auto put = [](void *dst, const void *src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    put(idx1, g_pairs.idx1.data(), sizeof(int32_t) * m);
    put(idx2, g_pairs.idx2.data(), sizeof(int32_t) * m);
    put(kinship, g_pairs.kin.data(), sizeof(double) * m);
    put(k0, g_pairs.k0.data(), sizeof(double) * g_pairs.k0.size());
    put(k2, g_pairs.k2.data(), sizeof(double) * g_pairs.k2.size());
    put(nsnp, g_pairs.nsnp.data(), sizeof(double) * m);
    put(inbreed, g_pairs.inbreed.data(), sizeof(double) * g_pairs.inbreed.size());
    return 0;
}

}  // extern "C"

void snpgpu::ws_pcr_pairs_clear() { g_pairs = PcrPairs(); }
