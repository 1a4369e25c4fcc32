// C ABI of libsnpgpu, classical multidimensional scaling (include/snpgpu.h section 1q): what snpgdsMDS needs.  The k algebraically
// largest eigenpairs of B = -1/2 J (D o D) J for a symmetric n x n distance matrix D in host or device memory.  Up to the dense
// threshold (dense_route, as for PCA) B is written out and decomposed whole; beyond it the block-Krylov solver of eigen.hip works
// on the operator q -> B q, which reads D as it lies: B is never formed and the caller's matrix never written.
// All argument errors are found before any device is touched; the input's own faults (a non-finite entry, asymmetry) by the scan.
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "eigen.h"
#include "host_util.h"
#include "workspace.h"

namespace snpgpu {
int64_t mds_tiles(int64_t n);
int mds_splits(int64_t n);
int launch_mds_scan(hipStream_t st, const double *D, int64_t ld, int64_t n, double *part, double *rowsum, double *totals, int *flags);
int launch_mds_operator(hipStream_t st, const double *D, int64_t ld, int64_t n, const double *Q, int m, double *Y, double *Wc, double *Zp);
int launch_mds_centre(hipStream_t st, const double *D, int64_t ld, int64_t n, const double *rowsum, const double *totals, double *B);
int launch_mds_one_minus(hipStream_t st, double *d, size_t count);
}  // namespace snpgpu

using namespace snpgpu;

namespace {

// ms of staging, of the scan, of the eigen solve, of the whole call; the route; operator products and their summed ms; staging
// windows; the value at or below which an eigenvalue counts as not positive
thread_local double g_stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

constexpr size_t MDS_STAGE_BYTES = size_t(256) << 20;      // host rows go to the device in copies of at most this
constexpr int MDS_MAX_VEC = 48;                            // vectors of one product launch: the solver's widest block
enum { T_STAGE = 0, T_SCAN = 1, T_APPLY = 2 };

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// q -> B q on the device matrix: centre, multiply by D o D, centre and halve
class MdsOperator : public EigOperator {
public:
    MdsOperator(Call &c, const double *D, int64_t ld, int64_t n, int device) : c_(c), D_(D), ld_(ld), n_(n), dev_(device) {}
    static size_t scratch_bytes(int64_t n) { return sizeof(double) * (size_t)MDS_MAX_VEC * (size_t)n * (size_t)(mds_splits(n) + 2); }
    int init()
    {
        int rc = 0;
        DevBuf *w = c_.bufs.get(sizeof(double) * (size_t)MDS_MAX_VEC * (size_t)n_, rc);
        DevBuf *z = c_.bufs.get(sizeof(double) * (size_t)MDS_MAX_VEC * (size_t)n_ * (size_t)(mds_splits(n_) + 1), rc);
        if (rc) return 1;
        wc_ = (double *)w->p; zp_ = (double *)z->p;
        return 0;
    }
    int64_t n() const override { return n_; }
    int device() const override { return dev_; }
    bool has_fp32_products() const override { return false; }
    int apply(const double *Q, int b, double *Y, bool) override
    {
        SNPGPU_HIP_CHECK(hipSetDevice(dev_));
        hipStream_t s = c_.st.s;
        if (c_.log.begin(T_APPLY, s)) return 1;
        for (int v0 = 0; v0 < b; v0 += MDS_MAX_VEC) {
            const int m = std::min(MDS_MAX_VEC, b - v0);
            if (launch_mds_operator(s, D_, ld_, n_, Q + (int64_t)v0 * n_, m, Y + (int64_t)v0 * n_, wc_, zp_)) return 1;
        }
        if (c_.log.end(s)) return 1;
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
        products++;
        return 0;
    }
    int64_t products = 0;

private:
    Call &c_;
    const double *D_;
    int64_t ld_, n_;
    int dev_;
    double *wc_ = nullptr, *zp_ = nullptr;
};

int check_matrix_args(const char *fn, const double *dist, int64_t n, int64_t ld, int mem)
{
    if (!dist) return fail(fn, "NULL argument: dist is NULL");
    if (n < 2) return fail(fn, "invalid number of samples: 'd' must have at least two rows");
    if (n >= (int64_t(1) << 31)) return fail(fn, "invalid number of samples");
    if (ld < n) return fail(fn, "invalid leading dimension: ld < n");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE && mem != SNPGPU_HOST_PINNED) return fail(fn, "invalid memory kind");
    return 0;
}

// the solver's device memory: the Krylov solver at its shortest cycle (eigen.hip halves its depth down to 4 where the device is
// short: 12 blocks of b vectors) and the operator's scratch, or the dense route's B, eigenvectors and syevd's work
size_t solver_bytes(int64_t n, int k)
{
    if (dense_route(n, k)) return sizeof(double) * 5 * (size_t)n * (size_t)n;
    const size_t b = (size_t)std::min<int64_t>(n, (k + 8 + 15) / 16 * 16);
    return sizeof(double) * 12 * b * (size_t)n + MdsOperator::scratch_bytes(n);
}

// The matrix on the device: the caller's where it lies there, else a copy of leading dimension n made in row windows.
int stage_matrix(const char *fn, Call &c, const double *dist, int64_t n, int64_t ld, int mem, size_t solver, const double **D, int64_t *ldD,
                 int64_t *windows)
{
    const size_t nn = sizeof(double) * (size_t)n * (size_t)n, scan = sizeof(double) * (size_t)n * (size_t)(mds_tiles(n) + 1);
    const size_t matrix = mem == SNPGPU_DEVICE ? 0 : nn;
    size_t free_b = 0, total_b = 0;
    SNPGPU_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (matrix + scan + solver + (size_t(64) << 20) > free_b)
        return fail(fn, "the device cannot hold this call: the matrix takes " + std::to_string(nn >> 20) + " MiB" +
                            (matrix ? "" : " (in place)") + " and the solver's work " + std::to_string((scan + solver) >> 20) + " MiB, " +
                            std::to_string(free_b >> 20) + " MiB are free (there is no CPU fallback)");
    *windows = 0;
    if (mem == SNPGPU_DEVICE) { *D = dist; *ldD = ld; return 0; }
    int rc = 0;
    DevBuf *d = c.bufs.get(nn, rc);
    if (rc) return 1;
    const size_t row_bytes = sizeof(double) * (size_t)n;
    const int64_t rows_max = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(env_bytes("SNPGPU_MDS_STAGE_BYTES", MDS_STAGE_BYTES) / row_bytes)));
    hipStream_t s = c.st.s;
    for (int64_t r0 = 0; r0 < n; r0 += rows_max) {
        const int64_t rows = std::min(rows_max, n - r0);
        if (c.log.begin(T_STAGE, s)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpy2DAsync((double *)d->p + r0 * n, row_bytes, dist + r0 * ld, sizeof(double) * (size_t)ld, row_bytes, (size_t)rows,
                                          hipMemcpyHostToDevice, s));
        if (c.log.end(s)) return 1;
        (*windows)++;
    }
    *D = (const double *)d->p; *ldD = n;
    return 0;
}

struct Scan {
    const double *rowsum = nullptr, *totals = nullptr;     // device
    double total = 0, diag = 0, max_row = 0;
};

int scan_matrix(const char *fn, Call &c, const double *D, int64_t ld, int64_t n, Scan *out)
{
    int rc = 0;
    DevBuf *rs = c.bufs.get(sizeof(double) * (size_t)n, rc), *tot = c.bufs.get(sizeof(double) * 3, rc), *fl = c.bufs.get(sizeof(int) * 2, rc);
    if (rc) return 1;
    hipStream_t s = c.st.s;
    int flags[2] = {0, 0};
    double totals[3] = {0, 0, 0};
    {
        DevBuf part;                                           // the per-tile partial sums live for the scan only
        if (part.alloc(sizeof(double) * (size_t)n * (size_t)mds_tiles(n))) return 1;
        if (c.log.begin(T_SCAN, s) ||
            launch_mds_scan(s, D, ld, n, (double *)part.p, (double *)rs->p, (double *)tot->p, (int *)fl->p) || c.log.end(s))
            return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(flags, fl->p, sizeof(flags), hipMemcpyDeviceToHost, s));
        SNPGPU_HIP_CHECK(hipMemcpyAsync(totals, tot->p, sizeof(totals), hipMemcpyDeviceToHost, s));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (flags[0]) return fail(fn, "NA values not allowed in 'd'");
    if (flags[1]) return fail(fn, "'d' must be exactly symmetric: d[i][j] and d[j][i] differ for at least one pair");
    out->rowsum = (const double *)rs->p; out->totals = (const double *)tot->p;
    out->total = totals[0]; out->diag = totals[1]; out->max_row = totals[2];
    return 0;
}

// in every vector the entry of largest magnitude (the lowest index on ties) is positive
void sign_rule(double *vectors, int k, int64_t n)
{
    for (int v = 0; v < k; v++) {
        double *x = vectors + (int64_t)v * n;
        int64_t at = 0;
        for (int64_t i = 1; i < n; i++)
            if (std::fabs(x[i]) > std::fabs(x[at])) at = i;
        if (x[at] < 0)
            for (int64_t i = 0; i < n; i++) x[i] = -x[i];
    }
}

int finish_stats(Call &c, double t0, int route, int64_t products, int64_t windows, double eig_ms, double pos_tol)
{
    if (c.log.sum_ms(T_STAGE, &g_stats[0]) || c.log.sum_ms(T_SCAN, &g_stats[1]) || c.log.sum_ms(T_APPLY, &g_stats[6])) return 1;
    g_stats[2] = eig_ms; g_stats[3] = now_ms() - t0; g_stats[4] = route; g_stats[5] = (double)products; g_stats[7] = (double)windows;
    g_stats[8] = pos_tol;
    return 0;
}

int mds(const char *fn, const double *dist, int64_t n, int64_t ld, int mem, int k, double *eigval, double *vectors, double *all_eigval,
        double *trace_b, int *route_out, int device)
{
    if (check_matrix_args(fn, dist, n, ld, mem)) return 1;
    if (!eigval || !vectors) return fail(fn, "NULL argument: eigval and vectors are required");
    if (k < 1 || k > n - 1) return fail(fn, "'k' must be in {1, 2, ..  n - 1}");
    for (double &s : g_stats) s = 0;
    const double t0 = now_ms();
    Call c;
    if (c.open_on(fn, device, nullptr, {mem == SNPGPU_DEVICE ? dist : nullptr})) return 1;
    hipStream_t s = c.st.s;
    const double *D = nullptr;
    int64_t ldD = 0, windows = 0;
    if (stage_matrix(fn, c, dist, n, ld, mem, solver_bytes(n, k), &D, &ldD, &windows)) return 1;
    Scan sc;
    if (scan_matrix(fn, c, D, ldD, n, &sc)) return 1;
    if (trace_b) *trace_b = (sc.total / (double)n - sc.diag) / 2;
    // |B|_2 <= |D o D|_inf / 2, and n eps of that is what rounding makes of an eigenvalue that is exactly zero (B 1 = 0 always):
    // eigenvalues at or below it are not counted as positive, by either route
    const double pos_tol = (double)n * std::ldexp(1.0, -52) * sc.max_row / 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double t_eig = now_ms();
    int route = 1;
    if (dense_route(n, k)) {
        int rc = 0;
        {
            DevBuf A, V;                                   // gone before the Krylov solver allocates its own work arrays
            const size_t nn = sizeof(double) * (size_t)n * (size_t)n;
            if (A.alloc(nn) || V.alloc(nn)) return 1;
            if (launch_mds_centre(s, D, ldD, n, sc.rowsum, sc.totals, (double *)A.p)) return 1;
            std::vector<double> w((size_t)n);
            rc = dense_topk(device, s, (double *)A.p, n, (int)n, w.data(), (double *)V.p, SNPGPU_DEVICE);
            if (!rc) {
                SNPGPU_HIP_CHECK(hipMemcpy(vectors, V.p, sizeof(double) * (size_t)k * (size_t)n, hipMemcpyDeviceToHost));
                memcpy(eigval, w.data(), sizeof(double) * (size_t)k);
                if (all_eigval) memcpy(all_eigval, w.data(), sizeof(double) * (size_t)n);
                route = 0;
            }
        }
        if (rc && rc != 2) return 1;
        if (rc == 2) set_error("");                        // the dense solver declined this size: the Krylov solver takes it
    }
    int64_t products = 0;
    if (route == 1) {
        MdsOperator op(c, D, ldD, n, device);
        if (op.init()) return 1;
        snpgpu_eig_info info{};
        const int rc = krylov_topk(op, k, nullptr, eigval, vectors, SNPGPU_HOST, &info);
        products = op.products;
        bool positive = !rc;
        for (int i = 0; positive && i < k; i++) positive = eigval[i] > pos_tol;
        // The solver accepts on |B v - theta v| / |theta|, which says nothing at theta ~ 0: a pair it could not settle, or one at
        // or below zero, is not returned
        if ((rc && info.restarts > 0) || (!rc && !positive))
            return fail(fn, "fewer than k = " + std::to_string(k) + " eigenvalues appear to be positive at n = " + std::to_string(n) +
                                ": the iterative solver of this size cannot settle eigenvalues at or below zero; ask for a smaller k");
        if (rc) return 1;
        if (all_eigval)
            for (int64_t i = 0; i < n; i++) all_eigval[i] = nan;
    }
    sign_rule(vectors, k, n);
    if (route_out) *route_out = route;
    return finish_stats(c, t0, route, products, windows, now_ms() - t_eig, pos_tol);
}

}  // namespace

extern "C" {

int snpgpu_mds(const double *dist, int64_t n, int64_t ld, int mem, int k, double *eigval, double *vectors, double *all_eigval,
               double *trace_b, int *route, int device)
{
    return mds("snpgpu_mds", dist, n, ld, mem, k, eigval, vectors, all_eigval, trace_b, route, device);
}

int snpgpu_mds_apply(const double *dist, int64_t n, int64_t ld, int mem, const double *Q, int b, double *Y, int device)
{
    const char *fn = "snpgpu_mds_apply";
    if (check_matrix_args(fn, dist, n, ld, mem)) return 1;
    if (!Q || !Y) return fail(fn, "NULL argument: Q and Y are required");
    if (b < 1) return fail(fn, "invalid number of vectors");
    for (double &s : g_stats) s = 0;
    const double t0 = now_ms();
    Call c;
    if (c.open_on(fn, device, nullptr, {mem == SNPGPU_DEVICE ? dist : nullptr})) return 1;
    hipStream_t s = c.st.s;
    const double *D = nullptr;
    int64_t ldD = 0, windows = 0;
    const size_t qb = sizeof(double) * (size_t)b * (size_t)n;
    if (stage_matrix(fn, c, dist, n, ld, mem, MdsOperator::scratch_bytes(n) + 2 * qb, &D, &ldD, &windows)) return 1;
    Scan sc;
    if (scan_matrix(fn, c, D, ldD, n, &sc)) return 1;
    MdsOperator op(c, D, ldD, n, device);
    int rc = 0;
    DevBuf *dq = c.bufs.get(qb, rc), *dy = c.bufs.get(qb, rc);
    if (rc || op.init()) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dq->p, Q, qb, hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    const double t_eig = now_ms();
    if (op.apply((const double *)dq->p, b, (double *)dy->p, false)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(Y, dy->p, qb, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return finish_stats(c, t0, 1, op.products, windows, now_ms() - t_eig, 0.0);
}

int snpgpu_gnrMDS(int what, int k, double *eigval, double *vectors, double *all_eigval, double *trace_b, int *route)
{
    const char *fn = "snpgpu_gnrMDS";
    if (need_ws(fn)) return 1;
    if (what != 0 && what != 1) return fail(fn, "invalid 'what': 0 = 1 - IBS, 1 = individual dissimilarity");
    if (!eigval || !vectors) return fail(fn, "NULL argument: eigval and vectors are required");
    const int64_t n = ws_n_samp();
    if (n < 2) return fail(fn, "invalid number of samples: 'd' must have at least two rows");
    if (k < 1 || k > n - 1) return fail(fn, "'k' must be in {1, 2, ..  n - 1}");
    const int device = ws_device();
    DevBuf dist;
    {
        struct Guard { snpgpu_ctx *c = nullptr; ~Guard() { if (c) snpgpu_destroy(c); } } g;    // gone before the solve
        if (ws_run_stream(what == 0 ? SNPGPU_IBS : SNPGPU_DISS, 0, &g.c)) return 1;
        if (dist.alloc(sizeof(double) * (size_t)n * (size_t)n)) return 1;
        if (what == 0 ? snpgpu_ibs_ave(g.c, (double *)dist.p, 0, SNPGPU_DEVICE) : snpgpu_diss(g.c, (double *)dist.p, 0, SNPGPU_DEVICE)) return 1;
        if (snpgpu_sync(g.c)) return 1;
        if (what == 0) {
            CallStream st;
            if (st.open(fn, device) || launch_mds_one_minus(st.s, (double *)dist.p, (size_t)n * (size_t)n)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(st.s));
        }
    }
    return mds(fn, (const double *)dist.p, n, n, SNPGPU_DEVICE, k, eigval, vectors, all_eigval, trace_b, route, device);
}

int snpgpu_mds_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_mds_stats: stats is NULL"); return 1; }
    for (int i = 0; i < 9; i++) stats[i] = g_stats[i];
    return 0;
}

}  // extern "C"
