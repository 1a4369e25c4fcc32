// The dense route to the top-k eigenpairs of a context's matrix (hipSOLVER syevd on an n x n copy), the choice between it and the
// block-Krylov solver of eigen.hip, and snpgpu_pca_eigen, the level-1 call behind gnrPCA.
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx_plan.h"
#include "eigen.h"

using namespace snpgpu;

namespace {

__global__ void negate_kernel(double *a, size_t n)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = -a[i];
}

// samples up to which the dense solver is used (the reference's own route: exact to LAPACK's tolerance, O(n^3)); beyond it
// the block-Krylov solver works on the resident panel, without an n x n copy.  The threshold dates from syevdx (4 s at n = 4096,
// 21 s at 8192, 124 s at 16 384 and 210 s at 20 000 on an MI355X, round 3); the syevd that replaced it takes 0.014 s at n = 540
// and 0.056 s at 2048 (syevdx: 0.070 and 0.89 s) and has not been measured beyond 2304: the threshold stays where it was.
int64_t dense_eigen_max()
{
    if (const char *e = getenv("SNPGPU_EIG_DENSE_MAX")) { const long long v = atoll(e); if (v >= 0 && v <= 46340) return v; }
    return 2048;
}

}  // namespace

namespace snpgpu {

// top-k eigenpairs of a dense symmetric matrix A (device, n x n, overwritten): the reference negates
// the packed matrix and asks LAPACK dspevx for eigenvalues IL=1..IU=k (src/genPCA.cpp:1308-1341,
// :1419; src/genEIGMIX.cpp:700-702); here A is negated on the device, hipSOLVER's syevd decomposes it
// whole and the first k pairs (ascending in -A) are the answer.  NOT syevdx with that index range: on
// multiple eigenvalues (copies of one block of samples: clusters that the fp32 parts of the accumulation
// split by 1e-7) it returned, now and then, a value from elsewhere in the spectrum with a vector that is
// no eigenvector at all -- relative residual of order 1, at k = 1 as at k = 16, INFO = 0
// (tests/test_gpu_eigen_spectra.py); syevd, which also serves the Krylov solver's projected matrices, is
// exact there.  eigval: k values (descending), eigvec: n x k column-major.
int dense_topk(int device, hipStream_t stream, double *A, int64_t n, int k, double *eigval, double *eigvec, int mem)
{
    if (k <= 0 || k > n) { set_error("Invalid 'eigen.cnt'."); return 1; }
    if (n > 46340) { set_error("dense eigen solver limited to n <= 46340 (larger n take the block-Krylov solver, csrc/eigen.hip)"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    DevBuf W, work, info;
    SolverHandle sv;
    if (W.alloc(sizeof(double) * (size_t)n) | info.alloc(sizeof(int))) return 1;
    const size_t nn = (size_t)n * (size_t)n;
    hipLaunchKernelGGL(negate_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, stream, A, nn);
    if (hipStreamSynchronize(stream) != hipSuccess) { set_error("dense_topk: negate failed"); return 1; }
    if (hipsolverCreate(&sv.h) != HIPSOLVER_STATUS_SUCCESS) { set_error("hipsolverCreate failed"); return 1; }
    hipsolverSetStream(sv.h, stream);
    int lwork = 0;
    if (hipsolverDnDsyevd_bufferSize(sv.h, HIPSOLVER_EIG_MODE_VECTOR, HIPSOLVER_FILL_MODE_LOWER, (int)n, A, (int)n, (double *)W.p,
                                     &lwork) != HIPSOLVER_STATUS_SUCCESS) {
        // (a workspace size that does not fit the interface) -- the callers fall back to the block-Krylov solver
        set_error("hipsolverDnDsyevd_bufferSize failed");
        return 2;
    }
    if (work.alloc(sizeof(double) * (size_t)std::max(lwork, 1))) return 1;
    hipsolverStatus_t s = hipsolverDnDsyevd(sv.h, HIPSOLVER_EIG_MODE_VECTOR, HIPSOLVER_FILL_MODE_LOWER, (int)n, A, (int)n,
                                            (double *)W.p, (double *)work.p, lwork, (int *)info.p);
    int hinfo = 0;
    hipError_t e = hipMemcpyAsync(&hinfo, info.p, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (s != HIPSOLVER_STATUS_SUCCESS || e != hipSuccess || hinfo != 0) {
        // message of src/genPCA.cpp:1333
        set_error("LAPACK::DSPEVX error (" + std::to_string(hinfo) +
                  "), infinite or missing values in the genetic covariance matrix!");
        return 1;
    }
    std::vector<double> w((size_t)k);
    if (hipMemcpy(w.data(), W.p, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost) != hipSuccess) { set_error("eigen copy failed"); return 1; }
    for (int i = 0; i < k; i++) w[(size_t)i] = -w[(size_t)i];
    if (eigval) memcpy(eigval, w.data(), sizeof(double) * (size_t)k);      // always host memory, as the Krylov route
    const hipMemcpyKind kv = (mem == SNPGPU_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (eigvec && hipMemcpy(eigvec, A, sizeof(double) * (size_t)n * (size_t)k, kv) != hipSuccess) { set_error("eigen copy failed"); return 1; }
    return 0;
}

// A request for a large share of the spectrum (eigen.cnt <= 0 = all, eigen.method = "DSPEV", or k of the order of n) is not a
// top-k problem: the Krylov solver's block would be k + 8 vectors wide with room for one or two blocks per cycle (n = 3000,
// k = 1000: one new block per restart), and with k = n it degenerates to a full QR + syevd inside six n x n work arrays.  Up to
// 16 384 samples such requests take the dense route whatever SNPGPU_EIG_DENSE_MAX says.
bool dense_route(int64_t n, int k)
{
    if (n <= dense_eigen_max()) return true;
    return n <= 16384 && (int64_t)k * 8 > n;
}

// the (n - 1) / trace factor of the iterative route, checked as LAPACK would report such a matrix (src/genPCA.cpp:1333)
int krylov_scale(snpgpu_ctx *c, double *scale)
{
    double tr = 0;
    if (snpgpu_pca_panel_trace(c, &tr)) return 1;
    if (!(tr > 0) || !std::isfinite(tr)) {
        snpgpu::set_error("LAPACK::DSPEVX error (-1), infinite or missing values in the genetic covariance matrix!");
        return 1;
    }
    *scale = (double)(c->plan.N - 1) / tr;
    return 0;
}

int ctx_topk_eigen(snpgpu_ctx *c, int k, const std::function<int(double *A)> &fill_dense,
                   const std::function<int(double *scale)> &prepare_panel, double *eigval, double *eigvec, int mem)
{
    const int64_t n = c->plan.N;
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    if (dense_route(n, k)) {
        int rc;
        {
            DevBuf A;           // gone before the Krylov solver allocates its own work arrays
            if (A.alloc(sizeof(double) * (size_t)n * (size_t)n)) return 1;
            rc = fill_dense((double *)A.p);
            if (!rc) rc = dense_topk(c->device, c->stream, (double *)A.p, n, k, eigval, eigvec, mem);
        }
        if (rc != 2) return rc;
        set_error("");          // the dense solver declined this size (the declined workspace query is not this call's outcome)
    }
    // block Krylov on the resident panel
    double scale = 0;
    if (prepare_panel(&scale)) return 1;
    snpgpu_ctx *panels[1] = {c};
    return snpgpu_panels_topk_eigen(panels, 1, scale, k, nullptr, eigval, eigvec, mem, nullptr);
}

}  // namespace snpgpu

extern "C" int snpgpu_pca_eigen(snpgpu_ctx *c, int k, double *eigval, double *eigvec, int mem)
{
    if (!c || c->plan.kind != SNPGPU_PCA_COV || !c->plan.full) { set_error("snpgpu_pca_eigen: needs a full PCA_COV context"); return 1; }
    if (k <= 0 || k > c->plan.N) { set_error("Invalid 'eigen.cnt'."); return 1; }
    return ctx_topk_eigen(
        c, k, [c](double *A) { return snpgpu_pca_cov(c, A, 0, 1, 0.0, nullptr, SNPGPU_DEVICE); },
        [c](double *scale) { return krylov_scale(c, scale); }, eigval, eigvec, mem);
}
