// Internal interface of the top-k eigen solver (eigen.hip) shared with the multi-device driver (multi.hip), and of the dense
// route (eigen_dense.hip) shared with the working space (workspace.hip, pca_randomized.hip).
#pragma once
#include <hipsolver/hipsolver.h>

#include <functional>
#include <vector>

#include "snpgpu_internal.h"

namespace snpgpu {

// y = scale * C q for blocks of vectors stored vector-major: Q, Y = double [b][n] on device(); apply() overwrites Y and
// returns when Y is complete.  fp32_products: the solver accepts a product with relative error ~1e-7 (kernels_eig.hip)
struct EigOperator {
    virtual ~EigOperator() {}
    virtual int64_t n() const = 0;
    virtual int device() const = 0;
    virtual int apply(const double *Q, int b, double *Y, bool fp32_products) = 0;
    virtual bool has_fp32_products() const { return true; }
};

// row panels resident on ONE device (a whole matrix, or one rank's share of it: then `reduce` sums `y_buf` over the ranks)
class PanelsOperator : public EigOperator {
public:
    PanelsOperator(const std::vector<snpgpu_ctx *> &panels, int64_t n, int device, double scale, double *y_buf,
                   snpgpu_reduce_fn reduce, void *user)
        : panels_(panels), n_(n), dev_(device), scale_(scale), y_buf_(y_buf), reduce_(reduce), user_(user) {}
    int64_t n() const override { return n_; }
    int device() const override { return dev_; }
    int apply(const double *Q, int b, double *Y, bool fp32_products) override;
    bool has_fp32_products() const override { return getenv("SNPGPU_EIG_BLAS") == nullptr; }      // not the two-dgemm form

private:
    std::vector<snpgpu_ctx *> panels_;
    int64_t n_;
    int dev_;
    double scale_;
    double *y_buf_;
    snpgpu_reduce_fn reduce_;
    void *user_;
};

// largest-k eigenpairs: eigval_host [k] descending (host), eigvec [k][n] = column-major n x k (`mem`: host or op.device())
int krylov_topk(EigOperator &op, int k, const snpgpu_eig_opts *opts, double *eigval_host, double *eigvec, int mem,
                snpgpu_eig_info *info);

struct SolverHandle {      // owns a hipSOLVER handle; declare it AFTER the buffers the handle is given, so that it goes first
    hipsolverHandle_t h = nullptr;
    ~SolverHandle() { if (h) hipsolverDestroy(h); }
};

// ---- the dense route (eigen_dense.hip) ----
// top-k eigenpairs of a dense symmetric matrix A (device, n x n, overwritten) by hipSOLVER's syevd.  eigval: k values (descending,
// host), eigvec: n x k column-major in `mem`.  Returns 2 where the solver declines the size (the caller takes the Krylov solver).
int dense_topk(int device, hipStream_t stream, double *A, int64_t n, int k, double *eigval, double *eigvec, int mem);
bool dense_route(int64_t n, int k);         // whether n samples / k eigenpairs take the dense solver
int krylov_scale(snpgpu_ctx *c, double *scale);

// Top-k eigenpairs of a context's finalised matrix by whichever route dense_route picks.  fill_dense(A) writes the dense n x n
// matrix to the device pointer A; prepare_panel(&scale) readies the resident panel for the Krylov solver and yields its scale
// (also called when the dense solver declines the size).  eigval: k values on the host, eigvec: n x k column-major in `mem`.
int ctx_topk_eigen(snpgpu_ctx *c, int k, const std::function<int(double *A)> &fill_dense,
                   const std::function<int(double *scale)> &prepare_panel, double *eigval, double *eigvec, int mem);

}  // namespace snpgpu
