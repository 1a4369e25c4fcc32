// What kernels_pcrelate.hip and its host layer pcrelate.hip share: tile geometry, the order of the operand and result planes, the
// launch declarations.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace snpgpu {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PCR_TILE = 128;       // output tile of one workgroup; n_pad is a multiple of it
constexpr int PCR_KB = 16;          // SNP rows staged in LDS per step
constexpr int PCR_KC = 8;           // columns of beta per pass of the beta kernel
constexpr int PCR_MAX_PC = 32;
constexpr double PCR_KIN_SPLIT = 0.17677669529663688110;       // 2^(-5/2): below it k0 = IBS0 / K0D

// operand planes [m][n_pad]; the first three are all a handle without SNPGPU_PCR_IBD needs
enum { PCR_OP_R = 0, PCR_OP_S = 1, PCR_OP_O = 2, PCR_OP_GD = 3, PCR_OP_C = 4, PCR_OP_I0 = 5, PCR_OP_I2 = 6, PCR_OP_A = 7, PCR_OP_B = 8,
       PCR_N_OPS = 9, PCR_N_OPS_KIN = 3 };
// result planes n x n, in the order of snpgpu_pcr_sums
enum { PCR_RR = 0, PCR_SS = 1, PCR_DD = 2, PCR_DC = 3, PCR_CC = 4, PCR_IBS0 = 5, PCR_K0D = 6, PCR_NS = 7, PCR_N_PLANES = 8 };

struct PcrJob { const double *x, *y; double *c; };      // c += x^T y
struct PcrJobs { PcrJob j[8]; };
struct PcrPlanes { const double *p[PCR_N_PLANES]; };    // NULL: not accumulated

// part: n_range * m * 2 * d1p doubles, cnt: n_range * m * 2 counters (scratch); n_range * range_bytes >= ceil(n / 4)
int launch_pcr_beta(hipStream_t st, const uint8_t *rows, int64_t rb, int m, int64_t n, const uint8_t *train, const double *W, int d1p, int d1,
                    int n_range, int64_t range_bytes, double *part, int32_t *cnt, double *beta, int32_t *num);
int launch_pcr_operands(hipStream_t st, const uint8_t *rows, int64_t rb, int m, int64_t n, int64_t n_pad, const double *beta,
                        const int32_t *num, int d1, const double *Vt, double lo, double hi, int n_planes, double *ops, int64_t plane_stride);
int launch_pcr_products(hipStream_t st, const PcrJobs &jobs, int n_jobs, int64_t n, int64_t n_pad, int m, bool tri);
int launch_pcr_diag(hipStream_t st, const PcrPlanes &P, int64_t n, double *inbreed, double *e);
int launch_pcr_final(hipStream_t st, const PcrPlanes &P, int64_t n, int64_t r0, int64_t rows, const double *e, double *kinship, double *k0,
                     double *k2, double *nsnp);
int launch_pcr_plane(hipStream_t st, const double *P, int64_t n, bool sym, int64_t r0, int64_t rows, double *out);

}  // namespace snpgpu
