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
// result planes n x n, in the order of snpgpu_pcr_sums; a row panel keeps a ninth slab CD with CD_ij = DC_ji
enum { PCR_RR = 0, PCR_SS = 1, PCR_DD = 2, PCR_DC = 3, PCR_CC = 4, PCR_IBS0 = 5, PCR_K0D = 6, PCR_NS = 7, PCR_N_PLANES = 8, PCR_CD = 8,
       PCR_N_SLABS = 9 };

// One product job: c += x^T y over the block's SNPs.  The product's entry (i, j) (global sample indices) goes to
// c[(i - row0) * ld + (j - col0)] where i < row_end and j < n.  PCR_JOB_TRANSPOSED: the workgroup of grid tile (I, J) computes the
// product's tile (J, I) and stores its entry (j, i) at the destination's (i, j) -- the panel's CD slab, which holds DC's other half
// with DC's own bits.  PCR_JOB_DIAG: workgroup x computes the diagonal tile (x, x) into the strip c[n_pad][PCR_TILE] (col0 = x * PCR_TILE).
enum { PCR_JOB_PLAIN = 0, PCR_JOB_TRANSPOSED = 1, PCR_JOB_DIAG = 2 };
struct PcrJob { const double *x, *y; double *c; int64_t ld, row0, col0, row_end; int mode; };
struct PcrJobs { PcrJob j[8]; };
struct PcrPlanes { const double *p[PCR_N_PLANES]; };    // NULL: not accumulated

// How the finaliser and the selection read the resident sums of a full object (the panel [0, n)) or of a row panel: the entry
// (i, j) of a slab is p[(i - row0) * ld + (j - col0)], rows [row0, row1), columns [col0, n).  A full object has no CD slab: its DC
// holds both halves.
struct PcrView {
    const double *p[PCR_N_SLABS];                       // NULL: not accumulated
    int64_t ld, row0, row1, col0;
    __host__ __device__ __forceinline__ double at(int k, int64_t i, int64_t j) const { return p[k][(i - row0) * ld + (j - col0)]; }
    // a plane that holds the tiles I <= J only
    __host__ __device__ __forceinline__ double sym(int k, int64_t i, int64_t j) const { return i <= j ? at(k, i, j) : at(k, j, i); }
    // DC_ij, from the CD slab where row i is not resident (so only CD's columns >= row1 are ever read, and only they are computed)
    __host__ __device__ __forceinline__ double dc(int64_t i, int64_t j) const
    {
        return (!p[PCR_CD] || (i >= row0 && i < row1)) ? at(PCR_DC, i, j) : at(PCR_CD, j, i);
    }
};

// The finaliser's expressions at (i, j), written as the definitions read (no contraction); e: 1 + inbreed of every sample; k0 / k2
// only with `probs` (they need the IBD slabs).  One of i, j is a resident row and both are >= col0.
__device__ __forceinline__ void pcr_pair_values(const PcrView &v, const double *__restrict__ e, int64_t i, int64_t j, bool probs, double &kin,
                                                double &k0, double &k2)
{
#pragma clang fp contract(off)
    kin = v.sym(PCR_RR, i, j) / (4.0 * v.sym(PCR_SS, i, j));
    if (!probs) return;
    const double ei = e[i], ej = e[j], cc = v.sym(PCR_CC, i, j);
    k2 = (v.sym(PCR_DD, i, j) - ej * v.dc(i, j) - ei * v.dc(j, i) + ei * ej * cc) / cc;
    k0 = kin < PCR_KIN_SPLIT ? v.sym(PCR_IBS0, i, j) / v.sym(PCR_K0D, i, j) : 1.0 - 4.0 * kin + k2;
}

// part: n_range * m * 2 * d1p doubles, cnt: n_range * m * 2 counters (scratch); n_range * range_bytes >= ceil(n / 4)
int launch_pcr_beta(hipStream_t st, const uint8_t *rows, int64_t rb, int m, int64_t n, const uint8_t *train, const double *W, int d1p, int d1,
                    int n_range, int64_t range_bytes, double *part, int32_t *cnt, double *beta, int32_t *num);
int launch_pcr_operands(hipStream_t st, const uint8_t *rows, int64_t rb, int m, int64_t n, int64_t n_pad, const double *beta,
                        const int32_t *num, int d1, const double *Vt, double lo, double hi, int n_planes, double *ops, int64_t plane_stride);
// grid tiles (tile0 + y, tile0_col + x), y < nt_rows, x < nt_cols (a full object: 0 and n_pad / PCR_TILE twice); tri: only I <= J
int launch_pcr_products(hipStream_t st, const PcrJobs &jobs, int n_jobs, int64_t n, int64_t n_pad, int m, bool tri, int tile0, int nt_rows,
                        int tile0_col, int nt_cols);
// RR_ii = RR[i * ld + (wrap ? i % wrap : i)]: a full plane (ld = n, wrap = 0) or a strip of diagonal tiles (ld = wrap = PCR_TILE)
int launch_pcr_diag(hipStream_t st, const double *RR, const double *SS, int64_t n, int64_t ld, int64_t wrap, double *inbreed, double *e);
int launch_pcr_final(hipStream_t st, const PcrPlanes &P, int64_t n, int64_t r0, int64_t rows, const double *e, double *kinship, double *k0,
                     double *k2, double *nsnp);
int launch_pcr_plane(hipStream_t st, const double *P, int64_t n, bool sym, int64_t r0, int64_t rows, double *out);
// the same two through a view: rows [r0, r0 + rows) x columns [col0, n) of the results ([rows][n - col0] each, any may be NULL) and
// of slab `which` (PCR_CD: DC transposed, whatever the view holds it in)
int launch_pcr_view_final(hipStream_t st, const PcrView &v, int64_t n, int64_t r0, int64_t rows, const double *e, double *kinship, double *k0,
                          double *k2, double *nsnp);
int launch_pcr_view_plane(hipStream_t st, const PcrView &v, int which, int64_t n, int64_t r0, int64_t rows, double *out);

// The selection of related pairs from the resident sums (kernels_select.hip: the walk of every selection): rows [v.row0, v.row1),
// the values of pcr_view_final_kernel at (idx2, idx1); s.v0 = k0, s.v1 = k2 (probs: only then evaluated), s.kin = kinship, s.v2 = nsnp
struct SelectArgs;
int launch_select_pcr(hipStream_t st, const PcrView &v, int64_t n, const double *e, bool probs, const SelectArgs &s, bool write);

}  // namespace snpgpu
