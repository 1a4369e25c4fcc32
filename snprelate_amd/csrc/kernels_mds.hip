// Classical multidimensional scaling of a symmetric distance matrix D (snpgdsMDS; mds.hip is the host layer): the kernels of
//     B = -1/2 J (D o D) J,   J = I - 1 1^T / n,   D o D = D with every entry squared.
// The Krylov route never forms B: y = B q is  w = q - mean(q),  z = (D o D) w,  y = -1/2 (z - mean(z))  (mds_centre_vec_kernel,
// mds_apply_kernel + mds_fold_kernel, mds_centre_vec_kernel), D read once per product as it lies and squared on the way.  The
// dense route writes B into a buffer of its own (mds_centre_kernel) from D, the row sums of D o D and their grand sum, which
// mds_scan_kernel + mds_rowsum_kernel + mds_totals_kernel produce together with the checks of the input.  No kernel here uses an
// atomic: every sum has a fixed order, the same input gives the same bits.
#include "snpgpu_internal.h"

namespace snpgpu {

typedef double f64x4 __attribute__((ext_vector_type(4)));
// two neighbouring doubles of a row: one 16-byte load.  A row of a matrix with an odd leading dimension starts on an 8-byte
// boundary only, so the type promises no more than that
typedef double f64x2u __attribute__((ext_vector_type(2), aligned(8)));

constexpr int MDS_TILE = 64;        // the scan's tiles
constexpr int MDS_STRIP = 64;       // output rows per workgroup of the product: 16 per wave
constexpr int MDS_CHUNK = 64;       // columns whose vectors are staged in LDS at a time
constexpr int MDS_VT = 3;           // 16-vector tiles per launch (48 vectors: the solver's widest block)
constexpr int MDS_WP = MDS_CHUNK + 2;

// ---- the scan --------------------------------------------------------------------------------------------------------------------
// One workgroup per tile pair (ti <= tj) reads tile A = D[I, J] and its mirror M = D[J, I] once, both along their rows:
//   flags[0]  a non-finite entry        flags[1]  A[r][c] != M[c][r] bitwise
//   part[tj][i in I] = sum_c A[i][c]^2 (c ascending)       part[ti][j in J] = sum_r A[r][j]^2 (r ascending; = the mirror's row sums
//   where the matrix is symmetric, and where it is not the call is refused).  Every (tile column, row) is written exactly once.
__global__ __launch_bounds__(256) void mds_scan_kernel(const double *__restrict__ D, int64_t ld, int64_t n, int64_t n_tiles,
                                                       double *__restrict__ part, int64_t part_ld, int *__restrict__ flags)
{
    __shared__ double sA[MDS_TILE][MDS_TILE + 1];
    // tile pair of this workgroup: blockIdx.x enumerates ti <= tj row by row
    // (row ti starts at pair ti n_tiles - ti (ti - 1) / 2: the root of that, then a step either way for the rounding)
    const int64_t p = blockIdx.x;
    const double t2 = 2.0 * (double)n_tiles + 1.0;
    int64_t ti = (int64_t)((t2 - sqrt(t2 * t2 - 8.0 * (double)p)) * 0.5);
    ti = ti < 0 ? 0 : (ti > n_tiles - 1 ? n_tiles - 1 : ti);
    while (ti > 0 && ti * n_tiles - ti * (ti - 1) / 2 > p) ti--;
    while (ti + 1 < n_tiles && (ti + 1) * n_tiles - (ti + 1) * ti / 2 <= p) ti++;
    const int64_t tj = ti + (p - (ti * n_tiles - ti * (ti - 1) / 2));
    const int64_t i0 = ti * MDS_TILE, j0 = tj * MDS_TILE;
    const int tid = threadIdx.x, c = tid & 63, rg = tid >> 6;
    bool bad = false, asym = false;
    for (int r = rg; r < MDS_TILE; r += 4) {
        double v = 0.0;
        if (i0 + r < n && j0 + c < n) {
            v = D[(i0 + r) * ld + j0 + c];
            bad |= !(fabs(v) <= 1.79769313486231570815e308);
        }
        sA[r][c] = v;
    }
    __syncthreads();
    if (tj != ti) {
        for (int r = rg; r < MDS_TILE; r += 4) {
            if (j0 + r < n && i0 + c < n) {
                const double m = D[(j0 + r) * ld + i0 + c];
                bad |= !(fabs(m) <= 1.79769313486231570815e308);
                asym |= __double_as_longlong(m) != __double_as_longlong(sA[c][r]);
            }
        }
    } else {
        for (int r = rg; r < MDS_TILE; r += 4)
            asym |= __double_as_longlong(sA[r][c]) != __double_as_longlong(sA[c][r]);
    }
    if (bad) flags[0] = 1;
    if (asym) flags[1] = 1;
    if (tid < MDS_TILE) {
        if (i0 + tid < n) {
            double s = 0.0;
            for (int k = 0; k < MDS_TILE; k++) s += sA[tid][k] * sA[tid][k];
            part[tj * part_ld + i0 + tid] = s;
        }
    } else if (tid < 2 * MDS_TILE && tj != ti) {
        const int t = tid - MDS_TILE;
        if (j0 + t < n) {
            double s = 0.0;
            for (int k = 0; k < MDS_TILE; k++) s += sA[k][t] * sA[k][t];
            part[ti * part_ld + j0 + t] = s;
        }
    }
}

// rowsum[i] = sum over the tile columns, ascending
__global__ __launch_bounds__(256) void mds_rowsum_kernel(const double *__restrict__ part, int64_t part_ld, int64_t n, int64_t n_tiles,
                                                         double *__restrict__ rowsum)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t t = 0; t < n_tiles; t++) s += part[t * part_ld + i];
    rowsum[i] = s;
}

// a fixed-order sum over one workgroup of 256: every thread adds its elements tid, tid + 256, ... in that order, then a tree
__device__ inline double block_sum_256(double mine, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = mine;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// totals[0] = sum of all d^2 (from the row sums), [1] = sum of the diagonal's d^2, [2] = the largest row sum.  One workgroup.
__global__ __launch_bounds__(256) void mds_totals_kernel(const double *__restrict__ D, int64_t ld, int64_t n,
                                                         const double *__restrict__ rowsum, double *__restrict__ totals)
{
    __shared__ double red[256];
    double s = 0.0, dg = 0.0, mx = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double r = rowsum[i], d = D[i * ld + i];
        s += r;
        dg += d * d;
        mx = r > mx ? r : mx;
    }
    const double total = block_sum_256(s, red), diag = block_sum_256(dg, red);
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + w] ? red[threadIdx.x] : red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) { totals[0] = total; totals[1] = diag; totals[2] = red[0]; }
}

// ---- the centrings of the vectors -----------------------------------------------------------------------------------------------
// dst[v][i] = scale * (src[v][i] - mean(src[v])), one workgroup per vector, the mean in the fixed order of block_sum_256
__global__ __launch_bounds__(256) void mds_centre_vec_kernel(const double *__restrict__ src, int64_t n, double scale,
                                                             double *__restrict__ dst)
{
    __shared__ double red[256];
    const double *s = src + (int64_t)blockIdx.x * n;
    double *d = dst + (int64_t)blockIdx.x * n;
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) a += s[i];
    const double mean = block_sum_256(a, red) / (double)n;
    for (int64_t i = threadIdx.x; i < n; i += 256) d[i] = scale * (s[i] - mean);
}

// ---- the product -----------------------------------------------------------------------------------------------------------------
// Zp[split][v][i] = sum over this split's columns j of D[i][j]^2 W[v][j].  A workgroup owns MDS_STRIP rows (16 per wave) and walks
// its share of the columns in chunks of MDS_CHUNK, whose vectors lie in LDS.  v_mfma_f64_16x16x4_f64 with D o D as the A operand:
//     A[row i][k]: lane (i = l & 15, k = l >> 4)      B[k][col v]: lane (v = l & 15, k = l >> 4)      D[i][v]: col v = l & 15, rows
//     i = (l >> 4) + 4 r.  A lane's 16-byte load holds D[i][j], D[i][j + 1] for j = chunk + 8 m + 2 (l >> 4): the first goes to one
//     product, the second to the next, each with the vector entries of its own column.
// Rows and columns past n are never read (their operands are zero), vectors past m are zero in LDS.
__global__ __launch_bounds__(256) void mds_apply_kernel(const double *__restrict__ D, int64_t ld, int64_t n,
                                                        const double *__restrict__ W, int m, int64_t chunks_per_split,
                                                        double *__restrict__ Zp)
{
    __shared__ double sW[MDS_VT * 16][MDS_WP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int nvt = (m + 15) / 16;
    const int64_t i0 = (int64_t)blockIdx.x * MDS_STRIP + 16 * wave;
    const int64_t row = i0 + lc;
    const bool row_ok = row < n;
    const double *__restrict__ prow = D + (row_ok ? row : 0) * ld;
    const int64_t n_chunks = (n + MDS_CHUNK - 1) / MDS_CHUNK;
    const int64_t c_begin = (int64_t)blockIdx.y * chunks_per_split;
    const int64_t c_end = c_begin + chunks_per_split < n_chunks ? c_begin + chunks_per_split : n_chunks;

    f64x4 acc[MDS_VT];
#pragma unroll
    for (int vt = 0; vt < MDS_VT; vt++) acc[vt] = (f64x4){0, 0, 0, 0};

    for (int64_t ch = c_begin; ch < c_end; ch++) {
        const int64_t jc = ch * MDS_CHUNK;
        __syncthreads();                                   // the previous chunk's vectors have been used
        for (int e = tid; e < MDS_VT * 16 * MDS_CHUNK; e += 256) {
            const int v = e / MDS_CHUNK, j = e % MDS_CHUNK;
            sW[v][j] = (v < m && jc + j < n) ? W[(int64_t)v * n + jc + j] : 0.0;
        }
        __syncthreads();
        // this lane's eight pairs of the chunk, squared
        double t[MDS_CHUNK / 8][2];
#pragma unroll
        for (int q = 0; q < MDS_CHUNK / 8; q++) {
            const int64_t j = jc + 8 * q + 2 * lk;
            double a = 0.0, b = 0.0;
            if (row_ok && j + 1 < n) {
                const f64x2u p = *reinterpret_cast<const f64x2u *>(prow + j);
                a = p[0]; b = p[1];
            } else if (row_ok && j < n) {
                a = prow[j];
            }
            t[q][0] = a * a; t[q][1] = b * b;
        }
#pragma unroll
        for (int q = 0; q < MDS_CHUNK / 8; q++)
#pragma unroll
            for (int e = 0; e < 2; e++)
#pragma unroll
                for (int vt = 0; vt < MDS_VT; vt++)
                    if (vt < nvt)
                        acc[vt] = __builtin_amdgcn_mfma_f64_16x16x4f64(t[q][e], sW[16 * vt + lc][8 * q + 2 * lk + e], acc[vt], 0, 0, 0);
    }
    double *__restrict__ out = Zp + (int64_t)blockIdx.y * (int64_t)m * n;
#pragma unroll
    for (int vt = 0; vt < MDS_VT; vt++) {
        const int v = 16 * vt + lc;
        if (v >= m) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t i = i0 + lk + 4 * r;
            if (i < n) out[(int64_t)v * n + i] = acc[vt][r];
        }
    }
}

// Z[e] = sum over the splits, ascending (e over m * n)
__global__ __launch_bounds__(256) void mds_fold_kernel(const double *__restrict__ Zp, int64_t mn, int splits, double *__restrict__ Z)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= mn) return;
    double s = Zp[e];
    for (int k = 1; k < splits; k++) s += Zp[(int64_t)k * mn + e];
    Z[e] = s;
}

// ---- the dense route's matrix ---------------------------------------------------------------------------------------------------
// B[i][j] = -1/2 ((d_ij^2 - (r_i + r_j) / n) + g / n^2): symmetric to the bit, r_i + r_j being so
__global__ __launch_bounds__(256) void mds_centre_kernel(const double *__restrict__ D, int64_t ld, int64_t n,
                                                         const double *__restrict__ rowsum, const double *__restrict__ totals,
                                                         double *__restrict__ B)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= n) return;
    const double d = D[i * ld + j], nn = (double)n;
    B[i * n + j] = -0.5 * ((d * d - (rowsum[i] + rowsum[j]) / nn) + totals[0] / (nn * nn));
}

// d = 1 - d over an n x n matrix (the IBS distance of snpgdsMDS, made where the finaliser left the IBS matrix)
__global__ __launch_bounds__(256) void mds_one_minus_kernel(double *__restrict__ d, size_t count)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) d[e] = 1.0 - d[e];
}

// ---- launches --------------------------------------------------------------------------------------------------------------------
int64_t mds_tiles(int64_t n) { return (n + MDS_TILE - 1) / MDS_TILE; }

// column splits of one product: the row strips alone fill the device from about 512 of them on; below that the columns are split,
// down to one chunk per workgroup
int mds_splits(int64_t n)
{
    const int64_t strips = (n + MDS_STRIP - 1) / MDS_STRIP, chunks = (n + MDS_CHUNK - 1) / MDS_CHUNK;
    int64_t s = (512 + strips - 1) / strips;
    s = s < chunks ? s : chunks;
    s = s < 32 ? s : 32;
    const int64_t per = (chunks + s - 1) / s;
    return (int)((chunks + per - 1) / per);               // no split without a chunk
}

// part: mds_tiles(n) * n doubles; rowsum: n; totals: 3; flags: 2 ints (cleared here)
int launch_mds_scan(hipStream_t st, const double *D, int64_t ld, int64_t n, double *part, double *rowsum, double *totals, int *flags)
{
    const int64_t T = mds_tiles(n);
    SNPGPU_HIP_CHECK(hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(mds_scan_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st, D, ld, n, T, part, n, flags);
    hipLaunchKernelGGL(mds_rowsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, n, n, T, rowsum);
    hipLaunchKernelGGL(mds_totals_kernel, dim3(1), dim3(256), 0, st, D, ld, n, rowsum, totals);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// Y = B Q for m <= 48 vectors [m][n]; Wc: m * n doubles, Zp: (mds_splits(n) + 1) * m * n doubles of scratch
int launch_mds_operator(hipStream_t st, const double *D, int64_t ld, int64_t n, const double *Q, int m, double *Y, double *Wc, double *Zp)
{
    if (m < 1 || m > MDS_VT * 16) { set_error("mds operator: 1 ... 48 vectors per launch"); return 1; }
    const int splits = mds_splits(n);
    const int64_t chunks = (n + MDS_CHUNK - 1) / MDS_CHUNK, per = (chunks + splits - 1) / splits, mn = (int64_t)m * n;
    double *Z = Zp + (int64_t)splits * mn;
    hipLaunchKernelGGL(mds_centre_vec_kernel, dim3((unsigned)m), dim3(256), 0, st, Q, n, 1.0, Wc);
    hipLaunchKernelGGL(mds_apply_kernel, dim3((unsigned)((n + MDS_STRIP - 1) / MDS_STRIP), (unsigned)splits), dim3(256), 0, st, D, ld, n,
                       (const double *)Wc, m, per, Zp);
    hipLaunchKernelGGL(mds_fold_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, st, (const double *)Zp, mn, splits, Z);
    hipLaunchKernelGGL(mds_centre_vec_kernel, dim3((unsigned)m), dim3(256), 0, st, (const double *)Z, n, -0.5, Y);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mds_centre(hipStream_t st, const double *D, int64_t ld, int64_t n, const double *rowsum, const double *totals, double *B)
{
    hipLaunchKernelGGL(mds_centre_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, st, D, ld, n, rowsum, totals, B);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mds_one_minus(hipStream_t st, double *d, size_t count)
{
    hipLaunchKernelGGL(mds_one_minus_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, d, count);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
