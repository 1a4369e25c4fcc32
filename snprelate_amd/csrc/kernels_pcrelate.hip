// PC-Relate (Conomos et al., AJHG 2016; include/snpgpu.h section 1r): kinship, k0, k2 and inbreeding from genotype
// residuals under individual-specific allele frequencies.  fp64 throughout, no atomics: every sum has one owner and a fixed order.
//   pcr_beta_*_kernel    per SNP: training counts, f_s and the regression beta_s = sum_{i in T} g~_is W_i.   lane = SNP, the row of W
//                        of a step is wave-uniform (the scheme of proj_snp_kernel<LOAD>); sample ranges, folded in ascending order
//   pcr_operand_kernel   mu_is from beta_s and V, the validity of (i, s), the nine operand planes [m][n_pad] (sample fastest)
//   pcr_product_kernel   C[i][j] += sum_s X[s][i] Y[s][j] on v_mfma_f64_16x16x4_f64: one workgroup per 128 x 128 tile of one plane, the
//                        block's SNPs as K in ascending order through LDS, the sums added to the resident plane by its only owner
//   pcr_diag_kernel / pcr_final_kernel / pcr_plane_kernel   the results and the mirrored planes, in row windows
#include "pcrelate_device.h"
#include "snpgpu_internal.h"

namespace snpgpu {

// ---- beta ----------------------------------------------------------------------------------------------------------------------
// rows: 2-bit rows of rb bytes (code 3 = missing); train [n] (0 / 1); W [n][d1p] (rows of non-training samples and the columns
// >= D + 1 are zero).  With g~ = g where called and 2 f_s where not, beta_s = sum_{called} g W_i + 2 f_s sum_{missing} W_i: both sums
// and the training counts come from ONE pass over the samples, before f_s is known.  The samples are cut into gridDim.z ranges of
// `range_bytes` row bytes (a lane alone walks its row at the latency of one load per byte); a range writes its partial sums
// part [range][m][2][d1p] and counts cnt [range][m][2] (genotype sum, calls), and pcr_beta_fold_kernel adds them in ascending
// range order: beta [m][d1], num [m].  blockIdx.y walks the columns in chunks of PCR_KC.
__global__ __launch_bounds__(64) void pcr_beta_part_kernel(const uint8_t *__restrict__ rows, int64_t rb, int m, int64_t n, int64_t range_bytes,
                                                           const uint8_t *__restrict__ train, const double *__restrict__ W, int d1p,
                                                           double *__restrict__ part, int32_t *__restrict__ cnt)
{
    const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
    const int c0 = (int)blockIdx.y * PCR_KC;
    const uint8_t *__restrict__ row = rows + (int64_t)(s < m ? s : m - 1) * rb;       // lanes past the block repeat its last row
    const int64_t nb = (n + 3) / 4;
    const int64_t b0 = (int64_t)blockIdx.z * range_bytes, b1 = b0 + range_bytes < nb ? b0 + range_bytes : nb;
    int sum = 0, num = 0;
    double ac[PCR_KC], am[PCR_KC];
#pragma unroll
    for (int j = 0; j < PCR_KC; j++) { ac[j] = 0.0; am[j] = 0.0; }
#pragma unroll 4
    for (int64_t b = b0; b < b1; b++) {
        const uint32_t w = row[b];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t i = 4 * b + u;
            if (i >= n) break;
            const uint32_t code = (w >> (2 * u)) & 3u;
            const bool called = code != 3u;
            if (called && train[i]) { sum += (int)code; num++; }
            const double g = called ? (double)code : 0.0, q = called ? 0.0 : 1.0;
            const double *__restrict__ wr = W + i * d1p + c0;                           // wave-uniform row
#pragma unroll
            for (int j = 0; j < PCR_KC; j++) {
                ac[j] = fma(g, wr[j], ac[j]);
                am[j] = fma(q, wr[j], am[j]);
            }
        }
    }
    if (s >= m) return;
    const int64_t at = (int64_t)blockIdx.z * m + s;
#pragma unroll
    for (int j = 0; j < PCR_KC; j++) {
        part[(at * 2) * d1p + c0 + j] = ac[j];
        part[(at * 2 + 1) * d1p + c0 + j] = am[j];
    }
    if (blockIdx.y == 0) { cnt[at * 2] = sum; cnt[at * 2 + 1] = num; }
}

__global__ __launch_bounds__(256) void pcr_beta_fold_kernel(const double *__restrict__ part, const int32_t *__restrict__ cnt, int m, int d1p,
                                                            int d1, int n_range, double *__restrict__ beta, int32_t *__restrict__ num)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)m * d1) return;
    const int64_t s = idx / d1;
    const int col = (int)(idx - s * d1);
    int sum = 0, calls = 0;
    double ac = 0.0, am = 0.0;
    for (int r = 0; r < n_range; r++) {
        const int64_t at = (int64_t)r * m + s;
        sum += cnt[at * 2]; calls += cnt[at * 2 + 1];
        ac += part[(at * 2) * d1p + col];
        am += part[(at * 2 + 1) * d1p + col];
    }
    const double f2 = calls > 0 ? 2.0 * ((double)sum / (double)(2 * calls)) : 0.0;    // 2 f_s: the imputed genotype
    beta[idx] = calls > 0 ? fma(f2, am, ac) : 0.0;
    if (col == 0) num[s] = calls;
}

int launch_pcr_beta(hipStream_t st, const uint8_t *rows, int64_t rb, int m, int64_t n, const uint8_t *train, const double *W, int d1p, int d1,
                    int n_range, int64_t range_bytes, double *part, int32_t *cnt, double *beta, int32_t *num)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(pcr_beta_part_kernel, dim3((unsigned)((m + 63) / 64), (unsigned)(d1p / PCR_KC), (unsigned)n_range), dim3(64), 0, st, rows,
                       rb, m, n, range_bytes, train, W, d1p, part, cnt);
    hipLaunchKernelGGL(pcr_beta_fold_kernel, dim3((unsigned)(((int64_t)m * d1 + 255) / 256)), dim3(256), 0, st, part, cnt, m, d1p, d1, n_range,
                       beta, num);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- operands ------------------------------------------------------------------------------------------------------------------
// Vt [D][n_pad]: the PCs, sample fastest; ops: n_planes planes of plane_stride doubles, each [m][n_pad].  Every operand of an (i, s)
// that is not valid -- a missing call, mu outside [lo, hi], a SNP without a called training sample, a column >= n -- is zero.
__global__ __launch_bounds__(256) void pcr_operand_kernel(const uint8_t *__restrict__ rows, int64_t rb, int m, int64_t n, int64_t n_pad,
                                                          const double *__restrict__ beta, const int32_t *__restrict__ num, int d1,
                                                          const double *__restrict__ Vt, double lo, double hi, int n_planes,
                                                          double *__restrict__ ops, int64_t plane_stride)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)m * n_pad) return;
    const int64_t s = idx / n_pad, i = idx - s * n_pad;
    uint32_t code = 3u;
    double mu = 0.0;
    if (i < n && num[s] > 0) {
        code = (rows[s * rb + (i >> 2)] >> (2 * (i & 3))) & 3u;
        const double *__restrict__ b = beta + s * d1;
        mu = b[0];
        for (int d = 1; d < d1; d++) mu = fma(b[d], Vt[(int64_t)(d - 1) * n_pad + i], mu);
        mu *= 0.5;
    }
    const bool valid = code != 3u && mu >= lo && mu <= hi;
    const double g = (double)code, q = 1.0 - mu, c = mu * q;
    double v[PCR_N_OPS];
    v[PCR_OP_R] = g - 2.0 * mu;
    v[PCR_OP_S] = sqrt(c);
    v[PCR_OP_O] = 1.0;
    v[PCR_OP_GD] = code == 0u ? mu : code == 2u ? q : 0.0;
    v[PCR_OP_C] = c;
    v[PCR_OP_I0] = code == 0u ? 1.0 : 0.0;
    v[PCR_OP_I2] = code == 2u ? 1.0 : 0.0;
    v[PCR_OP_A] = mu * mu;
    v[PCR_OP_B] = q * q;
#pragma unroll
    for (int p = 0; p < PCR_N_OPS; p++)
        if (p < n_planes) ops[p * plane_stride + idx] = valid ? v[p] : 0.0;
}

int launch_pcr_operands(hipStream_t st, const uint8_t *rows, int64_t rb, int m, int64_t n, int64_t n_pad, const double *beta,
                        const int32_t *num, int d1, const double *Vt, double lo, double hi, int n_planes, double *ops, int64_t plane_stride)
{
    if (m <= 0) return 0;
    const int64_t blocks = ((int64_t)m * n_pad + 255) / 256;
    hipLaunchKernelGGL(pcr_operand_kernel, dim3((unsigned)blocks), dim3(256), 0, st, rows, rb, m, n, n_pad, beta, num, d1, Vt, lo, hi,
                       n_planes, ops, plane_stride);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- products ------------------------------------------------------------------------------------------------------------------
// One workgroup: the 128 x 128 tile (I, J) of job blockIdx.z; four waves, 64 x 64 each (4 x 4 MFMA tiles, 16 f64x4 accumulators).
// PCR_KB SNP rows of both operands are staged per step; the LDS row stride of 144 doubles puts the k rows of lanes l and l + 16 of a
// ds_read_b64 on opposite halves of the 64-bank row (288 dwords = 32 mod 64): conflict-free.  A/B: one f64 per lane, A[i = lane & 15]
// [k = lane >> 4], B[k = lane >> 4][j = lane & 15]; D: column lane & 15, rows (lane >> 4) + 4 r.
constexpr int PCR_LDS_STRIDE = PCR_TILE + 16;

// The job says where the tile goes (pcrelate_device.h): a full plane, a row panel's slab, the panel's CD slab (the product's tile
// (J, I), stored transposed) or a strip of diagonal tiles.  Whatever the destination, the tile is the same instruction sequence
// over K, so a panel holds the full object's bits.
__global__ __launch_bounds__(256) void pcr_product_kernel(PcrJobs jobs, int64_t n, int64_t n_pad, int m, int tri, int tile0, int tile0_col)
{
    const PcrJob job = jobs.j[blockIdx.z];
    const bool diag = job.mode == PCR_JOB_DIAG, transposed = job.mode == PCR_JOB_TRANSPOSED;
    if (diag && blockIdx.y != 0) return;
    const int gI = diag ? (int)blockIdx.x : tile0 + (int)blockIdx.y, gJ = diag ? (int)blockIdx.x : tile0_col + (int)blockIdx.x;
    if (tri && gI > gJ) return;
    const int I = transposed ? gJ : gI, J = transposed ? gI : gJ;      // the product's tile
    __shared__ double sX[PCR_KB][PCR_LDS_STRIDE];
    __shared__ double sY[PCR_KB][PCR_LDS_STRIDE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const double *__restrict__ X = job.x + (int64_t)I * PCR_TILE;
    const double *__restrict__ Y = job.y + (int64_t)J * PCR_TILE;
    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    // a step's rows travel global -> registers -> LDS: the loads of step t + 1 are in flight while the MFMAs of step t run
    constexpr int NLD = PCR_KB * (PCR_TILE / 2) / 256;                                 // double2 per thread and operand
    const int fr = tid >> 6, fc = (tid & 63) * 2;                                      // this thread's rows fr + 4 q, columns fc, fc + 1
    double2 px[NLD], py[NLD];
    auto fetch = [&](int s0) {
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int r = s0 + fr + (256 / (PCR_TILE / 2)) * q;
            px[q] = make_double2(0.0, 0.0); py[q] = make_double2(0.0, 0.0);
            if (r < m) {                                                               // rows past the block are zero
                px[q] = *reinterpret_cast<const double2 *>(X + (int64_t)r * n_pad + fc);
                py[q] = *reinterpret_cast<const double2 *>(Y + (int64_t)r * n_pad + fc);
            }
        }
    };
    fetch(0);
    for (int s0 = 0; s0 < m; s0 += PCR_KB) {
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int r = fr + (256 / (PCR_TILE / 2)) * q;
            *reinterpret_cast<double2 *>(&sX[r][fc]) = px[q];
            *reinterpret_cast<double2 *>(&sY[r][fc]) = py[q];
        }
        __syncthreads();
        if (s0 + PCR_KB < m) fetch(s0 + PCR_KB);
#pragma unroll
        for (int k0 = 0; k0 < PCR_KB; k0 += 4) {
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                a[t] = sX[k0 + lk][wi + 16 * t + lc];
                b[t] = sY[k0 + lk][wj + 16 * t + lc];
            }
#pragma unroll
            for (int ti = 0; ti < 4; ti++)
#pragma unroll
                for (int tj = 0; tj < 4; tj++) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
        }
        __syncthreads();
    }
    // this workgroup is the tile's only owner in this launch: plain loads and stores
    double *__restrict__ C = job.c;
    const int64_t col0 = diag ? (int64_t)J * PCR_TILE : job.col0;
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
#pragma unroll
        for (int tj = 0; tj < 4; tj++) {
            const int64_t j = (int64_t)J * PCR_TILE + wj + 16 * tj + lc;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t i = (int64_t)I * PCR_TILE + wi + 16 * ti + lk + 4 * r;
                const int64_t di = transposed ? j : i, dj = transposed ? i : j;        // where the entry is stored
                if (di < job.row_end && dj < n) C[(di - job.row0) * job.ld + (dj - col0)] += acc[ti][tj][r];
            }
        }
}

int launch_pcr_products(hipStream_t st, const PcrJobs &jobs, int n_jobs, int64_t n, int64_t n_pad, int m, bool tri, int tile0, int nt_rows,
                        int tile0_col, int nt_cols)
{
    if (m <= 0 || n_jobs <= 0 || nt_rows <= 0 || nt_cols <= 0) return 0;
    hipLaunchKernelGGL(pcr_product_kernel, dim3((unsigned)nt_cols, (unsigned)nt_rows, (unsigned)n_jobs), dim3(256), 0, st, jobs, n, n_pad, m,
                       tri ? 1 : 0, tile0, tile0_col);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- results -------------------------------------------------------------------------------------------------------------------
// the entry (i, j) of a plane that holds the tiles I <= J only
__device__ __forceinline__ double pcr_sym(const double *__restrict__ P, int64_t n, int64_t i, int64_t j)
{
    return i <= j ? P[i * n + j] : P[j * n + i];
}

// inbreed_i = 2 kinship_ii - 1 and e_i = 1 + inbreed_i, written as the definitions read (no contraction: a host restatement of
// these few operations gives the same bits)
__global__ __launch_bounds__(256) void pcr_diag_kernel(const double *__restrict__ RR, const double *__restrict__ SS, int64_t n, int64_t ld,
                                                       int64_t wrap, double *__restrict__ inbreed, double *__restrict__ e)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t at = i * ld + (wrap ? i % wrap : i);
    const double kin = RR[at] / (4.0 * SS[at]);
    const double f = 2.0 * kin - 1.0;
    inbreed[i] = f;
    e[i] = 1.0 + f;
}

// rows [r0, r0 + rows) of kinship, k0, k2 and nsnp ([rows][n] each; any may be NULL; k0 / k2 need the IBD planes)
__global__ __launch_bounds__(256) void pcr_final_kernel(PcrPlanes P, int64_t n, int64_t r0, int64_t rows, const double *__restrict__ e,
                                                        double *__restrict__ kinship, double *__restrict__ k0, double *__restrict__ k2,
                                                        double *__restrict__ nsnp)
{
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * n) return;
    const int64_t i = r0 + idx / n, j = idx % n;
    const double kin = pcr_sym(P.p[PCR_RR], n, i, j) / (4.0 * pcr_sym(P.p[PCR_SS], n, i, j));
    if (kinship) kinship[idx] = kin;
    if (nsnp) nsnp[idx] = pcr_sym(P.p[PCR_NS], n, i, j);
    if (!k0 && !k2) return;
    const double ei = e[i], ej = e[j], cc = pcr_sym(P.p[PCR_CC], n, i, j);
    const double *__restrict__ DC = P.p[PCR_DC];
    const double v2 = (pcr_sym(P.p[PCR_DD], n, i, j) - ej * DC[i * n + j] - ei * DC[j * n + i] + ei * ej * cc) / cc;
    if (k2) k2[idx] = v2;
    if (k0) k0[idx] = kin < PCR_KIN_SPLIT ? pcr_sym(P.p[PCR_IBS0], n, i, j) / pcr_sym(P.p[PCR_K0D], n, i, j) : 1.0 - 4.0 * kin + v2;
}

int launch_pcr_diag(hipStream_t st, const double *RR, const double *SS, int64_t n, int64_t ld, int64_t wrap, double *inbreed, double *e)
{
    hipLaunchKernelGGL(pcr_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, RR, SS, n, ld, wrap, inbreed, e);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_pcr_final(hipStream_t st, const PcrPlanes &P, int64_t n, int64_t r0, int64_t rows, const double *e, double *kinship, double *k0,
                     double *k2, double *nsnp)
{
    hipLaunchKernelGGL(pcr_final_kernel, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), 0, st, P, n, r0, rows, e, kinship, k0, k2, nsnp);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// rows [r0, r0 + rows) of one plane as a full matrix: mirrored where only the tiles I <= J are held
__global__ __launch_bounds__(256) void pcr_plane_kernel(const double *__restrict__ P, int64_t n, int sym, int64_t r0, int64_t rows,
                                                        double *__restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * n) return;
    const int64_t i = r0 + idx / n, j = idx % n;
    out[idx] = sym ? pcr_sym(P, n, i, j) : P[i * n + j];
}

int launch_pcr_plane(hipStream_t st, const double *P, int64_t n, bool sym, int64_t r0, int64_t rows, double *out)
{
    hipLaunchKernelGGL(pcr_plane_kernel, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), 0, st, P, n, sym ? 1 : 0, r0, rows, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- results through a view ----------------------------------------------------------------------------------------------------
// The same results for a row panel, or for a full object read as the panel [0, n): rows [r0, r0 + rows) x columns [col0, n).
__global__ __launch_bounds__(256) void pcr_view_final_kernel(PcrView v, int64_t n, int64_t r0, int64_t rows, const double *__restrict__ e,
                                                             double *__restrict__ kinship, double *__restrict__ k0, double *__restrict__ k2,
                                                             double *__restrict__ nsnp)
{
    const int64_t nc = n - v.col0, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * nc) return;
    const int64_t i = r0 + idx / nc, j = v.col0 + idx % nc;
    double kin = 0.0, v0 = 0.0, v2 = 0.0;
    pcr_pair_values(v, e, i, j, k0 || k2, kin, v0, v2);
    if (kinship) kinship[idx] = kin;
    if (nsnp) nsnp[idx] = v.sym(PCR_NS, i, j);
    if (k0) k0[idx] = v0;
    if (k2) k2[idx] = v2;
}

__global__ __launch_bounds__(256) void pcr_view_plane_kernel(PcrView v, int which, int64_t n, int64_t r0, int64_t rows, double *__restrict__ out)
{
    const int64_t nc = n - v.col0, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * nc) return;
    const int64_t i = r0 + idx / nc, j = v.col0 + idx % nc;
    out[idx] = which == PCR_CD ? v.dc(j, i) : which == PCR_DC ? v.dc(i, j) : v.sym(which, i, j);
}

int launch_pcr_view_final(hipStream_t st, const PcrView &v, int64_t n, int64_t r0, int64_t rows, const double *e, double *kinship, double *k0,
                          double *k2, double *nsnp)
{
    const int64_t cells = rows * (n - v.col0);
    hipLaunchKernelGGL(pcr_view_final_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, v, n, r0, rows, e, kinship, k0, k2, nsnp);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_pcr_view_plane(hipStream_t st, const PcrView &v, int which, int64_t n, int64_t r0, int64_t rows, double *out)
{
    const int64_t cells = rows * (n - v.col0);
    hipLaunchKernelGGL(pcr_view_plane_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, v, which, n, r0, rows, out);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
