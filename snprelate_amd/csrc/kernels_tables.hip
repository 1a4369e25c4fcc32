// Per-SNP tables of a feed block, from the block's sum / num (O(B) work, launched by feed_syrk, ctx_feed.hip):
//   build_lut       decode table of one SYRK table            (DivideGeno/rsqrt_prod, src/genPCA.cpp:98-181)
//   uv_factor / uv_assign / uv_tables   tables, coefficients and slot map of the single-product SYRK (launch_build_uv)
//   homo_uv_tables / homo_totals        KING-homo tables, effective weights and block totals (launch_homo_tables)
#include "snpgpu_internal.h"

namespace snpgpu {

// ---------------------------------------------------------------------------
// build_lut: per-SNP values {z(0), z(1), z(2), z(missing)} (missing is 0 except for the EIGMIX weight
// table), stored as a per-SNP-PAIR table for the SYRK kernel.
// Arithmetic in fp64 like the reference, each entry rounded once to fp32.
__global__ __launch_bounds__(256) void build_lut_kernel(const int32_t *__restrict__ sum,
                                                        const int32_t *__restrict__ num, int64_t n_snp,
                                                        int64_t n_snp_pad, int mode, int split16,
                                                        float2 *__restrict__ lut,
                                                        unsigned long long *__restrict__ d_nlocus,
                                                        double *__restrict__ d_sumden, double *__restrict__ dvals,
                                                        const unsigned long long *__restrict__ d_missing,
                                                        double2 *__restrict__ ccoef, int exact_rows_always, int w_shift,
                                                        int exact_with_missing, int entry12, double *__restrict__ homo_const,
                                                        double4 *__restrict__ uvsp_miss, int x1_sparse_mac,
                                                        unsigned long long *__restrict__ d_short_runs)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;   // n_snp_pad is a multiple of 64: whole waves
    if (k >= n_snp_pad) return;
    double x = 0, y = 0, wmiss = 0, dden = 0, avg = 0, wtrue = 0;
    bool poly = false;
    int mac = 1 << 30, minor_is_counted = 1;
    if (k < n_snp) {
        const int s = sum[k], c = num[k];
        mac = (s < 2 * c - s) ? s : (2 * c - s);
        minor_is_counted = (s <= c);
        avg = (c > 0) ? ((double)s / c) : 0.0;               // DivideGeno, genPCA.cpp:98-142
        poly = (0 < s) && (s < 2 * c);                        // genPCA.cpp:1206
        if (mode == LUT_GCTA) {
            const double p = avg * 0.5;                       // rsqrt_prod, genPCA.cpp:145-181
            const double sc = (0 < p && p < 1) ? (1.0 / sqrt(p * (1 - p))) : 0.0;
            y = sc; x = -avg * sc;
        } else if (mode == LUT_BAYES) {
            const double p = (s + 1.0) / (2.0 * c + 2.0);     // genPCA.cpp:441-453
            const double sc = 1.0 / sqrt(p * (1 - p));
            y = sc; x = -avg * sc;
        } else if (mode == LUT_EIGMIX_NUM || mode == LUT_EIGMIX_MISSW) {
            const double af = 0.5 * avg;                      // genEIGMIX.cpp:116-121
            dden = 4 * af * (1 - af);
            if (mode == LUT_EIGMIX_NUM) { x = -avg; y = 1.0; }
            else wmiss = exact_rows_always ? dden : sqrt(dden);   // m_i * [d m_j]  |  [sqrt(d) m_i] * [sqrt(d) m_j]
        } else {
            const double p = (c > 0) ? (0.5 * s / c) : 0.0;   // genKING.cpp:236-248
            const double w = p * (1 - p);
            wtrue = (mode == LUT_HOMO_W1) ? w : w * w;
            if (exact_rows_always) {                          // v_i * [c v_j]: the whole weight (and scale) on the column side
                x = ldexp((mode == LUT_HOMO_W1) ? w : w * w, 2 * H3_HOMO_SHIFT);
            } else {
                x = (mode == LUT_HOMO_W1) ? sqrt(w) : w;
                if (split16) x = ldexp(x, H3_HOMO_SHIFT);    // keep p(1-p) ~ 1e-6 in fp16's normal range
            }
            y = 0;
        }
    }
    // pair table: SNPs (2p, 2p+1) share 16 float2 entries indexed by c0 + 4*c1 -> (z_2p(c0), z_2p+1(c1)),
    // so that the SYRK kernel decodes TWO operand values with one table read (ds_read_b64).
    // The even lane writes entries 0..7, the odd lane 8..15 (n_snp_pad is even, lanes pair up).
    const bool odd = (k & 1);
    if (split16) {
        // fp16 pair hi = fp16(z), lo = fp16(z - hi) (22 significant bits); entry = {hi0 | hi1 << 16, lo0 | lo1 << 16}
        double zd[4] = {x, x + y, x + 2.0 * y, wmiss};
        // Exact-row-side SYRK (syrk_h3_kernel<2, true>): 16-byte entries {hi pair, lo pair, row pair, row pair}.
        // Column operand w = y z 2^-w_shift (0 for a missing call); row operand (g - cs) 2^w_shift with the centre
        // cs = avg rounded to the fewest binary digits that keep (avg - cs)^2 <= Var(g)/64, so that the products have the
        // variance of the centred form at any allele frequency; the column term (avg - cs) w(g) = u + v g is summed per
        // chunk by colcorr_kernel and subtracted from every row at the flush.
        // A MISSING row call must contribute 0 = a w - (avg - cs) w, i.e. its row value is a = avg - cs: a real number,
        // kept as fp16(avg - cs).  In a block with missing calls cs therefore takes all 9 fractional digits an exact
        // fp16 (g - cs) allows, |avg - cs| <= 2^-10, and the rounding of a is <= 2^-21 (2^-25 absolute in the fp16
        // subnormal range) per missing cell: below the lo parts' own 2^-22 |w|.
        const bool has_missing = (*d_missing != 0ull);
        const bool exact_rows = ccoef && (exact_with_missing || !has_missing);
        // Rare variants in a block WITH missing calls (uvsp_miss; GCTA / Bayesian weights y^2 = 1 / (p (1 - p)) up to ~N): a
        // pair of carriers would put y^2 ~ 1e4 .. 1e5 into an fp32 accumulator whose other terms are O(1), and every later
        // addition of the run is then rounded at that magnitude (measured: 1.3e-5 off-diagonal figure on a rare-variant
        // spectrum with 2 % missing calls; 7.8e-6 on a flat one).  Such an SNP stays in the dense product with every CALLED
        // genotype replaced by the non-carrier's (the tables below: all three codes get the non-carrier's value), i.e. it
        // contributes y^2 avg'^2 m_i m_j exactly as before for pairs of non-carriers, and uv_sparse_kernel adds what the
        // carriers' pairs lack in fp64.
        // (weights below X1_SPARSE_MIN_W stay where they are: nothing large enters the accumulators, and the fp64 atomics of
        // the sparse path -- whose order is not fixed -- stay out of small data sets, where two runs are expected to agree bit
        // for bit)
        const bool rare = uvsp_miss && has_missing && exact_rows && y * y >= X1_SPARSE_MIN_W && (mode == LUT_GCTA || mode == LUT_BAYES) &&
                          mac <= x1_sparse_mac;
        const double g_nc = minor_is_counted ? 0.0 : 2.0;         // the non-carrier's genotype
        if (uvsp_miss && has_missing)
            uvsp_miss[k] = rare ? make_double4(y * y, minor_is_counted ? avg : 2.0 - avg, minor_is_counted ? 0.0 : 1.0, 1.0)
                                : make_double4(0, 0, 0, 0);
        if (rare) zd[0] = zd[1] = zd[2] = x + g_nc * y;
        // such a block runs as 4096-SNP fp32 runs (syrk_x1_kernel reads the flag): what the carriers leave in the dense product is
        // small, but the spectrum that holds them is the thinnest accuracy case (9.3e-6 with 8192-SNP runs, 5.9e-6 with 4096)
        if (rare && d_short_runs) *d_short_runs = 1ull;
        double cs = 1.0;
        if (ccoef) {
            if (exact_rows) {
                const double var = 0.5 * avg * (2.0 - avg);
                for (int kb = has_missing ? 9 : 0; kb <= 9; kb++) {
                    cs = ldexp(rint(ldexp(avg, kb)), -kb);
                    if ((avg - cs) * (avg - cs) * 64.0 <= var) break;
                }
                for (int c = 0; c < 3; c++) zd[c] = ldexp(zd[c] * y, -w_shift);
            }
            ccoef[k] = !exact_rows ? make_double2(0.0, 0.0)
                       : rare ? make_double2((avg - cs) * y * (x + g_nc * y), 0.0)      // w(g) = u + v g is the same for every call
                              : make_double2((avg - cs) * y * x, (avg - cs) * y * y);
        }
        uint32_t hl[4], ho[4], ar[4], ao[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const _Float16 hi = (_Float16)zd[c];    // each value on its own fp16 grid: 22 bits of THAT value in hi + lo
            const _Float16 lo = (_Float16)(zd[c] - (double)hi);
            hl[c] = (uint32_t)__builtin_bit_cast(uint16_t, hi) | ((uint32_t)__builtin_bit_cast(uint16_t, lo) << 16);
            // exact for c < 3; c == 3 (missing call, SNP / sample padding): the centre residual, see above
            const _Float16 a = (y != 0.0) ? (_Float16)ldexp((c < 3 ? (rare ? g_nc : (double)c) : avg) - cs, w_shift) : (_Float16)0.0;
            ar[c] = (uint32_t)__builtin_bit_cast(uint16_t, a);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) { ho[c] = (uint32_t)__shfl_xor((int)hl[c], 1); ao[c] = (uint32_t)__shfl_xor((int)ar[c], 1); }
        if (exact_rows && entry12) {
            // syrk_x1_kernel: 12-byte entries {hi pair, lo pair, row pair}; dword banks 3 c + {0, 1, 2} (mod 32) are distinct
            // for the 16 entries of a pair, so plain ds_read_b32 lookups are conflict-free and land in place
            uint32_t *dst = reinterpret_cast<uint32_t *>(lut) + ((k >> 1) * 16 + (odd ? 8 : 0)) * 3;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int idx = e + (odd ? 8 : 0), c0 = idx & 3, c1 = idx >> 2;
                const uint32_t a = odd ? ho[c0] : hl[c0], b = odd ? hl[c1] : ho[c1];   // SNP 2p, SNP 2p+1
                const uint32_t ra = odd ? ao[c0] : ar[c0], rb = odd ? ar[c1] : ao[c1];
                dst[3 * e] = (a & 0xFFFFu) | (b << 16);
                dst[3 * e + 1] = (a >> 16) | (b & 0xFFFF0000u);
                dst[3 * e + 2] = ra | (rb << 16);
            }
        } else if (exact_rows) {
            uint4 *dst = reinterpret_cast<uint4 *>(lut) + (k >> 1) * 16 + (odd ? 8 : 0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int idx = e + (odd ? 8 : 0), c0 = idx & 3, c1 = idx >> 2;
                const uint32_t a = odd ? ho[c0] : hl[c0], b = odd ? hl[c1] : ho[c1];   // SNP 2p, SNP 2p+1
                const uint32_t ra = odd ? ao[c0] : ar[c0], rb = odd ? ar[c1] : ao[c1];
                // the row pair twice: the two lane halves of the kernel read different copies (LDS banks)
                dst[e] = make_uint4((a & 0xFFFFu) | (b << 16), (a >> 16) | (b & 0xFFFF0000u), ra | (rb << 16), ra | (rb << 16));
            }
        } else {
            uint2 *dst = reinterpret_cast<uint2 *>(lut) + (k >> 1) * 16 + (odd ? 8 : 0);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int idx = e + (odd ? 8 : 0), c0 = idx & 3, c1 = idx >> 2;
                const uint32_t a = odd ? ho[c0] : hl[c0], b = odd ? hl[c1] : ho[c1];   // SNP 2p, SNP 2p+1
                dst[e] = make_uint2((a & 0xFFFFu) | (b << 16), (a >> 16) | (b & 0xFFFF0000u));
            }
        }
    } else {
        const float z[4] = {(float)x, (float)(x + y), (float)(x + 2.0 * y), (float)wmiss};
        float zo[4];
#pragma unroll
        for (int c = 0; c < 4; c++) zo[c] = __shfl_xor(z[c], 1);
        float2 *dst = lut + (k >> 1) * 16 + (odd ? 8 : 0);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int idx = e + (odd ? 8 : 0), c0 = idx & 3, c1 = idx >> 2;
            dst[e] = odd ? make_float2(zo[c0], z[c1]) : make_float2(z[c0], zo[c1]);
        }
    }
    if (homo_const && *d_missing == 0ull) {   // KING-homo: in a block without missing calls every pair gets the whole sum
        double v = wtrue;                     // (the masked SYRK of this table is skipped for such a block)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0 && v != 0.0) unsafeAtomicAdd(homo_const, v);
    }
    if (dvals) { dvals[2 * k] = dden; dvals[2 * k + 1] = -x; }   // {4p(1-p), avg} in fp64 for the per-sample sums
    if (d_sumden) {            // SumDenominator of CEigMix_AlgArith::Run, one fp64 atomic per wave
        double v = dden;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0 && v != 0.0) unsafeAtomicAdd(d_sumden, v);
    }
    if (d_nlocus) {
        const unsigned long long b = __ballot(poly);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(d_nlocus, (unsigned long long)__popcll(b));
    }
}

int launch_build_lut(hipStream_t st, const int32_t *sum, const int32_t *num, int64_t n_snp, int64_t n_snp_pad, const BuildLutOpts &o)
{
    if (n_snp_pad <= 0) return 0;
    hipLaunchKernelGGL(build_lut_kernel, dim3((unsigned)((n_snp_pad + 255) / 256)), dim3(256), 0, st, sum, num,
                       n_snp, n_snp_pad, o.lut_mode, o.split16 ? 1 : 0, o.lut, o.d_nlocus, o.d_sumden, o.dvals, o.d_missing, o.ccoef,
                       o.exact_rows_always ? 1 : 0, o.w_shift, o.exact_with_missing ? 1 : 0, o.entry12 ? 1 : 0, o.homo_const, o.uvsp_miss,
                       o.x1_sparse_mac, o.d_short_runs);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// Tables of the single-product SYRK (syrk_uv_kernel; blocks without missing calls).  Per SNP:
//   * the weight t = y^2 = 1 / (p (1 - p)) as a product of two fp16 numbers: u runs over the 1024 mantissas of its octave
//     (u ~ sqrt(t)), v = fp16(t / u); the pair with the smallest |u v - t| is kept.  One product of two 11-bit mantissas
//     reaches a given weight only to ~1e-6 rms (6.6e-6 at worst: the candidates' errors are a Poisson process of density
//     ~1 / 1.4e-6, the best one Laplace-distributed) -- round 3 bought that down with a second slot for a quarter of the SNPs
//     (1.25 x the MFMA work).  Round 4: WEIGHT TARGETS PER fp32 RUN.  The kernel runs a block as R launches ("runs", one fp64
//     flush each) and a run's flush may multiply its fp32 sums by a constant for free.  Run q therefore carries the factor
//     f_q = 1 - q / 4096 (exact in 13 bits: f_q x an fp32 partial is exact in fp64) and a SNP placed in run q needs
//     u v ~ t / f_q: R different targets per SNP, R x 1024 candidates, and SNP order inside a feed block is free (the sum is
//     order-independent).  uv_factor_kernel finds the best pair for every target, uv_assign_kernel deals the SNPs to the runs
//     (each SNP to its best target while the run has room -- deterministic, in SNP order; the ~1 % that overflow take their
//     next best), uv_tables_kernel builds the tables in slot order.  The factorisation error falls as 1 / R: 1.05e-6 rms for one
//     target, 0.37e-6 for three, 0.285e-6 for four (numpy emulation and tools/panel_error_distribution.py), with NO extra slots;
//     u v f_q IS the SNP's weight from then on (row / column / constant terms);
//   * integer centres c_a (rows), c_b (columns): one lane per 64-slot chunk walks its slots in order and keeps the running
//     mean of the products, cum = sum d_a d_b u v, near zero: (near, near) adds d^2 u v >= 0, (near, other neighbour) adds
//     d_near d_far u v <= 0 and is taken when it brings cum closer to zero -- but only for SNPs where it costs at most a
//     factor 6 in the variance of the products, (Var g + d_a^2)(Var g + d_b^2) <= 6 (Var g)^2: avg within ~0.3 of x.5.  A
//     far centre on a RARE variant would put +-u v ~ 1/p into every column of a carrier's row (cancelled later by the row
//     term, but carried through the fp32 sums); rare variants keep (near, near), whose products are sparse and whose
//     mean d^2 u v ~ 2 avg is small, and lean on the common SNPs of the chunk to cancel it;
//   * pair table entry c0 + 4 c1 = {(c0 - c_a) u | (c1 - c_a') u' << 16, (c0 - c_b) v | (c1 - c_b') v' << 16}: exact fp16
//     values, 0 for code 3 (SNP / sample padding);
//   * uvcoef = {d_b u v f, c_a, d_a u v f, c_b} for the row / column terms, kpart[chunk] = sum d_a d_b u v f.
// The K dimension of such a block is a list of SLOTS: slot_src maps slots to the block's SNPs for the transposition (-1: an
// empty slot; SNPs without weight -- monomorphic, rare variants on the fp64 path, padding -- own none).  One run (or a kind
// whose weight is exact: EIGMIX) = one target, slot k = SNP k, no map.
struct UvSnp { double t, avg; };
__device__ __forceinline__ UvSnp uv_snp_weight(const int32_t *__restrict__ sum, const int32_t *__restrict__ num, int64_t k,
                                               int64_t n_snp, int mode, bool *sparse)
{
    UvSnp r{0.0, 0.0};
    *sparse = false;
    if (k >= n_snp) return r;
    const int s = sum[k], c = num[k];
    r.avg = (c > 0) ? ((double)s / c) : 0.0;
    if (mode == LUT_GCTA) {
        const double p = r.avg * 0.5;
        r.t = (0 < p && p < 1) ? (1.0 / (p * (1 - p))) : 0.0;
    } else if (mode == LUT_EIGMIX_NUM) {
        r.t = 1.0;                                            // (g_i - 2p)(g_j - 2p): u = v = 1, no factorisation error
    } else {                                                  // LUT_BAYES
        const double p = (s + 1.0) / (2.0 * c + 2.0);
        r.t = 1.0 / (p * (1 - p));
    }
    // rare variants (<= UV_SPARSE_MAC copies of the minor allele) leave the dense product: uv_sparse_kernel adds their
    // few carrier pairs and their row / column terms in fp64 with the exact weight
    if (r.t > 0) {
        const int mac = (s < 2 * c - s) ? s : (2 * c - s);
        *sparse = (mac <= UV_SPARSE_MAC);
    }
    return r;
}

// one wave per SNP: the lanes share out the 1024 mantissas of u for each of the n_target targets t / f_q
__global__ __launch_bounds__(256) void uv_factor_kernel(const int32_t *__restrict__ sum, const int32_t *__restrict__ num,
                                                        int64_t n_snp, int64_t n_snp_pad, int mode, int n_target,
                                                        float *__restrict__ cand_err, uint32_t *__restrict__ cand_uv,
                                                        double2 *__restrict__ snp_tavg, double4 *__restrict__ uvsp,
                                                        const unsigned long long *__restrict__ d_missing)
{
    if (*d_missing != 0ull) return;
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_snp_pad) return;
    bool sparse;
    UvSnp w = uv_snp_weight(sum, num, k, n_snp, mode, &sparse);
    if (lane == 0) {
        uvsp[k] = sparse ? make_double4(w.t, (sum[k] <= num[k]) ? w.avg : 2.0 - w.avg, (sum[k] <= num[k]) ? 0.0 : 1.0, 1.0)
                         : make_double4(0, 0, 0, 0);
        snp_tavg[k] = make_double2(sparse ? 0.0 : w.t, w.avg);
    }
    if (sparse) w.t = 0;
    for (int q = 0; q < n_target; q++) {
        float rel = 0.f;
        uint32_t uv = 0;
        if (w.t > 0) {                                        // wave-uniform
            const double tt = w.t / uv_run_factor(q);
            const int e = ilogb(sqrt(tt));
            const float tf = (float)tt;
            double best = 1e300;
            int bm = 0;
            _Float16 bv = (_Float16)0.0;
#pragma unroll 4
            for (int i = 0; i < 16; i++) {
                const int m = lane * 16 + i;
                const double uc = ldexp(1.0 + (double)m * (1.0 / 1024.0), e);
                const _Float16 vh = (_Float16)(tf / (float)uc);             // any fp16 near the quotient: judged by the product
                const double err = fabs(uc * (double)vh - tt);
                if (err < best) { best = err; bm = m; bv = vh; }
            }
            for (int o = 32; o; o >>= 1) {                    // arg-min over the wave; ties to the smaller mantissa
                const double oe = __shfl_xor(best, o);
                const int om = __shfl_xor(bm, o);
                const int ov = __shfl_xor((int)__builtin_bit_cast(uint16_t, bv), o);
                if (oe < best || (oe == best && om < bm)) { best = oe; bm = om; bv = __builtin_bit_cast(_Float16, (uint16_t)ov); }
            }
            const _Float16 uh = (_Float16)ldexp(1.0 + (double)bm * (1.0 / 1024.0), e);
            rel = (float)(best / tt);
            uv = (uint32_t)__builtin_bit_cast(uint16_t, uh) | ((uint32_t)__builtin_bit_cast(uint16_t, bv) << 16);
        }
        if (lane == 0) { cand_err[k * UV_QMAX + q] = rel; cand_uv[k * UV_QMAX + q] = uv; }
    }
}

// ONE workgroup deals the block's weighted SNPs to the runs: in rounds, every SNP not yet placed asks for the run with its
// smallest factorisation error among those that still have room; a run takes the askers in SNP order up to its capacity.
// Run r owns the slots [r * cpr * 1024, min((r + 1) * cpr, n_chunk) * 1024) and carries target r % n_target; target q's slots
// are those of its runs q, q + n_target, ... in order.  Deterministic (no atomics).
__global__ __launch_bounds__(1024) void uv_assign_kernel(const float *__restrict__ cand_err, const double2 *__restrict__ snp_tavg,
                                                         int64_t n_snp_pad, int n_target, int cpr, int n_chunk,
                                                         int32_t *__restrict__ slot_of, int32_t *__restrict__ slot_src,
                                                         const unsigned long long *__restrict__ d_missing)
{
    if (*d_missing != 0ull) return;
    __shared__ int s_rem[UV_QMAX], s_cap[UV_QMAX], s_tot[UV_QMAX];
    __shared__ int s_wsum[UV_QMAX][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // thread t takes the SNPs t, t + 1024, ...: neighbouring lanes read neighbouring 32-byte candidate records (round 5; with 64
    // consecutive SNPs per thread every load touched 64 cache lines and the kernel took 1.05 ms per 65 536-SNP block, all latency).
    // "SNP order" below is therefore the order (thread, then SNP): any fixed order makes the deal deterministic
    for (int64_t k = tid; k < n_snp_pad; k += 1024) { slot_of[k] = -1; slot_src[k] = -1; }
    const int run_len = cpr * UV_CHS;
    if (tid < UV_QMAX) {
        int cap = 0;
        if (tid < n_target)
            for (int c0 = tid * cpr; c0 < n_chunk; c0 += n_target * cpr) cap += (((c0 + cpr < n_chunk) ? (c0 + cpr) : n_chunk) - c0) * UV_CHS;
        s_cap[tid] = s_rem[tid] = cap;
    }
    __syncthreads();
    for (int rnd = 0; rnd < n_target; rnd++) {
        int rem[UV_QMAX], cnt[UV_QMAX];
#pragma unroll
        for (int q = 0; q < UV_QMAX; q++) { rem[q] = s_rem[q]; cnt[q] = 0; }
        auto choose = [&](int64_t k) -> int {
            int bq = -1;
            float be = 0.f;
#pragma unroll
            for (int q = 0; q < UV_QMAX; q++)
                if (q < n_target && rem[q] > 0) {
                    const float e = cand_err[k * UV_QMAX + q];
                    if (bq < 0 || e < be) { bq = q; be = e; }
                }
            return bq;
        };
        for (int64_t k = tid; k < n_snp_pad; k += 1024)
            if (slot_of[k] < 0 && snp_tavg[k].x > 0) {
                const int q = choose(k);
#pragma unroll
                for (int j = 0; j < UV_QMAX; j++) cnt[j] += (j == q) ? 1 : 0;
            }
        // exclusive prefix of cnt[q] over the threads (SNP order): wave scan + wave totals in LDS
        int pre[UV_QMAX];
#pragma unroll
        for (int q = 0; q < UV_QMAX; q++) {
            int x = cnt[q];
            for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
            pre[q] = x - cnt[q];
            if (lane == 63) s_wsum[q][wave] = x;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < UV_QMAX; q++) {
            int before = 0, tot = 0;
            for (int w = 0; w < 16; w++) { const int v = s_wsum[q][w]; if (w < wave) before += v; tot += v; }
            pre[q] += before;
            if (tid == 0) s_tot[q] = tot;
        }
        for (int64_t k = tid; k < n_snp_pad; k += 1024)
            if (slot_of[k] < 0 && snp_tavg[k].x > 0) {
                const int q = choose(k);
                int rank = 0;
#pragma unroll
                for (int j = 0; j < UV_QMAX; j++) if (j == q) { rank = pre[j]; pre[j]++; }
                if (q >= 0 && rank < rem[q]) {
                    const int pos = (s_cap[q] - rem[q]) + rank;                    // position in target q's slot list
                    const int slot = (q + n_target * (pos / run_len)) * run_len + pos % run_len;
                    slot_of[k] = slot;
                    slot_src[slot] = (int32_t)k;
                }
            }
        __syncthreads();
        int left = 0;
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < UV_QMAX; q++) {
                const int take = s_tot[q] < s_rem[q] ? s_tot[q] : s_rem[q];
                left += s_tot[q] - take;
                s_rem[q] -= take;
            }
            s_tot[0] = left;
        }
        __syncthreads();
        left = s_tot[0];
        __syncthreads();
        if (left == 0) break;
    }
}

// tables, row / column coefficients and constants of the block's slots (256 per workgroup, four chunks of 64)
__global__ __launch_bounds__(256) void uv_tables_kernel(const uint32_t *__restrict__ cand_uv, const double2 *__restrict__ snp_tavg,
                                                        const int32_t *__restrict__ slot_src, int64_t n_snp_pad, int n_target,
                                                        int cpr, uint2 *__restrict__ lut, double4 *__restrict__ uvcoef,
                                                        double *__restrict__ kpart,
                                                        const unsigned long long *__restrict__ d_missing, int swap_odd)
{
    // swap_odd == 2 (syrk_uv16c_kernel): no tables -- `lut` receives the FACTORS of the slots instead, 256 bytes per 32-slot group:
    // dword ((side * 2 + kind) * 4 + quarter) * 4 + d = the fp16 pair of slots 8 quarter + 2 d, + 1; side 0 = row (u, c_a), 1 = column
    // (v, c_b); kind 0 = 2 u, kind 1 = -c u: the operand (g - c) u = (g / 2) (2 u) - c u is ONE packed fma on the converted nibbles
    if (*d_missing != 0ull) return;
    __shared__ double s_avg[256], s_w[256], s_f[256];
    __shared__ int s_ca[256], s_cb[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t slot = (int64_t)blockIdx.x * 256 + tid;     // n_snp_pad is a multiple of 256
    const int64_t k = slot_src ? (int64_t)slot_src[slot] : slot;
    const int q = (n_target > 1) ? (int)(((slot / UV_CHS) / cpr) % n_target) : 0;
    double u = 0, v = 0, avg = 0;
    const double f = (n_target > 1) ? uv_run_factor(q) : 1.0;
    if (k >= 0) {
        const double2 ta = snp_tavg[k];
        if (ta.x > 0) {
            const uint32_t uv = cand_uv[k * UV_QMAX + q];
            u = (double)__builtin_bit_cast(_Float16, (uint16_t)(uv & 0xFFFFu));
            v = (double)__builtin_bit_cast(_Float16, (uint16_t)(uv >> 16));
            avg = ta.y;
        }
    }
    s_avg[tid] = avg; s_w[tid] = u * v; s_f[tid] = f;          // u v exact: 22 significant bits
    __syncthreads();
    if (lane == 0) {
        double cum = 0.0, ks = 0.0;
        for (int i = tid; i < tid + 64; i++) {
            const double a = s_avg[i], w = s_w[i], wf = w * s_f[i];
            int ca = 0, cb = 0;
            if (w > 0) {
                const double near = rint(a);
                double far = near + (a > near ? 1.0 : -1.0);
                if (far < 0.0 || far > 2.0) far = near;
                const double dn = a - near, df = a - far, var = 0.5 * a * (2.0 - a);
                const double mnn = dn * dn * w, mnf = dn * df * w;
                ca = cb = (int)near;
                if (far != near && (var + dn * dn) * (var + df * df) <= 6.0 * var * var && fabs(cum + mnf) < fabs(cum + mnn)) {
                    cb = (int)far; cum += mnf; ks += dn * df * wf;
                } else { cum += mnn; ks += dn * dn * wf; }
                // uvcorr_kernel sums d uv g, not d uv (g - c): the centre parts are constants and travel with K
                ks += ((a - (double)cb) * (double)ca + (a - (double)ca) * (double)cb) * wf;
            }
            s_ca[i] = ca; s_cb[i] = cb;
        }
        kpart[slot >> 6] = ks;
    }
    __syncthreads();
    const int ca = s_ca[tid], cb = s_cb[tid];
    const double yt = u * v * f;
    uvcoef[slot] = (yt > 0) ? make_double4((avg - cb) * yt, (double)ca, (avg - ca) * yt, (double)cb) : make_double4(0, 0, 0, 0);
    if (swap_odd == 2) {
        const _Float16 h[4] = {(_Float16)(2.0 * u), (_Float16)(-(double)ca * u), (_Float16)(2.0 * v), (_Float16)(-(double)cb * v)};
        uint32_t mine[4], other[4];
#pragma unroll
        for (int e = 0; e < 4; e++) mine[e] = (uint32_t)__builtin_bit_cast(uint16_t, h[e]);
#pragma unroll
        for (int e = 0; e < 4; e++) other[e] = (uint32_t)__shfl_xor((int)mine[e], 1);
        if (!(slot & 1)) {
            uint32_t *fac = reinterpret_cast<uint32_t *>(lut) + (slot >> 5) * 64;
            const int pp = (int)(slot & 31) >> 1, kq = pp >> 2, d = pp & 3;
#pragma unroll
            for (int e = 0; e < 4; e++) fac[(e * 4 + kq) * 4 + d] = mine[e] | (other[e] << 16);      // e = side * 2 + kind
        }
        return;
    }
    uint32_t ab[4], ao[4];                                    // per code: row value | column value << 16
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const _Float16 a = (c < 3) ? (_Float16)((double)(c - ca) * u) : (_Float16)0.0;
        const _Float16 b = (c < 3) ? (_Float16)((double)(c - cb) * v) : (_Float16)0.0;
        ab[c] = (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) ao[c] = (uint32_t)__shfl_xor((int)ab[c], 1);
    const bool odd = (slot & 1);
    uint2 *dst = lut + (slot >> 1) * 16 + (odd ? 8 : 0);       // the even lane writes entries 0..7, the odd lane 8..15
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int idx = e + (odd ? 8 : 0), c0 = idx & 3, c1 = idx >> 2;
        const uint32_t x0 = odd ? ao[c0] : ab[c0], x1 = odd ? ab[c1] : ao[c1];   // slot 2p, slot 2p+1
        const uint32_t rowp = (x0 & 0xFFFFu) | (x1 << 16), colp = (x0 >> 16) | (x1 & 0xFFFF0000u);
        // swap_odd (syrk_uv16_kernel): pairs of an odd 8-SNP quarter -- bit 2 of the pair index -- carry {column pair, row pair}, so
        // that the two quarters a 32-lane LDS pass spans read different banks
        dst[e] = (swap_odd && ((slot >> 3) & 1)) ? make_uint2(colp, rowp) : make_uint2(rowp, colp);
    }
}

// n_target > 1: the block's slots are dealt to n_target runs of cpr table chunks (slot_of / slot_src are written);
// n_target == 1: slot k = SNP k (slot_src may be null)
int launch_build_uv(hipStream_t st, const int32_t *sum, const int32_t *num, int64_t n_snp, int64_t n_snp_pad, const BuildUvOpts &o)
{
    if (n_snp_pad <= 0) return 0;
    const int n_target = o.n_target, cpr = o.cpr;
    int32_t *slot_of = o.slot_of, *slot_src = o.slot_src;
    // the kernel's swap_odd: 0 plain tables, 1 swapped odd quarters (lookup form), 2 factor arrays (converted forms)
    const int swap_odd = o.form == UvForm::Mfma32x32x16 ? 0 : o.form == UvForm::Lookup16x16x32 ? 1 : 2;
    if (n_target < 1 || n_target > UV_QMAX || (n_target > 1 && ((n_snp_pad % UV_CHS) != 0 || !slot_src || !slot_of || cpr < 1))) {
        set_error("build_uv: invalid run plan");
        return 1;
    }
    const int n_chunk = (int)((n_snp_pad + UV_CHS - 1) / UV_CHS);
    hipLaunchKernelGGL(uv_factor_kernel, dim3((unsigned)((n_snp_pad + 3) / 4)), dim3(256), 0, st, sum, num, n_snp, n_snp_pad, o.lut_mode,
                       n_target, o.cand_err, o.cand_uv, o.snp_tavg, o.uvsp, o.d_missing);
    if (n_target > 1)
        hipLaunchKernelGGL(uv_assign_kernel, dim3(1), dim3(1024), 0, st, o.cand_err, o.snp_tavg, n_snp_pad, n_target, cpr, n_chunk, slot_of,
                           slot_src, o.d_missing);
    hipLaunchKernelGGL(uv_tables_kernel, dim3((unsigned)(n_snp_pad / 256)), dim3(256), 0, st, o.cand_uv, o.snp_tavg,
                       n_target > 1 ? slot_src : nullptr, n_snp_pad, n_target, cpr, o.lut, o.uvcoef, o.kpart, o.d_missing, swap_odd);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// KING-homo, blocks WITH missing calls (round 5).  The masked weight sums SumAFreq(i, j) = sum over the SNPs where BOTH samples are
// called of c_s, c = p (1 - p) resp. (p (1 - p))^2 (src/genKING.cpp:236-248), were two-product fp16 SYRKs of an indicator against a
// hi / lo column operand.  With the missing indicator mu:  sum_s c_s (1 - mu_is)(1 - mu_js) = C - M_i - M_j + B_ij,
//     C = sum_s c_s,    M_i = sum_s c_s mu_is  (per sample, fp64, O(N B)),    B_ij = sum_s c_s mu_is mu_js,
// and only B is a pair contraction -- of BINARY operands, so c_s = u v with two fp16 numbers makes it ONE exact product per SNP
// (syrk_uv_kernel's arithmetic: row value u, column value v for code 3, zero otherwise); a factorisation error of 1e-6 (best of the
// 1024 mantissas of u, as uv_factor_kernel) meets a term that is f^2 of the sum.  u v IS the SNP's weight in C and M as well.
// homo_uv_tables_kernel: one wave per SNP, both weights: tables (8-byte entries {row pair, column pair}, syrk_uv_kernel's format),
// the effective weights {w1, w2} (x 2^-16: the tables carry 2^16 c so that (p(1-p))^2 ~ 1e-10 stays in fp16's normal range) and
// the block totals into the context's two KING-homo scalars.  n_w = 1 (individual dissimilarity, whose weight is 8 p (1 - p)): the first
// weight only -- no second table, its effective weight stays 0.
__global__ __launch_bounds__(256) void homo_uv_tables_kernel(const int32_t *__restrict__ sum, const int32_t *__restrict__ num,
                                                             int64_t n_snp, int64_t n_snp_pad, uint2 *__restrict__ lut1,
                                                             uint2 *__restrict__ lut2, double2 *__restrict__ wts,
                                                             double *__restrict__ totals,
                                                             const unsigned long long *__restrict__ d_missing, int swap_odd, int n_w)
{
    if (*d_missing == 0ull) return;               // blocks without missing calls: every pair gets the whole sum (build_lut_kernel)
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_snp_pad) return;
    double c1 = 0.0;
    if (k < n_snp) {
        const int s = sum[k], c = num[k];
        const double p = (c > 0) ? (0.5 * s / c) : 0.0;       // genKING.cpp:236-248
        c1 = p * (1 - p);
    }
    uint32_t uv[2] = {0u, 0u};
    double weff[2] = {0.0, 0.0};
    for (int t = 0; t < n_w; t++) {
        const double tt = ldexp(t == 0 ? c1 : c1 * c1, 2 * H3_HOMO_SHIFT);
        if (!(tt > 0) || tt < 1e-7) continue;                  // wave-uniform (weights below 2^-16 x 1e-7 ~ 1e-12 count as zero)
        // (the search below is uv_factor_kernel's, as an inline copy: one shared function changed both kernels and missed the A/B
        // timing bound by 0.2 % / 0.4 %, profiles/prep_split_isa.md)
        const int e = ilogb(sqrt(tt));
        const float tf = (float)tt;
        double best = 1e300;
        int bm = 0;
        _Float16 bv = (_Float16)0.0;
#pragma unroll 4
        for (int i = 0; i < 16; i++) {
            const int m = lane * 16 + i;
            const double uc = ldexp(1.0 + (double)m * (1.0 / 1024.0), e);
            const _Float16 vh = (_Float16)(tf / (float)uc);
            const double err = fabs(uc * (double)vh - tt);
            if (err < best) { best = err; bm = m; bv = vh; }
        }
        for (int o = 32; o; o >>= 1) {                        // arg-min over the wave; ties to the smaller mantissa
            const double oe = __shfl_xor(best, o);
            const int om = __shfl_xor(bm, o);
            const int ov = __shfl_xor((int)__builtin_bit_cast(uint16_t, bv), o);
            if (oe < best || (oe == best && om < bm)) { best = oe; bm = om; bv = __builtin_bit_cast(_Float16, (uint16_t)ov); }
        }
        const _Float16 uh = (_Float16)ldexp(1.0 + (double)bm * (1.0 / 1024.0), e);
        uv[t] = (uint32_t)__builtin_bit_cast(uint16_t, uh) | ((uint32_t)__builtin_bit_cast(uint16_t, bv) << 16);
        weff[t] = ldexp((double)uh * (double)bv, -2 * H3_HOMO_SHIFT);
    }
    if (lane == 0) wts[k] = make_double2(weff[0], weff[1]);        // (the block totals: homo_totals_kernel, in a fixed order)
    // pair table of slots (2p, 2p+1): entry c0 + 4 c1 = {row value of slot 2p | of slot 2p+1 << 16, column values likewise}; lanes
    // 0..15 write the 16 entries of this SNP's pair, this SNP's half of each (the partner wave of the pair writes the other half)
    if (lane < 16) {
        const int c0 = lane & 3, c1i = lane >> 2;
        const bool odd = (k & 1);
        const bool mine3 = odd ? (c1i == 3) : (c0 == 3);
        for (int t = 0; t < n_w; t++) {
            uint16_t *e16 = reinterpret_cast<uint16_t *>((t == 0 ? lut1 : lut2) + (k >> 1) * 16 + lane);
            const int sw = (swap_odd && ((k >> 3) & 1)) ? 2 : 0;      // odd quarters: {column pair, row pair} (syrk_uv16_kernel)
            e16[(odd ? 1 : 0) + sw] = mine3 ? (uint16_t)(uv[t] & 0xFFFFu) : (uint16_t)0;       // row value (u)
            e16[(odd ? 3 : 2) - sw] = mine3 ? (uint16_t)(uv[t] >> 16) : (uint16_t)0;           // column value (v)
        }
    }
}

// totals[0..1] += the block's sums of the two effective weights: ONE workgroup, strided partial sums, wave and LDS reduction in a
// fixed order (65 536 waves adding to one address with atomics took 1.5 ms per block and depended on their arrival order)
__global__ __launch_bounds__(1024) void homo_totals_kernel(const double2 *__restrict__ wts, int64_t n, double *__restrict__ totals,
                                                           const unsigned long long *__restrict__ d_missing)
{
    if (*d_missing == 0ull) return;
    __shared__ double s1[16], s2[16];
    double a = 0.0, b = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += 1024) { const double2 w = wts[k]; a += w.x; b += w.y; }
    for (int o = 32; o; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); }
    if ((threadIdx.x & 63) == 0) { s1[threadIdx.x >> 6] = a; s2[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0, tb = 0.0;
        for (int w = 0; w < 16; w++) { ta += s1[w]; tb += s2[w]; }
        totals[0] += ta; totals[1] += tb;
    }
}

int launch_homo_tables(hipStream_t st, const int32_t *sum, const int32_t *num, int64_t n_snp, int64_t n_snp_pad, uint2 *lut1, uint2 *lut2,
                       double2 *wts, double *totals, const unsigned long long *d_missing, int swap_odd, int n_w)
{
    if (n_snp_pad <= 0) return 0;
    // tables of whole 1024-slot chunks (syrk_uv_kernel copies whole chunks): zero weights beyond the block
    const int64_t n_tab = (n_snp_pad + UV_CHS - 1) / UV_CHS * UV_CHS;
    hipLaunchKernelGGL(homo_uv_tables_kernel, dim3((unsigned)((n_tab + 3) / 4)), dim3(256), 0, st, sum, num, n_snp, n_tab, lut1, lut2, wts,
                       totals, d_missing, swap_odd, n_w);
    hipLaunchKernelGGL(homo_totals_kernel, dim3(1), dim3(1024), 0, st, wts, n_tab, totals, d_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
