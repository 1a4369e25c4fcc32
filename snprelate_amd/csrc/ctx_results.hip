// Accumulator contexts, their results: the pending terms settled into the panel, then one finaliser launch into the caller's
// layout.  Every finaliser is its check (check_out), its outputs (OutBuf) and its launch; stage_out (snpgpu_internal.h) is the
// sequence around the launch.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "ctx_plan.h"

using namespace snpgpu;

// column term of the exact-row SYRK (table 0 only): applied to the panel before anything reads the sums
int snpgpu::ctx_settle(snpgpu_ctx *c)
{
    if (!c->colterm_pending) return 0;
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    const int64_t rows_real = std::min<int64_t>(c->plan.row1 - c->plan.row0, c->plan.N - c->plan.row0);
    if (launch_colterm_settle(c->stream, (double *)c->acc_f64.p, c->plan.ncols_pad, c->plan.acc_tiles_c, rows_real, c->plan.ncols_pad, c->plan.N - c->plan.col0,
                              (double *)c->colterm.p, (double *)c->uvterm.p))
        return 1;
    c->colterm_pending = false;
    return 0;
}

int snpgpu::check_out(snpgpu_ctx *c, int kind_a, int kind_b, int packed, const char *fn, bool settle)
{
    if (!c) { set_error(std::string(fn) + ": NULL context"); return 1; }
    if (c->plan.kind != kind_a && c->plan.kind != kind_b) { set_error(std::string(fn) + ": wrong context kind"); return 1; }
    if (!packed && !c->plan.full) { set_error(std::string(fn) + ": full-matrix output needs a full (non-panel) context"); return 1; }
    if (settle && ctx_settle(c)) return 1;
    if (c->het_pending && c->plan.pc_mode == PM_DISS) {
        SNPGPU_HIP_CHECK(hipSetDevice(c->device));
        if (launch_diss_settle(c->stream, (uint32_t *)c->acc_u32.p, c->plan.rows_pad, c->plan.ncols_pad, (uint32_t *)c->het.p)) return 1;
        c->het_pending = false;
    }
    if (c->het_pending) {       // rank-one terms of the blocks the binary pair kernel took
        SNPGPU_HIP_CHECK(hipSetDevice(c->device));
        const bool homo = (c->plan.pc_mode == PM_KING_HOMO);     // planes {ibs1, 2 ibs0} instead of {n, ibs1, 2 ibs0, ...}
        if (launch_het_settle(c->stream, (uint32_t *)c->acc_u32.p, c->plane(), c->plan.rows_pad, c->plan.ncols_pad, (uint32_t *)c->het.p,
                              c->plan.kind == SNPGPU_KING_ROBUST, homo ? 0 : 1, homo ? 1 : 2))
            return 1;
        c->het_pending = false;
    }
    if (hipSetDevice(c->device) != hipSuccess) { set_error(std::string(fn) + ": hipSetDevice failed"); return 1; }
    return 0;
}

int snpgpu::finish(snpgpu_ctx *c)
{
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int snpgpu::upload_family(snpgpu_ctx *c, const int32_t *family, const int32_t **dfam)
{
    *dfam = nullptr;
    if (family) {
        if (!c->family.p && c->family.alloc(sizeof(int32_t) * (size_t)c->plan.N)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->family.p, family, sizeof(int32_t) * (size_t)c->plan.N, hipMemcpyHostToDevice, c->stream));
        *dfam = (const int32_t *)c->family.p;
    }
    return 0;
}

HomoTerms snpgpu::homo_terms(snpgpu_ctx *c)
{
    // split-fp16 tables are pre-scaled by 2^H3_HOMO_SHIFT (both operands): the sums carry 2^(2 shift)
    return HomoTerms{c->plan.mm_h3 ? std::ldexp(1.0, -2 * H3_HOMO_SHIFT) : 1.0, c->plan.want_het ? c->d_homo_w() : nullptr,
                     c->plan.homo_uv ? (const double *)c->homo_msum.p : nullptr,
                     c->plan.homo_uv ? (const uint32_t *)c->diss_called.p : nullptr,
                     c->plan.homo_uv ? (const uint32_t *)c->nosh.p : nullptr};
}

int snpgpu::beta_terms(snpgpu_ctx *c, int mode, double *avg, double *mn_out, const char *fn)
{
    const int nb = 1024;
    DevBuf part;
    if (part.alloc(sizeof(double) * 2 * nb)) return 1;
    std::vector<double> h(2 * nb);
    int rc = launch_beta_reduce(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, mode != 0, (double *)part.p,
                                (double *)part.p + nb, nb);
    if (!rc && hipMemcpyAsync(h.data(), part.p, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = 1;
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = 1;
    part.release();
    if (rc) { set_error(std::string(fn) + ": reduction failed"); return 1; }
    double mn = h[0], sum = 0;
    for (int i = 0; i < nb; i++) { if (h[i] < mn) mn = h[i]; sum += h[nb + i]; }
    *avg = sum / (double)(c->plan.N * (c->plan.N - 1) / 2);
    *mn_out = mn;
    return 0;
}

namespace {

size_t out_elems(snpgpu_ctx *c, int packed) { return packed ? (size_t)snpgpu_slab_size(c) : (size_t)c->plan.N * (size_t)c->plan.N; }

// the dissimilarity (out) or its packed sums (geno_sum, wsum)
int launch_diss(snpgpu_ctx *c, double *out, uint32_t *geno_sum, double *wsum, int packed)
{
    return launch_fin_diss(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (const double *)c->acc_f64.p,
                           std::ldexp(1.0, -2 * H3_HOMO_SHIFT), c->d_homo_w(), (const double *)c->homo_msum.p,
                           (const uint32_t *)c->diss_called.p, out, geno_sum, wsum, packed, (const uint32_t *)c->nosh.p);
}

// GCTA: the pending column / row terms of the fp16 SYRK are applied by the finaliser itself (one pass over the panel less)
int launch_gcta(snpgpu_ctx *c, double *out, int packed)
{
    return launch_fin_gcta(c->stream, c->geom(), (const double *)c->acc_f64.p, (const uint32_t *)c->acc_u32.p,
                           (const uint32_t *)c->miss_diag.p, c->d_nlocus(), out, packed,
                           c->colterm_pending ? (const double *)c->colterm.p : nullptr,
                           c->colterm_pending ? (const double *)c->uvterm.p : nullptr);
}

}  // namespace

extern "C" {

int snpgpu_ibs_num(snpgpu_ctx *c, int32_t *ibs0, int32_t *ibs1, int32_t *ibs2, int packed, int mem)
{
    if (check_out(c, SNPGPU_IBS, SNPGPU_IBS, packed, "snpgpu_ibs_num")) return 1;
    const size_t n = out_elems(c, packed) * sizeof(int32_t);
    OutBuf b0(c->stream, ibs0, n, mem), b1(c->stream, ibs1, n, mem), b2(c->stream, ibs2, n, mem);
    return stage_out(c, {&b0, &b1, &b2}, [&] {
        return launch_fin_ibs_num(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (int32_t *)b0.dev, (int32_t *)b1.dev, (int32_t *)b2.dev, packed);
    });
}

int snpgpu_ibs_ave(snpgpu_ctx *c, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_IBS, SNPGPU_IBS, packed, "snpgpu_ibs_ave")) return 1;
    OutBuf b(c->stream, out, out_elems(c, packed) * sizeof(double), mem);
    return stage_out(c, {&b}, [&] { return launch_fin_ibs_ave(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (double *)b.dev, packed); });
}

int snpgpu_king_robust_counts(snpgpu_ctx *c, uint32_t *out5, int mem)
{
    if (check_out(c, SNPGPU_KING_ROBUST, SNPGPU_KING_ROBUST, 1, "snpgpu_king_robust_counts")) return 1;
    OutBuf b(c->stream, out5, out_elems(c, 1) * 5 * sizeof(uint32_t), mem);
    return stage_out(c, {&b}, [&] { return launch_fin_king_counts(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (uint32_t *)b.dev); });
}

int snpgpu_king_robust(snpgpu_ctx *c, const int32_t *family, double *ibs0, double *kinship, int packed, int mem)
{
    if (check_out(c, SNPGPU_KING_ROBUST, SNPGPU_KING_ROBUST, packed, "snpgpu_king_robust")) return 1;
    const int32_t *dfam = nullptr;
    if (upload_family(c, family, &dfam)) return 1;
    const size_t n = out_elems(c, packed) * sizeof(double);
    OutBuf b0(c->stream, ibs0, n, mem), b1(c->stream, kinship, n, mem);
    return stage_out(c, {&b0, &b1}, [&] {
        return launch_fin_king_robust(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, dfam, (double *)b0.dev, (double *)b1.dev, packed);
    });
}

int snpgpu_king_homo(snpgpu_ctx *c, double *k0, double *k1, int packed, int mem)
{
    if (check_out(c, SNPGPU_KING_HOMO, SNPGPU_KING_HOMO, packed, "snpgpu_king_homo")) return 1;
    const size_t n = out_elems(c, packed) * sizeof(double);
    OutBuf b0(c->stream, k0, n, mem), b1(c->stream, k1, n, mem);
    return stage_out(c, {&b0, &b1}, [&] {
        const HomoTerms t = homo_terms(c);
        return launch_fin_king_homo(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (const double *)c->acc_f64.p, t.fscale,
                                    (double *)b0.dev, (double *)b1.dev, packed, t.w_const, t.msum, t.called, t.nosh);
    });
}

int snpgpu_diss(snpgpu_ctx *c, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_DISS, SNPGPU_DISS, packed, "snpgpu_diss")) return 1;
    OutBuf b(c->stream, out, out_elems(c, packed) * sizeof(double), mem);
    return stage_out(c, {&b}, [&] { return launch_diss(c, (double *)b.dev, nullptr, nullptr, packed); });
}

int snpgpu_diss_sums(snpgpu_ctx *c, uint32_t *geno_sum, double *wsum, int mem)
{
    if (check_out(c, SNPGPU_DISS, SNPGPU_DISS, 1, "snpgpu_diss_sums")) return 1;
    if (!geno_sum || !wsum) { set_error("snpgpu_diss_sums: NULL output"); return 1; }
    const size_t n = out_elems(c, 1);
    OutBuf b0(c->stream, geno_sum, n * sizeof(uint32_t), mem), b1(c->stream, wsum, n * sizeof(double), mem);
    return stage_out(c, {&b0, &b1}, [&] { return launch_diss(c, nullptr, (uint32_t *)b0.dev, (double *)b1.dev, 1); });
}

int snpgpu_grm_gcta(snpgpu_ctx *c, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_GRM_GCTA, SNPGPU_GRM_GCTA, packed, "snpgpu_grm_gcta", false)) return 1;     // (not settled: launch_gcta)
    OutBuf b(c->stream, out, out_elems(c, packed) * sizeof(double), mem);
    return stage_out(c, {&b}, [&] {
        // frozen: the panel already holds the final values (snpgpu_finalize_inplace)
        return c->frozen ? launch_fin_cov(c->stream, c->geom(), (const double *)c->acc_f64.p, 1.0, (double *)b.dev, packed)
                         : launch_gcta(c, (double *)b.dev, packed);
    });
}

int snpgpu_pca_cov(snpgpu_ctx *c, double *out, int packed, int normalize, double trace_in, double *trace_xtx, int mem)
{
    if (check_out(c, SNPGPU_PCA_COV, SNPGPU_PCA_COV, packed, "snpgpu_pca_cov")) return 1;
    double tr = 0;
    if (launch_trace(c->stream, c->geom(), (const double *)c->acc_f64.p, c->d_trace())) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(&tr, c->d_trace(), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (trace_xtx) *trace_xtx = tr;
    double scale = 1.0;
    if (normalize) {
        if (trace_in > 0) tr = trace_in;
        else if (!c->plan.full) { set_error("snpgpu_pca_cov: normalisation of a panel needs trace_in"); return 1; }
        scale = (double)(c->plan.N - 1) / tr;  // genPCA.cpp:1386-1390
    }
    if (!out) return 0;
    OutBuf b(c->stream, out, out_elems(c, packed) * sizeof(double), mem);
    return stage_out(c, {&b}, [&] { return launch_fin_cov(c->stream, c->geom(), (const double *)c->acc_f64.p, scale, (double *)b.dev, packed); });
}

int snpgpu_ibd_mom(snpgpu_ctx *c, const double *e, int kinship_constraint, double *k0, double *k1, int packed, int mem)
{
    if (check_out(c, SNPGPU_IBS, SNPGPU_IBS, packed, "snpgpu_ibd_mom")) return 1;
    if (!e) { set_error("snpgpu_ibd_mom: e is NULL"); return 1; }
    const size_t n = out_elems(c, packed) * sizeof(double);
    OutBuf b0(c->stream, k0, n, mem), b1(c->stream, k1, n, mem);
    return stage_out(c, {&b0, &b1}, [&] {
        return launch_fin_mom(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, e, kinship_constraint, (double *)b0.dev, (double *)b1.dev, packed);
    });
}

int snpgpu_eigmix(snpgpu_ctx *c, int diagadj, double scale, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_EIGMIX, SNPGPU_EIGMIX, packed, "snpgpu_eigmix")) return 1;
    OutBuf b(c->stream, out, out_elems(c, packed) * sizeof(double), mem);
    return stage_out(c, {&b}, [&] {
        const double *num = (const double *)c->acc_f64.p;
        if (!c->frozen)
            return launch_fin_eigmix(c->stream, c->geom(), num, num + c->plane(), (const uint32_t *)c->samp_het.p, (const double *)c->samp_dmiss.p,
                                     (const double *)c->samp_dsq.p, c->d_sumden(), diagadj, scale, (double *)b.dev, packed);
        if ((diagadj != 0) != (c->frozen_diagadj != 0)) { set_error("snpgpu_eigmix: the context was finalised in place with another 'diagadj'"); return 1; }
        return launch_fin_cov(c->stream, c->geom(), num, scale / c->frozen_scale, (double *)b.dev, packed);
    });
}

int snpgpu_indiv_beta(snpgpu_ctx *c, int mode, double *out, double *avg_val, int packed, int mem)
{
    if (check_out(c, SNPGPU_INDIV_BETA, SNPGPU_INDIV_BETA, packed, "snpgpu_indiv_beta")) return 1;
    if (!c->plan.full) { set_error("snpgpu_indiv_beta: needs a full (non-panel) context"); return 1; }
    if (mode < 0 || mode > 2) { set_error("snpgpu_indiv_beta: invalid mode"); return 1; }
    double avg = 0, mn = 0;
    if (beta_terms(c, mode, &avg, &mn, "snpgpu_indiv_beta")) return 1;
    if (avg_val) *avg_val = avg;
    if (!out) return 0;
    OutBuf b(c->stream, out, out_elems(c, packed) * sizeof(double), mem);
    return stage_out(c, {&b}, [&] { return launch_fin_beta(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, mode, avg, mn, (double *)b.dev, packed); });
}

// ---- results that stay in the panel ----------------------------------------------------------------------------------------------

int snpgpu_pca_panel_trace(snpgpu_ctx *c, double *trace)
{
    if (!c || c->plan.kind != SNPGPU_PCA_COV) { set_error("snpgpu_pca_panel_trace: needs a PCA_COV context"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    if (ctx_settle(c)) return 1;
    if (launch_trace(c->stream, c->geom(), (const double *)c->acc_f64.p, c->d_trace())) return 1;
    double tr = 0;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(&tr, c->d_trace(), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (trace) *trace = tr;
    return 0;
}

int snpgpu_pca_panel_matmul(snpgpu_ctx *c, double scale, const double *Q, int m, double *Y)
{
    if (snpgpu::ctx_panel_matmul_enqueue(c, scale, Q, m, Y)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int snpgpu_pca_panel_matmul_f32(snpgpu_ctx *c, double scale, const double *Q, int m, double *Y)
{
    if (snpgpu::ctx_panel_matmul_enqueue(c, scale, Q, m, Y, true)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int snpgpu_finalize_inplace(snpgpu_ctx *c, int diagadj, double scale)
{
    if (!c) { set_error("snpgpu_finalize_inplace: NULL context"); return 1; }
    if (c->plan.kind != SNPGPU_PCA_COV && c->plan.kind != SNPGPU_GRM_GCTA && c->plan.kind != SNPGPU_EIGMIX) {
        set_error("snpgpu_finalize_inplace: needs a PCA_COV, GRM_GCTA or EIGMIX context");
        return 1;
    }
    if (c->frozen) return 0;
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    double *P = (double *)c->acc_f64.p;
    if (c->plan.kind == SNPGPU_PCA_COV) return snpgpu::ctx_settle(c);    // raw sums; the (n-1)/trace factor travels with the products
    if (c->plan.kind == SNPGPU_GRM_GCTA) {
        if (launch_gcta(c, P, 2)) return 1;
        c->colterm_pending = false;
        c->frozen_scale = 1.0;
    } else {
        if (check_out(c, SNPGPU_EIGMIX, SNPGPU_EIGMIX, 1, "snpgpu_finalize_inplace")) return 1;
        if (launch_fin_eigmix(c->stream, c->geom(), P, P + c->plane(), (const uint32_t *)c->samp_het.p,
                              (const double *)c->samp_dmiss.p, (const double *)c->samp_dsq.p, c->d_sumden(), diagadj,
                              scale, P, 2))
            return 1;
        c->frozen_diagadj = diagadj;
        c->frozen_scale = scale;
    }
    c->acc_f32_valid = false;
    c->frozen = true;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

__global__ __launch_bounds__(256) void panel_entries_kernel(const double *__restrict__ P, int64_t ld, int64_t tiles_c, int64_t col0,
                                                            const int64_t *__restrict__ rows, const int64_t *__restrict__ cols, int64_t n,
                                                            double *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = P[snpgpu::acc_off(ld, tiles_c, rows[k] - col0, cols[k] - col0)];
}

int snpgpu_panel_entries(snpgpu_ctx *c, const int64_t *rows, const int64_t *cols, int64_t n_entries, double *out)
{
    if (!c || !(c->plan.kind == SNPGPU_PCA_COV || ((c->plan.kind == SNPGPU_GRM_GCTA || c->plan.kind == SNPGPU_EIGMIX) && c->frozen))) {
        set_error("snpgpu_panel_entries: needs a PCA_COV context, or a GRM_GCTA / EIGMIX context after snpgpu_finalize_inplace");
        return 1;
    }
    if (n_entries <= 0) return 0;
    if (!rows || !cols || !out) { set_error("snpgpu_panel_entries: invalid arguments"); return 1; }
    for (int64_t k = 0; k < n_entries; k++)
        if (rows[k] < c->plan.row0 || rows[k] >= c->plan.row1 || cols[k] < rows[k] || cols[k] >= c->plan.N) {
            set_error("snpgpu_panel_entries: entry " + std::to_string(k) + " lies outside the panel's upper trapezoid");
            return 1;
        }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    if (ctx_settle(c)) return 1;
    DevBuf idx, res;
    if (idx.alloc(sizeof(int64_t) * 2 * (size_t)n_entries) || res.alloc(sizeof(double) * (size_t)n_entries)) { idx.release(); res.release(); return 1; }
    int rc = 0;
    do {
        if (hipMemcpyAsync(idx.p, rows, sizeof(int64_t) * (size_t)n_entries, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync((int64_t *)idx.p + n_entries, cols, sizeof(int64_t) * (size_t)n_entries, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = 1; break; }
        hipLaunchKernelGGL(panel_entries_kernel, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->acc_f64.p,
                           c->plan.ncols_pad, c->plan.acc_tiles_c, c->plan.col0, (const int64_t *)idx.p, (const int64_t *)idx.p + n_entries, n_entries, (double *)res.p);
        if (hipMemcpyAsync(out, res.p, sizeof(double) * (size_t)n_entries, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { rc = 1; break; }
    } while (0);
    idx.release(); res.release();
    if (rc) { set_error("snpgpu_panel_entries: copy or launch failed"); return 1; }
    return 0;
}

}  // extern "C"
