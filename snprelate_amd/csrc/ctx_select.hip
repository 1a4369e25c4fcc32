// Accumulator contexts, selection of related pairs and of the sparse GRM (kernels_select.hip): a count pass, a scan, a write pass of
// the stored length.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "ctx_plan.h"

using namespace snpgpu;

namespace {

// the refusals about capacity and outputs that every selection shares
int check_capacity(const std::string &f, int64_t capacity, const void *const *outs, int n_outs)
{
    if (capacity < 0) { set_error(f + ": negative capacity"); return 1; }
    if (capacity == 0)
        for (int k = 0; k < n_outs; k++)
            if (outs[k]) { set_error(f + ": capacity 0 with a non-NULL output (count only: every output NULL)"); return 1; }
    return 0;
}

}  // namespace

int snpgpu::select_check_opts(const char *fn, const snpgpu_sel_opts *o, int64_t capacity, const void *const *outs, int n_outs)
{
    const std::string f(fn);
    if (!o) { set_error(f + ": NULL opts"); return 1; }
    if (o->what != SNPGPU_SEL_KING_ROBUST && o->what != SNPGPU_SEL_KING_HOMO && o->what != SNPGPU_SEL_MOM) {
        set_error(f + ": invalid 'what' (SNPGPU_SEL_KING_ROBUST, SNPGPU_SEL_KING_HOMO or SNPGPU_SEL_MOM)");
        return 1;
    }
    if (o->what == SNPGPU_SEL_MOM && !o->e) { set_error(f + ": e is NULL (SNPGPU_SEL_MOM needs the five expectations)"); return 1; }
    return check_capacity(f, capacity, outs, n_outs);
}

int snpgpu::select_grm_check_opts(const char *fn, const snpgpu_grm_sel_opts *o, int64_t capacity, const void *const *outs, int n_outs)
{
    const std::string f(fn);
    if (!o) { set_error(f + ": NULL opts"); return 1; }
    if (o->what != SNPGPU_SEL_GRM_GCTA && o->what != SNPGPU_SEL_GRM_EIGENSTRAT && o->what != SNPGPU_SEL_GRM_EIGMIX &&
        o->what != SNPGPU_SEL_GRM_INDIV_BETA) {
        set_error(f + ": invalid 'what' (SNPGPU_SEL_GRM_GCTA, SNPGPU_SEL_GRM_EIGENSTRAT, SNPGPU_SEL_GRM_EIGMIX or SNPGPU_SEL_GRM_INDIV_BETA)");
        return 1;
    }
    if (o->what == SNPGPU_SEL_GRM_EIGMIX && !(std::isfinite(o->scale) && o->scale > 0)) {
        set_error(f + ": invalid scale (SNPGPU_SEL_GRM_EIGMIX needs a finite positive one)");
        return 1;
    }
    if (o->what == SNPGPU_SEL_GRM_EIGMIX && o->mode != 0 && o->mode != 1) { set_error(f + ": invalid mode (EIGMIX: diagadj 0 or 1)"); return 1; }
    if (o->what == SNPGPU_SEL_GRM_INDIV_BETA && (o->mode < 0 || o->mode > 2)) { set_error(f + ": invalid mode (INDIV_BETA: 0, 1 or 2)"); return 1; }
    return check_capacity(f, capacity, outs, n_outs);
}

namespace {

thread_local double g_sel_ms[4] = {0, 0, 0, 0};    // count pass, scan, write pass (device), whole call (host clock) of the last selection
thread_local double g_grm_ms[5] = {0, 0, 0, 0, 0}; // ... of the last GRM selection, with the diagonal kernel before the whole call

struct EvPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EvPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    int make() { SNPGPU_HIP_CHECK(hipEventCreate(&a)); SNPGPU_HIP_CHECK(hipEventCreate(&b)); return 0; }
    double ms() const { float t = 0; return (a && b && hipEventElapsedTime(&t, a, b) == hipSuccess) ? (double)t : 0.0; }
};

int select_launch(snpgpu_ctx *c, const snpgpu_sel_opts *o, const int32_t *dfam, const SelectArgs &a, bool write)
{
    const uint32_t *acc = (const uint32_t *)c->acc_u32.p;
    if (o->what == SNPGPU_SEL_KING_ROBUST) return launch_select_king_robust(c->stream, c->geom(), acc, dfam, a, write);
    if (o->what == SNPGPU_SEL_MOM) return launch_select_mom(c->stream, c->geom(), acc, o->e, o->kinship_constraint, a, write);
    const HomoTerms t = homo_terms(c);      // as snpgpu_king_homo
    return launch_select_king_homo(c->stream, c->geom(), acc, (const double *)c->acc_f64.p, t.fscale, t.w_const, t.msum, t.called, t.nosh, a, write);
}

// The one sequence of every selection, after its checks: the sample mask, the count pass, the scan, *n_found, then the write pass of
// min(capacity, found) pairs into the outputs that are present.  launch(args, write) starts a pass of the kind at hand;
// ms3 = {count pass, scan, write pass} on the device.
template <class Launch>
int select_run(snpgpu_ctx *c, const uint8_t *samp_sel, double cutoff, int64_t capacity, int32_t *idx1, int32_t *idx2, double *v0, double *v1,
               double *kin, int mem, int64_t *n_found, double *ms3, Launch &&launch)
{
    const int64_t n_seg = select_segments(c->geom());
    // scratch of this call: the sample mask, the segment counts and their offsets
    DevBuf dsel, dcnt, doff;
    if (samp_sel) {
        if (dsel.alloc((size_t)c->plan.N)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(dsel.p, samp_sel, (size_t)c->plan.N, hipMemcpyHostToDevice, c->stream));
    }
    if (dcnt.alloc(sizeof(uint32_t) * (size_t)n_seg) || doff.alloc(sizeof(int64_t) * (size_t)(n_seg + 1))) return 1;
    EvPair ev[3];
    for (EvPair &e : ev) if (e.make()) return 1;
    SelectArgs a{(const uint8_t *)(samp_sel ? dsel.p : nullptr), cutoff, (uint32_t *)dcnt.p, (int64_t *)doff.p, 0,
                 nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t total = 0;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[0].a, c->stream));
    if (launch(a, false)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[0].b, c->stream));
    SNPGPU_HIP_CHECK(hipEventRecord(ev[1].a, c->stream));
    if (launch_select_scan(c->stream, (const uint32_t *)dcnt.p, n_seg, (int64_t *)doff.p)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[1].b, c->stream));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(&total, (const int64_t *)doff.p + n_seg, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n_found) *n_found = total;
    ms3[0] = ev[0].ms(); ms3[1] = ev[1].ms(); ms3[2] = 0.0;
    const int64_t nw = std::min(capacity, total);
    if (nw > 0 && (idx1 || idx2 || v0 || v1 || kin)) {
        // host destinations go through temporaries of the stored length; absent outputs stay absent
        const size_t ni = sizeof(int32_t) * (size_t)nw, nd = sizeof(double) * (size_t)nw;
        OutBuf b1(c->stream, idx1, ni, mem), b2(c->stream, idx2, ni, mem), b3(c->stream, v0, nd, mem), b4(c->stream, v1, nd, mem),
               b5(c->stream, kin, nd, mem);
        std::vector<OutBuf *> present;
        for (OutBuf *b : {&b1, &b2, &b3, &b4, &b5}) if (b->user) present.push_back(b);
        const int rc = stage_out(c, present, [&] {
            a.capacity = nw;
            a.idx1 = (int32_t *)b1.dev; a.idx2 = (int32_t *)b2.dev; a.v0 = (double *)b3.dev; a.v1 = (double *)b4.dev; a.kin = (double *)b5.dev;
            SNPGPU_HIP_CHECK(hipEventRecord(ev[2].a, c->stream));
            if (launch(a, true)) return 1;
            SNPGPU_HIP_CHECK(hipEventRecord(ev[2].b, c->stream));
            return 0;
        });
        if (rc) return 1;
        ms3[2] = ev[2].ms();
    }
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_select_pairs(snpgpu_ctx *c, const snpgpu_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2, double *v0, double *v1,
                        double *kinship, int mem, int64_t *n_found)
{
    const char *fn = "snpgpu_select_pairs";
    const void *outs[5] = {idx1, idx2, v0, v1, kinship};
    if (select_check_opts(fn, o, capacity, outs, 5)) return 1;
    if (!c) { set_error(std::string(fn) + ": NULL context"); return 1; }
    if (c->plan.kind != select_kind(o->what)) {
        set_error(std::string(fn) + ": 'what' does not match the context kind (KING_ROBUST on a KING_ROBUST context, KING_HOMO on a KING_HOMO context, "
                                    "MOM on an IBS context)");
        return 1;
    }
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) { set_error(std::string(fn) + ": outputs go to host memory or to the context's device"); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    // the pending terms, as before a finaliser launch (settle, het_pending)
    if (check_out(c, c->plan.kind, c->plan.kind, 1, fn)) return 1;
    const int32_t *dfam = nullptr;
    if (upload_family(c, o->what == SNPGPU_SEL_KING_ROBUST ? o->family : nullptr, &dfam)) return 1;
    if (select_run(c, o->samp_sel, o->kinship_cutoff, capacity, idx1, idx2, v0, o->what == SNPGPU_SEL_KING_ROBUST ? nullptr : v1 /* not written for this kind */,
                   kinship, mem, n_found, g_sel_ms, [&](const SelectArgs &a, bool write) { return select_launch(c, o, dfam, a, write); }))
        return 1;
    g_sel_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

/* diagnostics of the last snpgpu_select_pairs of this thread: ms of {count pass, scan, write pass} on the device and of the whole call */
int snpgpu_select_stats(double *ms4)
{
    if (!ms4) { set_error("snpgpu_select_stats: NULL output"); return 1; }
    for (int k = 0; k < 4; k++) ms4[k] = g_sel_ms[k];
    return 0;
}

int snpgpu_select_grm(snpgpu_ctx *c, const snpgpu_grm_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2, double *value, double *diag,
                      double *avg_val, int64_t *n_found)
{
    const char *fn = "snpgpu_select_grm";
    const std::string f(fn);
    const void *outs[3] = {idx1, idx2, value};
    if (select_grm_check_opts(fn, o, capacity, outs, 3)) return 1;
    if (!c) { set_error(f + ": NULL context"); return 1; }
    if (c->plan.kind != select_grm_kind(o->what)) {
        set_error(f + ": 'what' does not match the context kind (GCTA on a GRM_GCTA context, EIGENSTRAT on a PCA_COV context, EIGMIX on an EIGMIX "
                      "context, INDIV_BETA on an INDIV_BETA context)");
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    // the pending terms as the kind's finaliser takes them: GCTA folds its column / row terms on the fly and does not settle them
    if (check_out(c, c->plan.kind, c->plan.kind, 1, fn, o->what != SNPGPU_SEL_GRM_GCTA)) return 1;
    const double *num = (const double *)c->acc_f64.p;
    // a plane times a factor: Eigenstrat, and the contexts finalised in place
    bool plain = false;
    double factor = 1.0, avg = 0, mn = 0;
    if (o->what == SNPGPU_SEL_GRM_GCTA) {
        plain = c->frozen;
    } else if (o->what == SNPGPU_SEL_GRM_EIGENSTRAT) {
        double tr = 0;                                          // the trace and the refusal of a panel without trace_in: snpgpu_pca_cov's
        if (snpgpu_pca_cov(c, nullptr, 1, 1, o->trace_in, &tr, SNPGPU_HOST)) return 1;
        if (o->trace_in > 0) tr = o->trace_in;
        plain = true;
        factor = (double)(c->plan.N - 1) / tr;
    } else if (o->what == SNPGPU_SEL_GRM_EIGMIX) {
        if (c->frozen) {
            if ((o->mode != 0) != (c->frozen_diagadj != 0)) { set_error(f + ": the context was finalised in place with another 'diagadj'"); return 1; }
            plain = true;
            factor = o->scale / c->frozen_scale;
        }
    } else {
        if (!c->plan.full) { set_error("snpgpu_indiv_beta: needs a full (non-panel) context"); return 1; }
        if (beta_terms(c, o->mode, &avg, &mn, fn)) return 1;
    }
    if (avg_val) *avg_val = avg;
    auto launch = [&](const SelectArgs &a, SelPass pass, double *d) {
        const PanelGeom g = c->geom();
        if (plain) return launch_select_cov(c->stream, g, num, factor, a, pass, d);
        if (o->what == SNPGPU_SEL_GRM_GCTA)
            return launch_select_gcta(c->stream, g, num, (const uint32_t *)c->acc_u32.p, (const uint32_t *)c->miss_diag.p, c->d_nlocus(),
                                      c->colterm_pending ? (const double *)c->colterm.p : nullptr,
                                      c->colterm_pending ? (const double *)c->uvterm.p : nullptr, a, pass, d);
        if (o->what == SNPGPU_SEL_GRM_EIGMIX)
            return launch_select_eigmix(c->stream, g, num, num + c->plane(), (const uint32_t *)c->samp_het.p, (const double *)c->samp_dmiss.p,
                                        (const double *)c->samp_dsq.p, c->d_sumden(), o->mode, o->scale, a, pass, d);
        return launch_select_beta(c->stream, g, (const uint32_t *)c->acc_u32.p, o->mode, avg, mn, a, pass, d);
    };
    if (select_run(c, o->samp_sel, o->cutoff, capacity, idx1, idx2, nullptr, nullptr, value, SNPGPU_HOST, n_found, g_grm_ms,
                   [&](const SelectArgs &a, bool write) { return launch(a, write ? SEL_WRITE : SEL_COUNT, nullptr); }))
        return 1;
    g_grm_ms[3] = 0.0;
    const int64_t n_diag = std::min(c->plan.row1, c->plan.N) - c->plan.row0;
    if (diag && n_diag > 0) {
        EvPair ev;
        if (ev.make()) return 1;
        OutBuf b(c->stream, diag, sizeof(double) * (size_t)n_diag, SNPGPU_HOST);
        const int rc = stage_out(c, {&b}, [&] {
            SNPGPU_HIP_CHECK(hipEventRecord(ev.a, c->stream));
            if (launch(SelectArgs{}, SEL_DIAG, (double *)b.dev)) return 1;
            SNPGPU_HIP_CHECK(hipEventRecord(ev.b, c->stream));
            return 0;
        });
        if (rc) return 1;
        g_grm_ms[3] = ev.ms();
    }
    g_grm_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

/* diagnostics of the last snpgpu_select_grm of this thread: ms of {count pass, scan, write pass, diagonal kernel} on the device and of the
 * whole call */
int snpgpu_select_grm_stats(double *ms5)
{
    if (!ms5) { set_error("snpgpu_select_grm_stats: NULL output"); return 1; }
    for (int k = 0; k < 5; k++) ms5[k] = g_grm_ms[k];
    return 0;
}

}  // extern "C"
