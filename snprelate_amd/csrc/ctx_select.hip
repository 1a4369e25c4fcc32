// Accumulator contexts, selection of related pairs (kernels_select.hip): a count pass, a scan, a write pass of the stored length.
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "ctx_plan.h"

using namespace snpgpu;

int snpgpu::select_check_opts(const char *fn, const snpgpu_sel_opts *o, int64_t capacity, const void *const *outs, int n_outs)
{
    const std::string f(fn);
    if (!o) { set_error(f + ": NULL opts"); return 1; }
    if (o->what != SNPGPU_SEL_KING_ROBUST && o->what != SNPGPU_SEL_KING_HOMO && o->what != SNPGPU_SEL_MOM) {
        set_error(f + ": invalid 'what' (SNPGPU_SEL_KING_ROBUST, SNPGPU_SEL_KING_HOMO or SNPGPU_SEL_MOM)");
        return 1;
    }
    if (o->what == SNPGPU_SEL_MOM && !o->e) { set_error(f + ": e is NULL (SNPGPU_SEL_MOM needs the five expectations)"); return 1; }
    if (capacity < 0) { set_error(f + ": negative capacity"); return 1; }
    if (capacity == 0)
        for (int k = 0; k < n_outs; k++)
            if (outs[k]) { set_error(f + ": capacity 0 with a non-NULL output (count only: every output NULL)"); return 1; }
    return 0;
}

namespace {

thread_local double g_sel_ms[4] = {0, 0, 0, 0};    // count pass, scan, write pass (device), whole call (host clock) of the last selection

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
    const PanelGeom g = c->geom();
    const int64_t n_seg = select_segments(g);
    const int32_t *dfam = nullptr;
    if (upload_family(c, o->what == SNPGPU_SEL_KING_ROBUST ? o->family : nullptr, &dfam)) return 1;
    // scratch of this call: the sample mask, the segment counts and their offsets
    DevBuf dsel, dcnt, doff;
    if (o->samp_sel) {
        if (dsel.alloc((size_t)c->plan.N)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(dsel.p, o->samp_sel, (size_t)c->plan.N, hipMemcpyHostToDevice, c->stream));
    }
    if (dcnt.alloc(sizeof(uint32_t) * (size_t)n_seg) || doff.alloc(sizeof(int64_t) * (size_t)(n_seg + 1))) return 1;
    EvPair ev[3];
    for (EvPair &e : ev) if (e.make()) return 1;
    SelectArgs a{(const uint8_t *)(o->samp_sel ? dsel.p : nullptr), o->kinship_cutoff, (uint32_t *)dcnt.p, (int64_t *)doff.p, 0,
                 nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t total = 0;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[0].a, c->stream));
    if (select_launch(c, o, dfam, a, false)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[0].b, c->stream));
    SNPGPU_HIP_CHECK(hipEventRecord(ev[1].a, c->stream));
    if (launch_select_scan(c->stream, (const uint32_t *)dcnt.p, n_seg, (int64_t *)doff.p)) return 1;
    SNPGPU_HIP_CHECK(hipEventRecord(ev[1].b, c->stream));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(&total, (const int64_t *)doff.p + n_seg, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n_found) *n_found = total;
    g_sel_ms[0] = ev[0].ms(); g_sel_ms[1] = ev[1].ms(); g_sel_ms[2] = 0.0;
    const int64_t nw = std::min(capacity, total);
    if (nw > 0 && (idx1 || idx2 || v0 || v1 || kinship)) {
        // host destinations go through temporaries of the stored length; absent outputs stay absent
        const size_t ni = sizeof(int32_t) * (size_t)nw, nd = sizeof(double) * (size_t)nw;
        OutBuf b1(c->stream, idx1, ni, mem), b2(c->stream, idx2, ni, mem), b3(c->stream, v0, nd, mem), b4(c->stream, v1, nd, mem),
               b5(c->stream, kinship, nd, mem);
        if (o->what == SNPGPU_SEL_KING_ROBUST) b4.user = nullptr;                // v1 is not written for this kind
        std::vector<OutBuf *> present;
        for (OutBuf *b : {&b1, &b2, &b3, &b4, &b5}) if (b->user) present.push_back(b);
        const int rc = stage_out(c, present, [&] {
            a.capacity = nw;
            a.idx1 = (int32_t *)b1.dev; a.idx2 = (int32_t *)b2.dev; a.v0 = (double *)b3.dev; a.v1 = (double *)b4.dev; a.kin = (double *)b5.dev;
            SNPGPU_HIP_CHECK(hipEventRecord(ev[2].a, c->stream));
            if (select_launch(c, o, dfam, a, true)) return 1;
            SNPGPU_HIP_CHECK(hipEventRecord(ev[2].b, c->stream));
            return 0;
        });
        if (rc) return 1;
        g_sel_ms[2] = ev[2].ms();
    }
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

}  // extern "C"
