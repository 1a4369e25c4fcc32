// Accumulator contexts, their life: buffers, work lists and tile tables from the plan (ctx_plan.h, worklist.h), create and destroy,
// the timing switch, and what a caller may ask of a context between feeds (sync, counts, slab size).
#include <memory>
#include <string>
#include <vector>

#include <rocblas/rocblas.h>

#include "ctx_plan.h"
#include "host_util.h"
#include "worklist.h"

using namespace snpgpu;

static TilePanel tile_panel(const CtxPlan &p) { return TilePanel{p.row0, p.row1, p.col0, p.N}; }

static int upload_tile_grid(snpgpu_ctx *c, TileGrid &tg, DevBuf &tab, int tile_r, int tile_c, int S)
{
    const TileGridPlan t = plan_tile_grid(tile_panel(c->plan), tile_r, tile_c, S);
    tg.tile_r = tile_r; tg.tile_c = tile_c; tg.super = S;
    tg.n_tr = t.n_tr; tg.n_tc = t.n_tc; tg.n_sr = t.n_sr; tg.n_super = t.n_super; tg.grid = t.grid;
    if (tab.alloc(sizeof(int) * (size_t)(2 * tg.n_sr + 2))) return 1;
    tg.d_prefix = (int *)tab.p;
    tg.d_first = tg.d_prefix + tg.n_sr + 1;
    SNPGPU_HIP_CHECK(hipMemcpy(tg.d_prefix, t.prefix.data(), sizeof(int) * t.prefix.size(), hipMemcpyHostToDevice));
    SNPGPU_HIP_CHECK(hipMemcpy(tg.d_first, t.first.data(), sizeof(int) * t.first.size(), hipMemcpyHostToDevice));
    return 0;
}

// a work list on the device; n_cu: the device's CUs.  256 threads x <= 256 VGPRs: two workgroups per CU (one with <= 512)
static int upload_worklist(snpgpu_ctx *c, int n_cu, int tile_r, int tile_c, int S, DevBuf &buf, int &n_blocks, int wg_per_cu = 2, int copies = 1)
{
    static_assert(sizeof(WorkItem) == sizeof(int4), "the kernels read a work item as one int4");
    const std::vector<WorkItem> work =
        build_worklist(tile_panel(c->plan), tile_r, tile_c, S, (int64_t)wg_per_cu * n_cu, c->plan.tail_parts /* SNPGPU_I8_TAIL_PARTS */, copies);
    n_blocks = (int)work.size();
    if (work.empty()) return 0;
    if (buf.alloc(sizeof(WorkItem) * work.size())) return 1;
    SNPGPU_HIP_CHECK(hipMemcpy(buf.p, work.data(), sizeof(WorkItem) * work.size(), hipMemcpyHostToDevice));
    return 0;
}

// events, streams and the rocBLAS handle go here, on the context's device; the buffers release themselves after this body
snpgpu_ctx::~snpgpu_ctx()
{
    (void)hipSetDevice(device);
    for (int k = 0; k < 2; k++) {
        if (ev_copied[k]) (void)hipEventDestroy(ev_copied[k]);
        if (ev_consumed[k]) (void)hipEventDestroy(ev_consumed[k]);
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (blas) (void)rocblas_destroy_handle((rocblas_handle)blas);
    for (int w = 0; w < 2; w++)
        for (auto &p : ev[w]) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

static int zero_now(DevBuf &b)
{
    SNPGPU_HIP_CHECK(hipMemset(b.p, 0, b.bytes));
    return 0;
}

// Buffers and work lists of a context, from its plan alone (ctx_plan.h says why each path exists); n_cu: the device's CUs
static int alloc_ctx(snpgpu_ctx *c, int n_cu)
{
    const CtxPlan &p = c->plan;
    const size_t plane = (size_t)c->plane(), B = (size_t)p.Bmax, nc = (size_t)p.ncols_pad, RB = (size_t)p.RB;
    if (c->packed.alloc(B * RB) || c->sum.alloc(sizeof(int32_t) * B) || c->num.alloc(sizeof(int32_t) * B)) return 1;
    if (p.kind == SNPGPU_EIGMIX &&
        (c->dvals.alloc(sizeof(double) * 2 * B) || c->samp_dsq.alloc(sizeof(double) * RB * 4) ||
         c->samp_het.alloc(sizeof(uint32_t) * RB * 4) || c->samp_dmiss.alloc(sizeof(double) * RB * 4)))
        return 1;
    if (c->scalars.alloc(8 * snpgpu_ctx::SCALAR_SLOTS)) return 1;
    // 16 entries per SNP pair, whole chunks; x 2: the exact-row tables of blocks without missing calls have 16-byte entries
    for (int i = 0; i < p.n_lut; i++)
        if (c->lut[i].alloc(sizeof(float2) * 8 * 2 * (B + 2048))) return 1;
    if (p.use_pc) {
        if (c->acc_u32.alloc(sizeof(uint32_t) * plane * (size_t)p.n_u32)) return 1;
        if (p.pc_i8) {
            // padding to 128 (fp4 product: 256) SNPs + 4 k-steps of read-ahead
            if (c->w2.alloc(sizeof(uint32_t) * (B / 16 + 32) * nc)) return 1;
            if (upload_worklist(c, n_cu, p.pc_tile_r, p.pc_tile_c, I8_SUPER, c->i8_work, c->i8_blocks, p.pc_wg_per_cu)) return 1;
            if (p.want_het) {
                // per sample: #het, then #(g == 2), over the blocks the two-product kernel took
                if (c->het.alloc(sizeof(uint32_t) * 2 * nc) || zero_now(c->het) || c->het_blk.alloc(sizeof(uint32_t) * 2 * nc) ||
                    zero_now(c->het_blk))
                    return 1;
                if (upload_worklist(c, n_cu, p.nm_tile_r, p.nm_tile_c, I8_SUPER, c->i8_work_nm, c->i8_blocks_nm, p.nm_wg_per_cu)) return 1;
            }
        } else {
            const size_t pv = (p.pc_mode == PM_GCTA_MISS) ? 4 : 16;  // bytes per (sample, 32-SNP word)
            if (c->rowp.alloc(pv * (size_t)p.rows_pad * (size_t)p.KWmax) || c->colp.alloc(pv * nc * (size_t)p.KWmax)) return 1;
            if (upload_tile_grid(c, c->tg_pc, c->tg_pc_tab, PC_TILE_R, PC_TILE_C, PC_SUPER)) return 1;
        }
        if (p.pc_mode == PM_GCTA_MISS && c->miss_diag.alloc(sizeof(uint32_t) * RB * 4)) return 1;
        if (p.gcta_sparse &&
            (c->mm256.alloc(32 * (nc / 256) * (size_t)plan_round_up(p.Bmax, 256)) || upload_worklist(c, n_cu, 256, 256, 4, c->sp_work, c->sp_blocks, 1)))
            return 1;
    }
    // single-product kernel: blocks padded to 1024 SNPs (one slot per SNP); + read-ahead rows (up to 24 groups)
    const size_t Bpad = (size_t)p.Bpad(), words = sizeof(uint32_t) * (Bpad / 8 + 96) * nc;
    if (p.use_mm) {
        if (c->wt.alloc(words) || c->acc_f64.alloc(sizeof(double) * plane * (size_t)p.n_f64)) return 1;
        if (upload_tile_grid(c, c->tg_mm, c->tg_mm_tab, MM_TILE_R, MM_TILE_C, MM_SUPER)) return 1;
        if (p.mm_h3 && upload_worklist(c, n_cu, H3_TILE_R, H3_TILE_C, p.h3_super, c->h3_work, c->h3_blocks)) return 1;
        if (p.want_x1_list && upload_worklist(c, n_cu, X1_TILE, X1_TILE, p.x1_super, c->x1_work, c->x1_blocks, 1)) return 1;
        if (p.eigmix_x1 && c->wt12.alloc(words)) return 1;
        if (p.h3_exact_rows &&
            (c->ccoef.alloc(sizeof(double2) * (B + 2048)) ||
             c->tcorr.alloc(sizeof(double) * ((p.uv_enabled ? 5 : 2) * Bpad / H3_LUTCH + 16) * nc) || c->colterm.alloc(sizeof(double) * nc)))
            return 1;
        if (p.uv_enabled &&
            (c->uvcoef.alloc(sizeof(double4) * (Bpad + 512)) || c->uvsp.alloc(sizeof(double4) * (Bpad + 512)) ||
             c->uvkpart.alloc(sizeof(double) * (Bpad / UV_CHUNK + 16)) || c->uvterm.alloc(sizeof(double) * (2 * nc + 2)) ||
             c->uvlut.alloc(64 * (Bpad + 2048)) ||                       // 16 entries of 8 bytes per slot pair, whole 1024-slot chunks
             c->uvslot.alloc(sizeof(int32_t) * (2 * Bpad + 64)) ||       // slot -> SNP, SNP -> slot
             // per SNP: {t, avg} (16 bytes), per SNP and target: relative error (float) and u | v << 16
             c->uvcand.alloc((Bpad + 64) * (16 + 8 * UV_QMAX))))
            return 1;
    }
    // the pace-maker (see syrk_uv16c_kernel): 64 KiB per table chunk, fetched by every workgroup alongside its 8 KiB of factors
    if (p.uvc() && (c->uvpace.alloc((size_t)65536 * (Bpad / UV_CHS + 4)) || zero_now(c->uvpace))) return 1;
    // the carry scratch beside it: nothing in a slot needs clearing (a work item's first run only writes), the flags start free
    if (p.uvc_carry_all && (c->uvcarry.alloc(uv_carry_scratch_bytes(p.uvc_carry_slots)) ||
                            c->uvcarry_flags.alloc(uv_carry_flag_bytes(p.uvc_carry_slots)) || zero_now(c->uvcarry_flags)))
        return 1;
    if (p.homo_uv) {
        for (int i = 0; i < p.homo_weights; i++)
            if (c->homo_lut[i].alloc(64 * (Bpad + 2048))) return 1;
        if (c->homo_wts.alloc(sizeof(double2) * (Bpad + 2048)) ||
            c->homo_tc.alloc(sizeof(double2) * (Bpad / (8 * (H3_LUTCH / 16)) + 16) * nc) ||   // one partial per 256 SNPs
            c->homo_msum.alloc(sizeof(double) * 2 * nc) || zero_now(c->homo_msum))
            return 1;
        // every weight in one launch: work items (tile, weight)
        if (upload_worklist(c, n_cu, X1_TILE, X1_TILE, H3_SUPER / 2, c->homo_work, c->homo_blocks, 1, p.homo_weights)) return 1;
        // (KING-homo divides by the same kind of sum: 0 / 0 = NaN for a sample without a call, as the dissimilarity)
        if (c->diss_called.alloc(sizeof(uint32_t) * nc) || zero_now(c->diss_called)) return 1;
        if (c->nosh.alloc(sizeof(uint32_t) * (size_t)nosh_words((int64_t)nc)) || zero_now(c->nosh)) return 1;
    }
    return 0;
}

// accumulators and running terms start at zero
static int zero_ctx(snpgpu_ctx *c)
{
    DevBuf *all[] = {&c->acc_u32, &c->acc_f64, &c->miss_diag, &c->colterm, &c->uvterm, &c->samp_het, &c->samp_dmiss, &c->samp_dsq, &c->scalars};
    hipError_t e = hipSuccess;
    for (DevBuf *b : all)
        if (e == hipSuccess && b->p) e = hipMemsetAsync(b->p, 0, b->bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { set_error(std::string("memset failed: ") + hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" {

int snpgpu_create(int kind, int64_t n_samp, const snpgpu_opts *opts, snpgpu_ctx **out)
{
    if (!out) { set_error("snpgpu_create: out is NULL"); return 1; }
    *out = nullptr;
    snpgpu_opts o{};
    if (opts) o = *opts;
    CtxPlan plan;
    std::string why;
    if (plan_context(kind, n_samp, o, Switches::from_env(), &plan, &why)) { set_error("snpgpu_create: " + why); return 1; }
    if (use_device("snpgpu_create", o.device)) return 1;
    // the kernels are written for gfx950 (MI355X) and nothing else: MX-fp4 matrix instructions, 160 KiB of LDS per workgroup,
    // 512 registers per lane.  A device of another architecture could not load the code objects; say so here rather than at
    // the first launch.
    hipDeviceProp_t prop;
    SNPGPU_HIP_CHECK(hipGetDeviceProperties(&prop, o.device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0 || prop.sharedMemPerBlock < 160 * 1024) {
        set_error(std::string("snpgpu_create: device ") + std::to_string(o.device) + " is " + prop.gcnArchName +
                  "; libsnpgpu is built for gfx950 (MI355X) only");
        return 1;
    }
    const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;    // (256: an MI355X, should the count be absent)
    std::unique_ptr<snpgpu_ctx> c(new snpgpu_ctx());
    c->plan = plan;
    c->device = o.device;
    if (o.stream) {
        c->stream = (hipStream_t)o.stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_error("snpgpu_create: hipStreamCreate failed"); return 1; }
        c->own_stream = true;
    }
    if (alloc_ctx(c.get(), n_cu) || zero_ctx(c.get())) {
        const std::string keep = snpgpu_last_error();
        set_error("snpgpu_create: " + keep);
        return 1;
    }
    *out = c.release();
    return 0;
}

int snpgpu_destroy(snpgpu_ctx *ctx)
{
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return 0;
}

int snpgpu_set_timing(snpgpu_ctx *c, int enable)
{
    if (!c) { set_error("snpgpu_set_timing: NULL context"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int w = 0; w < 2; w++) {
        for (auto &p : c->ev[w]) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        c->ev[w].clear();
    }
    c->timing = enable != 0;
    return 0;
}

int snpgpu_get_timing(snpgpu_ctx *c, int which, double *ms_sum, int64_t *launches)
{
    if (!c || which < 0 || which > 1) { set_error("snpgpu_get_timing: invalid arguments"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    double s = 0;
    for (auto &p : c->ev[which]) {
        float ms = 0;
        SNPGPU_HIP_CHECK(hipEventElapsedTime(&ms, p.first, p.second));
        s += ms;
    }
    if (ms_sum) *ms_sum = s;
    if (launches) *launches = (int64_t)c->ev[which].size();
    return 0;
}

int snpgpu_sync(snpgpu_ctx *c)
{
    if (!c) return 0;
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    if (c->copy_stream) SNPGPU_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int snpgpu_counts(snpgpu_ctx *c, int64_t *n_snp_total, int64_t *n_locus)
{
    if (!c) { set_error("snpgpu_counts: NULL context"); return 1; }
    if (n_snp_total) *n_snp_total = c->n_snp_total;
    if (n_locus) {
        SNPGPU_HIP_CHECK(hipSetDevice(c->device));
        unsigned long long v = 0;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(&v, c->d_nlocus(), sizeof(v), hipMemcpyDeviceToHost, c->stream));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
        *n_locus = (int64_t)v;
    }
    return 0;
}

int64_t snpgpu_slab_size(const snpgpu_ctx *c)
{
    if (!c) return 0;
    // rows row0..row1-1 of the packed triangle: sum over i of (N - i)
    const int64_t r = c->plan.row1 - c->plan.row0;
    return r * c->plan.N - (c->plan.row0 + c->plan.row1 - 1) * r / 2;
}

}  // extern "C"
