// Accumulator contexts, the feed: a block's way from the caller's rows through the pre-pass (stage_block) to the pair counters
// (feed_counters) and the SYRK tables (feed_syrk), as the context's plan says (ctx_plan.h).
#include <cstring>
#include <string>

#include "ctx_plan.h"

using namespace snpgpu;

namespace {
struct EvScope {   // records a start/stop event pair around one launch when timing is on
    snpgpu_ctx *c; int which; hipEvent_t a = nullptr, b = nullptr;
    EvScope(snpgpu_ctx *c_, int w) : c(c_), which(w)
    {
        if (!c->timing) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, c->stream);
    }
    ~EvScope()
    {
        if (!a) return;
        (void)hipEventRecord(b, c->stream);
        c->ev[which].push_back({a, b});
    }
};

struct Block {             // one feed block on its way through the context
    int64_t n_snp = 0;
    const void *src = nullptr;   // device rows as the caller laid them out
    int turn = -1;         // pinned feeds: the staging buffer that holds them (-1: none)
    bool direct = false;   // IBS / KING-robust fed with 2-bit rows: the counters' pre-pass reads `src` itself, nothing is repacked
};
}  // namespace

// per-SNP statistics handed in by the caller (snpgpu_feed_stats): the block's "holds missing calls" flag from them
extern "C" __global__ __launch_bounds__(256) void stats_flag_kernel(const int32_t *__restrict__ num, int64_t n_snp, int64_t N,
                                                         unsigned long long *__restrict__ d_missing)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n_snp && (int64_t)num[k] < N) *d_missing = 1ull;
}

// host copy, then (unless the block goes to the counters directly) the aligned 2-bit copy and the per-SNP statistics
static int stage_block(snpgpu_ctx *c, const void *geno, int format, int mem, const int32_t *ext_sum, const int32_t *ext_num, Block &b)
{
    const CtxPlan &p = c->plan;
    hipStream_t st = c->stream;
    const int64_t n_snp = b.n_snp;
    const size_t row_bytes = (size_t)(format == SNPGPU_GENO_U8 ? p.N : (p.N + 3) / 4);
    const size_t in_bytes = (size_t)n_snp * row_bytes, want = (size_t)p.Bmax * row_bytes;
    b.src = geno;
    if (mem == SNPGPU_HOST_PINNED) {
        if (!c->copy_stream) {
            SNPGPU_HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            for (int k = 0; k < 2; k++) {
                SNPGPU_HIP_CHECK(hipEventCreateWithFlags(&c->ev_copied[k], hipEventDisableTiming));
                SNPGPU_HIP_CHECK(hipEventCreateWithFlags(&c->ev_consumed[k], hipEventDisableTiming));
            }
        }
        const int turn = b.turn = c->raw_turn;
        c->raw_turn ^= 1;
        if (c->raw2[turn].bytes < in_bytes) {
            SNPGPU_HIP_CHECK(hipStreamSynchronize(st));
            SNPGPU_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
            c->raw2[turn].release();
            if (c->raw2[turn].alloc(want)) return 1;
        } else if (c->host_src[turn]) {
            // the device buffer may be overwritten only after the repack that read it
            SNPGPU_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->ev_consumed[turn], 0));
        }
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->raw2[turn].p, geno, in_bytes, hipMemcpyHostToDevice, c->copy_stream));
        SNPGPU_HIP_CHECK(hipEventRecord(c->ev_copied[turn], c->copy_stream));
        SNPGPU_HIP_CHECK(hipStreamWaitEvent(st, c->ev_copied[turn], 0));
        c->host_src[turn] = geno;
        b.src = c->raw2[turn].p;
    } else if (mem == SNPGPU_HOST) {
        if (c->raw.bytes < in_bytes) {  // host feeds are staged through a device copy of the raw block
            SNPGPU_HIP_CHECK(hipStreamSynchronize(st));
            c->raw.release();
            if (c->raw.alloc(want)) return 1;
        }
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->raw.p, geno, in_bytes, hipMemcpyHostToDevice, st));
        b.src = c->raw.p;
    }
    SNPGPU_HIP_CHECK(hipMemsetAsync(c->d_missing(), 0, sizeof(unsigned long long), st));
    SNPGPU_HIP_CHECK(hipMemsetAsync(c->d_short_runs(), 0, sizeof(unsigned long long), st));
    // IBS / KING-robust counters fed with 2-bit rows: one pre-pass kernel straight from the caller's block (no statistics
    // are needed by these kinds beyond the missing-call flag); SNPGPU_PREP_TWO_PASS=1 keeps the two-kernel form
    b.direct = p.use_pc && p.pc_i8 && !p.use_mm && (p.pc_mode == PM_IBS || p.pc_mode == PM_KING_ROBUST) &&
               format == SNPGPU_GENO_PACKED2 && (((p.N + 3) / 4) % 4) == 0 && !ext_sum &&
               (reinterpret_cast<uintptr_t>(b.src) & 3u) == 0 && !getenv("SNPGPU_PREP_TWO_PASS");
    if (b.direct) return 0;
    uint8_t *packed = (uint8_t *)c->packed.p;
    if (ext_sum) {
        // the caller computed this block's per-SNP statistics elsewhere (its share of the SNPs on every rank + an all-gather,
        // multigpu.py shared_stats): re-layout only, statistics and the missing-call flag from the arrays (device memory)
        if (launch_repack(st, b.src, format, n_snp, p.N, packed, p.RB)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->sum.p, ext_sum, sizeof(int32_t) * (size_t)n_snp, hipMemcpyDeviceToDevice, st));
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->num.p, ext_num, sizeof(int32_t) * (size_t)n_snp, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(stats_flag_kernel, dim3((unsigned)((n_snp + 255) / 256)), dim3(256), 0, st, (const int32_t *)c->num.p, n_snp, p.N,
                           c->d_missing());
    } else if (launch_repack_stats(st, b.src, format, n_snp, p.N, packed, p.RB, (int32_t *)c->sum.p, (int32_t *)c->num.p, c->d_missing()))
        return 1;
    if (b.turn >= 0) SNPGPU_HIP_CHECK(hipEventRecord(c->ev_consumed[b.turn], st));
    return 0;
}

// the general MFMA counter kernel (+ the two-product kernel of the blocks without missing calls) on the words in w2
static int launch_counters_i8(snpgpu_ctx *c, int64_t n_pad, int64_t n_snp, const unsigned long long *d_missing)
{
    const CtxPlan &p = c->plan;
    EvScope ev(c, 0);
    return launch_pair_i8(c->stream, p.pc_mode, (const int4 *)c->i8_work.p, c->i8_blocks, (const uint32_t *)c->w2.p, p.ncols_pad,
                          (int)(n_pad / 32), (int)n_snp, (uint32_t *)c->acc_u32.p, c->plane(), d_missing, (const int4 *)c->i8_work_nm.p,
                          c->i8_blocks_nm, p.nomiss_fp4, p.general_fp4);
}

static int feed_counters(snpgpu_ctx *c, const Block &b)
{
    const CtxPlan &p = c->plan;
    hipStream_t st = c->stream;
    const int64_t n_snp = b.n_snp;
    const uint8_t *packed = (const uint8_t *)c->packed.p;
    const int32_t *sum = (const int32_t *)c->sum.p, *num = (const int32_t *)c->num.p;
    uint32_t *w2 = (uint32_t *)c->w2.p, *acc = (uint32_t *)c->acc_u32.p;
    const int64_t n_pad = plan_round_up(n_snp, 256);    // whole loop rounds of the MFMA pair kernels (4 k-steps of 64 / up to 4 of 32 SNPs)
    const int KW = (int)(2 * ((n_snp + 63) / 64));
    if (b.direct) {
        if (launch_transpose2_direct(st, (const uint8_t *)b.src, p.N, n_snp, p.col0, p.ncols_pad, (int)(n_pad / 16), w2,
                                     (uint32_t *)c->het.p, (uint32_t *)c->het_blk.p, c->d_missing()))
            return 1;
        if (b.turn >= 0) SNPGPU_HIP_CHECK(hipEventRecord(c->ev_consumed[b.turn], st));
        if (p.want_het) c->het_pending = true;
        return launch_counters_i8(c, n_pad, n_snp, p.want_het ? c->d_missing() : nullptr);
    }
    if (p.pc_mode == PM_GCTA_MISS && p.pc_i8) {
        if (launch_transpose2_missmask(st, packed, p.RB, n_snp, p.N, sum, num, p.col0, p.ncols_pad, (int)(n_pad / 16), w2,
                                       (uint32_t *)c->miss_diag.p, c->d_missing()))
            return 1;
        const int64_t mm_stride = plan_round_up(p.Bmax, 256);
        if (p.gcta_sparse) {      // the block's route (device side): sparse sets up to sp_max_rate missing calls, the dense product beyond
            const unsigned long long max_cells = (unsigned long long)(p.sp_max_rate * (double)p.N * (double)n_snp);
            if (launch_missmask256(st, packed, p.RB, n_snp, p.N, sum, num, p.col0, (int)(p.ncols_pad / 256), mm_stride, (uint4 *)c->mm256.p,
                                   max_cells, c->d_miss_route()))
                return 1;
        }
        EvScope ev(c, 0);
        if (p.gcta_sparse && launch_pair_sparse_miss(st, (const uint4 *)c->mm256.p, mm_stride, (int)n_snp, acc, p.ncols_pad,
                                                     (const int4 *)c->sp_work.p, c->sp_blocks, c->d_miss_route()))
            return 1;
        const unsigned long long *run = p.gcta_sparse ? c->d_miss_route() + 1 : c->d_missing();
        return p.miss_fp4 ? launch_pair_fp4_miss(st, (const int4 *)c->i8_work.p, c->i8_blocks, w2, p.ncols_pad, (int)(n_pad / 64), acc, run)
                          : launch_pair_i8(st, p.pc_mode, (const int4 *)c->i8_work.p, c->i8_blocks, w2, p.ncols_pad, (int)(n_pad / 32),
                                           (int)n_snp, acc, c->plane(), run);
    }
    if (p.pc_i8) {
        // (+ per-sample het counts of a block without missing calls, for the binary pair kernel)
        if (launch_transpose2(st, packed, p.RB, n_snp, p.col0, p.ncols_pad, (int)(n_pad / 16), w2, (uint32_t *)c->het.p, c->d_missing()))
            return 1;
        if (p.want_het) c->het_pending = true;
        return launch_counters_i8(c, n_pad, n_snp, p.want_het ? c->d_missing() : nullptr);
    }
    // bit planes + popcounts
    const bool gcta = p.pc_mode == PM_GCTA_MISS;
    if (gcta) {
        if (launch_bitplanes_miss(st, packed, p.RB, n_snp, p.N, sum, num, p.col0, p.ncols_pad, p.rows_pad, KW, (uint2 *)c->rowp.p,
                                  (uint2 *)c->colp.p, c->d_missing()) ||
            launch_miss_diag(st, (const uint2 *)c->colp.p, KW / 2, p.ncols_pad, p.col0, (uint32_t *)c->miss_diag.p, c->d_missing()))
            return 1;
    } else if (launch_bitplanes4(st, packed, p.RB, n_snp, p.N, p.col0, p.ncols_pad, p.rows_pad, KW, (uint4 *)c->rowp.p, (uint4 *)c->colp.p))
        return 1;
    EvScope ev(c, 0);
    return launch_pair_popcount(st, p.pc_mode, c->tg_pc, c->rowp.p, c->colp.p, KW, p.ncols_pad, acc, c->plane(), gcta ? c->d_missing() : nullptr);
}

// tables, words and products of the block's SYRK tables (run geometry: ctx_plan.h, plan_block)
static int feed_syrk(snpgpu_ctx *c, int64_t n_snp)
{
    const CtxPlan &p = c->plan;
    hipStream_t st = c->stream;
    const uint8_t *packed = (const uint8_t *)c->packed.p;
    const int32_t *sum = (const int32_t *)c->sum.p, *num = (const int32_t *)c->num.p;
    const uint32_t *wt = (const uint32_t *)c->wt.p;
    const BlockRuns b = plan_block(p, n_snp);
    const int64_t n_pad = b.n_pad;        // = the single-product kernel's K dimension: one slot per SNP
    const bool entry12 = c->x1_blocks > 0;     // 12-byte table entries (the syrk_x1_kernel list exists)
    int32_t *slot_src = (int32_t *)c->uvslot.p, *slot_of = slot_src ? slot_src + (c->uvslot.bytes / 8) : nullptr;
    // tables, row / column coefficients and the slot -> SNP map of a block without missing calls (table 0 of GRM / PCA /
    // EIGMIX contexts) come first: the transposition below follows the map
    if (p.uv_enabled && p.h3_a_kind[0] == 0) {
        char *cb = (char *)c->uvcand.p;
        const size_t nmax = c->uvcand.bytes / (16 + 8 * UV_QMAX);
        BuildUvOpts o;
        o.lut_mode = p.lut_mode[0];
        o.lut = (uint2 *)c->uvlut.p; o.uvcoef = (double4 *)c->uvcoef.p; o.kpart = (double *)c->uvkpart.p; o.uvsp = (double4 *)c->uvsp.p;
        o.cand_err = (float *)(cb + 16 * nmax); o.cand_uv = (uint32_t *)(cb + (16 + 4 * UV_QMAX) * nmax); o.snp_tavg = (double2 *)cb;
        o.slot_of = slot_of; o.slot_src = slot_src;
        o.n_target = b.uv_q; o.cpr = b.uv_cpr;
        o.d_missing = c->d_missing();
        o.form = p.uv_form;
        if (launch_build_uv(st, sum, num, n_snp, n_pad, o)) return 1;
    }
    {
        Transpose8Opts o;
        o.n_d = (int)(n_pad / 8); o.w8 = (uint32_t *)c->wt.p;
        o.d_block_flag = p.wt_block_flag ? c->d_missing() : nullptr;
        o.layout = p.wt_layout;
        o.slot_src = b.uv_q > 1 ? slot_src : nullptr;
        o.nibble_nomiss = p.uvc();
        if (launch_transpose8(st, packed, p.RB, n_snp, p.col0, p.ncols_pad, o)) return 1;
        if (p.eigmix_x1) {
            Transpose8Opts o12;
            o12.n_d = (int)(n_pad / 8); o12.w8 = (uint32_t *)c->wt12.p;
            o12.d_block_flag = c->d_missing();
            o12.layout = WordLayout::Entry12Missing;
            if (launch_transpose8(st, packed, p.RB, n_snp, p.col0, p.ncols_pad, o12)) return 1;
        }
    }
    // KING-homo: in a block without missing calls the masked weight sums are the same for every pair -- the table
    // pass adds them to two scalars, the SYRK of both tables exits (and the two-product counter kernel takes the block)
    const bool homo_nm = (p.kind == SNPGPU_KING_HOMO || p.kind == SNPGPU_DISS) && p.want_het;
    const bool short_runs = p.sparse_missing && p.x1_short_runs;
    for (int i = 0; i < p.n_lut; i++) {
        const bool eig0 = (p.kind == SNPGPU_EIGMIX && i == 0);
        const bool exact_rows = (p.h3_a_kind[i] == 0);      // (table 0 only)
        const bool uv = exact_rows && p.uv_enabled;
        {
            BuildLutOpts o;
            o.lut_mode = p.lut_mode[i]; o.split16 = p.mm_h3; o.lut = (float2 *)c->lut[i].p;
            o.d_nlocus = (i == 0 && p.kind == SNPGPU_GRM_GCTA) ? c->d_nlocus() : nullptr;
            o.d_sumden = eig0 ? c->d_sumden() : nullptr; o.dvals = eig0 ? (double *)c->dvals.p : nullptr;
            o.d_missing = c->d_missing();
            o.ccoef = (i == 0 && p.h3_exact_rows) ? (double2 *)c->ccoef.p : nullptr;
            o.exact_rows_always = p.h3_a_kind[i] > 0;
            o.w_shift = p.h3_w_shift;
            o.exact_with_missing = p.h3_exact_missing || (i == 0 && p.eigmix_x1);
            o.entry12 = i == 0 && entry12;
            o.homo_const = homo_nm ? c->d_homo_w() + i : nullptr;
            o.uvsp_miss = (i == 0 && p.sparse_missing) ? (double4 *)c->uvsp.p : nullptr;
            o.x1_sparse_mac = p.x1_sparse_mac;
            o.d_short_runs = (i == 0 && short_runs) ? c->d_short_runs() : nullptr;
            if (launch_build_lut(st, sum, num, n_snp, n_pad, o)) return 1;
        }
        // (EIGMIX with the single-product kernel: its exact-row kernel never runs, no column term)
        if (exact_rows && !p.uv_eigmix && launch_colcorr(st, wt, p.ncols_pad, (int)(n_pad / 8), (const double2 *)c->ccoef.p, (double *)c->tcorr.p,
                                                         (double *)c->colterm.p, c->d_missing(),
                                                         uv ? ColcorrBlocks::WithMissing : p.h3_exact_missing ? ColcorrBlocks::Every : ColcorrBlocks::WithoutMissing,
                                                         entry12 ? 1 : 0))
            return 1;
        if (uv) {     // a block without missing calls: rare variants in fp64, row / column terms of every slot
            if (launch_uv_sparse(st, packed, p.RB, n_snp, p.N, p.row0, p.row1, p.col0, (const double4 *)c->uvsp.p, c->plane_f64(i), p.ncols_pad,
                                 p.acc_tiles_c, p.ncols_pad, (double *)c->uvterm.p, c->d_missing()) ||
                launch_uvcorr(st, wt, p.ncols_pad, (int)(n_pad / 8), (const double4 *)c->uvcoef.p, (const double *)c->uvkpart.p,
                              (int)(n_pad / UV_CHUNK), (double2 *)c->tcorr.p, (double *)c->uvterm.p, c->d_missing(), p.uvc() ? 1 : 0))
                return 1;
        }
        // a block WITH missing calls: what the carriers of its rare variants lack in the exact-row product
        if (exact_rows && p.sparse_missing &&
            launch_uv_sparse(st, packed, p.RB, n_snp, p.N, p.row0, p.row1, p.col0, (const double4 *)c->uvsp.p, c->plane_f64(i), p.ncols_pad,
                             p.acc_tiles_c, p.ncols_pad, (double *)c->uvterm.p, c->d_missing(), 1))
            return 1;
        // EIGMIX numerator of a block with missing calls: the exact-row kernel's column term from the 12 * code words
        if (exact_rows && p.eigmix_x1 && launch_colcorr(st, (const uint32_t *)c->wt12.p, p.ncols_pad, (int)(n_pad / 8), (const double2 *)c->ccoef.p,
                                                        (double *)c->tcorr.p, (double *)c->colterm.p, c->d_missing(), ColcorrBlocks::WithMissing, 1))
            return 1;
        if (exact_rows) c->colterm_pending = true;
        if (eig0 && launch_eigmix_samples(st, wt, (int)(n_pad / 8), p.ncols_pad, p.col0, (const double *)c->dvals.p, (uint32_t *)c->samp_het.p,
                                          (double *)c->samp_dmiss.p, (double *)c->samp_dsq.p, p.wt_block_flag ? c->d_missing() : nullptr))
            return 1;
        // the weighted both-missing sums are only needed for blocks that contain missing calls
        const unsigned long long *skip = (p.lut_mode[i] == LUT_EIGMIX_MISSW || uv || homo_nm) ? c->d_missing() : nullptr;
        if (p.homo_uv) {
            // KING-homo block with missing calls: tables, effective weights, totals and per-sample missing sums of BOTH weights
            // once (i == 0), then ONE single-product launch: work items (tile, weight), the copy index picks table and plane
            const bool one_w = p.homo_weights == 1;      // dissimilarity: the first weight only
            if (i == 0 && launch_diss_called(st, packed, p.RB, n_snp, sum, num, p.col0, p.N - p.col0, (uint32_t *)c->diss_called.p))
                return 1;
            if (i == 0 && launch_nosh_block(st, packed, p.RB, n_snp, sum, num, p.col0, p.N - p.col0, p.ncols_pad, (uint32_t *)c->nosh.p))
                return 1;
            if (i == 0 && (launch_homo_tables(st, sum, num, n_snp, n_pad, (uint2 *)c->homo_lut[0].p, (uint2 *)c->homo_lut[1].p,
                                              (double2 *)c->homo_wts.p, c->d_homo_w(), c->d_missing(),
                                              p.homo_form == UvForm::Lookup16x16x32 ? 1 : 0, p.homo_weights) ||
                           launch_homo_miss_sums(st, wt, p.ncols_pad, (int)(n_pad / 8), (const double2 *)c->homo_wts.p, (double2 *)c->homo_tc.p,
                                                 (double *)c->homo_msum.p, c->d_missing())))
                return 1;
            SyrkUvOpts o;
            o.work_x1 = (const int4 *)c->homo_work.p; o.n_blocks_x1 = c->homo_blocks;
            o.lut = (const uint2 *)c->homo_lut[0].p; o.n_q = b.n_q;
            o.d_missing = c->d_missing();
            o.run_if_missing = true;
            o.copy_lut_bytes = one_w ? 0 : (int64_t)((const char *)c->homo_lut[1].p - (const char *)c->homo_lut[0].p);
            o.copy_acc_elems = c->plane();
            o.form = p.homo_form;
            o.n_launched = &c->syrk_launches;
            EvScope ev(c, 1);      // (one span per table, as the timing has always counted them)
            if (i == 0 && launch_syrk_uv(st, c->syrk_panel(c->wt, 0), o)) return 1;
            continue;
        }
        EvScope ev(c, 1);
        if (!p.mm_h3) {
            c->syrk_launches++;
            if (launch_syrk(st, c->tg_mm, wt, p.ncols_pad, (const float2 *)c->lut[i].p, b.n_q, c->plane_f64(i), p.ncols_pad, p.acc_tiles_c, skip))
                return 1;
            continue;
        }
        const bool x1e = exact_rows && p.eigmix_x1;       // EIGMIX numerator: exact-row kernel on its own words
        const bool x1m = exact_rows && (p.h3_exact_missing || x1e);
        SyrkH3Opts h;
        h.work = (const int4 *)c->h3_work.p; h.n_blocks = c->h3_blocks;
        h.lut = (const uint2 *)c->lut[i].p; h.n_q = b.n_q;
        h.d_skip_if_zero = skip;
        h.a_kind = p.h3_a_kind[i];
        h.d_missing = x1m ? nullptr : c->d_missing();
        h.promote_snps = p.h3_promote;
        h.work_x1 = (x1m && c->x1_blocks) ? (const int4 *)c->x1_work.p : nullptr; h.n_blocks_x1 = c->x1_blocks;
        h.d_short_runs = (i == 0 && short_runs) ? c->d_short_runs() : nullptr;
        h.n_launched = &c->syrk_launches;
        if (launch_syrk_h3(st, c->syrk_panel(x1e ? c->wt12 : c->wt, i), h)) return 1;
        if (uv) {
            SyrkUvOpts o;
            o.work_x1 = (const int4 *)c->x1_work.p; o.n_blocks_x1 = c->x1_blocks;
            o.lut = (const uint2 *)c->uvlut.p; o.n_q = b.n_q;
            o.d_missing = c->d_missing();
            o.run_chunks = b.uv_runs > 1 ? b.uv_cpr : 0; o.n_target = b.uv_q;
            o.form = p.uv_form;
            o.pace_src = c->uvpace.p; o.pace = p.uvc_pace;
            o.n_launched = &c->syrk_launches;
            if (p.uvc_carry_all) { o.carry_scr = c->uvcarry.p; o.carry_flags = (unsigned int *)c->uvcarry_flags.p; o.carry_slots = p.uvc_carry_slots; }
            if (launch_syrk_uv(st, c->syrk_panel(c->wt, i), o)) return 1;
        }
    }
    return 0;
}

static int feed_impl(snpgpu_ctx *c, const void *geno, int64_t n_snp, int format, int mem, const int32_t *ext_sum, const int32_t *ext_num)
{
    if (!c) { set_error("snpgpu_feed: NULL context"); return 1; }
    if (n_snp == 0) return 0;
    if (!geno || n_snp < 0) { set_error("snpgpu_feed: invalid block"); return 1; }
    if (n_snp > c->plan.Bmax) { set_error("snpgpu_feed: block larger than max_block_snps"); return 1; }
    if (c->frozen) { set_error("snpgpu_feed: the context was finalised in place (snpgpu_finalize_inplace); no blocks may follow"); return 1; }
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) { set_error("snpgpu_feed: invalid format"); return 1; }
    if (c->plan.kind == SNPGPU_KING_ROBUST && c->n_snp_total + n_snp >= 1073741824LL) {
        // guard of gnrIBD_KING_Robust, src/genKING.cpp:598-602
        set_error("The number of SNPs should be less than 1,073,741,824.");
        return 1;
    }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    Block b;
    b.n_snp = n_snp;
    if (stage_block(c, geno, format, mem, ext_sum, ext_num, b)) return 1;
    if (c->plan.use_pc && feed_counters(c, b)) return 1;
    if (c->plan.use_mm && feed_syrk(c, n_snp)) return 1;
    c->n_snp_total += n_snp;
    c->acc_f32_valid = false;       // (the eigen solver's fp32 copy of the sums is stale now)
    c->diag_mirrored = 0;           // (... and so are the lower triangles it mirrored: the feed kernels add no transposes below the diagonal)
    if (mem == SNPGPU_HOST) SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));  // caller may reuse its buffer
    return 0;
}

extern "C" {

int snpgpu_feed(snpgpu_ctx *c, const void *geno, int64_t n_snp, int format, int mem)
{
    return feed_impl(c, geno, n_snp, format, mem, nullptr, nullptr);
}

int snpgpu_feed_stats(snpgpu_ctx *c, const void *geno, int64_t n_snp, int format, int mem, const int32_t *sum, const int32_t *num)
{
    if (!sum || !num) { set_error("snpgpu_feed_stats: NULL statistics"); return 1; }
    return feed_impl(c, geno, n_snp, format, mem, sum, num);
}

int snpgpu_block_stats(snpgpu_ctx *c, const void *geno, int64_t n_snp, int format, int32_t *sum, int32_t *num)
{
    if (!c || !geno || !sum || !num || n_snp < 0 || n_snp > c->plan.Bmax) { set_error("snpgpu_block_stats: invalid arguments"); return 1; }
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) { set_error("snpgpu_block_stats: invalid format"); return 1; }
    if (n_snp == 0) return 0;
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    // (the aligned 2-bit copy lands in the context's own block buffer, which the next feed rewrites anyway; the flag word is
    // cleared by that feed as well)
    return launch_repack_stats(c->stream, geno, format, n_snp, c->plan.N, (uint8_t *)c->packed.p, c->plan.RB, sum, num, c->d_missing());
}

int snpgpu_host_wait(snpgpu_ctx *c, const void *host_buf)
{
    if (!c) { set_error("snpgpu_host_wait: NULL context"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    for (int k = 0; k < 2; k++)
        if (c->host_src[k] == host_buf && c->ev_copied[k]) SNPGPU_HIP_CHECK(hipEventSynchronize(c->ev_copied[k]));
    return 0;
}

}  // extern "C"
