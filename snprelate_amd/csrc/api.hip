// C ABI of libsnpgpu, level (1): streaming accumulator contexts (include/snpgpu.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include <rocblas/rocblas.h>

#include <chrono>

#include "ctx_plan.h"
#include "host_util.h"

namespace snpgpu {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

}  // namespace snpgpu

using namespace snpgpu;

static int build_tile_grid(snpgpu_ctx *c, TileGrid &tg, DevBuf &tab, int tile_r, int tile_c, int S)
{
    tg.tile_r = tile_r; tg.tile_c = tile_c; tg.super = S;
    tg.n_tr = (int)((c->plan.row1 - c->plan.row0 + tile_r - 1) / tile_r);
    tg.n_tc = (int)((c->plan.N - c->plan.col0 + tile_c - 1) / tile_c);
    tg.n_sr = (tg.n_tr + S - 1) / S;
    const int n_sc = (tg.n_tc + S - 1) / S;
    std::vector<int> prefix(tg.n_sr + 1, 0), first(tg.n_sr, 0);
    for (int sr = 0; sr < tg.n_sr; sr++) {
        // first super-column whose last sample column reaches the first row of this super-row
        const int64_t row_lo = (int64_t)sr * S * tile_r;
        int f = (int)(row_lo / ((int64_t)S * tile_c));
        if (f > n_sc) f = n_sc;
        first[sr] = f;
        prefix[sr + 1] = prefix[sr] + (n_sc - f);
    }
    tg.n_super = prefix[tg.n_sr];
    tg.grid = 8 * S * S * ((tg.n_super + 7) / 8);
    if (tab.alloc(sizeof(int) * (size_t)(2 * tg.n_sr + 2))) return 1;
    tg.d_prefix = (int *)tab.p;
    tg.d_first = tg.d_prefix + tg.n_sr + 1;
    SNPGPU_HIP_CHECK(hipMemcpy(tg.d_prefix, prefix.data(), sizeof(int) * prefix.size(), hipMemcpyHostToDevice));
    SNPGPU_HIP_CHECK(hipMemcpy(tg.d_first, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice));
    return 0;
}

// Work list of the int8 pair kernel and of the split-fp16 SYRK.  Tiles touching the upper trapezoid of the panel are grouped in
// S x S super-tiles; super-tile k goes to XCD k % 8 (workgroup b runs on XCD b % 8), so the tiles that are
// resident together on one XCD share operand rows/columns in its L2.  The chip runs `slots` workgroups
// at a time; the tiles of the last, partially filled round are split along K into the number of parts
// that makes that round shortest (their counters are flushed with atomics, so parts may share a tile).
// copies > 1: every tile appears `copies` times (copy index in bits 16.. of the item's fourth field): several independent
// products over the same tiles in ONE launch (KING-homo's two weight sums), balanced together
static int build_worklist(snpgpu_ctx *c, int tile_r, int tile_c, int S, DevBuf &buf, int &n_blocks, int wg_per_cu = 2, int copies = 1)
{
    const int n_tr = (int)((c->plan.row1 - c->plan.row0 + tile_r - 1) / tile_r);
    const int n_tc = (int)((c->plan.N - c->plan.col0 + tile_c - 1) / tile_c);
    const int n_sr = (n_tr + S - 1) / S, n_sc = (n_tc + S - 1) / S;
    // (tile row, tile column | copy << 20): the copy index travels in the column field until the items are written
    std::vector<std::vector<std::pair<int, int>>> queue(8);
    int k = 0;
    for (int sr = 0; sr < n_sr; sr++)
        for (int sc = 0; sc < n_sc; sc++) {
            std::vector<std::pair<int, int>> tiles;
            for (int a = 0; a < S; a++)
                for (int b = 0; b < S; b++) {
                    const int tr = sr * S + a, tc = sc * S + b;
                    if (tr < n_tr && tc < n_tc && (int64_t)(tc + 1) * tile_c > (int64_t)tr * tile_r)
                        for (int cp = 0; cp < copies; cp++) tiles.push_back({tr, tc | (cp << 20)});
                }
            if (tiles.empty()) continue;
            auto &q = queue[k++ & 7];
            q.insert(q.end(), tiles.begin(), tiles.end());
        }
    // even out the queues (diagonal super-tiles are smaller): move tiles from the longest to the shortest
    for (;;) {
        int lo = 0, hi = 0;
        for (int x = 1; x < 8; x++) {
            if (queue[x].size() < queue[lo].size()) lo = x;
            if (queue[x].size() > queue[hi].size()) hi = x;
        }
        if (queue[hi].size() <= queue[lo].size() + 1) break;
        queue[lo].push_back(queue[hi].back());
        queue[hi].pop_back();
    }
    int64_t T = 0;
    for (auto &q : queue) T += (int64_t)q.size();
    int ncu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    const int64_t slots = (int64_t)wg_per_cu * ncu;  // 256 threads x <= 256 VGPRs: two workgroups per CU (one with <= 512)
    const int64_t rem = T % slots;
    int parts = 1;
    if (rem > 0) {
        double best = 1.0;                           // duration of the last round in units of a whole tile
        for (int p = 2; p <= 8; p++) {
            const double d = (double)((rem * p + slots - 1) / slots) / p + 0.02 * (p - 1);   // + flush overhead
            if (d < best - 1e-9) { best = d; parts = p; }
        }
    }
    if (c->plan.tail_parts) parts = c->plan.tail_parts;      // SNPGPU_I8_TAIL_PARTS
    // split the last `rem` tiles, rem/8 from the end of every queue
    std::vector<int4> work;
    size_t longest = 0;
    std::vector<std::vector<int4>> items(8);
    for (int x = 0; x < 8; x++) {
        const auto &q = queue[x];
        const size_t n_split = (parts > 1) ? std::min(q.size(), (size_t)((rem + 7 - x) / 8)) : 0;
        for (size_t i = 0; i < q.size() - n_split; i++)
            items[x].push_back(make_int4(q[i].first, q[i].second & 0xFFFFF, 0, 1 | ((q[i].second >> 20) << 16)));
        for (int p = 0; p < parts; p++)
            for (size_t i = q.size() - n_split; i < q.size(); i++)
                items[x].push_back(make_int4(q[i].first, q[i].second & 0xFFFFF, p, parts | ((q[i].second >> 20) << 16)));
        longest = std::max(longest, items[x].size());
    }
    work.assign(longest * 8, make_int4(0, 0, 0, 0));
    for (int x = 0; x < 8; x++)
        for (size_t i = 0; i < items[x].size(); i++) work[i * 8 + x] = items[x][i];
    n_blocks = (int)work.size();
    if (work.empty()) return 0;
    if (buf.alloc(sizeof(int4) * work.size())) return 1;
    SNPGPU_HIP_CHECK(hipMemcpy(buf.p, work.data(), sizeof(int4) * work.size(), hipMemcpyHostToDevice));
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

// Buffers and work lists of a context, from its plan alone (ctx_plan.h says why each path exists).
static int alloc_ctx(snpgpu_ctx *c)
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
            if (build_worklist(c, p.pc_tile_r, p.pc_tile_c, I8_SUPER, c->i8_work, c->i8_blocks, p.pc_wg_per_cu)) return 1;
            if (p.want_het) {
                // per sample: #het, then #(g == 2), over the blocks the two-product kernel took
                if (c->het.alloc(sizeof(uint32_t) * 2 * nc) || zero_now(c->het) || c->het_blk.alloc(sizeof(uint32_t) * 2 * nc) ||
                    zero_now(c->het_blk))
                    return 1;
                if (build_worklist(c, p.nm_tile_r, p.nm_tile_c, I8_SUPER, c->i8_work_nm, c->i8_blocks_nm, p.nm_wg_per_cu)) return 1;
            }
        } else {
            const size_t pv = (p.pc_mode == PM_GCTA_MISS) ? 4 : 16;  // bytes per (sample, 32-SNP word)
            if (c->rowp.alloc(pv * (size_t)p.rows_pad * (size_t)p.KWmax) || c->colp.alloc(pv * nc * (size_t)p.KWmax)) return 1;
            if (build_tile_grid(c, c->tg_pc, c->tg_pc_tab, PC_TILE_R, PC_TILE_C, PC_SUPER)) return 1;
        }
        if (p.pc_mode == PM_GCTA_MISS && c->miss_diag.alloc(sizeof(uint32_t) * RB * 4)) return 1;
        if (p.gcta_sparse &&
            (c->mm256.alloc(32 * (nc / 256) * (size_t)round_up(p.Bmax, 256)) || build_worklist(c, 256, 256, 4, c->sp_work, c->sp_blocks, 1)))
            return 1;
    }
    // single-product kernel: blocks padded to 1024 SNPs (one slot per SNP); + read-ahead rows (up to 24 groups)
    const size_t Bpad = (size_t)p.Bpad(), words = sizeof(uint32_t) * (Bpad / 8 + 96) * nc;
    if (p.use_mm) {
        if (c->wt.alloc(words) || c->acc_f64.alloc(sizeof(double) * plane * (size_t)p.n_f64)) return 1;
        if (build_tile_grid(c, c->tg_mm, c->tg_mm_tab, MM_TILE_R, MM_TILE_C, MM_SUPER)) return 1;
        if (p.mm_h3 && build_worklist(c, H3_TILE_R, H3_TILE_C, p.h3_super, c->h3_work, c->h3_blocks)) return 1;
        if (p.want_x1_list && build_worklist(c, X1_TILE, X1_TILE, p.x1_super, c->x1_work, c->x1_blocks, 1)) return 1;
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
        if (build_worklist(c, X1_TILE, X1_TILE, H3_SUPER / 2, c->homo_work, c->homo_blocks, 1, p.homo_weights)) return 1;
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

int snpgpu_abi_version(void) { return SNPGPU_ABI_VERSION; }
const char *snpgpu_last_error(void) { return g_err.c_str(); }

int snpgpu_device_count(int *count)
{
    int n = 0;
    SNPGPU_HIP_CHECK(hipGetDeviceCount(&n));
    if (count) *count = n;
    return 0;
}

int snpgpu_synth_block(void *dst, int64_t n_samp, int64_t snp_begin, int64_t n_snp, uint32_t seed, double missing,
                       int spectrum, int special, int device, void *stream)
{
    if (!dst || n_samp <= 0 || n_snp < 0 || snp_begin < 0 || !(missing >= 0.0 && missing < 1.0) || spectrum < 0 || spectrum > 4) {
        set_error("snpgpu_synth_block: invalid arguments");
        return 1;
    }
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    const uint32_t miss32 = (uint32_t)std::floor(missing * 4294967296.0);
    // without a stream the block is written on the NULL stream, which does not order itself against the contexts' own
    // (non-blocking) streams: wait for whatever may still read `dst` (an earlier asynchronous snpgpu_feed of the same buffer)
    if (!stream) SNPGPU_HIP_CHECK(hipDeviceSynchronize());
    if (launch_synth_block((hipStream_t)stream, (uint8_t *)dst, n_samp, snp_begin, n_snp, seed, miss32, spectrum, special)) return 1;
    if (!stream) SNPGPU_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

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
    {
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
    }
    std::unique_ptr<snpgpu_ctx> c(new snpgpu_ctx());
    c->plan = plan;
    c->device = o.device;
    if (o.stream) {
        c->stream = (hipStream_t)o.stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_error("snpgpu_create: hipStreamCreate failed"); return 1; }
        c->own_stream = true;
    }
    if (alloc_ctx(c.get()) || zero_ctx(c.get())) {
        const std::string keep = g_err;
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
}  // namespace

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

// per-SNP statistics handed in by the caller (snpgpu_feed_stats): the block's "holds missing calls" flag from them
__global__ __launch_bounds__(256) void stats_flag_kernel(const int32_t *__restrict__ num, int64_t n_snp, int64_t N,
                                                         unsigned long long *__restrict__ d_missing)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n_snp && (int64_t)num[k] < N) *d_missing = 1ull;
}

static int feed_impl(snpgpu_ctx *c, const void *geno, int64_t n_snp, int format, int mem, const int32_t *ext_sum, const int32_t *ext_num);

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

namespace {
struct Block {             // one feed block on its way through the context
    int64_t n_snp = 0;
    const void *src = nullptr;   // device rows as the caller laid them out
    int turn = -1;         // pinned feeds: the staging buffer that holds them (-1: none)
    bool direct = false;   // IBS / KING-robust fed with 2-bit rows: the counters' pre-pass reads `src` itself, nothing is repacked
};
}  // namespace

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
    const int64_t n_pad = round_up(n_snp, 256);    // whole loop rounds of the MFMA pair kernels (4 k-steps of 64 / up to 4 of 32 SNPs)
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
        const int64_t mm_stride = round_up(p.Bmax, 256);
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
            EvScope ev(c, 1);      // (one span per table, as the timing has always counted them)
            if (i == 0 && launch_syrk_uv(st, c->syrk_panel(c->wt, 0), o)) return 1;
            continue;
        }
        EvScope ev(c, 1);
        if (!p.mm_h3) {
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
        if (launch_syrk_h3(st, c->syrk_panel(x1e ? c->wt12 : c->wt, i), h)) return 1;
        if (uv) {
            SyrkUvOpts o;
            o.work_x1 = (const int4 *)c->x1_work.p; o.n_blocks_x1 = c->x1_blocks;
            o.lut = (const uint2 *)c->uvlut.p; o.n_q = b.n_q;
            o.d_missing = c->d_missing();
            o.run_chunks = b.uv_runs > 1 ? b.uv_cpr : 0; o.n_target = b.uv_q;
            o.form = p.uv_form;
            o.pace_src = c->uvpace.p; o.pace = p.uvc_pace;
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

int snpgpu_host_alloc(size_t bytes, void **out)
{
    if (!out) { set_error("snpgpu_host_alloc: out is NULL"); return 1; }
    SNPGPU_HIP_CHECK(hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return 0;
}

int snpgpu_host_free(void *p)
{
    if (p) SNPGPU_HIP_CHECK(hipHostFree(p));
    return 0;
}

int snpgpu_host_wait(snpgpu_ctx *c, const void *host_buf)
{
    if (!c) { set_error("snpgpu_host_wait: NULL context"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    for (int k = 0; k < 2; k++)
        if (c->host_src[k] == host_buf && c->ev_copied[k]) SNPGPU_HIP_CHECK(hipEventSynchronize(c->ev_copied[k]));
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

// ---------------------------------------------------------------------------
// output staging: finalisers write device buffers; host destinations go through a temporary
namespace {

struct OutBuf {
    snpgpu_ctx *c;
    void *user;
    void *dev = nullptr;
    size_t bytes;
    int mem;
    bool temp = false;
    OutBuf(snpgpu_ctx *c_, void *user_, size_t bytes_, int mem_) : c(c_), user(user_), bytes(bytes_), mem(mem_) {}
    int prepare()
    {
        if (mem == SNPGPU_DEVICE) { dev = user; return 0; }
        SNPGPU_HIP_CHECK(hipMalloc(&dev, bytes ? bytes : 16));
        temp = true;
        return 0;
    }
    int commit()
    {
        if (temp) SNPGPU_HIP_CHECK(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    ~OutBuf()
    {
        if (temp && dev) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(dev);
        }
    }
};

int settle_colterm(snpgpu_ctx *c) { return snpgpu::ctx_settle(c); }

int check_out(snpgpu_ctx *c, int kind_a, int kind_b, int packed, const char *fn, bool settle = true)
{
    if (!c) { set_error(std::string(fn) + ": NULL context"); return 1; }
    if (c->plan.kind != kind_a && c->plan.kind != kind_b) { set_error(std::string(fn) + ": wrong context kind"); return 1; }
    if (!packed && !c->plan.full) { set_error(std::string(fn) + ": full-matrix output needs a full (non-panel) context"); return 1; }
    if (settle && settle_colterm(c)) return 1;
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

size_t out_elems(snpgpu_ctx *c, int packed) { return packed ? (size_t)snpgpu_slab_size(c) : (size_t)c->plan.N * (size_t)c->plan.N; }

int finish(snpgpu_ctx *c)
{
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_ibs_num(snpgpu_ctx *c, int32_t *ibs0, int32_t *ibs1, int32_t *ibs2, int packed, int mem)
{
    if (check_out(c, SNPGPU_IBS, SNPGPU_IBS, packed, "snpgpu_ibs_num")) return 1;
    const size_t n = out_elems(c, packed) * sizeof(int32_t);
    OutBuf b0(c, ibs0, n, mem), b1(c, ibs1, n, mem), b2(c, ibs2, n, mem);
    if (b0.prepare() || b1.prepare() || b2.prepare()) return 1;
    if (launch_fin_ibs_num(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (int32_t *)b0.dev, (int32_t *)b1.dev,
                           (int32_t *)b2.dev, packed))
        return 1;
    if (b0.commit() || b1.commit() || b2.commit()) return 1;
    return finish(c);
}

int snpgpu_ibs_ave(snpgpu_ctx *c, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_IBS, SNPGPU_IBS, packed, "snpgpu_ibs_ave")) return 1;
    OutBuf b(c, out, out_elems(c, packed) * sizeof(double), mem);
    if (b.prepare()) return 1;
    if (launch_fin_ibs_ave(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (double *)b.dev, packed)) return 1;
    if (b.commit()) return 1;
    return finish(c);
}

int snpgpu_king_robust_counts(snpgpu_ctx *c, uint32_t *out5, int mem)
{
    if (check_out(c, SNPGPU_KING_ROBUST, SNPGPU_KING_ROBUST, 1, "snpgpu_king_robust_counts")) return 1;
    OutBuf b(c, out5, out_elems(c, 1) * 5 * sizeof(uint32_t), mem);
    if (b.prepare()) return 1;
    if (launch_fin_king_counts(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (uint32_t *)b.dev)) return 1;
    if (b.commit()) return 1;
    return finish(c);
}

int snpgpu_king_robust(snpgpu_ctx *c, const int32_t *family, double *ibs0, double *kinship, int packed, int mem)
{
    if (check_out(c, SNPGPU_KING_ROBUST, SNPGPU_KING_ROBUST, packed, "snpgpu_king_robust")) return 1;
    const int32_t *dfam = nullptr;
    if (family) {
        if (!c->family.p && c->family.alloc(sizeof(int32_t) * (size_t)c->plan.N)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->family.p, family, sizeof(int32_t) * (size_t)c->plan.N, hipMemcpyHostToDevice, c->stream));
        dfam = (const int32_t *)c->family.p;
    }
    const size_t n = out_elems(c, packed) * sizeof(double);
    OutBuf b0(c, ibs0, n, mem), b1(c, kinship, n, mem);
    if (b0.prepare() || b1.prepare()) return 1;
    if (launch_fin_king_robust(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, dfam, (double *)b0.dev,
                               (double *)b1.dev, packed))
        return 1;
    if (b0.commit() || b1.commit()) return 1;
    return finish(c);
}

int snpgpu_king_homo(snpgpu_ctx *c, double *k0, double *k1, int packed, int mem)
{
    if (check_out(c, SNPGPU_KING_HOMO, SNPGPU_KING_HOMO, packed, "snpgpu_king_homo")) return 1;
    const size_t n = out_elems(c, packed) * sizeof(double);
    OutBuf b0(c, k0, n, mem), b1(c, k1, n, mem);
    if (b0.prepare() || b1.prepare()) return 1;
    // split-fp16 tables are pre-scaled by 2^H3_HOMO_SHIFT (both operands): the sums carry 2^(2 shift)
    const double fscale = c->plan.mm_h3 ? std::ldexp(1.0, -2 * H3_HOMO_SHIFT) : 1.0;
    if (launch_fin_king_homo(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (const double *)c->acc_f64.p, fscale,
                             (double *)b0.dev, (double *)b1.dev, packed, c->plan.want_het ? c->d_homo_w() : nullptr,
                             c->plan.homo_uv ? (const double *)c->homo_msum.p : nullptr,
                             c->plan.homo_uv ? (const uint32_t *)c->diss_called.p : nullptr,
                             c->plan.homo_uv ? (const uint32_t *)c->nosh.p : nullptr))
        return 1;
    if (b0.commit() || b1.commit()) return 1;
    return finish(c);
}

int snpgpu_diss(snpgpu_ctx *c, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_DISS, SNPGPU_DISS, packed, "snpgpu_diss")) return 1;
    OutBuf b(c, out, out_elems(c, packed) * sizeof(double), mem);
    if (b.prepare()) return 1;
    if (launch_fin_diss(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (const double *)c->acc_f64.p,
                        std::ldexp(1.0, -2 * H3_HOMO_SHIFT), c->d_homo_w(), (const double *)c->homo_msum.p,
                        (const uint32_t *)c->diss_called.p, (double *)b.dev, nullptr, nullptr, packed, (const uint32_t *)c->nosh.p))
        return 1;
    if (b.commit()) return 1;
    return finish(c);
}

int snpgpu_diss_sums(snpgpu_ctx *c, uint32_t *geno_sum, double *wsum, int mem)
{
    if (check_out(c, SNPGPU_DISS, SNPGPU_DISS, 1, "snpgpu_diss_sums")) return 1;
    if (!geno_sum || !wsum) { set_error("snpgpu_diss_sums: NULL output"); return 1; }
    const size_t n = out_elems(c, 1);
    OutBuf b0(c, geno_sum, n * sizeof(uint32_t), mem), b1(c, wsum, n * sizeof(double), mem);
    if (b0.prepare() || b1.prepare()) return 1;
    if (launch_fin_diss(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, (const double *)c->acc_f64.p,
                        std::ldexp(1.0, -2 * H3_HOMO_SHIFT), c->d_homo_w(), (const double *)c->homo_msum.p,
                        (const uint32_t *)c->diss_called.p, nullptr, (uint32_t *)b0.dev, (double *)b1.dev, 1, (const uint32_t *)c->nosh.p))
        return 1;
    if (b0.commit() || b1.commit()) return 1;
    return finish(c);
}

int snpgpu_grm_gcta(snpgpu_ctx *c, double *out, int packed, int mem)
{
    // the pending column / row terms of the fp16 SYRK are applied by the finaliser itself (one pass over the panel less)
    if (check_out(c, SNPGPU_GRM_GCTA, SNPGPU_GRM_GCTA, packed, "snpgpu_grm_gcta", false)) return 1;
    OutBuf b(c, out, out_elems(c, packed) * sizeof(double), mem);
    if (b.prepare()) return 1;
    if (c->frozen) {            // the panel already holds the final values (snpgpu_finalize_inplace)
        if (launch_fin_cov(c->stream, c->geom(), (const double *)c->acc_f64.p, 1.0, (double *)b.dev, packed)) return 1;
    } else if (launch_fin_gcta(c->stream, c->geom(), (const double *)c->acc_f64.p, (const uint32_t *)c->acc_u32.p,
                        (const uint32_t *)c->miss_diag.p, c->d_nlocus(), (double *)b.dev, packed,
                        c->colterm_pending ? (const double *)c->colterm.p : nullptr,
                        c->colterm_pending ? (const double *)c->uvterm.p : nullptr))
        return 1;
    if (b.commit()) return 1;
    return finish(c);
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
    OutBuf b(c, out, out_elems(c, packed) * sizeof(double), mem);
    if (b.prepare()) return 1;
    if (launch_fin_cov(c->stream, c->geom(), (const double *)c->acc_f64.p, scale, (double *)b.dev, packed)) return 1;
    if (b.commit()) return 1;
    return finish(c);
}


int snpgpu_pca_panel_trace(snpgpu_ctx *c, double *trace)
{
    if (!c || c->plan.kind != SNPGPU_PCA_COV) { set_error("snpgpu_pca_panel_trace: needs a PCA_COV context"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    if (settle_colterm(c)) return 1;
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
        if (launch_fin_gcta(c->stream, c->geom(), P, (const uint32_t *)c->acc_u32.p, (const uint32_t *)c->miss_diag.p,
                            c->d_nlocus(), P, 2, c->colterm_pending ? (const double *)c->colterm.p : nullptr,
                            c->colterm_pending ? (const double *)c->uvterm.p : nullptr))
            return 1;
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
    if (settle_colterm(c)) return 1;
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

int snpgpu_ibd_mom(snpgpu_ctx *c, const double *e, int kinship_constraint, double *k0, double *k1, int packed, int mem)
{
    if (check_out(c, SNPGPU_IBS, SNPGPU_IBS, packed, "snpgpu_ibd_mom")) return 1;
    if (!e) { set_error("snpgpu_ibd_mom: e is NULL"); return 1; }
    const size_t n = out_elems(c, packed) * sizeof(double);
    OutBuf b0(c, k0, n, mem), b1(c, k1, n, mem);
    if (b0.prepare() || b1.prepare()) return 1;
    if (launch_fin_mom(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, e, kinship_constraint, (double *)b0.dev,
                       (double *)b1.dev, packed))
        return 1;
    if (b0.commit() || b1.commit()) return 1;
    return finish(c);
}

// ---- selection of related pairs (kernels_select.hip) -------------------------------------------------------------------------------
}  // extern "C"

namespace {

thread_local double g_sel_ms[4] = {0, 0, 0, 0};    // count pass, scan, write pass (device), whole call (host clock) of the last selection

// the refusals that need neither a context nor a device; `fn`: the public name
int select_check_opts(const char *fn, const snpgpu_sel_opts *o, int64_t capacity, const void *const *outs, int n_outs)
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
    // split-fp16 tables are pre-scaled by 2^H3_HOMO_SHIFT (both operands): the sums carry 2^(2 shift) -- as snpgpu_king_homo
    const double fscale = c->plan.mm_h3 ? std::ldexp(1.0, -2 * H3_HOMO_SHIFT) : 1.0;
    return launch_select_king_homo(c->stream, c->geom(), acc, (const double *)c->acc_f64.p, fscale, c->plan.want_het ? c->d_homo_w() : nullptr,
                                   c->plan.homo_uv ? (const double *)c->homo_msum.p : nullptr,
                                   c->plan.homo_uv ? (const uint32_t *)c->diss_called.p : nullptr,
                                   c->plan.homo_uv ? (const uint32_t *)c->nosh.p : nullptr, a, write);
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
    if (o->what == SNPGPU_SEL_KING_ROBUST && o->family) {
        if (!c->family.p && c->family.alloc(sizeof(int32_t) * (size_t)c->plan.N)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(c->family.p, o->family, sizeof(int32_t) * (size_t)c->plan.N, hipMemcpyHostToDevice, c->stream));
        dfam = (const int32_t *)c->family.p;
    }
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
        OutBuf b1(c, idx1, sizeof(int32_t) * (size_t)nw, mem), b2(c, idx2, sizeof(int32_t) * (size_t)nw, mem), b3(c, v0, sizeof(double) * (size_t)nw, mem),
               b4(c, v1, sizeof(double) * (size_t)nw, mem), b5(c, kinship, sizeof(double) * (size_t)nw, mem);
        OutBuf *bs[5] = {&b1, &b2, &b3, &b4, &b5};
        if (o->what == SNPGPU_SEL_KING_ROBUST) bs[3]->user = nullptr;                // v1 is not written for this kind
        for (OutBuf *b : bs) if (b->user && b->prepare()) return 1;
        a.capacity = nw;
        a.idx1 = (int32_t *)b1.dev; a.idx2 = (int32_t *)b2.dev; a.v0 = (double *)b3.dev; a.v1 = (double *)b4.dev; a.kin = (double *)b5.dev;
        SNPGPU_HIP_CHECK(hipEventRecord(ev[2].a, c->stream));
        if (select_launch(c, o, dfam, a, true)) return 1;
        SNPGPU_HIP_CHECK(hipEventRecord(ev[2].b, c->stream));
        for (OutBuf *b : bs) if (b->user && b->commit()) return 1;
        if (finish(c)) return 1;
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

int snpgpu_eigmix(snpgpu_ctx *c, int diagadj, double scale, double *out, int packed, int mem)
{
    if (check_out(c, SNPGPU_EIGMIX, SNPGPU_EIGMIX, packed, "snpgpu_eigmix")) return 1;
    OutBuf b(c, out, out_elems(c, packed) * sizeof(double), mem);
    if (b.prepare()) return 1;
    const double *num = (const double *)c->acc_f64.p;
    if (c->frozen) {
        if ((diagadj != 0) != (c->frozen_diagadj != 0)) { set_error("snpgpu_eigmix: the context was finalised in place with another 'diagadj'"); return 1; }
        if (launch_fin_cov(c->stream, c->geom(), num, scale / c->frozen_scale, (double *)b.dev, packed)) return 1;
    } else if (launch_fin_eigmix(c->stream, c->geom(), num, num + c->plane(), (const uint32_t *)c->samp_het.p,
                          (const double *)c->samp_dmiss.p, (const double *)c->samp_dsq.p, c->d_sumden(), diagadj, scale,
                          (double *)b.dev, packed))
        return 1;
    if (b.commit()) return 1;
    return finish(c);
}

int snpgpu_indiv_beta(snpgpu_ctx *c, int mode, double *out, double *avg_val, int packed, int mem)
{
    if (check_out(c, SNPGPU_INDIV_BETA, SNPGPU_INDIV_BETA, packed, "snpgpu_indiv_beta")) return 1;
    if (!c->plan.full) { set_error("snpgpu_indiv_beta: needs a full (non-panel) context"); return 1; }
    if (mode < 0 || mode > 2) { set_error("snpgpu_indiv_beta: invalid mode"); return 1; }
    const int nb = 1024;
    DevBuf part;
    if (part.alloc(sizeof(double) * 2 * nb)) return 1;
    std::vector<double> h(2 * nb);
    int rc = launch_beta_reduce(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, mode != 0, (double *)part.p,
                                (double *)part.p + nb, nb);
    if (!rc && hipMemcpyAsync(h.data(), part.p, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = 1;
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = 1;
    part.release();
    if (rc) { set_error("snpgpu_indiv_beta: reduction failed"); return 1; }
    double mn = h[0], sum = 0;
    for (int i = 0; i < nb; i++) { if (h[i] < mn) mn = h[i]; sum += h[nb + i]; }
    const double avg = sum / (double)(c->plan.N * (c->plan.N - 1) / 2);
    if (avg_val) *avg_val = avg;
    if (!out) return 0;
    OutBuf b(c, out, out_elems(c, packed) * sizeof(double), mem);
    if (b.prepare()) return 1;
    if (launch_fin_beta(c->stream, c->geom(), (const uint32_t *)c->acc_u32.p, mode, avg, mn, (double *)b.dev, packed)) return 1;
    if (b.commit()) return 1;
    return finish(c);
}

}  // extern "C"
