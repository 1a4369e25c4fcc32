// C ABI of libsnpgpu, LD pruning (include/snpgpu.h section 1d): snpgpu_ld_prune, Perform_LD_Pruning (src/genLD.cpp:807-924)
// on one chromosome.  Kernels: kernels_ld.hip (staging, band tables, threshold bits).
//
// Why a data-parallel form is exact.  The reference keeps a list of kept SNPs; at candidate i an entry j is ERASED for good when
// |i - j| > slide_max_n or |pos[i] - pos[j]| > slide_max_bp, and every other entry is tested with |LD(j, i)| > threshold.  Erasure
// never looks at LD, so whether a kept j is still listed at candidate i is fixed by the positions: in the forward pass j is
// listed at i iff the window holds at every candidate j + 1 ... i, in the backward pass iff it holds at every candidate from the
// one after j's insertion (j - 1, or start - 1 for the pass's initial list) down to i.  W, the largest distance |i - j| that can
// be listed, therefore bounds every pair the scan can test, whatever it keeps (prune_width).  The decisions only read
// "|LD| > threshold" of such pairs: one bit per pair of the band (x, x + k), k = 1 ... W, computed on the device and scanned on
// the host with the reference's list rules.
//
// Device side, per call (nothing is sized by the whole chromosome but the caller's input): two row buffers of cap = blk + W
// staging rows used in turn (a full buffer finalises the rows whose W partners are all resident; its last W rows move to the
// other buffer as the halo of the next block, as in ld.hip's sliding window), band tables [P][W][9] with P * W * 36 bytes within
// PRUNE_TABLE_BUDGET, and the bit rows [P][ceil(W / 64)] copied to the host after each launch.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "host_util.h"

using namespace snpgpu;

namespace {

inline int64_t pr_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
constexpr size_t PRUNE_TABLE_BUDGET = size_t(1) << 30;   // bytes of band tables per launch
constexpr int64_t PRUNE_BLOCK_DEFAULT = 16384;          // rows per streamed block

// the reference's window test: kept SNP j is still listed at candidate i (position differences exact in 64 bits)
inline bool in_window(int64_t i, int64_t j, const int32_t *pos, int32_t max_bp, int32_t max_n)
{
    const int64_t d = i > j ? i - j : j - i;
    const int64_t p = (int64_t)pos[i] - (int64_t)pos[j];
    return d <= max_n && (p < 0 ? -p : p) <= max_bp;
}

// W: the largest |i - j| of a (kept j, candidate i) pair the scan can reach.  Every walk stops at its first miss; a walk that
// cannot beat the W found so far is skipped, so a window spanning the chromosome costs O(M) checks.
int64_t prune_width(int64_t M, int64_t start, const int32_t *pos, int32_t max_bp, int32_t max_n)
{
    if (M <= 1 || max_n <= 0 || max_bp < 0) return 0;
    int64_t W = 0;
    const int64_t cap = std::min<int64_t>(M - 1, max_n);
    // backward pass, initial list: any j >= start inside the window of start may be in it (the list stops at the first kept SNP
    // outside); such a j stays listed at start - 1, start - 2, ... until the first miss
    for (int64_t j = M - 1; j >= start && j > W && W < cap; j--) {
        if (!in_window(j, start, pos, max_bp, max_n)) continue;
        int64_t i = start - 1;
        while (i >= 0 && in_window(i, j, pos, max_bp, max_n)) i--;
        if (i + 1 < start) W = std::max(W, j - (i + 1));
    }
    // forward pass: kept j >= start is listed at j + 1, j + 2, ... until the first miss
    for (int64_t j = start; j < M - 1 && M - 1 - j > W && W < cap; j++) {
        int64_t i = j + 1;
        while (i < M && in_window(i, j, pos, max_bp, max_n)) i++;
        W = std::max(W, i - 1 - j);
    }
    // backward pass, SNPs kept below start: listed at j - 1, j - 2, ... until the first miss
    for (int64_t j = start - 1; j > W && W < cap; j--) {
        int64_t i = j - 1;
        while (i >= 0 && in_window(i, j, pos, max_bp, max_n)) i--;
        W = std::max(W, j - (i + 1));
    }
    return W;
}

// Perform_LD_Pruning's two passes over the bits (row x, word (k - 1) / 64, bit (k - 1) % 64 of pair (x, x + k)).  The list
// order of the reference (push_front in the backward pass) decides only which test fires first, not whether one does.
int prune_scan(int64_t M, int64_t start, const int32_t *pos, int32_t max_bp, int32_t max_n, const std::vector<uint64_t> &bits,
               int64_t W, uint8_t *keep)
{
    const int64_t wpr = (W + 63) / 64;
    bool outside = false;
    auto fires = [&](int64_t x, int64_t y) {          // x < y
        const int64_t k = y - x;
        if (k < 1 || k > W) { outside = true; return false; }
        return ((bits[(size_t)(x * wpr + (k - 1) / 64)] >> ((k - 1) & 63)) & 1) != 0;
    };
    std::vector<int64_t> list;
    auto step = [&](int64_t i) {
        bool inc = true;
        size_t o = 0;
        for (size_t e = 0; e < list.size(); e++) {
            const int64_t j = list[e];
            if (!in_window(i, j, pos, max_bp, max_n)) continue;          // erased
            if (inc && (j < i ? fires(j, i) : fires(i, j))) inc = false;
            list[o++] = j;
        }
        list.resize(o);
        keep[i] = inc ? 1 : 0;
        if (inc) list.push_back(i);
    };
    std::memset(keep, 0, (size_t)M);
    keep[start] = 1;
    list.push_back(start);
    for (int64_t i = start + 1; i < M; i++) step(i);
    list.clear();
    for (int64_t i = start; i < M; i++) {
        if (!keep[i]) continue;
        if (!in_window(i, start, pos, max_bp, max_n)) break;
        list.push_back(i);
    }
    for (int64_t i = start - 1; i >= 0; i--) step(i);
    if (outside) { set_error("snpgpu_ld_prune: internal error: a tested pair lies outside the band"); return 1; }
    return 0;
}

// 64 x 64 tiles a band launch computes (ld_count_kernel<true>'s exit rule)
int64_t band_tiles(int64_t n_i, int64_t n_b, int64_t W)
{
    int64_t t = 0;
    for (int64_t x = 0; x < (n_i + 63) / 64; x++)
        for (int64_t y = 0; y <= (63 + W) / 64; y++)
            if (64 * y - 63 <= W && 64 * x + 64 * y < n_b) t++;
    return t;
}

int check_args(const char *fn, const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int64_t start_idx, int method)
{
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, LD_GENO)) return 1;
    if (start_idx < 0 || start_idx >= n_snp) return fail(fn, "invalid start index (0 ... n_snp - 1)");
    if (method < SNPGPU_LD_COMPOSITE || method > SNPGPU_LD_CORR) return fail(fn, "invalid LD method (1 ... 4: composite, r, dprime, corr)");
    return 0;
}

// The threshold bits of the band of width W: host bits [M][ceil(W / 64)]
int prune_bits(const char *fn, const uint8_t *geno, int64_t M, int64_t N, int format, int mem, int64_t start, int64_t W,
               double threshold, int method, std::vector<uint64_t> &bits, const snpgpu_opts *opts, snpgpu_ld_prune_info *info)
{
    snpgpu_opts o{};
    if (opts) o = *opts;
    Call c;
    if (c.open(fn, o.device, info != nullptr, o.stream)) return 1;
    hipStream_t s = c.st.s;
    EventLog &tm = c.log;
    const int64_t wpr = (W + 63) / 64;
    try { bits.assign((size_t)(M * wpr), 0); }
    catch (...) { return fail(fn, "host allocation of the bit rows failed"); }
    if (W == 0) return 0;
    if (W > 0x3fffffffLL) return fail(fn, "invalid band width");

    const int64_t rbp = pr_up((N + 3) / 4, 32);
    const int64_t irb = format == SNPGPU_GENO_U8 ? N : (N + 3) / 4;
    const int64_t blk = o.max_block_snps > 0 ? o.max_block_snps : PRUNE_BLOCK_DEFAULT;
    const int64_t cap = std::min(M, blk + W);
    const int64_t P = std::max<int64_t>(64, std::min(pr_up(blk, 64), (int64_t)(PRUNE_TABLE_BUDGET / ((size_t)W * 36)) / 64 * 64));
    // the table kernel reads whole 64-row tiles, up to 63 rows past the resident ones: one spare tile
    const size_t rbytes = (size_t)(pr_up(cap, 64) + 64) * (size_t)rbp;
    int rc = 0;
    DevBuf *rows[2] = {c.bufs.get(rbytes, rc), cap < M ? c.bufs.get(rbytes, rc) : nullptr};
    DevBuf *tab = c.bufs.get((size_t)(P * W * 36), rc), *dbits = c.bufs.get((size_t)(P * wpr * 8), rc), *raw = c.bufs.get(0, rc);
    if (rc) return fail(fn, "device allocation failed");
    // rows past the data only meet pairs the kernel never writes; a defined content all the same, for the spare tile only
    for (DevBuf *r : rows)
        if (r) SNPGPU_HIP_CHECK(hipMemsetAsync((uint8_t *)r->p + (size_t)cap * rbp, 0xFF, r->bytes - (size_t)cap * rbp, s));

    enum { ST = 0, TAB = 1, BITS = 2, CPY = 3 };
    int64_t n_fed = 0, base = 0, n_res = 0, done = 0, launches = 0, tiles = 0;
    int cur = 0;
    while (n_fed < M) {
        const int64_t m = std::min(M - n_fed, cap - n_res);
        if (tm.begin(ST, s) || stage_ld_rows(s, *raw, geno + n_fed * irb, m, N, rbp, format, mem, (uint8_t *)rows[cur]->p + n_res * rbp) ||
            tm.end(s))
            return 1;
        n_res += m; n_fed += m;
        const bool last = n_fed == M;
        const int64_t i_end = last ? M : base + n_res - W;
        const uint8_t *res = (const uint8_t *)rows[cur]->p;
        for (int64_t i0 = done; i0 < i_end; i0 += P) {
            const int64_t n_i = std::min(P, i_end - i0);
            if (tm.begin(TAB, s) || launch_ld_count_band(s, res, (int)(i0 - base), (int)n_i, (int)n_res, (int)W, rbp, (int32_t *)tab->p) ||
                tm.end(s))
                return 1;
            if (tm.begin(BITS, s) ||
                launch_ld_prune_bits(s, (const int32_t *)tab->p, n_i, (int)W, i0, M, start, method, threshold, (uint64_t *)dbits->p) ||
                tm.end(s))
                return 1;
            if (tm.begin(CPY, s)) return 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(bits.data() + i0 * wpr, dbits->p, (size_t)(n_i * wpr) * 8, hipMemcpyDeviceToHost, s));
            if (tm.end(s)) return 1;
            launches++;
            tiles += band_tiles(n_i, n_res - (i0 - base), W);
        }
        done = i_end;
        if (!last) {
            const int nxt = cur ^ 1;
            if (tm.begin(ST, s)) return 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(rows[nxt]->p, res + (i_end - base) * rbp, (size_t)(W * rbp), hipMemcpyDeviceToDevice, s));
            if (tm.end(s)) return 1;
            cur = nxt; base = i_end; n_res = W;
        }
    }
    if (hipStreamSynchronize(s) != hipSuccess) return fail(fn, "kernel failed");
    if (info) {
        if (tm.sum_ms(ST, &info->ms_stage) || tm.sum_ms(TAB, &info->ms_tables) || tm.sum_ms(BITS, &info->ms_bits) ||
            tm.sum_ms(CPY, &info->ms_copy))
            return 1;
        info->table_launches = launches;
        info->table_tiles = tiles;
    }
    return 0;
}

void info_reset(snpgpu_ld_prune_info *info, int64_t M, int64_t W)
{
    if (!info) return;
    std::memset(info, 0, sizeof(*info));
    info->width = W;
    info->band_pairs = W * (M - W) + W * (W - 1) / 2;     // sum over x of min(W, M - 1 - x), W <= M - 1
}

}  // namespace

extern "C" {

int snpgpu_ld_prune(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int64_t start_idx, const int32_t *pos_bp,
                    int32_t slide_max_bp, int32_t slide_max_n, double ld_threshold, int method, uint8_t *keep,
                    const snpgpu_opts *opts, snpgpu_ld_prune_info *info)
{
    if (check_args("snpgpu_ld_prune", geno, n_snp, n_samp, format, mem, start_idx, method)) return 1;
    if (!pos_bp || !keep) { set_error("snpgpu_ld_prune: NULL argument"); return 1; }
    auto t0 = std::chrono::steady_clock::now();
    const int64_t W = prune_width(n_snp, start_idx, pos_bp, slide_max_bp, slide_max_n);
    double ms_width = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    info_reset(info, n_snp, W);
    std::vector<uint64_t> bits;
    if (prune_bits("snpgpu_ld_prune", (const uint8_t *)geno, n_snp, n_samp, format, mem, start_idx, W, ld_threshold, method, bits, opts,
                   info))
        return 1;
    t0 = std::chrono::steady_clock::now();
    if (prune_scan(n_snp, start_idx, pos_bp, slide_max_bp, slide_max_n, bits, W, keep)) return 1;
    if (info) {
        info->ms_scan = ms_width + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        int64_t k = 0;
        for (int64_t i = 0; i < n_snp; i++) k += keep[i];
        info->n_kept = k;
    }
    return 0;
}

int snpgpu_ld_prune_bits(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int64_t start_idx, int64_t width,
                         double ld_threshold, int method, uint64_t *bits, const snpgpu_opts *opts, snpgpu_ld_prune_info *info)
{
    if (check_args("snpgpu_ld_prune_bits", geno, n_snp, n_samp, format, mem, start_idx, method)) return 1;
    if (!bits) { set_error("snpgpu_ld_prune_bits: NULL argument"); return 1; }
    if (width < 0 || width > n_snp - 1) { set_error("snpgpu_ld_prune_bits: invalid band width (0 ... n_snp - 1)"); return 1; }
    info_reset(info, n_snp, width);
    std::vector<uint64_t> v;
    if (prune_bits("snpgpu_ld_prune_bits", (const uint8_t *)geno, n_snp, n_samp, format, mem, start_idx, width, ld_threshold, method, v,
                   opts, info))
        return 1;
    if (!v.empty()) std::memcpy(bits, v.data(), v.size() * 8);
    return 0;
}

}  // extern "C"
