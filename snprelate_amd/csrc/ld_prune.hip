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
// Device side, per call: the streamed band tables of ld_band.h (two row buffers of blk + W staging rows used in turn, tables
// [P][W][9] within a fixed byte budget), and the bit rows [P][ceil(W / 64)] copied to the host after each launch.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "ld_band.h"

using namespace snpgpu;

namespace {

// W: the largest |i - j| of a (kept j, candidate i) pair the scan can reach (in_window, ld_band.h: kept SNP j is still listed at
// candidate i).  Every walk stops at its first miss; a walk that cannot beat the W found so far is skipped, so a window spanning
// the chromosome costs O(M) checks.
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

    BandStream band;
    int rc = 0;
    band.open(c.bufs, geno, M, N, format, mem, W, o.max_block_snps, rc);
    DevBuf *dbits = c.bufs.get((size_t)(band.P * wpr * 8), rc);
    if (rc) return fail(fn, "device allocation failed");

    enum { ST = 0, TAB = 1, BITS = 2, CPY = 3 };
    if (band.run(c, ST, TAB, [&](const int32_t *tab, int64_t i0, int64_t n_i) -> int {
            if (tm.begin(BITS, s) || launch_ld_prune_bits(s, tab, n_i, (int)W, i0, M, start, method, threshold, (uint64_t *)dbits->p) ||
                tm.end(s))
                return 1;
            if (tm.begin(CPY, s)) return 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(bits.data() + i0 * wpr, dbits->p, (size_t)(n_i * wpr) * 8, hipMemcpyDeviceToHost, s));
            return tm.end(s);
        }))
        return 1;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(fn, "kernel failed");
    if (info) {
        if (tm.sum_ms(ST, &info->ms_stage) || tm.sum_ms(TAB, &info->ms_tables) || tm.sum_ms(BITS, &info->ms_bits) ||
            tm.sum_ms(CPY, &info->ms_copy))
            return 1;
        info->table_launches = band.launches;
        info->table_tiles = band.tiles;
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
