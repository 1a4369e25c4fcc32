// C ABI of libsnpgpu, LD scores (include/snpgpu.h section 1d): snpgpu_ld_score, score[i] = sum over the window partners j of i
// of the squared LD value of the pair, on one chromosome.  Kernels: kernels_ld.hip (staging, band tables) and
// kernels_ld_score.hip (terms, ordered fold).
//
// Host side: the window [lo[i], hi[i]] of every SNP from the sorted positions by two two-pointer passes, W = max (hi[i] - i),
// and the streamed band tables of ld_band.h with the two LD-score kernels after every table launch.  The device keeps the running
// sums, the valid counts and lo / hi for the whole chromosome (20 bytes per SNP) beside the streamer's buffers and the terms of
// one launch (8 bytes per pair beside the 36 of its table); the host gets n_snp doubles and n_snp counts at the end.
#include <cstring>
#include <vector>

#include "ld_band.h"

using namespace snpgpu;

namespace {

// lo[i] / hi[i]: first / last partner of i (i itself where it has none on that side); returns W.  With non-decreasing positions
// the partners of i are contiguous and lo / hi are non-decreasing, so each pass moves its second pointer forward only.
int64_t score_windows(int64_t M, const int32_t *pos, int32_t max_bp, int32_t max_n, std::vector<int32_t> &lo, std::vector<int32_t> &hi)
{
    lo.resize((size_t)M);
    hi.resize((size_t)M);
    const bool none = max_n <= 0 || max_bp < 0;
    int64_t W = 0, h = 0, l = 0;
    for (int64_t i = 0; i < M; i++) {
        h = std::max(h, i);
        while (!none && h + 1 < M && in_window(i, h + 1, pos, max_bp, max_n)) h++;
        if (none) h = i;
        hi[(size_t)i] = (int32_t)h;
        W = std::max(W, h - i);
        while (l < i && (none || !in_window(l, i, pos, max_bp, max_n))) l++;
        lo[(size_t)i] = (int32_t)l;
    }
    return W;
}

}  // namespace

extern "C" {

int snpgpu_ld_score(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pos_bp, int32_t slide_max_bp,
                    int32_t slide_max_n, int method, int flags, double *score, int32_t *n_valid, int32_t *n_window,
                    const snpgpu_opts *opts, snpgpu_ld_score_info *info)
{
    const char *fn = "snpgpu_ld_score";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, LD_GENO)) return 1;
    if (!score) return fail(fn, "NULL argument: score is NULL");
    if (method < SNPGPU_LD_COMPOSITE || method > SNPGPU_LD_CORR) return fail(fn, "invalid LD method (1 ... 4: composite, r, dprime, corr)");
    if (flags & ~(SNPGPU_LDSCORE_ADJUST | SNPGPU_LDSCORE_SELF)) return fail(fn, "invalid flags: unknown flag bits");
    const int64_t M = n_snp;
    if (pos_bp)
        for (int64_t i = 1; i < M; i++)
            if (pos_bp[i] < pos_bp[i - 1]) return fail(fn, "invalid positions: pos_bp decreases (SNPs must be sorted by position)");
    const int adjust = (flags & SNPGPU_LDSCORE_ADJUST) != 0;
    const double self = (flags & SNPGPU_LDSCORE_SELF) ? 1.0 : 0.0;

    std::vector<int32_t> lo, hi;
    int64_t W = 0;
    try { W = score_windows(M, pos_bp, slide_max_bp, slide_max_n, lo, hi); }
    catch (...) { return fail(fn, "host allocation of the windows failed"); }
    int64_t window_pairs = 0;
    for (int64_t i = 0; i < M; i++) window_pairs += hi[(size_t)i] - i;
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->width = W;
        info->band_pairs = W * (M - W) + W * (W - 1) / 2;     // sum over x of min(W, M - 1 - x), W <= M - 1
        info->window_pairs = window_pairs;
    }
    if (n_window)
        for (int64_t i = 0; i < M; i++) n_window[i] = hi[(size_t)i] - lo[(size_t)i];

    snpgpu_opts o{};
    if (opts) o = *opts;
    Call c;
    if (c.open(fn, o.device, info != nullptr, o.stream)) return 1;
    if (W == 0) {                                             // no pair anywhere: the self term alone
        for (int64_t i = 0; i < M; i++) score[i] = self;
        if (n_valid) std::memset(n_valid, 0, (size_t)M * sizeof(int32_t));
        return 0;
    }
    hipStream_t s = c.st.s;
    EventLog &tm = c.log;
    BandStream band;
    int rc = 0;
    band.open(c.bufs, geno, M, n_samp, format, mem, W, o.max_block_snps, rc);
    DevBuf *vals = c.bufs.get((size_t)(band.P * W) * 8, rc), *acc = c.bufs.get((size_t)M * 8, rc), *nv = c.bufs.get((size_t)M * 4, rc);
    DevBuf *dlo = c.bufs.get((size_t)M * 4, rc), *dhi = c.bufs.get((size_t)M * 4, rc), *cnt = c.bufs.get(LD_SCORE_COUNT_SLOTS * 8, rc);
    if (rc) return fail(fn, "device allocation failed");

    enum { ST = 0, TAB = 1, VAL = 2, FOLD = 3, CPY = 4 };
    if (tm.begin(ST, s)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dlo->p, lo.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dhi->p, hi.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemsetAsync(cnt->p, 0, LD_SCORE_COUNT_SLOTS * 8, s));
    if (launch_ld_score_init(s, (double *)acc->p, (int32_t *)nv->p, M, self) || tm.end(s)) return 1;
    if (band.run(c, ST, TAB, [&](const int32_t *tab, int64_t i0, int64_t n_i) -> int {
            if (tm.begin(VAL, s) ||
                launch_ld_score_terms(s, tab, n_i, (int)W, i0, (const int32_t *)dhi->p, method, adjust, (double *)vals->p, (uint64_t *)cnt->p) ||
                tm.end(s))
                return 1;
            if (tm.begin(FOLD, s) ||
                launch_ld_score_fold(s, (const double *)vals->p, n_i, (int)W, i0, M, (const int32_t *)dlo->p, (const int32_t *)dhi->p,
                                     (double *)acc->p, (int32_t *)nv->p))
                return 1;
            return tm.end(s);
        }))
        return 1;
    uint64_t valid_slots[LD_SCORE_COUNT_SLOTS] = {0};
    if (tm.begin(CPY, s)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(score, acc->p, (size_t)M * 8, hipMemcpyDeviceToHost, s));
    if (n_valid) SNPGPU_HIP_CHECK(hipMemcpyAsync(n_valid, nv->p, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(valid_slots, cnt->p, sizeof(valid_slots), hipMemcpyDeviceToHost, s));
    if (tm.end(s)) return 1;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(fn, "kernel failed");
    if (info) {
        if (tm.sum_ms(ST, &info->ms_stage) || tm.sum_ms(TAB, &info->ms_tables) || tm.sum_ms(VAL, &info->ms_values) ||
            tm.sum_ms(FOLD, &info->ms_fold) || tm.sum_ms(CPY, &info->ms_copy))
            return 1;
        for (uint64_t v : valid_slots) info->valid_pairs += (int64_t)v;
        info->table_launches = band.launches;
        info->table_tiles = band.tiles;
    }
    return 0;
}

}  // extern "C"
