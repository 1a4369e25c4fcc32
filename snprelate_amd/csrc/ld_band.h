// The streamed band tables of one chromosome, shared by snpgpu_ld_prune (ld_prune.hip) and snpgpu_ld_score (ld_score.hip): the
// 3 x 3 genotype tables of every pair (x, x + k), k = 1 ... W, in launches of at most P rows, with nothing sized by the whole
// chromosome but the caller's input.  Two row buffers of cap = blk + W staging rows are used in turn: a full buffer finalises the
// rows whose W partners are all resident, and its last W rows move to the other buffer as the halo of the next block (as in
// ld.hip's sliding window).  The tables [P][W][9] take P * W * 36 bytes within BAND_TABLE_BUDGET.  What a caller does with the
// tables of a launch (threshold bits, LD-score terms) is its `fin`, run on the same stream right after the table kernel.
#pragma once
#include <algorithm>

#include "host_util.h"

namespace snpgpu {

constexpr size_t BAND_TABLE_BUDGET = size_t(1) << 30;   // bytes of band tables per launch
constexpr int64_t BAND_BLOCK_DEFAULT = 16384;           // rows per streamed block

inline int64_t band_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// The window test of the reference's pruning scan, also the LD scores': |i - j| <= max_n and |pos[i] - pos[j]| <= max_bp, position
// differences exact in 64 bits; pos == nullptr: the SNP count alone decides.
inline bool in_window(int64_t i, int64_t j, const int32_t *pos, int32_t max_bp, int32_t max_n)
{
    const int64_t d = i > j ? i - j : j - i;
    if (d > max_n) return false;
    if (!pos) return true;
    const int64_t p = (int64_t)pos[i] - (int64_t)pos[j];
    return (p < 0 ? -p : p) <= max_bp;
}

// 64 x 64 tiles a band launch computes (ld_count_kernel<true>'s exit rule)
inline int64_t band_tiles(int64_t n_i, int64_t n_b, int64_t W)
{
    int64_t t = 0;
    for (int64_t x = 0; x < (n_i + 63) / 64; x++)
        for (int64_t y = 0; y <= (63 + W) / 64; y++)
            if (64 * y - 63 <= W && 64 * x + 64 * y < n_b) t++;
    return t;
}

struct BandStream {
    const uint8_t *geno = nullptr;
    int64_t M = 0, N = 0, W = 0, rbp = 0, irb = 0, cap = 0, P = 0;
    int format = 0, mem = 0;
    DevBuf *rows[2] = {nullptr, nullptr}, *tab = nullptr, *raw = nullptr;
    int64_t launches = 0, tiles = 0;

    // Sizes and device buffers for a band of width W in [1, 2^30); rc is the arena's (DevArena::get): test it after the caller's
    // own allocations.
    void open(DevArena &bufs, const void *geno_, int64_t M_, int64_t N_, int format_, int mem_, int64_t W_, int64_t max_block_snps,
              int &rc)
    {
        geno = (const uint8_t *)geno_; M = M_; N = N_; W = W_; format = format_; mem = mem_;
        rbp = band_up((N + 3) / 4, 32);
        irb = format == SNPGPU_GENO_U8 ? N : (N + 3) / 4;
        const int64_t blk = max_block_snps > 0 ? max_block_snps : BAND_BLOCK_DEFAULT;
        cap = std::min(M, blk + W);
        P = std::max<int64_t>(64, std::min(band_up(blk, 64), (int64_t)(BAND_TABLE_BUDGET / ((size_t)W * 36)) / 64 * 64));
        // the table kernel reads whole 64-row tiles, up to 63 rows past the resident ones: one spare tile
        const size_t rbytes = (size_t)(band_up(cap, 64) + 64) * (size_t)rbp;
        rows[0] = bufs.get(rbytes, rc);
        rows[1] = cap < M ? bufs.get(rbytes, rc) : nullptr;
        tab = bufs.get((size_t)(P * W * 36), rc);
        raw = bufs.get(0, rc);
    }

    // fin(tab, i0, n_i): the tables [n_i][W][9] of rows i0 ... i0 + n_i - 1 (chromosome indices) are on the stream; launches come
    // in ascending i0 and cover every row once.  ph_stage / ph_tables: the EventLog phases of staging and of the table kernel.
    template <class F> int run(Call &c, int ph_stage, int ph_tables, F &&fin)
    {
        hipStream_t s = c.st.s;
        EventLog &tm = c.log;
        // rows past the data only meet pairs the kernel never writes; a defined content all the same, for the spare tile only
        for (DevBuf *r : rows)
            if (r) SNPGPU_HIP_CHECK(hipMemsetAsync((uint8_t *)r->p + (size_t)cap * rbp, 0xFF, r->bytes - (size_t)cap * rbp, s));
        int64_t n_fed = 0, base = 0, n_res = 0, done = 0;
        int cur = 0;
        while (n_fed < M) {
            const int64_t m = std::min(M - n_fed, cap - n_res);
            if (tm.begin(ph_stage, s) ||
                stage_ld_rows(s, *raw, geno + n_fed * irb, m, N, rbp, format, mem, (uint8_t *)rows[cur]->p + n_res * rbp) || tm.end(s))
                return 1;
            n_res += m; n_fed += m;
            const bool last = n_fed == M;
            const int64_t i_end = last ? M : base + n_res - W;
            const uint8_t *res = (const uint8_t *)rows[cur]->p;
            for (int64_t i0 = done; i0 < i_end; i0 += P) {
                const int64_t n_i = std::min(P, i_end - i0);
                if (tm.begin(ph_tables, s) ||
                    launch_ld_count_band(s, res, (int)(i0 - base), (int)n_i, (int)n_res, (int)W, rbp, (int32_t *)tab->p) || tm.end(s))
                    return 1;
                if (fin((const int32_t *)tab->p, i0, n_i)) return 1;
                launches++;
                tiles += band_tiles(n_i, n_res - (i0 - base), W);
            }
            done = i_end;
            if (!last) {
                const int nxt = cur ^ 1;
                if (tm.begin(ph_stage, s)) return 1;
                SNPGPU_HIP_CHECK(hipMemcpyAsync(rows[nxt]->p, res + (i_end - base) * rbp, (size_t)(W * rbp), hipMemcpyDeviceToDevice, s));
                if (tm.end(s)) return 1;
                cur = nxt; base = i_end; n_res = W;
            }
        }
        return 0;
    }
};

}  // namespace snpgpu
