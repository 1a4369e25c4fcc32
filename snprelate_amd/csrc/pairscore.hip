// C ABI of libsnpgpu, genotype scores of listed sample pairs (include/snpgpu.h section 1i): gnrPairScore (src/genIBS.cpp:690-891).
// Kernels: kernels_pairscore.hip.
//
// The device counts, the host scores.  One pass over the 2-bit rows gives, per SNP, the 4 x 4 table of the listed pairs' codes and
// the allele flip, and per pair the 3 x 3 table of the SNPs' codes after the flip; neither depends on the method or on `dosage`.
// snpgpu_pair_score_final (no device) applies the 4 x 4 score map to a table and CalcAvgSD (src/dGenGWAS.cpp:2365-2379) to the
// integer Sum, SqSum and Num in the reference's fp64 operations, so the results equal its sequential double sums bit for bit.
// The genotypes are read block by block as the QC calls read them (host_util.h: RowBlocks).  All argument errors are found before
// any device is touched.
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_util.h"

// the fp64 expressions of the finaliser are the reference's and must stay separate operations
#pragma clang fp contract(off)

namespace snpgpu {
int launch_pair_snp_table(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, const int32_t *idx1, const int32_t *idx2,
                          int64_t n_pair, int32_t *snp_tab, uint8_t *flip);
int launch_pair_flip_words(hipStream_t st, const uint8_t *flip, int64_t n_snp, uint32_t *fw);
int launch_pair_words(hipStream_t st, const uint8_t *rows, int64_t rb, int64_t n_snp, const int32_t *idx, int64_t n_pair, uint32_t *words);
int launch_pair_count(hipStream_t st, const uint32_t *words, const uint32_t *fw, int64_t n_snp, int64_t n_pair, unsigned long long *tab);
int launch_pair_matrix(hipStream_t st, const uint8_t *geno, int64_t rb, int64_t n_snp, const int32_t *idx1, const int32_t *idx2,
                       int64_t n_pair, const uint8_t *flip, uint32_t map2, int elem_size, void *out);
}  // namespace snpgpu

using namespace snpgpu;

namespace {

// SNP-table ms, its launches, genotype bytes it read, word-transposition ms, pair-counter ms, matrix ms, launches of those three,
// genotype bytes the transposition and the matrix kernel read
thread_local double g_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

constexpr size_t PS_STAGE_BYTES = size_t(256) << 20;     // genotype bytes per streamed block
constexpr int64_t PS_MAX_BLOCK_SNPS = 65535 * 16;         // 65 535 words of 16 SNPs: grid.y of the transposition
constexpr size_t PS_WORDS_BYTES = size_t(1) << 30;        // sample-major words of one block, both lists
constexpr size_t PS_MATRIX_BYTES = size_t(256) << 20;     // score matrix of one block on the device
constexpr int64_t PS_MAX_PAIRS = int64_t(1) << 30;        // 2 n_pair called genotypes per SNP stay in int32

constexpr GenoLimits PS_GENO = {1, int64_t(1) << 31, int64_t(1) << 31, false, "invalid number of samples (1 ... 2^31 - 1)"};
enum { T_SNP = 0, T_WORDS = 1, T_COUNT = 2, T_MATRIX = 3 };

// map[g1][g2] of gnrPairScore (src/genIBS.cpp:717-736) as cell 4 g1 + g2; -1 where a genotype is missing and, in the two *.only
// maps, at some cells where both are called: there -1 is a score (the reference scores whatever g1 < 3 && g2 < 3 selects)
constexpr int M = -1;
const int8_t PS_MAPS[10][16] = {
    {2, 1, 0, M, 1, 2, 1, M, 0, 1, 2, M, M, M, M, M},     // IBS
    {1, 1, 0, M, 1, 1, 1, M, 0, 1, 1, M, M, M, M, M},     // IBS, dosage = FALSE
    {0, 0, 2, M, 1, 0, 1, M, 2, 0, 0, M, M, M, M, M},     // GVH
    {0, 0, 1, M, 1, 0, 1, M, 1, 0, 0, M, M, M, M, M},     // GVH, dosage = FALSE
    {0, 1, 2, M, 0, 0, 0, M, 2, 1, 0, M, M, M, M, M},     // HVG
    {0, 1, 1, M, 0, 0, 0, M, 1, 1, 0, M, M, M, M, M},     // HVG, dosage = FALSE
    {0, 0, 0, M, 1, 0, 0, M, 1, 0, 0, M, M, M, M, M},     // GVH.major
    {0, 0, 1, M, 0, 0, 1, M, 0, 0, 0, M, M, M, M, M},     // GVH.minor
    {0, 0, M, M, 1, 0, M, M, 1, 0, 0, M, M, M, M, M},     // GVH.major.only
    {0, 0, 1, M, M, 0, 1, M, M, 0, 0, M, M, M, M, M},     // GVH.minor.only
};

bool ps_need_major(int method) { return method >= SNPGPU_PS_GVH_MAJOR; }

const int8_t *ps_map(int method, int dosage)
{
    if (method < SNPGPU_PS_IBS || method > SNPGPU_PS_GVH_MINOR_ONLY) return nullptr;
    if (method <= SNPGPU_PS_HVG) return PS_MAPS[2 * (method - 1) + (dosage ? 0 : 1)];
    return PS_MAPS[6 + method - SNPGPU_PS_GVH_MAJOR];
}

int check_pairs(const char *fn, const int32_t *idx1, const int32_t *idx2, int64_t n_pair, int64_t n_samp)
{
    if (!idx1 || !idx2) return fail(fn, "NULL argument: idx1 / idx2 is NULL");
    if (n_pair < 1) return fail(fn, "invalid number of pairs: no pair is given");
    if (n_pair >= PS_MAX_PAIRS) return fail(fn, "invalid number of pairs: too many pairs (< 2^30)");
    for (int64_t p = 0; p < n_pair; p++)
        if (idx1[p] < 0 || idx1[p] >= n_samp || idx2[p] < 0 || idx2[p] >= n_samp)
            return fail(fn, "sample index out of range at pair " + std::to_string(p));
    return 0;
}

// both lists in device memory, the first and then the second
int upload_pairs(Call &c, const int32_t *idx1, const int32_t *idx2, int64_t n_pair, int32_t **didx)
{
    int rc = 0;
    DevBuf *b = c.bufs.get(sizeof(int32_t) * 2 * (size_t)n_pair, rc);
    if (rc) return 1;
    int32_t *d = (int32_t *)b->p;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(d, idx1, sizeof(int32_t) * (size_t)n_pair, hipMemcpyHostToDevice, c.st.s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(d + n_pair, idx2, sizeof(int32_t) * (size_t)n_pair, hipMemcpyHostToDevice, c.st.s));
    *didx = d;
    return 0;
}

// the SNP-table kernel on one block, timed
int snp_table_block(Call &c, const uint8_t *src, int64_t rb, int64_t nb, const int32_t *didx, int64_t n_pair, int32_t *tab, uint8_t *flip)
{
    hipStream_t s = c.st.s;
    if (c.log.begin(T_SNP, s) || launch_pair_snp_table(s, src, rb, nb, didx, didx + n_pair, n_pair, tab, flip) || c.log.end(s)) return 1;
    if (c.log.wait_last(&g_stats[0])) return 1;
    g_stats[1] += 1; g_stats[2] += (double)nb * (double)rb;
    return 0;
}

// largest multiple of 16 SNPs whose per-block buffer of bytes_per_snp stays within `bytes` (at least 16)
int64_t block_snps_for(size_t bytes, double bytes_per_snp)
{
    const double b = std::floor((double)bytes / bytes_per_snp / 16.0) * 16.0;
    return (int64_t)std::min<double>((double)PS_MAX_BLOCK_SNPS, std::max<double>(16.0, b));
}

// CalcAvgSD (src/dGenGWAS.cpp:2365-2379) on exact integer sums
void avg_sd(int64_t sum, int64_t sqsum, int64_t num, double *avg, double *sd)
{
    const double Sum = (double)sum, SqSum = (double)sqsum, Num = (double)num;
    if (num > 1) {
        const double Avg = Sum / Num;
        const double t = Num * Avg;
        const double u = t * Avg;
        *avg = Avg;
        *sd = std::sqrt((SqSum - u) / (double)(num - 1));
    } else if (num == 1) {
        *avg = Sum; *sd = std::nan("");
    } else {
        *avg = *sd = std::nan("");
    }
}

}  // namespace

extern "C" {

int snpgpu_pair_tables(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *idx1, const int32_t *idx2,
                       int64_t n_pair, int need_major, int64_t *pair_tab, int32_t *snp_tab, uint8_t *flip, int out_mem, int device)
{
    const char *fn = "snpgpu_pair_tables";
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, PS_GENO)) return 1;
    if (check_pairs(fn, idx1, idx2, n_pair, n_samp)) return 1;
    if (!pair_tab && !snp_tab && !flip) return fail(fn, "pair_tab, snp_tab and flip are all NULL");
    if (out_mem != SNPGPU_HOST && out_mem != SNPGPU_DEVICE) return fail(fn, "invalid out_mem");
    for (double &s : g_stats) s = 0;
    Call c;
    if (c.open(fn, device, true)) return 1;
    hipStream_t s = c.st.s;
    int32_t *didx = nullptr;
    if (upload_pairs(c, idx1, idx2, n_pair, &didx)) return 1;
    HostOut op, os, of;
    if (op.open(c.bufs, pair_tab, sizeof(int64_t) * 9 * (size_t)n_pair, out_mem, false, s) ||
        os.open(c.bufs, snp_tab, sizeof(int32_t) * 16 * (size_t)n_snp, out_mem, false, s) ||
        of.open(c.bufs, flip, (size_t)n_snp, out_mem, false, s))
        return 1;
    if (op.dev) SNPGPU_HIP_CHECK(hipMemsetAsync(op.dev, 0, op.bytes, s));
    const bool flip_pairs = pair_tab && need_major;

    RowBlocks blocks;
    const int64_t max_block = pair_tab ? block_snps_for(PS_WORDS_BYTES, 8.0 * (double)n_pair / 16.0) : PS_MAX_BLOCK_SNPS;
    if (blocks.open(c.bufs, geno, n_snp, n_samp, format, mem, PS_STAGE_BYTES, max_block, "SNPGPU_PAIR_BLOCK_SNPS")) return 1;
    const int64_t nwb = blocks.B / 16;
    int rc = 0;
    DevBuf *words = pair_tab ? c.bufs.get(sizeof(uint32_t) * 2 * (size_t)n_pair * (size_t)nwb, rc) : nullptr;
    DevBuf *fw = flip_pairs ? c.bufs.get(sizeof(uint32_t) * (size_t)nwb, rc) : nullptr;
    DevBuf *bflip = (flip_pairs && !flip) ? c.bufs.get((size_t)blocks.B, rc) : nullptr;     // the flips of one block
    if (rc) return 1;

    if (blocks.for_each(s, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
            uint8_t *fl = of.dev ? (uint8_t *)of.dev + i0 : bflip ? (uint8_t *)bflip->p : nullptr;
            if (os.dev || fl) {
                if (snp_table_block(c, src, rb, nb, didx, n_pair, os.dev ? (int32_t *)os.dev + 16 * i0 : nullptr, fl)) return 1;
            }
            if (!pair_tab) return 0;
            if (c.log.begin(T_WORDS, s) || (fw && launch_pair_flip_words(s, fl, nb, (uint32_t *)fw->p)) ||
                launch_pair_words(s, src, rb, nb, didx, n_pair, (uint32_t *)words->p) || c.log.end(s))
                return 1;
            if (c.log.wait_last(&g_stats[3])) return 1;
            if (c.log.begin(T_COUNT, s) ||
                launch_pair_count(s, (const uint32_t *)words->p, fw ? (const uint32_t *)fw->p : nullptr, nb, n_pair,
                                  (unsigned long long *)op.dev) ||
                c.log.end(s))
                return 1;
            if (c.log.wait_last(&g_stats[4])) return 1;
            g_stats[6] += 2; g_stats[7] += (double)nb * (double)rb;
            return 0;
        }))
        return 1;
    if (op.close(s) || os.close(s) || of.close(s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int snpgpu_pair_score_final(int table_kind, const void *table, const uint8_t *flip, int64_t n, int method, int dosage, double *out)
{
    const char *fn = "snpgpu_pair_score_final";
    const int8_t *map = ps_map(method, dosage);
    if (!map) return fail(fn, "Invalid 'method'.");
    if (table_kind != SNPGPU_PS_PAIR_TABLE && table_kind != SNPGPU_PS_SNP_TABLE) return fail(fn, "invalid table kind");
    if (!table || !out) return fail(fn, "NULL argument: table / out is NULL");
    if (n < 1) return fail(fn, "invalid number of rows");
    if (table_kind == SNPGPU_PS_SNP_TABLE && ps_need_major(method) && !flip) return fail(fn, "NULL argument: the method needs flip");
    if (table_kind == SNPGPU_PS_PAIR_TABLE) {
        const int64_t *t = (const int64_t *)table;
        for (int64_t i = 0; i < 9 * n; i++)
            if (t[i] < 0) return fail(fn, "a count is negative");
        for (int64_t i = 0; i < n; i++) {
            int64_t sum = 0, sq = 0, num = 0;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    const int64_t cnt = t[9 * i + 3 * a + b], v = map[4 * a + b];
                    sum += cnt * v; sq += cnt * v * v; num += cnt;
                }
            avg_sd(sum, sq, num, out + i, out + n + i);                  // n x 3, column-major
            out[2 * n + i] = (double)num;
        }
        return 0;
    }
    const int32_t *t = (const int32_t *)table;
    for (int64_t i = 0; i < 16 * n; i++)
        if (t[i] < 0) return fail(fn, "a count is negative");
    const bool major = ps_need_major(method);
    for (int64_t i = 0; i < n; i++) {
        const bool f = major && flip[i];
        int64_t sum = 0, sq = 0, num = 0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const int64_t cnt = t[16 * i + 4 * a + b], v = f ? map[4 * (2 - a) + (2 - b)] : map[4 * a + b];
                sum += cnt * v; sq += cnt * v * v; num += cnt;
            }
        avg_sd(sum, sq, num, out + 3 * i, out + 3 * i + 1);                // 3 x n
        out[3 * i + 2] = (double)num;
    }
    return 0;
}

int snpgpu_pair_score_matrix(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *idx1,
                             const int32_t *idx2, int64_t n_pair, int method, int dosage, int elem_kind, void *out_host, int device)
{
    const char *fn = "snpgpu_pair_score_matrix";
    const int8_t *map = ps_map(method, dosage);
    if (!map) return fail(fn, "Invalid 'method'.");
    if (elem_kind != SNPGPU_PS_ELEM_INT32 && elem_kind != SNPGPU_PS_ELEM_BIT2) return fail(fn, "invalid element kind");
    if (check_geno(fn, geno, n_snp, n_samp, format, mem, PS_GENO)) return 1;
    if (check_pairs(fn, idx1, idx2, n_pair, n_samp)) return 1;
    if (!out_host) return fail(fn, "NULL argument: out is NULL");
    for (double &s : g_stats) s = 0;
    uint32_t map2 = 0;
    for (int k = 0; k < 16; k++) map2 |= ((uint32_t)map[k] & 3u) << (2 * k);
    const size_t esz = elem_kind == SNPGPU_PS_ELEM_INT32 ? 4 : 1;
    Call c;
    if (c.open(fn, device, true)) return 1;
    hipStream_t s = c.st.s;
    int32_t *didx = nullptr;
    if (upload_pairs(c, idx1, idx2, n_pair, &didx)) return 1;
    RowBlocks blocks;
    if (blocks.open(c.bufs, geno, n_snp, n_samp, format, mem, PS_STAGE_BYTES, block_snps_for(PS_MATRIX_BYTES, (double)esz * (double)n_pair),
                    "SNPGPU_PAIR_BLOCK_SNPS"))
        return 1;
    int rc = 0;
    DevBuf *dout = c.bufs.get(esz * (size_t)n_pair * (size_t)blocks.B, rc);
    DevBuf *bflip = ps_need_major(method) ? c.bufs.get((size_t)blocks.B, rc) : nullptr;
    if (rc) return 1;
    if (blocks.for_each(s, [&](const uint8_t *src, int64_t rb, int64_t i0, int64_t nb) {
            uint8_t *fl = bflip ? (uint8_t *)bflip->p : nullptr;
            if (fl && snp_table_block(c, src, rb, nb, didx, n_pair, nullptr, fl)) return 1;
            if (c.log.begin(T_MATRIX, s) || launch_pair_matrix(s, src, rb, nb, didx, didx + n_pair, n_pair, fl, map2, (int)esz, dout->p) ||
                c.log.end(s))
                return 1;
            if (c.log.wait_last(&g_stats[5])) return 1;
            g_stats[6] += 1; g_stats[7] += (double)nb * (double)rb;
            SNPGPU_HIP_CHECK(hipMemcpyAsync((uint8_t *)out_host + esz * (size_t)n_pair * (size_t)i0, dout->p, esz * (size_t)n_pair * (size_t)nb,
                                            hipMemcpyDeviceToHost, s));
            return 0;
        }))
        return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int snpgpu_pair_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_pair_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 8; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
