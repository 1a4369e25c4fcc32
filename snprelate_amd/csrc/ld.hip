// C ABI of libsnpgpu, linkage disequilibrium (include/snpgpu.h section 1d): the streaming object behind snpgdsLDMat
// (gnrLDMat, src/genLD.cpp:957-1010) and the pair-table primitive.  Kernels: kernels_ld.hip.
//
// Device rows use the staging layout of the table kernel: rbp = round_up(ceil(N / 4), 32) bytes per SNP, samples >= N missing,
// every buffer a whole number of 64-row tiles plus one spare tile (the kernel reads whole tiles).
//   sliding window: two row buffers of `cap` = slide + blk rows used in turn; a full buffer (or the last SNP) finalises the
//     columns whose partners are all resident, in chunks of at most blk rows (tables [blk][slide][9]), and the last `slide`
//     rows move to the other buffer as the halo of the next block.  The result matrix stays on the host.
//   full matrix: all L rows resident; snpgpu_ld_result works through row panels of P rows against all L columns (tables
//     [P][L][9]) and copies each finished panel -- rows p0 ... p0 + P - 1 of the symmetric matrix -- straight to the caller.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"

using namespace snpgpu;

namespace {

inline int64_t ld_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
constexpr size_t LD_TABLE_BUDGET = size_t(1) << 30;   // bytes of tables + finalised values per launch pair
constexpr int64_t LD_BLOCK_DEFAULT = 16384;
enum { T_TABLE = 0, T_FINAL = 1, T_COPY = 2 };          // snpgpu_ld_get_timing's `which`: table kernel, finaliser, copies of the result

}  // namespace

struct snpgpu_ld {
    int device = 0;
    CallStream st;
    int64_t N = 0, L = 0, rb = 0, rbp = 0;
    int method = 0;
    int64_t slide = 0;          // 0: full matrix
    bool trim = false;
    int64_t out_rows = 0, out_cols = 0;
    int64_t blk = 0;            // sliding window: rows per table launch
    int64_t cap = 0;            // rows per row buffer
    DevBuf rows[2], raw, tab, dout;
    int cur = 0;
    int64_t n_fed = 0, base = 0, n_res = 0, done = 0;
    std::vector<double> host_out;   // sliding window: the whole result
    EventLog log;
};

namespace {

void ld_free(snpgpu_ld *ld)
{
    for (auto &b : ld->rows) b.release();
    ld->raw.release(); ld->tab.release(); ld->dout.release();
    delete ld;
}

// n rows of the caller's block -> staging rows at dst; returns when the caller's block has been read (the caller may overwrite
// or free it as soon as snpgpu_ld_feed returns)
int ld_stage(snpgpu_ld *ld, const uint8_t *src, int64_t n, int format, int mem, uint8_t *dst)
{
    if (stage_ld_rows(ld->st.s, ld->raw, src, n, ld->N, ld->rbp, format, mem, dst)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->st.s));
    return 0;
}

// sliding window: finalise the columns [done, i_end) whose partners are resident, then keep the last `slide` rows as the halo
int ld_band_process(snpgpu_ld *ld)
{
    const bool last = ld->n_fed == ld->L;
    const int64_t i_end = last ? ld->L : ld->base + ld->n_res - ld->slide;
    const uint8_t *rows = (const uint8_t *)ld->rows[ld->cur].p;
    hipStream_t s = ld->st.s;
    for (int64_t i0 = ld->done; i0 < i_end; i0 += ld->blk) {
        const int64_t n_i = std::min(ld->blk, i_end - i0);
        if (ld->log.begin(T_TABLE, s) ||
            launch_ld_count_band(s, rows, (int)(i0 - ld->base), (int)n_i, (int)ld->n_res, (int)ld->slide, ld->rbp, (int32_t *)ld->tab.p) ||
            ld->log.end(s))
            return 1;
        if (ld->log.begin(T_FINAL, s) ||
            launch_ld_final_band(s, (const int32_t *)ld->tab.p, n_i, (int)ld->slide, i0, ld->L, ld->method, (double *)ld->dout.p) ||
            ld->log.end(s))
            return 1;
        const int64_t n_out = std::min(n_i, ld->out_cols - i0);   // mat_trim drops the last `slide` columns
        if (n_out > 0) {
            if (ld->log.begin(T_COPY, s)) return 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(ld->host_out.data() + i0 * ld->slide, ld->dout.p, (size_t)(n_out * ld->slide) * 8,
                                            hipMemcpyDeviceToHost, s));
            if (ld->log.end(s)) return 1;
        }
    }
    ld->done = i_end;
    if (!last) {
        const int64_t keep = ld->base + ld->n_res - i_end;   // == slide
        const int nxt = ld->cur ^ 1;
        if (keep > 0)
            SNPGPU_HIP_CHECK(hipMemcpyAsync(ld->rows[nxt].p, rows + (i_end - ld->base) * ld->rbp, (size_t)(keep * ld->rbp),
                                            hipMemcpyDeviceToDevice, s));
        ld->cur = nxt;
        ld->base = i_end;
        ld->n_res = keep;
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_ld_create(int64_t n_samp, int64_t n_snp, int method, int64_t slide, int mat_trim, const snpgpu_opts *opts, snpgpu_ld **out)
{
    const char *fn = "snpgpu_ld_create";
    if (!out) return fail(fn, "out is NULL");
    *out = nullptr;
    if (check_dims(fn, n_snp, n_samp, LD_GENO)) return 1;
    if (method < SNPGPU_LD_COMPOSITE || method > SNPGPU_LD_COV) return fail(fn, "invalid LD method");
    snpgpu_opts o{};
    if (opts) o = *opts;
    snpgpu_ld *ld = new snpgpu_ld();
    if (ld->st.open(fn, o.device, o.stream)) { delete ld; return 1; }
    ld->device = o.device; ld->N = n_samp; ld->L = n_snp; ld->method = method;
    ld->rb = (n_samp + 3) / 4;
    ld->rbp = ld_up(ld->rb, 32);
    ld->slide = slide <= 0 ? 0 : std::min(slide, n_snp);
    ld->trim = mat_trim != 0;
    if (ld->slide == 0) { ld->out_rows = ld->out_cols = n_snp; }
    else { ld->out_rows = ld->slide; ld->out_cols = ld->trim ? n_snp - ld->slide : n_snp; }
    const int64_t want = o.max_block_snps > 0 ? o.max_block_snps : LD_BLOCK_DEFAULT;
    int rc = 0;
    if (ld->slide > 0) {
        const int64_t fit = (int64_t)(LD_TABLE_BUDGET / ((size_t)ld->slide * 44));
        ld->blk = std::max<int64_t>(64, std::min(ld_up(want, 64), fit / 64 * 64));
        ld->cap = std::min(ld->slide + ld->blk, n_snp);
        const size_t rbytes = (size_t)(ld_up(ld->cap, 64) + 64) * (size_t)ld->rbp;
        rc |= ld->rows[0].alloc(rbytes) | ld->rows[1].alloc(rbytes);
        rc |= ld->tab.alloc((size_t)ld->blk * (size_t)ld->slide * 36) | ld->dout.alloc((size_t)ld->blk * (size_t)ld->slide * 8);
        try { ld->host_out.assign((size_t)(ld->out_rows * ld->out_cols), __builtin_nan("")); }
        catch (...) { rc = 1; }
    } else {
        ld->cap = n_snp;
        rc |= ld->rows[0].alloc((size_t)(ld_up(n_snp, 64) + 64) * (size_t)ld->rbp);
    }
    // spare rows past the data are read by whole tiles: give them a defined content (all missing)
    for (auto &b : ld->rows)
        if (!rc && b.p && hipMemsetAsync(b.p, 0xFF, b.bytes, ld->st.s) != hipSuccess) rc = 1;
    if (!rc && hipStreamSynchronize(ld->st.s) != hipSuccess) rc = 1;
    if (rc) { ld_free(ld); return fail(fn, "allocation failed"); }
    *out = ld;
    return 0;
}

int snpgpu_ld_destroy(snpgpu_ld *ld)
{
    if (!ld) return 0;
    (void)hipSetDevice(ld->device);
    (void)hipStreamSynchronize(ld->st.s);
    ld_free(ld);
    return 0;
}

int snpgpu_ld_out_dims(const snpgpu_ld *ld, int64_t *rows, int64_t *cols)
{
    if (!ld) { set_error("snpgpu_ld_out_dims: NULL object"); return 1; }
    if (rows) *rows = ld->out_rows;
    if (cols) *cols = ld->out_cols;
    return 0;
}

int snpgpu_ld_feed(snpgpu_ld *ld, const void *geno, int64_t n_snp, int format, int mem)
{
    if (!ld || (!geno && n_snp > 0)) { set_error("snpgpu_ld_feed: NULL argument"); return 1; }
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) { set_error("snpgpu_ld_feed: invalid genotype format"); return 1; }
    if (n_snp < 0 || ld->n_fed + n_snp > ld->L) { set_error("snpgpu_ld_feed: more SNPs than announced at snpgpu_ld_create"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(ld->device));
    const uint8_t *src = (const uint8_t *)geno;
    const int64_t irb = format == SNPGPU_GENO_U8 ? ld->N : ld->rb;
    if (ld->slide == 0) {
        if (ld_stage(ld, src, n_snp, format, mem, (uint8_t *)ld->rows[0].p + ld->n_fed * ld->rbp)) return 1;
        ld->n_fed += n_snp;
        return 0;
    }
    for (int64_t o = 0; o < n_snp;) {
        const int64_t m = std::min(n_snp - o, ld->cap - ld->n_res);
        if (ld_stage(ld, src + o * irb, m, format, mem, (uint8_t *)ld->rows[ld->cur].p + ld->n_res * ld->rbp)) return 1;
        ld->n_res += m; ld->n_fed += m; o += m;
        if (ld->n_res == ld->cap || ld->n_fed == ld->L)
            if (ld_band_process(ld)) return 1;
    }
    return 0;
}

int snpgpu_ld_result(snpgpu_ld *ld, double *out, int out_mem)
{
    if (!ld || !out) { set_error("snpgpu_ld_result: NULL argument"); return 1; }
    if (ld->n_fed != ld->L) { set_error("snpgpu_ld_result: not all SNPs have been fed"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(ld->device));
    const hipMemcpyKind h2x = out_mem == SNPGPU_DEVICE ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
    if (ld->slide > 0) {
        if (!ld->host_out.empty())
            SNPGPU_HIP_CHECK(hipMemcpy(out, ld->host_out.data(), ld->host_out.size() * 8, h2x));
        return 0;
    }
    const int64_t L = ld->L;
    const int64_t P = std::max<int64_t>(64, std::min(ld_up(L, 64), (int64_t)(LD_TABLE_BUDGET / ((size_t)L * 44)) / 64 * 64));
    if (ld->tab.bytes < (size_t)(P * L * 36)) {
        ld->tab.release(); ld->dout.release();
        if (ld->tab.alloc((size_t)(P * L * 36)) || ld->dout.alloc((size_t)(P * L * 8))) return 1;
    }
    const uint8_t *rows = (const uint8_t *)ld->rows[0].p;
    const hipMemcpyKind d2x = out_mem == SNPGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = ld->st.s;
    for (int64_t p0 = 0; p0 < L; p0 += P) {
        const int64_t n_p = std::min(P, L - p0);
        if (ld->log.begin(T_TABLE, s) ||
            launch_ld_count_rect(s, rows + p0 * ld->rbp, (int)n_p, rows, (int)L, ld->rbp, (int32_t *)ld->tab.p) || ld->log.end(s))
            return 1;
        if (ld->log.begin(T_FINAL, s) ||
            launch_ld_final_rect(s, (const int32_t *)ld->tab.p, n_p, L, p0, ld->method, (double *)ld->dout.p) || ld->log.end(s))
            return 1;
        if (ld->log.begin(T_COPY, s)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(out + p0 * L, ld->dout.p, (size_t)(n_p * L) * 8, d2x, s));
        if (ld->log.end(s)) return 1;
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int snpgpu_ld_set_timing(snpgpu_ld *ld, int enable)
{
    if (!ld) { set_error("snpgpu_ld_set_timing: NULL object"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(ld->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->st.s));
    ld->log.clear();
    ld->log.on = enable != 0;
    return 0;
}

int snpgpu_ld_get_timing(snpgpu_ld *ld, int which, double *ms_sum, int64_t *launches)
{
    if (!ld || which < 0 || which > 2) { set_error("snpgpu_ld_get_timing: invalid argument"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(ld->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->st.s));
    double ms = 0;
    if (ld->log.sum_ms(which, &ms)) return 1;
    if (ms_sum) *ms_sum = ms;
    if (launches) *launches = ld->log.count(which);
    return 0;
}

int snpgpu_ld_pair_tables(const void *geno_a, int64_t n_a, const void *geno_b, int64_t n_b, int64_t n_samp, int format, int32_t *tab,
                          int device)
{
    const char *fn = "snpgpu_ld_pair_tables";
    if (check_geno(fn, geno_a, n_a, n_samp, format, SNPGPU_HOST, LD_GENO) || check_geno(fn, geno_b, n_b, n_samp, format, SNPGPU_HOST, LD_GENO))
        return 1;
    if (!tab) return fail(fn, "NULL argument");
    Call c;
    if (c.open(fn, device, false)) return 1;
    hipStream_t s = c.st.s;
    const int64_t rbp = ld_up((n_samp + 3) / 4, 32);
    const int64_t P = std::max<int64_t>(64, std::min(ld_up(n_a, 64), (int64_t)(LD_TABLE_BUDGET / ((size_t)n_b * 36)) / 64 * 64));
    int rc = 0;
    DevBuf *ra = c.bufs.get((size_t)(ld_up(n_a, 64) + 64) * rbp, rc), *rbuf = c.bufs.get((size_t)(ld_up(n_b, 64) + 64) * rbp, rc);
    DevBuf *dtab = c.bufs.get((size_t)(P * n_b * 36), rc), *raw = c.bufs.get(0, rc);
    if (rc) return 1;
    // spare rows past the data are read by whole tiles: all missing
    SNPGPU_HIP_CHECK(hipMemsetAsync(ra->p, 0xFF, ra->bytes, s));
    SNPGPU_HIP_CHECK(hipMemsetAsync(rbuf->p, 0xFF, rbuf->bytes, s));
    if (stage_ld_rows(s, *raw, (const uint8_t *)geno_a, n_a, n_samp, rbp, format, SNPGPU_HOST, (uint8_t *)ra->p) ||
        stage_ld_rows(s, *raw, (const uint8_t *)geno_b, n_b, n_samp, rbp, format, SNPGPU_HOST, (uint8_t *)rbuf->p))
        return 1;
    for (int64_t p0 = 0; p0 < n_a; p0 += P) {
        const int64_t n_p = std::min(P, n_a - p0);
        if (launch_ld_count_rect(s, (const uint8_t *)ra->p + p0 * rbp, (int)n_p, (const uint8_t *)rbuf->p, (int)n_b, rbp, (int32_t *)dtab->p))
            return 1;
        if (hipMemcpyAsync(tab + p0 * n_b * 9, dtab->p, (size_t)(n_p * n_b * 36), hipMemcpyDeviceToHost, s) != hipSuccess)
            return fail(fn, "copy of the tables failed");
    }
    if (hipStreamSynchronize(s) != hipSuccess) return fail(fn, "kernel failed");
    return 0;
}

}  // extern "C"
