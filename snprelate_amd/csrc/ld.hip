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

#include "snpgpu_internal.h"

using namespace snpgpu;

namespace {

inline int64_t ld_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
constexpr size_t LD_TABLE_BUDGET = size_t(1) << 30;   // bytes of tables + finalised values per launch pair
constexpr int64_t LD_BLOCK_DEFAULT = 16384;
constexpr size_t LD_RAW_BYTES = size_t(64) << 20;      // host-feed staging buffer, at most

}  // namespace

struct snpgpu_ld {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
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
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[3];   // table kernel, finaliser, device -> caller copies of the result
};

namespace {

void ld_free(snpgpu_ld *ld)
{
    for (auto &b : ld->rows) b.release();
    ld->raw.release(); ld->tab.release(); ld->dout.release();
    for (auto &v : ld->ev)
        for (auto &p : v) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (ld->own_stream && ld->stream) (void)hipStreamDestroy(ld->stream);
    delete ld;
}

// HIP events around one launch when timing is on
struct LdTimed {
    snpgpu_ld *ld; int which; hipEvent_t a = nullptr, b = nullptr;
    LdTimed(snpgpu_ld *l, int w) : ld(l), which(w)
    {
        if (!ld->timing) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, ld->stream);
    }
    ~LdTimed()
    {
        if (!a) return;
        (void)hipEventRecord(b, ld->stream);
        ld->ev[which].push_back({a, b});
    }
};

int64_t in_row_bytes(const snpgpu_ld *ld, int format) { return format == SNPGPU_GENO_U8 ? ld->N : ld->rb; }

// n rows of the caller's block -> staging rows at dst.  Host memory goes through `raw`, at most LD_RAW_BYTES per copy (allocated on
// the first host feed, sized by the rows actually fed).  Both paths return when the caller's block has been read.
int ld_stage(snpgpu_ld *ld, const uint8_t *src, int64_t n, int format, int mem, uint8_t *dst)
{
    const int64_t irb = in_row_bytes(ld, format);
    if (mem == SNPGPU_DEVICE) {
        if (launch_ld_stage(ld->stream, src, format, n, ld->N, ld->rbp, dst)) return 1;
    } else {
        const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)LD_RAW_BYTES / irb));
        if (ld->raw.bytes < (size_t)(chunk * irb)) {
            SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->stream));
            ld->raw.release();
            if (ld->raw.alloc((size_t)(chunk * irb))) return 1;
        }
        for (int64_t o = 0; o < n; o += chunk) {
            const int64_t m = std::min(chunk, n - o);
            SNPGPU_HIP_CHECK(hipMemcpyAsync(ld->raw.p, src + o * irb, (size_t)(m * irb), hipMemcpyHostToDevice, ld->stream));
            if (launch_ld_stage(ld->stream, ld->raw.p, format, m, ld->N, ld->rbp, dst + o * ld->rbp)) return 1;
        }
    }
    // the caller may overwrite or free its block as soon as the call returns
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->stream));
    return 0;
}

// sliding window: finalise the columns [done, i_end) whose partners are resident, then keep the last `slide` rows as the halo
int ld_band_process(snpgpu_ld *ld)
{
    const bool last = ld->n_fed == ld->L;
    const int64_t i_end = last ? ld->L : ld->base + ld->n_res - ld->slide;
    const uint8_t *rows = (const uint8_t *)ld->rows[ld->cur].p;
    for (int64_t i0 = ld->done; i0 < i_end; i0 += ld->blk) {
        const int64_t n_i = std::min(ld->blk, i_end - i0);
        {
            LdTimed t(ld, 0);
            if (launch_ld_count_band(ld->stream, rows, (int)(i0 - ld->base), (int)n_i, (int)ld->n_res, (int)ld->slide, ld->rbp,
                                     (int32_t *)ld->tab.p)) return 1;
        }
        {
            LdTimed t(ld, 1);
            if (launch_ld_final_band(ld->stream, (const int32_t *)ld->tab.p, n_i, (int)ld->slide, i0, ld->L, ld->method,
                                     (double *)ld->dout.p)) return 1;
        }
        const int64_t n_out = std::min(n_i, ld->out_cols - i0);   // mat_trim drops the last `slide` columns
        if (n_out > 0) {
            LdTimed t(ld, 2);
            SNPGPU_HIP_CHECK(hipMemcpyAsync(ld->host_out.data() + i0 * ld->slide, ld->dout.p, (size_t)(n_out * ld->slide) * 8,
                                            hipMemcpyDeviceToHost, ld->stream));
        }
    }
    ld->done = i_end;
    if (!last) {
        const int64_t keep = ld->base + ld->n_res - i_end;   // == slide
        const int nxt = ld->cur ^ 1;
        if (keep > 0)
            SNPGPU_HIP_CHECK(hipMemcpyAsync(ld->rows[nxt].p, rows + (i_end - ld->base) * ld->rbp, (size_t)(keep * ld->rbp),
                                            hipMemcpyDeviceToDevice, ld->stream));
        ld->cur = nxt;
        ld->base = i_end;
        ld->n_res = keep;
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->stream));
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_ld_create(int64_t n_samp, int64_t n_snp, int method, int64_t slide, int mat_trim, const snpgpu_opts *opts, snpgpu_ld **out)
{
    if (!out) { set_error("snpgpu_ld_create: out is NULL"); return 1; }
    *out = nullptr;
    if (n_samp <= 0 || n_samp >= (int64_t(1) << 24)) { set_error("snpgpu_ld_create: invalid number of samples (1 ... 2^24 - 1)"); return 1; }
    if (n_snp <= 0 || n_snp > 0x3fffffffLL) { set_error("snpgpu_ld_create: invalid number of SNPs"); return 1; }
    if (method < SNPGPU_LD_COMPOSITE || method > SNPGPU_LD_COV) { set_error("snpgpu_ld_create: invalid LD method"); return 1; }
    snpgpu_opts o{};
    if (opts) o = *opts;
    int ndev = 0;
    SNPGPU_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) { set_error("snpgpu_ld_create: no HIP device (the GPU path has no CPU fallback)"); return 1; }
    if (o.device < 0 || o.device >= ndev) { set_error("snpgpu_ld_create: invalid device ordinal"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(o.device));
    snpgpu_ld *ld = new snpgpu_ld();
    ld->device = o.device; ld->N = n_samp; ld->L = n_snp; ld->method = method;
    ld->rb = (n_samp + 3) / 4;
    ld->rbp = ld_up(ld->rb, 32);
    ld->slide = slide <= 0 ? 0 : std::min(slide, n_snp);
    ld->trim = mat_trim != 0;
    if (ld->slide == 0) { ld->out_rows = ld->out_cols = n_snp; }
    else { ld->out_rows = ld->slide; ld->out_cols = ld->trim ? n_snp - ld->slide : n_snp; }
    const int64_t want = o.max_block_snps > 0 ? o.max_block_snps : LD_BLOCK_DEFAULT;
    if (o.stream) ld->stream = (hipStream_t)o.stream;
    else if (hipStreamCreateWithFlags(&ld->stream, hipStreamNonBlocking) == hipSuccess) ld->own_stream = true;
    else { set_error("snpgpu_ld_create: hipStreamCreate failed"); delete ld; return 1; }
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
        if (!rc && b.p && hipMemsetAsync(b.p, 0xFF, b.bytes, ld->stream) != hipSuccess) rc = 1;
    if (!rc && hipStreamSynchronize(ld->stream) != hipSuccess) rc = 1;
    if (rc) { ld_free(ld); set_error("snpgpu_ld_create: allocation failed"); return 1; }
    *out = ld;
    return 0;
}

int snpgpu_ld_destroy(snpgpu_ld *ld)
{
    if (!ld) return 0;
    (void)hipSetDevice(ld->device);
    if (ld->stream) (void)hipStreamSynchronize(ld->stream);
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
    const int64_t irb = in_row_bytes(ld, format);
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
    for (int64_t p0 = 0; p0 < L; p0 += P) {
        const int64_t n_p = std::min(P, L - p0);
        {
            LdTimed t(ld, 0);
            if (launch_ld_count_rect(ld->stream, rows + p0 * ld->rbp, (int)n_p, rows, (int)L, ld->rbp, (int32_t *)ld->tab.p)) return 1;
        }
        {
            LdTimed t(ld, 1);
            if (launch_ld_final_rect(ld->stream, (const int32_t *)ld->tab.p, n_p, L, p0, ld->method, (double *)ld->dout.p)) return 1;
        }
        {
            LdTimed t(ld, 2);
            SNPGPU_HIP_CHECK(hipMemcpyAsync(out + p0 * L, ld->dout.p, (size_t)(n_p * L) * 8, d2x, ld->stream));
        }
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->stream));
    return 0;
}

int snpgpu_ld_set_timing(snpgpu_ld *ld, int enable)
{
    if (!ld) { set_error("snpgpu_ld_set_timing: NULL object"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(ld->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->stream));
    for (auto &v : ld->ev) {
        for (auto &p : v) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        v.clear();
    }
    ld->timing = enable != 0;
    return 0;
}

int snpgpu_ld_get_timing(snpgpu_ld *ld, int which, double *ms_sum, int64_t *launches)
{
    if (!ld || which < 0 || which > 2) { set_error("snpgpu_ld_get_timing: invalid argument"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(ld->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(ld->stream));
    double s = 0;
    for (auto &p : ld->ev[which]) {
        float ms = 0;
        SNPGPU_HIP_CHECK(hipEventElapsedTime(&ms, p.first, p.second));
        s += ms;
    }
    if (ms_sum) *ms_sum = s;
    if (launches) *launches = (int64_t)ld->ev[which].size();
    return 0;
}

int snpgpu_ld_pair_tables(const void *geno_a, int64_t n_a, const void *geno_b, int64_t n_b, int64_t n_samp, int format, int32_t *tab,
                          int device)
{
    if (!geno_a || !geno_b || !tab) { set_error("snpgpu_ld_pair_tables: NULL argument"); return 1; }
    if (n_a <= 0 || n_b <= 0 || n_a > 0x3fffffffLL || n_b > 0x3fffffffLL) { set_error("snpgpu_ld_pair_tables: invalid number of SNPs"); return 1; }
    if (n_samp <= 0 || n_samp >= (int64_t(1) << 24)) { set_error("snpgpu_ld_pair_tables: invalid number of samples (1 ... 2^24 - 1)"); return 1; }
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) { set_error("snpgpu_ld_pair_tables: invalid genotype format"); return 1; }
    int ndev = 0;
    SNPGPU_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) { set_error("snpgpu_ld_pair_tables: no HIP device (the GPU path has no CPU fallback)"); return 1; }
    if (device < 0 || device >= ndev) { set_error("snpgpu_ld_pair_tables: invalid device ordinal"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    // a throw-away object carries the stream and the staging buffer
    snpgpu_ld tmp;
    tmp.device = device; tmp.N = n_samp; tmp.rb = (n_samp + 3) / 4; tmp.rbp = ld_up(tmp.rb, 32);
    const int64_t P = std::max<int64_t>(64, std::min(ld_up(n_a, 64), (int64_t)(LD_TABLE_BUDGET / ((size_t)n_b * 36)) / 64 * 64));
    DevBuf ra, rbuf, dtab;
    int rc = 0;
    if (hipStreamCreateWithFlags(&tmp.stream, hipStreamNonBlocking) != hipSuccess) { set_error("snpgpu_ld_pair_tables: hipStreamCreate failed"); return 1; }
    rc |= ra.alloc((size_t)(ld_up(n_a, 64) + 64) * tmp.rbp) | rbuf.alloc((size_t)(ld_up(n_b, 64) + 64) * tmp.rbp);
    rc |= dtab.alloc((size_t)(P * n_b * 36));
    if (!rc && (hipMemsetAsync(ra.p, 0xFF, ra.bytes, tmp.stream) != hipSuccess || hipMemsetAsync(rbuf.p, 0xFF, rbuf.bytes, tmp.stream) != hipSuccess))
        rc = 1;
    if (!rc) rc = ld_stage(&tmp, (const uint8_t *)geno_a, n_a, format, SNPGPU_HOST, (uint8_t *)ra.p);
    if (!rc) rc = ld_stage(&tmp, (const uint8_t *)geno_b, n_b, format, SNPGPU_HOST, (uint8_t *)rbuf.p);
    for (int64_t p0 = 0; !rc && p0 < n_a; p0 += P) {
        const int64_t n_p = std::min(P, n_a - p0);
        rc = launch_ld_count_rect(tmp.stream, (const uint8_t *)ra.p + p0 * tmp.rbp, (int)n_p, (const uint8_t *)rbuf.p, (int)n_b, tmp.rbp,
                                  (int32_t *)dtab.p);
        if (!rc && hipMemcpyAsync(tab + p0 * n_b * 9, dtab.p, (size_t)(n_p * n_b * 36), hipMemcpyDeviceToHost, tmp.stream) != hipSuccess) {
            set_error("snpgpu_ld_pair_tables: copy of the tables failed");
            rc = 1;
        }
    }
    if (!rc && hipStreamSynchronize(tmp.stream) != hipSuccess) { set_error("snpgpu_ld_pair_tables: kernel failed"); rc = 1; }
    (void)hipStreamSynchronize(tmp.stream);
    ra.release(); rbuf.release(); dtab.release(); tmp.raw.release();
    (void)hipStreamDestroy(tmp.stream);
    tmp.stream = nullptr;
    return rc;
}

}  // extern "C"
