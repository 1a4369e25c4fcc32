// C ABI of libsnpgpu, selection and layout of genotypes (include/snpgpu.h sections 1j and 1k): the selected rectangle of a 2-bit
// genotype stream -- PACKED2 rows, the raw sample.order or snp.order node, a PLINK .bed file of either mode, a window of any,
// host-gathered segments -- as byte-aligned 2-bit rows of the selected samples and SNPs (gnrCopyGenoMem, src/SNPRelate.cpp:322-382,
// without a byte per genotype anywhere), in the GDS or the BED code set, SNP rows or sample rows.  Kernels: kernels_geno_select.hip.
//
// The kernels know rows and columns of dst, not SNPs and samples: after the argument checks the call speaks of dst's rows (SNPs
// for dst_major 0, samples for dst_major 1) and dst's columns, and a source is either `cross` (its rows are dst's columns: a
// transposition) or not (a row selection and a column gather).  The comments below say SNP and sample as dst_major 0 reads.
//
// A source in device memory is read where it lies, and so is a host source that fits the staging size, after one copy of its
// bytes.  A larger host source goes through one staging buffer in windows: whole source rows
// for SNP rows (copied straight from the caller's memory when they are taken in order, gathered row by row into a host buffer
// when a SNP list or row_bit picks them), windows of output SNPs for sample rows (every selected sample's segment of the window's
// SNP range, gathered on the host with a phase per row).  All argument errors are found before any device is touched.
#include <cstring>
#include <vector>

#include "geno_select.h"
#include "host_util.h"

using namespace snpgpu;

namespace snpgpu {

constexpr size_t SEL_STAGE_BYTES = size_t(256) << 20;    // source bytes per staging window
constexpr GenoLimits SEL_GENO = {1, int64_t(1) << 30, int64_t(1) << 31, false, "invalid number of samples (1 ... 2^30 - 1)"};
constexpr GenoLimits SEL_GENO_MAJOR1 = {1, int64_t(1) << 30, int64_t(1) << 30, false, "invalid number of samples (1 ... 2^30 - 1)"};

size_t sel_stage_bytes() { return env_bytes("SNPGPU_SELECT_STAGE_BYTES", SEL_STAGE_BYTES); }

// All argument errors of a selection: nothing here touches a device.
int sel_check_args(const char *fn, const snpgpu_geno_src *src, int src_code, const int32_t *samp_index, int64_t n_samp_out,
                   const int32_t *snp_index, int64_t n_snp_out, const void *dst, int dst_major, int dst_code, int dst_mem)
{
    if (!src) return fail(fn, "NULL argument: src is NULL");
    if (!src->bits) return fail(fn, "NULL argument: src->bits is NULL");
    if (!dst) return fail(fn, "NULL argument: dst is NULL");
    const auto mem_ok = [](int m) { return m == SNPGPU_HOST || m == SNPGPU_DEVICE || m == SNPGPU_HOST_PINNED; };
    if (!mem_ok(src->mem)) return fail(fn, "invalid memory kind");
    if (!mem_ok(dst_mem)) return fail(fn, "invalid dst_mem");
    if (src->major != 0 && src->major != 1) return fail(fn, "invalid major (0: a row is a SNP, 1: a row is a sample)");
    const auto code_ok = [](int c) { return c == SNPGPU_CODE_GDS || c == SNPGPU_CODE_BED; };
    if (!code_ok(src_code)) return fail(fn, "invalid src_code (SNPGPU_CODE_GDS or SNPGPU_CODE_BED)");
    if (!code_ok(dst_code)) return fail(fn, "invalid dst_code (SNPGPU_CODE_GDS or SNPGPU_CODE_BED)");
    if (dst_major != 0 && dst_major != 1) return fail(fn, "invalid dst_major (0: a row of dst is a SNP, 1: a row of dst is a sample)");
    const int major = src->major;
    // the axis dst packs holds at most 2^30 - 1 entries: for sample rows that is the SNPs
    const GenoLimits &lim = dst_major ? SEL_GENO_MAJOR1 : SEL_GENO;
    const int64_t n_rows = src->n_rows, n_cols = src->n_cols;
    const int64_t src_snp = major ? n_cols : n_rows, src_samp = major ? n_rows : n_cols;
    if (check_dims(fn, src_snp, src_samp, lim)) return 1;
    if (!samp_index && n_samp_out != src_samp) return fail(fn, "samp_index is NULL: n_samp_out should be the source's number of samples");
    if (!snp_index && n_snp_out != src_snp) return fail(fn, "snp_index is NULL: n_snp_out should be the source's number of SNPs");
    if (check_dims(fn, n_snp_out, n_samp_out, lim)) return 1;
    // the description: even, non-negative bit positions inside [bits, bits + n_bytes)
    if (src->n_bytes < 1) return fail(fn, "invalid n_bytes");
    if (src->bit0 < 0 || (src->bit0 & 1)) return fail(fn, "odd or negative bit position: bit0");
    if (!src->row_bit && (src->row_stride_bits < 0 || (src->row_stride_bits & 1)))
        return fail(fn, "odd or negative bit position: row_stride_bits");
    {
        const __int128 end = (__int128)src->n_bytes * 8, span = (__int128)2 * n_cols;
        if (src->row_bit) {
            for (int64_t r = 0; r < n_rows; r++) {
                if (src->row_bit[r] < 0 || (src->row_bit[r] & 1)) return fail(fn, "odd or negative bit position: row_bit[" + std::to_string(r) + "]");
                if ((__int128)src->bit0 + src->row_bit[r] + span > end)
                    return fail(fn, "an element outside n_bytes: row " + std::to_string(r) + " ends beyond the source");
            }
        } else if ((__int128)src->bit0 + (__int128)(n_rows - 1) * src->row_stride_bits + span > end) {
            return fail(fn, "an element outside n_bytes: row " + std::to_string(n_rows - 1) + " ends beyond the source");
        }
    }
    if (samp_index)
        for (int64_t j = 0; j < n_samp_out; j++)
            if (samp_index[j] < 0 || samp_index[j] >= src_samp) return fail(fn, "an index outside the source: samp_index[" + std::to_string(j) + "]");
    if (snp_index)
        for (int64_t k = 0; k < n_snp_out; k++)
            if (snp_index[k] < 0 || snp_index[k] >= src_snp) return fail(fn, "an index outside the source: snp_index[" + std::to_string(k) + "]");
    return 0;
}

}  // namespace snpgpu

namespace {

// ms of: source copies to the device, copy kernel, gather kernel, transposition kernel; launches; source bytes copied; ms of the
// result's copy to the host; staging windows
thread_local double g_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

enum { T_H2D = 0, T_COPY = 1, T_GATHER = 2, T_TRANS = 3, T_D2H = 4 };

size_t stage_bytes() { return sel_stage_bytes(); }
// SNPGPU_SELECT_LDS_WORDS: a smaller LDS budget of the gather kernel (0: source rows stay in global memory), to test that path
int64_t lds_words()
{
    if (const char *e = getenv("SNPGPU_SELECT_LDS_WORDS")) return std::min<int64_t>(SEL_LDS_WORDS, std::max<int64_t>(0, atoll(e)));
    return SEL_LDS_WORDS;
}

inline int64_t row_start(const snpgpu_geno_src &s, int64_t r) { return s.bit0 + (s.row_bit ? s.row_bit[r] : r * s.row_stride_bits); }

template <class T> int upload(Call &c, const T *h, size_t n, T *&d)
{
    int rc = 0;
    DevBuf *b = c.bufs.get(sizeof(T) * std::max<size_t>(n, 1), rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(b->p, h, sizeof(T) * n, hipMemcpyHostToDevice, c.st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c.st.s));          // h may be a temporary of the caller
    d = (T *)b->p;
    return 0;
}

int timed_h2d(Call &c, void *dst, const void *src, size_t bytes)
{
    if (c.log.begin(T_H2D, c.st.s)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c.st.s));
    g_stats[5] += (double)bytes;
    return c.log.end(c.st.s);
}

// SNP rows -> SNP rows of one view: the copy kernel for the run of samples from s0, the gather kernel for a list
int run_major0(Call &c, const SelBits &v, const int32_t *d_srow, const int32_t *d_samp, int64_t s0, int64_t n_out, int64_t n_cols,
               int64_t n_rows_out, uint8_t *dst, SelRecode code)
{
    hipStream_t s = c.st.s;
    g_stats[4] += 1;
    if (d_samp)
        return c.log.begin(T_GATHER, s) || launch_geno_gather(s, v, d_srow, d_samp, n_out, n_cols, n_rows_out, lds_words(), dst, code) ||
               c.log.end(s);
    return c.log.begin(T_COPY, s) || launch_geno_copy(s, v, d_srow, s0, n_out, n_rows_out, dst, code) || c.log.end(s);
}

// output SNPs [k0, k1) as segments of consecutive source columns (relative to cmin), at most SEL_TW long
void build_segs(const int32_t *snp, int64_t k0, int64_t k1, int64_t cmin, std::vector<SelSeg> &out)
{
    out.clear();
    for (int64_t k = k0; k < k1;) {
        const int64_t c = snp ? snp[k] : k;
        int64_t len = 1;
        while (k + len < k1 && len < SEL_TW && (snp ? (int64_t)snp[k + len] : k + len) == c + len) len++;
        out.push_back({(int32_t)k, (int32_t)(c - cmin), (int32_t)len});
        k += len;
    }
}

// dsegs: a device table of at least segs.size() entries, owned by the caller; segs stays alive until the stream is synchronised
int run_transpose(Call &c, const SelBits &v, const int32_t *d_samp, const std::vector<SelSeg> &segs, SelSeg *dsegs, int64_t n_out,
                  uint8_t *dst, SelRecode code)
{
    hipStream_t s = c.st.s;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dsegs, segs.data(), sizeof(SelSeg) * segs.size(), hipMemcpyHostToDevice, s));
    g_stats[4] += 1;
    return c.log.begin(T_TRANS, s) || launch_geno_transpose(s, v, d_samp, dsegs, (int64_t)segs.size(), n_out, dst, code) || c.log.end(s);
}

// fn: the entry point's name in the error messages
int convert(const char *fn, const snpgpu_geno_src *src, int src_code, const int32_t *samp_index, int64_t n_samp_out,
            const int32_t *snp_index, int64_t n_snp_out, void *dst, int dst_major, int dst_code, int dst_mem, int device, void *stream)
{
    if (sel_check_args(fn, src, src_code, samp_index, n_samp_out, snp_index, n_snp_out, dst, dst_major, dst_code, dst_mem)) return 1;
    const int major = src->major;
    const int64_t n_rows = src->n_rows, n_cols = src->n_cols;

    // from here on in dst's terms: rows and columns (see the head of this file)
    const SelRecode code = sel_recode(src_code, dst_code);
    const bool cross = major != dst_major;
    const int32_t *row_index = dst_major ? samp_index : snp_index, *col_index = dst_major ? snp_index : samp_index;
    const int64_t n_row_out = dst_major ? n_samp_out : n_snp_out, n_col_out = dst_major ? n_snp_out : n_samp_out;

    for (double &x : g_stats) x = 0;
    Call c;
    if (c.open_on(fn, device, stream, {src->mem == SNPGPU_DEVICE ? src->bits : nullptr, dst_mem == SNPGPU_DEVICE ? (const void *)dst : nullptr}))
        return 1;
    hipStream_t s = c.st.s;

    const int64_t rb = (n_col_out + 3) / 4;
    HostOut od;
    if (od.open(c.bufs, dst, (size_t)n_row_out * (size_t)rb, dst_mem == SNPGPU_DEVICE ? SNPGPU_DEVICE : SNPGPU_HOST, false, s)) return 1;
    uint8_t *ddst = (uint8_t *)od.dev;

    // the samples: a run of consecutive ones (from run_s0; NULL = all) or a list
    int64_t run_s0 = col_index ? col_index[0] : 0;
    for (int64_t j = 1; col_index && j < n_col_out && run_s0 >= 0; j++)
        if (col_index[j] != col_index[0] + j) run_s0 = -1;
    const bool host_src = src->mem != SNPGPU_DEVICE;
    const uint8_t *bits = (const uint8_t *)src->bits;
    std::vector<SelSeg> segs;
    int rc = 0;
    // a host source that fits the staging size goes to the device as it is and is read there like a device source
    const uint8_t *dbits = host_src ? nullptr : bits;
    if (host_src && (size_t)src->n_bytes <= stage_bytes()) {
        DevBuf *raw = c.bufs.get((size_t)src->n_bytes + 32, rc);
        if (rc || timed_h2d(c, raw->p, bits, (size_t)src->n_bytes)) return 1;
        dbits = (const uint8_t *)raw->p;
    }
    int32_t *dsamp = nullptr;
    if (run_s0 < 0 && (dbits || !cross) && upload(c, col_index, (size_t)n_col_out, dsamp)) return 1;

    if (dbits) {
        const int64_t shift = (int64_t)((uintptr_t)dbits & 3);
        int64_t *drb = nullptr;
        if (src->row_bit && upload(c, src->row_bit, (size_t)n_rows, drb)) return 1;
        SelBits v = {(const uint32_t *)(dbits - shift), (shift + src->n_bytes + 3) / 4, src->bit0 + 8 * shift, src->row_stride_bits, drb};
        g_stats[7] = 1;
        if (!cross) {
            int32_t *dsrow = nullptr;
            if (row_index && upload(c, row_index, (size_t)n_row_out, dsrow)) return 1;
            if (run_major0(c, v, dsrow, dsamp, run_s0, n_col_out, n_cols, n_row_out, ddst, code)) return 1;
        } else {
            if (run_s0 > 0) { if (drb) v.row_bit += run_s0; else v.bit0 += run_s0 * v.stride; }
            build_segs(row_index, 0, n_row_out, 0, segs);
            DevBuf *dsegs = c.bufs.get(sizeof(SelSeg) * segs.size(), rc);
            if (rc || run_transpose(c, v, dsamp, segs, (SelSeg *)dsegs->p, n_col_out, ddst, code)) return 1;
        }
    } else if (!cross && !row_index && !src->row_bit) {
        // whole source rows in order, straight from the caller's memory
        const int64_t stride = src->row_stride_bits, span = 2 * n_cols, stage = (int64_t)stage_bytes();
        const int64_t per = stride > 0 ? std::max<int64_t>(1, (8 * stage - span - 14) / stride + 1) : n_rows;
        const int64_t m_max = std::min(per, n_rows);
        DevBuf *raw = c.bufs.get((size_t)(((m_max - 1) * stride + span + 14) / 8 + 36), rc);
        if (rc) return 1;
        for (int64_t k0 = 0; k0 < n_rows; k0 += per) {
            const int64_t m = std::min(per, n_rows - k0), start = row_start(*src, k0);
            const int64_t lo = start >> 3, hi = (start + (m - 1) * stride + span + 7) >> 3;
            if (timed_h2d(c, raw->p, bits + lo, (size_t)(hi - lo))) return 1;
            const SelBits v = {(const uint32_t *)raw->p, (hi - lo + 3) / 4, start - 8 * lo, stride, nullptr};
            if (run_major0(c, v, nullptr, dsamp, run_s0, n_col_out, n_cols, m, ddst + k0 * rb, code)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));               // the staging buffer is reused by the next window
            g_stats[7] += 1;
        }
    } else if (!cross) {
        // the selected source rows, gathered on the host: a dword-aligned segment and a phase per row
        const int64_t span = 2 * n_cols, stage = (int64_t)stage_bytes();
        std::vector<int64_t> rbit((size_t)n_row_out), win(1, 0);
        int64_t off = 0, max_off = 0;
        for (int64_t k = 0; k < n_row_out; k++) {
            const int64_t start = row_start(*src, row_index ? row_index[k] : k);
            const int64_t seg = (((start + span + 7) >> 3) - (start >> 3) + 3) & ~int64_t(3);
            if (off > 0 && off + seg > stage) { win.push_back(k); off = 0; }
            rbit[(size_t)k] = 8 * off + (start & 7);
            off += seg;
            max_off = std::max(max_off, off);
        }
        win.push_back(n_row_out);
        int64_t *drb = nullptr;
        if (upload(c, rbit.data(), rbit.size(), drb)) return 1;
        DevBuf *raw = c.bufs.get((size_t)max_off + 32, rc);
        if (rc) return 1;
        std::vector<uint8_t> hbuf((size_t)max_off, 0);
        for (size_t w = 0; w + 1 < win.size(); w++) {
            const int64_t k0 = win[w], k1 = win[w + 1];
            int64_t used = 0;
            for (int64_t k = k0; k < k1; k++) {
                const int64_t start = row_start(*src, row_index ? row_index[k] : k), lo = start >> 3, hi = (start + span + 7) >> 3;
                std::memcpy(hbuf.data() + (rbit[(size_t)k] >> 3), bits + lo, (size_t)(hi - lo));
                used = (rbit[(size_t)k] >> 3) + ((hi - lo + 3) & ~int64_t(3));
            }
            if (timed_h2d(c, raw->p, hbuf.data(), (size_t)used)) return 1;
            const SelBits v = {(const uint32_t *)raw->p, used / 4, 0, 0, drb + k0};
            if (run_major0(c, v, nullptr, dsamp, run_s0, n_col_out, n_cols, k1 - k0, ddst + k0 * rb, code)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
            g_stats[7] += 1;
        }
    } else {
        // sample rows from the host in windows of output SNPs: every selected sample's segment of the window's range of source
        // SNPs, gathered on the host with a phase per row, so that every window's output is whole rows of its SNPs
        const int64_t stage = (int64_t)stage_bytes();
        const auto col = [&](int64_t k) { return row_index ? (int64_t)row_index[k] : k; };
        const auto seg_max = [](int64_t ncol) { return (((2 * ncol + 14) >> 3) + 4) & ~int64_t(3); };
        struct Win { int64_t k0, k1, cmin, cmax; };
        std::vector<Win> wins;
        int64_t max_bytes = 0, max_snps = 0;
        for (int64_t k = 0; k < n_row_out;) {
            Win w = {k, k + 1, col(k), col(k)};
            while (w.k1 < n_row_out) {
                const int64_t lo = std::min(w.cmin, col(w.k1)), hi = std::max(w.cmax, col(w.k1));
                if (n_col_out * seg_max(hi - lo + 1) > stage) break;
                w.cmin = lo; w.cmax = hi; w.k1++;
            }
            max_bytes = std::max(max_bytes, n_col_out * seg_max(w.cmax - w.cmin + 1));
            max_snps = std::max(max_snps, w.k1 - w.k0);                 // a window has at most one segment per SNP
            wins.push_back(w);
            k = w.k1;
        }
        DevBuf *raw = c.bufs.get((size_t)max_bytes + 32, rc), *drb = c.bufs.get(sizeof(int64_t) * (size_t)n_col_out, rc);
        DevBuf *dsegs = c.bufs.get(sizeof(SelSeg) * (size_t)max_snps, rc);
        if (rc) return 1;
        std::vector<uint8_t> hbuf((size_t)max_bytes, 0);
        std::vector<int64_t> rbit((size_t)n_col_out);
        for (const Win &w : wins) {
            const int64_t span = 2 * (w.cmax - w.cmin + 1);
            int64_t off = 0;
            for (int64_t j = 0; j < n_col_out; j++) {
                const int64_t start = row_start(*src, col_index ? col_index[j] : j) + 2 * w.cmin, lo = start >> 3, hi = (start + span + 7) >> 3;
                std::memcpy(hbuf.data() + off, bits + lo, (size_t)(hi - lo));
                rbit[(size_t)j] = 8 * off + (start & 7);
                off += (hi - lo + 3) & ~int64_t(3);
            }
            if (timed_h2d(c, raw->p, hbuf.data(), (size_t)off)) return 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(drb->p, rbit.data(), sizeof(int64_t) * rbit.size(), hipMemcpyHostToDevice, s));
            const SelBits v = {(const uint32_t *)raw->p, off / 4, 0, 0, (const int64_t *)drb->p};
            build_segs(row_index, w.k0, w.k1, w.cmin, segs);
            if (run_transpose(c, v, nullptr, segs, (SelSeg *)dsegs->p, n_col_out, ddst, code)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
            g_stats[7] += 1;
        }
    }

    if (c.log.begin(T_D2H, s) || od.close(s) || c.log.end(s)) return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    if (c.log.sum_ms(T_H2D, &g_stats[0]) || c.log.sum_ms(T_COPY, &g_stats[1]) || c.log.sum_ms(T_GATHER, &g_stats[2]) ||
        c.log.sum_ms(T_TRANS, &g_stats[3]) || c.log.sum_ms(T_D2H, &g_stats[6]))
        return 1;
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_geno_select(const snpgpu_geno_src *src, const int32_t *samp_index, int64_t n_samp_out, const int32_t *snp_index,
                       int64_t n_snp_out, void *dst, int dst_mem, int device, void *stream)
{
    return convert("snpgpu_geno_select", src, SNPGPU_CODE_GDS, samp_index, n_samp_out, snp_index, n_snp_out, dst, 0, SNPGPU_CODE_GDS,
                   dst_mem, device, stream);
}

int snpgpu_geno_convert(const snpgpu_geno_src *src, int src_code, const int32_t *samp_index, int64_t n_samp_out,
                        const int32_t *snp_index, int64_t n_snp_out, void *dst, int dst_major, int dst_code, int dst_mem, int device,
                        void *stream)
{
    return convert("snpgpu_geno_convert", src, src_code, samp_index, n_samp_out, snp_index, n_snp_out, dst, dst_major, dst_code, dst_mem,
                   device, stream);
}

int snpgpu_geno_select_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_geno_select_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 8; k++) stats[k] = g_stats[k];
    return 0;
}

int snpgpu_geno_convert_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_geno_convert_stats: stats is NULL"); return 1; }
    return snpgpu_geno_select_stats(stats);
}

}  // extern "C"
