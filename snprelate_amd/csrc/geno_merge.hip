// C ABI of libsnpgpu, data sets side by side (include/snpgpu.h section 1o): the selected rectangles of several 2-bit genotype
// sources in one PACKED2 row per output SNP, part after part at whatever code offset the parts before it leave, flagged rows
// re-coded to the other allele -- the genotype side of snpgdsCombineGeno (R/AllUtilities.R:1525-1556) and of gnrStrandSwitch
// (src/SNPRelate.cpp:454-494).  Kernel: kernels_geno_merge.hip.
//
// The output goes in windows of rows whose staged bytes fit SNPGPU_MERGE_STAGE_BYTES (one window when nothing is staged).  Per
// window every part becomes something the splice kernel reads at bit0 + k * stride:
//   where it lies   a major 0 source without row_bit whose samples are a run of consecutive ones, in device memory -- or a host
//                   source that fits the staging size of snpgpu_geno_select, which this call copies to the device once.  The SNP
//                   list, if any, goes to the device as it is.
//   staged          everything else (a sample list, sample rows, row_bit, a host source beyond the staging size): the window's
//                   rectangle through snpgpu_geno_select into byte-aligned device rows, with all its layouts and host windows.
// All argument errors are found before any device is touched.
#include <vector>

#include "geno_select.h"
#include "host_util.h"

using namespace snpgpu;

namespace {

// ms of staging / select, ms of the splice kernel, its launches, windows, bytes written
thread_local double g_stats[5] = {0, 0, 0, 0, 0};

enum { T_STAGE = 0, T_SPLICE = 1 };
constexpr int64_t MERGE_SAMP_END = int64_t(1) << 30;

size_t merge_stage_bytes() { return env_bytes("SNPGPU_MERGE_STAGE_BYTES", sel_stage_bytes()); }

// what one part is for the length of the call
struct PartPlan {
    snpgpu_geno_src src;           // the caller's description, or that of the copy this call made on the device
    int64_t run_s0 = 0;            // the first sample of a run of consecutive samples, -1 = a list
    bool to_device = false;        // a host source that this call copies to the device
    bool direct = false;           // read where it lies
    int64_t rb = 0;                // bytes of a staged row
    DevBuf *stage = nullptr;
    const int32_t *d_srow = nullptr;
    const uint8_t *d_flip = nullptr;
};

template <class T> int upload(Call &c, const T *h, size_t n, const T *&d)
{
    int rc = 0;
    DevBuf *b = c.bufs.get(sizeof(T) * std::max<size_t>(n, 1), rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(b->p, h, sizeof(T) * n, hipMemcpyHostToDevice, c.st.s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c.st.s));          // h may be a temporary of the caller
    d = (const T *)b->p;
    return 0;
}

// the description of output rows [k0, k0 + nk) of a source that is taken in order (snp_index NULL)
snpgpu_geno_src window_of(const snpgpu_geno_src &s, int64_t k0, int64_t nk)
{
    snpgpu_geno_src w = s;
    if (s.major) { w.n_cols = nk; w.bit0 = s.bit0 + 2 * k0; return w; }
    w.n_rows = nk;
    if (s.row_bit) { w.row_bit = s.row_bit + k0; return w; }
    // only the bytes of these rows: a host source beyond the staging size is not copied more than once over the windows
    const int64_t start = s.bit0 + k0 * s.row_stride_bits, lo = start >> 3;
    w.bits = (const uint8_t *)s.bits + lo;
    w.bit0 = start - 8 * lo;
    w.n_bytes = ((start + (nk - 1) * s.row_stride_bits + 2 * s.n_cols + 7) >> 3) - lo;
    return w;
}

}  // namespace

extern "C" {

int snpgpu_geno_merge(const snpgpu_merge_part *parts, int n_parts, int64_t n_snp_out, void *rows, int device, void *stream)
{
    const char *fn = "snpgpu_geno_merge";
    if (!parts) return fail(fn, "NULL argument: parts is NULL");
    if (!rows) return fail(fn, "NULL argument: rows is NULL");
    if (n_parts < 1) return fail(fn, "invalid n_parts (at least one part)");
    int64_t N = 0;
    for (int i = 0; i < n_parts; i++) {
        const std::string name = std::string(fn) + ": part " + std::to_string(i);
        if (sel_check_args(name.c_str(), &parts[i].src, SNPGPU_CODE_GDS, parts[i].samp_index, parts[i].n_samp, parts[i].snp_index, n_snp_out,
                           rows, 0, SNPGPU_CODE_GDS, SNPGPU_DEVICE))
            return 1;
        N += parts[i].n_samp;                                 // each below 2^30: no overflow before the test
        if (N >= MERGE_SAMP_END) return fail(fn, "invalid number of samples (1 ... 2^30 - 1): the parts together hold more");
    }

    for (double &x : g_stats) x = 0;
    Call c;
    std::vector<const void *> dev_ptrs(1, rows);
    for (int i = 0; i < n_parts; i++)
        if (parts[i].src.mem == SNPGPU_DEVICE) dev_ptrs.push_back(parts[i].src.bits);
    if (c.open_on(fn, device, stream, dev_ptrs)) return 1;
    hipStream_t s = c.st.s;

    const int64_t rb = (N + 3) / 4;

    // ---- the parts: where each is read from --------------------------------------------------------------------------------------
    int rc = 0;
    if (c.log.begin(T_STAGE, s)) return 1;
    std::vector<PartPlan> plan((size_t)n_parts);
    std::vector<int32_t> off((size_t)n_parts + 1, 0);
    // a window holds the rows whose STAGED bytes fit the budget: parts read where they lie need none, and alone they make one window
    int64_t row_bytes = 0;
    for (int i = 0; i < n_parts; i++) {
        const snpgpu_merge_part &p = parts[i];
        PartPlan &q = plan[(size_t)i];
        q.src = p.src;
        q.rb = (p.n_samp + 3) / 4;
        off[(size_t)i + 1] = off[(size_t)i] + (int32_t)p.n_samp;
        q.run_s0 = p.samp_index ? p.samp_index[0] : 0;
        for (int64_t j = 1; p.samp_index && j < p.n_samp && q.run_s0 >= 0; j++)
            if (p.samp_index[j] != p.samp_index[0] + j) q.run_s0 = -1;
        q.to_device = p.src.mem != SNPGPU_DEVICE && (size_t)p.src.n_bytes <= sel_stage_bytes();
        q.direct = (q.to_device || p.src.mem == SNPGPU_DEVICE) && p.src.major == 0 && !p.src.row_bit && q.run_s0 >= 0;
        if (!q.direct) row_bytes += q.rb;
    }
    const int64_t W = row_bytes ? std::min(n_snp_out, std::max<int64_t>(1, (int64_t)merge_stage_bytes() / row_bytes)) : n_snp_out;
    for (int i = 0; i < n_parts; i++) {
        const snpgpu_merge_part &p = parts[i];
        PartPlan &q = plan[(size_t)i];
        if (q.to_device) {
            DevBuf *raw = c.bufs.get((size_t)p.src.n_bytes + 32, rc);
            if (rc) return 1;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(raw->p, p.src.bits, (size_t)p.src.n_bytes, hipMemcpyHostToDevice, s));
            q.src.bits = raw->p;
            q.src.mem = SNPGPU_DEVICE;
        }
        if (q.direct) {
            if (p.snp_index && upload(c, p.snp_index, (size_t)n_snp_out, q.d_srow)) return 1;
        } else {
            q.stage = c.bufs.get((size_t)(W * q.rb) + 36, rc);
            if (rc) return 1;
        }
        if (p.flip && upload(c, p.flip, (size_t)n_snp_out, q.d_flip)) return 1;
    }
    const int32_t *d_off = nullptr;
    if (upload(c, off.data(), off.size(), d_off)) return 1;
    DevBuf *d_desc = c.bufs.get(sizeof(SplicePart) * (size_t)n_parts, rc);
    if (rc || c.log.end(s)) return 1;

    // ---- the windows ----------------------------------------------------------------------------------------------------------------
    std::vector<SplicePart> desc((size_t)n_parts);
    for (int64_t k0 = 0; k0 < n_snp_out; k0 += W) {
        const int64_t nk = std::min(W, n_snp_out - k0);
        if (c.log.begin(T_STAGE, s)) return 1;
        for (int i = 0; i < n_parts; i++) {
            const snpgpu_merge_part &p = parts[i];
            const PartPlan &q = plan[(size_t)i];
            SplicePart &d = desc[(size_t)i];
            d.flip = q.d_flip ? q.d_flip + k0 : nullptr;
            d.srow = nullptr;
            if (q.direct) {
                const int64_t shift = (int64_t)((uintptr_t)q.src.bits & 3);
                d.w = (const uint32_t *)((const uint8_t *)q.src.bits - shift);
                d.n_words = (shift + q.src.n_bytes + 3) / 4;
                d.stride = q.src.row_stride_bits;
                d.bit0 = q.src.bit0 + 8 * shift + 2 * q.run_s0 + (q.d_srow ? 0 : k0 * d.stride);
                d.srow = q.d_srow ? q.d_srow + k0 : nullptr;
                continue;
            }
            const snpgpu_geno_src sub = (p.snp_index || nk == n_snp_out) ? q.src : window_of(q.src, k0, nk);
            if (snpgpu_geno_select(&sub, p.samp_index, p.n_samp, p.snp_index ? p.snp_index + k0 : nullptr, nk, q.stage->p, SNPGPU_DEVICE,
                                   device, s))
                return 1;
            d.w = (const uint32_t *)q.stage->p;
            d.n_words = (nk * q.rb + 3) / 4;
            d.bit0 = 0;
            d.stride = 8 * q.rb;
        }
        SNPGPU_HIP_CHECK(hipMemcpyAsync(d_desc->p, desc.data(), sizeof(SplicePart) * desc.size(), hipMemcpyHostToDevice, s));
        if (c.log.end(s)) return 1;
        if (c.log.begin(T_SPLICE, s) ||
            launch_geno_splice(s, (const SplicePart *)d_desc->p, d_off, n_parts, N, nk, (uint8_t *)rows + k0 * rb) || c.log.end(s))
            return 1;
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));            // the staging rows and the descriptions are reused by the next window
        g_stats[2] += 1;
        g_stats[3] += 1;
    }
    g_stats[4] = (double)n_snp_out * (double)rb;
    if (c.log.sum_ms(T_STAGE, &g_stats[0]) || c.log.sum_ms(T_SPLICE, &g_stats[1])) return 1;
    return 0;
}

int snpgpu_geno_merge_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_geno_merge_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 5; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
