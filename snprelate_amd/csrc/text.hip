// C ABI of libsnpgpu, text out (include/snpgpu.h section 1m): snpgpu_text_render, device rows of SNPGPU_GENO_PACKED2 codes as
// lines of text in device memory (kernels_text.hip).  The buffer is a file's bytes verbatim: the caller appends it to the file.
//
// Fixed-width formats need no device pass to be sized: the line offsets are arithmetic.  With alleles of several lengths a first
// launch gives every line's length, the host turns the lengths into offsets, a second launch writes.  The caller's pools (line
// prefixes, alleles) are copied to the device for the length of the call.  All argument errors are found before any device is
// touched.
#include <vector>

#include "host_util.h"
#include "text.h"

using namespace snpgpu;

namespace {

// ms of the length pass, ms of the write pass, launches, bytes written, bytes of a lane's segment, columns of a tile
thread_local double g_stats[6] = {0, 0, 0, 0, (double)TEXT_SEG, (double)TEXT_TILE};
enum { T_LENGTHS = 0, T_WRITE = 1 };

}  // namespace

extern "C" {

int snpgpu_text_render(const void *rows, int64_t n_rows, int64_t n_cols, int format, const char *allele_pool,
                       const int64_t *allele_off, const char *prefix_pool, const int64_t *prefix_off, void *text, int64_t *line_off,
                       int device, void *stream)
{
    const char *fn = "snpgpu_text_render";
    if (!rows) return fail(fn, "NULL argument: rows is NULL");
    if (!line_off) return fail(fn, "NULL argument: line_off is NULL");
    if (format != SNPGPU_TEXT_DIGIT && format != SNPGPU_TEXT_PED_AB && format != SNPGPU_TEXT_PED_12 && format != SNPGPU_TEXT_PED_ALLELE)
        return fail(fn, "invalid format");
    if (n_cols < 1 || n_cols >= (int64_t(1) << 30)) return fail(fn, "invalid number of columns (1 ... 2^30 - 1)");
    if (n_rows < 1 || n_rows >= (int64_t(1) << 31)) return fail(fn, "invalid number of rows (1 ... 2^31 - 1)");
    const bool alleles = format == SNPGPU_TEXT_PED_ALLELE;
    bool one_byte = true;
    if (alleles) {
        if (!allele_pool) return fail(fn, "NULL argument: allele_pool is NULL");
        if (!allele_off) return fail(fn, "NULL argument: allele_off is NULL");
        if (allele_off[0] < 0) return fail(fn, "allele_off is not ascending: a negative offset");
        for (int64_t i = 0; i < 2 * n_cols; i++) {
            const int64_t l = allele_off[i + 1] - allele_off[i];
            if (l < 1) return fail(fn, "allele_off is not ascending (an empty allele is written \"0\"): allele " + std::to_string(i));
            one_byte = one_byte && l == 1;
        }
    }
    if ((prefix_pool == nullptr) != (prefix_off == nullptr)) return fail(fn, "NULL argument: prefix_pool and prefix_off go together");
    if (prefix_off) {
        if (prefix_off[0] < 0) return fail(fn, "prefix_off is not ascending: a negative offset");
        for (int64_t i = 0; i < n_rows; i++)
            if (prefix_off[i + 1] < prefix_off[i]) return fail(fn, "prefix_off is not ascending: row " + std::to_string(i));
    }

    for (int k = 0; k < 4; k++) g_stats[k] = 0;
    const bool fixed = !alleles || one_byte;
    if (fixed) {
        const int64_t line = (format == SNPGPU_TEXT_DIGIT ? n_cols : 4 * n_cols) + 1;
        for (int64_t i = 0; i <= n_rows; i++) line_off[i] = i * line + (prefix_off ? prefix_off[i] - prefix_off[0] : 0);
        if (!text) return 0;
    }

    Call c;
    if (c.open_on(fn, device, stream, {rows, (const void *)text})) return 1;
    hipStream_t s = c.st.s;

    // the caller's pools on the device, offsets relative to the copies
    int rc = 0;
    const int64_t pre_bytes = prefix_off ? prefix_off[n_rows] - prefix_off[0] : 0;
    const int64_t al_bytes = alleles ? allele_off[2 * n_cols] - allele_off[0] : 0;
    DevBuf *dpre = prefix_off ? c.bufs.get((size_t)pre_bytes + 16, rc) : nullptr;
    DevBuf *dpre_off = prefix_off ? c.bufs.get(sizeof(int64_t) * (size_t)(n_rows + 1), rc) : nullptr;
    DevBuf *dal = alleles ? c.bufs.get((size_t)al_bytes + 16, rc) : nullptr;
    DevBuf *dal_off = alleles && !fixed ? c.bufs.get(sizeof(int64_t) * (size_t)(2 * n_cols + 1), rc) : nullptr;
    if (rc) return 1;
    std::vector<int64_t> pre_rel, al_rel;
    if (prefix_off) {
        pre_rel.resize((size_t)n_rows + 1);
        for (int64_t i = 0; i <= n_rows; i++) pre_rel[(size_t)i] = prefix_off[i] - prefix_off[0];
        if (pre_bytes) SNPGPU_HIP_CHECK(hipMemcpyAsync(dpre->p, prefix_pool + prefix_off[0], (size_t)pre_bytes, hipMemcpyHostToDevice, s));
        SNPGPU_HIP_CHECK(hipMemcpyAsync(dpre_off->p, pre_rel.data(), sizeof(int64_t) * pre_rel.size(), hipMemcpyHostToDevice, s));
    }
    if (alleles) {
        SNPGPU_HIP_CHECK(hipMemcpyAsync(dal->p, allele_pool + allele_off[0], (size_t)al_bytes, hipMemcpyHostToDevice, s));
        if (!fixed) {
            al_rel.resize((size_t)(2 * n_cols) + 1);
            for (int64_t i = 0; i <= 2 * n_cols; i++) al_rel[(size_t)i] = allele_off[i] - allele_off[0];
            SNPGPU_HIP_CHECK(hipMemcpyAsync(dal_off->p, al_rel.data(), sizeof(int64_t) * al_rel.size(), hipMemcpyHostToDevice, s));
        }
    }

    const int64_t rshift = (int64_t)((uintptr_t)rows & 3), tshift = (int64_t)((uintptr_t)text & (TEXT_SEG - 1));
    TextJob j;
    j.rows_w = (const uint32_t *)((const uint8_t *)rows - rshift);
    j.rows_shift = rshift;
    j.rb = (n_cols + 3) / 4;
    j.n_cols = n_cols;
    j.text_al = text ? (uint8_t *)text - tshift : nullptr;
    j.text_shift = tshift;
    j.pre_pool = dpre ? (const uint8_t *)dpre->p : nullptr;
    j.pre_off = dpre_off ? (const int64_t *)dpre_off->p : nullptr;
    j.al_pool = dal ? (const uint8_t *)dal->p : nullptr;
    j.al_off = dal_off ? (const int64_t *)dal_off->p : nullptr;
    j.format = format;

    if (fixed) {
        g_stats[2] += 1;
        if (c.log.begin(T_WRITE, s) || launch_text_fixed(s, j, n_rows) || c.log.end(s)) return 1;
    } else {
        DevBuf *dlen = c.bufs.get(sizeof(int64_t) * (size_t)(n_rows + 1), rc);
        if (rc) return 1;
        g_stats[2] += 1;
        if (c.log.begin(T_LENGTHS, s) || launch_text_lengths(s, j, n_rows, (int64_t *)dlen->p) || c.log.end(s)) return 1;
        SNPGPU_HIP_CHECK(hipMemcpyAsync(line_off + 1, dlen->p, sizeof(int64_t) * (size_t)n_rows, hipMemcpyDeviceToHost, s));
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
        line_off[0] = 0;
        for (int64_t i = 0; i < n_rows; i++) line_off[i + 1] += line_off[i];
        if (text) {
            SNPGPU_HIP_CHECK(hipMemcpyAsync(dlen->p, line_off, sizeof(int64_t) * (size_t)(n_rows + 1), hipMemcpyHostToDevice, s));
            g_stats[2] += 1;
            if (c.log.begin(T_WRITE, s) || launch_text_variable(s, j, n_rows, (const int64_t *)dlen->p) || c.log.end(s)) return 1;
        }
    }
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    if (text) g_stats[3] = (double)line_off[n_rows];
    if (c.log.sum_ms(T_LENGTHS, &g_stats[0]) || c.log.sum_ms(T_WRITE, &g_stats[1])) return 1;
    return 0;
}

int snpgpu_text_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_text_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 6; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
