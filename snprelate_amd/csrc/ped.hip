// C ABI of libsnpgpu, PLINK .ped text in (include/snpgpu.h section 1n): snpgpu_ped_tokens, the allele tokens of indexed lines as a
// token matrix in device memory; snpgpu_ped_census, their counts per SNP; snpgpu_ped_codes, the matrix against the reference
// alleles as SNPGPU_GENO_PACKED2 sample rows (kernels_ped.hip).  The three calls are the two sweeps of gnrParsePED
// (src/ConvToGDS.cpp:1175-1361): tokens + census over every window of the text, the host's choice of the reference alleles, tokens +
// codes over every window again.  All argument errors are found before any device is touched.
#include <vector>

#include "ped.h"
#include "text_host.h"

using namespace snpgpu;

namespace {

// ms of the last tokens / census / codes kernel, launches of the last call, text bytes of the last snpgpu_ped_tokens, bytes of a
// chunk, of a lane's segment, of the halo
thread_local double g_stats[8] = {0, 0, 0, 0, 0, (double)CHUNK_BYTES, (double)CHUNK_SEG, (double)CHUNK_HALO};

int check_dims_ped(const char *fn, int64_t n_lines, int64_t n_snp)
{
    if (n_lines < 1 || n_lines >= (int64_t(1) << 31)) return fail(fn, "invalid number of lines (1 ... 2^31 - 1)");
    if (n_snp < 1 || n_snp >= (int64_t(1) << 30)) return fail(fn, "invalid number of SNPs (1 ... 2^30 - 1)");
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_ped_tokens(const void *text, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end, int64_t n_lines,
                      int64_t n_snp, void *tokens, int32_t *line_flags, int64_t *line_tokens, int device, void *stream)
{
    const char *fn = "snpgpu_ped_tokens";
    if (!text) return fail(fn, "NULL argument: text is NULL");
    if (!cell_begin) return fail(fn, "NULL argument: cell_begin is NULL");
    if (!line_end) return fail(fn, "NULL argument: line_end is NULL");
    if (!tokens) return fail(fn, "NULL argument: tokens is NULL");
    if (!line_flags) return fail(fn, "NULL argument: line_flags is NULL");
    if (!line_tokens) return fail(fn, "NULL argument: line_tokens is NULL");
    if (n_bytes < 1) return fail(fn, "invalid n_bytes");
    if (check_dims_ped(fn, n_lines, n_snp)) return 1;
    std::vector<PedLine> lines((size_t)n_lines);
    for (int64_t i = 0; i < n_lines; i++) {
        if (cell_begin[i] < 0 || line_end[i] > n_bytes || cell_begin[i] > line_end[i])
            return fail(fn, "an offset outside n_bytes or cell_begin > line_end: line " + std::to_string(i));
        lines[(size_t)i] = {cell_begin[i], line_end[i]};
    }

    Call c;
    if (c.open_on(fn, device, stream, {text, (const void *)tokens})) return 1;
    hipStream_t s = c.st.s;
    int rc = 0;
    DevBuf *dlines = c.bufs.get(sizeof(PedLine) * (size_t)n_lines, rc);
    DevBuf *dflags = c.bufs.get(sizeof(int32_t) * (size_t)n_lines, rc), *dcounts = c.bufs.get(sizeof(int64_t) * (size_t)n_lines, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dlines->p, lines.data(), sizeof(PedLine) * (size_t)n_lines, hipMemcpyHostToDevice, s));
    if (c.log.begin(0, s) ||
        launch_ped_tokens(s, text_view_in_place(text, n_bytes), (const PedLine *)dlines->p, n_lines, 2 * n_snp, (uint8_t *)tokens, (int32_t *)dflags->p, (int64_t *)dcounts->p) ||
        c.log.end(s))
        return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(line_flags, dflags->p, sizeof(int32_t) * (size_t)n_lines, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(line_tokens, dcounts->p, sizeof(int64_t) * (size_t)n_lines, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    g_stats[3] = 1;
    g_stats[4] = (double)n_bytes;
    return c.log.sum_ms(0, &g_stats[0]);
}

int snpgpu_ped_census(const void *tokens, const int32_t *line_flags, int64_t n_lines, int64_t n_snp, void *table, int device, void *stream)
{
    const char *fn = "snpgpu_ped_census";
    if (!tokens) return fail(fn, "NULL argument: tokens is NULL");
    if (!line_flags) return fail(fn, "NULL argument: line_flags is NULL");
    if (!table) return fail(fn, "NULL argument: table is NULL");
    if (check_dims_ped(fn, n_lines, n_snp)) return 1;
    Call c;
    if (c.open_on(fn, device, stream, {tokens, (const void *)table})) return 1;
    hipStream_t s = c.st.s;
    int rc = 0;
    DevBuf *dflags = c.bufs.get(sizeof(int32_t) * (size_t)n_lines, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dflags->p, line_flags, sizeof(int32_t) * (size_t)n_lines, hipMemcpyHostToDevice, s));
    if (c.log.begin(1, s) || launch_ped_census(s, (const uint8_t *)tokens, (const int32_t *)dflags->p, n_lines, n_snp, (uint32_t *)table) ||
        c.log.end(s))
        return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    g_stats[3] = 1;
    return c.log.sum_ms(1, &g_stats[1]);
}

int snpgpu_ped_codes(const void *tokens, int64_t n_lines, int64_t n_snp, const uint8_t *ref, void *rows, int device, void *stream)
{
    const char *fn = "snpgpu_ped_codes";
    if (!tokens) return fail(fn, "NULL argument: tokens is NULL");
    if (!ref) return fail(fn, "NULL argument: ref is NULL");
    if (!rows) return fail(fn, "NULL argument: rows is NULL");
    if (check_dims_ped(fn, n_lines, n_snp)) return 1;
    Call c;
    if (c.open_on(fn, device, stream, {tokens, (const void *)rows})) return 1;
    hipStream_t s = c.st.s;
    int rc = 0;
    DevBuf *dref = c.bufs.get((size_t)n_snp, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dref->p, ref, (size_t)n_snp, hipMemcpyHostToDevice, s));
    if (c.log.begin(2, s) || launch_ped_codes(s, (const uint8_t *)tokens, (const uint8_t *)dref->p, n_lines, n_snp, (uint8_t *)rows) ||
        c.log.end(s))
        return 1;
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    g_stats[3] = 1;
    return c.log.sum_ms(2, &g_stats[2]);
}

int snpgpu_ped_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_ped_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 8; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
