// C ABI of libsnpgpu, VCF text (include/snpgpu.h section 1l): snpgpu_vcf_index, the line index of a buffer of data lines
// (vcf_index.h, no HIP call), and snpgpu_vcf_genotypes, the sample cells of indexed lines reduced to SNPGPU_GENO_PACKED2 rows on
// the device (kernels_vcf.hip).  The file's own bytes go to the device; nothing per cell exists outside the rows.
//
// The call itself is text_host.h's: text in device memory is parsed where it lies, host text goes through one staging buffer in
// windows of whole lines, from the first sample cell of a window's first line to the end of its last one, at most
// SNPGPU_VCF_STAGE_BYTES unless one line alone is longer.  All argument errors are found before any device is touched.
#include <vector>

#include "text_host.h"
#include "vcf.h"
#include "vcf_index.h"

using namespace snpgpu;

namespace {

// ms of the text's copies to the device, ms of the kernel, launches, text bytes brought to the device or parsed in place, bytes
// of a chunk, of a lane's segment, of the halo
thread_local double g_stats[7] = {0, 0, 0, 0, (double)CHUNK_BYTES, (double)CHUNK_SEG, (double)CHUNK_HALO};

constexpr size_t VCF_STAGE_BYTES = size_t(256) << 20;

}  // namespace

extern "C" {

int snpgpu_vcf_index(const char *buf, int64_t n_bytes, int final, int64_t line_base, int64_t max_lines, int64_t *col_begin,
                     int64_t *line_end, int64_t *n_lines, int64_t *consumed)
{
    const char *fn = "snpgpu_vcf_index";
    if (!buf) return fail(fn, "NULL argument: buf is NULL");
    if (!col_begin) return fail(fn, "NULL argument: col_begin is NULL");
    if (!line_end) return fail(fn, "NULL argument: line_end is NULL");
    if (!n_lines) return fail(fn, "NULL argument: n_lines is NULL");
    if (!consumed) return fail(fn, "NULL argument: consumed is NULL");
    if (n_bytes < 0 || max_lines < 0 || line_base < 0) return fail(fn, "negative n_bytes, max_lines or line_base");
    const std::string err = vcf_index_lines(buf, n_bytes, final != 0, line_base, max_lines, col_begin, line_end, n_lines, consumed);
    return err.empty() ? 0 : fail(fn, err);
}

int snpgpu_vcf_genotypes(const void *text, int text_mem, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end,
                         const int32_t *num_allele, const int32_t *ref_index, int64_t n_lines, int64_t n_samp, void *rows,
                         int32_t *line_flags, int64_t *line_cells, int device, void *stream)
{
    const char *fn = "snpgpu_vcf_genotypes";
    const TextArgs a = {text, text_mem, n_bytes, cell_begin, line_end, n_lines, n_samp, rows, line_flags, line_cells, device, stream};
    if (check_text_args(fn, a, {{"num_allele", num_allele}, {"ref_index", ref_index}})) return 1;
    std::vector<VcfLine> lines((size_t)n_lines);
    for (int64_t i = 0; i < n_lines; i++) {
        if (check_text_line(fn, a, i)) return 1;
        if (num_allele[i] < 1) return fail(fn, "invalid num_allele: line " + std::to_string(i));
        if (ref_index[i] < -1) return fail(fn, "invalid ref_index: line " + std::to_string(i));
        lines[(size_t)i] = {cell_begin[i], line_end[i], num_allele[i], ref_index[i]};
    }

    const int64_t rb = (n_samp + 3) / 4;
    return parse_text_lines(fn, a, lines, (int64_t)env_bytes("SNPGPU_VCF_STAGE_BYTES", VCF_STAGE_BYTES), g_stats,
                            [&](hipStream_t s, const TextView &t, const VcfLine *l, int64_t i0, int64_t n, int32_t *flags, int64_t *cells) {
                                return launch_vcf_parse(s, t, l, n, n_samp, (uint8_t *)rows + i0 * rb, flags, cells);
                            });
}

int snpgpu_vcf_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_vcf_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 7; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
