// C ABI of libsnpgpu, Oxford GEN text (include/snpgpu.h section 1p): snpgpu_gen_genotypes, the probability triples of indexed lines
// called to SNPGPU_GENO_PACKED2 rows on the device (kernels_gen.hip), and snpgpu_gen_line_host, one line read the way the
// reference reads it (gen_line.h, no HIP call): what settles a line the kernel flags.
//
// The call itself is text_host.h's: text in device memory is parsed where it lies, host text goes through one staging buffer in
// windows of whole lines, from the sixth column of a window's first line to the end of its last one, at most
// SNPGPU_TEXT_STAGE_BYTES: a longer line is refused.  All argument errors are found before any device is touched.
#include <cstdio>
#include <string>
#include <vector>

#include "gen.h"
#include "gen_line.h"
#include "text_host.h"

using namespace snpgpu;

namespace {

// ms of the text's copies to the device, ms of the kernel, launches, text bytes brought to the device or parsed in place, bytes
// of a chunk, of a lane's segment, of the halo
thread_local double g_stats[7] = {0, 0, 0, 0, (double)CHUNK_BYTES, (double)CHUNK_SEG, (double)CHUNK_HALO};

constexpr size_t GEN_STAGE_BYTES = size_t(256) << 20;

}  // namespace

extern "C" {

int snpgpu_gen_genotypes(const void *text, int text_mem, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end,
                         int64_t n_lines, int64_t n_samp, double call_threshold, void *rows, int32_t *line_flags,
                         int64_t *line_cells, int device, void *stream)
{
    const char *fn = "snpgpu_gen_genotypes";
    const TextArgs a = {text, text_mem, n_bytes, cell_begin, line_end, n_lines, n_samp, rows, line_flags, line_cells, device, stream};
    if (check_text_args(fn, a, {})) return 1;
    const int64_t stage = (int64_t)env_bytes("SNPGPU_TEXT_STAGE_BYTES", GEN_STAGE_BYTES);
    std::vector<GenLine> lines((size_t)n_lines);
    for (int64_t i = 0; i < n_lines; i++) {
        if (check_text_line(fn, a, i)) return 1;
        if (text_mem != SNPGPU_DEVICE && line_end[i] - cell_begin[i] > stage)
            return fail(fn, "a line longer than the " + std::to_string(stage) + " bytes of a chunk (SNPGPU_TEXT_STAGE_BYTES): line " +
                                std::to_string(i));
        lines[(size_t)i] = {cell_begin[i], line_end[i]};
    }

    const int64_t rb = (n_samp + 3) / 4;
    return parse_text_lines(fn, a, lines, stage, g_stats,
                            [&](hipStream_t s, const TextView &t, const GenLine *l, int64_t i0, int64_t n, int32_t *flags, int64_t *cells) {
                                return launch_gen_parse(s, t, l, n, n_samp, call_threshold, (uint8_t *)rows + i0 * rb, flags, cells);
                            });
}

int snpgpu_gen_line_host(const char *line, int64_t n_bytes, int64_t n_samp, double call_threshold, uint8_t *codes, int64_t *column,
                         char *message, int64_t message_bytes)
{
    const char *fn = "snpgpu_gen_line_host";
    if (!line) return fail(fn, "NULL argument: line is NULL");
    if (!codes) return fail(fn, "NULL argument: codes is NULL");
    if (!column) return fail(fn, "NULL argument: column is NULL");
    if (!message) return fail(fn, "NULL argument: message is NULL");
    if (n_bytes < 0) return fail(fn, "invalid n_bytes");
    if (n_samp < 1 || n_samp >= (int64_t(1) << 30)) return fail(fn, "invalid number of samples (1 ... 2^30 - 1)");
    if (message_bytes < 1) return fail(fn, "invalid message_bytes");

    std::string msg;
    *column = gen_line_codes(line, n_bytes, n_samp, call_threshold, codes, msg);
    snprintf(message, (size_t)message_bytes, "%s", msg.c_str());
    return 0;
}

int snpgpu_gen_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_gen_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 7; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
