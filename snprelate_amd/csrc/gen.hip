// C ABI of libsnpgpu, Oxford GEN text (include/snpgpu.h section 1p): snpgpu_gen_genotypes, the probability triples of indexed lines
// called to SNPGPU_GENO_PACKED2 rows on the device (kernels_gen.hip), and snpgpu_gen_line_host, one line read the way the
// reference reads it (gen_line.h, no HIP call): what settles a line the kernel flags.
//
// Text in device memory is parsed where it lies, in one launch.  Host text goes through one staging buffer in windows of whole
// lines, as snpgpu_vcf_genotypes stages its own: from the sixth column of a window's first line to the end of its last one, at
// most SNPGPU_TEXT_STAGE_BYTES.  All argument errors are found before any device is touched.
#include <cstdio>
#include <string>
#include <vector>

#include "gen.h"
#include "gen_line.h"
#include "host_util.h"

using namespace snpgpu;

namespace {

// ms of the text's copies to the device, ms of the kernel, launches, text bytes brought to the device or parsed in place, bytes
// of a chunk, of a lane's segment, of the halo
thread_local double g_stats[7] = {0, 0, 0, 0, (double)CHUNK_BYTES, (double)CHUNK_SEG, (double)CHUNK_HALO};

constexpr int64_t GEN_STAGE_BYTES = int64_t(256) << 20;
enum { T_H2D = 0, T_KERNEL = 1 };

int64_t stage_bytes()
{
    if (const char *e = getenv("SNPGPU_TEXT_STAGE_BYTES")) { if (atoll(e) > 0) return (int64_t)atoll(e); }
    return GEN_STAGE_BYTES;
}

}  // namespace

extern "C" {

int snpgpu_gen_genotypes(const void *text, int text_mem, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end,
                         int64_t n_lines, int64_t n_samp, double call_threshold, void *rows, int32_t *line_flags,
                         int64_t *line_cells, int device, void *stream)
{
    const char *fn = "snpgpu_gen_genotypes";
    if (!text) return fail(fn, "NULL argument: text is NULL");
    if (!cell_begin) return fail(fn, "NULL argument: cell_begin is NULL");
    if (!line_end) return fail(fn, "NULL argument: line_end is NULL");
    if (!rows) return fail(fn, "NULL argument: rows is NULL");
    if (!line_flags) return fail(fn, "NULL argument: line_flags is NULL");
    if (!line_cells) return fail(fn, "NULL argument: line_cells is NULL");
    if (text_mem != SNPGPU_HOST && text_mem != SNPGPU_DEVICE && text_mem != SNPGPU_HOST_PINNED) return fail(fn, "invalid text_mem");
    if (n_bytes < 1) return fail(fn, "invalid n_bytes");
    if (n_lines < 1 || n_lines >= (int64_t(1) << 31)) return fail(fn, "invalid number of lines (1 ... 2^31 - 1)");
    if (n_samp < 1 || n_samp >= (int64_t(1) << 30)) return fail(fn, "invalid number of samples (1 ... 2^30 - 1)");
    const int64_t stage = stage_bytes();
    std::vector<GenLine> lines((size_t)n_lines);
    for (int64_t i = 0; i < n_lines; i++) {
        if (cell_begin[i] < 0 || line_end[i] > n_bytes || cell_begin[i] > line_end[i])
            return fail(fn, "an offset outside n_bytes or cell_begin > line_end: line " + std::to_string(i));
        if (text_mem != SNPGPU_DEVICE && line_end[i] - cell_begin[i] > stage)
            return fail(fn, "a line longer than the " + std::to_string(stage) + " bytes of a chunk (SNPGPU_TEXT_STAGE_BYTES): line " +
                                std::to_string(i));
        lines[(size_t)i] = {cell_begin[i], line_end[i]};
    }

    for (int k = 0; k < 4; k++) g_stats[k] = 0;
    Call c;
    if (c.open(fn, device, true, stream)) return 1;
    hipStream_t s = c.st.s;
    if (stream) {
        hipDevice_t d = -1;
        if (hipStreamGetDevice(s, &d) == hipSuccess && (int)d != device) return fail(fn, "the stream belongs to another device");
    }
    for (const void *p : {text_mem == SNPGPU_DEVICE ? text : nullptr, (const void *)rows}) {
        hipPointerAttribute_t a;
        if (!p) continue;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (a.type == hipMemoryTypeDevice && a.device != device) return fail(fn, "a device pointer of another device");
    }

    const int64_t rb = (n_samp + 3) / 4;
    int rc = 0;
    DevBuf *dlines = c.bufs.get(sizeof(GenLine) * (size_t)n_lines, rc);
    DevBuf *dflags = c.bufs.get(sizeof(int32_t) * (size_t)n_lines, rc), *dcells = c.bufs.get(sizeof(int64_t) * (size_t)n_lines, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dlines->p, lines.data(), sizeof(GenLine) * (size_t)n_lines, hipMemcpyHostToDevice, s));
    const auto launch = [&](const TextView &t, int64_t i0, int64_t i1) {
        g_stats[2] += 1;
        return c.log.begin(T_KERNEL, s) ||
               launch_gen_parse(s, t, (const GenLine *)dlines->p + i0, i1 - i0, n_samp, call_threshold, (uint8_t *)rows + i0 * rb,
                                (int32_t *)dflags->p + i0, (int64_t *)dcells->p + i0) ||
               c.log.end(s);
    };

    if (text_mem == SNPGPU_DEVICE) {
        const int64_t shift = (int64_t)((uintptr_t)text & 15);
        const TextView t = {(const uint32_t *)((const uint8_t *)text - shift), shift >> 2, (shift + n_bytes + 3) >> 2, shift};
        g_stats[3] = (double)n_bytes;
        if (launch(t, 0, n_lines)) return 1;
    } else {
        // windows of whole lines: [i0, i1) with the bytes [lo, hi) that hold their cells
        struct Win { int64_t i0, i1, lo, hi; };
        std::vector<Win> wins;
        int64_t max_bytes = 0;
        for (int64_t i = 0; i < n_lines;) {
            Win w = {i, i + 1, cell_begin[i], line_end[i]};
            while (w.i1 < n_lines) {
                const int64_t lo = std::min(w.lo, cell_begin[w.i1]), hi = std::max(w.hi, line_end[w.i1]);
                if (hi - lo > stage) break;
                w.lo = lo; w.hi = hi; w.i1++;
            }
            max_bytes = std::max(max_bytes, w.hi - w.lo);
            wins.push_back(w);
            i = w.i1;
        }
        DevBuf *raw = c.bufs.get((size_t)max_bytes + 32, rc);
        if (rc) return 1;
        for (const Win &w : wins) {
            const int64_t nb = w.hi - w.lo;
            if (nb > 0) {
                if (c.log.begin(T_H2D, s)) return 1;
                SNPGPU_HIP_CHECK(hipMemcpyAsync(raw->p, (const uint8_t *)text + w.lo, (size_t)nb, hipMemcpyHostToDevice, s));
                if (c.log.end(s)) return 1;
            }
            g_stats[3] += (double)nb;
            const TextView t = {(const uint32_t *)raw->p, 0, (nb + 3) >> 2, -w.lo};
            if (launch(t, w.i0, w.i1)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));               // the staging buffer is reused by the next window
        }
    }
    SNPGPU_HIP_CHECK(hipMemcpyAsync(line_flags, dflags->p, sizeof(int32_t) * (size_t)n_lines, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(line_cells, dcells->p, sizeof(int64_t) * (size_t)n_lines, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    if (c.log.sum_ms(T_H2D, &g_stats[0]) || c.log.sum_ms(T_KERNEL, &g_stats[1])) return 1;
    return 0;
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
