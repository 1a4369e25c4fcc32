// Host layer of the text parsers (vcf.hip, gen.hip, ped.hip) on top of host_util.h: the view of text that is parsed where it
// lies, and what snpgpu_vcf_genotypes and snpgpu_gen_genotypes share from their argument checks to their return.  A format adds
// its own checks, its line structs and its launch.
#pragma once
#include <initializer_list>

#include "host_util.h"
#include "text_chunk.h"
#include "text_windows.h"

namespace snpgpu {

// n_bytes of text in device memory at any alignment, as the kernels read it: offset p is byte p of the text
inline TextView text_view_in_place(const void *ptr, int64_t n_bytes)
{
    const int64_t shift = (int64_t)((uintptr_t)ptr & 15);
    return {(const uint32_t *)((const uint8_t *)ptr - shift), shift >> 2, (shift + n_bytes + 3) >> 2, shift};
}

// the arguments the two calls have in common (include/snpgpu.h sections 1l and 1p)
struct TextArgs {
    const void *text;
    int text_mem;
    int64_t n_bytes;
    const int64_t *cell_begin, *line_end;
    int64_t n_lines, n_samp;
    void *rows;
    int32_t *line_flags;
    int64_t *line_cells;
    int device;
    void *stream;
};
struct NamedPtr { const char *name; const void *p; };

// Everything but the lines (no HIP call).  extra: the format's own host arrays, which stand between line_end and rows in its
// argument list and in the order of its refusals.
inline int check_text_args(const char *fn, const TextArgs &a, std::initializer_list<NamedPtr> extra)
{
    const auto null = [&](const NamedPtr &x) { return x.p ? 0 : fail(fn, std::string("NULL argument: ") + x.name + " is NULL"); };
    const NamedPtr front[] = {{"text", a.text}, {"cell_begin", a.cell_begin}, {"line_end", a.line_end}};
    const NamedPtr back[] = {{"rows", a.rows}, {"line_flags", a.line_flags}, {"line_cells", a.line_cells}};
    for (const NamedPtr &x : front) if (null(x)) return 1;
    for (const NamedPtr &x : extra) if (null(x)) return 1;
    for (const NamedPtr &x : back) if (null(x)) return 1;
    if (a.text_mem != SNPGPU_HOST && a.text_mem != SNPGPU_DEVICE && a.text_mem != SNPGPU_HOST_PINNED) return fail(fn, "invalid text_mem");
    if (a.n_bytes < 1) return fail(fn, "invalid n_bytes");
    if (a.n_lines < 1 || a.n_lines >= (int64_t(1) << 31)) return fail(fn, "invalid number of lines (1 ... 2^31 - 1)");
    if (a.n_samp < 1 || a.n_samp >= (int64_t(1) << 30)) return fail(fn, "invalid number of samples (1 ... 2^30 - 1)");
    return 0;
}

// line i lies inside the text: the first check of a line, in front of the format's own
inline int check_text_line(const char *fn, const TextArgs &a, int64_t i)
{
    if (a.cell_begin[i] < 0 || a.line_end[i] > a.n_bytes || a.cell_begin[i] > a.line_end[i])
        return fail(fn, "an offset outside n_bytes or cell_begin > line_end: line " + std::to_string(i));
    return 0;
}

enum { T_TEXT_H2D = 0, T_TEXT_KERNEL = 1 };

// The checked call on the device.  Text in device memory is parsed where it lies, in one launch.  Host text goes through one
// staging buffer in windows of whole lines (text_windows.h), at most `stage` bytes unless one line alone is longer.
// launch(stream, text view, the lines' descriptions, i0, n, flags, cells): the format's kernel over the n lines from i0, whose
// descriptions, flags and cell counts stand at the three device pointers.
// stats: ms of the text's copies to the device, ms of the kernel, launches, text bytes brought to the device or parsed in place.
template <class Line, class Launch>
int parse_text_lines(const char *fn, const TextArgs &a, const std::vector<Line> &lines, int64_t stage, double *stats, Launch launch)
{
    for (int k = 0; k < 4; k++) stats[k] = 0;
    Call c;
    if (c.open_on(fn, a.device, a.stream, {a.text_mem == SNPGPU_DEVICE ? a.text : nullptr, (const void *)a.rows})) return 1;
    hipStream_t s = c.st.s;

    const size_t n_lines = (size_t)a.n_lines;
    int rc = 0;
    DevBuf *dlines = c.bufs.get(sizeof(Line) * n_lines, rc);
    DevBuf *dflags = c.bufs.get(sizeof(int32_t) * n_lines, rc), *dcells = c.bufs.get(sizeof(int64_t) * n_lines, rc);
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dlines->p, lines.data(), sizeof(Line) * n_lines, hipMemcpyHostToDevice, s));
    const auto run = [&](const TextView &t, int64_t i0, int64_t i1) {
        stats[2] += 1;
        return c.log.begin(T_TEXT_KERNEL, s) ||
               launch(s, t, (const Line *)dlines->p + i0, i0, i1 - i0, (int32_t *)dflags->p + i0, (int64_t *)dcells->p + i0) || c.log.end(s);
    };

    if (a.text_mem == SNPGPU_DEVICE) {
        stats[3] = (double)a.n_bytes;
        if (run(text_view_in_place(a.text, a.n_bytes), 0, a.n_lines)) return 1;
    } else {
        int64_t max_bytes = 0;
        const std::vector<TextWindow> wins = plan_text_windows(a.cell_begin, a.line_end, a.n_lines, stage, &max_bytes);
        DevBuf *raw = c.bufs.get((size_t)max_bytes + 32, rc);
        if (rc) return 1;
        for (const TextWindow &w : wins) {
            const int64_t nb = w.hi - w.lo;
            if (nb > 0) {
                if (c.log.begin(T_TEXT_H2D, s)) return 1;
                SNPGPU_HIP_CHECK(hipMemcpyAsync(raw->p, (const uint8_t *)a.text + w.lo, (size_t)nb, hipMemcpyHostToDevice, s));
                if (c.log.end(s)) return 1;
            }
            stats[3] += (double)nb;
            const TextView t = {(const uint32_t *)raw->p, 0, (nb + 3) >> 2, -w.lo};
            if (run(t, w.i0, w.i1)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));               // the staging buffer is reused by the next window
        }
    }
    SNPGPU_HIP_CHECK(hipMemcpyAsync(a.line_flags, dflags->p, sizeof(int32_t) * n_lines, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(a.line_cells, dcells->p, sizeof(int64_t) * n_lines, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    if (c.log.sum_ms(T_TEXT_H2D, &stats[0]) || c.log.sum_ms(T_TEXT_KERNEL, &stats[1])) return 1;
    return 0;
}

}  // namespace snpgpu
