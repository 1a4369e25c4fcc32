// The staging windows of host text (text_host.h: snpgpu_vcf_genotypes, snpgpu_gen_genotypes), no HIP call: which runs of whole
// lines go through the staging buffer together.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace snpgpu {

// the lines [i0, i1) and the bytes [lo, hi) of the text that hold their cells
struct TextWindow { int64_t i0, i1, lo, hi; };

// Greedy, in line order: a window takes the next line while the bytes from the smallest cell_begin to the largest line_end of
// its lines stay within `stage`; a line that alone is longer than `stage` is a window of its own.  The offsets need not ascend.
// *max_bytes: the largest hi - lo.
inline std::vector<TextWindow> plan_text_windows(const int64_t *cell_begin, const int64_t *line_end, int64_t n_lines, int64_t stage,
                                                 int64_t *max_bytes)
{
    std::vector<TextWindow> wins;
    *max_bytes = 0;
    for (int64_t i = 0; i < n_lines;) {
        TextWindow w = {i, i + 1, cell_begin[i], line_end[i]};
        while (w.i1 < n_lines) {
            const int64_t lo = std::min(w.lo, cell_begin[w.i1]), hi = std::max(w.hi, line_end[w.i1]);
            if (hi - lo > stage) break;
            w.lo = lo; w.hi = hi; w.i1++;
        }
        *max_bytes = std::max(*max_bytes, w.hi - w.lo);
        wins.push_back(w);
        i = w.i1;
    }
    return wins;
}

}  // namespace snpgpu
