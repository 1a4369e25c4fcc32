// Line index of VCF text (snpgpu_vcf_index, include/snpgpu.h section 1l): for every data line of a buffer the byte offsets of
// the starts of its first ten tab-separated columns (CHROM, POS, ID, REF, ALT, QUAL, FILTER, INFO, FORMAT, first sample cell)
// and its end.  Plain C++ with no HIP call and no dependence on the rest of the library, so that it can be compiled and run
// on its own (a stand-alone program under a sanitizer, the CPU tests).  The '#' header is the caller's: every line here is data.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

namespace snpgpu {

constexpr int VCF_INDEX_COLS = 10;

// buf[0, n_bytes): whole lines, except that the last one may be cut anywhere when !final (it is left to the next buffer:
// *consumed is the offset behind the last complete line) and may lack its '\n' when final.  A line ends before its '\n' and
// before a '\r' in front of that.  col_begin: [max_lines][VCF_INDEX_COLS], line_end: [max_lines]; line_base: lines in front
// of this buffer, for the 1-based line number of an error message.  Returns an empty string, or the refusal.
inline std::string vcf_index_lines(const char *buf, int64_t n_bytes, bool final, int64_t line_base, int64_t max_lines,
                                   int64_t *col_begin, int64_t *line_end, int64_t *n_lines, int64_t *consumed)
{
    int64_t n = 0, pos = 0;
    while (pos < n_bytes) {
        const char *nl = (const char *)memchr(buf + pos, '\n', (size_t)(n_bytes - pos));
        if (!nl && !final) break;                                     // a cut line: the next buffer's
        const int64_t next = nl ? (nl - buf) + 1 : n_bytes;
        int64_t end = nl ? nl - buf : n_bytes;
        if (end > pos && buf[end - 1] == '\r') end--;
        const std::string where = "line " + std::to_string(line_base + n + 1);
        if (end == pos) return where + " is empty";
        if (n >= max_lines) return where + ": more lines than max_lines = " + std::to_string(max_lines);
        int64_t *col = col_begin + n * VCF_INDEX_COLS;
        col[0] = pos;
        int64_t p = pos;
        for (int c = 1; c < VCF_INDEX_COLS; c++) {
            const char *tab = p < end ? (const char *)memchr(buf + p, '\t', (size_t)(end - p)) : nullptr;
            if (!tab) return where + " has " + std::to_string(c) + " columns: fewer than the 10 of a line with one sample";
            p = (tab - buf) + 1;
            col[c] = p;
        }
        line_end[n] = end;
        n++;
        pos = next;
    }
    *n_lines = n;
    *consumed = pos;
    return std::string();
}

}  // namespace snpgpu
