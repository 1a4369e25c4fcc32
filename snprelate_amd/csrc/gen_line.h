// One line of Oxford GEN text from its sixth column on, read the way the reference reads it (snpgpu_gen_line_host,
// include/snpgpu.h section 1p): CReadLine::GetCell splitting by space and tab, getFloat with the C library's strtof and the tree of
// gnrParseGEN (src/ConvToGDS.cpp:123-179, :506-532, :1120-1146).  Plain C++ with no HIP call and no dependence on the rest of the
// library, so that it can be compiled and run on its own (a stand-alone program under a sanitizer, the CPU tests).
#pragma once
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

namespace snpgpu {

inline const char *gen_skip_space(const char *p)
{
    while (isspace((unsigned char)*p)) p++;
    return p;
}

inline std::string gen_short_text(const char *p)
{
    return strlen(p) <= 16 ? std::string(p) : std::string(p, 16) + "...";
}

// getFloat with RaiseError: false and `err` when the reference throws
inline bool gen_get_float(const std::string &txt, double &val, std::string &err)
{
    const char *p = gen_skip_space(txt.c_str());
    char *end = (char *)p;
    val = strtof(p, &end);
    if (end == p) {
        if (*p != '.') { err = "Invalid float conversion \"" + gen_short_text(p) + "\"."; return false; }
        val = NAN;
        return true;
    }
    p = gen_skip_space(end);
    if (*p != 0) { err = "Invalid float conversion \"" + gen_short_text(p) + "\"."; return false; }
    return true;
}

// line[0, n_bytes): the 3 n_samp cells of one line, without the line end; the line ends at a NUL if it holds one, as the C string
// the reference holds.  codes: n_samp.  Returns 0 and an empty `message`, or the 1-based number of the failing cell counted from
// `line` and the reference's text.
inline int64_t gen_line_codes(const char *line, int64_t n_bytes, int64_t n_samp, double call_threshold, uint8_t *codes,
                              std::string &message)
{
    const std::string text(line, strnlen(line, (size_t)n_bytes));
    const char *cur = text.c_str();
    int64_t col = 0;
    std::string cell;
    message.clear();
    for (int64_t j = 0; j < n_samp; j++) {
        double pr[3];
        for (int q = 0; q < 3; q++) {
            // CReadLine::GetCell, splitting by space and tab
            const char *b = cur;
            while (*cur != '\t' && *cur != ' ' && *cur != 0) cur++;
            const char *e = cur;
            col++;
            if (b == e && *cur == 0) { message = "fewer columns than what expected."; return col; }
            if (j == n_samp - 1 && q == 2) {
                while (*cur == ' ') cur++;
                if (*cur != 0) { message = "more columns than what expected."; return col; }
            } else if (*cur == '\t') {
                cur++;
            } else {
                while (*cur == ' ') cur++;
            }
            if (e > b + 1 && ((b[0] == '"' && e[-1] == '"') || (b[0] == '\'' && e[-1] == '\''))) { b++; e--; }
            cell.assign(b, e);
            if (!gen_get_float(cell, pr[q], message)) return col;
        }
        const double aa = pr[0], ab = pr[1], bb = pr[2];
        if (aa >= ab) {
            if (aa >= bb) codes[j] = aa >= call_threshold ? 2 : 3;
            else codes[j] = bb >= call_threshold ? 0 : 3;
        } else {
            if (ab >= bb) codes[j] = ab >= call_threshold ? 1 : 3;
            else codes[j] = bb >= call_threshold ? 0 : 3;
        }
    }
    return 0;
}

}  // namespace snpgpu
