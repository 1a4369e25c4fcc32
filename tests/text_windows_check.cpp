// Stand-alone check of snprelate_amd/csrc/text_windows.h (test_cpu_textio.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers and runs it): plan_text_windows against a brute-force restatement of its rule.  Prints nothing
// and exits 0, or prints the failing case and exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "text_windows.h"

using snpgpu::TextWindow;

namespace {

int failures = 0;

void bad(const char *name, int64_t stage, const char *what, int64_t at)
{
    std::printf("%s, stage %lld: %s at %lld\n", name, (long long)stage, what, (long long)at);
    failures++;
}

// hi - lo of the lines [i0, i1), found line by line
int64_t span(const std::vector<int64_t> &cb, const std::vector<int64_t> &le, int64_t i0, int64_t i1)
{
    int64_t lo = cb[(size_t)i0], hi = le[(size_t)i0];
    for (int64_t i = i0 + 1; i < i1; i++) {
        if (cb[(size_t)i] < lo) lo = cb[(size_t)i];
        if (le[(size_t)i] > hi) hi = le[(size_t)i];
    }
    return hi - lo;
}

void check(const char *name, const std::vector<int64_t> &cb, const std::vector<int64_t> &le, int64_t stage)
{
    const int64_t n = (int64_t)cb.size();
    int64_t max_bytes = -1;
    const std::vector<TextWindow> wins = snpgpu::plan_text_windows(cb.data(), le.data(), n, stage, &max_bytes);
    int64_t next = 0, largest = 0;
    for (size_t k = 0; k < wins.size(); k++) {
        const TextWindow &w = wins[k];
        if (w.i0 != next || w.i1 <= w.i0 || w.i1 > n) { bad(name, stage, "the windows do not partition the lines in order: window", (int64_t)k); return; }
        next = w.i1;
        int64_t lo = cb[(size_t)w.i0], hi = le[(size_t)w.i0];
        for (int64_t i = w.i0; i < w.i1; i++) {
            if (cb[(size_t)i] < lo) lo = cb[(size_t)i];
            if (le[(size_t)i] > hi) hi = le[(size_t)i];
        }
        if (w.lo != lo || w.hi != hi) bad(name, stage, "lo, hi are not the smallest begin and the largest end: window", (int64_t)k);
        if (hi - lo > stage && w.i1 - w.i0 != 1) bad(name, stage, "more than one line beyond the stage: window", (int64_t)k);
        if (w.i1 < n && span(cb, le, w.i0, w.i1 + 1) <= stage) bad(name, stage, "the next line would have fitted: window", (int64_t)k);
        if (hi - lo > largest) largest = hi - lo;
    }
    if (next != n) bad(name, stage, "lines left over from", next);
    if (max_bytes != largest) bad(name, stage, "max_bytes is not the largest hi - lo, it is", max_bytes);
}

// lines of the given lengths, `gap` bytes between the end of one and the begin of the next
void lay_out(const std::vector<int64_t> &len, int64_t gap, std::vector<int64_t> &cb, std::vector<int64_t> &le)
{
    int64_t at = gap;
    cb.clear(); le.clear();
    for (int64_t l : len) { cb.push_back(at); le.push_back(at + l); at += l + gap; }
}

}  // namespace

int main()
{
    std::vector<int64_t> cb, le;

    lay_out({17}, 6, cb, le);
    for (int64_t stage : {1, 17, 40}) check("one line", cb, le, stage);

    lay_out(std::vector<int64_t>(9, 0), 6, cb, le);
    for (int64_t stage : {1, 6, 12, 1000}) check("all lines of length 0", cb, le, stage);
    lay_out(std::vector<int64_t>(9, 0), 0, cb, le);
    check("all lines empty at one offset", cb, le, 1);

    lay_out({10, 0, 30, 5, 100, 1, 1}, 6, cb, le);
    check("mixed lengths", cb, le, 40);
    check("mixed lengths", cb, le, 1);
    {
        int64_t max_bytes = 0;
        const std::vector<TextWindow> w40 = snpgpu::plan_text_windows(cb.data(), le.data(), 7, 40, &max_bytes);
        bool alone = false;
        for (const TextWindow &w : w40) alone = alone || (w.i0 == 4 && w.i1 == 5);
        if (!alone || max_bytes != 100) bad("mixed lengths", 40, "the line of 100 does not stand alone, max_bytes", max_bytes);
        const std::vector<TextWindow> w1 = snpgpu::plan_text_windows(cb.data(), le.data(), 7, 1, &max_bytes);
        if (w1.size() != 7) bad("mixed lengths", 1, "not one window per line: windows", (int64_t)w1.size());
    }

    // begins that do not ascend: the lines of a text listed in another order
    cb = {500, 0, 40, 900, 20, 480};
    le = {520, 30, 45, 1000, 25, 500};
    for (int64_t stage : {1, 30, 100, 520, 2000}) check("non-ascending cell_begin", cb, le, stage);

    uint64_t state = 12345;
    const auto rnd = [&](uint64_t m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (int64_t)((state >> 33) % m); };
    std::vector<int64_t> len(1000);
    for (int64_t &l : len) l = rnd(8) == 0 ? 0 : rnd(300);
    lay_out(len, 6, cb, le);
    for (int64_t stage : {1, 256, 5000}) check("1000 pseudo-random lines", cb, le, stage);

    return failures ? 1 : 0;
}
