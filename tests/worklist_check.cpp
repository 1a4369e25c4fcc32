// Stand-alone check of snprelate_amd/csrc/worklist.h (test_cpu_plan.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers and runs it): build_worklist and plan_tile_grid against a brute-force restatement of their rules
// and against lists written out by hand.  Prints nothing and exits 0, or prints the failing case and exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "worklist.h"

using snpgpu::TilePanel;
using snpgpu::WorkItem;

namespace {

int failures = 0;

struct Case { int64_t N, row0, row1; int tile_r, tile_c, S; int64_t slots; int forced, copies; };

void bad(const Case &k, const char *what, int64_t at)
{
    if (failures == 20) return;              // (enough said; the exit status is what counts)
    failures++;
    std::printf("N %lld rows [%lld, %lld) tile %d x %d S %d slots %lld forced %d copies %d: %s at %lld\n", (long long)k.N, (long long)k.row0,
                (long long)k.row1, k.tile_r, k.tile_c, k.S, (long long)k.slots, k.forced, k.copies, what, (long long)at);
}

TilePanel panel(const Case &k) { return TilePanel{k.row0, k.row1, k.row0, k.N}; }

int64_t tiles_over(int64_t samples, int tile) { int64_t n = 0; while (n * tile < samples) n++; return n; }

// The parts of the tail round, in exact integers: the p in 2 ... 8 with the smallest ceil(rem p / slots) / p + (p - 1) / 50, the
// smallest such p, if that is below 1 (one part).  Distinct values differ by 1 / 2800 or more, far above the rule's 1e-9 margin.
int chosen_parts(int64_t rem, int64_t slots)
{
    if (rem == 0) return 1;
    int best = 1;
    int64_t best_c = 1;                      // the rounds of the best so far, ceil(rem best / slots)
    for (int p = 2; p <= 8; p++) {
        int64_t c = 0;
        while (c * slots < rem * p) c++;
        // c / p + (p - 1) / 50 < best_c / best + (best - 1) / 50, times 50 p best
        if (50 * c * best + (int64_t)(p - 1) * p * best < 50 * best_c * p + (int64_t)(best - 1) * p * best) { best = p; best_c = c; }
    }
    return best;
}

void check(const Case &k)
{
    const std::vector<WorkItem> work = snpgpu::build_worklist(panel(k), k.tile_r, k.tile_c, k.S, k.slots, k.forced, k.copies);
    const int64_t n_tr = tiles_over(k.row1 - k.row0, k.tile_r), n_tc = tiles_over(k.N - k.row0, k.tile_c);
    if (work.size() % 8 != 0) { bad(k, "the length is no multiple of 8:", (int64_t)work.size()); return; }
    const size_t per_queue = work.size() / 8;

    // every tile of the upper trapezoid, for every copy: its parts value and how often each part was seen
    std::vector<int> parts_of((size_t)(n_tr * n_tc * k.copies), 0);
    std::vector<std::vector<int>> seen((size_t)(n_tr * n_tc * k.copies));
    int64_t n_tiles = 0;
    for (int64_t tr = 0; tr < n_tr; tr++)
        for (int64_t tc = 0; tc < n_tc; tc++) n_tiles += ((tc + 1) * k.tile_c > tr * k.tile_r) ? k.copies : 0;
    const int64_t rem = n_tiles % k.slots;
    const int want_parts = k.forced ? k.forced : chosen_parts(rem, k.slots);

    std::vector<int64_t> tiles_in_queue(8, 0);
    bool unpadded_queue = per_queue == 0;
    for (int x = 0; x < 8; x++) {
        // item i of queue x sits at i * 8 + x: whole tiles first, then the split tiles part by part in one order, then padding
        std::vector<WorkItem> q;
        bool padding = false;
        for (size_t i = 0; i < per_queue; i++) {
            const WorkItem &w = work[i * 8 + (size_t)x];
            if ((w.parts & 0xFFFF) == 0) {
                if (w.tile_r || w.tile_c || w.part || w.parts) bad(k, "a padding item is not all zero: item", (int64_t)(i * 8 + (size_t)x));
                padding = true;
                continue;
            }
            if (padding) { bad(k, "an item behind the padding of its queue: item", (int64_t)(i * 8 + (size_t)x)); continue; }
            q.push_back(w);
        }
        if (q.size() == per_queue) unpadded_queue = true;
        size_t whole = 0, split = 0;
        for (const WorkItem &w : q) {
            const int parts = w.parts & 0xFFFF, copy = w.parts >> 16;
            if (w.tile_r < 0 || w.tile_r >= n_tr || w.tile_c < 0 || w.tile_c >= n_tc || !((int64_t)(w.tile_c + 1) * k.tile_c > (int64_t)w.tile_r * k.tile_r)) {
                bad(k, "a tile outside the upper trapezoid: tile row", w.tile_r);
                continue;
            }
            if (copy < 0 || copy >= k.copies) { bad(k, "a copy index outside the copies:", copy); continue; }
            if (w.part < 0 || w.part >= parts) { bad(k, "a part outside its parts:", w.part); continue; }
            const size_t t = (size_t)((w.tile_r * n_tc + w.tile_c) * k.copies + copy);
            if (parts_of[t] && parts_of[t] != parts) bad(k, "a tile with two parts values: tile row", w.tile_r);
            parts_of[t] = parts;
            seen[t].resize((size_t)parts, 0);
            seen[t][(size_t)w.part]++;
            if (parts == 1) whole++;
            else if (w.part == 0) split++;
            if (parts > 1 && parts != want_parts) bad(k, "a split tile with other parts than the rule gives:", parts);
        }
        tiles_in_queue[(size_t)x] = (int64_t)(whole + split);
        // the queue gives its last min(tiles, (rem + 7 - x) / 8) tiles to the split, when there is one
        int64_t want_split = (want_parts > 1) ? (rem + 7 - x) / 8 : 0;
        if (want_split > tiles_in_queue[(size_t)x]) want_split = tiles_in_queue[(size_t)x];
        if ((int64_t)split != want_split) bad(k, "a queue splits another number of tiles than (rem + 7 - x) / 8: queue", x);
        if (rem == 0 && split) bad(k, "a split without a tail round: queue", x);
        if (q.size() != whole + split * (size_t)(split ? want_parts : 0)) { bad(k, "a queue of another length than its tiles and parts: queue", x); continue; }
        for (size_t i = 0; i < q.size(); i++) {
            if (i < whole) {
                if ((q[i].parts & 0xFFFF) != 1) bad(k, "a split tile before a whole one: queue", x);
                continue;
            }
            const size_t p = (i - whole) / split, j = (i - whole) % split;
            const WorkItem &first = q[whole + j];
            if ((size_t)q[i].part != p || q[i].tile_r != first.tile_r || q[i].tile_c != first.tile_c || q[i].parts != first.parts)
                bad(k, "the split tiles do not repeat part by part in one order: queue", x);
        }
    }
    if (!unpadded_queue) bad(k, "every queue ends in padding: items", (int64_t)work.size());
    for (int x = 0; x < 8; x++)
        for (int y = 0; y < 8; y++)
            if (tiles_in_queue[(size_t)x] > tiles_in_queue[(size_t)y] + 1) bad(k, "two queues differ by more than one tile: queue", x);

    for (int64_t tr = 0; tr < n_tr; tr++)
        for (int64_t tc = 0; tc < n_tc; tc++)
            for (int cp = 0; cp < k.copies; cp++) {
                const size_t t = (size_t)((tr * n_tc + tc) * k.copies + cp);
                const bool inside = (tc + 1) * k.tile_c > tr * k.tile_r;
                if (!inside) {
                    if (parts_of[t]) bad(k, "a tile below the trapezoid is listed: tile row", tr);
                    continue;
                }
                if (!parts_of[t]) { bad(k, "a tile is left out: tile row", tr); continue; }
                for (int n : seen[t])
                    if (n != 1) bad(k, "a part of a tile is not listed exactly once: tile row", tr);
            }
}

void check_grid(const Case &k)
{
    const snpgpu::TileGridPlan t = snpgpu::plan_tile_grid(panel(k), k.tile_r, k.tile_c, k.S);
    const int64_t n_tr = tiles_over(k.row1 - k.row0, k.tile_r), n_tc = tiles_over(k.N - k.row0, k.tile_c);
    const int64_t n_sr = tiles_over(n_tr, k.S), n_sc = tiles_over(n_tc, k.S);
    if (t.n_tr != n_tr || t.n_tc != n_tc || t.n_sr != n_sr) { bad(k, "tile grid: other tile counts, super-rows", t.n_sr); return; }
    if ((int64_t)t.prefix.size() != n_sr + 1 || (int64_t)t.first.size() != n_sr) { bad(k, "tile grid: table lengths", (int64_t)t.prefix.size()); return; }
    int64_t count = 0;
    for (int64_t sr = 0; sr < n_sr; sr++) {
        // the super-columns whose last sample column lies before the first row of the super-row hold no tile of the trapezoid
        int64_t before = 0;
        for (int64_t sc = 0; sc < n_sc; sc++) before += ((sc + 1) * k.S * k.tile_c <= sr * k.S * k.tile_r) ? 1 : 0;
        if (t.first[(size_t)sr] != before) bad(k, "tile grid: first super-column of super-row", sr);
        if (t.prefix[(size_t)sr] != count) bad(k, "tile grid: prefix of super-row", sr);
        count += n_sc - before;
    }
    if (t.prefix[(size_t)n_sr] != count || t.n_super != count) bad(k, "tile grid: n_super is not the count of valid super-tiles:", t.n_super);
    int64_t groups = 0;
    while (groups * 8 < count) groups++;
    if (t.grid != groups * 8 * k.S * k.S) bad(k, "tile grid: grid is not the workgroups of whole groups of 8 super-tiles:", t.grid);
}

void same(const Case &k, const std::vector<WorkItem> &want)
{
    const std::vector<WorkItem> got = snpgpu::build_worklist(panel(k), k.tile_r, k.tile_c, k.S, k.slots, k.forced, k.copies);
    if (got.size() != want.size()) { bad(k, "hand-written list: another length:", (int64_t)got.size()); return; }
    for (size_t i = 0; i < got.size(); i++)
        if (got[i].tile_r != want[i].tile_r || got[i].tile_c != want[i].tile_c || got[i].part != want[i].part || got[i].parts != want[i].parts)
            bad(k, "hand-written list: another item", (int64_t)i);
}

}  // namespace

int main()
{
    const int tiles[3][2] = {{128, 128}, {256, 256}, {256, 128}};
    for (int64_t N : {1, 255, 256, 257, 700, 1500, 4097}) {
        std::vector<Case> panels = {{N, 0, N}};
        if (N > 256) panels.push_back({N, 256, N < 512 ? N : 512});
        if (N > 512) panels.push_back({N, 512, N});
        for (Case k : panels)
            for (const auto &t : tiles)
                for (int S : {1, 2, 4}) {
                    k.tile_r = t[0]; k.tile_c = t[1]; k.S = S;
                    k.slots = 1; k.forced = 0; k.copies = 1;
                    check_grid(k);
                    for (int64_t slots : {1, 7, 256, 512})
                        for (int forced : {0, 1, 5, 64})
                            for (int copies : {1, 2}) {
                                k.slots = slots; k.forced = forced; k.copies = copies;
                                check(k);
                            }
                }
        // the grids the contexts ask for: 32 x 128 tiles in super-tiles of 8 (popcount pair kernel), 128 x 128 in 4 (fp32 SYRK)
        for (Case k : panels) {
            k.slots = 1; k.forced = 0; k.copies = 1;
            k.tile_r = 32; k.tile_c = 128; k.S = 8;
            check_grid(k);
            k.tile_r = 128; k.tile_c = 128; k.S = 4;
            check_grid(k);
        }
    }

    const WorkItem Z{0, 0, 0, 0};
    {
        // 256 samples in 128 x 128 tiles: (0, 0), (0, 1), (1, 1), one per super-tile and queue.  512 slots, 3 tiles in the tail round:
        // p parts last 1 / p + 0.02 (p - 1): 0.52, 0.373, 0.31, 0.28, 0.267, 0.2629 (p = 7), 0.265 -- seven parts each
        std::vector<WorkItem> want;
        for (int p = 0; p < 7; p++)
            for (const WorkItem &w : {WorkItem{0, 0, p, 7}, WorkItem{0, 1, p, 7}, WorkItem{1, 1, p, 7}, Z, Z, Z, Z, Z}) want.push_back(w);
        same(Case{256, 0, 256, 128, 128, 1, 512, 0, 1}, want);
    }
    {
        // the same tiles twice (copies = 2) in ONE 2 x 2 super-tile: queue 0 gets all six, {(0, 0), (0, 1), (1, 1)} x {copy 0, copy 1},
        // and hands them from its end to queues 1 ... 5.  4 slots: 2 tiles in the tail round; 2 parts last 1 / 2 + 0.02, 3: 2 / 3 + 0.04,
        // 4: 2 / 4 + 0.06 ... -- two parts, for the last tile of queues 0 and 1 ((2 + 7 - x) / 8 = 1, 1, 0 ...)
        const int c1 = 1 << 16;
        same(Case{256, 0, 256, 128, 128, 2, 4, 0, 2},
             {WorkItem{0, 0, 0, 2}, WorkItem{1, 1, 0, 2 | c1}, WorkItem{1, 1, 0, 1}, WorkItem{0, 1, 0, 1 | c1}, WorkItem{0, 1, 0, 1}, WorkItem{0, 0, 0, 1 | c1}, Z, Z,
              WorkItem{0, 0, 1, 2}, WorkItem{1, 1, 1, 2 | c1}, Z, Z, Z, Z, Z, Z});
    }
    {
        // rows [256, 512) of 700 samples in 256 x 128 tiles: one tile row, columns 256 ... 699 in four tiles, a queue each.  3 slots: one
        // tile in the tail round, queue 0's ((1 + 7 - x) / 8 = 1, 0 ...), in the three parts that are forced
        same(Case{700, 256, 512, 256, 128, 1, 3, 3, 1},
             {WorkItem{0, 0, 0, 3}, WorkItem{0, 1, 0, 1}, WorkItem{0, 2, 0, 1}, WorkItem{0, 3, 0, 1}, Z, Z, Z, Z,
              WorkItem{0, 0, 1, 3}, Z, Z, Z, Z, Z, Z, Z,
              WorkItem{0, 0, 2, 3}, Z, Z, Z, Z, Z, Z, Z});
    }
    return failures ? 1 : 0;
}
