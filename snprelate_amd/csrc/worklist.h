// Which workgroup computes which tile of a panel's upper trapezoid: the work lists of the MFMA pair kernels and of the split-fp16
// SYRKs, and the super-tile tables of the kernels that enumerate their tiles themselves.  Integer logic without HIP, so that
// tests/worklist_check.cpp can hold it to a brute-force restatement on the CPU; ctx_life.hip uploads what these functions return.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace snpgpu {

// sample rows [row0, row1) against columns [col0, N), as CtxPlan has them
struct TilePanel { int64_t row0, row1, col0, N; };

// {tile row, tile column, K part, K parts | copy << 16}, read by the kernels as one int4; all zero: padding (a workgroup without work)
struct WorkItem { int tile_r, tile_c, part, parts; };

// Tiles touching the upper trapezoid of the panel are grouped in S x S super-tiles; super-tile k goes to XCD k % 8 (workgroup b
// runs on XCD b % 8), so the tiles that are resident together on one XCD share operand rows/columns in its L2.  The chip runs
// `slots` workgroups at a time (workgroups per CU x CUs); the tiles of the last, partially filled round are split along K into the
// number of parts that makes that round shortest (their counters are flushed with atomics, so parts may share a tile), or into
// `forced_parts` when that is not 0.
// copies > 1: every tile appears `copies` times (copy index in bits 16.. of the item's fourth field): several independent
// products over the same tiles in ONE launch (KING-homo's two weight sums), balanced together
inline std::vector<WorkItem> build_worklist(const TilePanel &g, int tile_r, int tile_c, int S, int64_t slots, int forced_parts, int copies)
{
    const int n_tr = (int)((g.row1 - g.row0 + tile_r - 1) / tile_r);
    const int n_tc = (int)((g.N - g.col0 + tile_c - 1) / tile_c);
    const int n_sr = (n_tr + S - 1) / S, n_sc = (n_tc + S - 1) / S;
    // (tile row, tile column | copy << 20): the copy index travels in the column field until the items are written
    std::vector<std::vector<std::pair<int, int>>> queue(8);
    int k = 0;
    for (int sr = 0; sr < n_sr; sr++)
        for (int sc = 0; sc < n_sc; sc++) {
            std::vector<std::pair<int, int>> tiles;
            for (int a = 0; a < S; a++)
                for (int b = 0; b < S; b++) {
                    const int tr = sr * S + a, tc = sc * S + b;
                    if (tr < n_tr && tc < n_tc && (int64_t)(tc + 1) * tile_c > (int64_t)tr * tile_r)
                        for (int cp = 0; cp < copies; cp++) tiles.push_back({tr, tc | (cp << 20)});
                }
            if (tiles.empty()) continue;
            auto &q = queue[k++ & 7];
            q.insert(q.end(), tiles.begin(), tiles.end());
        }
    // even out the queues (diagonal super-tiles are smaller): move tiles from the longest to the shortest
    for (;;) {
        int lo = 0, hi = 0;
        for (int x = 1; x < 8; x++) {
            if (queue[x].size() < queue[lo].size()) lo = x;
            if (queue[x].size() > queue[hi].size()) hi = x;
        }
        if (queue[hi].size() <= queue[lo].size() + 1) break;
        queue[lo].push_back(queue[hi].back());
        queue[hi].pop_back();
    }
    int64_t T = 0;
    for (auto &q : queue) T += (int64_t)q.size();
    const int64_t rem = T % slots;
    int parts = 1;
    if (rem > 0) {
        double best = 1.0;                           // duration of the last round in units of a whole tile
        for (int p = 2; p <= 8; p++) {
            const double d = (double)((rem * p + slots - 1) / slots) / p + 0.02 * (p - 1);   // + flush overhead
            if (d < best - 1e-9) { best = d; parts = p; }
        }
    }
    if (forced_parts) parts = forced_parts;
    // split the last `rem` tiles, rem/8 from the end of every queue
    std::vector<WorkItem> work;
    size_t longest = 0;
    std::vector<std::vector<WorkItem>> items(8);
    for (int x = 0; x < 8; x++) {
        const auto &q = queue[x];
        const size_t n_split = (parts > 1) ? std::min(q.size(), (size_t)((rem + 7 - x) / 8)) : 0;
        for (size_t i = 0; i < q.size() - n_split; i++)
            items[x].push_back(WorkItem{q[i].first, q[i].second & 0xFFFFF, 0, 1 | ((q[i].second >> 20) << 16)});
        for (int p = 0; p < parts; p++)
            for (size_t i = q.size() - n_split; i < q.size(); i++)
                items[x].push_back(WorkItem{q[i].first, q[i].second & 0xFFFFF, p, parts | ((q[i].second >> 20) << 16)});
        longest = std::max(longest, items[x].size());
    }
    work.assign(longest * 8, WorkItem{0, 0, 0, 0});
    for (int x = 0; x < 8; x++)
        for (size_t i = 0; i < items[x].size(); i++) work[i * 8 + x] = items[x][i];
    return work;
}

// Super-tile tables of the kernels that find their tile from the workgroup index (TileGrid, snpgpu_internal.h): per super-row the
// first super-column that reaches the diagonal and the number of valid super-tiles before it; `grid` workgroups cover them
struct TileGridPlan {
    int n_tr, n_tc, n_sr, n_super, grid;
    std::vector<int> prefix, first;        // [n_sr + 1], [n_sr]
};

inline TileGridPlan plan_tile_grid(const TilePanel &g, int tile_r, int tile_c, int S)
{
    TileGridPlan t;
    t.n_tr = (int)((g.row1 - g.row0 + tile_r - 1) / tile_r);
    t.n_tc = (int)((g.N - g.col0 + tile_c - 1) / tile_c);
    t.n_sr = (t.n_tr + S - 1) / S;
    const int n_sc = (t.n_tc + S - 1) / S;
    t.prefix.assign(t.n_sr + 1, 0);
    t.first.assign(t.n_sr, 0);
    for (int sr = 0; sr < t.n_sr; sr++) {
        // first super-column whose last sample column reaches the first row of this super-row
        const int64_t row_lo = (int64_t)sr * S * tile_r;
        int f = (int)(row_lo / ((int64_t)S * tile_c));
        if (f > n_sc) f = n_sc;
        t.first[sr] = f;
        t.prefix[sr + 1] = t.prefix[sr] + (n_sc - f);
    }
    t.n_super = t.prefix[t.n_sr];
    t.grid = 8 * S * S * ((t.n_super + 7) / 8);
    return t;
}

}  // namespace snpgpu
