// Device code (and inline host code) shared by the translation units of the N x N pairwise accumulators -- kernels_pair.hip (the pair
// counters), kernels_syrk.hip (fp32 / three-product / exact-row SYRKs), kernels_syrk_uv.hip (the single-product SYRKs): vector types,
// the tile enumeration, the LDS access helpers, the fused-launch geometry and the skeleton pieces that the kernels have in common.
#pragma once
#include <algorithm>
#include <stdlib.h>
#include "snpgpu_internal.h"

namespace snpgpu {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// tile enumeration shared by both kernels: block id -> (XCD, super-tile, tile)
// Block b is observed to run on XCD b%8; the blocks of one XCD walk the super-tiles
// {xcd, xcd+8, ...} so that concurrently resident workgroups share rows/columns in that
// XCD's L2.  The mapping only affects speed, never results.
struct TileCoord { int tr, tc; bool valid; };
// Tiles per super-tile side, rows and columns of a tile.  Taken by reference: as three value arguments the constants of a translation
// unit whose kernels all pass the same ones are propagated into map_tile before it is simplified on its own, and the kernels'
// prologues come out as other code than with a second shape in the file (profiles/pair_split_isa.md).
struct TileShape { int S, tile_r, tile_c; };

__device__ __forceinline__ TileCoord map_tile(const int *__restrict__ prefix, const int *__restrict__ first,
                                              int n_sr, int n_super, const TileShape &shape, int n_tr, int n_tc)
{
    const int S = shape.S, tile_r = shape.tile_r, tile_c = shape.tile_c;
    TileCoord t; t.valid = false; t.tr = t.tc = 0;
    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int slot = id >> 3;
    const int ss = S * S;
    const int sq = slot / ss, within = slot - sq * ss;
    const int st = sq * 8 + xcd;
    if (st >= n_super) return t;
    int lo = 0, hi = n_sr;  // find sr with prefix[sr] <= st < prefix[sr+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= st) lo = mid; else hi = mid;
    }
    const int sr = lo, sc = first[sr] + (st - prefix[sr]);
    t.tr = sr * S + within / S;
    t.tc = sc * S + within % S;
    // inside the panel and touching the upper triangle (panel-relative coordinates)
    t.valid = (t.tr < n_tr) && (t.tc < n_tc) && ((int64_t)(t.tc + 1) * tile_c > (int64_t)t.tr * tile_r);
    return t;
}

// ---------------------------------------------------------------------------
// LDS addresses are carried as 32-bit byte offsets (a generic pointer that passes through an opaque asm loses its address
// space and comes back as 64-bit arithmetic plus null checks)
typedef __attribute__((address_space(3))) const char x1_lds_char;
typedef __attribute__((address_space(3))) const volatile uint32_t x1_lds_u32;
__device__ __forceinline__ uint32_t x1_lds_off(const void *shared_ptr)
{
    return (uint32_t)(uintptr_t)(x1_lds_char *)shared_ptr;
}
__device__ __forceinline__ uint32_t x1_lds32(uint32_t off)
{
    return *(x1_lds_u32 *)(uintptr_t)off;
}
// 16 bytes per lane HBM / L2 -> LDS without VGPRs (lane l lands at lds_base + 16 l).  Written as inline asm on purpose: the
// compiler models __builtin_amdgcn_global_load_lds as a FLAT access that may touch LDS *and* memory, and while one is
// pending every wait it inserts becomes vmcnt(0) / lgkmcnt(0) -- with a table copy in flight for most of a chunk that
// turned all the counted waits of the word loads and lookups into full drains.  An instruction the waitcnt pass does not
// see only makes its vmcnt(N) waits conservative (the counter is in-order and the copy adds outstanding requests); the
// kernels wait for the copy explicitly (s_waitcnt vmcnt + barrier) before the first lookup in the new table.
__device__ __forceinline__ void x1_lds_dma16(const void *gsrc, uint32_t lds_base)
{
    const uint32_t b = __builtin_amdgcn_readfirstlane(lds_base);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gsrc), "s"(b) : "memory");
}
typedef __attribute__((address_space(3))) const volatile u32x4 x1_lds_u128;
__device__ __forceinline__ u32x4 x1_lds128(uint32_t off)
{
    return *(x1_lds_u128 *)(uintptr_t)off;
}

// ---------------------------------------------------------------------------
// One launch for ALL fp32 runs of a block (round 5), work items (tile, run): an XCD's queue is walked in groups of G tiles, run by
// run inside a group -- G = 32 = the XCD's CUs: the same 32 tiles are up again one round (~250 us) later, their 512 KB fp64 regions
// still in the Infinity Cache (256 tiles x 512 KB = 128 MB per round, chip-wide), and the block has ONE tail round instead of one
// per run.  A/B on one box (ms per 65 536-SNP step, N = 100 000, profiles/r05_run_inner_ab.txt): one launch per run 470.8 / 474.3,
// G = 32 467.9 / 468.9 (-0.9 %; blocks with missing calls 986.2 -> 977.7), G = 64 472.1 / 473.2, G = 4 476.3 / 476.8, G = 1 (the six
// runs of a tile side by side on six CUs, all flushing the same lines at once) 487.7 / 489.0.  SNPGPU_RUN_INNER=0: one launch per run.
inline int run_inner_launch()
{
    static const int g = getenv("SNPGPU_RUN_INNER") ? std::max(0, std::min(atoi(getenv("SNPGPU_RUN_INNER")), 1 << 20)) : 32;
    return g;
}
// workgroups of a fused launch: every XCD queue (n_blocks / 8 items) padded to whole groups, times the runs
inline unsigned run_inner_grid(int n_blocks, int n_runs, int group)
{
    const int per_xcd = n_blocks / 8, groups = (per_xcd + group - 1) / group;
    return (unsigned)groups * (unsigned)group * (unsigned)n_runs * 8u;
}

// The launches that cover the n_chunk table chunks of a block in fp32 runs of `run` chunks (n_runs of them), over a work list of
// n_blocks items.  group > 0: ONE fused (tile, run) launch, `group` tiles of an XCD queue walked run by run; group == 0: one launch per
// run; group < 0: one launch whose work items walk their runs themselves (syrk_uv16c_kernel, SNPGPU_SYRK_UV16=3).
struct RunLaunch { unsigned grid; int chunk_lo, chunk_hi, n_runs, run_chunks, run_group, n_items8; };
struct RunLaunches {
    int n_blocks, n_chunk, run, n_runs, group;
    int count() const { return group ? 1 : (n_chunk + run - 1) / run; }
    RunLaunch at(int k) const        // launch k; with one launch per run, k is the run (the kernels' run arguments are unused then)
    {
        if (group > 0) return {run_inner_grid(n_blocks, n_runs, group), 0, n_chunk, n_runs, run, group, n_blocks / 8};
        if (group < 0) return {(unsigned)n_blocks, 0, n_chunk, n_runs, run, 0, 0};
        return {(unsigned)n_blocks, k * run, std::min(k * run + run, n_chunk), 1, 0, 1, 0};
    }
};

// ---------------------------------------------------------------------------
// Skeleton pieces that the kernels of the three translation units share.  A piece is shared only where the kernel that takes it
// keeps the code it had with its own inline copy (tools/kernel_isa.py; profiles/pair_split_isa.md lists the outcome per kernel).
// Workgroup b of a fused (tile, run) launch: XCD b & 7, position b >> 3 in that XCD's queue.  The queue is cut into groups of
// `run_group` tiles and a group is walked run by run (group, run, tile in group).  wi: the work item; valid: the tile exists.
struct FusedItem { int wi, run; bool valid; };
__device__ __forceinline__ FusedItem fused_item(int n_runs, int run_group, int n_items8)
{
    const int kpos = (int)blockIdx.x >> 3, span = run_group * n_runs;
    const int grp = kpos / span, within = kpos - grp * span, run = within / run_group, ti = grp * run_group + (within - run * run_group);
    return {ti * 8 + ((int)blockIdx.x & 7), run, ti < n_items8};
}

// Part `z` of the `w` parts into which the K range [lo, hi) of a tile is split, the parts `round` units long or a multiple of it (the
// pipe depth of the counters); beg >= end: the part is empty.  UNIFORM: the bounds through readfirstlane (the division runs on the
// VALU; a uniform row address that is built from them -- the buffer descriptor of the fp4 counters' word loads -- must sit in SGPRs).
struct KPart { int beg, end; };
template <bool UNIFORM = false> __device__ __forceinline__ KPart k_part(int lo, int hi, int z, int w, int round = 1)
{
    const int per = (((hi - lo + w - 1) / w) + round - 1) / round * round;
    KPart k;
    k.beg = UNIFORM ? __builtin_amdgcn_readfirstlane(lo + z * per) : lo + z * per;
    k.end = (k.beg + per < hi) ? (k.beg + per) : hi;
    if (UNIFORM) k.end = __builtin_amdgcn_readfirstlane(k.end);
    return k;
}

// The 2 x 2 waves of a workgroup and a lane's place in its wave's MFMA tiles.  32 x 32 tiles: sample li of a tile, K half kh
// (C/D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 kh); 16 x 16 sub-tiles: sample l16, K quarter kq (row = r + 4 kq).
struct WaveCoord { int tid, lane, wave, wr, wc, li, kh, l16, kq; };
__device__ __forceinline__ WaveCoord wave_coord()
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return {tid, lane, wave, wave >> 1, wave & 1, lane & 31, lane >> 5, lane & 15, lane >> 4};
}

// zeroed accumulators: every vector of a (multi-dimensional) array of them
template <typename V> __device__ __forceinline__ void zero_acc(V &v)
{
#pragma unroll
    for (int r = 0; r < (int)(sizeof(V) / sizeof(v[0])); r++) v[r] = 0;
}
template <typename V, int N> __device__ __forceinline__ void zero_acc(V (&a)[N])
{
#pragma unroll
    for (int i = 0; i < N; i++) zero_acc(a[i]);
}

// rows of real samples at / below `first_row` (a lane's first row); padding rows are never written (they stay 0)
__device__ __forceinline__ int64_t flush_rows_left(int64_t n_rows_real, int64_t first_row)
{
    return (n_rows_real > 0 ? n_rows_real : ((int64_t)1 << 40)) - first_row;
}
// The flush address of a wave made opaque: the row addresses are computed at the flush, not hoisted out of the K loop (where the
// compiler kept them alive in scratch)
__device__ __forceinline__ double *flush_ptr(double *pacc)
{
    asm volatile("" : "+v"(pacc));
    return pacc;
}

// fp64 flush of a wave's TM x TN tiles of 32 x 32 fp32 sums by fire-and-forget atomics (one owner per element and launch part: no
// contention; fp32 partials are exactly representable in fp64, so the panel sums do not depend on the order in which the K parts of a
// tile arrive), one sched_barrier per row: address and convert temporaries stay short-lived.  SCALED: f_q x fp32 partial, exact in fp64
// (13 + 24 bits), as a global atomic; otherwise the plain sum through unsafeAtomicAdd.  CLEAR: the sums start again from 0 (a flush
// inside the K loop).
template <bool SCALED, bool CLEAR = false, int TM, int TN>
__device__ __forceinline__ void flush_tiles32(double *pacc, int64_t rs, int64_t rows_left, f32x16 (&c32)[TM][TN], double fscale)
{
    double *pflush = flush_ptr(pacc);
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = i * 32 + (r & 3) + 8 * (r >> 2);
            double *__restrict__ pr = pflush + (int64_t)row * rs;
            const bool real_row = (row < rows_left);
#pragma unroll
            for (int j = 0; j < TN; j++) {
                if (real_row && SCALED)
                    (void)__builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double *)(pr + 32 * j),
                                                                  (double)c32[i][j][r] * fscale);
                else if (real_row) unsafeAtomicAdd(pr + 32 * j, (double)c32[i][j][r]);
                if (CLEAR) c32[i][j][r] = 0.f;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
}

// The same for row i of a wave's TS x TS sub-tiles of 16 x 16: sub-tile j adds f_q x its partial; the sub-tiles j < nc carry their
// factors already and take part only if `carried_too` (syrk_uv16c_kernel: sums carried across runs meet the panel in the last run)
template <int TS>
__device__ __forceinline__ void flush_row16(double *pflush, int64_t rs, int64_t rows_left, const f32x4 (&c)[TS][TS], int i, double fscale,
                                            int nc, bool carried_too)
{
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = i * 16 + r;
        double *__restrict__ pr = pflush + (int64_t)row * rs;
        if (row < rows_left) {
#pragma unroll
            for (int j = 0; j < TS; j++)
                if (j >= nc || carried_too)
                    (void)__builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double *)(pr + 16 * j),
                                                                  (double)c[i][j][r] * (j < nc ? 1.0 : fscale));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// u32 counter flush of a wave's 32 x 32 tile (i, j): the counter of accumulator register 0 / of register r (C/D layout as above)
__device__ __forceinline__ uint32_t *tile32_counter0(uint32_t *acc, int64_t ncols_pad, int row_base, int64_t col_base, int i, int j,
                                                      int li, int kh)
{
    return acc + (int64_t)(row_base + 32 * i + 4 * kh) * ncols_pad + col_base + 32 * j + li;
}
__device__ __forceinline__ uint32_t *tile32_counter(uint32_t *p0, int64_t ncols_pad, int r)
{
    return p0 + (int64_t)((r & 3) + 8 * (r >> 2)) * ncols_pad;
}
}  // namespace snpgpu
