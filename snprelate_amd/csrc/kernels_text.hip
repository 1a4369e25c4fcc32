// 2-bit rows -> lines of text (snpgpu_text_render, include/snpgpu.h section 1m; host layer: text.hip).  One workgroup per line.
//   text_fixed_kernel     every piece has the same width (1 byte: Eigenstrat digits; 4 bytes: "\tX Y" of PED with constant or
//                         one-byte alleles), so a byte of the line knows its column by a shift.  The workgroup walks the line in
//                         chunks of TEXT_CHUNK bytes, one aligned 16-byte segment per lane: the lane builds its 16 bytes in registers
//                         and stores them at once.
//   text_lengths_kernel   variable-width lines, first pass: the line's length = prefix + sum over columns of width(column, code) + 1
//   text_variable_kernel  second pass.  TEXT_TILE columns per step, four per lane; a workgroup-wide exclusive scan of their widths
//                         (in LDS, 64-bit) places every piece.  The tile's bytes are then walked in aligned 16-byte segments as
//                         above: a lane finds the piece of its first byte by bisection of the scan and steps on from there, so a
//                         piece of any length (a 5 000-byte allele) is just many segments.  The bytes between the last whole
//                         segment and the tile's end are carried through LDS to the lane that stores that segment in the next tile.
// Loads of the rows are aligned dwords that hold a byte of the line's own row.  Stores are aligned 16-byte segments inside the
// line, single bytes only in the segments the line shares with its neighbours (its first and last).  No atomics, no data-dependent
// order: the text is a pure function of the input.
#include "text.h"

namespace snpgpu {

namespace {

// the code of column `col` of the row that starts at byte row0 of j.rows_w (col < n_cols)
__device__ __forceinline__ uint32_t code_at(const TextJob &j, int64_t row0, int64_t col)
{
    const int64_t a = row0 + (col >> 2);
    const uint32_t d = j.rows_w[a >> 2];
    return (d >> (8 * ((uint32_t)a & 3u) + 2 * ((uint32_t)col & 3u))) & 3u;
}

// bytes [lo, hi) of the aligned segment at byte q of text_al
__device__ __forceinline__ void store_segment(uint8_t *text_al, int64_t q, const uint32_t (&v)[4], int lo, int hi)
{
    if (lo == 0 && hi == TEXT_SEG) {
        *reinterpret_cast<uint4 *>(text_al + q) = make_uint4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < TEXT_SEG; i++)
        if (i >= lo && i < hi) text_al[q + i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
}

struct Prefix { int64_t begin, len; };

__device__ __forceinline__ Prefix prefix_of(const TextJob &j, int64_t r)
{
    if (!j.pre_off) return {0, 0};
    const int64_t b = j.pre_off[r];
    return {b, j.pre_off[r + 1] - b};
}

// bytes of the piece of (col, code) in a variable-width line
__device__ __forceinline__ int64_t piece_width(const TextJob &j, int64_t col, uint32_t code)
{
    if (code == 3u) return 4;
    const int64_t o0 = j.al_off[2 * col], o1 = j.al_off[2 * col + 1], o2 = j.al_off[2 * col + 2];
    const int64_t l1 = o1 - o0, l2 = o2 - o1;
    return 2 + (code == 0u ? 2 * l2 : code == 1u ? l1 + l2 : 2 * l1);
}

}  // namespace

__global__ __launch_bounds__(TEXT_THREADS) void text_fixed_kernel(TextJob j)
{
    const int64_t r = blockIdx.x;
    const int wsh = j.format == SNPGPU_TEXT_DIGIT ? 0 : 2;
    const int64_t body = j.n_cols << wsh;
    const Prefix pf = prefix_of(j, r);
    const int64_t start = j.text_shift + r * (body + 1) + (j.pre_off ? pf.begin - j.pre_off[0] : 0);
    const int64_t end = start + pf.len + body + 1;
    const int64_t row0 = j.rows_shift + r * j.rb;
    const bool table = j.format == SNPGPU_TEXT_PED_ALLELE;
    const uint32_t c1 = j.format == SNPGPU_TEXT_PED_12 ? '1' : 'A', c2 = j.format == SNPGPU_TEXT_PED_12 ? '2' : 'B';

    for (int64_t q = (start & ~int64_t(TEXT_SEG - 1)) + TEXT_SEG * (int64_t)threadIdx.x; q < end; q += TEXT_CHUNK) {
        const int lo = q < start ? (int)(start - q) : 0;
        const int hi = end - q < TEXT_SEG ? (int)(end - q) : TEXT_SEG;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < TEXT_SEG; i++) {
            if (i < lo || i >= hi) continue;
            const int64_t rel = q + i - start;
            uint32_t c;
            if (rel < pf.len) {
                c = j.pre_pool[pf.begin + rel];
            } else if (rel - pf.len == body) {
                c = '\n';
            } else {
                const int64_t x = rel - pf.len, col = x >> wsh;
                const uint32_t code = code_at(j, row0, col);
                if (wsh == 0) {
                    c = code < 3u ? '0' + code : '9';
                } else {
                    const uint32_t k = (uint32_t)x & 3u;
                    if (k == 0u) c = '\t';
                    else if (k == 2u) c = ' ';
                    else if (code == 3u) c = '0';
                    else {
                        const uint32_t a1 = table ? j.al_pool[2 * col] : c1, a2 = table ? j.al_pool[2 * col + 1] : c2;
                        c = k == 1u ? (code == 0u ? a2 : a1) : (code == 2u ? a1 : a2);
                    }
                }
            }
            v[i >> 2] |= c << (8 * (i & 3));
        }
        store_segment(j.text_al, q, v, lo, hi);
    }
}

__global__ __launch_bounds__(TEXT_THREADS) void text_lengths_kernel(TextJob j, int64_t *__restrict__ len)
{
    __shared__ int64_t s_sum[TEXT_THREADS];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x, row0 = j.rows_shift + r * j.rb;
    int64_t sum = 0;
    for (int64_t col = tid; col < j.n_cols; col += TEXT_THREADS) sum += piece_width(j, col, code_at(j, row0, col));
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = TEXT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) s_sum[tid] += s_sum[tid + d];
        __syncthreads();
    }
    if (tid == 0) len[r] = prefix_of(j, r).len + s_sum[0] + 1;
}

__global__ __launch_bounds__(TEXT_THREADS) void text_variable_kernel(TextJob j, const int64_t *__restrict__ line_off)
{
    __shared__ int64_t s_start[TEXT_TILE + 1];         // where a tile's pieces start behind the tile's first byte; [TEXT_TILE]: their sum
    __shared__ int64_t s_scan[2][TEXT_THREADS];
    __shared__ uint8_t s_code[TEXT_TILE];
    __shared__ uint8_t s_carry[2][TEXT_SEG];

    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x, row0 = j.rows_shift + r * j.rb;
    const Prefix pf = prefix_of(j, r);
    const int64_t ls = j.text_shift + line_off[r];      // the line's first byte in text_al
    const int64_t n_tiles = (j.n_cols + TEXT_TILE - 1) / TEXT_TILE;
    int64_t base = 0;                                   // bytes of the tiles before this one

    for (int64_t t = 0; t < n_tiles; t++) {
        const int64_t col0 = t * TEXT_TILE;
        // ---- widths of the tile's pieces and their exclusive scan: a lane's four columns are one byte of the row -----------------------
        int64_t w[TEXT_LANE_COLS], lane_sum = 0;
#pragma unroll
        for (int k = 0; k < TEXT_LANE_COLS; k++) {
            const int64_t col = col0 + TEXT_LANE_COLS * tid + k;
            uint32_t code = 3u;
            w[k] = 0;
            if (col < j.n_cols) {
                code = code_at(j, row0, col);
                w[k] = piece_width(j, col, code);
            }
            s_code[TEXT_LANE_COLS * tid + k] = (uint8_t)code;
            lane_sum += w[k];
        }
        s_scan[0][tid] = lane_sum;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < TEXT_THREADS; d <<= 1) {
            s_scan[cur ^ 1][tid] = s_scan[cur][tid] + (tid >= d ? s_scan[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        int64_t at = s_scan[cur][tid] - lane_sum;
#pragma unroll
        for (int k = 0; k < TEXT_LANE_COLS; k++) {
            s_start[TEXT_LANE_COLS * tid + k] = at;
            at += w[k];
        }
        if (tid == TEXT_THREADS - 1) s_start[TEXT_TILE] = at;
        __syncthreads();
        const int64_t total = s_start[TEXT_TILE];

        // ---- the tile's bytes [ra, rbn) of text_al; whole segments [sa, se), the rest is carried ------------------------------------
        const bool last = t == n_tiles - 1;
        const int64_t body0 = ls + pf.len + base;                                // the tile's first piece
        const int64_t ra = t == 0 ? ls : body0;
        const int64_t rbn = body0 + total + (last ? 1 : 0);
        const int64_t sa = ra & ~int64_t(TEXT_SEG - 1);
        const int64_t se = last ? rbn : (rbn & ~int64_t(TEXT_SEG - 1));

        // the byte at `a` (ra <= a < rbn), stepping through the pieces with the cursor (idx, pend): idx < 0 = not yet looked up
        int idx = -1;
        int64_t pbeg = 0, pend = 0, la = 0;
        const uint8_t *pa = nullptr, *pb = nullptr;
        uint32_t pcode = 3u;
        const auto byte_at = [&](int64_t a) -> uint32_t {
            if (a < ls + pf.len) return j.pre_pool[pf.begin + (a - ls)];
            const int64_t x = a - body0;
            if (x >= total) return '\n';
            if (idx < 0 || x >= pend) {
                if (idx < 0) {
                    int l = 0, h = TEXT_TILE;
                    while (h - l > 1) {
                        const int m = (l + h) >> 1;
                        if (s_start[m] <= x) l = m; else h = m;
                    }
                    idx = l;
                } else {
                    idx++;
                }
                pbeg = s_start[idx];
                pend = s_start[idx + 1];
                pcode = s_code[idx];
                if (pcode != 3u) {
                    const int64_t col = col0 + idx;
                    const int64_t o0 = j.al_off[2 * col], o1 = j.al_off[2 * col + 1], o2 = j.al_off[2 * col + 2];
                    pa = j.al_pool + (pcode == 0u ? o1 : o0);
                    la = pcode == 0u ? o2 - o1 : o1 - o0;
                    pb = j.al_pool + (pcode == 2u ? o0 : o1);
                }
            }
            const int64_t k = x - pbeg;
            if (k == 0) return '\t';
            if (pcode == 3u) return k == 2 ? ' ' : '0';
            if (k <= la) return pa[k - 1];
            if (k == la + 1) return ' ';
            return pb[k - la - 2];
        };

        for (int64_t q = sa + TEXT_SEG * (int64_t)tid; q < se; q += TEXT_CHUNK) {
            const int lo = q < ls ? (int)(ls - q) : 0;                           // only the line's first segment
            const int hi = se - q < TEXT_SEG ? (int)(se - q) : TEXT_SEG;         // only the line's last segment
            const int nc = q < ra ? (int)(ra - q) : 0;                           // bytes of the tile before: t > 0, q == sa
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            idx = -1;
#pragma unroll
            for (int i = 0; i < TEXT_SEG; i++) {
                if (i < lo || i >= hi) continue;
                const uint32_t c = (t > 0 && i < nc) ? (uint32_t)s_carry[t & 1][i] : byte_at(q + i);
                v[i >> 2] |= c << (8 * (i & 3));
            }
            store_segment(j.text_al, q, v, lo, hi);
        }
        if (!last && tid < TEXT_SEG && se + tid < rbn) {
            idx = -1;
            s_carry[(t + 1) & 1][tid] = (uint8_t)byte_at(se + tid);
        }
        base += total;
        __syncthreads();
    }
}

int launch_text_fixed(hipStream_t st, const TextJob &j, int64_t n_rows)
{
    hipLaunchKernelGGL(text_fixed_kernel, dim3((unsigned)n_rows), dim3(TEXT_THREADS), 0, st, j);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_text_lengths(hipStream_t st, const TextJob &j, int64_t n_rows, int64_t *len)
{
    hipLaunchKernelGGL(text_lengths_kernel, dim3((unsigned)n_rows), dim3(TEXT_THREADS), 0, st, j, len);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_text_variable(hipStream_t st, const TextJob &j, int64_t n_rows, const int64_t *line_off)
{
    hipLaunchKernelGGL(text_variable_kernel, dim3((unsigned)n_rows), dim3(TEXT_THREADS), 0, st, j, line_off);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
