// The splice of snpgpu_geno_merge (include/snpgpu.h section 1o; host layer: geno_merge.hip): 2-bit rows of several parts side by
// side in one merged row, part i's n_i codes from code off[i] = n_0 + ... + n_(i-1) -- an offset that is in general no multiple of
// 4, let alone of 16 -- with the codes of a flagged row of a part flipped (0 / 1 / 2 / 3 -> 2 / 1 / 0 / 3).  Two bits per genotype
// all the way: a funnel-shifted copy per part (geno_copy_kernel's scheme) ORed together per dword of dst.
// Loads are aligned dwords below SplicePart::n_words; stores are 16 bytes where a lane's four dwords lie inside the row, else
// dwords where dst is aligned and bytes at the ends of a row, all inside the n_rows x rb bytes of dst.
#include "geno_select.h"
#include "geno_select_device.h"

namespace snpgpu {

constexpr int SPLICE_LDS_PARTS = 64;               // up to here the descriptions and offsets of the parts are read from LDS

// 16 codes flipped: 00 -> 10, 01 -> 01, 10 -> 00, 11 -> 11 (the high bit toggles where the low bit is clear)
__device__ __forceinline__ uint32_t splice_flip(uint32_t x) { return x ^ ((~x & 0x55555555u) << 1); }

// thread t = (row k, unit u): unit u of a row is the 16 aligned bytes of dst that start at row byte 16 u - (address of the row & 15),
// four dwords of 16 codes each.  A dword's codes [c, c + 16) of the merged row (those below 0 or from N on belong to no part) are
// gathered part by part: the part of the lane's first code by a search over off, which is the same for every row, then onwards
// while the codes reach into the next part -- three or more parts per dword when parts have fewer than 16 codes.  What a part
// needs per row (its description, the row's bit position and flip byte) is loaded when the lane enters the part, not per dword.
template <bool LDS>
__global__ __launch_bounds__(256) void geno_splice_kernel(const SplicePart *__restrict__ g_parts, const int32_t *__restrict__ g_off,
                                                          int n_parts, int64_t N, int64_t k_first, int64_t n_rows, int64_t rb, int64_t units,
                                                          uint8_t *__restrict__ dst)
{
    __shared__ SplicePart s_parts[LDS ? SPLICE_LDS_PARTS : 1];
    __shared__ int32_t s_off[LDS ? SPLICE_LDS_PARTS + 1 : 1];
    if (LDS) {
        for (int i = threadIdx.x; i <= n_parts; i += 256) {
            s_off[i] = g_off[i];
            if (i < n_parts) s_parts[i] = g_parts[i];
        }
        __syncthreads();
    }
    const SplicePart *parts = LDS ? s_parts : g_parts;
    const int32_t *off = LDS ? s_off : g_off;

    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t kk = t / units;
    if (kk >= n_rows) return;
    const int64_t u = t - kk * units, k = k_first + kk;
    uint8_t *row = dst + k * rb;
    const int64_t i0 = 16 * u - (int64_t)((uintptr_t)row & 15);
    if (i0 >= rb) return;
    const int64_t c0 = 4 * i0, first = c0 < 0 ? 0 : c0;                        // first < N: a byte of the row at or behind i0 holds it
    int p = 0;
    for (int a = 0, b = n_parts; a < b;) {                                     // the last part with off[p] <= first
        const int m = (a + b) >> 1;
        if ((int64_t)off[m] <= first) { p = m; a = m + 1; } else b = m;
    }
    int cur = -1;                                                              // the part whose row is described by q, o, oe, base, fl
    SplicePart q = {};
    int64_t o = 0, oe = 0, base = 0;
    bool fl = false;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t c = c0 + 16 * j, lo = c < 0 ? 0 : c, hi = c + 16 < N ? c + 16 : N;
        uint32_t x = 0u;
        while (lo < hi && p < n_parts) {
            if (cur != p) {
                q = parts[p];
                o = off[p];
                oe = off[p + 1];
                base = q.bit0 + (q.srow ? (int64_t)q.srow[k] : k) * q.stride - 2 * o;      // bit of merged code 0, were the part that long
                fl = q.flip && q.flip[k];
                cur = p;
            }
            if (o >= hi) break;
            const int64_t a = o > lo ? o : lo, e = oe < hi ? oe : hi;
            uint32_t y = sel_fetch32(q.w, q.n_words, base + 2 * a);            // the part's codes from merged code a on
            if (fl) y = splice_flip(y);                                        // before the mask: a neighbour's codes stay as they are
            const uint32_t cnt = (uint32_t)(e - a);                            // 1 ... 16 codes of this part, by count: the padding
            if (cnt < 16u) y &= ~(~0u << (2u * cnt));                          // of its staged row never reaches a neighbour
            x |= y << (2u * (uint32_t)(a - c));
            if (oe > hi) break;                                                // the part goes on in the next dword
            p++;
            if (oe == hi) break;
        }
        v[j] = sel_pad16<3>(x, N - c);
    }
    if (i0 >= 0 && i0 + 16 <= rb) {
        *reinterpret_cast<uint4 *>(row + i0) = make_uint4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) sel_store_unit(row, i0 + 4 * j, rb, v[j]);
}

int launch_geno_splice(hipStream_t st, const SplicePart *parts, const int32_t *off, int n_parts, int64_t N, int64_t n_rows, uint8_t *dst)
{
    const int64_t rb = (N + 3) / 4, units = (rb + 30) / 16;                    // covers every alignment of a row
    const int64_t rows_per = std::max<int64_t>(1, (int64_t(1) << 30) * 256 / units);     // at most 2^30 workgroups per launch
    for (int64_t k0 = 0; k0 < n_rows; k0 += rows_per) {
        const int64_t n = std::min(rows_per, n_rows - k0);
        const dim3 grid((unsigned)((n * units + 255) / 256));
        if (n_parts <= SPLICE_LDS_PARTS)
            hipLaunchKernelGGL(geno_splice_kernel<true>, grid, dim3(256), 0, st, parts, off, n_parts, N, k0, n, rb, units, dst);
        else
            hipLaunchKernelGGL(geno_splice_kernel<false>, grid, dim3(256), 0, st, parts, off, n_parts, N, k0, n, rb, units, dst);
    }
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
