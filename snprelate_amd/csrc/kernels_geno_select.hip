// Selection and layout of genotypes on the device (snpgpu_geno_select, snpgpu_geno_convert, include/snpgpu.h sections 1j and 1k;
// host layer: geno_select.hip): from a 2-bit stream whose rows start at any even bit to byte-aligned 2-bit rows of the selected
// samples and SNPs, in the source's code set or the other one (GDS <-> PLINK BED).  Below a row is a SNP and a column a sample, as
// for dst_major 0; the host layer exchanges the two for dst_major 1.
//   geno_copy_kernel       SNP rows -> SNP rows, consecutive samples: a funnel-shifted copy, one lane per aligned dword of dst
//   geno_gather_kernel     SNP rows -> SNP rows, a sample list: the source rows of a workgroup in LDS, 16 gathered codes per dword
//   geno_transpose_kernel  sample rows -> SNP rows: 64 samples x 1024 SNPs per workgroup through transpose_2bit_64x64
// Loads are aligned dwords below SelBits::n_words, the dwords that hold a byte of the source; stores are dwords where dst is
// aligned and bytes at the ends of a row, all inside the n_rows x rb bytes of dst.
// Every kernel is instantiated per SelRecode as <MAP, PAD>: MAP recodes a finished dword of 16 codes (a map per code commutes with
// the funnel shifts, the gather and transpose_2bit_64x64), PAD is the code of dst's unused codes.  Codes that no source element
// fills are written in the SOURCE's code set as the code MAP sends to PAD (sel_pad_src), so that one map per output dword serves.
#include "geno_select.h"
#include "geno_select_device.h"
#include "prep_device.h"

namespace snpgpu {

__device__ __forceinline__ int64_t sel_row_bit(const SelBits &s, int64_t r) { return s.bit0 + (s.row_bit ? s.row_bit[r] : r * s.stride); }

enum { SEL_MAP_ID = 0, SEL_MAP_BED_GDS = 1, SEL_MAP_GDS_BED = 2 };

// 16 codes recoded: BED -> GDS {2, 3, 1, 0}, GDS -> BED {3, 2, 0, 1}.  The high bit of both is the inverted high bit; the low bit is
// high ^ low, inverted for GDS -> BED.
template <int MAP> __device__ __forceinline__ uint32_t sel_map(uint32_t x)
{
    if (MAP == SEL_MAP_BED_GDS) return (~x & 0xAAAAAAAAu) | ((x ^ (x >> 1)) & 0x55555555u);
    if (MAP == SEL_MAP_GDS_BED) return (~x & 0xAAAAAAAAu) | (~(x ^ (x >> 1)) & 0x55555555u);
    return x;
}

// 16 x the source code that MAP sends to PAD (3 or 0): BED 1 -> GDS 3, BED 3 -> GDS 0, GDS 2 -> BED 0, GDS 0 -> BED 3
template <int MAP, int PAD> __device__ __forceinline__ constexpr uint32_t sel_pad_src()
{
    return MAP == SEL_MAP_BED_GDS ? (PAD == 3 ? 0x55555555u : 0xFFFFFFFFu)
         : MAP == SEL_MAP_GDS_BED ? (PAD == 0 ? 0xAAAAAAAAu : 0u)
                                  : (PAD == 3 ? 0xFFFFFFFFu : 0u);
}

// ---- SNP rows -> SNP rows, samples s0 ... s0 + n_out - 1 ---------------------------------------------------------------------
// thread t = (output row k, unit u): unit u of a row is the aligned dword of dst that starts at row byte 4 u - (address of the row & 3)
template <int MAP, int PAD>
__global__ __launch_bounds__(256) void geno_copy_kernel(SelBits s, const int32_t *__restrict__ srow, int64_t s0, int64_t n_out,
                                                        int64_t n_rows_out, int64_t rb, int64_t units, uint8_t *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = t / units;
    if (k >= n_rows_out) return;
    const int64_t u = t - k * units;
    uint8_t *row = dst + k * rb;
    const int64_t i0 = 4 * u - (int64_t)((uintptr_t)row & 3);
    if (i0 >= rb) return;
    const int64_t p = sel_row_bit(s, srow ? (int64_t)srow[k] : k) + 2 * s0;
    uint32_t v;
    if (i0 >= 0) v = sel_fetch32(s.w, s.n_words, p + 8 * i0);
    else v = sel_fetch32(s.w, s.n_words, p) << (uint32_t)(-8 * i0);           // the row's first bytes in the upper bytes of the unit
    // (code c of the unit is sample s0 + 4 i0 + c; the codes of bytes before the row are never stored)
    sel_store_unit(row, i0, rb, sel_pad16<PAD>(sel_map<MAP>(v), n_out - 4 * i0));
}

// ---- SNP rows -> SNP rows, sample samp[j] at code j ----------------------------------------------------------------------------
// A workgroup takes R consecutive output rows: their source rows go to LDS once (LDS = 0: they stay in global memory, for rows
// that do not fit), and every index is read once for the R rows.
template <int LDS, int MAP, int PAD>
__global__ __launch_bounds__(256) void geno_gather_kernel(SelBits s, const int32_t *__restrict__ srow, const int32_t *__restrict__ samp,
                                                          int64_t n_out, int64_t n_cols, int64_t n_rows_out, int R, int64_t rb,
                                                          uint8_t *__restrict__ dst)
{
    extern __shared__ uint32_t sel_lds[];
    const int64_t k0 = (int64_t)blockIdx.x * R;
    const int64_t nw_max = (2 * n_cols + 31 + 30) >> 5;                        // dwords a row touches at the worst phase
    const uint32_t *src[SEL_GATHER_ROWS];
    uint32_t ph[SEL_GATHER_ROWS];
#pragma unroll
    for (int i = 0; i < SEL_GATHER_ROWS; i++) {
        src[i] = s.w; ph[i] = 0;
        if (i < R && k0 + i < n_rows_out) {
            const int64_t p = sel_row_bit(s, srow ? (int64_t)srow[k0 + i] : k0 + i);
            src[i] = s.w + (p >> 5);
            ph[i] = (uint32_t)p & 31u;
            if (LDS) {
                const int64_t nw = ((int64_t)ph[i] + 2 * n_cols + 31) >> 5, left = s.n_words - (p >> 5);
                for (int64_t d = threadIdx.x; d < nw; d += 256) sel_lds[i * nw_max + d] = d < left ? src[i][d] : 0u;
            }
        }
    }
    if (LDS) __syncthreads();
    const int64_t units = (rb + 6) / 4;                                        // covers every alignment of a row
    for (int64_t u = threadIdx.x; u < units; u += 256) {
        // the 16 indices of row bytes 4 u ... 4 u + 3, shared by the R rows; a row whose address is not a multiple of 4 shifts them
        // by whole bytes, so units are taken on the ROW's bytes here and aligned per row below
        uint32_t v[SEL_GATHER_ROWS];
#pragma unroll
        for (int i = 0; i < SEL_GATHER_ROWS; i++) v[i] = 0u;
        const int64_t j0 = 16 * u;
        int32_t idx[16];
        if (j0 + 16 <= n_out) {                                                // 64 aligned bytes of the list
            const int4 *q = reinterpret_cast<const int4 *>(samp + j0);
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int4 a = q[t];
                idx[4 * t] = a.x; idx[4 * t + 1] = a.y; idx[4 * t + 2] = a.z; idx[4 * t + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 16; c++) idx[c] = j0 + c < n_out ? samp[j0 + c] : -1;
        }
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const int64_t smp = idx[c];
#pragma unroll
            for (int i = 0; i < SEL_GATHER_ROWS; i++) {
                if (i >= R) break;
                uint32_t code = sel_pad_src<MAP, PAD>() & 3u;                  // an absent index: dst's padding after the map
                if (smp >= 0) {
                    const int64_t q = (int64_t)ph[i] + 2 * smp;
                    const uint32_t wv = LDS ? sel_lds[i * nw_max + (q >> 5)] : src[i][q >> 5];
                    code = (wv >> ((uint32_t)q & 31u)) & 3u;
                }
                v[i] |= code << (2 * c);
            }
        }
#pragma unroll
        for (int i = 0; i < SEL_GATHER_ROWS; i++) {
            if (i >= R || k0 + i >= n_rows_out) break;
            uint8_t *row = dst + (k0 + i) * rb;
            const int64_t i0 = 4 * u;
            if (i0 >= rb) break;
            const uint32_t o = sel_map<MAP>(v[i]);
            if (((uintptr_t)(row + i0) & 3) == 0) sel_store_unit(row, i0, rb, o);
            else
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (i0 + b < rb) row[i0 + b] = (uint8_t)(o >> (8 * b));
        }
    }
}

// ---- sample rows -> SNP rows ---------------------------------------------------------------------------------------------------
// 16 bytes x (the codes of 64 samples of one SNP) to p, any alignment, the first nbytes of them
__device__ __forceinline__ void sel_store16(uint8_t *__restrict__ p, const uint32_t (&x)[4], int nbytes)
{
    const int a = (int)((uintptr_t)p & 3);
    if (nbytes == 16 && a == 0) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
        q[0] = x[0]; q[1] = x[1]; q[2] = x[2]; q[3] = x[3];
    } else if (nbytes == 16) {
        const int h = 4 - a;                                                   // bytes up to the next dword of dst
        for (int b = 0; b < h; b++) p[b] = (uint8_t)(x[0] >> (8 * b));
        uint32_t *q = reinterpret_cast<uint32_t *>(p + h);
        const uint32_t sh = 8u * (uint32_t)h;
#pragma unroll
        for (int i = 0; i < 3; i++) q[i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], sh);
        for (int b = 0; b < a; b++) p[h + 12 + b] = (uint8_t)(x[3] >> (8 * (h + b)));
    } else {
#pragma unroll
        for (int b = 0; b < 16; b++)
            if (b < nbytes) p[b] = (uint8_t)(x[b >> 2] >> (8 * (b & 3)));
    }
}

// Workgroup = (segment of <= SEL_TW consecutive SNPs, block of 64 output samples).  Read side as load_tile_64
// (kernels_transpose.hip): a wave's loads read contiguous bytes of ONE sample row -- per lane one dword load and, only when the row's
// phase is not 0 and the next dword belongs to the source, a second one (sel_fetch32: two 4-byte loads, not one 8-byte load),
// funnel-shifted to the phase, so that the LDS tile holds 16 SNPs per dword from the segment's first SNP -- and the waves pick
// their 64 x 64 sub-tiles from LDS.  lane = sample on the read side, SNP on the write side.  Samples >= n_out are rows of the code that
// becomes PAD (the padding of the last byte); SNPs beyond the segment are not stored.
template <int MAP, int PAD>
__global__ __launch_bounds__(256) void geno_transpose_kernel(SelBits s, const int32_t *__restrict__ samp, const SelSeg *__restrict__ segs,
                                                             int64_t n_sblk, int64_t n_out, int64_t rb, uint8_t *__restrict__ dst)
{
    __shared__ uint32_t tile[64][SEL_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t sblk = (int64_t)blockIdx.x % n_sblk;
    const SelSeg g = segs[(int64_t)blockIdx.x / n_sblk];
    const int nd = (g.len + 15) >> 4;                                          // dwords of 16 SNPs that hold one of the segment
    for (int r = wave; r < 64; r += 4) {
        const int64_t j = 64 * sblk + r;
        uint32_t v = sel_pad_src<MAP, PAD>();
        if (j < n_out && lane < nd)
            v = sel_fetch32(s.w, s.n_words, sel_row_bit(s, samp ? (int64_t)samp[j] : j) + 2 * (int64_t)g.c + 32 * lane);
        tile[r][lane] = v;
    }
    __syncthreads();
    const int64_t jb = 16 * sblk;                                              // row byte of this block of samples
    const int nbytes = (int)(rb - jb < 16 ? rb - jb : 16);
    for (int cc = wave; 64 * cc < g.len; cc += 4) {
        const uint4 q = *reinterpret_cast<const uint4 *>(&tile[lane][4 * cc]);
        uint32_t x[4] = {q.x, q.y, q.z, q.w};
        transpose_2bit_64x64(x, lane);                                         // lane = SNP now: x = the codes of the 64 samples
        if constexpr (MAP != SEL_MAP_ID) {
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = sel_map<MAP>(x[i]);
        }
        const int e = 64 * cc + lane;
        if (e < g.len) sel_store16(dst + ((int64_t)g.k + e) * rb + jb, x, nbytes);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
namespace {

template <int MAP, int PAD>
int copy_launch(hipStream_t st, const SelBits &s, const int32_t *srow, int64_t s0, int64_t n_out, int64_t n_rows_out, uint8_t *dst)
{
    const int64_t rb = (n_out + 3) / 4, units = (rb + 6) / 4;
    const int64_t rows_per = std::max<int64_t>(1, (int64_t(1) << 30) * 256 / units);     // at most 2^30 workgroups per launch
    for (int64_t k0 = 0; k0 < n_rows_out; k0 += rows_per) {
        const int64_t n = std::min(rows_per, n_rows_out - k0);
        SelBits w = s;
        if (!srow) { if (w.row_bit) w.row_bit += k0; else w.bit0 += k0 * w.stride; }
        hipLaunchKernelGGL((geno_copy_kernel<MAP, PAD>), dim3((unsigned)((n * units + 255) / 256)), dim3(256), 0, st, w,
                           srow ? srow + k0 : nullptr, s0, n_out, n, rb, units, dst + k0 * rb);
    }
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int MAP, int PAD>
int gather_launch(hipStream_t st, const SelBits &s, const int32_t *srow, const int32_t *samp, int64_t n_out, int64_t n_cols,
                  int64_t n_rows_out, int64_t lds_words, uint8_t *dst)
{
    const int64_t rb = (n_out + 3) / 4, nw_max = (2 * n_cols + 61) >> 5;
    const bool lds = nw_max <= lds_words;
    const int R = (int)std::max<int64_t>(1, std::min<int64_t>(SEL_GATHER_ROWS, lds ? lds_words / nw_max : SEL_GATHER_ROWS));
    const int64_t groups = (n_rows_out + R - 1) / R;
    if (groups >= (int64_t(1) << 31)) { set_error("snpgpu_geno_convert: too many rows for one launch"); return 1; }
    if (lds)
        hipLaunchKernelGGL((geno_gather_kernel<1, MAP, PAD>), dim3((unsigned)groups), dim3(256), (size_t)(R * nw_max) * 4, st, s, srow, samp,
                           n_out, n_cols, n_rows_out, R, rb, dst);
    else
        hipLaunchKernelGGL((geno_gather_kernel<0, MAP, PAD>), dim3((unsigned)groups), dim3(256), 0, st, s, srow, samp, n_out, n_cols,
                           n_rows_out, R, rb, dst);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int MAP, int PAD>
int transpose_launch(hipStream_t st, const SelBits &s, const int32_t *samp, const SelSeg *segs, int64_t n_segs, int64_t n_out, uint8_t *dst)
{
    const int64_t rb = (n_out + 3) / 4, n_sblk = (n_out + 63) / 64;
    const int64_t per = std::max<int64_t>(1, (int64_t(1) << 30) / n_sblk);              // segments per launch
    for (int64_t g0 = 0; g0 < n_segs; g0 += per) {
        const int64_t n = std::min(per, n_segs - g0);
        hipLaunchKernelGGL((geno_transpose_kernel<MAP, PAD>), dim3((unsigned)(n * n_sblk)), dim3(256), 0, st, s, samp, segs + g0, n_sblk,
                           n_out, rb, dst);
    }
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

// the instantiation <MAP, PAD> of a SelRecode
#define SEL_DISPATCH(rc, fn, ...)                                      \
    switch (rc) {                                                      \
    case SEL_GDS_GDS: return fn<SEL_MAP_ID, 3>(__VA_ARGS__);           \
    case SEL_BED_BED: return fn<SEL_MAP_ID, 0>(__VA_ARGS__);           \
    case SEL_BED_GDS: return fn<SEL_MAP_BED_GDS, 3>(__VA_ARGS__);      \
    default:          return fn<SEL_MAP_GDS_BED, 0>(__VA_ARGS__);      \
    }

int launch_geno_copy(hipStream_t st, const SelBits &s, const int32_t *srow, int64_t s0, int64_t n_out, int64_t n_rows_out, uint8_t *dst,
                     SelRecode rc)
{
    SEL_DISPATCH(rc, copy_launch, st, s, srow, s0, n_out, n_rows_out, dst)
}

int launch_geno_gather(hipStream_t st, const SelBits &s, const int32_t *srow, const int32_t *samp, int64_t n_out, int64_t n_cols,
                       int64_t n_rows_out, int64_t lds_words, uint8_t *dst, SelRecode rc)
{
    SEL_DISPATCH(rc, gather_launch, st, s, srow, samp, n_out, n_cols, n_rows_out, lds_words, dst)
}

int launch_geno_transpose(hipStream_t st, const SelBits &s, const int32_t *samp, const SelSeg *segs, int64_t n_segs, int64_t n_out,
                          uint8_t *dst, SelRecode rc)
{
    SEL_DISPATCH(rc, transpose_launch, st, s, samp, segs, n_segs, n_out, dst)
}

}  // namespace snpgpu
