// SNP-major 2-bit rows -> sample-major words (HBM-bound; launched by feed_counters and feed_syrk, ctx_feed.hip, and proj.hip):
//   transpose8        pair-coded words for the SYRK kernels
//   transpose2<0/1>   2-bit words for the MFMA pair kernels (<1>: the missing mask of the GCTA denominators, + miss_diag2)
//   transpose2_direct the same words straight from a caller block of 2-bit rows (+ het_commit)
//   bitplanes<0/1>    bit planes for the popcount pair kernel
//               (the role of PackSNPGeno1b, src/dGenGWAS.cpp:1429-1475, with a 4-plane encoding)
//   missmask256 / miss_route   256-sample sets of missing calls for the sparse GCTA denominators
// transpose8 / transpose2* share the block-swap transposition transpose_2bit_64x64 and the LDS tile of load_tile_64.
#include "snpgpu_internal.h"
#include "prep_device.h"

namespace snpgpu {

// ---------------------------------------------------------------------------
// bitplanes: each wave owns 64 SNPs (one per lane on the read side) x 64 samples.
// Lane l reads the 16 bytes holding samples s0..s0+63 of SNP k0+l; for every sample s a wave
// ballot of "code(s) has property P" is the 64-SNP plane word of that sample, which lane s keeps
// (lane = sample on the write side).  Planes per sample:
//   V = call present, H = heterozygous (g==1), O = g==0, T = g==2      (all zero when missing)
// so that the pair kernel needs 8 (IBS) / 11 (KING) bit-ops per 32 SNP pairs.
// Output word index kw = snp/32; planes of one (sample, kw) are one uint4 {V,H,O,T}.
template <int MISS_ONLY>
__global__ __launch_bounds__(256) void bitplanes_kernel(const uint8_t *__restrict__ packed, int64_t RB,
                                                        int64_t n_snp, int64_t N, const int32_t *__restrict__ sum,
                                                        const int32_t *__restrict__ num, int64_t col0,
                                                        int64_t ncols_pad, int64_t rows_pad, int KW,
                                                        void *__restrict__ rowp_, void *__restrict__ colp_,
                                                        const unsigned long long *__restrict__ d_skip_if_zero)
{
    if (MISS_ONLY && d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t k0 = ((int64_t)blockIdx.y * 4 + wave) * 64;  // first SNP of this wave
    if (k0 >= (int64_t)KW * 32) return;
    const int64_t sc0 = (int64_t)blockIdx.x * 64;              // first column sample (panel relative)
    const int64_t s0 = col0 + sc0;                             // absolute sample
    const int64_t k = k0 + lane;
    uint4 q = make_uint4(~0u, ~0u, ~0u, ~0u);
    bool poly = false;
    if (k < n_snp) {
        if (s0 < RB * 4) q = *reinterpret_cast<const uint4 *>(packed + k * RB + (s0 >> 2));
        if (MISS_ONLY) {
            const int s = sum[k], c = num[k];
            poly = (0 < s) && (s < 2 * c);
        }
    }
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t r0[4] = {0, 0, 0, 0}, r1[4] = {0, 0, 0, 0};  // lo (SNP k0..k0+31) / hi (k0+32..) words, planes V,H,O,T
#pragma unroll
    for (int ws = 0; ws < 4; ws++) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int s = ws * 16 + j;
            const uint32_t code = (w[ws] >> (2 * j)) & 3u;
            const bool mine = (lane == s);
            if (MISS_ONLY) {
                // plane 0: missing call at a polymorphic SNP, real samples only (genPCA.cpp:1201-1224)
                const bool in_range = (s0 + s) < N;
                const unsigned long long m = __ballot(code == 3u && poly && in_range);
                if (mine) { r0[0] = (uint32_t)m; r1[0] = (uint32_t)(m >> 32); }
            } else {
                const unsigned long long mv = __ballot(code != 3u);
                const unsigned long long mh = __ballot(code == 1u);
                const unsigned long long mo = __ballot(code == 0u);
                const unsigned long long mt = __ballot(code == 2u);
                if (mine) {
                    r0[0] = (uint32_t)mv; r1[0] = (uint32_t)(mv >> 32);
                    r0[1] = (uint32_t)mh; r1[1] = (uint32_t)(mh >> 32);
                    r0[2] = (uint32_t)mo; r1[2] = (uint32_t)(mo >> 32);
                    r0[3] = (uint32_t)mt; r1[3] = (uint32_t)(mt >> 32);
                }
            }
        }
    }
    const int kw0 = (int)(k0 >> 5);
    const int64_t sc = sc0 + lane;  // panel-relative sample of this lane
    if (MISS_ONLY) {
        uint2 *rowp = (uint2 *)rowp_;
        uint2 *colp = (uint2 *)colp_;
        const int kp = kw0 >> 1;  // uint2 = two consecutive 32-SNP words
        colp[(int64_t)kp * ncols_pad + sc] = make_uint2(r0[0], r1[0]);
        if (sc < rows_pad) rowp[((sc >> 3) * (KW >> 1) + kp) * 8 + (sc & 7)] = make_uint2(r0[0], r1[0]);
    } else {
        uint4 *rowp = (uint4 *)rowp_;
        uint4 *colp = (uint4 *)colp_;
        const uint4 a = make_uint4(r0[0], r0[1], r0[2], r0[3]);
        const uint4 b = make_uint4(r1[0], r1[1], r1[2], r1[3]);
        colp[(int64_t)kw0 * ncols_pad + sc] = a;
        colp[(int64_t)(kw0 + 1) * ncols_pad + sc] = b;
        if (sc < rows_pad) {
            // [row group of 8][word][8 rows]: the pair kernel's wave reads 8 rows of one word at once
            rowp[((sc >> 3) * KW + kw0) * 8 + (sc & 7)] = a;
            rowp[((sc >> 3) * KW + kw0 + 1) * 8 + (sc & 7)] = b;
        }
    }
}

// (transpose_2bit_64x64, the block-swap transposition of a 64 x 64 tile spread over a wave: prep_device.h)

// Read side of the transposition kernels: a workgroup takes 64 SNPs (or slots) x TR_SAMPLES samples of the repacked block
// (rows of RB bytes, a multiple of 64, samples >= N already code 3).  Every wave instruction reads 256 contiguous bytes of ONE
// row (lane = 16 samples) into the LDS tile; the waves then pick their 64 x 64 sub-tiles from it with one 16-byte read per lane.
// (Before, a lane read 16 bytes of its own row: 64 cache lines per load instruction, which -- not the bit work -- set the time.)
// row_of(r) = row of `packed` for tile row r, or -1 for a row of `fill`.
constexpr int TR_SAMPLES = 1024;
constexpr int TR_PITCH = TR_SAMPLES / 16 + 4;         // dwords per tile row (16-byte aligned)
// grid of a transposition kernel: TR_SAMPLES samples x 64 SNPs (slots) per workgroup
static dim3 transpose_grid(int64_t ncols_pad, int n_snp64) { return dim3((unsigned)((ncols_pad + TR_SAMPLES - 1) / TR_SAMPLES), (unsigned)n_snp64); }
template <typename RowOf>
__device__ __forceinline__ void load_tile_64(uint32_t (*tile)[TR_PITCH], const uint8_t *__restrict__ packed, int64_t RB,
                                             int64_t s_first, uint32_t fill, RowOf row_of)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (s_first >> 2) + 4 * lane;        // byte offset of this lane's dword in a row
    for (int r = wave; r < 64; r += 4) {
        const int64_t k = row_of(r);
        tile[r][lane] = (k >= 0 && b + 4 <= RB) ? *reinterpret_cast<const uint32_t *>(packed + k * RB + b) : fill;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// transpose8: SNP-major 2-bit rows -> sample-major PAIR-coded words for the SYRK kernel.
//   W8[d][sample] (uint32) covers SNPs 8d .. 8d+7 of that sample: byte p = 8 * (c0 + 4*c1) with
//   c0/c1 the codes of SNPs 8d+2p / 8d+2p+1, i.e. the byte offset of the pair's float2 table entry:
//   ONE v_add_u32_sdwa (table address = base + byte) per two genotypes, no shift/mask.
// Block-swap transposition (transpose_2bit_64x64): lane = SNP on the read side, lane = sample on the write side.
// d_wide16 != nullptr and *d_wide16 == 0 (a block without missing calls in a context with the exact-row SYRK): the
// byte is 16 * (c0 + 4*c1), the offset of a 16-byte table entry.
__global__ __launch_bounds__(256) void transpose8_kernel(const uint8_t *__restrict__ packed, int64_t RB,
                                                         int64_t n_snp, int64_t col0, int64_t ncols_pad,
                                                         int n_d, uint32_t *__restrict__ w8,
                                                         const unsigned long long *__restrict__ d_wide16, int layout,
                                                         const int32_t *__restrict__ slot_src, int nibble_nomiss)
{
    // bytes carry the table offset of the pair's entry; layout is a WordLayout (snpgpu_internal.h):
    // Entry8Or16 / Entry16: 8 / 16 * code;  Entry12: 12 * code
    // Entry12Or8: 12 * code, or 8 * code in a block without missing calls (syrk_uv_kernel: 8-byte entries)
    // Entry12Missing: 12 * code, and only for a block WITH missing calls (EIGMIX: a second word array for the exact-row
    // kernel next to the 8 * code words its other tables read)
    // nibble_nomiss (syrk_uv16c_kernel, Entry12Or8): in a block without missing calls byte p = c0 | c1 << 4 -- two e2m1 nibbles
    // of value c / 2 that v_cvt_scalef32_pk_f16_fp4 turns into an fp16 pair, no table
    constexpr int L8Or16 = (int)WordLayout::Entry8Or16, L12 = (int)WordLayout::Entry12, L12Or8 = (int)WordLayout::Entry12Or8,
                  L12Missing = (int)WordLayout::Entry12Missing;
    if (layout == L12Missing && *d_wide16 == 0ull) return;
    const bool nib = nibble_nomiss && layout == L12Or8 && *d_wide16 == 0ull;
    const uint32_t mul = (layout == L12Or8) ? ((*d_wide16 == 0ull) ? 8u : 12u)
                         : (layout == L12 || layout == L12Missing) ? 12u : (layout != L8Or16 || (d_wide16 && *d_wide16 == 0ull)) ? 16u : 8u;
    __shared__ uint32_t tile[64][TR_PITCH];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t k0 = (int64_t)blockIdx.y * 64;
    if (k0 >= (int64_t)n_d * 8) return;
    const int64_t sc_wg = (int64_t)blockIdx.x * TR_SAMPLES;
    // the K dimension of a block without missing calls that runs as several fp32 runs is a list of SLOTS (uv_assign_kernel deals
    // the SNPs to the runs): slot_src maps them to the block's SNPs (-1: empty)
    const bool slots = slot_src && layout == L12Or8 && *d_wide16 == 0ull;
    load_tile_64(tile, packed, RB, col0 + sc_wg, ~0u, [&](int r) -> int64_t {
        const int64_t k = k0 + r;
        return slots ? (int64_t)slot_src[k] : (k < n_snp ? k : (int64_t)-1);
    });
    const int d0 = (int)(k0 >> 3);
    for (int cc = wave; cc < TR_SAMPLES / 64; cc += 4) {
        const int64_t sc = sc_wg + 64 * cc + lane;
        if (sc - lane >= ncols_pad) break;
        const uint4 q = *reinterpret_cast<const uint4 *>(&tile[lane][4 * cc]);
        uint32_t x[4] = {q.x, q.y, q.z, q.w};
        transpose_2bit_64x64(x, lane);               // lane = sample now: x = the codes of the 64 SNPs (slots)
#pragma unroll
        for (int g = 0; g < 8; g++) {   // 8 SNPs = 4 pairs per output word: nibble p = c0 + 4 c1 of pair p -> byte p = nibble * mul
            uint32_t v = (x[g >> 1] >> (16 * (g & 1))) & 0xFFFFu;
            v = (v | (v << 8)) & 0x00FF00FFu;
            v = (v | (v << 4)) & 0x0F0F0F0Fu;
            w8[(int64_t)(d0 + g) * ncols_pad + sc] = nib ? ((v & 0x03030303u) | ((v & 0x0C0C0C0Cu) << 2))
                                                         : v * mul;  // 15 * 16 < 256: no carry between the bytes
        }
    }
}

int launch_transpose8(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t col0, int64_t ncols_pad,
                      const Transpose8Opts &o)
{
    hipLaunchKernelGGL(transpose8_kernel, transpose_grid(ncols_pad, (o.n_d + 7) / 8), dim3(256), 0, st, packed, RB, n_snp, col0, ncols_pad,
                       o.n_d, o.w8, o.d_block_flag, (int)o.layout, o.slot_src, o.nibble_nomiss ? 1 : 0);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// sample-major 2-bit words for the MFMA pair kernels: W2[d / 2][sample][d & 1] = codes of SNPs 16d .. 16d+15
// (code m at bits 2m), same block-swap transposition as above; SNPs >= n_snp and samples >= N are 3
// (missing -> every operand value 0).
__device__ __forceinline__ uint32_t spread16(uint32_t x)
{
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// MASK = 1 (GCTA denominators): code 3 only for "missing call at a polymorphic SNP of a real sample"
// (genPCA.cpp:1201-1224), every other cell 0; exits when the block holds no missing call.
template <int MASK>
__global__ __launch_bounds__(256) void transpose2_kernel(const uint8_t *__restrict__ packed, int64_t RB,
                                                         int64_t n_snp, int64_t col0, int64_t ncols_pad,
                                                         int n_d, uint32_t *__restrict__ w2, int64_t N,
                                                         const int32_t *__restrict__ sum, const int32_t *__restrict__ num,
                                                         const unsigned long long *__restrict__ d_skip_if_zero,
                                                         uint32_t *__restrict__ het, int classic)
{
    if (MASK && d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    __shared__ uint32_t tile[64][TR_PITCH];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t k0 = (int64_t)blockIdx.y * 64;
    if (k0 >= (int64_t)n_d * 16) return;
    const int64_t sc_wg = (int64_t)blockIdx.x * TR_SAMPLES;
    load_tile_64(tile, packed, RB, col0 + sc_wg, MASK ? 0u : ~0u, [&](int r) -> int64_t {
        const int64_t k = k0 + r;
        if (k >= n_snp) return -1;
        if (MASK) {                                  // only polymorphic SNPs count (genPCA.cpp:1206)
            const int s = sum[k], c = num[k];
            if (!((0 < s) && (s < 2 * c))) return -1;
        }
        return k;
    });
    const int d0 = (int)(k0 >> 4);
    for (int cc = wave; cc < TR_SAMPLES / 64; cc += 4) {
        const int64_t sc0 = sc_wg + 64 * cc;
        if (sc0 >= ncols_pad) break;
        const uint4 q = *reinterpret_cast<const uint4 *>(&tile[lane][4 * cc]);
        uint32_t x[4] = {q.x, q.y, q.z, q.w};
        if (MASK) {
            // code 3 only where a real sample has a missing call (at a polymorphic SNP: the others were loaded as 0), 0 elsewhere
            const int64_t rem = N - (col0 + sc0);    // samples of this 64-chunk that exist
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint32_t m3 = code3_below(x[t], rem - 16 * t);
                x[t] = m3 | (m3 << 1);
            }
        }
        transpose_2bit_64x64(x, lane);               // lane = sample now
        const int64_t sc = sc0 + lane;
        if (classic) {   // W2[d][sample]: the projection kernels (lane = SNP) read it
#pragma unroll
            for (int t = 0; t < 4; t++) w2[(int64_t)(d0 + t) * ncols_pad + sc] = x[t];
        } else {   // word rows 2 r and 2 r + 1 of a sample lie side by side (W2 = uint2[row pair][sample]): one 8-byte load per 32 SNPs
            uint2 *__restrict__ w2p = reinterpret_cast<uint2 *>(w2);
            w2p[(int64_t)(d0 >> 1) * ncols_pad + sc] = make_uint2(x[0], x[1]);
            w2p[(int64_t)((d0 >> 1) + 1) * ncols_pad + sc] = make_uint2(x[2], x[3]);
        }
        // per-sample het counts of a block WITHOUT missing calls: the rank-one terms of the binary pair kernel
        // (I8Scheme<PM_IBS_NOMISS>); d_skip_if_zero is the block's missing-call flag here
        // (het[0 .. ncols_pad) = #het, het[ncols_pad .. 2 ncols_pad) = #(g == 2))
        if (!MASK && het && *d_skip_if_zero == 0ull) {
            uint32_t c = 0, t2 = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                c += (uint32_t)__popc(x[t] & ~(x[t] >> 1) & GENO_LO_BITS);
                t2 += (uint32_t)__popc(~x[t] & (x[t] >> 1) & GENO_LO_BITS);
            }
            if (c) atomicAdd(het + sc, c);
            if (t2) atomicAdd(het + ncols_pad + sc, t2);
        }
    }
}

// per-sample number of code-3 cells of the masked words, added to diag[col0 + sample] (M(s,s) of the GCTA denominators)
__global__ __launch_bounds__(256) void miss_diag2_kernel(const uint32_t *__restrict__ w2, int n_d, int64_t ncols_pad,
                                                         int64_t col0, uint32_t *__restrict__ diag,
                                                         const unsigned long long *__restrict__ d_skip_if_zero)
{
    if (d_skip_if_zero && *d_skip_if_zero == 0ull) return;
    const int64_t sc = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sc >= ncols_pad) return;
    uint32_t c = 0;
    const uint2 *__restrict__ w2p = reinterpret_cast<const uint2 *>(w2);      // n_d is even (blocks padded to >= 128 SNPs)
    for (int d = 0; d < n_d / 2; d++) {
        const uint2 w = w2p[(int64_t)d * ncols_pad + sc];
        c += __popc(code3_mask(w.x)) + __popc(code3_mask(w.y));
    }
    diag[col0 + sc] += c;
}

// The pre-pass of the IBS / KING counters in ONE pass over a caller block of 2-bit rows (SNPGPU_GENO_PACKED2): the same
// block-swap transposition as transpose2_kernel<0>, read straight from the caller's rows (row stride ceil(N/4) bytes, dword
// loads; samples >= N and SNPs >= n_snp become code 3), plus the two things the statistics pass delivered to these kinds:
// the block's "holds missing calls" flag and -- into a per-block buffer, committed by het_commit_kernel once the flag is
// final -- the per-sample het counts of a block without missing calls.  Saves one write and one read of the block
// (repack_stats_kernel + transpose2_kernel: 0.40 ms per 65 536-SNP block at N = 10 000, 8 % of an IBS step).
// Read side (round 3): a workgroup takes 64 SNPs x TR_SAMPLES samples; every wave instruction reads 256 contiguous bytes of ONE
// row (lane = 16 samples) into an LDS tile, and the waves then pick their 64 x 64 sub-tiles from it.  (Before, a lane read 16
// bytes of its own row -- 64 cache lines per load instruction: 241 us per 65 536-SNP block at N = 10 000 whatever the
// transposition cost.)
__global__ __launch_bounds__(256) void transpose2_direct_kernel(const uint8_t *__restrict__ src, int64_t rb_in, int64_t N,
                                                                int64_t n_snp, int64_t col0, int64_t ncols_pad, int n_d,
                                                                uint32_t *__restrict__ w2, uint32_t *__restrict__ het_blk,
                                                                unsigned long long *__restrict__ d_missing)
{
    __shared__ uint32_t tile[64][TR_PITCH];                // [SNP][dword of 16 samples], pitch 68 dwords (16-byte aligned rows)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t k0 = (int64_t)blockIdx.y * 64;
    if (k0 >= (int64_t)n_d * 16) return;
    const int64_t sc_wg = (int64_t)blockIdx.x * TR_SAMPLES;      // panel-relative first sample of the workgroup
    const int64_t sd = col0 + sc_wg + 16 * lane;                 // first sample of this lane's dword (byte offset sd / 4)
    for (int r = wave; r < 64; r += 4) {
        const int64_t k = k0 + r;
        uint32_t v = ~0u;                                        // samples >= N and SNPs >= n_snp: code 3
        if (k < n_snp && sd < N) {
            const uint8_t *row = src + k * rb_in;
            const int64_t b = sd >> 2;
            if (b + 4 <= rb_in) v = *reinterpret_cast<const uint32_t *>(row + b);          // rb_in % 4 == 0 (launcher)
            else
                for (int e = 0; e < 4; e++)
                    if (b + e < rb_in) v = (v & ~(0xFFu << (8 * e))) | ((uint32_t)row[b + e] << (8 * e));
            const int64_t rem = N - sd;                          // samples of this dword that exist
            if (rem < 16) v |= ~0u << (2 * rem);
        }
        tile[r][lane] = v;
    }
    __syncthreads();
    const int64_t n_real = n_snp - k0;               // real SNPs among the workgroup's 64
    for (int cc = wave; cc < TR_SAMPLES / 64; cc += 4) {
        const int64_t sc0 = sc_wg + 64 * cc;
        if (sc0 >= ncols_pad) break;
        const uint4 q = *reinterpret_cast<const uint4 *>(&tile[lane][4 * cc]);
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
        transpose_2bit_64x64(w, lane);               // lane = sample now: w = the codes of the 64 SNPs
        const int64_t sc = sc0 + lane;
        const int d0 = (int)(k0 >> 4);
        {
            uint2 *__restrict__ w2p = reinterpret_cast<uint2 *>(w2);          // row pairs side by side, as transpose2_kernel
            w2p[(int64_t)(d0 >> 1) * ncols_pad + sc] = make_uint2(w[0], w[1]);
            w2p[(int64_t)((d0 >> 1) + 1) * ncols_pad + sc] = make_uint2(w[2], w[3]);
        }
        // a missing call = code 3 of a real sample at a real SNP (codes of SNPs >= n_snp are padding)
        uint32_t any3 = 0, c = 0, t2 = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            any3 |= code3_below(w[t], n_real - 16 * t);
            c += (uint32_t)__popc(w[t] & ~(w[t] >> 1) & GENO_LO_BITS);
            t2 += (uint32_t)__popc(~w[t] & (w[t] >> 1) & GENO_LO_BITS);
        }
        if (col0 + sc >= N) any3 = 0u;
        if (__ballot(any3 != 0u) && lane == 0) *d_missing = 1ull;       // only ever tested against zero
        if (het_blk) {
            if (c) atomicAdd(het_blk + sc, c);
            if (t2) atomicAdd(het_blk + ncols_pad + sc, t2);
        }
    }
}

// het[j] += het_blk[j] if the block held no missing call (the binary pair kernel took it); het_blk is cleared either way
__global__ __launch_bounds__(256) void het_commit_kernel(uint32_t *__restrict__ het, uint32_t *__restrict__ het_blk,
                                                         int64_t ncols_pad, const unsigned long long *__restrict__ d_missing)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= 2 * ncols_pad) return;                   // #het, then #(g == 2)
    const uint32_t v = het_blk[j];
    if (v) {
        if (*d_missing == 0ull) het[j] += v;
        het_blk[j] = 0u;
    }
}

int launch_transpose2_direct(hipStream_t st, const uint8_t *src, int64_t n_samp, int64_t n_snp, int64_t col0,
                             int64_t ncols_pad, int n_d, uint32_t *w2, uint32_t *het, uint32_t *het_blk,
                             unsigned long long *d_missing)
{
    const int64_t rb_in = (n_samp + 3) / 4;
    // (n_d * 16 SNPs in groups of 64)
    hipLaunchKernelGGL(transpose2_direct_kernel, transpose_grid(ncols_pad, (n_d + 3) / 4), dim3(256), 0, st, src, rb_in, n_samp, n_snp, col0, ncols_pad, n_d, w2,
                       het ? het_blk : nullptr, d_missing);
    if (het)
        hipLaunchKernelGGL(het_commit_kernel, dim3((unsigned)((2 * ncols_pad + 255) / 256)), dim3(256), 0, st, het, het_blk, ncols_pad,
                           d_missing);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_transpose2(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t col0,
                      int64_t ncols_pad, int n_d, uint32_t *w2, uint32_t *het, const unsigned long long *d_missing, bool classic)
{
    hipLaunchKernelGGL(transpose2_kernel<0>, transpose_grid(ncols_pad, (n_d + 3) / 4), dim3(256), 0, st, packed, RB, n_snp, col0, ncols_pad, n_d, w2,
                       (int64_t)0, (const int32_t *)nullptr, (const int32_t *)nullptr, d_missing, het, classic ? 1 : 0);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_transpose2_missmask(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                               const int32_t *sum, const int32_t *num, int64_t col0, int64_t ncols_pad, int n_d,
                               uint32_t *w2, uint32_t *diag, const unsigned long long *d_skip_if_zero)
{
    hipLaunchKernelGGL(transpose2_kernel<1>, transpose_grid(ncols_pad, (n_d + 3) / 4), dim3(256), 0, st, packed, RB, n_snp, col0, ncols_pad, n_d, w2, n_samp,
                       sum, num, d_skip_if_zero, (uint32_t *)nullptr, 0);
    hipLaunchKernelGGL(miss_diag2_kernel, dim3((unsigned)((ncols_pad + 255) / 256)), dim3(256), 0, st, w2, n_d, ncols_pad,
                       col0, diag, d_skip_if_zero);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// GCTA denominators, sparse form (round 4).  The both-missing counts M(i, j) = #{polymorphic SNPs where i AND j are missing}
// are a dense N^2 B contraction for the int8 kernel (81 ms per 32 768-SNP block at N = 100 000, 15 % of the step) whatever the
// missing rate f -- but only f^2 of its products are non-zero.  missmask256_kernel writes, per SNP and group of 256 samples, the
// 256-bit set of samples with a missing call (SNP-major 2-bit rows in, MM[group][snp][8 dwords] out; monomorphic / all-missing
// SNPs, which GCTA does not count -- src/genPCA.cpp:1206 --, and the sample padding give empty sets); pair_sparse_miss_kernel
// (kernels_pair.hip) walks a 256 x 256 tile's two lists of sets and counts the pairs in LDS.
__global__ __launch_bounds__(256) void missmask256_kernel(const uint8_t *__restrict__ packed, int64_t RB, int64_t n_snp,
                                                          int64_t N, const int32_t *__restrict__ sum, const int32_t *__restrict__ num,
                                                          int64_t col0, int n_groups, int64_t snp_stride, uint4 *__restrict__ mm,
                                                          const unsigned long long *__restrict__ d_run)
{
    if (*d_run == 0ull) return;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int G = blockIdx.y;
    if (k >= snp_stride || G >= n_groups) return;
    uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k < n_snp) {
        const int s = sum[k], c = num[k];
        if (0 < s && s < 2 * c) {                                         // genPCA.cpp:1206
            const int64_t s0 = col0 + (int64_t)G * 256;                   // first sample of the group (col0 is a multiple of 256)
            const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(packed + k * RB + (s0 >> 2));   // RB is a multiple of 64
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = src[q];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    uint32_t x = code3_mask(w[t]);                        // code 3 -> bit 2 j
                    x = (x | (x >> 1)) & 0x33333333u;
                    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
                    x = (x | (x >> 4)) & 0x00FF00FFu;
                    x = (x | (x >> 8)) & 0x0000FFFFu;                     // 16 samples -> 16 bits
                    out[2 * q + (t >> 1)] |= x << (16 * (t & 1));
                }
            }
            const int64_t left = N - s0;                                  // samples of this group that exist (padding is code 3)
            if (left < 256)
#pragma unroll
                for (int d = 0; d < 8; d++) {
                    const int64_t r = left - 32 * d;
                    if (r <= 0) out[d] = 0u;
                    else if (r < 32) out[d] &= (1u << r) - 1u;
                }
        }
    }
    uint4 *dst = mm + ((int64_t)G * snp_stride + k) * 2;
    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

// which form of the both-missing contraction takes this block: flags[0] = sparse (0 < missing calls <= max_cells), flags[1] =
// dense int8 product (more missing calls than that); both 0 for a block without missing calls.  The block's number of missing
// calls = sum over its SNPs of N - num[k] (d_missing is only a flag); one workgroup, summed in a fixed order.
__global__ __launch_bounds__(256) void miss_route_kernel(const int32_t *__restrict__ num, int64_t n_snp, int64_t N,
                                                         unsigned long long max_cells, unsigned long long *__restrict__ flags)
{
    __shared__ unsigned long long part[256];
    unsigned long long m = 0;
    for (int64_t k = threadIdx.x; k < n_snp; k += 256) m += (unsigned long long)(N - num[k]);
    part[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long t = part[0];
        flags[0] = (t != 0ull && t <= max_cells) ? 1ull : 0ull;
        flags[1] = (t > max_cells) ? 1ull : 0ull;
    }
}

int launch_missmask256(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t N, const int32_t *sum,
                       const int32_t *num, int64_t col0, int n_groups, int64_t snp_stride, uint4 *mm,
                       unsigned long long max_cells, unsigned long long *flags)
{
    hipLaunchKernelGGL(miss_route_kernel, dim3(1), dim3(256), 0, st, num, n_snp, N, max_cells, flags);
    if (n_snp > 0 && n_groups > 0)
        hipLaunchKernelGGL(missmask256_kernel, dim3((unsigned)((snp_stride + 255) / 256), (unsigned)n_groups), dim3(256), 0, st, packed, RB,
                           n_snp, N, sum, num, col0, n_groups, snp_stride, mm, flags);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_bitplanes4(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                      int64_t col0, int64_t ncols_pad, int64_t rows_pad, int KW, uint4 *rowp, uint4 *colp)
{
    dim3 grid((unsigned)(ncols_pad / 64), (unsigned)((KW / 2 + 3) / 4));
    hipLaunchKernelGGL(bitplanes_kernel<0>, grid, dim3(256), 0, st, packed, RB, n_snp, n_samp,
                       (const int32_t *)nullptr, (const int32_t *)nullptr, col0, ncols_pad, rows_pad, KW,
                       (void *)rowp, (void *)colp, (const unsigned long long *)nullptr);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_bitplanes_miss(hipStream_t st, const uint8_t *packed, int64_t RB, int64_t n_snp, int64_t n_samp,
                          const int32_t *sum, const int32_t *num, int64_t col0, int64_t ncols_pad,
                          int64_t rows_pad, int KW, uint2 *rowp, uint2 *colp,
                          const unsigned long long *d_missing_cells)
{
    dim3 grid((unsigned)(ncols_pad / 64), (unsigned)((KW / 2 + 3) / 4));
    hipLaunchKernelGGL(bitplanes_kernel<1>, grid, dim3(256), 0, st, packed, RB, n_snp, n_samp, sum, num, col0,
                       ncols_pad, rows_pad, KW, (void *)rowp, (void *)colp, d_missing_cells);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
