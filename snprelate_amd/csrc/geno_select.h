// What geno_select.hip (host layer) and kernels_geno_select.hip share: the device view of a source and the launch declarations.
// geno_merge.hip builds on both: the argument checks and the staging size of a selection, and the splice kernel's declarations.
#pragma once
#include <algorithm>

#include "snpgpu_internal.h"

namespace snpgpu {

// A source (or a staged window of one) as the kernels see it: aligned dwords, bit positions relative to w.
struct SelBits {
    const uint32_t *w;
    int64_t n_words;               // the dwords that hold a byte of the source: nothing beyond them is loaded
    int64_t bit0, stride;          // row r starts at bit0 + r * stride ...
    const int64_t *row_bit;        // ... or, if not NULL (device memory), at bit0 + row_bit[r]
};

constexpr int SEL_TW = 1024;                       // SNPs of a transposition workgroup: 64 dwords of a sample row
constexpr int SEL_PITCH = SEL_TW / 16 + 4;         // dwords per LDS tile row (16-byte aligned, as TR_PITCH)
constexpr int SEL_GATHER_ROWS = 8;                 // most output rows of a gather workgroup
constexpr int64_t SEL_LDS_WORDS = 16384;           // LDS dwords of a gather workgroup (64 KiB)

// <= SEL_TW SNPs that are consecutive in the source (column c ...) and in dst (row k ...)
struct SelSeg { int32_t k, c, len; };

// The code sets of a source and of dst (SNPGPU_CODE_GDS / SNPGPU_CODE_BED) as the kernels are instantiated: the map applied to every
// output dword of 16 codes and the code that fills the unused codes of a row's last byte of dst.
enum SelRecode {
    SEL_GDS_GDS = 0,               // identity, padding 3: snpgpu_geno_select
    SEL_BED_BED = 1,               // identity, padding 0
    SEL_BED_GDS = 2,               // {2, 3, 1, 0}, padding 3
    SEL_GDS_BED = 3                // {3, 2, 0, 1}, padding 0
};
inline SelRecode sel_recode(int src_code, int dst_code)
{
    return src_code == dst_code ? (dst_code == SNPGPU_CODE_BED ? SEL_BED_BED : SEL_GDS_GDS)
                                : (dst_code == SNPGPU_CODE_BED ? SEL_GDS_BED : SEL_BED_GDS);
}

// In the launchers a "row" is a row of dst and a "column" one of its 2-bit codes, whichever of SNP and sample each is.
// srow: source row of every output row (device) or NULL = in order; dst: [n_rows_out][ceil(n_out / 4)]
int launch_geno_copy(hipStream_t st, const SelBits &s, const int32_t *srow, int64_t s0, int64_t n_out, int64_t n_rows_out, uint8_t *dst,
                     SelRecode rc);
int launch_geno_gather(hipStream_t st, const SelBits &s, const int32_t *srow, const int32_t *samp, int64_t n_out, int64_t n_cols,
                       int64_t n_rows_out, int64_t lds_words, uint8_t *dst, SelRecode rc);
// samp: source row of every output column (device) or NULL = in order
int launch_geno_transpose(hipStream_t st, const SelBits &s, const int32_t *samp, const SelSeg *segs, int64_t n_segs, int64_t n_out,
                          uint8_t *dst, SelRecode rc);

// ---- what snpgpu_geno_merge shares with the selection (geno_select.hip) ---------------------------------------------------------
// every refusal of snpgpu_geno_select / snpgpu_geno_convert that needs no device, under the name fn; 0 = accepted
int sel_check_args(const char *fn, const snpgpu_geno_src *src, int src_code, const int32_t *samp_index, int64_t n_samp_out,
                   const int32_t *snp_index, int64_t n_snp_out, const void *dst, int dst_major, int dst_code, int dst_mem);
// source bytes per staging window (SNPGPU_SELECT_STAGE_BYTES, else 256 MiB)
size_t sel_stage_bytes();

// ---- the splice (kernels_geno_merge.hip) ---------------------------------------------------------------------------------------
// One part of a window of merged rows as the kernel sees it: row k of the window starts at bit bit0 + r * stride of the aligned
// dwords w, r = srow[k] or k, and is flipped (0 / 1 / 2 / 3 -> 2 / 1 / 0 / 3) where flip[k] is not zero.
struct SplicePart {
    const uint32_t *w;
    int64_t n_words;               // nothing beyond them is loaded
    int64_t bit0, stride;
    const int32_t *srow;           // device, the source row of every row of the window, or NULL = in order
    const uint8_t *flip;           // device, one byte per row of the window, or NULL
};
// parts, off: device memory; off[i] is the first code of part i in a merged row, off[n_parts] = N.  dst: [n_rows][ceil(N / 4)]
int launch_geno_splice(hipStream_t st, const SplicePart *parts, const int32_t *off, int n_parts, int64_t N, int64_t n_rows, uint8_t *dst);

}  // namespace snpgpu
