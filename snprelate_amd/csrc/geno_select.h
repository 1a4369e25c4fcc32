// What geno_select.hip (host layer) and kernels_geno_select.hip share: the device view of a source and the launch declarations.
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

}  // namespace snpgpu
