// What text.hip (host layer) and kernels_text.hip share: the device view of a render call (snpgpu_text_render, include/snpgpu.h
// section 1m) and the geometry of its kernels.
#pragma once
#include "snpgpu_internal.h"

namespace snpgpu {

constexpr int TEXT_THREADS = 256;                         // lanes of a line's workgroup
constexpr int TEXT_SEG = 16;                              // text bytes of a lane per step: one aligned 16-byte store
constexpr int TEXT_CHUNK = TEXT_THREADS * TEXT_SEG;       // text bytes of a workgroup per step (fixed-width lines)
constexpr int TEXT_LANE_COLS = 4;                         // columns of a lane per step (variable-width lines): one byte of the row
constexpr int TEXT_TILE = TEXT_THREADS * TEXT_LANE_COLS;  // columns of a workgroup per step (variable-width lines)

// One render call as the kernels see it.  Row r, byte b is byte rows_shift + r * rb + b of the aligned dwords rows_w; byte p of
// the text is byte text_shift + p of the 16-byte aligned text_al.  Only dwords that hold a byte of a row are loaded, only bytes
// of [text, text + line_off[n_rows]) are stored.
struct TextJob {
    const uint32_t *rows_w;
    int64_t rows_shift, rb, n_cols;
    uint8_t *text_al;
    int64_t text_shift;
    const uint8_t *pre_pool;       // device copies of the caller's pools and offsets; pre_off NULL: no prefixes
    const int64_t *pre_off;
    const uint8_t *al_pool;        // SNPGPU_TEXT_PED_ALLELE: s1, s2 of column c are pieces 2c, 2c + 1 of the pool
    const int64_t *al_off;
    int format;
};

// fixed-width formats (and SNPGPU_TEXT_PED_ALLELE when every allele is one byte: al_pool is then the per-column table)
int launch_text_fixed(hipStream_t st, const TextJob &j, int64_t n_rows);
// variable-width lines: len[r] = bytes of line r (prefix and '\n' included); then the bytes at line_off[r] (device, n_rows + 1)
int launch_text_lengths(hipStream_t st, const TextJob &j, int64_t n_rows, int64_t *len);
int launch_text_variable(hipStream_t st, const TextJob &j, int64_t n_rows, const int64_t *line_off);

}  // namespace snpgpu
