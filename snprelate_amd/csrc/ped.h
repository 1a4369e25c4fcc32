// What ped.hip (host layer) and kernels_ped.hip share (include/snpgpu.h section 1n).
#pragma once
#include "text_chunk.h"

namespace snpgpu {

constexpr int PED_ALLELES = 94;                           // the token bytes 0x21 ... 0x7E a census counts
constexpr int PED_CENSUS_SNPS = 128;                      // SNPs (= lanes) of a census workgroup: 94 x 128 counters of LDS
constexpr int PED_CODE_THREADS = 256;

// one line: [begin, end) from the first byte of its seventh column to the end of the line, in the caller's offsets
struct PedLine { int64_t begin, end; };

enum { PED_FLAG_TOKEN = 1, PED_FLAG_EMPTY = 2, PED_FLAG_COUNT = 8 };

// tokens: [n_lines][n_tok] token bytes; flags: [n_lines]; counts: [n_lines] tokens found (all device memory)
int launch_ped_tokens(hipStream_t st, const TextView &t, const PedLine *lines, int64_t n_lines, int64_t n_tok, uint8_t *tokens,
                      int32_t *flags, int64_t *counts);
// table: uint32 [n_snp][PED_ALLELES], the unflagged lines' tokens other than '0' added to it
int launch_ped_census(hipStream_t st, const uint8_t *tokens, const int32_t *flags, int64_t n_lines, int64_t n_snp, uint32_t *table);
// rows: [n_lines][ceil(n_snp / 4)] codes against ref[n_snp]
int launch_ped_codes(hipStream_t st, const uint8_t *tokens, const uint8_t *ref, int64_t n_lines, int64_t n_snp, uint8_t *rows);

}  // namespace snpgpu
