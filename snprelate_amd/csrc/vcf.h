// What vcf.hip (host layer) and kernels_vcf.hip share: a line's description, the flags and the code words of a chunk.  The chunk
// geometry and the view of the text are text_chunk.h's.
#pragma once
#include "text_chunk.h"

namespace snpgpu {

constexpr int VCF_CODE_WORDS = (CHUNK_BYTES + 1 + 3 + 15) / 16 + 1;   // dwords of 16 codes: a chunk's cells and the carried byte

// one line: [begin, end) from its first sample cell to the end of its last one, in the caller's offsets
struct VcfLine { int64_t begin, end; int32_t num_allele, ref_index; };

enum { VCF_FLAG_GRAMMAR = 1, VCF_FLAG_RANGE = 2, VCF_FLAG_DIGITS = 4, VCF_FLAG_CELLS = 8 };

// rows: [n_lines][ceil(n_samp / 4)]; flags, cells: [n_lines] (all device memory)
int launch_vcf_parse(hipStream_t st, const TextView &t, const VcfLine *lines, int64_t n_lines, int64_t n_samp, uint8_t *rows,
                     int32_t *flags, int64_t *cells);

}  // namespace snpgpu
