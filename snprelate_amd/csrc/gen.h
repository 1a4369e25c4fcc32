// What gen.hip (host layer) and kernels_gen.hip share: a line's description, the flags and the geometry of the call stage
// (snpgpu_gen_genotypes, include/snpgpu.h section 1p).  The chunk geometry and the view of the text are text_chunk.h's.
#pragma once
#include "text_chunk.h"

namespace snpgpu {

constexpr int GEN_MAX_TOKENS = CHUNK_BYTES / 2;           // a token start needs a separator in front of it
constexpr int GEN_GROUP = 12;                             // tokens of one byte of a row: four samples of three probabilities
constexpr int GEN_SIG_DIGITS = 15;                        // significant digits the kernel reads: 10^15 < 2^53
constexpr int GEN_MAX_DECIMALS = 22;                      // digits behind the point: 10^22 is the last exact power of ten in fp64

// one line: [begin, end) from its sixth column to the end of its last cell, in the caller's offsets
struct GenLine { int64_t begin, end; };

enum {
    GEN_FLAG_BYTE = 1,             // a token byte that is neither a digit nor the token's single point
    GEN_FLAG_DOT = 2,              // a token without a digit: "."
    GEN_FLAG_DIGITS = 4,           // more than GEN_SIG_DIGITS significant digits or more than GEN_MAX_DECIMALS decimals
    GEN_FLAG_LONG = 8,             // a token longer than the halo
    GEN_FLAG_EMPTY = 16,           // an empty cell: a tab beside a separator or at the line's end, a separator first
    GEN_FLAG_COUNT = 32            // tokens != 3 n_samp
};

// rows: [n_lines][ceil(n_samp / 4)]; flags, cells: [n_lines] (all device memory)
int launch_gen_parse(hipStream_t st, const TextView &t, const GenLine *lines, int64_t n_lines, int64_t n_samp, double call_threshold,
                     uint8_t *rows, int32_t *flags, int64_t *cells);

}  // namespace snpgpu
