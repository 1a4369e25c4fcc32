// What vcf.hip (host layer) and kernels_vcf.hip share: the device view of VCF text, a line's description and the chunk geometry.
#pragma once
#include "snpgpu_internal.h"

namespace snpgpu {

constexpr int VCF_THREADS = 256;                          // lanes of a line's workgroup
constexpr int VCF_SEG = 16;                               // text bytes of a lane per chunk: four aligned dwords
constexpr int VCF_CHUNK = VCF_THREADS * VCF_SEG;          // text bytes of a workgroup per step
constexpr int VCF_HALO = 64;                              // bytes staged behind a chunk: a GT that crosses its end is read from LDS
constexpr int VCF_CODE_WORDS = (VCF_CHUNK + 1 + 3 + 15) / 16 + 1;     // dwords of 16 codes: a chunk's cells and the carried byte

// Text (or a staged window of it) as the kernel sees it: 16-byte aligned dwords; the caller's offset p is byte p + delta of w.
struct VcfText {
    const uint32_t *w;
    int64_t word_lo, word_hi;      // the dwords that hold a byte of the text: nothing outside them is loaded
    int64_t delta;
};

// one line: [begin, end) from its first sample cell to the end of its last one, in the caller's offsets
struct VcfLine { int64_t begin, end; int32_t num_allele, ref_index; };

enum { VCF_FLAG_GRAMMAR = 1, VCF_FLAG_RANGE = 2, VCF_FLAG_DIGITS = 4, VCF_FLAG_CELLS = 8 };

// rows: [n_lines][ceil(n_samp / 4)]; flags, cells: [n_lines] (all device memory)
int launch_vcf_parse(hipStream_t st, const VcfText &t, const VcfLine *lines, int64_t n_lines, int64_t n_samp, uint8_t *rows,
                     int32_t *flags, int64_t *cells);

}  // namespace snpgpu
