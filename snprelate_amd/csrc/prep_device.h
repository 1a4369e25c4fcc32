// Device code that more than one pre-pass translation unit needs (kernels_prep.hip, kernels_terms.hip, kernels_transpose.hip, kernels_geno_select.hip)
// and the 2-bit plane split that the statistics units (kernels_pop.hip, kernels_qc.hip, kernels_pairscore.hip) share with them.
#pragma once
#include "snpgpu_internal.h"

namespace snpgpu {

// A dword holds 16 genotype codes, code j at bits 2j: code bits (hi,lo): 0=(0,0) 1=(0,1) 2=(1,0) 3=(1,1).
// The planes lo / hi carry a code's low / high bit at bit 2j.
constexpr uint32_t GENO_LO_BITS = 0x55555555u;
__device__ __forceinline__ uint32_t geno_lo(uint32_t w) { return w & GENO_LO_BITS; }
__device__ __forceinline__ uint32_t geno_hi(uint32_t w) { return (w >> 1) & GENO_LO_BITS; }
__device__ __forceinline__ uint32_t code3_mask(uint32_t w) { return w & (w >> 1) & GENO_LO_BITS; }   // code 3 = both bits -> bit 2j

__device__ __forceinline__ void count_word(uint32_t w, int &n1, int &n2, int &nm)
{
    const uint32_t lo = geno_lo(w), hi = geno_hi(w);
    n1 += __popc(lo & ~hi);
    n2 += __popc(hi & ~lo);
    nm += __popc(lo & hi);
}

// code3_mask of the codes below position r of a word (r <= 0: none, r >= 16: all): the cells beyond a tail are padding
// (the mask spelled out: on top of code3_mask it changes transpose2_direct_kernel beyond a reordering)
__device__ __forceinline__ uint32_t code3_below(uint32_t w, int64_t r)
{
    uint32_t m3 = w & (w >> 1) & GENO_LO_BITS;
    if (r <= 0) m3 = 0u;
    else if (r < 16) m3 &= (1u << (2 * r)) - 1u;
    return m3;
}

// Transposition of a 64 x 64 matrix of 2-bit elements spread over a wave: lane r holds row r as 128 bits (element e at
// bits 2e of x[0..3]); on return lane r holds column r in the same form.  Recursive block swap, blocks of 32, 16, 8, 4, 2, 1
// elements: a lane of the upper half of a block pair (bit j of the lane clear) keeps its elements with bit j clear and takes
// its partner's elements with bit j clear into the positions with bit j set; the lower half the other way round.  The two
// widest blocks move whole dwords, the others cost one rotate and one bit-field insert per dword: ~70 vector instructions and
// 20 cross-lane moves for 4096 genotypes, where the ballot form (one ballot per sample and bit plane, kept by the one lane
// it belongs to) took ~500 -- the pre-pass kernels were bound by exactly those.
__device__ __forceinline__ void transpose_2bit_64x64(uint32_t (&x)[4], int lane)
{
    {
        const bool hi = (lane & 32) != 0;
        const uint32_t r0 = (uint32_t)__shfl_xor((int)(hi ? x[0] : x[2]), 32), r1 = (uint32_t)__shfl_xor((int)(hi ? x[1] : x[3]), 32);
        if (hi) { x[0] = r0; x[1] = r1; } else { x[2] = r0; x[3] = r1; }
    }
    {
        const bool hi = (lane & 16) != 0;
        const uint32_t r0 = (uint32_t)__shfl_xor((int)(hi ? x[0] : x[1]), 16), r1 = (uint32_t)__shfl_xor((int)(hi ? x[2] : x[3]), 16);
        if (hi) { x[0] = r0; x[2] = r1; } else { x[1] = r0; x[3] = r1; }
    }
#pragma unroll
    for (int st = 0; st < 4; st++) {
        const int j = 8 >> st;                                        // elements per block
        const uint32_t m = st == 0 ? 0x0000FFFFu : st == 1 ? 0x00FF00FFu : st == 2 ? 0x0F0F0F0Fu : 0x33333333u;
        const int sh = 2 * j;                                         // bits per block
        const bool hi = (lane & j) != 0;
        const uint32_t keep = hi ? ~m : m;
        const uint32_t rot = hi ? (uint32_t)sh : (uint32_t)(32 - sh); // rotate right: upper half takes y << sh, lower y >> sh
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t y = (uint32_t)__shfl_xor((int)x[d], j);
            const uint32_t r = __builtin_amdgcn_alignbit(y, y, rot);
            x[d] = (x[d] & keep) | (r & ~keep);
        }
    }
}

}  // namespace snpgpu
