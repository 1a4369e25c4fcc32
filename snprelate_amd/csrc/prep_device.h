// Device code that more than one pre-pass translation unit needs (kernels_prep.hip, kernels_terms.hip, kernels_transpose.hip)
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

}  // namespace snpgpu
