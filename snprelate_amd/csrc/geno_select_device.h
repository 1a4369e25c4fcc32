// Device pieces the genotype layout kernels share (kernels_geno_select.hip, kernels_geno_merge.hip): the 32-bit fetch at any bit of a
// stream of aligned dwords, the padding of a dword of 16 codes and the store of one aligned dword of dst that may reach over a
// row's ends.
#pragma once
#include "geno_select.h"

namespace snpgpu {

// 32 bits from bit p (>= 0, inside the source) of the stream; dwords beyond the source read as 0
__device__ __forceinline__ uint32_t sel_fetch32(const uint32_t *__restrict__ w, int64_t n_words, int64_t p)
{
    const int64_t d = p >> 5;
    const uint32_t sh = (uint32_t)p & 31u;
    const uint32_t lo = d < n_words ? w[d] : 0u;
    const uint32_t hi = (sh && d + 1 < n_words) ? w[d + 1] : 0u;
    return __builtin_amdgcn_alignbit(hi, lo, sh);
}

// codes rem ... 15 of a dword of 16 codes (rem ... 3 of a byte of 4) become PAD: 3 is the padding of pack_2bit_rows, 0 that of a
// .bed row
template <int PAD> __device__ __forceinline__ uint32_t sel_pad16(uint32_t v, int64_t rem)
{
    if (PAD == 3) return rem >= 16 ? v : rem <= 0 ? ~0u : v | (~0u << (2 * rem));
    return rem >= 16 ? v : rem <= 0 ? 0u : v & ~(~0u << (2 * rem));
}

// the dword of dst at row byte i0 (any of its bytes may lie outside the row [0, rb)): one store when whole, bytes otherwise
__device__ __forceinline__ void sel_store_unit(uint8_t *__restrict__ row, int64_t i0, int64_t rb, uint32_t v)
{
    if (i0 >= 0 && i0 + 4 <= rb) { *reinterpret_cast<uint32_t *>(row + i0) = v; return; }
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (i0 + b >= 0 && i0 + b < rb) row[i0 + b] = (uint8_t)(v >> (8 * b));
}

}  // namespace snpgpu
