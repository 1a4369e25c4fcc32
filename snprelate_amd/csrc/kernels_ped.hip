// PLINK .ped text -> allele tokens -> 2-bit rows (snpgpu_ped_tokens / _census / _codes, include/snpgpu.h section 1n; host layer:
// ped.hip).
//   ped_tokens_kernel   one workgroup per line, on the skeleton of text_chunk.h: the text from the line's seventh column goes
//                       through LDS in chunks, every lane marks the bytes of its segment that are neither tab nor space, and the
//                       scan of their counts numbers them.  In a regular line every such byte IS a token (CReadLine::GetCell,
//                       src/ConvToGDS.cpp:123-179, splitting by space and tab): it is followed by a separator or the line's end,
//                       and every separator is one tab or a run of spaces.  One byte of look-ahead decides both, so the lane reads
//                       the dword behind its segment from LDS.  Anything else is flagged and left to the host.
//   ped_census_kernel   a workgroup owns PED_CENSUS_SNPS SNPs of the window's token matrix, a lane one SNP: it walks the unflagged
//                       lines, counts its two tokens per line in LDS (94 counters, '0' not counted) and adds them to its own
//                       entries of the table.  No atomics: successive windows add on the stream.
//   ped_codes_kernel    a lane per byte of a sample row: [t1 == ref] + [t2 == ref], 3 when either token is '0'; tail padding 3.
// Loads of the text are aligned dwords inside [word_lo, word_hi).  Stores are bytes of the line's own tokens / row / counters.
#include <algorithm>

#include "ped.h"

namespace snpgpu {

__global__ __launch_bounds__(CHUNK_THREADS) void ped_tokens_kernel(TextView t, const PedLine *__restrict__ lines, int64_t n_tok,
                                                                   uint8_t *__restrict__ tokens, int32_t *__restrict__ flags,
                                                                   int64_t *__restrict__ counts)
{
    __shared__ uint32_t s_text[CHUNK_LDS_WORDS];
    __shared__ int s_wave[CHUNK_THREADS / 64];
    __shared__ uint32_t s_flags;

    const int tid = threadIdx.x;
    const int64_t line = blockIdx.x;
    const int64_t b = lines[line].begin + t.delta, e = lines[line].end + t.delta;
    uint8_t *out = tokens + line * n_tok;
    if (tid == 0) s_flags = 0u;

    const auto is_sep = [](uint32_t c) { return c == '\t' || c == ' '; };
    uint32_t fl = 0u;
    int64_t n_seen = 0;            // tokens in front of this chunk

    for (int64_t cb = b & ~int64_t(CHUNK_SEG - 1);; cb += CHUNK_BYTES) {
        uint32_t v[4];
        chunk_stage(t, cb, tid, s_text, v);
        const int64_t seg = cb + CHUNK_SEG * tid;
        uint32_t mask = chunk_mask(v, seg, b, e, [](uint32_t c) { return c != '\t' && c != ' '; });
        int before = 0, total = 0;
        chunk_scan(__popc(mask), tid, s_wave, before, total);

        // ---- the grammar, with the byte behind each byte: the next one of the segment, or the first one of the next segment ------------
        const uint32_t behind = s_text[4 * tid + 4] & 0xFFu;
#pragma unroll
        for (int j = 0; j < CHUNK_SEG; j++) {
            const int64_t p = seg + j;
            if (p < b || p >= e) continue;
            const uint32_t c = (v[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            const uint32_t n = j < CHUNK_SEG - 1 ? (v[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu : behind;
            const bool at_end = p + 1 >= e;
            if (!is_sep(c)) {
                if ((!at_end && !is_sep(n)) || c < 0x21u || c > 0x7Eu) fl |= PED_FLAG_TOKEN;
            } else {
                if (p == b) fl |= PED_FLAG_EMPTY;                                            // the seventh column is empty
                if (c == '\t' ? (at_end || is_sep(n)) : (!at_end && n == '\t')) fl |= PED_FLAG_EMPTY;
            }
        }

        // ---- the tokens of this segment --------------------------------------------------------------------------------------------
        int64_t k = n_seen + before;
        while (mask) {
            const int j = __ffs(mask) - 1;
            mask &= mask - 1u;
            if (k < n_tok) out[k] = (uint8_t)((v[j >> 2] >> (8 * (j & 3))) & 0xFFu);
            k++;
        }
        n_seen += total;
        const bool last = cb + CHUNK_BYTES >= e;
        __syncthreads();                                   // s_text and s_wave are written again by the next chunk
        if (last) break;
    }

    if (fl) atomicOr(&s_flags, fl);
    __syncthreads();
    if (tid == 0) {
        flags[line] = (int32_t)(s_flags | (n_seen != n_tok ? (uint32_t)PED_FLAG_COUNT : 0u));
        counts[line] = n_seen;
    }
}

__global__ __launch_bounds__(PED_CENSUS_SNPS) void ped_census_kernel(const uint8_t *__restrict__ tokens, const int32_t *__restrict__ flags,
                                                                     int64_t n_lines, int64_t n_snp, uint32_t *__restrict__ table)
{
    __shared__ uint32_t s_cnt[PED_ALLELES * PED_CENSUS_SNPS];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * PED_CENSUS_SNPS + tid;
    for (int c = 0; c < PED_ALLELES; c++) s_cnt[c * PED_CENSUS_SNPS + tid] = 0u;          // a lane touches only its own column
    if (j >= n_snp) return;
    for (int64_t i = 0; i < n_lines; i++) {
        if (flags[i]) continue;
        const uint8_t *p = tokens + i * 2 * n_snp + 2 * j;
        const uint32_t t1 = p[0], t2 = p[1];
        if (t1 != '0' && t1 - 0x21u < (uint32_t)PED_ALLELES) s_cnt[(t1 - 0x21u) * PED_CENSUS_SNPS + tid]++;
        if (t2 != '0' && t2 - 0x21u < (uint32_t)PED_ALLELES) s_cnt[(t2 - 0x21u) * PED_CENSUS_SNPS + tid]++;
    }
    for (int c = 0; c < PED_ALLELES; c++) {
        const uint32_t n = s_cnt[c * PED_CENSUS_SNPS + tid];
        if (n) table[j * PED_ALLELES + c] += n;
    }
}

__global__ __launch_bounds__(PED_CODE_THREADS) void ped_codes_kernel(const uint8_t *__restrict__ tokens, const uint8_t *__restrict__ ref,
                                                                     int64_t n_lines, int64_t n_snp, uint8_t *__restrict__ rows)
{
    const int64_t rb = (n_snp + 3) / 4, n = n_lines * rb;
    for (int64_t x = (int64_t)blockIdx.x * PED_CODE_THREADS + threadIdx.x; x < n; x += (int64_t)gridDim.x * PED_CODE_THREADS) {
        const int64_t line = x / rb, byte = x - line * rb;
        const uint8_t *p = tokens + line * 2 * n_snp;
        uint32_t out = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t j = 4 * byte + k;
            uint32_t code = 3u;
            if (j < n_snp) {
                const uint32_t t1 = p[2 * j], t2 = p[2 * j + 1], r = ref[j];
                if (t1 != '0' && t2 != '0') code = (t1 == r ? 1u : 0u) + (t2 == r ? 1u : 0u);
            }
            out |= code << (2 * k);
        }
        rows[x] = (uint8_t)out;
    }
}

int launch_ped_tokens(hipStream_t st, const TextView &t, const PedLine *lines, int64_t n_lines, int64_t n_tok, uint8_t *tokens,
                      int32_t *flags, int64_t *counts)
{
    hipLaunchKernelGGL(ped_tokens_kernel, dim3((unsigned)n_lines), dim3(CHUNK_THREADS), 0, st, t, lines, n_tok, tokens, flags, counts);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ped_census(hipStream_t st, const uint8_t *tokens, const int32_t *flags, int64_t n_lines, int64_t n_snp, uint32_t *table)
{
    const int64_t blocks = (n_snp + PED_CENSUS_SNPS - 1) / PED_CENSUS_SNPS;
    hipLaunchKernelGGL(ped_census_kernel, dim3((unsigned)blocks), dim3(PED_CENSUS_SNPS), 0, st, tokens, flags, n_lines, n_snp, table);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ped_codes(hipStream_t st, const uint8_t *tokens, const uint8_t *ref, int64_t n_lines, int64_t n_snp, uint8_t *rows)
{
    const int64_t n = n_lines * ((n_snp + 3) / 4);
    const int64_t blocks = std::min<int64_t>((n + PED_CODE_THREADS - 1) / PED_CODE_THREADS, int64_t(1) << 20);
    hipLaunchKernelGGL(ped_codes_kernel, dim3((unsigned)blocks), dim3(PED_CODE_THREADS), 0, st, tokens, ref, n_lines, n_snp, rows);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
