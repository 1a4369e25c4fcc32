// The skeleton the text parsers share (kernels_vcf.hip, kernels_ped.hip): one workgroup walks a line of text in chunks through
// LDS, a 16-byte segment per lane with a halo behind the chunk; every lane marks the bytes of its segment it is interested in
// (tabs, token bytes) and a workgroup-wide exclusive scan of the counts numbers them along the line.
#pragma once
#include "snpgpu_internal.h"

namespace snpgpu {

constexpr int CHUNK_THREADS = 256;                        // lanes of a line's workgroup
constexpr int CHUNK_SEG = 16;                             // text bytes of a lane per chunk: four aligned dwords
constexpr int CHUNK_BYTES = CHUNK_THREADS * CHUNK_SEG;    // text bytes of a workgroup per step
constexpr int CHUNK_HALO = 64;                            // bytes staged behind a chunk: what crosses its end is read from LDS
constexpr int CHUNK_LDS_WORDS = (CHUNK_BYTES + CHUNK_HALO) / 4;

// Text (or a staged window of it) as a kernel sees it: 16-byte aligned dwords; the caller's offset p is byte p + delta of w.
struct TextView {
    const uint32_t *w;
    int64_t word_lo, word_hi;      // the dwords that hold a byte of the text: nothing outside them is loaded
    int64_t delta;
};

#ifdef __HIPCC__
// Stages the chunk that starts at byte cb (a multiple of CHUNK_SEG) and its halo into s_text[CHUNK_LDS_WORDS]; v: the four dwords
// of this lane's segment, the bytes cb + CHUNK_SEG * tid ...  Dwords outside the text read as 0.  No barrier.
__device__ __forceinline__ void chunk_stage(const TextView &t, int64_t cb, int tid, uint32_t *s_text, uint32_t (&v)[4])
{
    const int64_t d0 = (cb >> 2) + 4 * tid;
    if (d0 >= t.word_lo && d0 + 4 <= t.word_hi) {
        const uint4 q = *reinterpret_cast<const uint4 *>(t.w + d0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (d0 + i >= t.word_lo && d0 + i < t.word_hi) ? t.w[d0 + i] : 0u;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) s_text[4 * tid + i] = v[i];
    if (tid < CHUNK_HALO / 4) {
        const int64_t d = ((cb + CHUNK_BYTES) >> 2) + tid;
        s_text[CHUNK_BYTES / 4 + tid] = (d >= t.word_lo && d < t.word_hi) ? t.w[d] : 0u;
    }
}

// bit j: byte j of the segment (at `seg` of the line's text) lies in [b, e) and pred(byte) holds
template <class Pred>
__device__ __forceinline__ uint32_t chunk_mask(const uint32_t (&v)[4], int64_t seg, int64_t b, int64_t e, Pred pred)
{
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < CHUNK_SEG; j++) {
        const uint32_t c = (v[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        if (pred(c) && seg + j >= b && seg + j < e) mask |= 1u << j;
    }
    return mask;
}

// Workgroup-wide exclusive scan of cnt over the lanes: `before` = the sum over the lanes in front of this one, `total` = over all.
// One barrier, which also publishes what chunk_stage wrote; s_wave[CHUNK_THREADS / 64] must not be written again before the
// workgroup's next barrier.
__device__ __forceinline__ void chunk_scan(int cnt, int tid, int *s_wave, int &before, int &total)
{
    const int lane = tid & 63, wv = tid >> 6;
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    before = incl - cnt;
    total = 0;
#pragma unroll
    for (int i = 0; i < CHUNK_THREADS / 64; i++) {
        if (i < wv) before += s_wave[i];
        total += s_wave[i];
    }
}
#endif

}  // namespace snpgpu
