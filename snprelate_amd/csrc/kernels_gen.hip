// Oxford GEN genotype probabilities -> 2-bit rows (snpgpu_gen_genotypes, include/snpgpu.h section 1p; host layer: gen.hip).
//   gen_parse_kernel   one workgroup per line, on the skeleton of text_chunk.h: the text from the line's sixth column goes through
//                      LDS in chunks, every lane marks the token starts of its segment (a byte that is neither space nor tab
//                      behind a space, a tab or the start), and the scan of their counts numbers them along the line.  The lane
//                      that owns a start reads the token from LDS -- through the halo when it crosses the chunk's end -- as a
//                      decimal integer m and a count k of digits behind the point, and rounds m / 10^k ONCE to single precision
//                      (gen_round: what strtof gives, src/ConvToGDS.cpp:506-532).  The floats go to LDS by token number; after a
//                      barrier a lane takes twelve of them, four samples, through the decision tree of gnrParseGEN
//                      (src/ConvToGDS.cpp:1134-1145) and stores one byte of the row.  The tokens of an unfinished byte, at most
//                      eleven, are carried to the next chunk in front of its own.
// Whatever is not `digits [ '.' digits ]` or `'.' digits` within the digit budget, every empty cell and every wrong token count is
// flagged and left to the host (snpgpu_gen_line_host).
// Loads are aligned dwords inside [word_lo, word_hi).  Stores are bytes of the line's own row only; tokens beyond 3 n_samp are
// counted and never stored.  No atomics but one OR of the flags in LDS.
#include "gen.h"

namespace snpgpu {

namespace {

__device__ const double GEN_P10[GEN_MAX_DECIMALS + 1] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                                         1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// m / 10^k (m < 10^15, k <= 22) rounded once to single precision.  Both operands are exact in fp64, so d is the correctly rounded
// double of the quotient, and it lies on the same side of every float midpoint as the quotient does -- unless it IS the midpoint:
// then the sign of d 10^k - m, which one fma gives exactly, says where the quotient lies, and zero is a true tie.  The quotient
// is 0 or within 1e-22 ... 1e15: never subnormal, never infinite as a float.
__device__ __forceinline__ float gen_round(uint64_t m, int k)
{
    if (m == 0) return 0.0f;
    const double p = GEN_P10[k], dm = (double)(int64_t)m;
    const double d = dm / p;
    uint64_t bits = (uint64_t)__double_as_longlong(d);
    const uint64_t low = bits & 0x1FFFFFFFull;             // the 29 bits of the significand a float does not have
    bool up = low > 0x10000000ull;
    if (low == 0x10000000ull) {
        const double r = fma(d, p, -dm);                   // > 0: d is above the quotient, which is below the midpoint
        up = r < 0.0 || (r == 0.0 && (bits & 0x20000000ull) != 0);
    }
    bits = (bits & ~0x1FFFFFFFull) + (up ? 0x20000000ull : 0ull);
    return (float)__longlong_as_double((long long)bits);   // exact
}

// the tree of src/ConvToGDS.cpp:1134-1145: strtof's floats widened, compared as doubles; NaN never reaches the kernel's floats
__device__ __forceinline__ uint32_t gen_call(float f_aa, float f_ab, float f_bb, double thr)
{
    const double aa = f_aa, ab = f_ab, bb = f_bb;
    if (aa >= ab) {
        if (aa >= bb) return aa >= thr ? 2u : 3u;
        return bb >= thr ? 0u : 3u;
    }
    if (ab >= bb) return ab >= thr ? 1u : 3u;
    return bb >= thr ? 0u : 3u;
}

// one byte of a row: the first n of the samples s0 ... s0 + 3 from val[3 n]; samples beyond n_samp and beyond n are code 0
__device__ __forceinline__ uint8_t gen_byte(const float *val, int n, int64_t s0, int64_t n_samp, double thr)
{
    uint32_t out = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (q < n && s0 + q < n_samp) out |= gen_call(val[3 * q], val[3 * q + 1], val[3 * q + 2], thr) << (2 * q);
    return (uint8_t)out;
}

}  // namespace

__global__ __launch_bounds__(CHUNK_THREADS) void gen_parse_kernel(TextView t, const GenLine *__restrict__ lines, int64_t n_samp, int64_t rb,
                                                                  double thr, uint8_t *__restrict__ rows, int32_t *__restrict__ flags,
                                                                  int64_t *__restrict__ cells)
{
    __shared__ uint32_t s_text[CHUNK_LDS_WORDS];
    __shared__ float s_val[GEN_GROUP + GEN_MAX_TOKENS];    // the carried tokens end at GEN_GROUP, the chunk's own start there
    __shared__ int s_wave[CHUNK_THREADS / 64];
    __shared__ uint32_t s_flags;

    const int tid = threadIdx.x;
    const int64_t line = blockIdx.x;
    const int64_t b = lines[line].begin + t.delta, e = lines[line].end + t.delta;
    uint8_t *row = rows + line * rb;
    if (tid == 0) s_flags = 0u;

    const auto is_sep = [](uint32_t c) { return c == '\t' || c == ' '; };
    uint32_t fl = 0u;
    int64_t n_seen = 0;            // tokens in front of this chunk
    int carried = 0;               // those of them whose byte of the row is not complete: s_val[GEN_GROUP - carried, GEN_GROUP)

    for (int64_t cb = b & ~int64_t(CHUNK_SEG - 1);; cb += CHUNK_BYTES) {
        // ---- stage the chunk; the token starts of this lane's segment and their scan (text_chunk.h) ------------------------------------
        uint32_t v[4];
        chunk_stage(t, cb, tid, s_text, v);
        const int64_t seg = cb + CHUNK_SEG * tid;
        uint32_t front = __shfl_up(v[3], 1, 64);           // the dword in front of the segment: the neighbour's, or loaded by a wave's first lane
        if ((tid & 63) == 0) {
            const int64_t d = (cb >> 2) + 4 * tid - 1;
            front = (d >= t.word_lo && d < t.word_hi) ? t.w[d] : 0u;
        }
        const uint32_t body = chunk_mask(v, seg, b, e, [](uint32_t c) { return c != '\t' && c != ' '; });
        // a byte of a token starts it when the byte in front is not one: a separator, or outside [b, e) -- then the byte is at b
        const uint32_t starts = body & ~((body << 1) | ((seg > b && !is_sep(front >> 24)) ? 1u : 0u));
        int before = 0, total = 0;
        chunk_scan(__popc(starts), tid, s_wave, before, total);

        // ---- empty cells, with the byte behind each separator: the next one of the segment, or the first one of the next segment ----------
        const uint32_t behind = s_text[4 * tid + 4] & 0xFFu;
#pragma unroll
        for (int j = 0; j < CHUNK_SEG; j++) {
            const int64_t p = seg + j;
            const uint32_t c = (v[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            if (p < b || p >= e || !is_sep(c)) continue;
            const uint32_t n = j < CHUNK_SEG - 1 ? (v[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu : behind;
            const bool at_end = p + 1 >= e;
            if (p == b) fl |= GEN_FLAG_EMPTY;                                                // the sixth column is empty
            if (c == '\t' ? (at_end || is_sep(n)) : (!at_end && n == '\t')) fl |= GEN_FLAG_EMPTY;
        }

        // ---- the tokens that start in this segment: digits [ '.' digits ] or '.' digits as m and k, one float each -------------------------
        int idx = before;
        uint32_t todo = starts;
        while (todo) {
            const int j = __ffs(todo) - 1;
            todo &= todo - 1u;
            const int r0 = CHUNK_SEG * tid + j;            // of the token's first byte in s_text; r0 + CHUNK_HALO is still staged
            const int64_t p0 = seg + j;
            uint64_t m = 0;
            int nd = 0, k = 0;
            bool point = false, digit = false;
            for (int i = 0; p0 + i < e; i++) {
                const int r = r0 + i;
                const uint32_t c = (s_text[r >> 2] >> (8 * (r & 3))) & 0xFFu;
                if (is_sep(c)) break;
                if (i == CHUNK_HALO) { fl |= GEN_FLAG_LONG; break; }
                const uint32_t dg = c - '0';
                if (dg < 10u) {
                    digit = true;
                    if (point) k++;
                    if ((m | dg) != 0 && ++nd <= GEN_SIG_DIGITS) m = m * 10 + dg;             // leading zeros are not significant
                } else if (c == '.' && !point) {
                    point = true;
                } else {
                    fl |= GEN_FLAG_BYTE;
                }
            }
            if (!digit) fl |= GEN_FLAG_DOT;
            if (nd > GEN_SIG_DIGITS || k > GEN_MAX_DECIMALS) {
                fl |= GEN_FLAG_DIGITS;
                k = k > GEN_MAX_DECIMALS ? GEN_MAX_DECIMALS : k;
            }
            s_val[GEN_GROUP + idx] = gen_round(m, k);
            idx++;
        }
        __syncthreads();

        // ---- twelve tokens are a byte of the row; what is left of them is carried ------------------------------------------------------------
        const int have = carried + total;
        const int ng = have / GEN_GROUP, left = have - ng * GEN_GROUP;
        const int64_t byte0 = (n_seen - carried) / GEN_GROUP;
        const float *val = s_val + GEN_GROUP - carried;
        for (int g = tid; g < ng; g += CHUNK_THREADS)
            if (byte0 + g < rb) row[byte0 + g] = gen_byte(val + GEN_GROUP * g, 4, 4 * (byte0 + g), n_samp, thr);
        n_seen += total;
        if (cb + CHUNK_BYTES >= e) {
            // the last chunk: the complete samples of the unfinished byte; whatever a short line leaves unfilled is 0
            const int64_t bl = byte0 + ng;
            for (int64_t i = bl + tid; i < rb; i += CHUNK_THREADS)
                row[i] = i == bl ? gen_byte(val + GEN_GROUP * ng, left / 3, 4 * bl, n_samp, thr) : (uint8_t)0;
            break;
        }
        const float keep = tid < left ? val[GEN_GROUP * ng + tid] : 0.0f;
        __syncthreads();
        if (tid < left) s_val[GEN_GROUP - left + tid] = keep;
        carried = left;
        // (the next chunk's barrier in chunk_scan orders these stores before the reads; s_text is not read again until then)
    }

    if (fl) atomicOr(&s_flags, fl);
    __syncthreads();
    if (tid == 0) {
        flags[line] = (int32_t)(s_flags | (n_seen != 3 * n_samp ? (uint32_t)GEN_FLAG_COUNT : 0u));
        cells[line] = n_seen;
    }
}

int launch_gen_parse(hipStream_t st, const TextView &t, const GenLine *lines, int64_t n_lines, int64_t n_samp, double call_threshold,
                     uint8_t *rows, int32_t *flags, int64_t *cells)
{
    const int64_t rb = (n_samp + 3) / 4;
    hipLaunchKernelGGL(gen_parse_kernel, dim3((unsigned)n_lines), dim3(CHUNK_THREADS), 0, st, t, lines, n_samp, rb, call_threshold, rows,
                       flags, cells);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
