// VCF genotype columns -> 2-bit rows (snpgpu_vcf_genotypes, include/snpgpu.h section 1l; host layer: vcf.hip).
//   vcf_parse_kernel   one workgroup per line.  The line's text from its first sample cell goes through LDS in chunks of
//                      CHUNK_BYTES bytes, a 16-byte segment per lane, with CHUNK_HALO bytes behind the chunk.  Every lane finds the
//                      tabs of its segment; a workgroup-wide exclusive scan of the tab counts gives every tab the index of the
//                      cell behind it, and the lane that owns the tab reduces that cell's GT sub-field to a dosage code
//                      (gnrParseVCF4's loop, src/ConvToGDS.cpp:910-987).  Codes are OR-ed four per byte into LDS; whole bytes go
//                      to the row after every chunk and the partly filled byte is carried to the next one.
// Loads are aligned dwords inside [word_lo, word_hi), the dwords that hold a byte of the text.  A GT that runs beyond the halo
// (dozens of alleles in one cell) is read on from global memory by the same rule, so no cell is ever given up for its length.
// Stores are bytes of the line's own row only; cells beyond n_samp are counted and never stored.  The only atomics are on LDS,
// and OR commutes: the result does not depend on the order of the lanes.
#include "vcf.h"

namespace snpgpu {

namespace {

struct VcfCellParser {
    const uint32_t *s_text;
    const uint32_t *__restrict__ w;
    int64_t cb, e;                 // the staged chunk starts at byte cb; the line ends at e (bytes of w)
    int32_t num_allele, ref_index;
    uint32_t flags;

    __device__ __forceinline__ uint32_t byte_at(int64_t p) const                 // cb <= p < e
    {
        const int64_t r = p - cb;
        const uint32_t d = r < CHUNK_BYTES + CHUNK_HALO ? s_text[r >> 2] : w[p >> 2];
        return (d >> (8 * ((uint32_t)p & 3u))) & 0xFFu;
    }

    // the dosage code of the cell that starts at `start`
    __device__ uint32_t parse(int64_t start)
    {
        if (start >= e) { flags |= VCF_FLAG_CELLS; return 0u; }                  // an empty last cell
        int64_t p = start;
        int dosage = 0;
        bool missing = false;
        while (p < e) {
            uint32_t c = byte_at(p);
            if (c == '\t' || c == ':') break;
            if (c - '0' < 10u) {
                int val = 0, nd = 0;
                do {
                    if (nd < 9) val = val * 10 + (int)(c - '0');
                    nd++;
                    p++;
                    c = p < e ? byte_at(p) : (uint32_t)'\t';
                } while (c - '0' < 10u);
                if (nd > 9) flags |= VCF_FLAG_DIGITS;
                else if (val >= num_allele) flags |= VCF_FLAG_RANGE;
                if (val == ref_index) dosage++;
            } else if (c == '.') {
                missing = true;
            } else {
                flags |= VCF_FLAG_GRAMMAR;
            }
            // everything up to the next '|' or '/' is skipped
            bool sep = false;
            while (p < e) {
                c = byte_at(p);
                if (c == '\t' || c == ':') break;
                p++;
                if (c == '|' || c == '/') { sep = true; break; }
            }
            if (!sep) break;
        }
        return missing ? 3u : (uint32_t)(dosage < 2 ? dosage : 2);
    }
};

}  // namespace

__global__ __launch_bounds__(CHUNK_THREADS) void vcf_parse_kernel(TextView t, const VcfLine *__restrict__ lines, int64_t n_samp, int64_t rb,
                                                                uint8_t *__restrict__ rows, int32_t *__restrict__ flags,
                                                                int64_t *__restrict__ cells)
{
    __shared__ uint32_t s_text[(CHUNK_BYTES + CHUNK_HALO) / 4];
    __shared__ uint32_t s_codes[VCF_CODE_WORDS];
    __shared__ int s_wave[CHUNK_THREADS / 64];
    __shared__ uint32_t s_flags;

    const int tid = threadIdx.x;
    const int64_t line = blockIdx.x;
    const VcfLine ln = lines[line];
    const int64_t b = ln.begin + t.delta, e = ln.end + t.delta;
    uint8_t *row = rows + line * rb;

    for (int i = tid; i < VCF_CODE_WORDS; i += CHUNK_THREADS) s_codes[i] = 0u;
    if (tid == 0) s_flags = 0u;

    VcfCellParser ps = {s_text, t.w, 0, e, ln.num_allele, ln.ref_index, 0u};
    int64_t n_cells = 1;           // cells seen so far: the first one and one behind every tab
    int64_t kb = 0;                // the cell whose code lies at bit 0 of s_codes: a multiple of 4

    for (int64_t cb = b & ~int64_t(CHUNK_SEG - 1);; cb += CHUNK_BYTES) {
        // ---- stage the chunk and its halo; the tab mask of this lane's segment and its scan (text_chunk.h) ------------------------------
        uint32_t v[4];
        chunk_stage(t, cb, tid, s_text, v);
        const int64_t seg = cb + CHUNK_SEG * tid;
        uint32_t mask = chunk_mask(v, seg, b, e, [](uint32_t c) { return c == '\t'; });
        const int cnt = __popc(mask);
        int before = 0, total = 0;
        chunk_scan(cnt, tid, s_wave, before, total);

        // ---- the cells that start in this chunk ------------------------------------------------------------------------------
        ps.cb = cb;
        const auto put = [&](int64_t k, uint32_t code) {
            if (k >= n_samp || code == 0u) return;
            const int64_t rel = k - kb;
            atomicOr(&s_codes[rel >> 4], code << (2 * ((uint32_t)rel & 15u)));
        };
        if (cb <= b && tid == 0) put(0, ps.parse(b));                            // the first chunk: the first cell has no tab of its own
        int64_t k = n_cells + before;
        while (mask) {
            const int j = __ffs(mask) - 1;
            mask &= mask - 1u;
            put(k, ps.parse(seg + j + 1));
            k++;
        }
        n_cells += total;
        __syncthreads();

        // ---- whole bytes to the row; the partly filled one is carried ----------------------------------------------------------
        const bool last = cb + CHUNK_BYTES >= e;
        const int64_t avail = (n_cells < n_samp ? n_cells : n_samp) - kb;        // codes in s_codes
        const int64_t nfull = avail >> 2, byte0 = kb >> 2;
        const auto code_byte = [&](int64_t i) { return (s_codes[i >> 2] >> (8 * ((uint32_t)i & 3u))) & 0xFFu; };
        if (!last) {
            for (int64_t i = tid; i < nfull; i += CHUNK_THREADS) row[byte0 + i] = (uint8_t)code_byte(i);
            const uint32_t carry = code_byte(nfull);
            __syncthreads();
            for (int i = tid; i < VCF_CODE_WORDS; i += CHUNK_THREADS) s_codes[i] = i == 0 ? carry : 0u;
            kb += 4 * nfull;
            // (the next chunk's barrier after staging orders these stores before its atomics; s_text is not read until then)
            continue;
        }
        // the last chunk: the unused codes of the row's last byte are 3, and so is whatever a short line leaves unfilled
        const uint32_t pad = (0xFFu << (2 * ((uint32_t)avail & 3u))) & 0xFFu;
        for (int64_t i = tid; byte0 + i < rb; i += CHUNK_THREADS)
            row[byte0 + i] = (uint8_t)(i < nfull ? code_byte(i) : i == nfull ? (code_byte(i) | pad) : 0xFFu);
        break;
    }

    if (ps.flags) atomicOr(&s_flags, ps.flags);
    __syncthreads();
    if (tid == 0) {
        flags[line] = (int32_t)(s_flags | (n_cells != n_samp ? (uint32_t)VCF_FLAG_CELLS : 0u));
        cells[line] = n_cells;
    }
}

int launch_vcf_parse(hipStream_t st, const TextView &t, const VcfLine *lines, int64_t n_lines, int64_t n_samp, uint8_t *rows,
                     int32_t *flags, int64_t *cells)
{
    const int64_t rb = (n_samp + 3) / 4;
    hipLaunchKernelGGL(vcf_parse_kernel, dim3((unsigned)n_lines), dim3(CHUNK_THREADS), 0, st, t, lines, n_samp, rb, rows, flags, cells);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace snpgpu
