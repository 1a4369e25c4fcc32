// Selection of related pairs from one panel (snpgpu_select_pairs; snpgdsIBDSelection, R/IBD.R:463-531, applied to the resident counters
// instead of to n x n matrices): the pairs (i, j), row0 <= i < row1, i < j < N, with sel[i] && sel[j] and kinship(i, j) >= cutoff, written
// in the reference's order -- i ascending, then j ascending = which(lower.tri & flag, arr.ind = TRUE) with ID1 = sample[col],
// ID2 = sample[row] -- and nothing else: bytes proportional to the number of selected pairs.
//
// No atomic decides where a pair goes.  Two passes over the panel with the SAME walk:
//   count  a workgroup (4 waves) takes a row; wave w takes the w-th quarter of the row's 64-column chunks (contiguous, so segment order is
//          column order) and counts its hits: counts[4 (i - row0) + w], uint32
//   scan   exclusive prefix sums over the 4 x rows segment counts, int64 (5e9 pairs do not fit 32 bits); offsets[last] = the total
//   write  the same walk; a wave starts at its segment's offset, places the hits of a chunk with a 64-bit ballot and the popcount of the
//          lower lanes, and carries the running offset to the next chunk.  Only positions below `capacity` are stored.
// The write pass evaluates the value functions again (fin_values.h: the same functions as the finalisers, on the same counters, so the
// same hits) instead of reading a bit mask left by the count pass: DESIGN.md 20.
// Chunks are aligned to 64 columns (a wave reads 256 contiguous bytes of each uint32 plane); rows are spread over grid.x with a stride
// loop (a panel may have more rows than grid.y allows).
// The sparse GRM (snpgpu_select_grm) is the same walk over the GCTA / covariance / EIGMIX / IndivBeta value functions,
// one value per pair, plus a small kernel for the diagonal.
// PC-Relate (snpgpu_pcr_select) is the same walk over the finaliser's expressions on the resident fp64 sums of a row
// panel, four values per pair.
#include "fin_values.h"
#include "pcrelate_device.h"

#include <cmath>

namespace snpgpu {

namespace {

constexpr int SEL_WAVES = 4;       // waves per workgroup = segments per row

struct SelKingRobust {
    KingRobustArgs v;
    __device__ __forceinline__ void values(int64_t rel, int64_t, int64_t i, int64_t j, double &v0, double &v1, double &kin) const
    {
        king_robust_value(v, rel, i, j, v0, kin);
        v1 = 0.0;                                      // (not an output of this kind)
    }
};
struct SelKingHomo {
    KingHomoArgs v;
    __device__ __forceinline__ void values(int64_t rel, int64_t relf, int64_t i, int64_t j, double &v0, double &v1, double &kin) const
    {
        king_homo_value(v, rel, relf, i, j, v0, v1);
        kin = kinship_k0k1(v0, v1);
    }
};
struct SelMom {
    MomArgs v;
    __device__ __forceinline__ void values(int64_t rel, int64_t, int64_t, int64_t, double &v0, double &v1, double &kin) const
    {
        mom_value(v, rel, v0, v1);
        kin = kinship_k0k1(v0, v1);
    }
};

// The GRM kinds: ONE value per pair, what the kind's finaliser writes at (i, j), compared with the cutoff and stored in `kin`; value()
// serves the diagonal kernel too (i == j).  The fp64 planes are tile-major (acc_off): 256 x 256 tiles whose rows are 256 contiguous
// doubles, so the 64 aligned columns of a chunk never leave a tile and are 512 contiguous bytes -- four full 128-byte lines per
// wave and plane, as coalesced as the 256 bytes of a uint32 plane.  These kinds keep the walk and its 64-column alignment.
struct SelGcta {
    GctaArgs v;
    __device__ __forceinline__ double value(int64_t rel, int64_t relf, int64_t i, int64_t j) const { return gcta_value(v, rel, relf, i, j); }
};
struct SelCov {
    CovArgs v;
    __device__ __forceinline__ double value(int64_t, int64_t relf, int64_t, int64_t) const { return cov_value(v, relf); }
};
struct SelEigmix {
    EigmixArgs v;
    __device__ __forceinline__ double value(int64_t, int64_t relf, int64_t i, int64_t j) const { return eigmix_value(v, relf, i, j); }
};
struct SelBeta {
    BetaArgs v;
    __device__ __forceinline__ double value(int64_t rel, int64_t, int64_t i, int64_t j) const { return beta_value(v, rel, i, j); }
};
// a GRM functor behind the three-value interface of the walk (NV = 1: only `kin` is stored)
template <class G>
struct SelOne {
    G g;
    __device__ __forceinline__ void values(int64_t rel, int64_t relf, int64_t i, int64_t j, double &, double &, double &kin) const
    {
        kin = g.value(rel, relf, i, j);
    }
};

// PC-Relate: what pcr_view_final_kernel writes at (j, i), the entry of the lower triangle that snpgdsIBDSelection reads for the pair
// i < j (k2's two DC terms are subtracted in the other order at (i, j)); v0 = k0, v1 = k2, the fourth value = nsnp.  The slabs are
// row-major with their own origin: the walk's rel / relf are not used.
struct SelPcr {
    PcrView v;
    const double *e;
    int probs;
    __device__ __forceinline__ void values(int64_t, int64_t, int64_t i, int64_t j, double &v0, double &v1, double &kin) const
    {
        pcr_pair_values(v, e, j, i, probs != 0, kin, v0, v1);
    }
    __device__ __forceinline__ double fourth(int64_t i, int64_t j) const { return v.sym(PCR_NS, j, i); }
};

struct SelOut {
    int32_t *idx1, *idx2; double *v0, *v1, *kin;       // any may be nullptr
    int64_t capacity;
    double *v2;                                        // NV = 4 only
};

// WRITE = false: counts[seg] = hits of the segment;  WRITE = true: the hits stored from offsets[seg] on.  NV: values stored per pair
// (4: v0, v1, kin and f.fourth(i, j);  3: v0, v1, kin;  1: kin alone)
template <class F, bool WRITE, int NV = 3>
__global__ __launch_bounds__(64 * SEL_WAVES) void select_kernel(PanelGeom g, F f, const uint8_t *__restrict__ sel, int all, double cutoff,
                                                               uint32_t *__restrict__ counts, const int64_t *__restrict__ offsets, SelOut o)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t i = g.row0 + blockIdx.x; i < g.row1; i += gridDim.x) {
        const int64_t seg = (i - g.row0) * SEL_WAVES + w;
        int64_t off = 0;
        if (WRITE) {
            off = offsets[seg];
            if (off >= o.capacity) continue;                            // (wave-uniform: nothing of this segment is stored)
        }
        uint32_t cnt = 0;
        if (!sel || sel[i]) {
            const int64_t c_first = (i + 1) & ~(int64_t)63;             // aligned chunk that holds column i + 1
            const int64_t nch = (g.N - c_first + 63) >> 6;              // chunks of this row (<= 0: the last row)
            const int64_t per = (nch + SEL_WAVES - 1) / SEL_WAVES;
            const int64_t ch0 = w * per, ch1 = (ch0 + per < nch) ? (ch0 + per) : nch;
            for (int64_t ch = ch0; ch < ch1; ch++) {
                const int64_t j = c_first + (ch << 6) + lane;
                bool hit = false;
                double v0 = 0, v1 = 0, kin = 0;
                if (j > i && j < g.N && (!sel || sel[j])) {
                    const int64_t rel = (i - g.row0) * g.ncols_pad + (j - g.col0);                         // uint32 planes: row-major
                    const int64_t relf = acc_off(g.ncols_pad, g.f64_tiles_c, i - g.row0, j - g.col0);      // fp64 planes
                    f.values(rel, relf, i, j, v0, v1, kin);
                    hit = all || kin >= cutoff;                         // (a NaN kinship fails every comparison)
                }
                const unsigned long long m = __ballot(hit);
                if (WRITE) {
                    const int64_t pos = off + __popcll(m & ((1ull << lane) - 1ull));
                    if (hit && pos < o.capacity) {
                        if (o.idx1) o.idx1[pos] = (int32_t)i;
                        if (o.idx2) o.idx2[pos] = (int32_t)j;
                        if (NV >= 3) {
                            if (o.v0) o.v0[pos] = v0;
                            if (o.v1) o.v1[pos] = v1;
                        }
                        if (o.kin) o.kin[pos] = kin;
                        if constexpr (NV == 4) {
                            if (o.v2) o.v2[pos] = f.fourth(i, j);
                        }
                    }
                    off += __popcll(m);
                    if (off >= o.capacity) break;
                } else {
                    cnt += (uint32_t)__popcll(m);
                }
            }
        }
        if (!WRITE && lane == 0) counts[seg] = cnt;
    }
}

// exclusive scan of n uint32 counts into n + 1 int64 offsets, one workgroup: thread t sums its contiguous run, the 256 run sums are
// scanned in LDS, the run is walked again
__global__ __launch_bounds__(256) void select_scan_kernel(const uint32_t *__restrict__ counts, int64_t n, int64_t *__restrict__ offsets)
{
    __shared__ int64_t part[256];
    const int64_t per = (n + 255) / 256;
    const int64_t a = (int64_t)threadIdx.x * per, b = (a + per < n) ? (a + per) : n;
    int64_t s = 0;
    for (int64_t k = a; k < b; k++) s += counts[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 256; t++) { const int64_t v = part[t]; part[t] = run; run += v; }
        offsets[n] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t k = a; k < b; k++) { offsets[k] = run; run += counts[k]; }
}

// diag[k] = the entry (row0 + k, row0 + k) of the panel's real rows, by the value function of the pairs
template <class G>
__global__ __launch_bounds__(256) void select_diag_kernel(PanelGeom g, G f, double *__restrict__ diag)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, i = g.row0 + k;
    if (i >= g.row1 || i >= g.N) return;
    const int64_t rel = k * g.ncols_pad + (i - g.col0);
    const int64_t relf = acc_off(g.ncols_pad, g.f64_tiles_c, k, i - g.col0);
    diag[k] = f.value(rel, relf, i, i);
}

template <class F, int NV = 3>
int run_select(hipStream_t st, const PanelGeom &g, const F &f, const SelectArgs &s, bool write)
{
    const int64_t nrows = g.row1 - g.row0;
    if (nrows <= 0) return 0;
    const unsigned grid = (unsigned)(nrows < SELECT_MAX_GRID ? nrows : SELECT_MAX_GRID);
    const int all = std::isfinite(s.cutoff) ? 0 : 1;
    SelOut o{s.idx1, s.idx2, s.v0, s.v1, s.kin, s.capacity, s.v2};
    if (write)
        hipLaunchKernelGGL((select_kernel<F, true, NV>), dim3(grid), dim3(64 * SEL_WAVES), 0, st, g, f, s.sel, all, s.cutoff, s.counts, s.offsets, o);
    else
        hipLaunchKernelGGL((select_kernel<F, false, NV>), dim3(grid), dim3(64 * SEL_WAVES), 0, st, g, f, s.sel, all, s.cutoff, s.counts, s.offsets, o);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

// a GRM kind's count pass, write pass or diagonal
template <class G>
int run_select_grm(hipStream_t st, const PanelGeom &g, const G &f, const SelectArgs &s, SelPass pass, double *diag)
{
    if (pass != SEL_DIAG) return run_select<SelOne<G>, 1>(st, g, SelOne<G>{f}, s, pass == SEL_WRITE);
    const int64_t nrows = (g.row1 < g.N ? g.row1 : g.N) - g.row0;
    if (nrows <= 0) return 0;
    hipLaunchKernelGGL(select_diag_kernel<G>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, g, f, diag);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int64_t select_segments(const PanelGeom &g) { return (g.row1 > g.row0 ? g.row1 - g.row0 : 0) * SEL_WAVES; }

int launch_select_scan(hipStream_t st, const uint32_t *counts, int64_t n_seg, int64_t *offsets)
{
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, st, counts, n_seg, offsets);
    SNPGPU_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_select_king_robust(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const int32_t *family, const SelectArgs &s, bool write)
{
    SelKingRobust f{KingRobustArgs{acc, g.rows_pad * g.ncols_pad, family}};
    return run_select(st, g, f, s, write);
}

int launch_select_king_homo(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *facc, double fscale, const double *w_const,
                            const double *msum, const uint32_t *called, const uint32_t *nosh, const SelectArgs &s, bool write)
{
    SelKingHomo f{KingHomoArgs{acc, facc, g.rows_pad * g.ncols_pad, fscale, w_const, msum, g.col0, g.ncols_pad, called, nosh}};
    return run_select(st, g, f, s, write);
}

int launch_select_mom(hipStream_t st, const PanelGeom &g, const uint32_t *acc, const double *e, int constraint, const SelectArgs &s, bool write)
{
    SelMom f{MomArgs{acc, g.rows_pad * g.ncols_pad, e[0], e[1], e[2], e[3], e[4], constraint}};
    return run_select(st, g, f, s, write);
}

int launch_select_pcr(hipStream_t st, const PcrView &v, int64_t n, const double *e, bool probs, const SelectArgs &s, bool write)
{
    const PanelGeom g{n, v.row0, v.row1, v.col0, v.row1 - v.row0, v.ld, 0};
    SelPcr f{v, e, probs ? 1 : 0};
    return run_select<SelPcr, 4>(st, g, f, s, write);
}

int launch_select_gcta(hipStream_t st, const PanelGeom &g, const double *num, const uint32_t *miss, const uint32_t *miss_diag,
                       const unsigned long long *d_nlocus, const double *colterm, const double *uvterm, const SelectArgs &s, SelPass pass,
                       double *diag)
{
    SelGcta f{GctaArgs{num, miss, d_nlocus, miss_diag, colterm, uvterm, g.row0, g.col0, g.ncols_pad}};
    return run_select_grm(st, g, f, s, pass, diag);
}

int launch_select_cov(hipStream_t st, const PanelGeom &g, const double *num, double scale, const SelectArgs &s, SelPass pass, double *diag)
{
    SelCov f{CovArgs{num, scale}};
    return run_select_grm(st, g, f, s, pass, diag);
}

int launch_select_eigmix(hipStream_t st, const PanelGeom &g, const double *num, const double *dd, const uint32_t *het, const double *dmiss,
                         const double *dsq, const double *d_sumden, int diagadj, double scale, const SelectArgs &s, SelPass pass, double *diag)
{
    SelEigmix f{EigmixArgs{num, dd, het, dmiss, dsq, d_sumden, diagadj, scale}};
    return run_select_grm(st, g, f, s, pass, diag);
}

int launch_select_beta(hipStream_t st, const PanelGeom &g, const uint32_t *acc, int mode, double avg, double mn, const SelectArgs &s,
                       SelPass pass, double *diag)
{
    SelBeta f{BetaArgs{acc, g.rows_pad * g.ncols_pad, mode, avg, mn}};
    return run_select_grm(st, g, f, s, pass, diag);
}

}  // namespace snpgpu
