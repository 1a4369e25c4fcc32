// What kernels_admix.hip and its host layer admix.hip share: the segment geometry of the sums and the launch declarations
// (include/snpgpu.h section 1s).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace snpgpu {

constexpr int ADMIX_MAX_POP = 32;
// The owners of the sums.  A per-SNP sum over the samples (u, v, the SNP's part of L) is cut at the ABSOLUTE sample indices
// s * ADMIX_SSEG: one thread adds the called samples of a segment in ascending order, the segments are folded in ascending order.
// A per-sample sum over the SNPs (a) is cut at the ABSOLUTE SNP indices s * ADMIX_JSEG in the same way; a segment that an internal
// block leaves unfinished is carried in memory and continued, in order, by the next block.  Neither cut depends on the feeds or on
// the internal block, so neither do the bits.
constexpr int ADMIX_SSEG = 4096;        // a multiple of the 64 samples of one 16-byte load
constexpr int ADMIX_JSEG = 1024;        // a multiple of 16

struct AdmixState {
    const uint8_t *rows;    // resident 2-bit rows [m][rbr], code 3 = missing; rbr a multiple of 16, the padding bytes 0xFF
    int64_t rbr, n, m;
    int K;
    const double *Q;        // [n][K]
    const double *F;        // [m][K]
};

// SNPs [j0, j1) against all samples: lpart [n_sseg][m] and, with uv, upart / vpart [n_sseg][m][K] (sum_i w1 q_ik, sum_i w0 q_ik)
int launch_admix_snp(hipStream_t st, const AdmixState &s, int64_t j0, int64_t j1, bool uv, double *upart, double *vpart, double *lpart);
// all samples against SNPs [j0, j1): apart [n_jseg][n][K], the segment that holds j0 continued where j0 is not its first SNP
int launch_admix_samp(hipStream_t st, const AdmixState &s, int64_t j0, int64_t j1, double *apart);
// after the last block: F' [m][K] (NULL: F stays) and lsnp [m] from the segments' partial sums; Q' [n][K]; L = the sum of lsnp
int launch_admix_fold_snp(hipStream_t st, const AdmixState &s, const double *upart, const double *vpart, const double *lpart, double f_min,
                          double *Fnew, double *lsnp);
int launch_admix_fold_samp(hipStream_t st, const AdmixState &s, const double *apart, double *Qnew);
int launch_admix_loglik(hipStream_t st, const double *lsnp, int64_t m, double *out);

}  // namespace snpgpu
