// Launch geometry of the PCA projection kernels (kernels_proj.hip): how many workgroups of four 64-row groups, how many column
// passes, and into how many parts the reduction range is split.  Integer logic without HIP, so that tests/proj_grid_check.cpp can
// print it on the CPU and tests/test_cpu_proj_grid.py can hold every shape of the GPU tests to the geometry it is there for.
#pragma once
#include <cstdint>

namespace snpgpu {

constexpr int PJ_KC_CORR = 8;     // output columns per wave pass of the SNP-side kernels (16 measured slower)
constexpr int PJ_KC = 16;         //   ... of the sample-side kernel

// grid (gx, gy, split); every part of the split reduces `per` samples (SNP side) or SNPs (sample side), the last one what is left
struct ProjGrid { int64_t gx, gy, split, per; };

// SNP side: lane = SNP, reduction over the N samples
inline ProjGrid proj_snp_grid(int64_t N, int64_t n_snp, int k)
{
    const int kc = PJ_KC_CORR;
    const int64_t gx = (n_snp + 255) / 256, gy = (k + kc - 1) / kc;
    // about 8 waves per SIMD: split the samples when SNP groups x column passes are few
    int64_t split = (8192 + gx * 4 * gy - 1) / (gx * 4 * gy);
    if (split < 1) split = 1;
    if (split > 64) split = 64;
    int64_t per = ((N + split - 1) / split + 7) & ~(int64_t)7;
    if (per < 256) per = 256;
    split = (N + per - 1) / per;
    return ProjGrid{gx, gy, split, per};
}

// sample side: lane = sample, reduction over the n_snp SNPs of one block
inline ProjGrid proj_samp_grid(int64_t N, int64_t n_snp, int k)
{
    const int64_t groups = (N + 63) / 64;
    // enough waves to fill the chip: split the SNP range when there are few sample groups
    int64_t split = (4096 + groups - 1) / groups;
    if (split < 1) split = 1;
    if (split > 64) split = 64;
    int64_t per = (n_snp + split - 1) / split;
    if (per < 64) per = 64;
    split = (n_snp + per - 1) / per;
    return ProjGrid{(groups + 3) / 4, (k + PJ_KC - 1) / PJ_KC, split, per};
}

}  // namespace snpgpu
