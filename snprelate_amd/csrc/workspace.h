// What the other host units (grm_merge.hip, pca_randomized.hip) need from the genotype working space of workspace.hip.
#pragma once
#include <functional>
#include <vector>

#include "snpgpu_internal.h"

namespace snpgpu {

constexpr int64_t WS_BLOCK = 8192;  // SNPs per feed; plays the role of the reference's cache-sized block

int need_ws(const char *fn);        // refuses (with fn's name) while no working space is set
int64_t ws_n_samp();
int64_t ws_n_snp();                 // the currently selected SNPs
int ws_device();

// per-SNP sum / num (/ heterozygote count) over the selected SNPs, on the device (launch_snp_stats)
int ws_stats(std::vector<int32_t> &sum, std::vector<int32_t> &num, std::vector<int32_t> *het = nullptr);

// The block loop of the reference's CXxx::Run: f(rows, i0, nb) for the selected SNPs [i0, i0 + nb) in blocks of WS_BLOCK, `rows` =
// their gathered 2-bit host rows.  Stops at the first non-zero return, which it returns.
int ws_for_each_block(const std::function<int(const uint8_t *rows, int64_t i0, int64_t nb)> &f);

// A context of `kind` for the working space's samples and device, fed the selected SNPs by that loop; the caller destroys it.
int ws_run_stream(int kind, int bayesian, snpgpu_ctx **out);

// All selected rows in one host block: refuses without a working space, with fewer than min_samp samples (callers ask for two or
// none) or without a selected SNP.
int ws_all_rows(const char *fn, int64_t min_samp, std::vector<uint8_t> &buf);

struct ProjGuard {
    snpgpu_proj *p = nullptr;
    ~ProjGuard() { if (p) snpgpu_proj_destroy(p); }
};
int proj_open(int n_eig, ProjGuard &g);     // a projector of the working space's samples and device, WS_BLOCK SNPs per block

// the pairs kept by snpgpu_gnrPCRelatePairs (pcrelate.hip) go with the working space: snpgpu_ws_clear releases them
void ws_pcr_pairs_clear();

// grm_avg_value, src/genPCA.cpp:1605: written by snpgpu_gnrGRM, snpgpu_gnrIBD_Beta and snpgpu_gnrGRMMerge, read by snpgpu_gnrGRM_avg_val
extern double g_grm_avg_value;

}  // namespace snpgpu
