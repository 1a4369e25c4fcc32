// C ABI of libsnpgpu, level (2): host-side mirrors of the reference's registered `.Call`
// routines for this path (src/SNPRelate.cpp:1154-1205) over an in-memory genotype matrix.
// (snpgpu_gnrGRMMerge: grm_merge.hip; snpgpu_gnrPCA_randomized: pca_randomized.hip; the eigen routes: eigen_dense.hip.)
//
// The reference keeps an implicit process-global working space (GWAS::MCWorkingGeno,
// src/dGenGWAS.cpp:2000) that gnrSetGenoSpace / gnrSelSNP_Base set and the compute calls
// consume; g_ws below plays that role.  In an R deployment the GDS-backed reader is kept and
// feeds level (1) directly; this layer exists for hosts without gdsfmt.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "eigen.h"
#include "workspace.h"

using namespace snpgpu;

namespace {

struct WorkSpace {
    bool set = false;
    int device = 0;
    int64_t n_snp_all = 0, n_samp = 0, rb = 0;  // rb = ceil(n_samp/4) bytes per SNP row
    std::vector<uint8_t> packed;                // [n_snp_all][rb] 2-bit rows
    std::vector<int64_t> sel;                   // indices of the currently selected SNPs
    // the selection kept by snpgpu_gnrIBDPairs for snpgpu_gnrIBDPairs_get
    std::vector<int32_t> pair_idx1, pair_idx2;
    std::vector<double> pair_v0, pair_v1, pair_kin;
    std::vector<int32_t> grm_idx1, grm_idx2;            // the sparse GRM of the last snpgpu_gnrGRMPairs
    std::vector<double> grm_value, grm_diag;
    double grm_pairs_avg = 0;
};
WorkSpace g_ws;

// gather the selected SNP rows [i0,i1) into a contiguous 2-bit block
void gather_block(int64_t i0, int64_t i1, std::vector<uint8_t> &buf)
{
    buf.resize((size_t)(i1 - i0) * (size_t)g_ws.rb);
    for (int64_t i = i0; i < i1; i++)
        memcpy(&buf[(size_t)(i - i0) * g_ws.rb], &g_ws.packed[(size_t)g_ws.sel[i] * g_ws.rb], (size_t)g_ws.rb);
}

snpgpu_opts ws_opts()
{
    snpgpu_opts o{};
    o.device = g_ws.device;
    return o;
}

// run the block loop of CXxx::Run over the selected SNPs
int run_stream(int kind, int bayesian, snpgpu_ctx **out)
{
    snpgpu_opts o = ws_opts();
    o.bayesian = bayesian;
    o.max_block_snps = WS_BLOCK;
    snpgpu_ctx *c = nullptr;
    if (snpgpu_create(kind, g_ws.n_samp, &o, &c)) return 1;
    if (ws_for_each_block([&](const uint8_t *rows, int64_t, int64_t nb) {
            return snpgpu_feed(c, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST);
        })) {
        snpgpu_destroy(c);
        return 1;
    }
    *out = c;
    return 0;
}

struct CtxGuard {
    snpgpu_ctx *c = nullptr;
    ~CtxGuard() { if (c) snpgpu_destroy(c); }
};

// k eigenvalues, then NaN up to n (src/genPCA.cpp:1343-1345)
void eigval_nan_padded(const std::vector<double> &w, double *eigval, int64_t n)
{
    if (!eigval) return;
    for (size_t i = 0; i < w.size(); i++) eigval[i] = w[i];
    for (int64_t i = (int64_t)w.size(); i < n; i++) eigval[i] = std::numeric_limits<double>::quiet_NaN();
}

}  // namespace

namespace snpgpu {

double g_grm_avg_value = 0;

int need_ws(const char *fn)
{
    if (!g_ws.set) { set_error(std::string(fn) + ": no genotype working space (call snpgpu_ws_set_geno first)"); return 1; }
    return 0;
}

int ws_run_stream(int kind, int bayesian, snpgpu_ctx **out) { return run_stream(kind, bayesian, out); }

int64_t ws_n_samp() { return g_ws.n_samp; }
int64_t ws_n_snp() { return (int64_t)g_ws.sel.size(); }
int ws_device() { return g_ws.device; }

int ws_for_each_block(const std::function<int(const uint8_t *rows, int64_t i0, int64_t nb)> &f)
{
    std::vector<uint8_t> buf;
    const int64_t L = (int64_t)g_ws.sel.size();
    for (int64_t i0 = 0; i0 < L; i0 += WS_BLOCK) {
        const int64_t i1 = std::min(L, i0 + WS_BLOCK);
        gather_block(i0, i1, buf);
        if (const int rc = f(buf.data(), i0, i1 - i0)) return rc;
    }
    return 0;
}

int ws_all_rows(const char *fn, int64_t min_samp, std::vector<uint8_t> &buf)
{
    if (need_ws(fn)) return 1;
    const int64_t L = (int64_t)g_ws.sel.size();
    if (g_ws.n_samp < min_samp) { set_error(std::string(fn) + ": at least two samples are needed"); return 1; }
    if (L < 1) { set_error(std::string(fn) + ": no SNP in the working dataset"); return 1; }
    gather_block(0, L, buf);
    return 0;
}

int ws_stats(std::vector<int32_t> &sum, std::vector<int32_t> &num, std::vector<int32_t> *het)
{
    const int64_t L = (int64_t)g_ws.sel.size();
    sum.assign((size_t)L, 0);
    num.assign((size_t)L, 0);
    if (het) het->assign((size_t)L, 0);
    if (L == 0) return 0;
    SNPGPU_HIP_CHECK(hipSetDevice(g_ws.device));
    const int64_t N = g_ws.n_samp, RB = (N + 255) / 256 * 64;
    DevBuf raw, packed, dsum, dnum, dhet, dmiss;
    if (raw.alloc((size_t)WS_BLOCK * g_ws.rb) | packed.alloc((size_t)WS_BLOCK * RB) | dsum.alloc(sizeof(int32_t) * WS_BLOCK) |
        dnum.alloc(sizeof(int32_t) * WS_BLOCK) | dhet.alloc(sizeof(int32_t) * WS_BLOCK) | dmiss.alloc(8))
        return 1;
    return ws_for_each_block([&](const uint8_t *rows, int64_t i0, int64_t nb) {
        hipError_t e = hipMemcpy(raw.p, rows, (size_t)nb * (size_t)g_ws.rb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(dmiss.p, 0, 8);
        if (e != hipSuccess) { set_error(std::string("ws_stats: ") + hipGetErrorString(e)); return 1; }
        if (launch_repack(nullptr, raw.p, SNPGPU_GENO_PACKED2, nb, N, (uint8_t *)packed.p, RB) |
            launch_snp_stats(nullptr, (const uint8_t *)packed.p, RB, nb, N, (int32_t *)dsum.p, (int32_t *)dnum.p,
                             (unsigned long long *)dmiss.p, (int32_t *)dhet.p))
            return 1;
        e = hipMemcpy(&sum[i0], dsum.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&num[i0], dnum.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost);
        if (e == hipSuccess && het) e = hipMemcpy(&(*het)[i0], dhet.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_error(std::string("ws_stats: ") + hipGetErrorString(e)); return 1; }
        return 0;
    });
}

int proj_open(int n_eig, ProjGuard &g)
{
    snpgpu_opts o = ws_opts();
    o.max_block_snps = WS_BLOCK;
    return snpgpu_proj_create(g_ws.n_samp, n_eig, &o, &g.p);
}

}  // namespace snpgpu

extern "C" {

int snpgpu_ws_set_geno(const void *geno, int64_t n_snp, int64_t n_samp, int format, int device)
{
    if (!geno || n_snp <= 0 || n_samp <= 0) { set_error("snpgpu_ws_set_geno: invalid arguments"); return 1; }
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) { set_error("snpgpu_ws_set_geno: invalid format"); return 1; }
    int ndev = 0;
    SNPGPU_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("snpgpu_ws_set_geno: invalid device ordinal"); return 1; }
    g_ws.set = false;
    g_ws.device = device;
    g_ws.n_snp_all = n_snp; g_ws.n_samp = n_samp; g_ws.rb = (n_samp + 3) / 4;
    g_ws.packed.assign((size_t)n_snp * g_ws.rb, 0);
    const uint8_t *src = (const uint8_t *)geno;
    if (format == SNPGPU_GENO_PACKED2) {
        memcpy(g_ws.packed.data(), src, g_ws.packed.size());
    } else {
        for (int64_t l = 0; l < n_snp; l++) {
            uint8_t *row = &g_ws.packed[(size_t)l * g_ws.rb];
            const uint8_t *g = src + (size_t)l * n_samp;
            for (int64_t i = 0; i < n_samp; i++) {
                unsigned v = g[i] > 3 ? 3u : g[i];
                row[i >> 2] |= (uint8_t)(v << (2 * (i & 3)));
            }
        }
    }
    const int tail = (int)(g_ws.rb * 4 - n_samp);  // padding codes are stored as missing
    if (tail)
        for (int64_t l = 0; l < n_snp; l++) g_ws.packed[(size_t)(l + 1) * g_ws.rb - 1] |= (uint8_t)(0xFF << (2 * (4 - tail)));
    g_ws.sel.resize((size_t)n_snp);
    for (int64_t l = 0; l < n_snp; l++) g_ws.sel[(size_t)l] = l;
    g_ws.set = true;
    return 0;
}

int snpgpu_ws_clear(void)
{
    g_ws = WorkSpace();
    ws_pcr_pairs_clear();
    return 0;
}

int snpgpu_ws_get_geno_dim(int64_t *n_snp, int64_t *n_samp)
{
    if (need_ws("snpgpu_ws_get_geno_dim")) return 1;
    if (n_snp) *n_snp = (int64_t)g_ws.sel.size();
    if (n_samp) *n_samp = g_ws.n_samp;
    return 0;
}

// Get_AF_MR_perSNP, src/dGenGWAS.cpp:472-552 (RDim_Sample_X_SNP branch)
int snpgpu_ws_snp_rate_freq(double *af, double *maf, double *missrate)
{
    if (need_ws("snpgpu_ws_snp_rate_freq")) return 1;
    std::vector<int32_t> sum, num;
    if (ws_stats(sum, num)) return 1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t l = 0; l < sum.size(); l++) {
        const double F = (num[l] > 0) ? ((double)sum[l] / (2 * num[l])) : nan;
        if (af) af[l] = F;
        if (maf) maf[l] = std::isnan(F) ? nan : std::min(F, 1 - F);
        if (missrate) missrate[l] = 1 - ((double)num[l]) / (double)g_ws.n_samp;
    }
    return 0;
}

// CdBaseWorkSpace::Select_SNP_Base, src/dGenGWAS.cpp:361-397
int snpgpu_ws_sel_snp_base(int remove_mono, double maf, double missrate, int32_t *n_excluded, uint8_t *sel_out)
{
    if (need_ws("snpgpu_ws_sel_snp_base")) return 1;
    std::vector<int32_t> sum, num;
    if (ws_stats(sum, num)) return 1;
    std::vector<int64_t> keep;
    int32_t excluded = 0;
    for (size_t l = 0; l < sum.size(); l++) {
        bool flag;
        if (num[l] > 0) {
            const double F = (double)sum[l] / (2 * num[l]);
            const double MAF = std::min(F, 1 - F);
            const double MR = 1 - ((double)num[l]) / (double)g_ws.n_samp;
            flag = true;
            if (remove_mono && MAF <= 0) flag = false;
            if (flag && MAF < maf) flag = false;
            if (flag && MR > missrate) flag = false;
        } else
            flag = false;
        if (sel_out) sel_out[l] = flag ? 1 : 0;
        if (flag) keep.push_back(g_ws.sel[l]); else excluded++;
    }
    g_ws.sel.swap(keep);
    if (n_excluded) *n_excluded = excluded;
    return 0;
}

// gnrSelSNP_Base_Ex(afreq, remove_mono, maf, missrate), src/SNPRelate.cpp:215-239 -> Select_SNP_Base_Ex,
// src/dGenGWAS.cpp:399-469: the monomorphic / MAF tests use the CALLER's allele frequencies (a non-finite one drops
// the SNP), only the missing rate comes from the genotypes.
int snpgpu_ws_sel_snp_base_ex(const double *afreq, int remove_mono, double maf, double missrate, int32_t *n_excluded,
                              uint8_t *sel_out)
{
    if (need_ws("snpgpu_ws_sel_snp_base_ex")) return 1;
    if (!afreq) { set_error("snpgpu_ws_sel_snp_base_ex: afreq is NULL"); return 1; }
    std::vector<int32_t> sum, num;
    if (ws_stats(sum, num)) return 1;
    std::vector<int64_t> keep;
    int32_t excluded = 0;
    for (size_t l = 0; l < num.size(); l++) {
        bool flag = true;
        if (std::isfinite(afreq[l])) {
            const double MF = std::min(afreq[l], 1 - afreq[l]);
            const double MR = 1.0 - (double)num[l] / (double)g_ws.n_samp;
            if (remove_mono && MF <= 0) flag = false;
            if (flag && MF < maf) flag = false;
            if (flag && MR > missrate) flag = false;
        } else
            flag = false;
        if (sel_out) sel_out[l] = flag ? 1 : 0;
        if (flag) keep.push_back(g_ws.sel[l]); else excluded++;
    }
    g_ws.sel.swap(keep);
    if (n_excluded) *n_excluded = excluded;
    return 0;
}

int snpgpu_gnrIBSNum(int, int, int32_t *ibs0, int32_t *ibs1, int32_t *ibs2)
{
    if (need_ws("snpgpu_gnrIBSNum")) return 1;
    CtxGuard g;
    if (run_stream(SNPGPU_IBS, 0, &g.c)) return 1;
    return snpgpu_ibs_num(g.c, ibs0, ibs1, ibs2, 0, SNPGPU_HOST);
}

int snpgpu_gnrIBSAve(int, int use_matrix, int, double *out)
{
    if (need_ws("snpgpu_gnrIBSAve")) return 1;
    CtxGuard g;
    if (run_stream(SNPGPU_IBS, 0, &g.c)) return 1;
    return snpgpu_ibs_ave(g.c, out, use_matrix ? 1 : 0, SNPGPU_HOST);
}

int snpgpu_gnrIBD_KING_Robust(const int32_t *family, int, int use_matrix, int, double *ibs0, double *kinship)
{
    if (need_ws("snpgpu_gnrIBD_KING_Robust")) return 1;
    if ((int64_t)g_ws.sel.size() >= 1073741824LL) {  // src/genKING.cpp:598-602
        set_error("The number of SNPs should be less than 1,073,741,824.");
        return 1;
    }
    CtxGuard g;
    if (run_stream(SNPGPU_KING_ROBUST, 0, &g.c)) return 1;
    return snpgpu_king_robust(g.c, family, ibs0, kinship, use_matrix ? 1 : 0, SNPGPU_HOST);
}

int snpgpu_gnrIBD_KING_Homo(int, int use_matrix, int, double *k0, double *k1)
{
    if (need_ws("snpgpu_gnrIBD_KING_Homo")) return 1;
    CtxGuard g;
    if (run_stream(SNPGPU_KING_HOMO, 0, &g.c)) return 1;
    return snpgpu_king_homo(g.c, k0, k1, use_matrix ? 1 : 0, SNPGPU_HOST);
}

// gnrDiss, src/genIBS.cpp:652-683: always the full n x n matrix
int snpgpu_gnrDiss(int, int, double *out)
{
    if (need_ws("snpgpu_gnrDiss")) return 1;
    CtxGuard g;
    if (run_stream(SNPGPU_DISS, 0, &g.c)) return 1;
    return snpgpu_diss(g.c, out, 0, SNPGPU_HOST);
}

// gnrGRM method switch, src/genPCA.cpp:1633-1710
int snpgpu_gnrGRM(int, const char *method, int use_matrix, int, double *out)
{
    if (need_ws("snpgpu_gnrGRM")) return 1;
    if (!method) { set_error("Invalid 'method'!"); return 1; }
    const int64_t n = g_ws.n_samp;
    CtxGuard g;
    if (strcmp(method, "Eigenstrat") == 0) {
        if (run_stream(SNPGPU_PCA_COV, 0, &g.c)) return 1;
        return snpgpu_pca_cov(g.c, out, use_matrix ? 1 : 0, 1, 0.0, nullptr, SNPGPU_HOST);
    } else if (strcmp(method, "GCTA") == 0) {
        if (run_stream(SNPGPU_GRM_GCTA, 0, &g.c)) return 1;
        return snpgpu_grm_gcta(g.c, out, use_matrix ? 1 : 0, SNPGPU_HOST);
    } else if (strcmp(method, "Corr") == 0) {
        // always a full matrix, src/genPCA.cpp:1658-1685
        if (run_stream(SNPGPU_GRM_GCTA, 0, &g.c)) return 1;
        if (snpgpu_grm_gcta(g.c, out, 0, SNPGPU_HOST)) return 1;
        std::vector<double> diag((size_t)n);
        for (int64_t i = 0; i < n; i++) diag[(size_t)i] = sqrt(out[i + n * i]);
        for (int64_t i = 0; i < n; i++) {
            out[i + n * i] = 1;
            for (int64_t j = i + 1; j < n; j++)
                out[i + n * j] = out[j + n * i] = out[j + n * i] / (diag[(size_t)i] * diag[(size_t)j]);
        }
        return 0;
    }
    else if (strcmp(method, "EIGMIX") == 0) {      // CalcEigMixGRM: no diagonal adjustment, times 2
        if (run_stream(SNPGPU_EIGMIX, 0, &g.c)) return 1;
        return snpgpu_eigmix(g.c, 0, 2.0, out, use_matrix ? 1 : 0, SNPGPU_HOST);
    } else if (strcmp(method, "IndivBeta") == 0) {  // CalcIndivBetaGRM
        if (run_stream(SNPGPU_INDIV_BETA, 0, &g.c)) return 1;
        double avg = 0;
        if (snpgpu_indiv_beta(g.c, 2, out, &avg, use_matrix ? 1 : 0, SNPGPU_HOST)) return 1;
        g_grm_avg_value = avg;
        return 0;
    }
    set_error("Invalid 'method'!");  // src/genPCA.cpp:1710
    return 1;
}

int snpgpu_gnrGRM_avg_val(double *avg_val)
{
    if (avg_val) *avg_val = g_grm_avg_value;
    return 0;
}

// the expectations e[5] of gnrIBD_PLINK (Init_EPrIBD_IBS, src/genIBD.cpp:253-338) over the selected SNPs; afreq_out: double [n_snp] or NULL
static int ws_mom_expect(const double *allele_freq, double *afreq_out, double e[5])
{
    std::vector<int32_t> sum, num, het;
    if (ws_stats(sum, num, &het)) return 1;
    // E[IBS state | IBD state] per SNP as polynomials in the allele frequencies p, q = 1 - p (PLINK's method of moments;
    // the reference's Init_EPrIBD_IBS, src/genIBD.cpp:253-338).  Each monomial c p^a q^b stands for drawing a copies of
    // allele A and b of allele B; with frequencies estimated from the same sample the draws are without replacement, and
    // the unbiased estimate multiplies the monomial by   [x]_a / x^a * [y]_b / y^b * T^(a+b) / [T]_(a+b)
    // ([v]_k = v (v-1) ... (v-k+1); x, y = allele counts, T = x + y).  Caller-supplied frequencies take the plain monomials.
    struct Mono { double c; int a, b; };
    static const Mono E00[] = {{2, 2, 2}};
    static const Mono E01[] = {{4, 3, 1}, {4, 1, 3}};
    static const Mono E02[] = {{1, 0, 4}, {1, 4, 0}, {4, 2, 2}};
    static const Mono E11[] = {{2, 2, 1}, {2, 1, 2}};
    static const Mono E12[] = {{1, 3, 0}, {1, 0, 3}, {1, 2, 1}, {1, 1, 2}};
    static const struct { const Mono *m; int n; } POLY[5] = {{E00, 1}, {E01, 2}, {E02, 3}, {E11, 2}, {E12, 4}};
    auto falling = [](double v, int k) { double r = 1; for (int m = 1; m < k; m++) r *= (v - m) / v; return r; };   // [v]_k / v^k
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double tot[5] = {0, 0, 0, 0, 0};
    long nValid = 0;
    for (size_t l = 0; l < sum.size(); l++) {
        const long nAB = het[l], nAA = (sum[l] - het[l]) / 2, nBB = num[l] - nAA - nAB;
        const double x = allele_freq ? 0.0 : 2.0 * nAA + nAB, y = allele_freq ? 0.0 : 2.0 * nBB + nAB, T = x + y;
        double p = allele_freq ? allele_freq[l] : (T > 0 ? x / T : nan);
        if (allele_freq && std::isfinite(p) && (p < 0 || p > 1)) p = nan;
        if (afreq_out) afreq_out[l] = p;
        const double q = 1 - p;
        double val[5];
        bool finite = true;
        for (int k = 0; k < 5; k++) {
            double v = 0;
            for (int t = 0; t < POLY[k].n; t++) {
                const Mono &m = POLY[k].m[t];
                double term = m.c;
                for (int r = 0; r < m.a; r++) term *= p;
                for (int r = 0; r < m.b; r++) term *= q;
                if (!allele_freq) term *= falling(x, m.a) * falling(y, m.b) / falling(T, m.a + m.b);
                v += term;
            }
            val[k] = v;
            finite = finite && std::isfinite(v);
        }
        if (finite) { for (int k = 0; k < 5; k++) tot[k] += val[k]; nValid++; }      // SNPs with a non-finite term are skipped
    }
    const double s00 = tot[0], s01 = tot[1], s02 = tot[2], s11 = tot[3], s12 = tot[4];
    e[0] = s00 / nValid; e[1] = s01 / nValid; e[2] = s02 / nValid; e[3] = s11 / nValid; e[4] = s12 / nValid;
    return 0;
}

// gnrIBD_PLINK, src/genIBS.cpp:558-639 with Init_EPrIBD_IBS, src/genIBD.cpp:253-338
int snpgpu_gnrIBD_PLINK(int, const double *allele_freq, int kinship_constraint, int use_matrix, int, double *k0,
                        double *k1, double *afreq_out)
{
    if (need_ws("snpgpu_gnrIBD_PLINK")) return 1;
    double e[5];
    if (ws_mom_expect(allele_freq, afreq_out, e)) return 1;
    CtxGuard g;
    if (run_stream(SNPGPU_IBS, 0, &g.c)) return 1;
    return snpgpu_ibd_mom(g.c, e, kinship_constraint, k0, k1, use_matrix ? 1 : 0, SNPGPU_HOST);
}

// Related pairs of the working space (include/snpgpu.h): one accumulation, a count, then the selection itself -- host memory
// proportional to the number of selected pairs, no n x n matrix
int snpgpu_gnrIBDPairs(int what, const int32_t *family, const double *allele_freq, int kinship_constraint, double kinship_cutoff,
                       const uint8_t *samp_sel, int, int, int64_t *n_found)
{
    if (what != SNPGPU_SEL_KING_ROBUST && what != SNPGPU_SEL_KING_HOMO && what != SNPGPU_SEL_MOM) {
        set_error("snpgpu_gnrIBDPairs: invalid 'what' (SNPGPU_SEL_KING_ROBUST, SNPGPU_SEL_KING_HOMO or SNPGPU_SEL_MOM)");
        return 1;
    }
    if (need_ws("snpgpu_gnrIBDPairs")) return 1;
    if (what == SNPGPU_SEL_KING_ROBUST && (int64_t)g_ws.sel.size() >= 1073741824LL) {  // src/genKING.cpp:598-602
        set_error("The number of SNPs should be less than 1,073,741,824.");
        return 1;
    }
    g_ws.pair_idx1.clear(); g_ws.pair_idx2.clear(); g_ws.pair_v0.clear(); g_ws.pair_v1.clear(); g_ws.pair_kin.clear();
    double e[5] = {0, 0, 0, 0, 0};
    if (what == SNPGPU_SEL_MOM && ws_mom_expect(allele_freq, nullptr, e)) return 1;
    snpgpu_sel_opts o{};
    o.what = what;
    o.kinship_constraint = kinship_constraint;
    o.family = family;
    o.e = what == SNPGPU_SEL_MOM ? e : nullptr;
    o.kinship_cutoff = kinship_cutoff;
    o.samp_sel = samp_sel;
    CtxGuard g;
    if (run_stream(select_kind(what), 0, &g.c)) return 1;
    int64_t n = 0;
    if (snpgpu_select_pairs(g.c, &o, 0, nullptr, nullptr, nullptr, nullptr, nullptr, SNPGPU_HOST, &n)) return 1;
    if (n > 0) {
        g_ws.pair_idx1.resize((size_t)n); g_ws.pair_idx2.resize((size_t)n);
        g_ws.pair_v0.resize((size_t)n); g_ws.pair_v1.assign((size_t)n, 0.0); g_ws.pair_kin.resize((size_t)n);
        int64_t again = 0;
        if (snpgpu_select_pairs(g.c, &o, n, g_ws.pair_idx1.data(), g_ws.pair_idx2.data(), g_ws.pair_v0.data(), g_ws.pair_v1.data(),
                                g_ws.pair_kin.data(), SNPGPU_HOST, &again))
            return 1;
        if (again != n) { set_error("snpgpu_gnrIBDPairs: the selection changed between the count and the fetch"); return 1; }
    }
    if (n_found) *n_found = n;
    return 0;
}

int snpgpu_gnrIBDPairs_get(int32_t *idx1, int32_t *idx2, double *v0, double *v1, double *kinship)
{
    const size_t n = g_ws.pair_idx1.size();
    if (n == 0) return 0;
    if (idx1) memcpy(idx1, g_ws.pair_idx1.data(), sizeof(int32_t) * n);
    if (idx2) memcpy(idx2, g_ws.pair_idx2.data(), sizeof(int32_t) * n);
    if (v0) memcpy(v0, g_ws.pair_v0.data(), sizeof(double) * n);
    if (v1) memcpy(v1, g_ws.pair_v1.data(), sizeof(double) * n);
    if (kinship) memcpy(kinship, g_ws.pair_kin.data(), sizeof(double) * n);
    return 0;
}

// The sparse GRM of the working space (include/snpgpu.h): one accumulation, a count, then the selection itself, as snpgpu_gnrIBDPairs
int snpgpu_gnrGRMPairs(const char *method, double cutoff, const uint8_t *samp_sel, int, int, int64_t *n_found)
{
    const char *fn = "snpgpu_gnrGRMPairs";
    if (!method) { set_error(std::string(fn) + ": Invalid 'method'!"); return 1; }
    snpgpu_grm_sel_opts o{};
    if (strcmp(method, "GCTA") == 0) o.what = SNPGPU_SEL_GRM_GCTA;
    else if (strcmp(method, "Eigenstrat") == 0) o.what = SNPGPU_SEL_GRM_EIGENSTRAT;
    else if (strcmp(method, "EIGMIX") == 0) { o.what = SNPGPU_SEL_GRM_EIGMIX; o.mode = 0; o.scale = 2.0; }      // as snpgpu_gnrGRM
    else if (strcmp(method, "IndivBeta") == 0) { o.what = SNPGPU_SEL_GRM_INDIV_BETA; o.mode = 2; }
    else if (strcmp(method, "Corr") == 0) {
        set_error(std::string(fn) + ": method 'Corr' is not built for the sparse GRM (G_ij / sqrt(G_ii G_jj) needs the diagonal of every column, "
                                    "which a row panel does not hold)");
        return 1;
    } else {
        set_error(std::string(fn) + ": Invalid 'method' '" + method + "'!");
        return 1;
    }
    if (need_ws(fn)) return 1;
    o.cutoff = cutoff;
    o.samp_sel = samp_sel;
    g_ws.grm_idx1.clear(); g_ws.grm_idx2.clear(); g_ws.grm_value.clear(); g_ws.grm_diag.clear(); g_ws.grm_pairs_avg = 0;
    CtxGuard g;
    if (run_stream(select_grm_kind(o.what), 0, &g.c)) return 1;
    int64_t n = 0;
    if (snpgpu_select_grm(g.c, &o, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n)) return 1;
    g_ws.grm_idx1.resize((size_t)n); g_ws.grm_idx2.resize((size_t)n); g_ws.grm_value.resize((size_t)n);
    g_ws.grm_diag.resize((size_t)g_ws.n_samp);
    int64_t again = 0;
    // (capacity 0 takes no pair output: with no pair found only the diagonal and the average are fetched)
    if (snpgpu_select_grm(g.c, &o, n, n ? g_ws.grm_idx1.data() : nullptr, n ? g_ws.grm_idx2.data() : nullptr, n ? g_ws.grm_value.data() : nullptr,
                          g_ws.grm_diag.data(), &g_ws.grm_pairs_avg, &again))
        return 1;
    if (again != n) { set_error(std::string(fn) + ": the selection changed between the count and the fetch"); return 1; }
    if (n_found) *n_found = n;
    return 0;
}

int snpgpu_gnrGRMPairs_get(int32_t *idx1, int32_t *idx2, double *value, double *diag, double *avg_val)
{
    const size_t n = g_ws.grm_idx1.size();
    if (idx1 && n) memcpy(idx1, g_ws.grm_idx1.data(), sizeof(int32_t) * n);
    if (idx2 && n) memcpy(idx2, g_ws.grm_idx2.data(), sizeof(int32_t) * n);
    if (value && n) memcpy(value, g_ws.grm_value.data(), sizeof(double) * n);
    if (diag && !g_ws.grm_diag.empty()) memcpy(diag, g_ws.grm_diag.data(), sizeof(double) * g_ws.grm_diag.size());
    if (avg_val) *avg_val = g_ws.grm_pairs_avg;
    return 0;
}

int snpgpu_gnrIBD_Beta(int inbreeding, int, int use_matrix, int, double *out, double *avg_val)
{
    if (need_ws("snpgpu_gnrIBD_Beta")) return 1;
    CtxGuard g;
    if (run_stream(SNPGPU_INDIV_BETA, 0, &g.c)) return 1;
    double avg = 0;
    if (snpgpu_indiv_beta(g.c, inbreeding ? 1 : 0, out, &avg, use_matrix ? 1 : 0, SNPGPU_HOST)) return 1;
    g_grm_avg_value = avg;
    if (avg_val) *avg_val = avg;
    return 0;
}

// gnrEigMix, src/genEIGMIX.cpp:656-740
int snpgpu_gnrEigMix(int eigen_cnt, int, int diagadj, int, double *ibd, double *eigval, double *eigvec, double *afreq)
{
    if (need_ws("snpgpu_gnrEigMix")) return 1;
    const int64_t n = g_ws.n_samp;
    if (afreq) {
        std::vector<int32_t> sum, num;
        if (ws_stats(sum, num)) return 1;
        for (size_t l = 0; l < sum.size(); l++) afreq[l] = (num[l] > 0) ? (0.5 * sum[l] / num[l]) : 0.0;   // 0.5*avg_geno, :116
    }
    CtxGuard g;
    if (run_stream(SNPGPU_EIGMIX, 0, &g.c)) return 1;
    if (ibd && snpgpu_eigmix(g.c, diagadj, 1.0, ibd, 0, SNPGPU_HOST)) return 1;
    int k = eigen_cnt;
    if (k < 0 || k > n) k = (int)n;          // :676
    if ((eigval || eigvec) && k > 0) {
        // beyond the dense solver the coancestry matrix replaces the sums in place, block Krylov on the panel
        snpgpu_ctx *c = g.c;
        std::vector<double> w((size_t)k);
        if (ctx_topk_eigen(
                c, k, [=](double *A) { return snpgpu_eigmix(c, diagadj, 1.0, A, 0, SNPGPU_DEVICE); },
                [=](double *scale) { *scale = 1.0; return snpgpu_finalize_inplace(c, diagadj, 1.0); }, w.data(), eigvec, SNPGPU_HOST))
            return 1;
        eigval_nan_padded(w, eigval, n);
    }
    return 0;
}

// gnrPCA "exact", src/genPCA.cpp:1355-1452
int snpgpu_gnrPCA(int eigen_cnt, int, int bayesian, int, double *trace_xtx, double *genmat, double *eigval,
                  double *eigvec, double *trace_val)
{
    if (need_ws("snpgpu_gnrPCA")) return 1;
    const int64_t n = g_ws.n_samp;
    CtxGuard g;
    if (run_stream(SNPGPU_PCA_COV, bayesian, &g.c)) return 1;
    double tr = 0;
    if (snpgpu_pca_cov(g.c, genmat, 0, 1, 0.0, &tr, SNPGPU_HOST)) return 1;
    if (trace_xtx) *trace_xtx = tr;
    if (trace_val) *trace_val = (double)(n - 1);  // trace after the (n-1)/trace scaling, :1390
    if (eigval || eigvec) {
        if (eigen_cnt < 0) { set_error("Invalid 'eigen.cnt'."); return 1; }
        int k = eigen_cnt > n ? (int)n : eigen_cnt;
        if (k > 0) {
            std::vector<double> w((size_t)k);
            if (snpgpu_pca_eigen(g.c, k, w.data(), eigvec, SNPGPU_HOST)) return 1;
            eigval_nan_padded(w, eigval, n);
        }
    }
    return 0;
}

// gnrPCACorr, src/genPCA.cpp:1455-1484 (matrix result; the GDS-node variant Run2 appends the same blocks)
int snpgpu_gnrPCACorr(int len_eig, const double *eigvec, int, int, double *out)
{
    if (need_ws("snpgpu_gnrPCACorr")) return 1;
    if (!eigvec || !out || len_eig <= 0) { set_error("snpgpu_gnrPCACorr: invalid argument"); return 1; }
    ProjGuard g;
    if (proj_open(len_eig, g)) return 1;
    if (snpgpu_proj_set_eigvec(g.p, eigvec, SNPGPU_HOST)) return 1;
    return ws_for_each_block([&](const uint8_t *rows, int64_t i0, int64_t nb) {
        return snpgpu_proj_snp_corr(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST, out + (size_t)i0 * (size_t)len_eig, SNPGPU_HOST);
    });
}

// gnrPCASNPLoading, src/genPCA.cpp:1488-1531
int snpgpu_gnrPCASNPLoading(const double *eigval, const double *eigvec, int len_eig, double trace_xtx, int, int bayesian,
                            int, double *loading, double *afreq, double *scale)
{
    if (need_ws("snpgpu_gnrPCASNPLoading")) return 1;
    if (!eigval || !eigvec || !loading || !afreq || !scale || len_eig <= 0) {
        set_error("snpgpu_gnrPCASNPLoading: invalid argument");
        return 1;
    }
    const int64_t n = g_ws.n_samp;
    // scale eigenvectors with eigenvalues, :1499-1507
    std::vector<double> ev((size_t)n * (size_t)len_eig);
    const double sc = (double)(n - 1) / trace_xtx;
    for (int i = 0; i < len_eig; i++) {
        const double f = std::sqrt(sc / eigval[i]);
        for (int64_t j = 0; j < n; j++) ev[(size_t)i * n + j] = eigvec[(size_t)i * n + j] * f;
    }
    ProjGuard g;
    if (proj_open(len_eig, g)) return 1;
    if (snpgpu_proj_set_eigvec(g.p, ev.data(), SNPGPU_HOST)) return 1;
    return ws_for_each_block([&](const uint8_t *rows, int64_t i0, int64_t nb) {
        return snpgpu_proj_snp_loading(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST, bayesian,
                                       loading + (size_t)i0 * (size_t)len_eig, afreq + i0, scale + i0, SNPGPU_HOST);
    });
}

// gnrPCASampLoading, src/genPCA.cpp:1535-1562
int snpgpu_gnrPCASampLoading(int eigen_cnt, const double *snp_loadings, const double *avg_freq, const double *scale, int,
                             int, double *out)
{
    if (need_ws("snpgpu_gnrPCASampLoading")) return 1;
    if (!snp_loadings || !avg_freq || !scale || !out || eigen_cnt <= 0) {
        set_error("snpgpu_gnrPCASampLoading: invalid argument");
        return 1;
    }
    ProjGuard g;
    if (proj_open(eigen_cnt, g)) return 1;
    if (ws_for_each_block([&](const uint8_t *rows, int64_t i0, int64_t nb) {
            return snpgpu_proj_samp_loading_feed(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST,
                                                 snp_loadings + (size_t)i0 * (size_t)eigen_cnt, avg_freq + i0, scale + i0, SNPGPU_HOST);
        }))
        return 1;
    return snpgpu_proj_samp_loading(g.p, out, SNPGPU_HOST);
}

// EIGMIX: y = (g - 2 p) / sqrt(sum_snp 4 p (1 - p)) over the called genotypes (CEigMix_SNPLoad / CEigMix_SampleLoad,
// src/genEIGMIX.cpp:440-512, 516-620)
static void eigmix_norm(const double *afreq, int64_t L, std::vector<double> &avg, std::vector<double> &scale)
{
    double sum = 0;
    for (int64_t i = 0; i < L; i++) sum += 4 * afreq[i] * (1 - afreq[i]);
    const double sc = 1 / std::sqrt(sum);
    avg.resize((size_t)L); scale.assign((size_t)L, sc);
    for (int64_t i = 0; i < L; i++) avg[(size_t)i] = 2 * afreq[i];
}

// gnrEigMixSNPLoading, src/genEIGMIX.cpp:739-775
int snpgpu_gnrEigMixSNPLoading(const double *eigval, const double *eigvec, int len_eig, const double *afreq, int, int,
                               double *loading)
{
    if (need_ws("snpgpu_gnrEigMixSNPLoading")) return 1;
    if (!eigval || !eigvec || !afreq || !loading || len_eig <= 0) { set_error("snpgpu_gnrEigMixSNPLoading: invalid argument"); return 1; }
    const int64_t n = g_ws.n_samp, L = (int64_t)g_ws.sel.size();
    std::vector<double> ev((size_t)n * (size_t)len_eig), avg, scale;
    for (int i = 0; i < len_eig; i++) {          // scale eigenvectors with eigenvalues, :750-758
        const double f = std::sqrt(1 / eigval[i]);
        for (int64_t j = 0; j < n; j++) ev[(size_t)i * n + j] = eigvec[(size_t)i * n + j] * f;
    }
    eigmix_norm(afreq, L, avg, scale);
    ProjGuard g;
    if (proj_open(len_eig, g)) return 1;
    if (snpgpu_proj_set_eigvec(g.p, ev.data(), SNPGPU_HOST)) return 1;
    return ws_for_each_block([&](const uint8_t *rows, int64_t i0, int64_t nb) {
        return snpgpu_proj_snp_loading_ext(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST, avg.data() + i0, scale.data() + i0,
                                           SNPGPU_HOST, loading + (size_t)i0 * (size_t)len_eig, SNPGPU_HOST);
    });
}

// gnrEigMixSampLoading, src/genEIGMIX.cpp:777-803
int snpgpu_gnrEigMixSampLoading(int eigen_cnt, const double *snp_loadings, const double *afreq, int, int, double *out)
{
    if (need_ws("snpgpu_gnrEigMixSampLoading")) return 1;
    if (!snp_loadings || !afreq || !out || eigen_cnt <= 0) { set_error("snpgpu_gnrEigMixSampLoading: invalid argument"); return 1; }
    const int64_t L = (int64_t)g_ws.sel.size();
    std::vector<double> avg, scale;
    eigmix_norm(afreq, L, avg, scale);
    ProjGuard g;
    if (proj_open(eigen_cnt, g)) return 1;
    if (ws_for_each_block([&](const uint8_t *rows, int64_t i0, int64_t nb) {
            return snpgpu_proj_samp_loading_feed(g.p, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST,
                                                 snp_loadings + (size_t)i0 * (size_t)eigen_cnt, avg.data() + i0, scale.data() + i0,
                                                 SNPGPU_HOST);
        }))
        return 1;
    return snpgpu_proj_samp_loading(g.p, out, SNPGPU_HOST);
}

// gnrLDMat(method, NumSlide, MatTrim, NumThread, Verbose), src/genLD.cpp:957-1010: the selected SNPs in WS_BLOCK blocks
int snpgpu_gnrLDMat(int method, int64_t slide, int mat_trim, int num_thread, int, double *out)
{
    if (need_ws("snpgpu_gnrLDMat")) return 1;
    if (num_thread <= 0) { set_error("Invalid 'num.thread'."); return 1; }
    if (!out) { set_error("snpgpu_gnrLDMat: out is NULL"); return 1; }
    const snpgpu_opts o = ws_opts();
    snpgpu_ld *ld = nullptr;
    if (snpgpu_ld_create(g_ws.n_samp, (int64_t)g_ws.sel.size(), method, slide, mat_trim, &o, &ld)) return 1;
    int rc = ws_for_each_block([&](const uint8_t *rows, int64_t, int64_t nb) {
        return snpgpu_ld_feed(ld, rows, nb, SNPGPU_GENO_PACKED2, SNPGPU_HOST);
    });
    if (!rc) rc = snpgpu_ld_result(ld, out, SNPGPU_HOST);
    snpgpu_ld_destroy(ld);
    return rc;
}

// gnrLDpruning(StartIdx, pos_bp, slide_max_bp, slide_max_n, LD_threshold, method, NumThread, verbose), src/genLD.cpp:1014-1035:
// the selected SNPs (one chromosome, as the R loop sets them) in one host block
int snpgpu_gnrLDpruning(int64_t start_idx, const int32_t *pos_bp, int32_t slide_max_bp, int32_t slide_max_n, double ld_threshold,
                        int method, int num_thread, int, uint8_t *keep)
{
    if (need_ws("snpgpu_gnrLDpruning")) return 1;
    if (num_thread <= 0) { set_error("Invalid 'num.thread'."); return 1; }
    if (!pos_bp || !keep) { set_error("snpgpu_gnrLDpruning: NULL argument"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrLDpruning", 0, buf)) return 1;
    const snpgpu_opts o = ws_opts();
    return snpgpu_ld_prune(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, start_idx, pos_bp,
                           slide_max_bp, slide_max_n, ld_threshold, method, keep, &o, nullptr);
}

// snpgpu_ld_score on the selected SNPs (one chromosome, as the caller's loop sets them) in one host block
int snpgpu_gnrLDScore(const int32_t *pos_bp, int32_t slide_max_bp, int32_t slide_max_n, int method, int flags, int num_thread, int,
                      double *score, int32_t *n_valid, int32_t *n_window)
{
    if (need_ws("snpgpu_gnrLDScore")) return 1;
    if (num_thread <= 0) { set_error("Invalid 'num.thread'."); return 1; }
    if (!score) { set_error("snpgpu_gnrLDScore: NULL argument: score is NULL"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrLDScore", 0, buf)) return 1;
    const snpgpu_opts o = ws_opts();
    return snpgpu_ld_score(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, pos_bp, slide_max_bp,
                           slide_max_n, method, flags, score, n_valid, n_window, &o, nullptr);
}

// gnrIBD_MLE(AlleleFreq, KinshipConstraint, MaxIterCnt, RelTol, CoeffCorrect, method, IfOutNum, NumThread, Verbose),
// src/genIBD.cpp:1465-1548, on the selected SNPs (method 0 = EM only)
int snpgpu_gnrIBD_MLE(const double *allele_freq, int, int max_niter, double reltol, int coeff_correct, int method,
                      int out_num_iter, int num_thread, int, double *k0, double *k1, double *afreq, int32_t *niter)
{
    if (method == 1 || method == 2) {
        set_error(std::string("snpgpu_gnrIBD_MLE: method \"") + (method == 1 ? "downhill.simplex" : "Jacquard") +
                  "\" is not built on the GPU path (only \"EM\")");
        return 1;
    }
    if (method != 0) { set_error("Invalid MLE method!"); return 1; }
    if (num_thread <= 0) { set_error("Invalid 'num.thread'."); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrIBD_MLE", 2, buf)) return 1;
    return snpgpu_ibd_mle(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, allele_freq,
                          max_niter, reltol, coeff_correct, 0, 0, k0, k1, out_num_iter ? niter : nullptr, afreq, SNPGPU_HOST,
                          g_ws.device);
}

// the listed pairs of the selected samples (snpgdsIBDMLEPairs): EM, Est_PLINK_Kinship without the constraint as gnrIBD_MLE
int snpgpu_gnrIBD_MLE_Pairs(const double *allele_freq, const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int max_niter,
                            double reltol, int coeff_correct, int num_thread, int, double *k0, double *k1, double *loglik,
                            int32_t *niter, double *afreq)
{
    if (num_thread <= 0) { set_error("Invalid 'num.thread'."); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrIBD_MLE_Pairs", 2, buf)) return 1;
    return snpgpu_ibd_mle_pairs(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, allele_freq,
                                idx1, idx2, n_pairs, 0, 0, max_niter, reltol, coeff_correct, k0, k1, loglik, niter, afreq,
                                SNPGPU_HOST, g_ws.device);
}

// the listed pairs by method: 0 EM, 1 downhill simplex (coef = k0 then k1), 2 Jacquard (coef = D1 ... D8)
int snpgpu_gnrIBD_MLE_PairsMethod(const double *allele_freq, const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int method,
                                  int max_niter, double reltol, int coeff_correct, int num_thread, int, double *coef, double *loglik,
                                  int32_t *niter, double *afreq)
{
    if (method < 0 || method > 2) {
        set_error("snpgpu_gnrIBD_MLE_PairsMethod: invalid method " + std::to_string(method) +
                  " (0 = EM, 1 = downhill simplex, 2 = Jacquard)");
        return 1;
    }
    if (num_thread <= 0) { set_error("Invalid 'num.thread'."); return 1; }
    if (!coef) { set_error("snpgpu_gnrIBD_MLE_PairsMethod: coef is NULL"); return 1; }
    if (n_pairs < 1) { set_error("snpgpu_gnrIBD_MLE_PairsMethod: no pair is listed (n_pairs < 1)"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrIBD_MLE_PairsMethod", 2, buf)) return 1;
    const int64_t L = (int64_t)g_ws.sel.size();
    if (method == 2)
        return snpgpu_ibd_jacquard_pairs(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, allele_freq, idx1, idx2, n_pairs,
                                         max_niter, reltol, coef, loglik, niter, afreq, SNPGPU_HOST, g_ws.device);
    return snpgpu_ibd_mle_pairs(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, allele_freq, idx1, idx2, n_pairs,
                                method == 1 ? 2 : 0, 0, max_niter, reltol, coeff_correct, coef, coef + n_pairs, loglik, niter, afreq,
                                SNPGPU_HOST, g_ws.device);
}

// gnrIBD_LogLik(AFreq, k0, k1) and gnrIBD_LogLik_k01(AFreq, k0, k1), src/genIBD.cpp:1289-1330 and their .Call wrappers
int snpgpu_gnrIBD_LogLik(const double *afreq, const double *k0, const double *k1, double *out)
{
    if (!k0 || !k1) { set_error("snpgpu_gnrIBD_LogLik: k0 / k1 is NULL"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrIBD_LogLik", 2, buf)) return 1;
    return snpgpu_ibd_loglik(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, afreq, k0, k1,
                             0, 0, out, nullptr, SNPGPU_HOST, g_ws.device);
}

// gnrFst(Pop, nPop, Method), src/genFst.cpp:170-242, and the Fst case of gnrSlidingWindow, src/genSlideWin.cpp:101-327, on the
// selected SNPs.  What does not depend on the working space is checked first, so that it is refused without a device.
static int ws_fst(const char *fn, const int32_t *pop, int n_pop, const char *method, const int64_t *offsets, const int32_t *snp_index,
                  int64_t n_win, double *fst_win, double *beta_win, double *fst_snp)
{
    if (n_pop < 2) { set_error(std::string(fn) + ": There should be at least two populations!"); return 1; }
    if (!pop || !fst_win) { set_error(std::string(fn) + ": NULL argument"); return 1; }
    int code = 0;
    if (method && strcmp(method, "W&C84") == 0) code = SNPGPU_FST_WC84;
    else if (method && strcmp(method, "W&H02") == 0) code = SNPGPU_FST_WH02;
    else { set_error(std::string(fn) + ": 'method' should be one of \"W&C84\", \"W&H02\""); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows(fn, 0, buf)) return 1;
    const int64_t L = (int64_t)g_ws.sel.size();
    std::vector<int32_t> pop0((size_t)g_ws.n_samp);
    for (int64_t i = 0; i < g_ws.n_samp; i++) pop0[(size_t)i] = pop[i] - 1;     // R's factor codes start at 1
    if (!offsets)
        return snpgpu_fst(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, pop0.data(), n_pop, code, fst_win, fst_snp,
                          beta_win, g_ws.device);
    return snpgpu_fst_windows(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, pop0.data(), n_pop, code, offsets, snp_index,
                              n_win, fst_win, beta_win, fst_snp, g_ws.device);
}

int snpgpu_gnrFst(const int32_t *pop, int n_pop, const char *method, double *fst, double *fst_snp, double *beta)
{
    return ws_fst("snpgpu_gnrFst", pop, n_pop, method, nullptr, nullptr, 1, fst, beta, fst_snp);
}

int snpgpu_gnrSlidingWindowFst(const int32_t *pop, int n_pop, const char *method, const int64_t *offsets, const int32_t *snp_index,
                               int64_t n_win, double *fst_win, double *beta_win, double *fst_snp)
{
    if (!offsets) { set_error("snpgpu_gnrSlidingWindowFst: offsets is NULL"); return 1; }
    return ws_fst("snpgpu_gnrSlidingWindowFst", pop, n_pop, method, offsets, snp_index, n_win, fst_win, beta_win, fst_snp);
}

int snpgpu_gnrIBD_LogLik_k01(const double *afreq, double k0, double k1, double *out)
{
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrIBD_LogLik_k01", 2, buf)) return 1;
    return snpgpu_ibd_loglik(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, afreq,
                             nullptr, nullptr, k0, k1, out, nullptr, SNPGPU_HOST, g_ws.device);
}

// gnrSampFreq (src/SNPRelate.cpp:275-283), gnrHWE (src/genHWE.cpp:117-137) and gnrIndInb (src/genIBD.cpp:1847-2006) on the selected
// SNPs.  What does not depend on the working space is checked first, so that it is refused without a device.
int snpgpu_gnrSampFreq(double *out)
{
    if (!out) { set_error("snpgpu_gnrSampFreq: out is NULL"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrSampFreq", 0, buf)) return 1;
    const int64_t L = (int64_t)g_ws.sel.size();
    std::vector<int32_t> miss((size_t)g_ws.n_samp);
    if (snpgpu_geno_counts(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, nullptr, miss.data(), SNPGPU_HOST, g_ws.device))
        return 1;
    for (int64_t i = 0; i < g_ws.n_samp; i++) out[i] = (double)miss[(size_t)i] / (double)L;     // GetSampMissingRates: cnt /= fSNPNum
    return 0;
}

int snpgpu_gnrHWE(double *pvalue)
{
    if (!pvalue) { set_error("snpgpu_gnrHWE: pvalue is NULL"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrHWE", 0, buf)) return 1;
    return snpgpu_hwe(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, pvalue, g_ws.device);
}

int snpgpu_gnrIndInb(const double *afreq, const char *method, double reltol, int out_num_iter, int, double *coeff, int32_t *niter)
{
    static const char *const names[6] = {"mom.weir", "mom.visscher", "mle", "gcta1", "gcta2", "gcta3"};
    int code = 0;
    for (int k = 0; k < 6 && method; k++)
        if (strcmp(method, names[k]) == 0) code = k + 1;
    if (!code) {
        set_error("snpgpu_gnrIndInb: 'method' should be one of \"mom.weir\", \"mom.visscher\", \"mle\", \"gcta1\", \"gcta2\", \"gcta3\"");
        return 1;
    }
    if (!coeff) { set_error("snpgpu_gnrIndInb: coeff is NULL"); return 1; }
    if (code == SNPGPU_INB_MLE && !std::isfinite(reltol)) { set_error("snpgpu_gnrIndInb: `reltol' should a real number."); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows("snpgpu_gnrIndInb", 0, buf)) return 1;
    return snpgpu_ind_inb(buf.data(), (int64_t)g_ws.sel.size(), g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, afreq, code, reltol, coeff,
                          out_num_iter ? niter : nullptr, nullptr, SNPGPU_HOST, g_ws.device);
}

// gnrPairScore (src/genIBS.cpp:711-891) on the selected SNPs: the tables of snpgpu_pair_tables and the host finaliser, or the
// score matrix.  Method and type are checked first, so that an unknown one is refused without a device.
int snpgpu_gnrPairScore(const int32_t *idx1, const int32_t *idx2, int64_t n_pair, const char *method, const char *type, int dosage, int,
                        void *out)
{
    const char *fn = "snpgpu_gnrPairScore";
    static const char *const names[7] = {"IBS", "GVH", "HVG", "GVH.major", "GVH.minor", "GVH.major.only", "GVH.minor.only"};
    static const char *const types[4] = {"per.pair", "per.snp", "matrix", "gds.file"};
    int code = 0, kind = -1;
    for (int k = 0; k < 7 && method; k++)
        if (strcmp(method, names[k]) == 0) code = k + 1;
    if (!code) { set_error(std::string(fn) + ": Invalid 'method'."); return 1; }
    for (int k = 0; k < 4 && type; k++)
        if (strcmp(type, types[k]) == 0) kind = k;
    if (kind < 0) { set_error(std::string(fn) + ": Invalid 'type'."); return 1; }
    if (!out) { set_error(std::string(fn) + ": out is NULL"); return 1; }
    if (!idx1 || !idx2 || n_pair < 1) { set_error(std::string(fn) + ": no pair is given"); return 1; }
    std::vector<uint8_t> buf;
    if (ws_all_rows(fn, 0, buf)) return 1;
    const int64_t L = (int64_t)g_ws.sel.size();
    const int major = code >= SNPGPU_PS_GVH_MAJOR;
    if (kind == 0) {
        std::vector<int64_t> tab(9 * (size_t)n_pair);
        if (snpgpu_pair_tables(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, idx1, idx2, n_pair, major, tab.data(), nullptr,
                               nullptr, SNPGPU_HOST, g_ws.device))
            return 1;
        return snpgpu_pair_score_final(SNPGPU_PS_PAIR_TABLE, tab.data(), nullptr, n_pair, code, dosage, (double *)out);
    }
    if (kind == 1) {
        std::vector<int32_t> tab(16 * (size_t)L);
        std::vector<uint8_t> flip((size_t)L);
        if (snpgpu_pair_tables(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, idx1, idx2, n_pair, major, nullptr, tab.data(),
                               flip.data(), SNPGPU_HOST, g_ws.device))
            return 1;
        return snpgpu_pair_score_final(SNPGPU_PS_SNP_TABLE, tab.data(), flip.data(), L, code, dosage, (double *)out);
    }
    return snpgpu_pair_score_matrix(buf.data(), L, g_ws.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, idx1, idx2, n_pair, code, dosage,
                                    kind == 2 ? SNPGPU_PS_ELEM_INT32 : SNPGPU_PS_ELEM_BIT2, out, g_ws.device);
}

}  // extern "C"
