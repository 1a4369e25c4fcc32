// gpu_shim.cpp -- the `.Call` routines of SNPRelate's pairwise hot path bound to libsnpgpu (include/snpgpu.h).
//
// Added to the package's src/ directory next to the kept sources.  R headers and gdsfmt are not in this
// repository's build image, so this file is NOT compiled or run here; every libsnpgpu call below is exercised in
// exactly this order and with exactly these buffer shapes by tests/test_gpu_shim_order.py through ctypes.
//
// What stays (reference v1.46.0): R/*.R unchanged (same snpgds* signatures, same `.Call(gnrXxx, ...)` sites:
// R/IBS.R:36,68, R/IBD.R:383,399,594, R/PCA.R:70), `.InitFile2` and the working space (gnrSetGenoSpace /
// gnrSelSNP_Base, src/SNPRelate.cpp:76-210), the GDS block reader CGenoReadBySNP (src/dGenGWAS.cpp:1218-1397), the
// progress bar / interrupt polling, the `out.gds` row appends (GDS_Array_AppendData) and LAPACK-free results.
// What goes: the bodies of the eight routines below -- the CIBSCount / CKINGRobust / CKINGHomo / CGCTA_AlgArith /
// CExactPCA / CEigMix / CIndivBeta `Run` calls with their thread pools and SIMD loops -- and CalcEigen's dspevx call.
//
// Registration (src/SNPRelate.cpp:1154-1205): the eight entries of callMethods[] point at the functions below,
// names and arity unchanged -- see r_shim/registration.inc.  R_useDynamicSymbols(FALSE) stays.
//
//   routine replaced                                            reference body
//   gpu_gnrIBSNum(NumThread, Verbose)                           src/genIBS.cpp:500-550
//   gpu_gnrIBSAve(NumThread, useMatrix, Verbose)                src/genIBS.cpp:441-497
//   gpu_gnrIBD_KING_Robust(FamilyID, NumThread, useMatrix, V.)  src/genKING.cpp:576-679
//   gpu_gnrIBD_KING_Homo(NumThread, useMatrix, Verbose)         src/genKING.cpp:493-570
//   gpu_gnrGRM(NumThread, Method, GDS, useMatrix, Verbose)      src/genPCA.cpp:1614-1717 (+ grm_output :1586-1602,
//                                                                grm_save_to_gds :1571-1584)
//   gpu_gnrGRM_avg_val()                                        src/genPCA.cpp:1605-1611
//   gpu_gnrPCA(EigenCnt, Algorithm, NumThread, ParamList, V.)   src/genPCA.cpp:1355-1452 (+ CalcEigen :1262-1346)
//   gpu_gnrLDMat(method, NumSlide, MatTrim, NumThread, Verbose) src/genLD.cpp:957-1010
//   gpu_gnrIBD_MLE(AlleleFreq, KinshipConstraint, MaxIterCnt,    src/genIBD.cpp:1465-1548 (method 0 = EM; the Jacquard
//                  RelTol, CoeffCorrect, method, IfOutNum,       form, .Call(gnrIBD_MLE_Jacquard, ...), stays on the kept
//                  NumThread, Verbose)                           CPU routine)
//   gpu_gnrIBD_LogLik(AFreq, k0, k1)                            src/genIBD.cpp:1289-1310 and its .Call wrapper
//   gpu_gnrIBD_LogLik_k01(AFreq, k0, k1)                        src/genIBD.cpp:1312-1330 and its .Call wrapper
//   gpu_gnrLDpruning(StartIdx, pos_bp, slide_max_bp,             src/genLD.cpp:1014-1035 (+ Perform_LD_Pruning :807-924)
//                    slide_max_n, LD_threshold, method,
//                    NumThread, verbose)
//   gpu_gnrFst(Pop, nPop, Method)                               src/genFst.cpp:170-242
//   gpu_gnrSampFreq()                                           src/SNPRelate.cpp:275-283
//   gpu_gnrHWE()                                                src/genHWE.cpp:117-137
//   gpu_gnrIndInb(afreq, method, reltol, num_iter, verbose)     src/genIBD.cpp:1847-2006
//   gpu_gnrIndInbCoef(snp, afreq, reltol)                       src/genIBD.cpp:1814-1827
//   gpu_gnrDistPerm(n, dist, merge, n.perm, z.threshold)        src/SNPRelate.cpp:549-677
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dGenGWAS.h"   // kept: MCWorkingGeno, CdBaseWorkSpace, CGenoReadBySNP, CProgress, CachingSNPData, SEXP_Verbose
#include <snpgpu.h>

using namespace GWAS;

namespace {

[[noreturn]] void gpu_fail() { throw ErrCoreArray("%s", snpgpu_last_error()); }

// additive knobs, never a signature change: options(snpgpu.device=) / options(snpgpu.block.snps=), else the environment
int opt_int(const char *r_option, const char *env, int dflt)
{
    SEXP v = Rf_GetOption1(Rf_install(r_option));
    if (v != R_NilValue && Rf_length(v) == 1) {
        const int x = Rf_asInteger(v);
        if (x != NA_INTEGER) return x;
    }
    const char *e = getenv(env);
    return (e && *e) ? atoi(e) : dflt;
}

// One accumulator context; released in the destructor, i.e. before gdsfmt's catch block turns the C++ exception
// into Rf_error (no longjmp ever crosses live device state).
struct Accumulator {
    snpgpu_ctx *ctx = nullptr;
    C_UInt8 *blk[2] = {nullptr, nullptr};      // page-locked block buffers of the reader
    ~Accumulator()
    {
        if (ctx) snpgpu_destroy(ctx);           // waits for the stream, so the buffers are idle afterwards
        for (int k = 0; k < 2; k++)
            if (blk[k]) snpgpu_host_free(blk[k]);
    }

    // Streams the working space (set up by .InitFile2 -> gnrSetGenoSpace / gnrSelSNP_Base, exactly as before)
    // through a context of `kind`: the reader loop of every CXxx::Run without its body.
    void stream(int kind, bool bayesian, size_t block_snps, bool verbose)
    {
        CdBaseWorkSpace &space = MCWorkingGeno.Space();
        const size_t n_samp = space.SampleNum();
        snpgpu_opts o;
        memset(&o, 0, sizeof(o));
        o.device = opt_int("snpgpu.device", "SNPGPU_DEVICE", 0);
        o.bayesian = bayesian ? 1 : 0;
        o.max_block_snps = (int64_t)block_snps;
        if (snpgpu_create(kind, (int64_t)n_samp, &o, &ctx)) gpu_fail();
        for (int k = 0; k < 2; k++)
            if (snpgpu_host_alloc(n_samp * block_snps, (void **)&blk[k])) gpu_fail();
        // kept reader: uint8 [B][n_samp], sample fastest, values > 3 clamped to 3; its one prefetch thread stays
        CGenoReadBySNP reader(1, space, block_snps, verbose ? -1 : 0, false);
        reader.Init();
        for (int k = 0;; k ^= 1) {
            if (snpgpu_host_wait(ctx, blk[k])) gpu_fail();       // the copy of two blocks ago has left this buffer
            if (!reader.Read(blk[k])) break;
            // asynchronous: the H2D copy of this block overlaps the kernels of the previous one
            if (snpgpu_feed(ctx, blk[k], (int64_t)reader.Count(), SNPGPU_GENO_U8, SNPGPU_HOST_PINNED)) gpu_fail();
            reader.ProgressForward(reader.Count());              // progress + R_CheckUserInterrupt as before
        }
        if (snpgpu_sync(ctx)) gpu_fail();
    }
};

// options(snpgpu.devices = c(0, 1, ...)) / SNPGPU_DEVICES="0,1,...": more than one entry selects the multi-device object
// (snpgpu_multi: ONE R process drives all listed GPUs -- row panels of the output triangle, the block copied to the
// first device once and forwarded over xGMI, packed slabs gathered into the R vector)
std::vector<int32_t> opt_devices()
{
    std::vector<int32_t> d;
    SEXP v = Rf_GetOption1(Rf_install("snpgpu.devices"));
    if (v != R_NilValue && Rf_length(v) > 0) {
        SEXP iv = PROTECT(Rf_coerceVector(v, INTSXP));
        for (R_xlen_t i = 0; i < Rf_xlength(iv); i++) d.push_back(INTEGER(iv)[i]);
        UNPROTECT(1);
    } else if (const char *e = getenv("SNPGPU_DEVICES")) {
        for (const char *p = e; *p;) { d.push_back((int32_t)strtol(p, (char **)&p, 10)); while (*p == ',' || *p == ' ') p++; }
    }
    return d;
}

// The same reader loop over a multi-device object (`pass` of `n_passes`: KING-robust's 20 B of counters per pair may need
// several walks over the SNPs, each with its own resident panels -- snpgpu_multi_opts).
struct MultiAccumulator {
    snpgpu_multi *m = nullptr;
    C_UInt8 *blk[2] = {nullptr, nullptr};
    ~MultiAccumulator()
    {
        if (m) snpgpu_multi_destroy(m);
        for (int k = 0; k < 2; k++)
            if (blk[k]) snpgpu_host_free(blk[k]);
    }
    // panels_per_device: 0 = options(snpgpu.panels.per.device=) / SNPGPU_PANELS_PER_DEVICE, default -1 (the library picks the fewest
    // that fit the devices' free memory).  A job of several passes must cut the triangle the SAME way in every pass -- the plan is
    // plan_rows(n, devices x panels_per_device x passes) --, and the automatic choice reads hipMemGetInfo, which may differ from
    // one pass to the next: pass 0 resolves it, chosen_ppd() hands the value to the later passes.
    int chosen_ppd() const
    {
        snpgpu_multi_status st;
        if (!m || snpgpu_multi_get_status(m, &st)) gpu_fail();
        return (int)st.panels_per_device;
    }
    void stream(int kind, bool bayesian, size_t block_snps, bool verbose, const std::vector<int32_t> &devices, int n_passes = 1, int pass = 0,
                int panels_per_device = 0)
    {
        CdBaseWorkSpace &space = MCWorkingGeno.Space();
        const size_t n_samp = space.SampleNum();
        snpgpu_opts o;
        memset(&o, 0, sizeof(o));
        o.bayesian = bayesian ? 1 : 0;
        o.max_block_snps = (int64_t)block_snps;
        snpgpu_multi_opts mo;
        memset(&mo, 0, sizeof(mo));
        mo.devices = &devices[0];
        mo.n_devices = (int32_t)devices.size();
        mo.panels_per_device = panels_per_device != 0 ? panels_per_device
                                                      : opt_int("snpgpu.panels.per.device", "SNPGPU_PANELS_PER_DEVICE", -1);   // -1: the fewest that fit (library)
        mo.n_passes = n_passes;
        mo.pass = pass;
        if (snpgpu_multi_create(kind, (int64_t)n_samp, &o, &mo, &m)) gpu_fail();
        for (int k = 0; k < 2; k++)
            if (!blk[k] && snpgpu_host_alloc(n_samp * block_snps, (void **)&blk[k])) gpu_fail();
        CGenoReadBySNP reader(1, space, block_snps, verbose ? -1 : 0, false);
        reader.Init();
        for (int k = 0;; k ^= 1) {
            if (snpgpu_multi_host_wait(m, blk[k])) gpu_fail();
            if (!reader.Read(blk[k])) break;
            if (snpgpu_multi_feed(m, blk[k], (int64_t)reader.Count(), SNPGPU_GENO_U8, SNPGPU_HOST_PINNED)) gpu_fail();
            reader.ProgressForward(reader.Count());
        }
        if (snpgpu_multi_sync(m)) gpu_fail();
    }
};

// packed upper triangle (row-major with diagonal) -> full symmetric column-major matrix, in place at the end of `full`
void tri_to_full(const std::vector<double> &tri, size_t n, double *full)
{
    for (size_t i = 0, k = 0; i < n; i++)
        for (size_t j = i; j < n; j++, k++) full[i * n + j] = full[j * n + i] = tri[k];
}

size_t counter_block() { return (size_t)opt_int("snpgpu.block.snps", "SNPGPU_BLOCK_SNPS", 65536); }   // IBS / KING / beta
size_t syrk_block() { return (size_t)opt_int("snpgpu.block.snps", "SNPGPU_BLOCK_SNPS", 32768); }      // GRM / PCA / EIGMIX (bench.py feeds 65536-SNP blocks of 2-bit rows; the byte genotypes of the kept reader make that 6.5 GB per buffer at N = 100 000, hence half of it here)

// n x n REALSXP matrix or the packed upper triangle as a plain numeric vector (useMatrix = TRUE: R wraps it with
// Matrix::dspMatrix(uplo = "L"), R/Internal.R:46-51 -- column-major lower == row-major upper, the CdMatTri order)
SEXP alloc_result(size_t n, bool packed)
{
    return packed ? Rf_allocVector(REALSXP, (R_xlen_t)(n * (n + 1) / 2)) : Rf_allocMatrix(REALSXP, (int)n, (int)n);
}

// snpgdsGRM(out.fn=): the finished matrix goes row by row into the "grm" node the R wrapper created
// (valdim = c(n, 0), R/IBD.R:586-589).  `tri` is the packed upper triangle; row i of the symmetric matrix is
// {tri(0,i) .. tri(i-1,i), tri(i,i) .. tri(i,n-1)}.
void append_rows(const std::vector<double> &tri, size_t n, PdGDSObj node, bool verbose)
{
    if (verbose) Rprintf("Saving to the GDS file:\n");
    std::vector<double> row(n);
    CProgress progress(verbose ? (C_Int64)n : -1);
    for (size_t i = 0; i < n; i++) {
        for (size_t k = 0; k < i; k++) row[k] = tri[i + k * (2 * n - k - 1) / 2];       // idx(k, i), k < i
        const double *p = &tri[i + i * (2 * n - i - 1) / 2];                            // idx(i, i)
        for (size_t j = i; j < n; j++) row[j] = p[j - i];
        GDS_Array_AppendData(node, (int)n, &row[0], svFloat64);
        progress.Forward(1);
    }
}

double grm_avg_val = 0;     // value of the last IndivBeta run (the reference keeps the same global, genPCA.cpp:1605)

}  // namespace

extern "C" {

// --------------------------------------------------------------------------------------------------------------
COREARRAY_DLL_EXPORT SEXP gpu_gnrIBSNum(SEXP NumThread, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("IBS", verbose);
        const size_t n = MCWorkingGeno.Space().SampleNum();
        Accumulator acc;
        acc.stream(SNPGPU_IBS, false, counter_block(), verbose);
        PROTECT(rv_ans = Rf_allocVector(VECSXP, 3));
        for (int k = 0; k < 3; k++) SET_VECTOR_ELT(rv_ans, k, Rf_allocMatrix(INTSXP, (int)n, (int)n));
        // three full symmetric int32 matrices, written straight into R's memory
        if (snpgpu_ibs_num(acc.ctx, INTEGER(VECTOR_ELT(rv_ans, 0)), INTEGER(VECTOR_ELT(rv_ans, 1)),
                           INTEGER(VECTOR_ELT(rv_ans, 2)), 0, SNPGPU_HOST))
            gpu_fail();
        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
        UNPROTECT(1);
    COREARRAY_CATCH
}

COREARRAY_DLL_EXPORT SEXP gpu_gnrIBSAve(SEXP NumThread, SEXP useMatrix, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("IBS", verbose);
        const size_t n = MCWorkingGeno.Space().SampleNum();
        const bool packed = (Rf_asLogical(useMatrix) == TRUE);
        Accumulator acc;
        acc.stream(SNPGPU_IBS, false, counter_block(), verbose);
        PROTECT(rv_ans = alloc_result(n, packed));
        if (snpgpu_ibs_ave(acc.ctx, REAL(rv_ans), packed ? 1 : 0, SNPGPU_HOST)) gpu_fail();
        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
        UNPROTECT(1);
    COREARRAY_CATCH
}

COREARRAY_DLL_EXPORT SEXP gpu_gnrIBD_KING_Robust(SEXP FamilyID, SEXP NumThread, SEXP useMatrix, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("KING IBD", verbose);
        // SumSq <= 4 L must fit uint32 (src/genKING.cpp:598-602); snpgpu_feed enforces the same bound per stream,
        // checked here first so that no device memory is touched for an invalid request
        if (MCWorkingGeno.Space().SNPNum() >= 1073741824)
            throw ErrCoreArray("The number of SNPs should be less than 1,073,741,824.");
        const size_t n = MCWorkingGeno.Space().SampleNum();
        const bool packed = (Rf_asLogical(useMatrix) == TRUE);
        const std::vector<int32_t> devices = opt_devices();
        if (devices.size() > 1) {
            // several GPUs, and as many passes over the SNP stream as options(snpgpu.passes=) asks for: every pass gathers
            // the packed slabs of its own panels into the same two vectors
            const int n_passes = opt_int("snpgpu.passes", "SNPGPU_PASSES", 1);
            std::vector<double> t0, t1;
            PROTECT(rv_ans = Rf_allocVector(VECSXP, 2));
            SET_VECTOR_ELT(rv_ans, 0, alloc_result(n, packed));
            SET_VECTOR_ELT(rv_ans, 1, alloc_result(n, packed));
            double *o0 = REAL(VECTOR_ELT(rv_ans, 0)), *o1 = REAL(VECTOR_ELT(rv_ans, 1));
            if (!packed) { t0.resize(n * (n + 1) / 2); t1.resize(n * (n + 1) / 2); }
            int ppd = 0;                                   // resolved by pass 0, the same for every later pass
            for (int q = 0; q < n_passes; q++) {
                MultiAccumulator acc;
                acc.stream(SNPGPU_KING_ROBUST, false, counter_block(), verbose, devices, n_passes, q, ppd);
                if (q == 0) ppd = acc.chosen_ppd();
                if (snpgpu_multi_king_robust(acc.m, INTEGER(FamilyID), packed ? o0 : &t0[0], packed ? o1 : &t1[0], SNPGPU_HOST)) gpu_fail();
            }
            if (!packed) { tri_to_full(t0, n, o0); tri_to_full(t1, n, o1); }
            if (verbose) Rprintf("%s    Done.\n", TimeToStr());
            UNPROTECT(1);
            return rv_ans;
        }
        Accumulator acc;
        acc.stream(SNPGPU_KING_ROBUST, false, counter_block(), verbose);
        PROTECT(rv_ans = Rf_allocVector(VECSXP, 2));
        SET_VECTOR_ELT(rv_ans, 0, alloc_result(n, packed));      // IBS0
        SET_VECTOR_ELT(rv_ans, 1, alloc_result(n, packed));      // kinship
        // FamilyID: as.integer(as.factor(family.id)) from R/IBD.R:360-364 -- levels 1..k, NA_INTEGER (= INT_MIN,
        // negative) for "no family", which is the ABI's convention for NA
        if (snpgpu_king_robust(acc.ctx, INTEGER(FamilyID), REAL(VECTOR_ELT(rv_ans, 0)), REAL(VECTOR_ELT(rv_ans, 1)),
                               packed ? 1 : 0, SNPGPU_HOST))
            gpu_fail();
        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
        UNPROTECT(1);
    COREARRAY_CATCH
}

COREARRAY_DLL_EXPORT SEXP gpu_gnrIBD_KING_Homo(SEXP NumThread, SEXP useMatrix, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("KING IBD", verbose);
        const size_t n = MCWorkingGeno.Space().SampleNum();
        const bool packed = (Rf_asLogical(useMatrix) == TRUE);
        Accumulator acc;
        acc.stream(SNPGPU_KING_HOMO, false, syrk_block(), verbose);   // integer half + the two masked fp sums
        PROTECT(rv_ans = Rf_allocVector(VECSXP, 2));
        SET_VECTOR_ELT(rv_ans, 0, alloc_result(n, packed));      // k0
        SET_VECTOR_ELT(rv_ans, 1, alloc_result(n, packed));      // k1
        if (snpgpu_king_homo(acc.ctx, REAL(VECTOR_ELT(rv_ans, 0)), REAL(VECTOR_ELT(rv_ans, 1)), packed ? 1 : 0, SNPGPU_HOST))
            gpu_fail();
        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
        UNPROTECT(1);
    COREARRAY_CATCH
}

// gnrDiss, src/genIBS.cpp:652-683: always the full n x n matrix
COREARRAY_DLL_EXPORT SEXP gpu_gnrDiss(SEXP NumThread, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("Dissimilarity", verbose);
        const size_t n = MCWorkingGeno.Space().SampleNum();
        Accumulator acc;
        acc.stream(SNPGPU_DISS, false, syrk_block(), verbose);        // SumGeno counters + the masked weight sum
        PROTECT(rv_ans = Rf_allocMatrix(REALSXP, (int)n, (int)n));
        if (snpgpu_diss(acc.ctx, REAL(rv_ans), 0, SNPGPU_HOST)) gpu_fail();
        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
        UNPROTECT(1);
    COREARRAY_CATCH
}

// --------------------------------------------------------------------------------------------------------------
COREARRAY_DLL_EXPORT SEXP gpu_gnrGRM_avg_val() { return Rf_ScalarReal(grm_avg_val); }

COREARRAY_DLL_EXPORT SEXP gpu_gnrGRM(SEXP NumThread, SEXP Method, SEXP GDS, SEXP useMatrix, SEXP Verbose)
{
    const char *method = CHAR(STRING_ELT(Method, 0));
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        PdGDSObj node = NULL;                                  // snpgdsGRM(out.fn=): the "grm" node of the output file
        if (!Rf_isNull(GDS)) node = GDS_Node_Path(GDS_R_SEXP2FileRoot(GDS), "grm", TRUE);
        CachingSNPData("GRM Calculation", verbose);
        const size_t n = MCWorkingGeno.Space().SampleNum();

        int kind;
        if (strcmp(method, "GCTA") == 0 || strcmp(method, "Corr") == 0) kind = SNPGPU_GRM_GCTA;
        else if (strcmp(method, "Eigenstrat") == 0) kind = SNPGPU_PCA_COV;
        else if (strcmp(method, "EIGMIX") == 0) kind = SNPGPU_EIGMIX;       // "Weighted" arrives as "EIGMIX" (R/IBD.R:551-555)
        else if (strcmp(method, "IndivBeta") == 0) kind = SNPGPU_INDIV_BETA;
        else throw ErrCoreArray("Invalid 'method'!");

        const std::vector<int32_t> devices = opt_devices();
        if (devices.size() > 1 && (kind == SNPGPU_GRM_GCTA || kind == SNPGPU_PCA_COV) && strcmp(method, "Corr") != 0) {
            MultiAccumulator acc;
            acc.stream(kind, false, syrk_block(), verbose, devices);
            const bool packed = node ? true : (Rf_asLogical(useMatrix) == TRUE);
            std::vector<double> tri;
            if (node || !packed) tri.resize(n * (n + 1) / 2);
            if (!node) PROTECT(rv_ans = alloc_result(n, packed));
            double *out = (node || !packed) ? &tri[0] : REAL(rv_ans);
            if (kind == SNPGPU_GRM_GCTA ? snpgpu_multi_grm_gcta(acc.m, out, SNPGPU_HOST)
                                        : snpgpu_multi_pca_cov(acc.m, out, 1, NULL, SNPGPU_HOST))
                gpu_fail();
            if (node) append_rows(tri, n, node, verbose);
            else if (!packed) tri_to_full(tri, n, REAL(rv_ans));
            if (verbose) Rprintf("%s    Done.\n", TimeToStr());
            if (!node) UNPROTECT(1);
            return rv_ans;
        }
        Accumulator acc;
        acc.stream(kind, false, kind == SNPGPU_INDIV_BETA ? counter_block() : syrk_block(), verbose);

        // "Corr" is always a full matrix (src/genPCA.cpp:1658-1685); a GDS target takes the packed triangle
        const bool corr = (strcmp(method, "Corr") == 0);
        const bool packed = node ? true : (!corr && Rf_asLogical(useMatrix) == TRUE);
        std::vector<double> tri;
        double *out;
        if (node) {
            tri.resize(n * (n + 1) / 2);
            out = &tri[0];
        } else {
            PROTECT(rv_ans = alloc_result(n, packed));
            out = REAL(rv_ans);
        }
        int rc;
        switch (kind) {
        case SNPGPU_GRM_GCTA: rc = snpgpu_grm_gcta(acc.ctx, out, packed ? 1 : 0, SNPGPU_HOST); break;
        case SNPGPU_PCA_COV:   // Eigenstrat: covariance times (n - 1) / trace
            rc = snpgpu_pca_cov(acc.ctx, out, packed ? 1 : 0, 1, 0.0, NULL, SNPGPU_HOST); break;
        case SNPGPU_EIGMIX:    // CalcEigMixGRM: no diagonal adjustment, times 2 (src/genEIGMIX.cpp:645-653)
            rc = snpgpu_eigmix(acc.ctx, 0, 2.0, out, packed ? 1 : 0, SNPGPU_HOST); break;
        default:               // CalcIndivBetaGRM: min-based transform, keeps the average for gnrGRM_avg_val
            rc = snpgpu_indiv_beta(acc.ctx, 2, out, &grm_avg_val, packed ? 1 : 0, SNPGPU_HOST); break;
        }
        if (rc) gpu_fail();

        if (corr) {            // scaled GRM: unit diagonal, g_ij / sqrt(g_ii g_jj)
            std::vector<double> sd(n);
            for (size_t i = 0; i < n; i++) sd[i] = sqrt(out[i * n + i]);
            for (size_t i = 0; i < n; i++) {
                out[i * n + i] = 1;
                for (size_t j = i + 1; j < n; j++) out[i * n + j] = out[j * n + i] = out[j * n + i] / (sd[i] * sd[j]);
            }
        }
        if (node) append_rows(tri, n, node, verbose);
        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
        if (!node) UNPROTECT(1);
    COREARRAY_CATCH
}

// --------------------------------------------------------------------------------------------------------------
COREARRAY_DLL_EXPORT SEXP gpu_gnrPCA(SEXP EigenCnt, SEXP Algorithm, SEXP NumThread, SEXP ParamList, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("PCA", verbose);
        const char *alg = CHAR(STRING_ELT(Algorithm, 0));
        const size_t n = MCWorkingGeno.Space().SampleNum();

        if (strcmp(alg, "exact") == 0) {
            const bool bayesian = (Rf_asLogical(RGetListElement(ParamList, "bayesian")) == TRUE);
            const bool need_genmat = (Rf_asLogical(RGetListElement(ParamList, "need.genmat")) == TRUE);
            const bool genmat_only = (Rf_asLogical(RGetListElement(ParamList, "genmat.only")) == TRUE);
            const std::vector<int32_t> devices = opt_devices();
            // eigen.method is validated on every route ("DSPEV" = all eigenvalues, src/genPCA.cpp:1262-1346): a request for the
            // whole spectrum is a dense problem -- it takes the single-device route below, which returns all n eigenvalues as the
            // reference does, also when several devices are configured
            const char *em_all = CHAR(STRING_ELT(RGetListElement(ParamList, "eigen.method"), 0));
            if (strcmp(em_all, "DSPEV") != 0 && strcmp(em_all, "DSPEVX") != 0) throw ErrCoreArray("Unknown 'eigen.method'.");
            if (devices.size() > 1 && (genmat_only || strcmp(em_all, "DSPEV") != 0)) {
                // configs[3]: the covariance stays distributed over the GPUs as row panels; only the trace, (on request) the
                // matrix, and the top eigenpairs -- block Krylov over all devices, snpgpu_multi_topk_eigen -- come back
                MultiAccumulator acc;
                acc.stream(SNPGPU_PCA_COV, bayesian, syrk_block(), verbose, devices);
                PROTECT(rv_ans = Rf_allocVector(VECSXP, 5));
                double trace_xtx = 0;
                if (need_genmat) {
                    std::vector<double> tri(n * (n + 1) / 2);
                    if (snpgpu_multi_pca_cov(acc.m, &tri[0], 1, &trace_xtx, SNPGPU_HOST)) gpu_fail();
                    SET_VECTOR_ELT(rv_ans, 1, Rf_allocMatrix(REALSXP, (int)n, (int)n));
                    tri_to_full(tri, n, REAL(VECTOR_ELT(rv_ans, 1)));
                } else if (snpgpu_multi_pca_cov(acc.m, NULL, 1, &trace_xtx, SNPGPU_HOST)) gpu_fail();
                SET_VECTOR_ELT(rv_ans, 0, Rf_ScalarReal(trace_xtx));
                SET_VECTOR_ELT(rv_ans, 4, Rf_ScalarReal((double)(n - 1)));
                if (!genmat_only) {
                    int n_eig = Rf_asInteger(EigenCnt);
                    if (n_eig < 0) throw ErrCoreArray("Invalid 'eigen.cnt'.");
                    if ((size_t)n_eig > n) n_eig = (int)n;
                    if (n_eig > 0) {
                        SET_VECTOR_ELT(rv_ans, 2, Rf_allocVector(REALSXP, (R_xlen_t)n));
                        SET_VECTOR_ELT(rv_ans, 3, Rf_allocMatrix(REALSXP, (int)n, n_eig));
                        double *val = REAL(VECTOR_ELT(rv_ans, 2));
                        // scale <= 0: (n - 1) / trace over all panels, src/genPCA.cpp:1386-1390
                        if (snpgpu_multi_topk_eigen(acc.m, 0.0, n_eig, NULL, val, REAL(VECTOR_ELT(rv_ans, 3)), SNPGPU_HOST, NULL)) gpu_fail();
                        for (size_t i = (size_t)n_eig; i < n; i++) val[i] = R_NaN;
                    }
                }
                if (verbose) Rprintf("%s    Done.\n", TimeToStr());
                UNPROTECT(1);
                return rv_ans;
            }
            Accumulator acc;
            acc.stream(SNPGPU_PCA_COV, bayesian, syrk_block(), verbose);

            PROTECT(rv_ans = Rf_allocVector(VECSXP, 5));         // TraceXTX, genmat, eigenval, eigenvect, TraceVal
            double trace_xtx = 0;
            double *genmat = NULL;
            if (need_genmat) {
                SET_VECTOR_ELT(rv_ans, 1, Rf_allocMatrix(REALSXP, (int)n, (int)n));
                genmat = REAL(VECTOR_ELT(rv_ans, 1));
            }
            // covariance times (n - 1) / trace; genmat == NULL only returns the trace
            if (snpgpu_pca_cov(acc.ctx, genmat, 0, 1, 0.0, &trace_xtx, SNPGPU_HOST)) gpu_fail();
            SET_VECTOR_ELT(rv_ans, 0, Rf_ScalarReal(trace_xtx));
            // trace after the scaling: n - 1 up to rounding; taken from the matrix when it is there, as the reference does
            double trace_val = (double)(n - 1);
            if (genmat) { trace_val = 0; for (size_t i = 0; i < n; i++) trace_val += genmat[i * n + i]; }
            SET_VECTOR_ELT(rv_ans, 4, Rf_ScalarReal(trace_val));

            if (!genmat_only) {
                if (verbose) Rprintf("%s    Begin (eigenvalues and eigenvectors)\n", TimeToStr());
                int n_eig = Rf_asInteger(EigenCnt);
                if (n_eig < 0) throw ErrCoreArray("Invalid 'eigen.cnt'.");
                if ((size_t)n_eig > n) n_eig = (int)n;
                if (n_eig > 0) {
                    const char *em = CHAR(STRING_ELT(RGetListElement(ParamList, "eigen.method"), 0));
                    const bool all = (strcmp(em, "DSPEV") == 0);               // all eigenvalues, first n_eig vectors
                    if (!all && strcmp(em, "DSPEVX") != 0) throw ErrCoreArray("Unknown 'eigen.method'.");
                    const int k = all ? (int)n : n_eig;
                    SET_VECTOR_ELT(rv_ans, 2, Rf_allocVector(REALSXP, (R_xlen_t)n));
                    SET_VECTOR_ELT(rv_ans, 3, Rf_allocMatrix(REALSXP, (int)n, n_eig));
                    double *val = REAL(VECTOR_ELT(rv_ans, 2));
                    std::vector<double> vec_all;
                    double *vec = REAL(VECTOR_ELT(rv_ans, 3));
                    if (all) { vec_all.resize(n * n); vec = &vec_all[0]; }
                    // top-k eigenpairs of the normalised covariance on the device (descending, as -dspevx(-C) gives
                    // them): hipSOLVER's dense solver up to SNPGPU_EIG_DENSE_MAX samples, the block-Krylov solver of
                    // csrc/eigen.hip on the resident panel beyond (any n); a failure carries LAPACK's wording, "... infinite or missing values in the genetic
                    // covariance matrix!"
                    if (snpgpu_pca_eigen(acc.ctx, k, val, vec, SNPGPU_HOST)) gpu_fail();
                    for (size_t i = (size_t)k; i < n; i++) val[i] = R_NaN;      // CalcEigen :1343-1345
                    if (all) memcpy(REAL(VECTOR_ELT(rv_ans, 3)), vec, sizeof(double) * n * (size_t)n_eig);
                }
            }
            UNPROTECT(1);

        } else if (strcmp(alg, "randomized") == 0) {
            // CRandomPCA::Run makes iter.num + 2 passes over the SNPs; here the selected genotypes are read ONCE
            // through the kept reader, kept as 2-bit rows in host memory (N L / 4 bytes) and handed to the
            // workspace-level routine, which runs every pass on the device.
            const int aux_dim = Rf_asInteger(RGetListElement(ParamList, "aux.dim"));
            const int iter_num = Rf_asInteger(RGetListElement(ParamList, "iter.num"));
            const double *aux_mat = REAL(RGetListElement(ParamList, "aux.mat"));    // rnorm(aux.dim * n.samp)
            const int n_eig = Rf_asInteger(EigenCnt);
            CdBaseWorkSpace &space = MCWorkingGeno.Space();
            const size_t n_snp = space.SNPNum(), rb = (n + 3) / 4, blk = 4096;
            std::vector<C_UInt8> packed(n_snp * rb), buf(n * blk);
            {
                CGenoReadBySNP reader(1, space, blk, verbose ? -1 : 0, false);
                reader.Init();
                size_t at = 0;
                while (reader.Read(&buf[0])) {
                    for (size_t s = 0; s < reader.Count(); s++, at++) {
                        const C_UInt8 *g = &buf[s * n];
                        C_UInt8 *q = &packed[at * rb];
                        for (size_t i = 0; i < n; i++) {
                            if ((i & 3) == 0) q[i >> 2] = 0;
                            q[i >> 2] |= (C_UInt8)((g[i] > 3 ? 3 : g[i]) << (2 * (i & 3)));
                        }
                        if (n & 3) q[rb - 1] |= (C_UInt8)(0xFF << (2 * (n & 3)));      // padding = missing
                    }
                    reader.ProgressForward(reader.Count());
                }
            }
            const int device = opt_int("snpgpu.device", "SNPGPU_DEVICE", 0);
            struct WsGuard { ~WsGuard() { snpgpu_ws_clear(); } } guard;
            if (snpgpu_ws_set_geno(&packed[0], (int64_t)n_snp, (int64_t)n, SNPGPU_GENO_PACKED2, device)) gpu_fail();
            const int hsize = aux_dim * (iter_num + 1);
            std::vector<double> vecs(n * (size_t)n_eig);
            double trace2 = 0;
            PROTECT(rv_ans = Rf_allocVector(VECSXP, 3));         // sigma [n], V^T [hsize x n], 2 * TraceXTX
            SET_VECTOR_ELT(rv_ans, 0, Rf_allocVector(REALSXP, (R_xlen_t)n));
            SET_VECTOR_ELT(rv_ans, 1, Rf_allocMatrix(REALSXP, hsize, (int)n));
            if (snpgpu_gnrPCA_randomized(n_eig, aux_dim, iter_num, aux_mat, 1, verbose ? 1 : 0,
                                         REAL(VECTOR_ELT(rv_ans, 0)), &vecs[0], &trace2))
                gpu_fail();
            // R/PCA.R:84 uses the first eigen.cnt ROWS of V^T: element (r, s) of an hsize x n column-major matrix
            double *vt = REAL(VECTOR_ELT(rv_ans, 1));
            memset(vt, 0, sizeof(double) * (size_t)hsize * n);
            for (int r = 0; r < n_eig; r++)
                for (size_t s = 0; s < n; s++) vt[(size_t)r + (size_t)hsize * s] = vecs[s + n * (size_t)r];
            SET_VECTOR_ELT(rv_ans, 2, Rf_ScalarReal(trace2));
            UNPROTECT(1);
        } else
            throw "Invalid 'algorithm'.";

        if (verbose) Rprintf("%s    Done.\n", TimeToStr());
    COREARRAY_CATCH
}

// --------------------------------------------------------------------------------------------------------------
// LD between SNP pairs: the kept reader streams the working space into an LD object (snpgpu_ld_*), which finalises the
// sliding-window columns block by block (or the full matrix by row panels at the end) straight into R's matrix.
COREARRAY_DLL_EXPORT SEXP gpu_gnrLDMat(SEXP method, SEXP NumSlide, SEXP MatTrim, SEXP NumThread, SEXP Verbose)
{
    const int n_slide = Rf_asInteger(NumSlide);
    const int trim_flag = Rf_asLogical(MatTrim);
    if (trim_flag == NA_INTEGER) Rf_error("'mat.trim' should be TRUE or FALSE");
    if (Rf_asInteger(NumThread) <= 0) Rf_error("Invalid 'num.thread'.");
    const bool verbose = SEXP_Verbose(Verbose);
    COREARRAY_TRY
        CachingSNPData("LD matrix", verbose);
        CdBaseWorkSpace &space = MCWorkingGeno.Space();
        const size_t n_samp = space.SampleNum();
        struct LD {
            snpgpu_ld *ld = nullptr;
            ~LD() { if (ld) snpgpu_ld_destroy(ld); }
        } obj;
        snpgpu_opts o;
        memset(&o, 0, sizeof(o));
        o.device = opt_int("snpgpu.device", "SNPGPU_DEVICE", 0);
        if (snpgpu_ld_create((int64_t)n_samp, (int64_t)space.SNPNum(), Rf_asInteger(method), n_slide, trim_flag ? 1 : 0, &o, &obj.ld))
            gpu_fail();
        int64_t rows = 0, cols = 0;
        if (snpgpu_ld_out_dims(obj.ld, &rows, &cols)) gpu_fail();
        const size_t block_snps = syrk_block();
        std::vector<C_UInt8> buf(n_samp * block_snps);
        CGenoReadBySNP reader(1, space, block_snps, verbose ? -1 : 0, false);
        reader.Init();
        while (reader.Read(&buf[0])) {
            if (snpgpu_ld_feed(obj.ld, &buf[0], (int64_t)reader.Count(), SNPGPU_GENO_U8, SNPGPU_HOST)) gpu_fail();
            reader.ProgressForward(reader.Count());
        }
        PROTECT(rv_ans = Rf_allocMatrix(REALSXP, (int)rows, (int)cols));
        if (snpgpu_ld_result(obj.ld, REAL(rv_ans), SNPGPU_HOST)) gpu_fail();
        UNPROTECT(1);
    COREARRAY_CATCH
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------------------
// IBD by maximum likelihood: the kept reader packs the working space into 2-bit rows in host memory, which one
// snpgpu_ibd_mle / snpgpu_ibd_loglik call takes to the device (the EM needs every SNP of a pair in every iteration).
namespace {

struct PackedSpace {
    std::vector<C_UInt8> rows;
    size_t n_samp = 0, n_snp = 0;
    void read(const char *msg, bool verbose, size_t min_samp = 2)
    {
        CachingSNPData(msg, verbose);
        CdBaseWorkSpace &space = MCWorkingGeno.Space();
        n_samp = space.SampleNum();
        n_snp = space.SNPNum();
        if (n_samp < min_samp) throw ErrCoreArray("%s", min_samp > 1 ? "at least two samples are needed" : "no sample in the working dataset");
        if (n_snp < 1) throw ErrCoreArray("%s", "no SNP in the working dataset");
        const size_t rb = (n_samp + 3) / 4, block = syrk_block();
        rows.assign(n_snp * rb, 0xFF);
        std::vector<C_UInt8> buf(n_samp * block);
        CGenoReadBySNP reader(1, space, block, verbose ? -1 : 0, false);
        reader.Init();
        size_t l0 = 0;
        while (reader.Read(&buf[0])) {
            const size_t cnt = reader.Count();
            for (size_t l = 0; l < cnt; l++) {
                C_UInt8 *r = &rows[(l0 + l) * rb];
                for (size_t s = 0; s < n_samp; s++) {
                    const unsigned g = buf[l * n_samp + s] > 2 ? 3u : buf[l * n_samp + s];
                    r[s >> 2] = (C_UInt8)((r[s >> 2] & ~(3u << (2 * (s & 3)))) | (g << (2 * (s & 3))));
                }
            }
            l0 += cnt;
            reader.ProgressForward(cnt);
        }
    }
};

double as_real(SEXP x) { return REAL(Rf_coerceVector(x, REALSXP))[0]; }

constexpr unsigned int R_LGLSXP = 10;   // LGLSXP of <Rinternals.h>: gnrLDpruning returns a logical vector (R/LD.R does L[flag] <- rv)

}  // namespace

extern "C" {

COREARRAY_DLL_EXPORT SEXP gpu_gnrIBD_MLE(SEXP AlleleFreq, SEXP KinshipConstraint, SEXP MaxIterCnt, SEXP RelTol,
                                         SEXP CoeffCorrect, SEXP method, SEXP IfOutNum, SEXP NumThread, SEXP Verbose)
{
    const bool verbose = SEXP_Verbose(Verbose);
    const int mle_method = Rf_asInteger(method);
    const bool out_num = Rf_asLogical(IfOutNum) == TRUE;
    (void)KinshipConstraint;          // accepted, no effect: Est_PLINK_Kinship is called without the constraint (:823)
    if (Rf_asInteger(NumThread) <= 0) Rf_error("Invalid 'num.thread'.");
    COREARRAY_TRY
        PackedSpace ps;
        ps.read("MLE IBD", verbose);
        const int n = (int)ps.n_samp;
        if (mle_method != 0) {
            snpgpu_gnrIBD_MLE(nullptr, 0, 0, 0, 0, mle_method, 0, 1, 0, nullptr, nullptr, nullptr, nullptr);   // sets the message
            gpu_fail();
        }
        const int max_niter = Rf_asInteger(MaxIterCnt);
        const double reltol = as_real(RelTol);
        const int coeff_correct = Rf_asLogical(CoeffCorrect) == TRUE ? 1 : 0;
        // every allocation goes into the protected list at once: the next one may collect anything unprotected
        PROTECT(rv_ans = Rf_allocVector(VECSXP, 4));
        SET_VECTOR_ELT(rv_ans, 0, Rf_allocMatrix(REALSXP, n, n));
        SET_VECTOR_ELT(rv_ans, 1, Rf_allocMatrix(REALSXP, n, n));
        SET_VECTOR_ELT(rv_ans, 2, Rf_allocVector(REALSXP, (R_xlen_t)ps.n_snp));
        if (out_num) SET_VECTOR_ELT(rv_ans, 3, Rf_allocMatrix(INTSXP, n, n));
        SEXP k0 = VECTOR_ELT(rv_ans, 0), k1 = VECTOR_ELT(rv_ans, 1), afreq = VECTOR_ELT(rv_ans, 2);
        if (snpgpu_ibd_mle(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST,
                           Rf_isNull(AlleleFreq) ? nullptr : REAL(AlleleFreq), max_niter, reltol, coeff_correct, 0, 0,
                           REAL(k0), REAL(k1), out_num ? INTEGER(VECTOR_ELT(rv_ans, 3)) : nullptr, REAL(afreq), SNPGPU_HOST,
                           opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(1);
    COREARRAY_CATCH
}

// k0 / k1: n x n matrices, or R_NilValue with the global pair (k0_all, k1_all)
static SEXP ibd_loglik(SEXP AFreq, SEXP k0, SEXP k1, double k0_all, double k1_all)
{
    COREARRAY_TRY
        PackedSpace ps;
        ps.read("MLE IBD log likelihood", false);
        const int n = (int)ps.n_samp;
        // the working space must be the one the coefficients were estimated on (snpgpu_ibd_loglik reads n_snp / n x n)
        if (!Rf_isNull(AFreq) && Rf_xlength(AFreq) != (R_xlen_t)ps.n_snp)
            throw ErrCoreArray("%s", "'afreq' should have one entry per SNP of the working space");
        if (!Rf_isNull(k0) && (Rf_xlength(k0) != (R_xlen_t)n * n || Rf_xlength(k1) != (R_xlen_t)n * n))
            throw ErrCoreArray("%s", "'k0' and 'k1' should be n x n matrices of the working space's samples");
        PROTECT(rv_ans = Rf_allocMatrix(REALSXP, n, n));
        if (snpgpu_ibd_loglik(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST,
                              Rf_isNull(AFreq) ? nullptr : REAL(AFreq), Rf_isNull(k0) ? nullptr : REAL(k0),
                              Rf_isNull(k0) ? nullptr : REAL(k1), k0_all, k1_all, REAL(rv_ans), nullptr, SNPGPU_HOST,
                              opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(1);
    COREARRAY_CATCH
}

COREARRAY_DLL_EXPORT SEXP gpu_gnrIBD_LogLik(SEXP AFreq, SEXP k0, SEXP k1)
{
    return ibd_loglik(AFreq, k0, k1, 0, 0);
}

COREARRAY_DLL_EXPORT SEXP gpu_gnrIBD_LogLik_k01(SEXP AFreq, SEXP k0, SEXP k1)
{
    return ibd_loglik(AFreq, R_NilValue, R_NilValue, as_real(k0), as_real(k1));
}

// LD pruning of the working space (one chromosome, set by the R loop): the kept reader packs it into 2-bit rows in host memory,
// and one snpgpu_ld_prune call counts the window's pair tables on the device and runs the greedy scan.  Coercions as gnrLDpruning:
// Rf_asInteger(StartIdx) - 1, Rf_asInteger of both window limits (R's double.xmax for an infinite slide.max.bp becomes NA_integer_,
// so that no SNP is in any window), Rf_asReal of the threshold.
COREARRAY_DLL_EXPORT SEXP gpu_gnrLDpruning(SEXP StartIdx, SEXP pos_bp, SEXP slide_max_bp, SEXP slide_max_n, SEXP LD_threshold,
                                           SEXP method, SEXP NumThread, SEXP verbose)
{
    const int start = Rf_asInteger(StartIdx) - 1;
    const int max_bp = Rf_asInteger(slide_max_bp), max_n = Rf_asInteger(slide_max_n);
    const int ld_method = Rf_asInteger(method);
    const bool vb = Rf_asLogical(verbose) == TRUE;
    if (Rf_asInteger(NumThread) <= 0) Rf_error("Invalid 'num.thread'.");
    COREARRAY_TRY
        const double threshold = as_real(LD_threshold);
        PackedSpace ps;
        ps.read("LD pruning", vb, 1);
        SEXP pos = PROTECT(Rf_coerceVector(pos_bp, INTSXP));
        if (Rf_xlength(pos) != (R_xlen_t)ps.n_snp) throw ErrCoreArray("%s", "'pos_bp' should have one entry per SNP of the working space");
        std::vector<uint8_t> keep(ps.n_snp, 0);
        snpgpu_opts o;
        memset(&o, 0, sizeof(o));
        o.device = opt_int("snpgpu.device", "SNPGPU_DEVICE", 0);
        if (snpgpu_ld_prune(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, start,
                            INTEGER(pos), max_bp, max_n, threshold, ld_method, &keep[0], &o, nullptr))
            gpu_fail();
        rv_ans = Rf_allocVector(R_LGLSXP, (R_xlen_t)ps.n_snp);
        PROTECT(rv_ans);
        int *p = INTEGER(rv_ans);            // a logical vector's data are ints (TRUE = 1)
        for (size_t i = 0; i < ps.n_snp; i++) p[i] = keep[i] ? TRUE : 0;
        UNPROTECT(2);
    COREARRAY_CATCH
}

// gnrFst(Pop, nPop, Method), src/genFst.cpp:170-242: list(Fst, per-SNP ratios[, beta]).  One pass over the working space's 2-bit rows
// gives the exact per-population allele counters on the device; the Fst terms are fp64 in the reference's order (snpgpu_fst).
COREARRAY_DLL_EXPORT SEXP gpu_gnrFst(SEXP Pop, SEXP nPop, SEXP Method)
{
    const int n_pop = Rf_asInteger(nPop);
    const char *method = CHAR(STRING_ELT(Method, 0));
    COREARRAY_TRY
        const bool wh02 = strcmp(method, "W&H02") == 0;
        if (!wh02 && strcmp(method, "W&C84") != 0) throw ErrCoreArray("%s", "'method' should be \"W&C84\" or \"W&H02\"");
        PackedSpace ps;
        ps.read("Fst", false, 1);
        if (Rf_xlength(Pop) != (R_xlen_t)ps.n_samp) throw ErrCoreArray("%s", "'Pop' should have one entry per sample of the working space");
        std::vector<int32_t> pop(ps.n_samp);
        const int *codes = INTEGER(Pop);              // a factor's codes start at 1
        for (size_t i = 0; i < ps.n_samp; i++) pop[i] = codes[i] - 1;
        PROTECT(rv_ans = Rf_allocVector(VECSXP, wh02 ? 3 : 2));
        SET_VECTOR_ELT(rv_ans, 0, Rf_allocVector(REALSXP, 1));
        SET_VECTOR_ELT(rv_ans, 1, Rf_allocVector(REALSXP, (R_xlen_t)ps.n_snp));
        if (wh02) SET_VECTOR_ELT(rv_ans, 2, Rf_allocMatrix(REALSXP, n_pop, n_pop));      // symmetric: either storage order
        if (snpgpu_fst(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, &pop[0], n_pop,
                       wh02 ? SNPGPU_FST_WH02 : SNPGPU_FST_WC84, REAL(VECTOR_ELT(rv_ans, 0)), REAL(VECTOR_ELT(rv_ans, 1)),
                       wh02 ? REAL(VECTOR_ELT(rv_ans, 2)) : nullptr, opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(1);
    COREARRAY_CATCH
}

// gnrSampFreq(), src/SNPRelate.cpp:275-283: the missing rate of every sample from the exact per-sample counters of one pass
COREARRAY_DLL_EXPORT SEXP gpu_gnrSampFreq()
{
    COREARRAY_TRY
        PackedSpace ps;
        ps.read("Sample missing rates", false, 1);
        std::vector<int32_t> miss(ps.n_samp);
        if (snpgpu_geno_counts(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, nullptr, &miss[0],
                               SNPGPU_HOST, opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        PROTECT(rv_ans = Rf_allocVector(REALSXP, (R_xlen_t)ps.n_samp));
        for (size_t i = 0; i < ps.n_samp; i++) REAL(rv_ans)[i] = (double)miss[i] / (double)ps.n_snp;
        UNPROTECT(1);
    COREARRAY_CATCH
}

// gnrHWE(), src/genHWE.cpp:117-137: the exact test per SNP on the counters of one pass (snpgpu_hwe)
COREARRAY_DLL_EXPORT SEXP gpu_gnrHWE()
{
    COREARRAY_TRY
        PackedSpace ps;
        ps.read("HWE", false, 1);
        PROTECT(rv_ans = Rf_allocVector(REALSXP, (R_xlen_t)ps.n_snp));
        if (snpgpu_hwe(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, REAL(rv_ans),
                       opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(1);
    COREARRAY_CATCH
}

static int inb_method_code(const char *m)
{
    static const char *const names[6] = {"mom.weir", "mom.visscher", "mle", "gcta1", "gcta2", "gcta3"};
    for (int k = 0; k < 6; k++)
        if (strcmp(m, names[k]) == 0) return k + 1;
    return 0;
}

// gnrIndInb(afreq, method, reltol, num_iter, verbose), src/genIBD.cpp:1847-2006: list(coefficients, iteration counts or NULL)
COREARRAY_DLL_EXPORT SEXP gpu_gnrIndInb(SEXP afreq, SEXP method, SEXP reltol, SEXP num_iter, SEXP verbose)
{
    const int code = inb_method_code(CHAR(STRING_ELT(method, 0)));
    const double rtol = as_real(reltol);
    const bool want_iter = Rf_asLogical(num_iter) == 1 && code == SNPGPU_INB_MLE;
    COREARRAY_TRY
        if (!code) throw ErrCoreArray("%s", "invalid 'method' of gnrIndInb");
        PackedSpace ps;
        ps.read("Individual inbreeding coefficients", Rf_asLogical(verbose) == 1, 1);
        const double *af = nullptr;
        SEXP af_real = R_NilValue;                     // the coerced copy stays protected across the allocations below
        if (!Rf_isNull(afreq)) {
            if (Rf_xlength(afreq) != (R_xlen_t)ps.n_snp) throw ErrCoreArray("%s", "'afreq' should have one entry per SNP of the working space");
            af_real = Rf_coerceVector(afreq, REALSXP);
        }
        PROTECT(af_real);
        if (af_real != R_NilValue) af = REAL(af_real);
        PROTECT(rv_ans = Rf_allocVector(VECSXP, 2));
        SET_VECTOR_ELT(rv_ans, 0, Rf_allocVector(REALSXP, (R_xlen_t)ps.n_samp));
        if (want_iter) SET_VECTOR_ELT(rv_ans, 1, Rf_allocVector(INTSXP, (R_xlen_t)ps.n_samp));
        if (snpgpu_ind_inb(&ps.rows[0], (int64_t)ps.n_snp, (int64_t)ps.n_samp, SNPGPU_GENO_PACKED2, SNPGPU_HOST, af, code, rtol,
                           REAL(VECTOR_ELT(rv_ans, 0)), want_iter ? INTEGER(VECTOR_ELT(rv_ans, 1)) : nullptr, nullptr, SNPGPU_HOST,
                           opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(2);
    COREARRAY_CATCH
}

// gnrIndInbCoef(snp, afreq, reltol), src/genIBD.cpp:1814-1827: the MLE of one individual as a one-sample call of snpgpu_ind_inb
// (one byte per genotype; anything outside 0 ... 2, NA_INTEGER included, is a missing call)
COREARRAY_DLL_EXPORT SEXP gpu_gnrIndInbCoef(SEXP snp, SEXP afreq, SEXP reltol)
{
    if (Rf_xlength(reltol) != 1) Rf_error("%s", "`reltol' should a real number.");
    const double rtol = as_real(reltol);
    COREARRAY_TRY
        const R_xlen_t n = Rf_xlength(snp);
        if (Rf_xlength(afreq) != n) throw ErrCoreArray("%s", "'snp' and 'afreq' should have the same length");
        SEXP snp_int = PROTECT(Rf_coerceVector(snp, INTSXP)), af_real = PROTECT(Rf_coerceVector(afreq, REALSXP));
        const int *g = INTEGER(snp_int);
        std::vector<uint8_t> rows((size_t)n);
        for (R_xlen_t i = 0; i < n; i++) rows[(size_t)i] = (g[i] >= 0 && g[i] <= 2) ? (uint8_t)g[i] : (uint8_t)3;
        double f = 0;
        if (snpgpu_ind_inb(&rows[0], (int64_t)n, 1, SNPGPU_GENO_U8, SNPGPU_HOST, REAL(af_real), SNPGPU_INB_MLE,
                           rtol, &f, nullptr, nullptr, SNPGPU_HOST, opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(2);
        rv_ans = Rf_ScalarReal(f);
    COREARRAY_CATCH
}

// R's random number interface (<R_ext/Random.h>; the reference's gnrDistPerm uses the same three)
void GetRNGstate(void);
void PutRNGstate(void);
double unif_rand(void);

// gnrDistPerm(n, dist, merge, n.perm, z.threshold), src/SNPRelate.cpp:549-677: list(z, n1, n2, group).  The permutations run on
// the device with a counter-based stream (snpgpu_dist_perm); its 64-bit seed is drawn here from R's generator, so set.seed()
// still governs a run -- the values differ from the CPU routine's, which consumes R's stream draw by draw.
COREARRAY_DLL_EXPORT SEXP gpu_gnrDistPerm(SEXP N_Dist, SEXP Dist, SEXP Merge, SEXP N_Perm, SEXP Z_Threshold)
{
    const int n = Rf_asInteger(N_Dist), n_perm = Rf_asInteger(N_Perm);
    const double z_threshold = as_real(Z_Threshold);
    GetRNGstate();
    const uint64_t hi = (uint64_t)(unif_rand() * 4294967296.0), lo = (uint64_t)(unif_rand() * 4294967296.0);
    PutRNGstate();
    COREARRAY_TRY
        if (n < 2) throw ErrCoreArray("%s", "gnrDistPerm: a tree has at least two samples");
        if (Rf_xlength(Dist) != (R_xlen_t)n * n || Rf_xlength(Merge) != 2 * (R_xlen_t)(n - 1))
            throw ErrCoreArray("%s", "gnrDistPerm: 'dist' should be n x n and 'merge' (n - 1) x 2");
        SEXP dist = PROTECT(Rf_coerceVector(Dist, REALSXP)), merge = PROTECT(Rf_coerceVector(Merge, INTSXP));
        PROTECT(rv_ans = Rf_allocVector(VECSXP, 4));
        SET_VECTOR_ELT(rv_ans, 0, Rf_allocVector(REALSXP, n - 1));
        SET_VECTOR_ELT(rv_ans, 1, Rf_allocVector(INTSXP, n - 1));
        SET_VECTOR_ELT(rv_ans, 2, Rf_allocVector(INTSXP, n - 1));
        SET_VECTOR_ELT(rv_ans, 3, Rf_allocVector(INTSXP, n));
        // R's matrix is column-major: dist[A[i] + n A[j]] there is dist[A[j]][A[i]] here, the transposed matrix -- the reference
        // indexes REAL(Dist) as dist[I[i] * n + I[j]] too, so the same buffer gives the same entries
        if (snpgpu_gnrDistPerm(n, REAL(dist), INTEGER(merge), n_perm, z_threshold, (hi << 32) | lo, REAL(VECTOR_ELT(rv_ans, 0)),
                               INTEGER(VECTOR_ELT(rv_ans, 1)), INTEGER(VECTOR_ELT(rv_ans, 2)), INTEGER(VECTOR_ELT(rv_ans, 3)),
                               opt_int("snpgpu.device", "SNPGPU_DEVICE", 0)))
            gpu_fail();
        UNPROTECT(3);
    COREARRAY_CATCH
}

}  // extern "C"
