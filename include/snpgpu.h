/*
 * snpgpu.h -- C ABI of libsnpgpu: MI355X (gfx950) pairwise relatedness kernels
 * behind SNPRelate's snpgds* hot path.
 *
 * Plain C, no SEXP / no torch types: pointers, sizes, status codes.  Every
 * entry point names the reference interface it replaces (paths relative to
 * the SNPRelate source tree, v1.46.0).  The R-side `.Call` shim that binds
 * these for a drop-in build of the package is shown in INTEGRATION.md.
 *
 * Two levels:
 *   (1) streaming accumulators  (snpgpu_create / _feed / finalisers / _destroy)
 *       replace the `CXxx::Run(CdMatTri<T>&, NumThread, verbose)` algorithm
 *       classes; the caller keeps the reference's GDS block reader
 *       (CGenoReadBySNP, src/dGenGWAS.cpp:1218-1397) and hands each block over;
 *   (2) workspace calls (snpgpu_ws_* / snpgpu_gnr*) mirror the registered
 *       `.Call` routines one to one (src/SNPRelate.cpp:1154-1205) on an
 *       in-memory genotype matrix, for hosts without gdsfmt (tests, Python).
 *
 * Conventions
 *   genotypes : SNP-major blocks, sample fastest (what CGenoReadBySNP::Read
 *               returns): SNPGPU_GENO_U8      uint8 [n_snp][n_samp], >2 = missing
 *                           (every byte 3..255 is a missing call, none is an error)
 *                         SNPGPU_GENO_PACKED2 uint8 [n_snp][ceil(n_samp/4)],
 *                           4 genotypes/byte LSB first, 3 = missing (GDS bit2);
 *                           the unused codes of a row's last byte (n_samp % 4
 *                           != 0) are ignored, whatever they hold
 *   triangles : packed upper, row-major with diagonal (CdMatTri,
 *               src/dGenGWAS.h:511-583): idx(i,j) = j + i(2N-i-1)/2, i <= j
 *   matrices  : full symmetric n x n, column-major == row-major
 *   status    : 0 = ok, non-zero = error; message via snpgpu_last_error()
 *   memory    : `mem` says whether a caller pointer is host or device memory
 *               (device pointers must belong to the context's device)
 *   threading : one context is used from one host thread at a time; calls
 *               block until the result is in the caller's buffer, in host or
 *               in device memory.  The exceptions are named where they are
 *               declared: snpgpu_feed of a device block, and the projector
 *               calls (1b) whose every pointer is device memory.
 */
#ifndef SNPGPU_H
#define SNPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNPGPU_ABI_VERSION 2

typedef struct snpgpu_ctx snpgpu_ctx;

enum snpgpu_kind {
    SNPGPU_IBS         = 1, /* CIBSCount        src/genIBS.cpp:145-329  */
    SNPGPU_KING_ROBUST = 2, /* CKINGRobust      src/genKING.cpp:283-482 */
    SNPGPU_KING_HOMO   = 3, /* CKINGHomo        src/genKING.cpp:58-266  */
    SNPGPU_GRM_GCTA    = 4, /* CGCTA_AlgArith   src/genPCA.cpp:1131-1238 */
    SNPGPU_PCA_COV     = 5, /* CExactPCA        src/genPCA.cpp:378-465 (also GRM "Eigenstrat") */
    SNPGPU_EIGMIX      = 6, /* CEigMix_AlgArith src/genEIGMIX.cpp:43-160 (also GRM "EIGMIX") */
    SNPGPU_INDIV_BETA  = 7, /* CIndivBeta       src/genBeta.cpp:57-252 (also GRM "IndivBeta") */
    SNPGPU_DISS        = 8  /* individual dissimilarity, IBS::DoDissCalculate src/genIBS.cpp:333-419 */
};

enum snpgpu_geno_format { SNPGPU_GENO_U8 = 0, SNPGPU_GENO_PACKED2 = 1 };
enum snpgpu_mem {
    SNPGPU_HOST = 0,        /* pageable host memory: the call returns when the block has been copied   */
    SNPGPU_DEVICE = 1,      /* device memory of the context's device                                   */
    SNPGPU_HOST_PINNED = 2  /* memory from snpgpu_host_alloc: snpgpu_feed only enqueues an asynchronous
                               copy on a second stream (double-buffered on the device), so the copy of
                               block k+1 overlaps the kernels of block k; call snpgpu_host_wait before
                               refilling the same buffer                                               */
};

typedef struct snpgpu_opts {
    int32_t device;         /* HIP device ordinal                                   */
    int32_t bayesian;       /* PCA_COV only: Bayesian normalisation, genPCA.cpp:441-453 */
    int64_t row_begin;      /* output panel = sample rows [row_begin,row_end) x cols>=row */
    int64_t row_end;        /*   0,0 = whole triangle. row_begin must be a multiple of 256 */
    int64_t max_block_snps; /* largest n_snp a single snpgpu_feed will pass (0 = 32768) */
    void   *stream;         /* hipStream_t to run on, or NULL for the context's own  */
} snpgpu_opts;

/* ---- library ---------------------------------------------------------- */
int         snpgpu_abi_version(void);
const char *snpgpu_last_error(void);  /* thread-local; replaces gnrErrMsg, src/SNPRelate.cpp:1099 */
int         snpgpu_device_count(int *count);

/* Synthetic genotype blocks for benchmarks and full-size parity tests (SURVEY.md 8(d) generator; no reference
 * counterpart): writes SNPs [snp_begin, snp_begin + n_snp) of the seeded data set as SNPGPU_GENO_PACKED2 rows
 * [n_snp][ceil(n_samp/4)] into DEVICE memory `dst`.  Counter-based: every cell is a pure integer function of
 * (seed, snp, sample), identical on every GPU and re-computable for single samples on the CPU
 * (oracle/synth.py).  spectrum 0: per-SNP p ~ U(0.05, 0.95); 1: p = u^3 / 2 (rare variants); 2: p ~ U(0.01, 0.5).
 * 3: three sub-populations (sample % 3) with Fst ~ 0.1 around an ancestral p ~ U(0.05, 0.95); 4: linkage disequilibrium --
 * blocks of 48 consecutive SNPs copied from 6 founder haplotypes per block, 2 % of the haplotype alleles drawn independently.
 * missing: iid missing-call rate.  special != 0 plants monomorphic / all-missing SNPs (snp % 997 in {3, 5, 7}).
 * stream: hipStream_t or NULL (the call then synchronises the device before -- an earlier asynchronous snpgpu_feed may
 * still be reading `dst` -- and after writing the block). */
int snpgpu_synth_block(void *dst, int64_t n_samp, int64_t snp_begin, int64_t n_snp, uint32_t seed, double missing,
                       int spectrum, int special, int device, void *stream);

/* ---- (1) streaming accumulators --------------------------------------- */
/* replaces the construction + memset part of CXxx::Run
 * (e.g. src/genIBS.cpp:280-299) */
int snpgpu_create(int kind, int64_t n_samp, const snpgpu_opts *opts, snpgpu_ctx **out);
int snpgpu_destroy(snpgpu_ctx *ctx);

/* replaces one iteration of `while (WS.Read(Geno))` { pack / centre ; BatchWork }
 * (src/genIBS.cpp:312-327, src/genKING.cpp:465-480, src/genPCA.cpp:428-462, :1185-1230).
 * Asynchronous w.r.t. the device when `mem` is SNPGPU_DEVICE: the block must stay allocated and unchanged until the pre-pass
 * has read it -- snpgpu_sync, or any call that orders after the context's stream. */
int snpgpu_feed(snpgpu_ctx *ctx, const void *geno, int64_t n_snp, int format, int mem);
/* The block's per-SNP statistics (sum of called genotypes, number of calls over ALL n_samp samples; vec_u8_geno_count,
 * src/dVect.cpp:30-117) computed ONCE per node instead of once per rank: every rank calls snpgpu_block_stats on its share of the
 * block's SNP rows (device memory, rows of the given format; sum / num: device arrays of n_snp int32), all-gathers the two arrays
 * (8 bytes per SNP) and feeds the whole block with snpgpu_feed_stats, which then only re-lays the rows out (sum / num: device
 * memory).  Same results as snpgpu_feed bit for bit (integer statistics).  snprelate_amd/multigpu.py: shared_stats=True. */
int snpgpu_block_stats(snpgpu_ctx *ctx, const void *geno, int64_t n_snp, int format, int32_t *sum, int32_t *num);
int snpgpu_feed_stats(snpgpu_ctx *ctx, const void *geno, int64_t n_snp, int format, int mem, const int32_t *sum, const int32_t *num);
int snpgpu_sync(snpgpu_ctx *ctx);
/* page-locked host buffers for SNPGPU_HOST_PINNED feeds (the R shim allocates the reader's two
 * block buffers with this instead of VEC_AUTO_PTR, src/genIBS.cpp:305) */
int snpgpu_host_alloc(size_t bytes, void **out);
int snpgpu_host_free(void *p);
/* block until the last asynchronous copy out of `host_buf` issued by this context is complete */
int snpgpu_host_wait(snpgpu_ctx *ctx, const void *host_buf);
/* number of SNPs fed so far, and of those the polymorphic ones (GCTA's nLocus,
 * src/genPCA.cpp:1206; maintained by GRM_GCTA contexts only -- the IBS / KING-robust counters need no per-SNP
 * statistics and their pre-pass does not compute any) */
int snpgpu_counts(snpgpu_ctx *ctx, int64_t *n_snp_total, int64_t *n_locus);
/* Optional HIP-event timing of the dominant pair kernel launches inside snpgpu_feed
 * (events are recorded on the context's stream around each launch).  `which`: 0 = bit-plane
 * pair kernel, 1 = MFMA SYRK kernel.  Returns the summed kernel time and the number of timed
 * spans since timing was (re-)enabled: one span per feed block for the counters, one per table and
 * feed block for the SYRK family, whatever number of kernel launches a span holds
 * (snpgpu_diag_syrk_launches counts those). */
int snpgpu_set_timing(snpgpu_ctx *ctx, int enable);
int snpgpu_get_timing(snpgpu_ctx *ctx, int which, double *ms_sum, int64_t *launches);
/* size (elements) of the packed slab this context's panel produces */
int64_t snpgpu_slab_size(const snpgpu_ctx *ctx);

/* Finalisers.  `packed` != 0: write the packed-triangle slab of the panel
 * (rows row_begin..row_end-1; the whole triangle for a full context) --
 * the `useMatrix=TRUE` outputs.  `packed` == 0: write the full symmetric
 * n x n matrix (full contexts only). */

/* gnrIBSNum finaliser, src/genIBS.cpp:521-543: three int32 matrices */
int snpgpu_ibs_num(snpgpu_ctx *ctx, int32_t *ibs0, int32_t *ibs1, int32_t *ibs2,
                   int packed, int mem);
/* gnrIBSAve finaliser, src/genIBS.cpp:463-490 */
int snpgpu_ibs_ave(snpgpu_ctx *ctx, double *out, int packed, int mem);
/* raw KING-robust counters {IBS0,nLoci,SumSq,N1_Aa,N2_Aa} (TS_KINGRobust,
 * src/genKING.cpp:274-281), packed slab, uint32 [npair][5] */
int snpgpu_king_robust_counts(snpgpu_ctx *ctx, uint32_t *out5, int mem);
/* gnrIBD_KING_Robust finaliser, src/genKING.cpp:614-667.
 * family: int32 [n_samp] (host), negative = NA; NULL = all NA */
int snpgpu_king_robust(snpgpu_ctx *ctx, const int32_t *family, double *ibs0, double *kinship,
                       int packed, int mem);
/* gnrIBD_KING_Homo finaliser, src/genKING.cpp:516-560 */
int snpgpu_king_homo(snpgpu_ctx *ctx, double *k0, double *k1, int packed, int mem);
/* gnrDiss finaliser, src/genIBS.cpp:652-683: SumGeno / SumAFreq off the diagonal, 2 SumGeno / SumAFreq on it
 * (IEEE division: 0/0 = NaN, x/0 = Inf, as the reference) */
int snpgpu_diss(snpgpu_ctx *ctx, double *out, int packed, int mem);
/* the dissimilarity sums themselves (diagnostics, tests), packed slab: SumGeno = sum of g_i (2 - g_j) + (2 - g_i) g_j and
 * SumAFreq = sum of 8 p (1 - p), both over the SNPs where both samples are called */
int snpgpu_diss_sums(snpgpu_ctx *ctx, uint32_t *geno_sum, double *wsum, int mem);
/* GCTA GRM: numerator / (2 (nLocus - Denom)), src/genPCA.cpp:1232-1236 + grm_output :1586-1602 */
int snpgpu_grm_gcta(snpgpu_ctx *ctx, double *out, int packed, int mem);
/* PCA covariance.  normalize != 0 applies C *= (n-1)/trace (src/genPCA.cpp:1386-1390;
 * needs the whole diagonal, i.e. a full context, unless `trace_in` > 0 is supplied);
 * trace_xtx receives the trace of this panel's diagonal BEFORE scaling (may be NULL). */
int snpgpu_pca_cov(snpgpu_ctx *ctx, double *out, int packed, int normalize, double trace_in,
                   double *trace_xtx, int mem);
/* PLINK method of moments on an IBS context: per-pair k0/k1 (Est_PLINK_Kinship,
 * src/genIBD.cpp:341-390; loops of gnrIBD_PLINK, src/genIBS.cpp:590-628).
 * e[5] = {E00, E01, E02, E11, E12} of EPrIBS_IBD (Init_EPrIBD_IBS, src/genIBD.cpp:253-338). */
int snpgpu_ibd_mom(snpgpu_ctx *ctx, const double *e, int kinship_constraint, double *k0, double *k1,
                   int packed, int mem);
/* EIGMIX coancestry: numerator / (SumDenominator - Denom), optional diagonal adjustment, times
 * `scale` (2 for snpgdsGRM(method="EIGMIX"), src/genEIGMIX.cpp:146-155, :645-653) */
int snpgpu_eigmix(snpgpu_ctx *ctx, int diagadj, double scale, double *out, int packed, int mem);
/* individual beta.  mode 0/1: gnrIBD_Beta with inbreeding = FALSE/TRUE (src/genBeta.cpp:384-452),
 * mode 2: CalcIndivBetaGRM (min-based transform, src/genBeta.cpp:263-357).  avg_val receives
 * grm_avg_value.  Full contexts only (the transform needs all pairs). */
int snpgpu_indiv_beta(snpgpu_ctx *ctx, int mode, double *out, double *avg_val, int packed, int mem);
/* top-k eigenpairs of the (normalised, full-context) PCA covariance:
 * replaces CalcEigen / LAPACK dspevx (src/genPCA.cpp:1262-1346).
 * eigval: HOST double [k] descending, whatever `mem` says (as snpgpu_panels_topk_eigen); eigvec: double [n_samp][k]
 * column-major (n x k) in `mem`.
 * n <= SNPGPU_EIG_DENSE_MAX (default 2048): hipSOLVER's dense syevd on the finalised matrix, the k largest pairs of it
 * (the reference asks LAPACK for the index range 1..k; syevdx with that range fails on multiple eigenvalues);
 * larger n: the block-Krylov solver below on the resident panel (no n x n copy). */
int snpgpu_pca_eigen(snpgpu_ctx *ctx, int k, double *eigval, double *eigvec, int mem);

/* Building block of the distributed top-k eigen solver (snprelate_amd/eigen.py) that replaces
 * LAPACK dspevx at sizes where a dense solve is impossible: with the symmetric covariance held as
 * row panels on several devices,   Y += scale * C Q   is the sum over panels of
 *     Y[I]     += scale * P[I, r0:N]   Q[r0:N]
 *     Y[r1:N]  += scale * P[I, r1:N]^T Q[I]          (I = [r0,r1) = the panel's rows)
 * This call adds ONE panel's contribution (one pass over the fp64 panel accumulator on fp64 MFMAs, every
 * tile used for both triangles, after mirroring the panel's diagonal block; SNPGPU_EIG_BLAS=1: two rocBLAS
 * dgemms).  Q, Y: device pointers, column-major n_samp x m
 * (leading dimension n_samp).  PCA_COV contexts only; no feeds may follow. */
int snpgpu_pca_panel_matmul(snpgpu_ctx *ctx, double scale, const double *Q, int m, double *Y);
/* The same product with the panel values and the vectors rounded to fp32 and fp32 matrix instructions: half the time of
 * the fp64 form (which is bound by the fp64 matrix rate and its atomics); sums of more than 1024 terms and the result stay
 * fp64.  Relative error of a product ~5e-7 rms: what the Krylov solver runs most of its products on (snpgpu_eig_opts). */
int snpgpu_pca_panel_matmul_f32(snpgpu_ctx *ctx, double scale, const double *Q, int m, double *Y);
/* trace of this panel's diagonal (raw sums, before any scaling) */
int snpgpu_pca_panel_trace(snpgpu_ctx *ctx, double *trace);

/* Turn the accumulators into the FINAL matrix in place (the panel rectangle of fp64 sums becomes the result itself), so that
 * the panel product / the eigen solver below can work on matrices that are more than raw sums: GRM_GCTA
 * (numerator / (2 (nLocus - Denom)), src/genPCA.cpp:1232-1236) and EIGMIX (src/genEIGMIX.cpp:146-155 with `diagadj`, times
 * `scale`).  For PCA_COV it only settles pending terms (the (n-1)/trace factor travels with the products).  No block may be
 * fed afterwards; the kind's own finaliser (snpgpu_grm_gcta / snpgpu_eigmix) keeps working and copies the stored matrix out. */
int snpgpu_finalize_inplace(snpgpu_ctx *ctx, int diagadj, double scale);
/* Sampled reads of the panel's fp64 result plane (host arrays; sample indices with row_begin <= rows[k] < row_end, cols[k] >=
 * rows[k]): the FINAL matrix entries after snpgpu_finalize_inplace (GRM_GCTA / EIGMIX), the settled raw sums of a PCA_COV
 * context otherwise.  For parity checks at sizes where no slab can be copied out whole (sampled tiles of the
 * 500 000-sample job recomputed in fp64 on the host); no reference counterpart. */
int snpgpu_panel_entries(snpgpu_ctx *ctx, const int64_t *rows, const int64_t *cols, int64_t n_entries, double *out);

/* Related pairs straight from the resident counters: the table snpgdsIBDSelection(ibdobj, kinship.cutoff, samp.sel)
 * (R/IBD.R:463-531) would cut out of the n x n matrices of snpgdsIBDKING / snpgdsIBDMoM, without those matrices -- only the selected
 * pairs leave the device.  Selected: the pairs idx1 < idx2 of the panel (row_begin <= idx1 < row_end) with samp_sel[idx1] &&
 * samp_sel[idx2] and kinship >= kinship_cutoff (R/IBD.R:500-506: a NaN kinship is never selected; a non-finite cutoff -- NaN, +-Inf,
 * is.finite() is FALSE for all three -- selects every pair, NaN pairs included).  Order: idx1 ascending, then idx2 ascending =
 * which(lower.tri & flag, arr.ind = TRUE) with ID1 = sample[col], ID2 = sample[row] (R/IBD.R:520-526); the same call gives the same
 * arrays.  The values are those of the kind's finaliser, bit for bit:
 *   SNPGPU_SEL_KING_ROBUST  KING_ROBUST context: IBS0 and kinship of snpgpu_king_robust (family as there)
 *   SNPGPU_SEL_KING_HOMO    KING_HOMO context:   k0, k1 of snpgpu_king_homo, kinship = (1 - k0 - k1) * 0.5 + k1 * 0.25 (R/IBD.R:487)
 *   SNPGPU_SEL_MOM          IBS context:         k0, k1 of snpgpu_ibd_mom(e, kinship_constraint), the same kinship
 * This direct route has no reference counterpart (the reference selects from matrices it has already built). */
enum snpgpu_sel_kind { SNPGPU_SEL_KING_ROBUST = 1, SNPGPU_SEL_KING_HOMO = 2, SNPGPU_SEL_MOM = 3 };
typedef struct snpgpu_sel_opts {
    int32_t        what;                /* snpgpu_sel_kind; must match the context's kind                    */
    int32_t        kinship_constraint;  /* MOM only                                                          */
    const int32_t *family;              /* KING_ROBUST: host int32 [n_samp], negative = NA; NULL = all NA    */
    const double  *e;                   /* MOM: host double [5], as snpgpu_ibd_mom                           */
    double         kinship_cutoff;      /* non-finite: every pair                                            */
    const uint8_t *samp_sel;            /* host uint8 [n_samp], nonzero = selected; NULL = all               */
} snpgpu_sel_opts;
/* idx1 < idx2: 0-based sample indices; v0 / v1: IBS0 / (not written) for KING_ROBUST, k0 / k1 otherwise; any output may be
 * NULL (capacity 0 with all NULL = count only).  Outputs in `mem` (host or the context's device), `capacity` elements each: the first
 * `capacity` pairs of the order above are stored, nothing is written behind them, and *n_found is always the number of ALL selected
 * pairs.  Refused: a NULL context or NULL opts, a `what` that does not match the context kind, MOM without e, a negative capacity,
 * a non-NULL output with capacity 0. */
int snpgpu_select_pairs(snpgpu_ctx *ctx, const snpgpu_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2,
                        double *v0, double *v1, double *kinship, int mem, int64_t *n_found);
/* diagnostics (tools/ibd_select_bench.py): milliseconds of the last snpgpu_select_pairs on this thread, double [4] = {count pass,
 * scan, write pass} on the device and the whole call on the host clock; no reference counterpart */
int snpgpu_select_stats(double *ms4);

/* The sparse GRM straight from the resident sums: every sample's own entry (diag) and the pairs idx1 < idx2 of the panel with
 * samp_sel[idx1] && samp_sel[idx2] and value >= cutoff (a NaN value is never selected; a non-finite cutoff selects every pair), in
 * the order of snpgpu_select_pairs (idx1 ascending, then idx2 ascending), by the same count pass, scan and write pass: no atomic,
 * the same call gives the same arrays.  The values are those of the kind's finaliser, bit for bit:
 *   SNPGPU_SEL_GRM_GCTA        GRM_GCTA context:   snpgpu_grm_gcta (pending terms folded on the fly: further feeds may follow)
 *   SNPGPU_SEL_GRM_EIGENSTRAT  PCA_COV context:    snpgpu_pca_cov(normalize = 1, trace_in); a panel needs trace_in > 0
 *   SNPGPU_SEL_GRM_EIGMIX      EIGMIX context:     snpgpu_eigmix(diagadj = mode, scale)
 *   SNPGPU_SEL_GRM_INDIV_BETA  INDIV_BETA context: snpgpu_indiv_beta(mode), full contexts only
 * Contexts frozen by snpgpu_finalize_inplace (GCTA, EIGMIX) are read as their finalisers read them.  The correlation form of
 * snpgpu_gnrGRM ("Corr") is not built: G_ij / sqrt(G_ii G_jj) needs the diagonal of every column, which a row panel does not hold.
 * No reference counterpart (the reference builds the whole matrix). */
enum snpgpu_grm_sel_kind { SNPGPU_SEL_GRM_GCTA = 1, SNPGPU_SEL_GRM_EIGENSTRAT = 2, SNPGPU_SEL_GRM_EIGMIX = 3, SNPGPU_SEL_GRM_INDIV_BETA = 4 };
typedef struct snpgpu_grm_sel_opts {
    int32_t what;            /* snpgpu_grm_sel_kind; must match the context's kind                     */
    int32_t mode;            /* EIGMIX: diagadj; INDIV_BETA: 0 / 1 / 2 as snpgpu_indiv_beta            */
    double  scale;           /* EIGMIX only (2 for snpgdsGRM(method = "EIGMIX"))                       */
    double  trace_in;        /* EIGENSTRAT on a panel: the trace of ALL panels; 0 = the context's own  */
    double  cutoff;          /* value >= cutoff; non-finite: every pair                                */
    const uint8_t *samp_sel; /* host [n_samp] or NULL                                                  */
} snpgpu_grm_sel_opts;
/* Host outputs only (a device destination is not built).  idx1, idx2, value: `capacity` elements each, the first `capacity` pairs
 * are stored and nothing is written behind them, *n_found is always the number of ALL selected pairs; capacity 0 with the three
 * NULL counts only.  diag: double [min(row_end, n_samp) - row_begin], the finaliser's entry (i, i) of every row of the panel
 * whatever samp_sel says; avg_val: the grm_avg_value of INDIV_BETA; both independent of capacity, each may be NULL.  Refused
 * before any device call: NULL opts, an unknown `what`, EIGMIX with a non-finite or non-positive scale, a mode out of range, a
 * negative capacity, a pair output with capacity 0, a NULL context; then a `what` that does not match the context kind. */
int snpgpu_select_grm(snpgpu_ctx *ctx, const snpgpu_grm_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2,
                      double *value, double *diag, double *avg_val, int64_t *n_found);
/* diagnostics (tools/grm_pairs_bench.py): milliseconds of the last snpgpu_select_grm on this thread, double [5] = {count pass, scan,
 * write pass, diagonal kernel} on the device and the whole call on the host clock; no reference counterpart */
int snpgpu_select_grm_stats(double *ms5);

/* Top-k eigenpairs of the symmetric matrix held as row panels: replaces CalcEigen / LAPACK dspevx for ANY n
 * (src/genPCA.cpp:1262-1346; the same call behind gnrEigMix, src/genEIGMIX.cpp:700-702).  Thick-restarted block Krylov +
 * Rayleigh-Ritz in C++ / HIP (csrc/eigen.hip): the O(n^2) product runs on the panels, the tall-skinny algebra on their
 * device.  `panels`: contexts on ONE device -- PCA_COV, or GRM_GCTA / EIGMIX after snpgpu_finalize_inplace -- that tile
 * [0, n) of the triangle, or (one process per GPU) this rank's share of it: then opts->reduce must sum opts->y_buf
 * (double [block][n], device memory owned by the caller) over the ranks in place, e.g. one RCCL all-reduce.
 * The matrix is `scale` times the panels' contents (PCA: (n-1) / trace, src/genPCA.cpp:1386-1390).
 * eigval: HOST double [k] descending; eigvec: double [n][k] column-major (n x k) in `mem` (host, or the panels' device). */
typedef int (*snpgpu_reduce_fn)(void *user);
typedef struct snpgpu_eig_opts {
    double   tol;            /* largest relative residual |C v - theta v| / |theta| accepted (0 = 1e-9)            */
    int32_t  block;          /* vectors per Krylov block (0 = k + 8 rounded up to a multiple of 16)               */
    int32_t  depth;          /* blocks per restart cycle (0 = 24, fewer while the device lacks the memory)        */
    int32_t  max_restarts;   /* 0 = 60                                                                             */
    uint32_t seed;           /* start block (0 = 20240601); identical on every rank                               */
    double  *y_buf;          /* with `reduce`: the buffer every product is formed in before it is reduced         */
    snpgpu_reduce_fn reduce; /* NULL: the panels are the whole matrix                                              */
    void    *user;
    double   fp32_until;     /* mixed precision.  Restart cycles run entirely on fp32 products until the residual falls
                                below this (or stops falling); from then on only the product of a cycle's first block --
                                the vectors the previous cycle returned -- is fp64, which also yields their true
                                residual: that fp64 figure is what accepts the result (and is `max_rel_residual`).
                                0 = 1e-5, < 0 = fp64 products only (also: SNPGPU_EIG_FP32=0)                         */
} snpgpu_eig_opts;
typedef struct snpgpu_eig_info {
    int32_t restarts, matmuls, block, depth;
    double  max_rel_residual;
    int32_t matmuls_fp32;    /* how many of `matmuls` were fp32 products */
    int32_t reserved;
} snpgpu_eig_info;
int snpgpu_panels_topk_eigen(snpgpu_ctx *const *panels, int n_panels, double scale, int k, const snpgpu_eig_opts *opts,
                             double *eigval, double *eigvec, int mem, snpgpu_eig_info *info);

/* ---- (1c) several GPUs driven by ONE host process (an R session) ----------------------------------------------------
 * north_star: "the N x N output triangle is row-block partitioned across the 8 GPUs of one node with a final gather over
 * xGMI".  The object cuts the packed triangle into equal-area row panels (the device-level analogue of Array_SplitJobs,
 * src/dGenGWAS.cpp:2202-2216), `panels_per_device` per device (several even out the memory: the last equal-area panel is
 * a square holding a triangle), and creates one accumulator context per panel.  snpgpu_multi_feed moves a block across
 * PCIe ONCE, to devices[0], and forwards it to the other devices over xGMI (hipMemcpyPeerAsync, double-buffered, under the
 * kernels of the previous block); there is no collective on the data path.  The gathers below write the packed triangle
 * (CdMatTri order) -- every panel's slab is a contiguous range of it -- into host memory, or into device memory of
 * devices[0] through peer copies.  n_passes > 1: only the panels of pass `pass` are resident (output-stationary: KING-robust
 * keeps 20 B per pair, 2.5 TB at N = 500 000); the caller walks the SNP stream once per pass and every pass's gather fills
 * its own ranges of the same output.  A device may be listed more than once (tests: several "devices" on one GPU). */
typedef struct snpgpu_multi snpgpu_multi;
typedef struct snpgpu_multi_opts {
    const int32_t *devices;      /* HIP device ordinals                                  */
    int32_t n_devices;
    int32_t panels_per_device;   /* 0 = 1; -1 = the fewest that fit the devices' free memory (accumulators + per-panel scratch).
                                    With n_passes > 1 every pass must use the SAME value (the plan is cut into devices x panels x passes
                                    panels): resolve -1 once, in pass 0, and give the later passes what snpgpu_multi_get_status reports */
    int32_t n_passes;            /* 0 = 1                                                */
    int32_t pass;                /* 0 .. n_passes - 1                                    */
} snpgpu_multi_opts;
/* opts: bayesian and max_block_snps are used (device, rows and stream are set per panel) */
int snpgpu_multi_create(int kind, int64_t n_samp, const snpgpu_opts *opts, const snpgpu_multi_opts *mopts, snpgpu_multi **out);
int snpgpu_multi_destroy(snpgpu_multi *m);
/* number of resident panels; whether the eigen solver's broadcast / reduce go through RCCL (distinct devices and librccl
 * loadable; SNPGPU_MULTI_COMM=peer|rccl overrides) or through peer copies */
int snpgpu_multi_info(const snpgpu_multi *m, int *n_panels, int *uses_rccl);
/* one broadcast + one sum-reduction of a known pattern over the object's devices through the exchange path the eigen solver
 * uses (RCCL communicator, or peer copies when none could be built -- which snpgpu_multi_create reports on stderr and
 * SNPGPU_MULTI_COMM=rccl turns into an error): non-zero, with a message, if any device returns the wrong sum */
int snpgpu_multi_comm_selftest(snpgpu_multi *m, int *uses_rccl);
/* After a successful snpgpu_multi_comm_selftest the two data paths have been exercised as well (round 6): a known 2-bit block forwarded
 * from the first device to every other one the way snpgpu_multi_feed does it, verified on each receiving device, and a known slab
 * from every device written into its range of one buffer on the first device the way the gathers do it (one host thread per device,
 * asynchronous peer copies), verified there.  What the object found out about its devices: */
typedef struct snpgpu_multi_status {
    int32_t n_devices, n_distinct_devices, n_panels;
    int32_t panels_per_device;   /* of the plan: the resolved value when snpgpu_multi_opts.panels_per_device was -1                 */
    int32_t uses_rccl;           /* the eigen solver's broadcast / reduce go through an RCCL communicator                            */
    int32_t peer_pairs;          /* ordered pairs (a, b) of distinct devices of the list ...                                        */
    int32_t peer_pairs_enabled;  /* ... of which hipDeviceCanAccessPeer said yes and hipDeviceEnablePeerAccess succeeded (the others:
                                    a line on stderr at create; their copies are staged through host memory by the runtime)         */
    int32_t selftest_comm, selftest_feed, selftest_gather;   /* snpgpu_multi_comm_selftest: -1 not run, 0 failed, 1 passed           */
    int32_t reserved[6];
} snpgpu_multi_status;
int snpgpu_multi_get_status(const snpgpu_multi *m, snpgpu_multi_status *out);
/* panel i: its context (any level-1 call may be made on it), rows and device */
int snpgpu_multi_panel(const snpgpu_multi *m, int i, snpgpu_ctx **ctx, int64_t *row_begin, int64_t *row_end, int *device);
/* as snpgpu_feed; SNPGPU_DEVICE = memory of devices[0], which must stay untouched until snpgpu_multi_sync */
int snpgpu_multi_feed(snpgpu_multi *m, const void *geno, int64_t n_snp, int format, int mem);
int snpgpu_multi_host_wait(snpgpu_multi *m, const void *host_buf);
int snpgpu_multi_sync(snpgpu_multi *m);
int snpgpu_multi_counts(snpgpu_multi *m, int64_t *n_snp_total, int64_t *n_locus);
/* gathers of the packed triangle; `mem`: SNPGPU_HOST, or SNPGPU_DEVICE = memory of devices[0] */
int snpgpu_multi_ibs_num(snpgpu_multi *m, int32_t *ibs0, int32_t *ibs1, int32_t *ibs2, int mem);
int snpgpu_multi_ibs_ave(snpgpu_multi *m, double *out, int mem);
int snpgpu_multi_king_robust(snpgpu_multi *m, const int32_t *family, double *ibs0, double *kinship, int mem);
int snpgpu_multi_king_robust_counts(snpgpu_multi *m, uint32_t *out5, int mem);
int snpgpu_multi_king_homo(snpgpu_multi *m, double *k0, double *k1, int mem);
int snpgpu_multi_diss(snpgpu_multi *m, double *out, int mem);
int snpgpu_multi_grm_gcta(snpgpu_multi *m, double *out, int mem);
int snpgpu_multi_eigmix(snpgpu_multi *m, int diagadj, double scale, double *out, int mem);
/* snpgpu_select_pairs over the resident panels in order of row_begin, results concatenated: the global order (idx1, then idx2) of
 * snpgdsIBDSelection, R/IBD.R:463-531; a pass of an n_passes > 1 object returns its own panels' pairs.  `capacity` and *n_found refer
 * to the concatenation.  Host outputs only.  No reference counterpart, as snpgpu_select_pairs. */
int snpgpu_multi_select_pairs(snpgpu_multi *m, const snpgpu_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2,
                              double *v0, double *v1, double *kinship, int mem /* host */, int64_t *n_found);
/* snpgpu_select_grm over the resident panels in order of row_begin, the pairs concatenated as in snpgpu_multi_select_pairs.
 * diag: double [n_samp]; every resident panel writes its own rows, a pass of an n_passes > 1 object leaves the other rows
 * untouched.  EIGENSTRAT with trace_in == 0 takes snpgpu_multi_pca_trace (the whole trace only when all panels are resident).
 * INDIV_BETA is refused: it needs a full context. */
int snpgpu_multi_select_grm(snpgpu_multi *m, const snpgpu_grm_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2,
                            double *value, double *diag, int64_t *n_found);
int snpgpu_multi_pca_trace(snpgpu_multi *m, double *trace);
/* out may be NULL (trace only); normalize != 0: C *= (n-1)/trace with the trace of ALL panels */
int snpgpu_multi_pca_cov(snpgpu_multi *m, double *out, int normalize, double *trace_xtx, int mem);
/* snpgpu_finalize_inplace on every panel */
int snpgpu_multi_finalize_inplace(snpgpu_multi *m, int diagadj, double scale);
/* top-k eigenpairs over all devices (a one-pass plan; GRM_GCTA / EIGMIX after snpgpu_multi_finalize_inplace): the
 * tall-skinny algebra runs on devices[0], every product Y = C Q on all devices -- the vector block is broadcast, the
 * partial products are reduced (RCCL ncclBroadcast / ncclReduce, or peer copies).  PCA_COV with scale <= 0: the
 * (n-1)/trace factor of gnrPCA.  eigval: host; eigvec: n x k column-major in `mem` (host / devices[0]); opts->reduce must
 * be NULL. */
int snpgpu_multi_topk_eigen(snpgpu_multi *m, double scale, int k, const snpgpu_eig_opts *opts, double *eigval, double *eigvec,
                            int mem, snpgpu_eig_info *info);

/* ---- (1b) PCA projections: SNP correlations, SNP loadings, sample loadings ---
 * A projector holds the sample-side matrix and per-block scratch; the caller keeps its block reader
 * (CGenoReadBySNP) and hands over one block at a time, as for the accumulators.  All arithmetic is fp64.
 * Matrices use R's layouts: eigvec = n_samp x n_eig column-major ([n_eig][n_samp]); per-block outputs
 * = n_eig x n_snp column-major ([n_snp][n_eig]); sample loadings = n_samp x n_eig column-major.
 * Synchronisation.  A call that is given any host pointer (block, inputs or results) blocks until its results are in the caller's
 * buffers and its host inputs may be reused.  A call whose every pointer is device memory -- snpgpu_proj_set_eigvec of device
 * eigenvectors; a block call with a device block, or geno == NULL, and device inputs and results -- is STREAM-ORDERED, as snpgpu_feed
 * of a device block: it is enqueued on the projector's stream (opts->stream, or the projector's own non-blocking stream) and
 * returns at once.  Its inputs must stay unchanged, and its results are complete, only after snpgpu_proj_sync or any work that
 * orders after that stream; later calls on the same projector are ordered after it.  (The randomised PCA runs its per-block
 * products this way, without a synchronisation per block.)  snpgpu_proj_samp_loading always blocks. */
typedef struct snpgpu_proj snpgpu_proj;
int snpgpu_proj_create(int64_t n_samp, int n_eig, const snpgpu_opts *opts, snpgpu_proj **out);
int snpgpu_proj_destroy(snpgpu_proj *p);
int snpgpu_proj_sync(snpgpu_proj *p);
/* eigenvectors of the samples (for gnrPCASNPLoading already multiplied by sqrt((n-1)/TraceXTX/eigenval),
 * src/genPCA.cpp:1499-1507) */
int snpgpu_proj_set_eigvec(snpgpu_proj *p, const double *eigvec, int mem);
/* body of CPCA_SNPCorr::Run (src/genPCA.cpp:860-899): Pearson correlation of each SNP of the block with
 * each eigenvector over the called genotypes; NaN for < 2 calls or zero variance */
int snpgpu_proj_snp_corr(snpgpu_proj *p, const void *geno, int64_t n_snp, int format, int mem,
                         double *out, int out_mem);
/* body of CPCA_SNPLoad::Run (src/genPCA.cpp:1000-1035): loading [n_snp][n_eig], afreq [n_snp] (mean
 * genotype), scale [n_snp] */
int snpgpu_proj_snp_loading(snpgpu_proj *p, const void *geno, int64_t n_snp, int format, int mem, int bayesian,
                            double *loading, double *afreq, double *scale, int out_mem);
/* the same product with the caller's centring and scaling, loading = sum_i (g_i - avg) * scale * eigvec_i over the
 * called genotypes: body of CEigMix_SNPLoad::Run (src/genEIGMIX.cpp:440-512) with avg = 2 * afreq and
 * scale = 1 / sqrt(sum 4 p (1 - p)) */
int snpgpu_proj_snp_loading_ext(snpgpu_proj *p, const void *geno, int64_t n_snp, int format, int mem, const double *avg,
                                const double *scale, int in_mem, double *loading, int out_mem);
/* body of CPCA_SampleLoad::Run (src/genPCA.cpp:1070-1110): accumulate one block; sload [n_snp][n_eig]
 * (SNP loadings times sqrt(ss/eigenval), R/PCA.R:283-285), afreq / scale as returned above */
int snpgpu_proj_samp_loading_feed(snpgpu_proj *p, const void *geno, int64_t n_snp, int format, int mem,
                                  const double *sload, const double *afreq, const double *scale, int in_mem);
/* The sums accumulated so far, n_samp x n_eig.  The accumulator is only read: a second call returns the same bytes, and a
 * block fed afterwards adds to the same sums.  A projector starts with zero sums. */
int snpgpu_proj_samp_loading(snpgpu_proj *p, double *out, int out_mem);
/* zero the accumulator for another pass (stream-ordered; the eigenvectors and the staged block stay) */
int snpgpu_proj_samp_loading_reset(snpgpu_proj *p);
/* In the four block calls geno == NULL reuses the block staged by the previous block call on this projector
 * (same n_snp; format and mem are then ignored): the randomised PCA multiplies every block by Y and by Y^T in one pass. */

/* ---- (2) workspace level: mirrors of the registered .Call routines ------ */
/* gnrSetGenoSpace(Node, SelSamp, SelSNP), src/SNPRelate.cpp:76-114: install an
 * in-memory genotype matrix (host, copied) as the process-global working space */
int snpgpu_ws_set_geno(const void *geno, int64_t n_snp, int64_t n_samp, int format, int device);
/* gnrSelSNP_Base(remove_mono, maf, missrate), src/SNPRelate.cpp:184-210 ->
 * CdBaseWorkSpace::Select_SNP_Base, src/dGenGWAS.cpp:361-397.
 * sel_out: uint8 [n_snp of the current selection] (may be NULL) */
int snpgpu_ws_sel_snp_base(int remove_mono, double maf, double missrate,
                           int32_t *n_excluded, uint8_t *sel_out);
/* gnrSelSNP_Base_Ex(afreq, remove_mono, maf, missrate), src/SNPRelate.cpp:215-239 ->
 * CdBaseWorkSpace::Select_SNP_Base_Ex, src/dGenGWAS.cpp:399-469: as above, but the monomorphic / MAF tests use the
 * caller's allele frequencies afreq [n_snp of the current selection] (non-finite = excluded) */
int snpgpu_ws_sel_snp_base_ex(const double *afreq, int remove_mono, double maf, double missrate,
                              int32_t *n_excluded, uint8_t *sel_out);
/* gnrGetGenoDim(), src/SNPRelate.cpp:158-181: {n_snp, n_samp} after selection */
int snpgpu_ws_get_geno_dim(int64_t *n_snp, int64_t *n_samp);
/* per-SNP allele frequency / missing rate over the working space
 * (Get_AF_MR_perSNP, src/dGenGWAS.cpp:472-552); any pointer may be NULL */
int snpgpu_ws_snp_rate_freq(double *af, double *maf, double *missrate);
int snpgpu_ws_clear(void);

/* gnrIBSNum(NumThread, Verbose), src/genIBS.cpp:500-550 */
int snpgpu_gnrIBSNum(int num_thread, int verbose, int32_t *ibs0, int32_t *ibs1, int32_t *ibs2);
/* gnrIBSAve(NumThread, useMatrix, Verbose), src/genIBS.cpp:441-497 */
int snpgpu_gnrIBSAve(int num_thread, int use_matrix, int verbose, double *out);
/* gnrIBD_KING_Robust(FamilyID, NumThread, useMatrix, Verbose), src/genKING.cpp:576-679 */
int snpgpu_gnrIBD_KING_Robust(const int32_t *family, int num_thread, int use_matrix, int verbose,
                              double *ibs0, double *kinship);
/* gnrIBD_KING_Homo(NumThread, useMatrix, Verbose), src/genKING.cpp:493-570 */
int snpgpu_gnrIBD_KING_Homo(int num_thread, int use_matrix, int verbose, double *k0, double *k1);
/* gnrDiss(NumThread, Verbose), src/genIBS.cpp:652-683: out = the full n x n matrix */
int snpgpu_gnrDiss(int num_thread, int verbose, double *out);
/* gnrGRM(NumThread, Method, GDS, useMatrix, Verbose), src/genPCA.cpp:1614-1717;
 * methods on this path: "GCTA", "Eigenstrat", "Corr", "EIGMIX", "IndivBeta" */
int snpgpu_gnrGRM(int num_thread, const char *method, int use_matrix, int verbose, double *out);
/* gnrGRMMerge(OutGDS, GDSList, Cmd, Weight, Verbose), src/genPCA.cpp:1721-1853 (caller R/IBD.R:624-741):
 * weighted combination of n_grm GRMs of the same N samples.  grm[k]: host, N x N doubles (symmetric; the rows the
 * kept GDS reader delivers).  cmd = the second element of the files' "command" node; ":method = IndivBeta" selects
 * the beta merge (back-transform with avg_val[k], re-baseline to the new minimum, :1744-1833), anything else the plain
 * weighted sum (:1835-1851).  out: host, N x N.  After a beta merge snpgpu_gnrGRM_avg_val returns the merged
 * average, as the reference's gnrGRM_avg_val does. */
int snpgpu_gnrGRMMerge(int n_grm, int64_t N, const double *const *grm, const char *cmd, const double *avg_val,
                       const double *weight, double *out, int device);
/* of the last snpgpu_gnrGRMMerge on this thread that passed its argument checks: stats[0] row slabs copied to the device (every
 * input travels in slabs of the staging budget, once for the weighted sum and twice for the beta merge), [1] kernels launched */
int snpgpu_grm_merge_stats(double *stats);
/* gnrIBD_PLINK(NumThread, AlleleFreq, UseSpecificAFreq, KinshipConstrict, useMatrix, Verbose),
 * src/genIBS.cpp:558-639.  allele_freq may be NULL (then the allele-count correction is used);
 * afreq_out: double [n_snp] */
int snpgpu_gnrIBD_PLINK(int num_thread, const double *allele_freq, int kinship_constraint, int use_matrix,
                        int verbose, double *k0, double *k1, double *afreq_out);
/* Related pairs of the working space without any n x n matrix: accumulate once (as snpgpu_gnrIBD_KING_Robust / _KING_Homo / _PLINK
 * do, `what` = snpgpu_sel_kind; MOM: the expectations of snpgpu_gnrIBD_PLINK from allele_freq or, NULL, the allele counts), select with
 * snpgpu_select_pairs, keep the selection in the working space until the next call or snpgpu_ws_clear.  Equals snpgdsIBDSelection
 * (R/IBD.R:463-531) of the corresponding snpgdsIBDKING / snpgdsIBDMoM result; the route itself has no reference counterpart.
 * samp_sel: host uint8 [n_samp] or NULL. */
int snpgpu_gnrIBDPairs(int what, const int32_t *family, const double *allele_freq, int kinship_constraint, double kinship_cutoff,
                       const uint8_t *samp_sel, int num_thread, int verbose, int64_t *n_found);
/* the kept selection: host arrays of n_found elements each, any may be NULL (v1 is 0 for KING_ROBUST) */
int snpgpu_gnrIBDPairs_get(int32_t *idx1, int32_t *idx2, double *v0, double *v1, double *kinship);
/* The sparse GRM of the working space without the n x n matrix: accumulate once as snpgpu_gnrGRM does (method "GCTA", "Eigenstrat",
 * "EIGMIX", "IndivBeta"; "Corr" is refused, see snpgpu_select_grm), select with snpgpu_select_grm, keep the result in the working
 * space until the next call or snpgpu_ws_clear.  samp_sel: host uint8 [n_samp] or NULL.  No reference counterpart. */
int snpgpu_gnrGRMPairs(const char *method, double cutoff, const uint8_t *samp_sel, int num_thread, int verbose, int64_t *n_found);
/* the kept result: idx1, idx2, value of n_found elements, diag of n_samp, avg_val (IndivBeta; 0 otherwise); any may be NULL */
int snpgpu_gnrGRMPairs_get(int32_t *idx1, int32_t *idx2, double *value, double *diag, double *avg_val);
/* gnrIBD_Beta(Inbreeding, NumThread, useMatrix, Verbose), src/genBeta.cpp:361-460 */
int snpgpu_gnrIBD_Beta(int inbreeding, int num_thread, int use_matrix, int verbose, double *out, double *avg_val);
/* gnrGRM_avg_val(), src/genPCA.cpp:1605-1611 */
int snpgpu_gnrGRM_avg_val(double *avg_val);
/* gnrEigMix(EigenCnt, NumThread, ParamList{diagadj, ibdmat}, Verbose), src/genEIGMIX.cpp:656-740.
 * ibd (n x n), eigval [n] (NaN beyond eigen_cnt), eigvec (n x eigen_cnt), afreq [n_snp]: any may be NULL */
int snpgpu_gnrEigMix(int eigen_cnt, int num_thread, int diagadj, int verbose, double *ibd, double *eigval,
                     double *eigvec, double *afreq);
/* gnrPCA(EigenCnt, "exact", NumThread, ParamList, Verbose), src/genPCA.cpp:1355-1452.
 * genmat (n x n) may be NULL; eigval: double [n] (entries >= eigen_cnt are NaN as in
 * CalcEigen :1343-1345), eigvec: n x eigen_cnt; both may be NULL (genmat.only). */
int snpgpu_gnrPCA(int eigen_cnt, int num_thread, int bayesian, int verbose, double *trace_xtx,
                  double *genmat, double *eigval, double *eigvec, double *trace_val);

/* gnrPCA(EigenCnt, "randomized", NumThread, ParamList{aux.dim, iter.num, aux.mat}, Verbose): CRandomPCA::Run,
 * src/genPCA.cpp:472-803.  aux_mat = aux_dim x n_samp as R's rnorm(aux.dim * n.samp) is read ([aux_dim][n_samp]).
 * Returns what R/PCA.R:80-89 uses of the routine's list: sigma [n_samp] (zero beyond min(hsize, n_samp),
 * hsize = aux_dim * (iter_num + 1)), the first eigen_cnt rows of V^T as eigvec (n_samp x eigen_cnt
 * column-major) and trace2 = 2 * TraceXTX. */
int snpgpu_gnrPCA_randomized(int eigen_cnt, int aux_dim, int iter_num, const double *aux_mat, int num_thread,
                             int verbose, double *sigma, double *eigvec, double *trace2);
/* gnrPCACorr(LenEig, EigenVect, NumThread, GDSNode=NULL, Verbose), src/genPCA.cpp:1455-1484:
 * out = LenEig x n_snp column-major */
int snpgpu_gnrPCACorr(int len_eig, const double *eigvec, int num_thread, int verbose, double *out);
/* gnrPCASNPLoading(EigenVal, EigenVect, TraceXTX, NumThread, Bayesian, Verbose), src/genPCA.cpp:1488-1531:
 * eigvec = n_samp x len_eig; loading = len_eig x n_snp, afreq / scale = [n_snp] */
int snpgpu_gnrPCASNPLoading(const double *eigval, const double *eigvec, int len_eig, double trace_xtx,
                            int num_thread, int bayesian, int verbose, double *loading, double *afreq, double *scale);
/* gnrPCASampLoading(EigenCnt, SNPLoadings, AvgFreq, Scale, NumThread, Verbose), src/genPCA.cpp:1535-1562:
 * snp_loadings = eigen_cnt x n_snp; out = n_samp x eigen_cnt */
int snpgpu_gnrPCASampLoading(int eigen_cnt, const double *snp_loadings, const double *avg_freq, const double *scale,
                             int num_thread, int verbose, double *out);

/* gnrEigMixSNPLoading(EigenVal, EigenVect, AFreq, NumThread, Verbose), src/genEIGMIX.cpp:739-775:
 * loading = len_eig x n_snp */
int snpgpu_gnrEigMixSNPLoading(const double *eigval, const double *eigvec, int len_eig, const double *afreq,
                               int num_thread, int verbose, double *loading);
/* gnrEigMixSampLoading(SNPLoadings, AFreq, NumThread, Verbose), src/genEIGMIX.cpp:777-803: out = n_samp x eigen_cnt */
int snpgpu_gnrEigMixSampLoading(int eigen_cnt, const double *snp_loadings, const double *afreq, int num_thread,
                                int verbose, double *out);

/* ---- (1d) linkage disequilibrium between SNP pairs: snpgdsLDMat ------------------------------------------------------------
 * Every method is a function of the pair's 3 x 3 genotype table n_ab (samples with genotype a at the first SNP and b at the
 * second, over the samples called at both), counted exactly on the matrix cores and finalised in fp64 with the reference's
 * formulas and NaN rules (src/genLD.cpp:177-525).  Output layout of gnrLDMat (src/genLD.cpp:957-1010), column-major:
 *   slide <= 0 : the full n_snp x n_snp symmetric matrix, diagonal included;
 *   slide  > 0 : clamped to n_snp; column i holds LD(i, i + k) in row k - 1, k = 1 ... slide: slide x n_snp with NaN past the last
 *                SNP, or with mat_trim slide x (n_snp - slide).
 * Streaming as for the accumulators: SNP blocks of any size in file order.  The sliding-window form keeps the last `slide` rows of
 * a block as the halo of the next one (device memory: one block plus its halo); the full form keeps the n_snp packed rows
 * resident and works through the matrix by row panels. */
typedef struct snpgpu_ld snpgpu_ld;
enum snpgpu_ld_method { SNPGPU_LD_COMPOSITE = 1, SNPGPU_LD_R = 2, SNPGPU_LD_DPRIME = 3,
                        SNPGPU_LD_CORR = 4, SNPGPU_LD_COV = 5 };   /* gnrLDMat's `method` codes */
/* opts: device, stream and max_block_snps (SNPs per internal block of the sliding-window form; 0 = 16384) are used */
int snpgpu_ld_create(int64_t n_samp, int64_t n_snp, int method, int64_t slide, int mat_trim, const snpgpu_opts *opts,
                     snpgpu_ld **out);
int snpgpu_ld_destroy(snpgpu_ld *ld);
/* R's nrow / ncol of the result */
int snpgpu_ld_out_dims(const snpgpu_ld *ld, int64_t *rows, int64_t *cols);
/* the next n_snp SNPs (rows of `format`, in `mem`: host or the device's memory).  SNPGPU_DEVICE: the block must be complete when
 * the call is made (the object's stream is not ordered after the caller's; e.g. synchronise the writing stream first).  Either way
 * the call returns when the block has been read, so the caller may reuse or free it at once. */
int snpgpu_ld_feed(snpgpu_ld *ld, const void *geno, int64_t n_snp, int format, int mem);
/* after all n_snp SNPs were fed: the rows x cols matrix, column-major, into host or device memory */
int snpgpu_ld_result(snpgpu_ld *ld, double *out, int out_mem);
/* HIP-event timing on the object's stream: which = 0 table (count) kernel, 1 finaliser, 2 copies of finished values from the
 * device to the result (host memory of the object, or the caller's buffer); summed ms and operations since enabled */
int snpgpu_ld_set_timing(snpgpu_ld *ld, int enable);
int snpgpu_ld_get_timing(snpgpu_ld *ld, int which, double *ms_sum, int64_t *launches);
/* every pair of two row sets -> int32 tab[n_a][n_b][9], cell 3 a + b (a: genotype in set A, b: in set B); host in, host out.
 * Any pair set, e.g. the reference tables of the pruning tests (snpgpu_ld_prune itself counts its band with the sliding-window
 * launches). */
int snpgpu_ld_pair_tables(const void *geno_a, int64_t n_a, const void *geno_b, int64_t n_b, int64_t n_samp, int format,
                          int32_t *tab, int device);
/* gnrLDMat(method, NumSlide, MatTrim, NumThread, Verbose), src/genLD.cpp:957-1010, on the working space's selected SNPs;
 * out: host, snpgpu_ld_out_dims' rows x cols */
int snpgpu_gnrLDMat(int method, int64_t slide, int mat_trim, int num_thread, int verbose, double *out);

/* LD pruning of one chromosome: Perform_LD_Pruning (src/genLD.cpp:807-924), the greedy forward pass from start_idx and the
 * backward pass below it, with the reference's sliding-window list (an entry outside the window of the candidate is erased for
 * good) and test |LD(kept, candidate)| > ld_threshold (the kept SNP is the first argument; NaN never prunes).  Erasure depends on
 * the positions only, so the pairs the scan can test lie within a band of width W that the host computes from pos_bp and the two
 * limits; their tables are counted on the matrix cores in streamed row blocks (one block plus a halo of W rows resident, table
 * launches within a fixed byte budget), the finaliser turns each into one threshold bit with the LD methods of snpgdsLDMat, and
 * the sequential scan runs on the host over those bits.
 *   geno: SNPGPU_GENO_PACKED2 or SNPGPU_GENO_U8 rows [n_snp] in `mem` (host, or complete device memory as for snpgpu_ld_feed)
 *   start_idx: 0-based; pos_bp: host int32 [n_snp]; slide_max_bp / slide_max_n: the reference's int window limits (differences of
 *   positions are taken exactly in 64 bits); method 1 ... 4 (composite, r, dprime, corr); keep: host uint8 [n_snp], 1 = kept
 *   opts: device, stream and max_block_snps (rows per streamed block, 0 = 16384; small values force several blocks) are used
 *   info: may be NULL.  n_samp < 2^24. */
typedef struct snpgpu_ld_prune_info {
    int64_t width;          /* W: largest distance y - x of a pair (x, y) the scan can test                                    */
    int64_t band_pairs;     /* pairs (x, x + k), k = 1 ... W, x + k < n_snp: tables counted and finalised                        */
    int64_t n_kept;         /* SNPs kept                                                                                         */
    int64_t table_launches; /* band table launches (each followed by one finaliser launch and one copy)                          */
    int64_t table_tiles;    /* 64 x 64 pair tiles those launches computed                                                        */
    double ms_stage;        /* HIP events: rows into the staging layout (host -> device copies, staging kernel, halo copies)     */
    double ms_tables;       /*   band table kernel                                                                               */
    double ms_bits;         /*   threshold-bit finaliser                                                                         */
    double ms_copy;         /*   bit rows device -> host                                                                         */
    double ms_scan;         /* host clock: window, band width and the scan                                                      */
} snpgpu_ld_prune_info;
int snpgpu_ld_prune(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int64_t start_idx, const int32_t *pos_bp,
                    int32_t slide_max_bp, int32_t slide_max_n, double ld_threshold, int method, uint8_t *keep,
                    const snpgpu_opts *opts, snpgpu_ld_prune_info *info);
/* The threshold bits snpgpu_ld_prune scans, for a band of the given width (diagnostics and tests): bits host uint64
 * [n_snp][ceil(width / 64)], bit (k - 1) % 64 of word (k - 1) / 64 of row x = |LD(x, x + k)| > ld_threshold for x >= start_idx and
 * |LD(x + k, x)| > ld_threshold for x < start_idx; 0 past the last SNP.  info as above (n_kept 0, ms_scan 0). */
int snpgpu_ld_prune_bits(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int64_t start_idx, int64_t width,
                         double ld_threshold, int method, uint64_t *bits, const snpgpu_opts *opts, snpgpu_ld_prune_info *info);
/* gnrLDpruning(StartIdx, pos_bp, slide_max_bp, slide_max_n, LD_threshold, method, NumThread, verbose), src/genLD.cpp:1014-1035,
 * on the working space's selected SNPs; start_idx 0-based (the routine's StartIdx - 1), pos_bp [n selected], keep: host uint8 */
int snpgpu_gnrLDpruning(int64_t start_idx, const int32_t *pos_bp, int32_t slide_max_bp, int32_t slide_max_n, double ld_threshold,
                        int method, int num_thread, int verbose, uint8_t *keep);

/* LD scores of one chromosome: score[i] = sum over the window partners j of i of the squared LD value of the pair.  The SNPs
 * are in file order with non-decreasing positions.  Pair (i, j), i != j, is in the window iff |i - j| <= slide_max_n and
 * |pos[i] - pos[j]| <= slide_max_bp (differences exact in 64 bits; pos_bp NULL: the SNP count alone decides); the partners of i
 * are then one range [lo, hi], and slide_max_n <= 0 or slide_max_bp < 0 leaves no pair.  Each unordered pair is evaluated once
 * with the lower index as the first SNP (the orientation of snpgdsLDMat's band): v = the LD value of `method` (1 ... 4: composite,
 * r, dprime, corr), t = v * v, and with SNPGPU_LDSCORE_ADJUST t = t - (1 - t) / (n - 2), n = the samples called at both SNPs.
 * The pair is valid iff v is not NaN and, when adjusting, n > 2.  score[i] starts at 1.0 with SNPGPU_LDSCORE_SELF, else 0.0, and
 * adds t of the valid partners lo ... hi in ascending order, one left fold in fp64 without contraction: a plain loop over
 * snpgdsLDMat's values gives the same bits, whatever max_block_snps.  The tables are counted as for snpgpu_ld_prune (streamed row
 * blocks, one block plus a halo of W = max (hi - i) rows resident); the terms and the fold run on the device, and only the
 * three result vectors come back.
 *   geno: SNPGPU_GENO_PACKED2 or SNPGPU_GENO_U8 rows [n_snp] in `mem` (host, or complete device memory as for snpgpu_ld_feed)
 *   score: host double [n_snp]; n_valid (valid partners) and n_window (hi - lo, partners in the window): host int32 [n_snp] or NULL
 *   opts: device, stream and max_block_snps (rows per streamed block, 0 = 16384) are used; info: may be NULL.  n_samp < 2^24.
 * NULL geno / score, a method outside 1 ... 4, unknown flag bits and decreasing positions are refused before any device call. */
typedef struct snpgpu_ld_score_info {
    int64_t width;          /* W: largest distance hi - i of a pair in a window                                                  */
    int64_t band_pairs;     /* pairs (x, x + k), k = 1 ... W, x + k < n_snp: tables counted                                      */
    int64_t window_pairs;   /* unordered pairs inside a window: evaluated                                                        */
    int64_t valid_pairs;    /* of those, valid ones (counted by the terms kernel)                                                */
    int64_t table_launches; /* band table launches (each followed by one terms and one fold launch)                              */
    int64_t table_tiles;    /* 64 x 64 pair tiles those launches computed                                                        */
    double ms_stage;        /* HIP events: rows into the staging layout, halo copies, window upload                              */
    double ms_tables;       /*   band table kernel                                                                               */
    double ms_values;       /*   terms kernel                                                                                    */
    double ms_fold;         /*   fold kernel                                                                                     */
    double ms_copy;         /*   results device -> host                                                                          */
} snpgpu_ld_score_info;
enum { SNPGPU_LDSCORE_ADJUST = 1, SNPGPU_LDSCORE_SELF = 2 };
int snpgpu_ld_score(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pos_bp,
                    int32_t slide_max_bp, int32_t slide_max_n, int method, int flags,
                    double *score, int32_t *n_valid, int32_t *n_window,
                    const snpgpu_opts *opts, snpgpu_ld_score_info *info);
/* snpgpu_ld_score on the working space's selected SNPs (one chromosome, as the caller sets them): the entry an R wrapper calls */
int snpgpu_gnrLDScore(const int32_t *pos_bp, int32_t slide_max_bp, int32_t slide_max_n, int method, int flags, int num_thread,
                      int verbose, double *score, int32_t *n_valid, int32_t *n_window);

/* ---- (1e) IBD by maximum likelihood: snpgdsIBDMLE (method "EM") and snpgdsIBDMLELogLik -----------------------------------------
 * gnrIBD_MLE (src/genIBD.cpp:1465-1548) on resident rows: allele frequencies as InitAFreq (:1122-1165; allele_freq: host
 * [n_snp] or NULL = sum / 2n over the calls, non-finite -> -1), start values from the IBS counters and Est_PLINK_Kinship with
 * the plain-monomial E[IBS | IBD] of Init_EPrIBD_IBS(afreq, NULL, false) and no constraint (:823), clamped to >= 0.005
 * (:824-832), then EMAlg (:582-656) per pair with max_niter / reltol, and LOGLIK_ADJUST's six candidates when coeff_correct.
 * geno: SNPGPU_GENO_PACKED2 rows [n_snp][ceil(n_samp/4)] in `mem` (host or the device's memory).  Outputs in out_mem: full
 * n_samp x n_samp k0, k1 and (may be NULL) int32 niter, 0 on the diagonal; afreq_out: host [n_snp] (may be NULL), -1 where
 * InitAFreq gives -1.  row_begin / row_end: the pairs (i, j > i) with row_begin <= i < row_end, their mirrors and the diagonal
 * entries (i, i) of those rows only (0, 0 = the whole matrix); other entries are left as they were.  n_samp < 2 or n_snp < 1
 * is an error. */
int snpgpu_ibd_mle(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                   int max_niter, double reltol, int coeff_correct, int64_t row_begin, int64_t row_end, double *k0, double *k1,
                   int32_t *niter, double *afreq_out, int out_mem, int device);
/* Do_MLE_LogLik / Do_MLE_LogLik_k01 (src/genIBD.cpp:1289-1330): EM_LogLik of every pair i <= j (diagonal included) at (k0, k1)
 * taken from the n x n matrices k0 / k1 (in out_mem), or at the global (k0_all, k1_all) when both are NULL; out: n x n, out_mem */
int snpgpu_ibd_loglik(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                      const double *k0, const double *k1, double k0_all, double k1_all, double *out, double *afreq_out,
                      int out_mem, int device);
/* of the last snpgpu_ibd_mle on this thread: stats[0] EM kernel ms, [1] ms of all its kernels (EM, candidates, output),
 * [2] lane-sweeps that advanced a pair, [3] lane-sweeps issued (HIP events; counts from the kernel) */
int snpgpu_ibd_mle_stats(double *stats);
/* gnrIBD_MLE(AlleleFreq, KinshipConstraint, MaxIterCnt, RelTol, CoeffCorrect, method, IfOutNum, NumThread, Verbose) on the
 * working space's selected SNPs.  method 0 (EM) only: 1 (downhill simplex) and 2 (Jacquard) return an error.  kinship_constraint
 * is accepted and has no effect, as in the reference.  k0, k1: host n x n; afreq: host [n_snp] (may be NULL); niter: host n x n
 * int32, written when out_num_iter != 0 */
int snpgpu_gnrIBD_MLE(const double *allele_freq, int kinship_constraint, int max_niter, double reltol, int coeff_correct,
                      int method, int out_num_iter, int num_thread, int verbose, double *k0, double *k1, double *afreq,
                      int32_t *niter);
/* The same estimates for a LIST of pairs (snpgdsIBDMLEPairs, snpgdsPairIBD): no n x n object is built, only the distinct listed
 * samples are transposed, and one wave per pair runs the IBS counts, Est_PLINK_Kinship (kinship_constraint is its last argument),
 * the 0.005 clamp, EMAlg and LOGLIK_ADJUST.  idx1 / idx2: host [n_pairs], 0-based samples in any order, repeats and idx1 == idx2
 * allowed; an index outside 0 ... n_samp - 1 or n_pairs < 1 is an error.  Frequencies come from all n_samp rows, or from
 * allele_freq.  mode 0: EM; mode 1: the start values only (the method of moments, before the clamp), loglik NaN, niter 0;
 * mode 2: the downhill simplex (Simplex / SimplexMin<double, 2> / NM_LogLik, src/genIBD.cpp:60-189, :661-779) from the same
 * clamped start values, niter = the routine's count of function evaluations (nfunk, 2 when it stops at once), coefficients NaN
 * and loglik 0 for a pair without a shared call; any other mode is an error that names it.
 * Outputs in out_mem, [n_pairs]: k0, k1, loglik (the log-likelihood of the returned coefficients, after LOGLIK_ADJUST; may be NULL),
 * int32 niter (may be NULL); afreq_out as in snpgpu_ibd_mle.  A pair's result depends on its two samples only: listed twice, or in
 * a second call, it has the same bits. */
int snpgpu_ibd_mle_pairs(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                         const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int mode, int kinship_constraint, int max_niter,
                         double reltol, int coeff_correct, double *k0, double *k1, double *loglik, int32_t *niter,
                         double *afreq_out, int out_mem, int device);
/* Jacquard's nine condensed coefficients of the listed pairs (snpgdsIBDMLEPairs, method "Jacquard"): PrIBDTabJacq + EM_Jacq_Alg
 * (src/genIBD.cpp:864-1072) per pair from D1 ... D8 = 0.01, with EMAlg's stop rule (max_niter, reltol).  There are no IBS counts and
 * no coeff_correct in this method.  The table is not symmetric in the two samples: (idx2, idx1) exchanges D3 with D5 and D4 with D6.
 * As in the reference, an SNP at which BOTH samples are MM (code 2) enters nothing: its `case 2` / `case 2` entry has no `break`
 * and falls through to `default`, which zeroes all nine probabilities, and the EM skips such SNPs.  That quirk is reproduced.
 * d: eight planes [8][n_pairs] (D1 ... D8; D9 = 1 - their sum), required; loglik, niter and afreq_out may be NULL.  Inputs, index
 * checks and out_mem as snpgpu_ibd_mle_pairs. */
int snpgpu_ibd_jacquard_pairs(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq,
                              const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int max_niter, double reltol, double *d,
                              double *loglik, int32_t *niter, double *afreq_out, int out_mem, int device);
/* of the last snpgpu_ibd_mle_pairs or snpgpu_ibd_jacquard_pairs on this thread: stats[0] ms of its one-wave-per-pair kernel, [1] ms
 * of all its kernels, [2] wave-sweeps (sweeps of one pair's SNPs by one wave: EM iterations, candidate sweeps, function-evaluation
 * sweeps of the simplex), [3] pairs */
int snpgpu_ibd_mle_pairs_stats(double *stats);
/* snpgpu_ibd_mle_pairs (mode 0, no constraint) on the working space's selected SNPs and samples; idx1 / idx2 index the selected
 * samples.  Host outputs [n_pairs]; loglik, niter and afreq may be NULL */
int snpgpu_gnrIBD_MLE_Pairs(const double *allele_freq, const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int max_niter,
                            double reltol, int coeff_correct, int num_thread, int verbose, double *k0, double *k1, double *loglik,
                            int32_t *niter, double *afreq);
/* The listed pairs by `method` on the working space: 0 EM (as snpgpu_gnrIBD_MLE_Pairs), 1 downhill simplex (coef: host
 * [2][n_pairs], k0 then k1), 2 Jacquard (coef: host [8][n_pairs], D1 ... D8; coeff_correct has no effect); any other method is an
 * error.  loglik, niter and afreq may be NULL */
int snpgpu_gnrIBD_MLE_PairsMethod(const double *allele_freq, const int32_t *idx1, const int32_t *idx2, int64_t n_pairs, int method,
                                  int max_niter, double reltol, int coeff_correct, int num_thread, int verbose, double *coef,
                                  double *loglik, int32_t *niter, double *afreq);
/* gnrIBD_LogLik(AFreq, k0, k1) / gnrIBD_LogLik_k01(AFreq, k0, k1): out host n x n; afreq may be NULL (estimated) */
int snpgpu_gnrIBD_LogLik(const double *afreq, const double *k0, const double *k1, double *out);
int snpgpu_gnrIBD_LogLik_k01(const double *afreq, double k0, double k1, double *out);

/* ---- (1f) population statistics: snpgdsFst and the Fst scan of snpgdsSlidingWindow ---------------------------------------------
 * Everything gnrFst (src/genFst.cpp:170-242) needs from a SNP is 2 K integers: per population the allele count ACnt (sum of the
 * called genotypes) and Cnt (2 x called samples) of WC84 / WH02 (:56-74, :103-120).  One pass over the 2-bit rows produces them
 * exactly (integer arithmetic: bit-identical whatever the reduction order); the rest is fp64 on the counters, with the reference's
 * operation order inside a SNP and sums over SNPs taken sequentially in ascending order.  A SNP where a population has no called
 * sample has a NaN ratio and enters no sum.  (n_c of W&C84 sums Cnt^2 exactly; the reference's int product overflows beyond
 * 23 170 called samples in a population.)
 *   geno   rows [n_snp] of `format` (SNPGPU_GENO_PACKED2 rows are read where they lie, padding codes of the last byte ignored;
 *          SNPGPU_GENO_U8 goes through the repack) in `mem`: host, or complete device memory of `device`.  2-bit rows in device
 *          memory are counted by one launch; host rows and one-byte genotypes are streamed through a staging buffer in SNP blocks;
 *          the counters of all n_snp SNPs stay on the device (8 K bytes per SNP)
 *   pop    host int32 [n_samp], 0-based population index; n_pop = K >= 2, every population with at least one sample
 *   method SNPGPU_FST_WC84 (Weir & Cockerham 1984) or SNPGPU_FST_WH02 (Weir & Hill 2002)
 * Argument errors (n_pop < 2, an index outside [0, K), an empty population, an unknown method, an unsorted or out-of-range
 * window list) are refused before any device is touched. */
enum snpgpu_fst_method { SNPGPU_FST_WC84 = 1, SNPGPU_FST_WH02 = 2 };
/* acnt / cnt: int32 [n_snp][n_pop] in out_mem */
int snpgpu_pop_counts(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop,
                      int32_t *acnt, int32_t *cnt, int out_mem, int device);
/* gnrFst: fst = the ratio of sums (W&C84) / 1 - H_W / H_B of the summed H (W&H02); fst_snp: host [n_snp] or NULL, the per-SNP
 * ratios; beta: host [n_pop][n_pop] or NULL, W&H02 only (symmetric) */
int snpgpu_fst(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop, int method,
               double *fst, double *fst_snp, double *beta, int device);
/* the same for n_win SNP sets in CSR form (host): window w = snp_index[offsets[w] ... offsets[w + 1]), 0-based rows of geno in
 * ascending order; offsets[0] = 0.  fst_win: host [n_win] (NaN for an empty window); beta_win: host [n_win][n_pop][n_pop] or
 * NULL; fst_snp as above.  The genotypes are read once however the windows overlap. */
int snpgpu_fst_windows(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *pop, int n_pop, int method,
                       const int64_t *offsets, const int32_t *snp_index, int64_t n_win, double *fst_win, double *beta_win,
                       double *fst_snp, int device);
/* of the last call above on this thread: stats[0] ms of the counter kernel (HIP events, summed over the blocks), [1] its launches,
 * [2] ms from the first to the last Fst kernel (per-SNP terms, window sums; the device-to-host copies of the window results that
 * lie between the launches of a W&H02 scan included), [3] genotype bytes the counter kernel read, [4] launches of the W&H02 window
 * sums (each takes as many windows as its buffer of K x K sums holds; 0 for W&C84 and for snpgpu_pop_counts).  stats: 5 doubles */
int snpgpu_pop_stats(double *stats);
/* gnrFst(Pop, nPop, Method) on the working space's selected SNPs: pop 1-based as R passes a factor, method "W&C84" / "W&H02" */
int snpgpu_gnrFst(const int32_t *pop, int n_pop, const char *method, double *fst, double *fst_snp, double *beta);
/* the Fst case (FunIdx 1) of gnrSlidingWindow(FUNIdx, WinSize, Shift, Unit, WinStart, AsIs, chflag, ChrPos, Param, Verbose): the
 * windows of one chromosome in CSR form over the working space's selected SNPs (the host computes the membership) */
int snpgpu_gnrSlidingWindowFst(const int32_t *pop, int n_pop, const char *method, const int64_t *offsets, const int32_t *snp_index,
                               int64_t n_win, double *fst_win, double *beta_win, double *fst_snp);

/* ---- (1g) quality-control statistics: snpgdsSampMissRate, snpgdsHWE, snpgdsIndInb ------------------------------------------------
 * All three come from one pass over the 2-bit rows with a lane per word column of samples: the exact genotype counts of every SNP
 * and the missing calls of every sample (integer atomics: bit-identical whatever the order), and fp64 work on them.
 *   geno   rows [n_snp] of `format` (SNPGPU_GENO_PACKED2 rows are read where they lie, padding codes of the last byte ignored;
 *          SNPGPU_GENO_U8 goes through the repack) in `mem`: host, or complete device memory of `device`.  2-bit rows in device
 *          memory are read by one launch per 1 048 560 SNPs; host rows and one-byte genotypes are streamed through a staging buffer in SNP blocks
 * Argument errors (an unknown method, a non-finite reltol, NULL outputs) are refused before any device is touched. */
/* snp_cnt: int32 [n_snp][3], the samples with g = 0, 1, 2; samp_missing: int32 [n_samp], the SNPs with g > 2; both in out_mem,
 * either may be NULL */
int snpgpu_geno_counts(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, int32_t *snp_cnt,
                       int32_t *samp_missing, int out_mem, int device);
/* gnrHWE (src/genHWE.cpp:46-137): the p-value of the Wigginton-Cutler-Abecasis exact test on (AA = #g==2, AB = #g==1, BB = #g==0)
 * per SNP; NaN for a SNP without a call.  One lane per SNP runs the recurrence from the midpoint down and then up in the
 * reference's operation order (terms and normalising sum bit-identical to it) and a second time for the p-value, which adds
 * term / sum over the terms not greater than the observed one in that generation order (the reference adds them in ascending index
 * order: the two differ by the order of a sum of at most rare_copies / 2 + 1 non-negative terms).  SNPs are assigned to lanes in
 * descending order of rare_copies (sorted on the host from the counters), so the lanes of a wave finish together.  The product
 * rare_copies x (2 genotypes - rare_copies) is taken in 64 bits (the reference's int overflows beyond 32 767 samples).
 * pvalue: host [n_snp] */
int snpgpu_hwe(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, double *pvalue, int device);
/* the test on given counts: snp_cnt int32 [n_snp][3] (g = 0, 1, 2) and pvalue [n_snp] both in `mem` */
int snpgpu_hwe_counts(const int32_t *snp_cnt, int64_t n_snp, double *pvalue, int mem, int device);
/* gnrIndInb (src/genIBD.cpp:1847-2006).  allele_freq: host [n_snp] or NULL = estimated from the counters (the moment methods:
 * calc_afreq's sum / num * 0.5; SNPGPU_INB_MLE: GetAlleleFreqs' sum / (2 num); NaN for a SNP without a call).
 * Moment methods: per SNP a table of the three values a genotype adds (fp64, the reference's operations in its order, no FMA
 * contraction) and one lane per sample that walks the SNPs in ascending order, sums carried across streamed blocks: the result is
 * the reference's sequential sum bit for bit.  Non-finite values add nothing and do not count; mom.weir adds numerator and
 * 2 p (1 - p) for every called genotype, so a NaN frequency poisons the samples called there.
 * SNPGPU_INB_MLE (_inb_mle, :1393-1438): rows transposed once to resident sample-major words, one wave per sample, sums over the
 * SNPs reduced in the wave (so compared within a tolerance, not bit for bit); start value _inb_mom_ratio clamped to
 * [0.001, 0.999], a non-finite start is returned as it is with niter -1, a sample that never meets the stop test reports 10 001.
 *   coeff: double [n_samp], niter: int32 [n_samp] or NULL (written for SNPGPU_INB_MLE only), both in out_mem;
 *   afreq_out: host [n_snp] or NULL, the frequencies used */
enum snpgpu_inb_method { SNPGPU_INB_MOM_WEIR = 1, SNPGPU_INB_MOM_VISSCHER = 2, SNPGPU_INB_MLE = 3, SNPGPU_INB_GCTA1 = 4,
                         SNPGPU_INB_GCTA2 = 5, SNPGPU_INB_GCTA3 = 6 /* = mom.visscher */ };
int snpgpu_ind_inb(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const double *allele_freq, int method,
                   double reltol, double *coeff, int32_t *niter, double *afreq_out, int out_mem, int device);
/* of the last call above on this thread (HIP events, summed over the streamed blocks): stats[0] ms of the counter kernel, [1] its
 * launches, [2] genotype bytes it read, [3] ms of the moment kernel (table kernel included), [4] ms of the MLE kernel, [5] its
 * lane-steps that held a genotype word, [6] lane-steps issued (the ratio is the fill of a wave's last 64-word stride: geometry), [7] ms of the HWE kernel */
int snpgpu_qc_stats(double *stats);
/* gnrSampFreq() (src/SNPRelate.cpp:275-283): missing rate per sample over the working space's selected SNPs; out host [n_samp] */
int snpgpu_gnrSampFreq(double *out);
/* gnrHWE(): pvalue host [n selected SNPs] */
int snpgpu_gnrHWE(double *pvalue);
/* gnrIndInb(afreq, method, reltol, num_iter, verbose): method "mom.weir", "mom.visscher", "mle", "gcta1", "gcta2", "gcta3";
 * afreq host [n selected SNPs] or NULL; coeff host [n_samp]; niter host [n_samp], written for "mle" when out_num_iter != 0 */
int snpgpu_gnrIndInb(const double *afreq, const char *method, double reltol, int out_num_iter, int verbose, double *coeff,
                     int32_t *niter);

/* ---- (1h) hierarchical clustering and the permutation test of the tree: snpgdsHCluster, snpgdsCutTree ----------------------------
 * snpgpu_hclust_average is host code and touches no device: R's hclust(as.dist(dist), method = "average") on an n x n matrix with
 * leading dimension ld, of which, like as.dist, only the lower triangle (dist[i * ld + j], i > j) is read.
 *   merge   int32 [n - 1][2], R's convention: singletons negative, earlier rows positive and 1-based, a singleton before a cluster,
 *           two singletons as (-i, -j) with i < j, two clusters with the smaller row number first
 *   height  double [n - 1], the average (Lance-Williams) distance of each merge
 *   order   int32 [n], 1-based: the leaves with the first column of every merge to the left
 * Nearest-neighbour lists: every row keeps its nearest neighbour among the later rows, the globally closest pair is merged into the
 * row of lower index by (m_i d_ik + m_j d_jk) / (m_i + m_j), the rows that pointed at either are scanned again.  Both scans compare
 * with a strict <, so of tied distances the one of lowest index wins.  Refused: n < 2, a non-finite entry in the lower triangle. */
int snpgpu_hclust_average(int64_t n, const double *dist, int64_t ld, int32_t *merge, double *height, int32_t *order);
/* gnrDistPerm (src/SNPRelate.cpp:502-677).  dist: double [n][n] in `mem` (host, or device memory of `device`); merge: host int32
 * [n - 1][2] as above.  For merge m with member list A (the n1 members of the first column, then the n2 of the second), N = n1 + n2,
 * NSub1 = min(n1, n2), NSub2 = N - NSub1: obs = mean of dist[A[i] * n + A[j]] over i < n1 <= j; every permutation re-splits A into
 * NSub1 and NSub2 members and takes the same mean; z = (obs - mean) / sd with sd over n_perm - 1, and z = 0 when n1 = n2 = 1 or
 * whenever sd > 0 is false (NaN included).  group: host int32 [n], the reference's sequential pass over the merges (:628-664).
 * Outputs on the host: z, n1, n2 [n - 1] and group [n] are required; obs, perm_mean, perm_sd [n - 1] may be NULL (perm_mean and
 * perm_sd are NaN for a merge of two singletons).
 * Deliberate differences from the reference, whose Mersenne-Twister stream cannot be followed in parallel:
 *   random stream   Philox4x32-10 keyed by `seed`, counter (draw >> 2, permutation, merge, 0), word draw & 3, u = (x + 0.5) 2^-32
 *   draw rule       the reference's: for i in 0 ... NSub1 - 1 swap slot i with slot i + min(Range - 1, (int)(u (Range - 1) + 0.5)),
 *                   Range = N - i, the product and the sum rounded separately (no fused multiply-add)
 *   start           every permutation starts from the merge's member order rotated by an offset of its own, floor(u N) with u from
 *                   word 0 of the block with counter (2^32 - 1, permutation, merge, 0).  The reference carries the arrangement
 *                   over, which mixes it; started from the plain member order every time, the draw rule (slot i stays, and the
 *                   last slot is drawn, with half the probability of the others) would favour some re-splits of a small cluster
 *                   and shift its z by more than the Monte-Carlo spread
 *   result          a function of (dist, merge, n_perm, seed) alone, bit-identical from run to run: every sum has a fixed order,
 *                   mean and sd are taken over the n_perm values in index order (two passes)
 * The device holds the matrix gathered into leaf order (n^2 doubles), the row sums of every merge (at most n^2 / 2 + n doubles) and
 * the n_perm (n - 1) permutation values; a call the device cannot hold is refused.  Refused before the first HIP call: n < 2,
 * n_perm < 50, a non-finite z_threshold, NULL required arguments, and a merge whose entries are out of range, refer to a row that
 * is not earlier, or use a sample or a row twice. */
int snpgpu_dist_perm(const double *dist, int64_t n, int mem, const int32_t *merge, int n_perm, double z_threshold, uint64_t seed, double *z,
                     int32_t *n1, int32_t *n2, int32_t *group, double *obs, double *perm_mean, double *perm_sd, int device);
/* gnrDistPerm(n, dist, merge, n.perm, z.threshold): merge as R holds it, column-major int [2][n - 1]; everything in host memory */
int snpgpu_gnrDistPerm(int n_dist, const double *dist, const int32_t *merge, int n_perm, double z_threshold, uint64_t seed, double *z,
                       int32_t *n1, int32_t *n2, int32_t *group, int device);
/* of the last snpgpu_dist_perm / snpgpu_gnrDistPerm on this thread (HIP events): stats[0] ms of the gather and row-sum pass, [1] ms
 * of the permutation kernels, [2] launches timed in [0], [3] launches timed in [1], [4] matrix elements the permutations gathered,
 * [5] permutations evaluated */
int snpgpu_tree_stats(double *stats);

/* ---- (1i) genotype scores of listed sample pairs: snpgdsPairScore ------------------------------------------------------------------
 * gnrPairScore (src/genIBS.cpp:690-891): pair j is (idx1[j], idx2[j]), 0-based sample indices in host memory; a sample may be in
 * both lists and may be paired with itself.  A score is map[g1][g2] of the method's 4 x 4 integer map wherever g1 < 3 && g2 < 3;
 * the two *.only maps hold -1 at some such cells, and there -1 is a score like any other (it enters Sum, SqSum and Num and is
 * written to the matrix).  The four *.major / *.minor methods first flip a SNP (every g < 3 becomes 2 - g) when gsum < n, n the
 * number of called genotypes over both lists and gsum their sum, a sample counting once per appearance.
 * The device only counts, whatever the method: per SNP the table of the pairs' codes before any flip, per pair the table of the
 * SNPs' codes after it.  snpgpu_pair_score_final turns a table into (Avg, SD, Num) on the host; all sums are integers, put
 * through CalcAvgSD's fp64 operations (src/dGenGWAS.cpp:2365-2379), so the results are the reference's bit for bit.
 *   geno   as in (1g); 2-bit rows in device memory are read in place, everything else is streamed in SNP blocks
 * Refused before any device is touched: n_pair < 1, an index outside [0, n_samp), an unknown method / kind, NULL outputs. */
enum snpgpu_pair_method { SNPGPU_PS_IBS = 1, SNPGPU_PS_GVH = 2, SNPGPU_PS_HVG = 3, SNPGPU_PS_GVH_MAJOR = 4, SNPGPU_PS_GVH_MINOR = 5,
                          SNPGPU_PS_GVH_MAJOR_ONLY = 6, SNPGPU_PS_GVH_MINOR_ONLY = 7 };
enum snpgpu_pair_table { SNPGPU_PS_PAIR_TABLE = 0, SNPGPU_PS_SNP_TABLE = 1 };
enum snpgpu_pair_elem { SNPGPU_PS_ELEM_INT32 = 0, SNPGPU_PS_ELEM_BIT2 = 1 };
/* pair_tab: int64 [n_pair][9], cell 3 a + b = the SNPs where the pair has codes (a, b), a, b < 3, counted after the flip when
 *           need_major != 0 and as stored otherwise
 * snp_tab:  int32 [n_snp][16], cell 4 a + b = the pairs with codes (a, b), a, b < 4 (3 = missing), as stored
 * flip:     uint8 [n_snp], 1 where gsum < n (computed whatever need_major is)
 * all three in out_mem; any may be NULL, not all */
int snpgpu_pair_tables(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *idx1, const int32_t *idx2,
                       int64_t n_pair, int need_major, int64_t *pair_tab, int32_t *snp_tab, uint8_t *flip, int out_mem, int device);
/* Host code, touches no device.  table: n rows of a pair table (SNPGPU_PS_PAIR_TABLE, counted with need_major as the method needs)
 * or of a SNP table with its flip bytes (SNPGPU_PS_SNP_TABLE; flip may be NULL for IBS / GVH / HVG).  dosage selects the 0 / 1 / 2
 * or the 0 / 1 form of IBS, GVH and HVG and is ignored by the other methods.  out: (Avg, SD, Num) per row, laid out as the R object:
 * pair table n x 3 column-major (out[i], out[n + i], out[2 n + i]), SNP table 3 x n (out[3 i ...]).  Num > 1: Avg = Sum / Num,
 * SD = sqrt((SqSum - Num Avg Avg) / (Num - 1)); Num == 1: Avg = Sum, SD = NaN; Num == 0: both NaN. */
int snpgpu_pair_score_final(int table_kind, const void *table, const uint8_t *flip, int64_t n, int method, int dosage, double *out);
/* The score of every (SNP, pair) after the flip, out_host [n_snp][n_pair] (R's n_pair x n_snp matrix), streamed to the host in SNP
 * blocks: SNPGPU_PS_ELEM_INT32 int32 with INT_MIN (NA_integer_) where a genotype is missing; SNPGPU_PS_ELEM_BIT2 uint8 holding the
 * two bits a bit2 node keeps of the reference's byte: 3 for missing, and 3 for a score of -1 */
int snpgpu_pair_score_matrix(const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const int32_t *idx1,
                             const int32_t *idx2, int64_t n_pair, int method, int dosage, int elem_kind, void *out_host, int device);
/* gnrPairScore(SampIdx1, SampIdx2, Method, Type, Dosage, GDSNode, Verbose) on the working space's selected SNPs.  method "IBS",
 * "GVH", "HVG", "GVH.major", "GVH.minor", "GVH.major.only", "GVH.minor.only"; type and host `out`: "per.pair" double n_pair x 3
 * column-major, "per.snp" double 3 x n_snp, "matrix" int32 n_pair x n_snp column-major, "gds.file" uint8 of the same shape (the
 * bytes appended to the bit2 node) */
int snpgpu_gnrPairScore(const int32_t *idx1, const int32_t *idx2, int64_t n_pair, const char *method, const char *type, int dosage,
                        int verbose, void *out);
/* of the last snpgpu_pair_tables / snpgpu_pair_score_matrix on this thread (HIP events, summed over the streamed blocks): stats[0]
 * ms of the SNP-table kernel, [1] its launches, [2] genotype bytes it read, [3] ms of the transposition to sample-major words (flip
 * masks included), [4] ms of the per-pair counter, [5] ms of the matrix kernel, [6] launches timed in [3] ... [5], [7] genotype bytes
 * the transposition and the matrix kernel read */
int snpgpu_pair_stats(double *stats);

/* ---- (1j) selection and layout of genotypes: sample subsets, snp.order nodes, snpgdsGetGeno ---------------------------------------
 * The selected rectangle of a genotype bit stream as SNPGPU_GENO_PACKED2 rows (gnrCopyGenoMem, src/SNPRelate.cpp:322-382, minus
 * the byte per genotype): dst receives [n_snp_out][ceil(n_samp_out / 4)] bytes, sample samp_index[j] at code j of the row of SNP
 * snp_index[k], the unused codes of a row's last byte 3.  One description covers byte-aligned PACKED2 rows (major 0, stride 8 rb),
 * the raw sample.order node (major 0, stride 2 n_samp: a row starts at any even bit), the raw snp.order node (major 1, stride
 * 2 n_snp), a window of either (pointer advanced, phase in bit0) and host-gathered segments with a phase per row (row_bit). */
typedef struct snpgpu_geno_src {
    const void    *bits;            /* 2 bits per genotype, LSB first, 3 = missing                          */
    int32_t        mem;             /* SNPGPU_HOST / SNPGPU_DEVICE / SNPGPU_HOST_PINNED                      */
    int32_t        major;           /* 0: a row is a SNP, columns are samples; 1: a row is a sample         */
    int64_t        n_rows, n_cols;
    int64_t        bit0;            /* element (r, c) lives at bit  bit0 + r * row_stride_bits + 2 c  ...    */
    int64_t        row_stride_bits;
    const int64_t *row_bit;         /* ... or, if not NULL (host, n_rows entries), at bit row_bit[r] + 2 c   */
    int64_t        n_bytes;         /* extent of `bits`: no byte outside [bits, bits + n_bytes) is needed    */
} snpgpu_geno_src;
/* samp_index / snp_index: host, 0-based positions in the source, NULL = all in order; they may permute and repeat entries.
 * dst in dst_mem (host, pinned host or device memory of `device`); stream: NULL or a stream of `device` (the call returns with the
 * work complete either way).  The kernels load aligned dwords that hold a byte of [bits, bits + n_bytes) and nothing else, and
 * store inside dst's n_snp_out * ceil(n_samp_out / 4) bytes only.  Host sources are staged in windows of whole source rows (a
 * major 1 source larger than the staging size: in windows of SNPs); SNPGPU_SELECT_STAGE_BYTES forces the staging size.
 * Refused before any device is touched: NULL src / bits / dst, an odd or negative bit position or stride, major other than 0 / 1,
 * an index outside the source, an element outside n_bytes, dimensions beyond 2^30 - 1 samples or 2^31 - 1 SNPs, an unknown mem;
 * refused before any launch: a device pointer or a stream that belongs to another device than `device`. */
int snpgpu_geno_select(const snpgpu_geno_src *src, const int32_t *samp_index, int64_t n_samp_out, const int32_t *snp_index,
                       int64_t n_snp_out, void *dst, int dst_mem, int device, void *stream);
/* of the last snpgpu_geno_select on this thread (HIP events, summed over the windows): stats[0] ms of the host-to-device copies of
 * the source, [1] ms of the copy kernel (major 0, consecutive samples), [2] ms of the gather kernel (major 0, a sample list), [3] ms
 * of the transposition kernel (major 1), [4] kernel launches, [5] source bytes brought to the device, [6] ms of the copy of the
 * result to the host, [7] staging windows */
int snpgpu_geno_select_stats(double *stats);

/* ---- (1k) PLINK BED: the other 2-bit code set and the other layout of dst ----------------------------------------------------------
 * snpgpu_geno_select with a code set on either side and a choice of which axis dst packs.  Both code sets hold 2 bits per
 * genotype, 4 per byte, LSB first:
 *   SNPGPU_CODE_GDS  the number of A alleles 0 / 1 / 2, 3 = missing; the unused codes of a row's last byte are 3
 *                    (SNPGPU_GENO_PACKED2, the GDS genotype node)
 *   SNPGPU_CODE_BED  0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; the unused codes of a row's last byte
 *                    are 0 (a PLINK .bed file after its 3-byte header: mode 1 is major 0 with stride 8 ceil(n_samp / 4), mode 0
 *                    is major 1 with stride 8 ceil(n_snp / 4))
 * BED -> GDS is {2, 3, 1, 0} (src/ConvToGDS.cpp:585), GDS -> BED is {3, 2, 0, 1} (src/SNPRelate.cpp:801); equal codes copy.
 * The padding of a source is never read as a genotype; dst's padding is that of dst_code.
 *   dst_major 0  dst is [n_snp_out][ceil(n_samp_out / 4)]: SNP rows, as snpgpu_geno_select (BED mode 1)
 *   dst_major 1  dst is [n_samp_out][ceil(n_snp_out / 4)]: sample rows, sample samp_index[j] in row j, SNP snp_index[k] at
 *                code k (BED mode 0)
 * dst_major 1 runs the same kernels with the two axes and the two index lists exchanged, so the limits follow dst's axes: the
 * axis packed into dst's rows holds at most 2^30 - 1 entries, the row axis 2^31 - 1.  dst_major 0: 2^30 - 1 samples and
 * 2^31 - 1 SNPs, as snpgpu_geno_select; dst_major 1: 2^30 - 1 SNPs, and samples stay at 2^30 - 1 (the description of a source
 * allows no more).  Sources, staging windows, memory kinds, stream and every other refusal are those of snpgpu_geno_select; the
 * staging windows of a host source larger than the staging size are whole source rows when the source's major equals dst_major,
 * windows of dst's rows otherwise.  Also refused before any device is touched: a src_code, dst_code or dst_major that is none of
 * the above.  snpgpu_geno_select is the call (SNPGPU_CODE_GDS, SNPGPU_CODE_GDS, dst_major 0). */
enum { SNPGPU_CODE_GDS = 0, SNPGPU_CODE_BED = 1 };
int snpgpu_geno_convert(const snpgpu_geno_src *src, int src_code, const int32_t *samp_index, int64_t n_samp_out,
                        const int32_t *snp_index, int64_t n_snp_out, void *dst, int dst_major, int dst_code, int dst_mem, int device,
                        void *stream);
/* of the last snpgpu_geno_convert on this thread: the fields of snpgpu_geno_select_stats ([1], [2]: the source's major equals
 * dst_major; [3]: it differs).  The two calls share the record: either one reports the last call of either. */
int snpgpu_geno_convert_stats(double *stats);

/* ---- (1l) VCF text: the genotype columns of data lines as SNPGPU_GENO_PACKED2 rows ----------------------------------------------------
 * What gnrParseVCF4 (src/ConvToGDS.cpp:667-997) does per sample cell, on the device: the file's own bytes go there and 2-bit rows
 * come out, with nothing per cell in between.  The fixed columns (CHROM ... FORMAT) stay with the host: snpgpu_vcf_index finds
 * them, the caller reads them and hands every kept line's allele count and reference allele to snpgpu_vcf_genotypes.
 *
 * snpgpu_vcf_index: the line index of a buffer of data lines (the '#' header is the caller's).  Makes no HIP call.
 *   buf, n_bytes   whole lines; without `final` the buffer ends at its last '\n' and whatever follows is left to the next call:
 *                  *consumed is the offset behind the last complete line.  With `final` a last line without '\n' is a line.
 *   col_begin      [max_lines][10]: the offsets of the starts of columns 1 ... 10 (CHROM ... FORMAT, first sample cell)
 *   line_end       [max_lines]: the end of the line, before its '\n' and before a '\r' in front of that
 *   line_base      lines in front of this buffer: error messages name the 1-based line line_base + i + 1
 * Refused: a line with fewer than 10 columns, an empty line, more than max_lines lines. */
int snpgpu_vcf_index(const char *buf, int64_t n_bytes, int final, int64_t line_base, int64_t max_lines, int64_t *col_begin,
                     int64_t *line_end, int64_t *n_lines, int64_t *consumed);
/* snpgpu_vcf_genotypes: line i's sample cells are the tab-separated pieces of text[cell_begin[i], line_end[i]).
 *   text, text_mem SNPGPU_HOST, SNPGPU_HOST_PINNED (both staged in windows of whole lines) or SNPGPU_DEVICE (any alignment, parsed
 *                  where it lies); only aligned dwords that hold a byte of [text, text + n_bytes) are loaded
 *   num_allele     per line: 1 + the number of ALT alleles; an allele index >= it is flagged
 *   ref_index      per line: the allele that is counted (0 = REF); -1 counts none (every called genotype is 0)
 *   rows           DEVICE memory of `device`: [n_lines][ceil(n_samp / 4)], the unused codes of a row's last byte 3.  A caller that
 *                  wants the rows on the host composes with snpgpu_geno_select (device source, host dst).
 *   line_flags, line_cells   host, n_lines: the flags below and the number of cells found
 * A cell's GT is the cell up to its first ':'.  At every allele position a run of decimal digits is an allele index and '.' a
 * missing allele; everything up to the next '|' or '/' is skipped.  The code is the number of alleles equal to ref_index, at
 * most 2; 3 when any allele is missing; 0 for an empty GT.  Ploidy is whatever the cell holds.
 * The kernel raises nothing: it flags the line, whose row may then hold anything (inside its own bytes), and the caller decides:
 *   1  an allele position starts with a byte that is neither a digit nor '.' (whitespace, a sign, a quote, "/0", "0//0")
 *   2  an allele index >= num_allele
 *   4  an allele index of more than 9 digits
 *   8  line_cells != n_samp, or the last cell is empty; cells beyond n_samp are counted and never stored
 * No device memory grows with n_lines x n_samp but rows; no atomics touch global memory; the result is a pure function of the
 * input.  Refused before any device is touched: NULL pointers, an unknown text_mem, offsets outside n_bytes or cell_begin >
 * line_end, n_samp outside 1 ... 2^30 - 1, n_lines outside 1 ... 2^31 - 1, num_allele < 1, ref_index < -1; before any launch: a
 * device pointer or a stream of another device. */
int snpgpu_vcf_genotypes(const void *text, int text_mem, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end,
                         const int32_t *num_allele, const int32_t *ref_index, int64_t n_lines, int64_t n_samp, void *rows,
                         int32_t *line_flags, int64_t *line_cells, int device, void *stream);
/* of the last snpgpu_vcf_genotypes on this thread: [0] ms of the text's copies to the device, [1] ms of the kernel, [2] launches,
 * [3] text bytes copied (or parsed in place), [4] bytes of a workgroup's chunk, [5] of a lane's segment, [6] of the halo */
int snpgpu_vcf_stats(double *stats);

/* ---- (1m) text out: SNPGPU_GENO_PACKED2 rows as lines of text ---------------------------------------------------------------------------
 * What gnrConvGDS2PED and gnrConvGDS2EIGEN (src/SNPRelate.cpp:685-767, :828-859) do with one `ofstream <<` per genotype, on the
 * device: 2-bit rows go in, the file's own bytes come out.  Every row becomes one line: an optional prefix, one piece per column,
 * '\n'.  Who is a row is the caller's business: a SNP for .eigenstratgeno, a sample for .ped (rows transposed with
 * snpgpu_geno_convert, dst_major = 1, first).
 *   rows           DEVICE memory of `device`: [n_rows][ceil(n_cols / 4)] codes, byte-aligned rows, any alignment of the first
 *   format         the piece of a column with code 0 / 1 / 2 / 3:
 *                    SNPGPU_TEXT_DIGIT        "0" "1" "2" "9"
 *                    SNPGPU_TEXT_PED_AB       "\tB B" "\tA B" "\tA A" "\t0 0"
 *                    SNPGPU_TEXT_PED_12       "\t2 2" "\t1 2" "\t1 1" "\t0 0"
 *                    SNPGPU_TEXT_PED_ALLELE   "\t" s2 " " s2, "\t" s1 " " s2, "\t" s1 " " s1, "\t0 0" with the column's alleles
 *   allele_pool, allele_off   SNPGPU_TEXT_PED_ALLELE only (host): s1, s2 of column c are the bytes [allele_off[2c], allele_off[2c + 1])
 *                  and [allele_off[2c + 1], allele_off[2c + 2]) of the pool; 2 n_cols + 1 offsets, every allele at least one byte
 *                  (the caller writes "0" for an empty one), of any length.  When all are one byte long every line has the same
 *                  length and the fixed-width kernel runs with the pool as its table.
 *   prefix_pool, prefix_off   both NULL, or (host) the bytes [prefix_off[r], prefix_off[r + 1]) copied to the head of line r
 *   text           DEVICE memory of `device`, any alignment, line_off[n_rows] bytes -- or NULL: the call only sizes.  A caller that
 *                  wants the text on the host copies it.
 *   line_off       host, n_rows + 1: line r is text[line_off[r], line_off[r + 1]), line_off[0] = 0
 * Sizing a fixed-width format (all but alleles of several lengths) is arithmetic and touches no device; else a first launch
 * gives every line's length and the second one writes.  The kernels store only inside [text, text + line_off[n_rows]), load only
 * aligned dwords that hold a byte of the rows, use no global atomics; the text is a pure function of the input.
 * Refused before any device is touched: NULL pointers, an unknown format, n_cols outside 1 ... 2^30 - 1, n_rows outside
 * 1 ... 2^31 - 1, offsets that are not ascending; before any launch: a device pointer or a stream of another device. */
enum snpgpu_text_format { SNPGPU_TEXT_DIGIT = 0, SNPGPU_TEXT_PED_AB = 1, SNPGPU_TEXT_PED_12 = 2, SNPGPU_TEXT_PED_ALLELE = 3 };
int snpgpu_text_render(const void *rows, int64_t n_rows, int64_t n_cols, int format, const char *allele_pool,
                       const int64_t *allele_off, const char *prefix_pool, const int64_t *prefix_off, void *text, int64_t *line_off,
                       int device, void *stream);
/* of the last snpgpu_text_render on this thread: [0] ms of the length pass, [1] ms of the write pass, [2] launches, [3] bytes
 * written, [4] bytes of a lane's segment, [5] columns of a workgroup's tile */
int snpgpu_text_stats(double *stats);

/* ---- (1n) PLINK .ped text in: allele tokens of data lines as SNPGPU_GENO_PACKED2 sample rows ----------------------------------------------
 * What gnrParsePED (src/ConvToGDS.cpp:1175-1361) does per allele token -- one std::string and one std::map lookup, over two passes
 * of the file --, on the device.  The six leading columns of a line stay with the host; it hands over where the seventh starts.
 * The reference reads the file twice, and so do these calls: over every window of the text snpgpu_ped_tokens + snpgpu_ped_census,
 * then the host picks every SNP's reference allele from the table, then over every window snpgpu_ped_tokens + snpgpu_ped_codes.
 *
 * snpgpu_ped_tokens: line i's tokens are the maximal runs of bytes of text[cell_begin[i], line_end[i]) that are neither tab nor
 * space.
 *   text           DEVICE memory of `device`, any alignment; only aligned dwords that hold a byte of [text, text + n_bytes) are loaded
 *   tokens         DEVICE memory: the token matrix uint8 [n_lines][2 n_snp], token k of a line its k-th token's byte; tokens beyond
 *                  2 n_snp are counted and never stored
 *   line_flags, line_tokens   host, n_lines: the flags below and the number of tokens found
 * A token is regular when it is one byte in 0x21 ... 0x7E and its separator is one tab or a run of spaces: then it is the cell
 * CReadLine::GetCell (src/ConvToGDS.cpp:123-179) returns.  The kernel raises nothing: it flags the line, whose tokens may then
 * hold anything (inside its own bytes), and the caller settles it:
 *   1  a token of more than one byte, or a byte outside 0x21 ... 0x7E
 *   2  an empty token: a tab behind a tab or a space, a space behind a tab, a separator at cell_begin, a tab at the line's end
 *   8  line_tokens != 2 n_snp
 * snpgpu_ped_census: adds to table (DEVICE, uint32 [n_snp][94], zeroed by the caller before the first window) the number of times
 * byte 0x21 + c other than '0' is a token of SNP j in the lines whose line_flags (host) are 0: entry [j][c].  A workgroup owns a
 * range of SNPs; successive windows add on the stream.
 * snpgpu_ped_codes: rows (DEVICE, [n_lines][ceil(n_snp / 4)], tail padding 3) from the token matrix: [t1 == ref[j]] + [t2 == ref[j]],
 * 3 when either token is '0'.  ref (host, n_snp): the reference allele's byte, 0 = it is not a single byte (no token equals it).
 * The rows of flagged lines hold anything: the caller patches them.
 * No atomics touch global memory; the results are pure functions of the input.  Refused before any device is touched: NULL
 * pointers, offsets outside n_bytes or cell_begin > line_end, n_snp outside 1 ... 2^30 - 1, n_lines outside 1 ... 2^31 - 1; before
 * any launch: a device pointer or a stream of another device. */
int snpgpu_ped_tokens(const void *text, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end, int64_t n_lines,
                      int64_t n_snp, void *tokens, int32_t *line_flags, int64_t *line_tokens, int device, void *stream);
int snpgpu_ped_census(const void *tokens, const int32_t *line_flags, int64_t n_lines, int64_t n_snp, void *table, int device,
                      void *stream);
int snpgpu_ped_codes(const void *tokens, int64_t n_lines, int64_t n_snp, const uint8_t *ref, void *rows, int device, void *stream);
/* on this thread: [0] [1] [2] ms of the last tokens / census / codes kernel, [3] launches of the last call, [4] text bytes of the
 * last snpgpu_ped_tokens, [5] bytes of a workgroup's chunk, [6] of a lane's segment, [7] of the halo */
int snpgpu_ped_stats(double *stats);

/* ---- (1o) data sets side by side: snpgdsCombineGeno, snpgdsAlleleSwitch ------------------------------------------------------------
 * What snpgdsCombineGeno (R/AllUtilities.R:1525-1556) does with one int per genotype -- abs(t(x - t(g))), rbind, 1024 SNPs at a
 * time -- and gnrStrandSwitch (src/SNPRelate.cpp:454-494) with a byte per genotype, on the device and at two bits per genotype
 * all the way: the selected rectangles of several sources next to each other in one SNPGPU_GENO_PACKED2 row per output SNP, part
 * i's columns from code n_samp_0 + ... + n_samp_(i-1) on (an offset that is in general no multiple of 4), with the rows named by
 * `flip` re-coded to the other allele.  Which SNPs match and which are flipped is the caller's business (allele names, strands
 * and frequencies: host work).
 *   rows           DEVICE memory of `device`: [n_snp_out][ceil(N / 4)] bytes, N = the sum of n_samp; the unused codes of a row's
 *                  last byte are 3.  The first row may start at any byte address; nothing outside those bytes is stored.
 *                  rows must not overlap a source that lies in device memory: the sources are read while rows is written.
 * A host source that fits the staging size of snpgpu_geno_select goes to the device once.  A major 0 source without row_bit
 * whose samples are consecutive is then read where it lies on the device; every other part's rectangle of a window of output rows
 * is first brought to byte-aligned device rows by the selection of snpgpu_geno_select (every layout, memory kind and staging
 * window of a source is that call's).  One kernel splices a window.  A window holds the output rows whose staged bytes fit
 * SNPGPU_MERGE_STAGE_BYTES (default: the staging size of snpgpu_geno_select), at least one, and all rows when no part is staged.
 * There is no cap on n_parts: the descriptions of the parts live in device memory.
 * Refused before any device is touched: NULL parts / rows / bits; n_parts < 1, n_samp < 1 or n_snp_out < 1; an index outside
 * its source; N > 2^30 - 1; everything snpgpu_geno_select refuses about a source (the message names the part).  Refused before
 * any launch: a device pointer or a stream that belongs to another device than `device`. */
typedef struct snpgpu_merge_part {
    snpgpu_geno_src src;            /* as for snpgpu_geno_select: any layout, host / pinned / device memory                    */
    const int32_t  *snp_index;      /* host, n_snp_out entries: the source SNP of every output row; NULL = in order; may        */
                                    /* permute and repeat                                                                      */
    const int32_t  *samp_index;     /* host, n_samp entries: the source sample of every column this part contributes;          */
                                    /* NULL = all, in order                                                                    */
    int64_t         n_samp;         /* columns this part contributes (>= 1)                                                    */
    const uint8_t  *flip;           /* host, n_snp_out entries: non-zero = codes 0 / 1 / 2 / 3 of that row become 2 / 1 / 0 / 3; */
                                    /* NULL = none                                                                             */
} snpgpu_merge_part;
int snpgpu_geno_merge(const snpgpu_merge_part *parts, int n_parts, int64_t n_snp_out, void *rows, int device, void *stream);
/* of the last snpgpu_geno_merge on this thread (HIP events, summed over the windows): stats[0] ms of bringing the parts to aligned
 * rows (staging and selection), [1] ms of the splice kernel, [2] its launches, [3] windows, [4] bytes written to rows */
int snpgpu_geno_merge_stats(double *stats);

/* ---- (1p) Oxford GEN text: genotype probabilities of data lines called to SNPGPU_GENO_PACKED2 rows ---------------------------------------
 * What gnrParseGEN (src/ConvToGDS.cpp:1015-1157) does per sample -- three std::string cells, three strtof, one decision tree --, on
 * the device: the file's own bytes go there and 2-bit rows come out.  The five leading columns of a line (SNP id, rs id, position,
 * allele A, allele B) stay with the host; it hands over where the sixth starts.
 *
 * snpgpu_gen_genotypes: line i's tokens are the maximal runs of bytes of text[cell_begin[i], line_end[i]) that are neither tab nor
 * space; token t is probability t % 3 (AA, AB, BB) of sample t / 3.
 *   text, text_mem SNPGPU_HOST, SNPGPU_HOST_PINNED (both staged in windows of whole lines of at most SNPGPU_TEXT_STAGE_BYTES,
 *                  default 256 MiB) or SNPGPU_DEVICE (any alignment, parsed where it lies); only aligned dwords that hold a byte
 *                  of [text, text + n_bytes) are loaded
 *   call_threshold the double the reference compares with: a sample is called when its largest probability is >= it
 *   rows           DEVICE memory of `device`: [n_lines][ceil(n_samp / 4)], the unused codes of a row's last byte 0
 *   line_flags, line_cells   host, n_lines: the flags below and the number of tokens found
 * A regular token is `digits [ '.' digits ]` or `'.' digits` with at most 15 significant digits (leading zeros not counted) and at
 * most 22 digits behind the point.  Its digits are an integer m < 10^15 and a count k, both exact in fp64, so m / 10^k is the
 * correctly rounded double; it is rounded to single precision once more WITHOUT double rounding -- when it is exactly a midpoint
 * of two floats the sign of fma(d, 10^k, -m) says on which side the decimal number lies -- and is then the float strtof gives
 * (getFloat, src/ConvToGDS.cpp:506-532).  The three floats are widened to double and go through the tree of
 * src/ConvToGDS.cpp:1134-1145 with >= throughout: 2 = AA, 1 = AB, 0 = BB, 3 = no probability reaches call_threshold.
 * The kernel raises nothing: it flags the line, whose row may then hold anything (inside its own bytes), and the caller settles it
 * with snpgpu_gen_line_host:
 *    1  a token byte that is neither a digit nor the token's one point (signs, exponents, inf, nan, hex forms, quotes, '\r' and
 *       other isspace bytes, NUL)
 *    2  a token without a digit: "."
 *    4  more than 15 significant digits, or more than 22 digits behind the point
 *    8  a token longer than the halo (64 bytes)
 *   16  an empty cell: a tab beside a separator or at the line's end, a separator at cell_begin
 *   32  line_cells != 3 n_samp; tokens beyond 3 n_samp are counted and never stored
 * No device memory grows with n_lines x n_samp but rows; no atomics touch global memory; the result is a pure function of the
 * input.  Refused before any device is touched: NULL pointers, an unknown text_mem, offsets outside n_bytes or cell_begin >
 * line_end, n_samp outside 1 ... 2^30 - 1, n_lines outside 1 ... 2^31 - 1, host text with a line longer than a window; before any
 * launch: a device pointer or a stream of another device. */
int snpgpu_gen_genotypes(const void *text, int text_mem, int64_t n_bytes, const int64_t *cell_begin, const int64_t *line_end,
                         int64_t n_lines, int64_t n_samp, double call_threshold, void *rows, int32_t *line_flags,
                         int64_t *line_cells, int device, void *stream);
/* snpgpu_gen_line_host: the 3 n_samp cells of one line from its sixth column on (line, n_bytes: without the line end; the line ends
 * at a NUL if it holds one), read as the reference reads them: cells split by space and tab (CReadLine::GetCell,
 * src/ConvToGDS.cpp:123-179: a run of spaces is one separator, a tab is one, matching quotes are dropped, spaces may follow the
 * last cell), every cell through getFloat with the C library's strtof ("." is NaN, isspace bytes around the number are skipped),
 * the tree as above.  Makes no HIP call.
 *   codes          host, n_samp: one code 0 / 1 / 2 / 3 per sample
 *   column         0 when the line is read; else the 1-based number of the failing cell counted from `line` (the reference's
 *                  COLUMN is 5 more), and message (message_bytes) holds the reference's text: "fewer columns than what
 *                  expected.", "more columns than what expected.", "Invalid float conversion \"...\"."
 * The return value is non-zero for an argument error only (NULL pointers, n_samp outside 1 ... 2^30 - 1, n_bytes < 0). */
int snpgpu_gen_line_host(const char *line, int64_t n_bytes, int64_t n_samp, double call_threshold, uint8_t *codes,
                         int64_t *column, char *message, int64_t message_bytes);
/* of the last snpgpu_gen_genotypes on this thread: [0] ms of the text's copies to the device, [1] ms of the kernel, [2] launches,
 * [3] text bytes copied (or parsed in place), [4] bytes of a workgroup's chunk, [5] of a lane's segment, [6] of the halo */
int snpgpu_gen_stats(double *stats);

/* ---- (1q) classical multidimensional scaling of a distance matrix: snpgdsMDS ---------------------------------------------------------
 * For a symmetric n x n matrix dist (double, row-major, leading dimension ld >= n, in `mem`: SNPGPU_HOST, SNPGPU_HOST_PINNED, or
 * SNPGPU_DEVICE = memory of `device`) the k algebraically largest eigenpairs of
 *     B = -1/2 J (D o D) J,   J = I - 1 1^T / n,   D o D = dist with every entry squared
 * -- what R's cmdscale(dist, k) decomposes.  Largest by value, never by magnitude: B is indefinite for distances that are not
 * Euclidean (IBS, dissimilarity) and always has the eigenpair (0, 1).
 *   eigval      host [k], descending
 *   vectors     host [k][n], unit eigenvectors; in each the entry of largest magnitude (the lowest index on ties) is positive.  The
 *               points of cmdscale are vectors[i] * sqrt(eigval[i]) for the positive eigenvalues
 *   all_eigval  host [n] or NULL: every eigenvalue, descending, on the dense route; NaN on the Krylov route
 *   trace_b     the trace of B, (sum_ij d_ij^2 / n - sum_i d_ii^2) / 2, or NULL
 *   route       0 dense, 1 Krylov, or NULL
 * The matrix is read where it lies and never written; host memory is copied to the device in row windows of
 * SNPGPU_MDS_STAGE_BYTES (default 256 MiB).  One scan checks the entries and makes the row sums of D o D in a fixed order.  Up to
 * the dense threshold of snpgpu_pca_eigen (SNPGPU_EIG_DENSE_MAX) B is written to a buffer of its own and decomposed whole; beyond
 * it the block-Krylov solver works on q -> B q = -1/2 centre((D o D) centre(q)), D read once per product and squared on the way, B
 * never formed.  No atomics: the same input gives the same bits on the dense route and in every product.
 * That solver accepts a pair on |B v - theta v| / |theta|, which says nothing at theta ~ 0: a call in which it does not converge, or
 * returns an eigenvalue at or below n 2^-52 max_i sum_j d_ij^2 / 2 (what rounding makes of an exact zero), fails with "fewer than
 * k = ... eigenvalues appear to be positive"; the dense route returns such eigenvalues as they are.
 * Refused before any device is touched: NULL dist / eigval / vectors, n < 2, ld < n, an unknown memory kind, k outside
 * 1 ... n - 1 ("'k' must be in {1, 2, ..  n - 1}"); by the scan: a non-finite entry ("NA values not allowed in 'd'"), a pair
 * d[i][j] != d[j][i] (bitwise: "'d' must be exactly symmetric"); a matrix that does not fit the device beside the solver's work is
 * refused with both figures.  There is no CPU fallback. */
int snpgpu_mds(const double *dist, int64_t n, int64_t ld, int mem, int k, double *eigval, double *vectors, double *all_eigval,
               double *trace_b, int *route, int device);
/* Y = B Q for b >= 1 vectors, Q and Y host [b][n]: the operator of the Krylov route alone, with the same staging, scan and refusals */
int snpgpu_mds_apply(const double *dist, int64_t n, int64_t ld, int mem, const double *Q, int b, double *Y, int device);
/* snpgpu_mds on the working space: the IBS (what = 0: 1 - ibs, made on the device) or dissimilarity (what = 1) matrix of the selected
 * SNPs is finalised into device memory and decomposed there; the n x n matrix never reaches the host */
int snpgpu_gnrMDS(int what, int k, double *eigval, double *vectors, double *all_eigval, double *trace_b, int *route);
/* of the last snpgpu_mds / snpgpu_mds_apply / snpgpu_gnrMDS on this thread: stats[0] ms of the staging copies, [1] ms of the scan,
 * [2] ms of the eigen solve (host clock), [3] ms of the whole call (host clock), [4] the route, [5] operator products, [6] their
 * summed ms (HIP events), [7] staging windows, [8] the value at or below which an eigenvalue does not count as positive */
int snpgpu_mds_stats(double *stats);

/* ---- diagnostics (no reference counterpart) ---------------------------------------------------------------------------
 * What THIS device's matrix pipe sustains right now: a register-only stream of one MFMA instruction (never waiting on memory,
 * two waves per SIMD) run for `seconds`, rate taken over the second half.  The kernels of this library run against the socket
 * power cap, which depends on the operands' bit patterns and differs by a few per cent from box to box: bench.py measures it in
 * the run it reports (roofline.sustained_peak_measured).  tflops: TFLOP/s of the instruction; implied_mhz (may be NULL): the shader
 * clock that rate corresponds to (rate / flop per clock of the whole device). */
enum snpgpu_diag_mode {
    SNPGPU_DIAG_F16_ZERO = 0,      /* v_mfma_f32_32x32x16_f16, all operands zero: the unthrottled rate                              */
    SNPGPU_DIAG_F16_EXACT_ROW = 1, /* row operand small integers, column operand real-valued: the exact-row SYRK's operand classes */
    SNPGPU_DIAG_F16_UV = 2,        /* both operands (g - c) x fp16 factor: the single-product SYRK's operand classes                */
    SNPGPU_DIAG_FP4 = 3,           /* v_mfma_scale_f32_32x32x64_f8f6f4 on e2m1 operands {0, 1/2, 1} x {0, +-1}: the pair counters'  */
    SNPGPU_DIAG_F16_UV_16X16X32 = 4, /* the operands of mode 2 through v_mfma_f32_16x16x32_f16 (same flops, a quarter of the
                                      accumulator registers per instruction): what the other instruction shape sustains        */
    SNPGPU_DIAG_FP4_16X16X128 = 5, /* the operands of mode 3 through v_mfma_scale_f32_16x16x128_f8f6f4                            */
    SNPGPU_DIAG_F16_EXACT_ROW_16X16X32 = 6 /* the operands of mode 1 through v_mfma_f32_16x16x32_f16                            */
};
int snpgpu_diag_mfma_rate(int device, int mode, double seconds, double *tflops, double *implied_mhz);
/* What the fp64 vector pipe sustains right now: a register-only stream of independent v_fma_f64 chains (never waiting on memory)
 * run for `seconds`, rate over the second half.  tflops: TFLOP/s counting an FMA as two flops */
int snpgpu_diag_fp64_rate(int device, double seconds, double *tflops);
/* PCI address "dddd:bb:dd.f" of HIP device `device` (hipDeviceGetPCIBusId): which physical GPU a rank really drives */
int snpgpu_diag_device_pci(int device, char *buf, int len);
/* The kernel path a context of `kind` over n_samp samples would take under the CURRENT environment, as "key=value" lines in buf
 * (NUL-terminated; an error when len is too small): the plan snpgpu_create allocates from and snpgpu_feed reads, the names of the
 * kernels a block with / without missing calls takes, and -- block_snps > 0 -- the fp32 run geometry of a block of that many SNPs.
 * Makes no HIP call (opts->device is ignored, opts may be NULL): the dispatch can be checked on a host without a GPU.  Refusals of
 * snpgpu_create that do not depend on the device (invalid panel rows, a form the dissimilarity kind lacks) are returned as such. */
int snpgpu_diag_plan(int kind, int64_t n_samp, const snpgpu_opts *opts, int64_t block_snps, char *buf, int len);
/* Work items of the GRM / PCA single-product kernel that found no free slot of its carry scratch (SNPGPU_UVC_CARRY_SLOTS) since the
 * context was created or the count was last reset: they added their partial sums to the panel after every fp32 run instead (slower,
 * the same result up to rounding).  0 for contexts without the scratch.  Waits for the context's stream. */
int snpgpu_diag_carry_fallbacks(snpgpu_ctx *ctx, int64_t *count, int reset);

/* ---- 1r. PC-Relate: ancestry-adjusted kinship (no reference counterpart) ------------------------------------
 * Kinship, k0, k2 and inbreeding from genotype residuals under individual-specific allele frequencies (Conomos, Reiner, Weir,
 * Thornton, AJHG 2016), fp64 throughout.  V = [1, pcs] is n_samp x (n_pc + 1); per SNP s, with T the training samples:
 *   f_s = sum_{i in T, called} g_is / (2 #{i in T called}); g~_is = g_is where called, else 2 f_s; a SNP without a called training
 *   sample contributes nothing.  beta_s = sum_{i in T} g~_is W_i with W = V_T (V_T^T V_T)^-1 (made on the host at creation);
 *   mu_is = (beta_s0 + sum_d beta_sd V_id) / 2; (i, s) is valid iff called and maf_thresh <= mu_is <= 1 - maf_thresh.
 * Over the valid (i, s), with R = g - 2 mu, c = mu (1 - mu), S = sqrt(c), gD = mu / 0 / 1 - mu for g = 0 / 1 / 2, I0 = [g = 0],
 * I2 = [g = 2], A = mu^2, B = (1 - mu)^2, the n x n planes summed over all SNPs fed are, in the order of snpgpu_pcr_sums,
 *   0 RR = sum R_i R_j   1 SS = sum S_i S_j   2 DD = sum gD_i gD_j   3 DC = sum gD_i c_j (not symmetric)   4 CC = sum c_i c_j
 *   5 IBS0 = sum (I0_i I2_j + I2_i I0_j)   6 K0D = sum (A_i B_j + B_i A_j)   7 NS = the SNPs valid for both
 * and kinship = RR / (4 SS); inbreed_i = 2 kinship_ii - 1; with e_i = 1 + inbreed_i,
 *   k2 = (DD_ij - e_j DC_ij - e_i DC_ji + e_i e_j CC_ij) / CC_ij; k0 = IBS0 / K0D where kinship < 2^(-5/2), else 1 - 4 kinship + k2.
 * A zero denominator gives NaN.  The diagonal goes through the same expressions: its kinship is (1 + f_i) / 2, its k0 and k2 carry
 * no meaning.  Not built: the small-sample correction, per-variant scaling, multi-device objects, results in device memory,
 * anything below fp64.  (Row panels and the selection of related pairs on the device: the end of this section.)
 * Every sum has one owner and a fixed order (no atomics): the same feeds give the same bits.  A feed is cut into internal blocks
 * whose nine operand planes stay within SNPGPU_PCR_STAGE_BYTES (environment, read at creation; default 1 GiB, at least 16 SNPs).
 * Argument errors are refused before any HIP call; planes that do not fit the device's free memory are refused with both figures. */
typedef struct snpgpu_pcr snpgpu_pcr;
enum { SNPGPU_PCR_IBD = 1 };   /* also accumulate DD, DC, CC, IBS0, K0D; without it only RR, SS, NS */
/* pcs: host [n_samp][n_pc], 0 <= n_pc <= 32, all finite; training: host [n_samp] (non-zero = in T) or NULL = all, at least
 * n_pc + 2 samples; maf_thresh inside (0, 0.5); opts: device and stream are read.  Collinear PCs in T are refused. */
int snpgpu_pcr_create(int64_t n_samp, int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags,
                      const snpgpu_opts *opts, snpgpu_pcr **out);
/* n_snp rows (SNPGPU_GENO_PACKED2 or SNPGPU_GENO_U8, host or device memory, as snpgpu_ld_feed takes them); returns when they have
 * been read.  beta: host [n_snp][n_pc + 1] receiving the regression coefficients of these SNPs, or NULL */
int snpgpu_pcr_feed(snpgpu_pcr *pcr, const void *geno, int64_t n_snp, int format, int mem, double *beta);
/* host arrays, any may be NULL: kinship, k0, k2, nsnp n x n (row-major, full), inbreed [n].  k0 / k2 need SNPGPU_PCR_IBD.  May be
 * called between feeds. */
int snpgpu_pcr_result(snpgpu_pcr *pcr, double *kinship, double *inbreed, double *k0, double *k2, double *nsnp);
/* one accumulated plane as a full host n x n matrix, `which` in the order above (2 ... 6 need SNPGPU_PCR_IBD) */
int snpgpu_pcr_sums(snpgpu_pcr *pcr, int which, double *plane);
/* stats[0] internal blocks, [1] product launches, [2] .. [5] HIP-event ms of the beta, operand, product and finaliser phases,
 * [6] bytes of the resident planes, [7] SNPs of an internal block -- since creation */
int snpgpu_pcr_stats(snpgpu_pcr *pcr, double *stats);
int snpgpu_pcr_destroy(snpgpu_pcr *pcr);
/* create / feed / result on the working space's selected SNPs and device (fed in its blocks) */
int snpgpu_gnrPCRelate(int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags,
                       double *kinship, double *inbreed, double *k0, double *k2, double *nsnp);

/* Row panels.  A panel object keeps rows [row_begin, row_end) x columns [row_begin, n_samp) of every plane as a
 * slab -- three without SNPGPU_PCR_IBD, nine with it: the eight planes and CD with CD_ij = DC_ji, the half of DC a panel's rows do
 * not hold (accumulated for the columns >= row_end only: inside the diagonal block DC holds both halves) -- and the diagonal tiles of RR and SS for the inbreeding of all n_samp samples.  Its internal blocks and tiles are the
 * full object's: after the same feeds every sum, result and selected value equals, bit for bit, what an object of
 * snpgpu_pcr_create with the same arguments holds at the same (i, j), however the rows are cut into panels.
 * row_begin: a non-negative multiple of 128; row_begin < row_end <= n_samp, row_end a multiple of 128 or n_samp.  The other
 * arguments, the checks and the refusal of memory that does not fit: as snpgpu_pcr_create.  snpgpu_pcr_feed, snpgpu_pcr_stats ([6]:
 * the bytes of slabs and strips) and snpgpu_pcr_destroy take a panel handle; snpgpu_pcr_result and snpgpu_pcr_sums refuse it. */
int snpgpu_pcr_create_panel(int64_t n_samp, int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags,
                            int64_t row_begin, int64_t row_end, const snpgpu_opts *opts, snpgpu_pcr **out);
/* The rows and columns of the panel of snpgpu_pcr_result's matrices: host [row_end - row_begin][n_samp - row_begin], row-major, any
 * may be NULL; inbreed [n_samp], all samples.  A full handle is the panel [0, n_samp).  May be called between feeds. */
int snpgpu_pcr_panel_result(snpgpu_pcr *pcr, double *kinship, double *inbreed, double *k0, double *k2, double *nsnp);
/* one accumulated plane in the same shape; `which` as snpgpu_pcr_sums, or 8 = CD: DC transposed */
int snpgpu_pcr_panel_sums(snpgpu_pcr *pcr, int which, double *plane);
/* the two product launches a panel adds to a full object's, in HIP-event ms since creation: ms2[0] the CD job (DC's other half,
 * stored transposed), ms2[1] the strips of diagonal tiles.  Both are part of snpgpu_pcr_stats' [4] as well; 0 for a full handle. */
int snpgpu_pcr_panel_stats(snpgpu_pcr *pcr, double *ms2);
/* The related pairs of a panel (or of a full handle), selected on the device from the resident sums: row_begin <= idx1 < row_end,
 * idx1 < idx2 < n_samp, samp_sel[idx1] && samp_sel[idx2] (host [n_samp], NULL = all), kinship >= kinship_cutoff; a NaN kinship is
 * never selected, a non-finite cutoff selects every pair.  Order: idx1 ascending, then idx2 ascending.  The values are what
 * snpgpu_pcr_result holds at (idx2, idx1), the entry snpgdsIBDSelection reads.  Host outputs, any may be NULL: the first `capacity`
 * pairs are stored, nothing behind them; *n_found = all selected pairs; capacity 0 takes no pair output (count only); inbreed
 * [n_samp] is written whatever the capacity.  k0 / k2 need SNPGPU_PCR_IBD. */
typedef struct snpgpu_pcr_sel_opts { double kinship_cutoff; const uint8_t *samp_sel; } snpgpu_pcr_sel_opts;
int snpgpu_pcr_select(snpgpu_pcr *pcr, const snpgpu_pcr_sel_opts *o, int64_t capacity, int32_t *idx1, int32_t *idx2,
                      double *kinship, double *k0, double *k2, double *nsnp, double *inbreed, int64_t *n_found);
/* the last snpgpu_pcr_select of this thread: HIP-event ms of {count pass, scan, write pass}, then the whole call on the host clock */
int snpgpu_pcr_select_stats(double *ms4);
/* The related pairs of the working space's selected SNPs, panel by panel in ascending row order: create, feed every block as
 * snpgpu_gnrPCRelate does, select, append.  panel_rows: a positive multiple of 128, or >= the number of samples (one panel), or 0 =
 * the largest multiple of 128 that fits the device's free memory beside the selection's outputs of all its pairs; the pairs found
 * never depend on it.  The result is kept until
 * the next call or snpgpu_ws_clear; snpgpu_gnrPCRelatePairs_get copies it (*n_found entries each, inbreed [n_samp]; k0 / k2 only
 * with SNPGPU_PCR_IBD). */
int snpgpu_gnrPCRelatePairs(int n_pc, const double *pcs, const uint8_t *training, double maf_thresh, int flags, int64_t panel_rows,
                            double kinship_cutoff, const uint8_t *samp_sel, int verbose, int64_t *n_found, int64_t *n_panels);
int snpgpu_gnrPCRelatePairs_get(int32_t *idx1, int32_t *idx2, double *kinship, double *k0, double *k2, double *nsnp, double *inbreed);

/* ---- 1s. Ancestry proportions by EM (no reference counterpart) -----------------------------------------------
 * The likelihood model of FRAPPE (Tang et al. 2005) and ADMIXTURE: g_ij ~ Binomial(2, sum_k q_ik f_kj) over the called genotypes
 * (a code of 3 contributes nothing anywhere), fp64 throughout.  State: Q [n_samp][n_pop], rows on the simplex, and F [m][n_pop],
 * the frequency of the counted allele of SNP j in population k, kept inside [f_min, 1 - f_min].  One iteration from (Q, F):
 *   h1_ij = sum_k q_ik f_kj            h0_ij = sum_k q_ik (1 - f_kj)      (h0 is its own sum of positive terms, not 1 - h1)
 *   w1_ij = g_ij / h1_ij               w0_ij = (2 - g_ij) / h0_ij
 *   a_ik  = sum_j (w1_ij f_kj + w0_ij (1 - f_kj))      q'_ik = q_ik a_ik / sum_k' q_ik' a_ik'   (no called SNP: the row stays)
 *   u_kj  = f_kj sum_i w1_ij q_ik      v_kj = (1 - f_kj) sum_i w0_ij q_ik
 *   f'_kj = clamp(u_kj / (u_kj + v_kj), f_min, 1 - f_min)                                        (u + v = 0: f_kj stays)
 *   L(Q, F) = sum_ij g_ij log h1_ij + (2 - g_ij) log h0_ij
 * Q' and F' are both made from the old (Q, F): one pass over the genotypes per iteration.  With SNPGPU_ADMIX_FIX_F only Q moves
 * (supervised estimation, projection onto given frequencies).
 * Every sum has one owner and a fixed order (no atomics).  The per-SNP sums are cut at the absolute sample indices s * 4096, the
 * per-sample sums at the absolute SNP indices s * 1024, the parts are folded in ascending order, L is the fold of the SNPs' parts by
 * one workgroup: the bits depend neither on how the rows were cut into feeds, nor on their format or memory kind, nor on block_snps.
 * Not built: acceleration (SQUAREM, quasi-Newton), cross-validation, multi-device objects, results in device memory, anything
 * below fp64.  Argument errors and calls out of order are refused before any HIP call: snpgpu_admix_create makes none, host rows
 * fed before the device is open are copied and wait, and so do the values of snpgpu_admix_set; the first run, get or feed of device
 * rows opens the device and takes what waits.  An object that does not fit the device's free memory is refused there with both
 * figures. */
typedef struct snpgpu_admix snpgpu_admix;
enum { SNPGPU_ADMIX_FIX_F = 1 };   /* snpgpu_admix_run: F stays, only Q moves */
/* n_pop in 2 ... 32; max_snps: the rows the object can take (they stay resident as 2-bit rows); f_min inside (0, 0.5); block_snps:
 * the SNPs of an internal block of a pass, a multiple of 16 up to 2^20, or 0 = all of max_snps (at most 2^20: nothing is staged
 * per block, so the free memory sets no smaller one); opts: device and stream are read. */
int snpgpu_admix_create(int64_t n_samp, int n_pop, int64_t max_snps, double f_min, int64_t block_snps, const snpgpu_opts *opts,
                        snpgpu_admix **out);
/* appends n_snp rows (SNPGPU_GENO_PACKED2 or SNPGPU_GENO_U8, host or device memory, as snpgpu_pcr_feed takes them); returns when
 * they have been read */
int snpgpu_admix_feed(snpgpu_admix *ad, const void *geno, int64_t n_snp, int format, int mem);
/* host q [n_samp][n_pop]: finite, non-negative, every row with a positive sum (normalised on entry); host f [rows fed][n_pop]: finite
 * (clamped on entry).  Either may be NULL = keep.  Rows fed after f was set need f set again. */
int snpgpu_admix_set(snpgpu_admix *ad, const double *q, const double *f);
/* Up to max_iter iterations t = 0, 1, ...; loglik [max_iter + 1] (host): loglik[t] = L of the state before iteration t, which falls
 * out of the pass that makes it.  Stops after iteration t >= 1 when loglik[t] - loglik[t - 1] < tol; then one likelihood-only pass:
 * *n_done iterations were made and loglik[*n_done] belongs to the state snpgpu_admix_get returns.  max_iter = 0 evaluates L.  The
 * passes run back to back on the object's stream; the host reads one scalar per pass. */
int snpgpu_admix_run(snpgpu_admix *ad, int max_iter, double tol, int flags, double *loglik, int *n_done);
/* host q [n_samp][n_pop], f [rows F was set for][n_pop]; either may be NULL */
int snpgpu_admix_get(snpgpu_admix *ad, double *q, double *f);
/* stats[0] internal blocks of the last pass, [1] kernel launches, [2] HIP-event ms of the passes, [3] resident bytes, [4] SNPs of an
 * internal block, [5] iterations -- since creation */
int snpgpu_admix_stats(snpgpu_admix *ad, double *stats);
int snpgpu_admix_destroy(snpgpu_admix *ad);
/* create / feed / set / run / get on the working space's selected SNPs and device; q, f: the starting values (both required) */
int snpgpu_gnrAdmix(int n_pop, double f_min, int64_t block_snps, const double *q, const double *f, int max_iter, double tol, int flags,
                    double *loglik, int *n_done, double *q_res, double *f_res);

/* Diagnostic: kernel launches of the SYRK family that the feeds of this context have enqueued since it was created -- with
 * SNPGPU_RUN_INNER=0 one per fp32 run of a block, otherwise one per block and kernel.  snpgpu_get_timing's `launches` counts the
 * timed spans instead: one per table and feed block. */
int snpgpu_diag_syrk_launches(snpgpu_ctx *ctx, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* SNPGPU_H */
