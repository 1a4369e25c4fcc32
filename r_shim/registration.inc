// Registration delta for src/SNPRelate.cpp (R_init_SNPRelate, the callMethods[] table at :1154-1205).
// The entries below REPLACE the entries of the same names; every other entry, R_registerRoutines and
// R_useDynamicSymbols(info, FALSE) stay as they are.  Names and arity are unchanged, so R/*.R is untouched.
//
//   extern "C" declarations (top of the file, next to the other routine declarations):
extern SEXP gpu_gnrGRM(SEXP, SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrGRM_avg_val();
extern SEXP gpu_gnrIBD_KING_Homo(SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIBD_KING_Robust(SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIBSAve(SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIBSNum(SEXP, SEXP);
extern SEXP gpu_gnrPCA(SEXP, SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrLDMat(SEXP, SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIBD_MLE(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIBD_LogLik(SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIBD_LogLik_k01(SEXP, SEXP, SEXP);
extern SEXP gpu_gnrLDpruning(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrDiss(SEXP, SEXP);
extern SEXP gpu_gnrFst(SEXP, SEXP, SEXP);
extern SEXP gpu_gnrSampFreq();
extern SEXP gpu_gnrHWE();
extern SEXP gpu_gnrIndInb(SEXP, SEXP, SEXP, SEXP, SEXP);
extern SEXP gpu_gnrIndInbCoef(SEXP, SEXP, SEXP);
extern SEXP gpu_gnrDistPerm(SEXP, SEXP, SEXP, SEXP, SEXP);
//
//   table entries:
//     { "gnrGRM",             (DL_FUNC)&gpu_gnrGRM,             5 },
//     { "gnrGRM_avg_val",     (DL_FUNC)&gpu_gnrGRM_avg_val,     0 },
//     { "gnrIBD_KING_Homo",   (DL_FUNC)&gpu_gnrIBD_KING_Homo,   3 },
//     { "gnrIBD_KING_Robust", (DL_FUNC)&gpu_gnrIBD_KING_Robust, 4 },
//     { "gnrIBSAve",          (DL_FUNC)&gpu_gnrIBSAve,          3 },
//     { "gnrIBSNum",          (DL_FUNC)&gpu_gnrIBSNum,          2 },
//     { "gnrPCA",             (DL_FUNC)&gpu_gnrPCA,             5 },
//     { "gnrLDMat",           (DL_FUNC)&gpu_gnrLDMat,           5 },
//     { "gnrIBD_MLE",         (DL_FUNC)&gpu_gnrIBD_MLE,         9 },
//     { "gnrIBD_LogLik",      (DL_FUNC)&gpu_gnrIBD_LogLik,      3 },
//     { "gnrIBD_LogLik_k01",  (DL_FUNC)&gpu_gnrIBD_LogLik_k01,  3 },
//     { "gnrLDpruning",       (DL_FUNC)&gpu_gnrLDpruning,       8 },
//     { "gnrDiss",            (DL_FUNC)&gpu_gnrDiss,            2 },
//     { "gnrFst",             (DL_FUNC)&gpu_gnrFst,             3 },
//     { "gnrSampFreq",        (DL_FUNC)&gpu_gnrSampFreq,        0 },
//     { "gnrHWE",             (DL_FUNC)&gpu_gnrHWE,             0 },
//     { "gnrIndInb",          (DL_FUNC)&gpu_gnrIndInb,          5 },
//     { "gnrIndInbCoef",      (DL_FUNC)&gpu_gnrIndInbCoef,      3 },
//     { "gnrDistPerm",        (DL_FUNC)&gpu_gnrDistPerm,        5 },
//
// The CPU bodies (gnrGRM ... in src/genPCA.cpp, src/genIBS.cpp, src/genKING.cpp) may stay in the package as
// unregistered functions -- e.g. behind options(snpgpu.enable = FALSE) with a second table -- or be deleted together
// with ThreadPool.cpp and the SIMD kernels they were the only users of.
