"""Host-side mirror of the reference's R interface for the pairwise hot path.

Same function names, argument names/meaning, defaults, return fields and error
behaviour as the R functions (R is absent from the build image, so the host
side above the C ABI is Python; the R shim a maintainer would add is in
INTEGRATION.md):

    snpgdsOpen / snpgdsClose      R/AllUtilities.R:32-155   (in-memory GenoFile)
    snpgdsIBS, snpgdsIBSNum       R/IBS.R:22-73
    snpgdsIBDKING                 R/IBD.R:333-419
    snpgdsGRM                     R/IBD.R:543-615  (methods GCTA, Eigenstrat, Corr, EIGMIX/Weighted, IndivBeta)
    snpgdsMergeGRM                R/IBD.R:624-741
    snpgdsIBDMoM                  R/IBD.R:22-68    (PLINK method of moments)
    snpgdsIndivBeta               R/IBD.R:838-866
    snpgdsEIGMIX                  R/PCA.R:311-338
    snpgdsPCA                     R/PCA.R:22-91    (algorithm="exact")
    snpgdsSNPRateFreq             R/AllUtilities.R (allele freq / MAF / missing rate)
    snpgdsLDMat                   R/LD.R:53-92     (LD between SNP pairs)
    snpgdsIBDMLE                  R/IBD.R:79-156   (IBD by maximum likelihood, method "EM")
    snpgdsIBDMLELogLik            R/IBD.R:162-205
    snpgdsLDpruning               R/LD.R:100-243   (LD-based SNP pruning)
    snpgdsDiss                    R/IBD.R:432-450  (individual dissimilarity)
    snpgdsFst                     R/IBD.R:756-830  (fixation index, W&C84 / W&H02)
    snpgdsSlidingWindow           R/AllUtilities.R:1998-2239 (window scan of Fst / allele frequencies / a callable)
    snpgdsSampMissRate            R/AllUtilities.R:230-248   (missing rate per sample)
    snpgdsHWE                     R/AllUtilities.R:255-279   (exact test of Hardy-Weinberg equilibrium per SNP)
    snpgdsSelectSNP               R/AllUtilities.R:286-299   (the SNPs that pass the filters)
    snpgdsIndInbCoef              R/AllUtilities.R:312-341   (inbreeding coefficient of one individual, on the host)
    snpgdsIndInb                  R/AllUtilities.R:349-378   (individual inbreeding coefficients, six methods)
    snpgdsIBDSelection            R/IBD.R:463-531  (table of pairs at or above a kinship cutoff, on the host)
    snpgdsIBDPairs                no reference counterpart: the same table straight from the GPU counters
    snpgdsLDScore                 no reference counterpart: per-SNP sums of squared LD over a window, folded on the GPU
    snpgdsGetGeno                 R/AllUtilities.R:1006-1025 (the selected rectangle of the genotype node)
    snpgdsOpenBED                 R/Conversion.R:433-653 (snpgdsBED2GDS + snpgdsOpen: a PLINK .bed/.bim/.fam triple read in place)
    snpgdsGDS2BED                 R/Conversion.R:310-425 (the selected rectangle as PLINK .bed/.bim/.fam)
    snpgdsOption                  R/AllUtilities.R:1910-1990 (without a file: the chromosome codes snpgdsOpenBED takes)
    snpgdsGDS2PED                 R/Conversion.R:26-124  (the selected rectangle as PLINK text .ped/.map, the lines made on the GPU)
    snpgdsGDS2Eigen               R/Conversion.R:695-785 (the selected rectangle as EIGENSTRAT .eigenstratgeno/.snp/.ind)
    snpgdsOpenPED                 R/Conversion.R:132-302 (snpgdsPED2GDS + snpgdsOpen: PLINK text .ped/.map parsed on the GPU)
    snpgdsOpenGEN                 R/Conversion.R:795-964 (snpgdsGEN2GDS + snpgdsOpen: Oxford .gen/.sample read and called on the GPU)
    snpgdsSNPList                 R/AllUtilities.R:637-658   (SNP ids, positions, alleles and allele frequencies of one data set)
    snpgdsSNPListIntersect        R/AllUtilities.R:667-736   (the SNPs several data sets share, and who counts the other allele)
    snpgdsCombineGeno             R/AllUtilities.R:1285-1583 (data sets merged: the genotypes spliced on the GPU)
    snpgdsAlleleSwitch            R/AllUtilities.R:1686-1751 (a data set re-coded against given A alleles, the rows flipped on the GPU)
    snpgdsMDS                     no reference counterpart: the tutorial's cmdscale(1 - ibs$ibs, k), the eigenpairs found on the GPU
    snpgdsAdmixProp               R/PCA.R:347-425  (admixture proportions from eigenvectors, on the host)
    snpgdsAdmixTable              R/PCA.R:525-556  (their summary by group, on the host)
    snpgdsAdmix                   no reference counterpart: ancestry proportions by EM on the binomial likelihood, on the GPU

All arithmetic on genotype matrices runs on the MI355X through libsnpgpu.so
(`_lib`); there is no CPU fallback.  The one exception is snpgdsIndInbCoef, which
takes one individual's vectors and, like its R original, computes on the host.  R's ``NULL`` is ``None``, ``NaN`` is ``float('nan')``; R lists
are dicts with the same field names.
"""
import ctypes
import math
import time
import warnings

import numpy as np

from . import _lib
from . import gds as _gds
from . import bed as _bed
from . import vcf as _vcf
from . import merge as _merge
from .gds import GenoFile, open_gds, pack_2bit_rows  # noqa: F401




def snpgdsOpen(filename, stream=False, **_):
    """snpgdsOpen (R/AllUtilities.R:32-155).  stream=True: the genotype node stays on disk and is read block by block
    (gds.GenoStream: `.blocks(n)` feeds accumulators with 2-bit rows; the snpgds* functions below still work on it -- they set
    up a working space of the selected genotypes, for which the node is read once on first use)."""
    if stream:
        from .gds import open_gds_stream
        return open_gds_stream(filename)
    return open_gds(filename)


def snpgdsClose(gdsobj):
    return None


def _cat(verbose, *a):
    if verbose:
        print(*a, sep="")


def _init_file2(cmd, gdsobj, sample_id, snp_id, autosome_only=True, remove_monosnp=True,
                maf=float("nan"), missing_rate=float("nan"), num_thread=1, verbose=True, device=0, allele_freq=None):
    """.InitFile2, R/Internal.R:166-484: sample/SNP selection, autosome filter,
    gnrSetGenoSpace, gnrSelSNP_Base (gnrSelSNP_Base_Ex when allele.freq is given), gnrGetGenoDim.
    allele_freq follows the reference's bookkeeping: given per entry of `snp_id` (or per SNP of the file), it is
    brought into DATASET order with match(snp.ids[kept], snp.id) (R/Internal.R:355,370,405), drives the SNP filter
    (non-finite = excluded) and is returned subset to the surviving SNPs as ws["allele_freq"]."""
    if not isinstance(gdsobj, (GenoFile, _gds.GenoStream)):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    if num_thread is None or (isinstance(num_thread, float) and math.isnan(num_thread)):
        import os
        num_thread = os.cpu_count() or 1
    num_thread = int(num_thread)
    if num_thread < 1:
        raise ValueError("`num.thread' should be a positive value or NA.")
    _cat(verbose and cmd, cmd)

    sample_ids = gdsobj.sample_id
    samp_flag = None
    if sample_id is not None:
        want = np.asarray(sample_id)
        samp_flag = np.isin(sample_ids, want)
        if int(samp_flag.sum()) != len(want):
            raise ValueError("Some of sample.id do not exist!")
        if samp_flag.sum() <= 0:
            raise ValueError("No sample in the working dataset.")
        sample_ids = sample_ids[samp_flag]

    snp_ids = gdsobj.snp_id
    snp_flag = np.ones(len(snp_ids), bool)
    want = None
    if allele_freq is not None:
        allele_freq = np.ascontiguousarray(allele_freq, np.float64)
    if snp_id is not None:
        want = np.asarray(snp_id)
        if allele_freq is not None and len(allele_freq) != len(want):
            raise ValueError("'length(allele.freq)' should be 'length(snp.id)'.")
        snp_flag = np.isin(snp_ids, want)
        if int(snp_flag.sum()) != len(want):
            raise ValueError("Some of snp.id do not exist!")
        if snp_flag.sum() <= 0:
            raise ValueError("No SNP in the working dataset.")
    elif allele_freq is not None and len(allele_freq) != len(snp_ids):
        raise ValueError("'length(allele.freq)' should be the number of SNPs.")
    if autosome_only is not False:
        chrom = gdsobj.snp_chromosome
        if autosome_only is True and chrom.dtype.kind in "USO":
            # a text node (snpgdsOpenBED(cvt_chr="char")): the labels that parse into the autosome range
            val, ok = _bed.chrom_numeric(chrom)
            chrom = np.where(ok, val, gdsobj.autosome_start - 1)
        if autosome_only is True:
            # gnrChromRangeNumeric, src/SNPRelate.cpp:1035-1062 with snpgdsOption() defaults
            auto = (chrom >= gdsobj.autosome_start) & (chrom <= gdsobj.autosome_end)
            m = int(len(snp_ids) - (snp_flag & auto).sum())
            _cat(verbose, "Excluding %d SNP%s (non-autosomes or non-selection)" % (m, "" if m == 1 else "s"))
        else:
            auto = (chrom == autosome_only)
            _cat(verbose, "Keeping %d SNPs according to chromosome %s" % (int((snp_flag & auto).sum()), autosome_only))
        snp_flag &= auto
    if allele_freq is not None:
        if want is not None:
            # allele.freq[match(snp.ids[snp.id], tmp.id)]: position of every kept dataset SNP in the caller's list
            order = np.argsort(want, kind="stable")
            pos = order[np.searchsorted(want[order], snp_ids[snp_flag])]
            allele_freq = allele_freq[pos]
        else:
            allele_freq = allele_freq[snp_flag]
    snp_ids = snp_ids[snp_flag]

    # gnrSetGenoSpace: the selected rectangle becomes the working space.  With a sample selection it comes from the device
    # (snpgpu_geno_select: no byte per genotype on the way) -- out of the object's packed rows, or for a GenoStream out of the
    # file's node through the reader; without a device the host unpacks, selects and packs (the same bytes).
    n_samp = gdsobj.n_samp
    if samp_flag is not None and not samp_flag.all():
        if _device_visible():
            samp_index = np.flatnonzero(samp_flag).astype(np.int32)
            if isinstance(gdsobj, _gds.GenoStream) and getattr(gdsobj, "_packed", None) is None:
                # only the SNP range that holds a selected SNP is read; the flags pick the rows inside it
                kept = np.flatnonzero(snp_flag)
                k0, k1 = (int(kept[0]), int(kept[-1]) + 1) if kept.size else (0, 0)
                rows = [r for _, _, r in gdsobj.select_blocks(65536, samp_index=samp_index, snp_begin=k0, snp_end=k1, device=device, to="host")]
                packed = (np.concatenate(rows, 0) if rows else np.empty((0, (len(samp_index) + 3) // 4), np.uint8))[snp_flag[k0:k1]]
            else:
                packed = _lib.geno_select(gdsobj.packed, 0, gdsobj.n_snp, n_samp, row_stride_bits=8 * ((n_samp + 3) // 4),
                                          samp_index=samp_index, device=device,
                                          snp_index=None if snp_flag.all() else np.flatnonzero(snp_flag).astype(np.int32))
        else:
            from .gds import unpack_2bit_rows
            g = unpack_2bit_rows(gdsobj.packed[snp_flag], n_samp)[:, samp_flag]
            packed = pack_2bit_rows(g)
        n_samp = int(samp_flag.sum())
    else:
        packed = gdsobj.packed[snp_flag]
    packed = np.ascontiguousarray(packed)
    L = _lib.lib()
    _lib.check(L.snpgpu_ws_set_geno(_lib._ptr(packed), packed.shape[0], n_samp, _lib.GENO_PACKED2, int(device)))

    if remove_monosnp or np.isfinite(maf) or np.isfinite(missing_rate):
        t_maf, t_miss = maf, missing_rate
        if not np.isfinite(maf):
            maf = -1.0               # R/Internal.R:438-439
        if not np.isfinite(missing_rate):
            missing_rate = 2.0
        sel = np.zeros(packed.shape[0], np.uint8)
        nex = ctypes.c_int32(0)
        if allele_freq is None:
            _lib.check(L.snpgpu_ws_sel_snp_base(int(bool(remove_monosnp)), float(maf), float(missing_rate),
                                                ctypes.byref(nex), _lib._ptr(sel)))
        else:
            allele_freq = np.ascontiguousarray(allele_freq)
            _lib.check(L.snpgpu_ws_sel_snp_base_ex(_lib._ptr(allele_freq), int(bool(remove_monosnp)), float(maf),
                                                   float(missing_rate), ctypes.byref(nex), _lib._ptr(sel)))
            allele_freq = np.ascontiguousarray(allele_freq[sel.astype(bool)])
        snp_ids = snp_ids[sel.astype(bool)]
        packed = packed[sel.astype(bool)]
        _cat(verbose, "Excluding %d SNP%s (monomorphic: %s, MAF: %s, missing rate: %s)" %
             (nex.value, "" if nex.value == 1 else "s", str(bool(remove_monosnp)).upper(), t_maf, t_miss))

    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(L.snpgpu_ws_get_geno_dim(ctypes.byref(a), ctypes.byref(b)))
    if verbose:
        print("    # of samples: %d" % b.value)
        print("    # of SNPs: %d" % a.value)
        print("    using %d thread%s (the GPU path ignores num.thread)" % (num_thread, "" if num_thread == 1 else "s"))
    return dict(sample_id=sample_ids, snp_id=snp_ids, n_snp=a.value, n_samp=b.value,
                num_thread=num_thread, verbose=verbose, packed=packed, device=int(device), allele_freq=allele_freq)


def _device_visible():
    """whether snpgpu_device_count reports a device (the selection of _init_file2 runs there when it does)"""
    try:
        return _lib.device_count() > 0
    except _lib.SnpGpuError:
        return False


def _tri_or_full(n, use_matrix):
    return np.empty(_lib.tri_size(n) if use_matrix else (n, n), np.float64)


def snpgdsSNPRateFreq(gdsobj, sample_id=None, snp_id=None, with_id=False, device=0):
    """Allele frequency, MAF and missing rate per SNP (Get_AF_MR_perSNP,
    src/dGenGWAS.cpp:472-552) over the selected samples."""
    ws = _init_file2(None, gdsobj, sample_id, snp_id, autosome_only=False, remove_monosnp=False,
                     verbose=False, device=device)
    L = ws["n_snp"]
    af, maf, mr = (np.empty(L, np.float64) for _ in range(3))
    _lib.check(_lib.lib().snpgpu_ws_snp_rate_freq(_lib._ptr(af), _lib._ptr(maf), _lib._ptr(mr)))
    rv = dict(AlleleFreq=af, MinorFreq=maf, MissingRate=mr)
    if with_id:
        rv.update(sample_id=ws["sample_id"], snp_id=ws["snp_id"])
    return rv


def snpgdsIBS(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
              maf=float("nan"), missing_rate=0.01, num_thread=1, useMatrix=False, verbose=True, device=0):
    ws = _init_file2("Identity-By-State (IBS) analysis on genotypes:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    if not isinstance(useMatrix, bool):
        raise TypeError("is.logical(useMatrix) is not TRUE")
    out = _tri_or_full(ws["n_samp"], useMatrix)
    _lib.check(_lib.lib().snpgpu_gnrIBSAve(ws["num_thread"], int(useMatrix), int(verbose), _lib._ptr(out)))
    return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], ibs=out)


def snpgdsIBSNum(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                 maf=float("nan"), missing_rate=0.01, num_thread=1, verbose=True, device=0):
    ws = _init_file2("Identity-By-State (IBS) analysis on genotypes:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    n = ws["n_samp"]
    o = [np.empty((n, n), np.int32) for _ in range(3)]
    _lib.check(_lib.lib().snpgpu_gnrIBSNum(ws["num_thread"], int(verbose), *[_lib._ptr(x) for x in o]))
    return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], ibs0=o[0], ibs1=o[1], ibs2=o[2])


def _family_codes(family_id, sample_id, ws, verbose):
    """family.id of snpgdsIBDKING (R/IBD.R:350-372) -> int32 codes for the ABI (-1 = NA), or None when no family is given"""
    n = ws["n_samp"]
    if family_id is None:
        if verbose:
            print("No family is specified, and all individuals are treated as singletons.")
        return None
    family_id = np.asarray(family_id)
    if n != len(family_id):
        raise ValueError("'length(family.id)' should be the number of samples.")
    if sample_id is not None:
        # family.id[match(sample.id, ws$sample.id)] (R/IBD.R:356-357), reproduced as it stands: the vector is
        # re-indexed by the position of each requested sample in the dataset-ordered working set
        ws_ids = np.asarray(ws["sample_id"])
        order = np.argsort(ws_ids, kind="stable")
        family_id = family_id[order[np.searchsorted(ws_ids[order], np.asarray(sample_id))]]
    # as.integer(as.factor(family.id)): every non-NA value is a level (negative integers too); "" and NA -> NA
    # (R/IBD.R:359-364).  -1 is only the ABI's code for NA after the factorisation.
    fam = np.full(n, -1, np.int32)
    if family_id.dtype.kind in "fc":
        good = ~np.isnan(family_id.astype(float))
    elif family_id.dtype.kind in "US":
        good = family_id != ""
    elif family_id.dtype.kind == "O":
        good = np.array([x is not None and x != "" for x in family_id])
    else:
        good = np.ones(n, bool)
    if good.any():
        _, codes = np.unique(family_id[good], return_inverse=True)
        fam[good] = codes.astype(np.int32) + 1
    _cat(verbose, "# of families: %d, and within- and between-family "
         "relationship are estimated differently." % len(np.unique(fam[fam >= 0])))
    return fam


def snpgdsIBDKING(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                  maf=float("nan"), missing_rate=0.01, type="KING-robust", family_id=None,
                  num_thread=1, useMatrix=False, verbose=True, device=0):
    ws = _init_file2("IBD analysis (KING method of moment) on genotypes:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    if type not in ("KING-robust", "KING-homo"):
        raise ValueError("'arg' should be one of 'KING-robust', 'KING-homo'")   # match.arg
    n = ws["n_samp"]
    fam = _family_codes(family_id, sample_id, ws, verbose and type == "KING-robust")
    a, b = _tri_or_full(n, useMatrix), _tri_or_full(n, useMatrix)
    rv = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], afreq=None)
    if type == "KING-homo":
        _cat(verbose, "Relationship inference in a homogeneous population.")
        _lib.check(_lib.lib().snpgpu_gnrIBD_KING_Homo(ws["num_thread"], int(useMatrix), int(verbose),
                                                      _lib._ptr(a), _lib._ptr(b)))
        rv.update(k0=a, k1=b)
    else:
        _cat(verbose, "Relationship inference in the presence of population stratification.")
        _lib.check(_lib.lib().snpgpu_gnrIBD_KING_Robust(_lib._ptr(fam), ws["num_thread"], int(useMatrix),
                                                        int(verbose), _lib._ptr(a), _lib._ptr(b)))
        rv.update(IBS0=a, kinship=b)
    return rv


def snpgdsGRM(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
              maf=float("nan"), missing_rate=0.01, method="GCTA", num_thread=1, useMatrix=False,
              out_fn=None, out_prec="double", out_compress="LZMA_RA", with_id=True, verbose=True, device=0):
    """snpgdsGRM (R/IBD.R:543-615).  out_fn: the reference writes a GDS file (FileFormat SNPRELATE_OUTPUT) through
    gdsfmt; gdsfmt is not available to this Python mirror, which stores THE SAME NODES (command, sample.id, snp.id,
    grm, avg_val) in a numpy archive under the given name -- readable by snpgdsMergeGRM here, NOT by the reference
    (and the reference's files are not readable here).  out_prec "double" / "single" selects the stored element
    type as in the reference; out_compress is accepted for signature compatibility and has no effect on the archive."""
    if out_prec not in ("double", "single"):
        raise ValueError("'arg' should be one of 'double', 'single'")     # match.arg
    all_methods = ("GCTA", "Eigenstrat", "EIGMIX", "Weighted", "Corr", "IndivBeta")
    if method not in all_methods:
        raise ValueError("'arg' should be one of " + ", ".join("'%s'" % m for m in all_methods))
    if method == "Weighted":          # R/IBD.R:552-556
        method = "EIGMIX"
    mtxt = {"Corr": "Scaled GCTA (correlation)", "EIGMIX": "EIGMIX / Weighted GCTA"}.get(method, method)
    ws = _init_file2("Genetic Relationship Matrix (GRM, %s):" % mtxt, gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    n = ws["n_samp"]
    # "Corr" always returns a full matrix (genPCA.cpp:1658); the output file always holds full rows (grm_save_to_gds)
    packed = bool(useMatrix) and method != "Corr" and out_fn is None
    out = _tri_or_full(n, packed)
    _lib.check(_lib.lib().snpgpu_gnrGRM(ws["num_thread"], method.encode(), int(packed), int(verbose),
                                        _lib._ptr(out)))
    avg = ctypes.c_double(0)
    if method == "IndivBeta":
        _lib.check(_lib.lib().snpgpu_gnrGRM_avg_val(ctypes.byref(avg)))
    if out_fn is not None:            # R/IBD.R:567-586,609-613: nodes of the SNPRELATE_OUTPUT file, nothing returned
        nodes = {"command": np.array(["snpgdsGRM", ":method = " + method]), "sample.id": ws["sample_id"],
                 "snp.id": ws["snp_id"], "grm": out if out_prec == "double" else out.astype(np.float32)}
        if method == "IndivBeta":
            nodes["avg_val"] = avg.value
        _gds.write_output(out_fn, nodes)
        return None
    if with_id:
        rv = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], method=method, grm=out)
        if method == "IndivBeta":
            rv["avg_val"] = avg.value
        return rv
    return out


def write_sparse_grm(prefix, sample_id, idx1, idx2, value, diag, samp_sel=None):
    """The text files of snpgdsGRMPairs(out_fn=prefix), from host arrays:
        prefix.grm.id   one line per sample: the id twice, tab-separated (family id, individual id)
        prefix.grm.sp   one line per stored entry, `row<TAB>col<TAB>value`: 0-based indices into prefix.grm.id with row >= col, sorted by
                        row, then by col, so the diagonal line `i i diag[i]` closes the lines of row i; values as %.17g, which reads
                        back to the same double
    idx1 < idx2 index sample_id; a pair becomes the line idx2, idx1.  samp_sel (a mask over sample_id): prefix.grm.id lists the selected
    samples only, the indices refer to that list, and the pairs must lie among them."""
    ids = np.asarray(sample_id)
    n = ids.size
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    value, diag = np.asarray(value, np.float64), np.asarray(diag, np.float64)
    if not (idx1.shape == idx2.shape == value.shape and idx1.ndim == 1) or diag.shape != (n,):
        raise ValueError("idx1, idx2 and value should have one entry per pair, diag one per sample")
    if idx1.size and not ((0 <= idx1).all() and (idx1 < idx2).all() and (idx2 < n).all()):
        raise ValueError("pairs should be 0 <= idx1 < idx2 < %d" % n)
    keep = np.ones(n, bool) if samp_sel is None else np.asarray(samp_sel) != 0
    if keep.shape != (n,):
        raise ValueError("'samp_sel' should have %d entries" % n)
    if not (keep[idx1].all() and keep[idx2].all()):
        raise ValueError("a pair holds a sample that 'samp_sel' leaves out")
    new = np.cumsum(keep) - 1                                   # index within the list of selected samples
    own = np.flatnonzero(keep)
    row = np.concatenate([new[idx2], new[own]])
    col = np.concatenate([new[idx1], new[own]])
    val = np.concatenate([value, diag[own]])
    order = np.lexsort((col, row))
    with open(prefix + ".grm.id", "w") as f:
        f.writelines("%s\t%s\n" % (s, s) for s in ids[own].tolist())
    with open(prefix + ".grm.sp", "w") as f:
        f.writelines("%d\t%d\t%.17g\n" % t for t in zip(row[order].tolist(), col[order].tolist(), val[order].tolist()))


def _pairs_samp_sel(fn, samp_sel, n, dense=None):
    """samp_sel of the calls that select pairs on the device -- a logical vector over the n working samples or strictly increasing
    0-based indices -- as a uint8 mask, None for all.  dense: the calls whose matrices serve any other selection (for the message)."""
    if samp_sel is None:
        return None
    sel = np.asarray(samp_sel)
    if sel.dtype.kind == "b" and sel.shape == (n,):
        mask = sel
    elif sel.dtype.kind in "iu" and sel.ndim == 1 and (sel.size == 0 or (sel.min() >= 0 and sel.max() < n and np.all(np.diff(sel) > 0))):
        mask = np.zeros(n, bool)
        mask[sel] = True
    else:
        msg = "%s: 'samp.sel' should be a logical vector over the %d samples or strictly increasing indices" % (fn, n)
        if dense:
            msg += "; for a permuting or repeating selection use snpgdsIBDSelection on the matrices of %s" % dense
        raise ValueError(msg)
    return np.ascontiguousarray(mask, np.uint8)


def snpgdsGRMPairs(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                   maf=float("nan"), missing_rate=0.01, method="GCTA", cutoff=0.05, samp_sel=None, num_thread=1,
                   with_id=True, out_fn=None, verbose=True, device=0):
    """The sparse GRM of snpgdsGRM(gdsobj, ..., method) without its n x n matrix: every sample's own entry and the pairs at or above
    `cutoff` (a non-finite cutoff: every pair; a NaN entry is never a pair).  No reference counterpart.  The sums are accumulated once
    on the GPU as for snpgdsGRM and only the diagonal and the selected pairs come back (snpgpu_gnrGRMPairs), each with the value
    snpgdsGRM would hold at that place.  method: "GCTA", "Eigenstrat", "EIGMIX" (= "Weighted"), "IndivBeta"; "Corr" is refused -- its
    entries need the diagonal of every column, which a row panel of the sums does not hold.  samp_sel: a logical vector over the
    working samples or strictly increasing 0-based indices; it restricts the pairs, not `diag`.
    Returns sample_id, snp_id, method, ID1, ID2 (sample ids), idx1 < idx2 (0-based into sample_id, ordered by idx1, then idx2), value,
    diag [n], n_pairs and, for IndivBeta, avg_val; with_id=False leaves the ids out.  out_fn="prefix" also writes prefix.grm.id and
    prefix.grm.sp (write_sparse_grm): sample ids, and `row col value` lines of the lower triangle with the diagonal.  That is the
    layout sparse-GRM readers of the GCTA family are understood to take; it has not been checked against such a program."""
    all_methods = ("GCTA", "Eigenstrat", "EIGMIX", "Weighted", "Corr", "IndivBeta")
    if method not in all_methods:
        raise ValueError("'arg' should be one of " + ", ".join("'%s'" % m for m in all_methods))
    if method == "Corr":
        raise ValueError("snpgdsGRMPairs: method 'Corr' is not built for the sparse GRM (its entries need the diagonal of every column); "
                         "use snpgdsGRM")
    if method == "Weighted":          # R/IBD.R:552-556
        method = "EIGMIX"
    if isinstance(cutoff, (bool, np.bool_)) or not isinstance(cutoff, (int, float, np.integer, np.floating)):
        raise TypeError("is.numeric(cutoff) is not TRUE")
    mtxt = {"EIGMIX": "EIGMIX / Weighted GCTA"}.get(method, method)
    ws = _init_file2("Genetic Relationship Matrix (GRM, %s):" % mtxt, gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    n = ws["n_samp"]
    mask = _pairs_samp_sel("snpgdsGRMPairs", samp_sel, n)
    L = _lib.lib()
    found = ctypes.c_int64(0)
    _lib.check(L.snpgpu_gnrGRMPairs(method.encode(), float(cutoff), _lib._ptr(mask), ws["num_thread"], int(bool(verbose)), ctypes.byref(found)))
    m = found.value
    i1, i2, val, diag = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64), np.empty(n, np.float64)
    avg = ctypes.c_double(0)
    _lib.check(L.snpgpu_gnrGRMPairs_get(_lib._ptr(i1), _lib._ptr(i2), _lib._ptr(val), _lib._ptr(diag), ctypes.byref(avg)))
    ids = np.asarray(ws["sample_id"])
    if out_fn is not None:
        write_sparse_grm(out_fn, ids, i1, i2, val, diag, mask)
    rv = dict(method=method, idx1=i1, idx2=i2, value=val, diag=diag, n_pairs=m)
    if with_id:
        rv.update(sample_id=ws["sample_id"], snp_id=ws["snp_id"], ID1=ids[i1], ID2=ids[i2])
    if method == "IndivBeta":
        rv["avg_val"] = avg.value
    _cat(verbose, "%d pair%s selected" % (m, "" if m == 1 else "s"))
    return rv


def snpgdsMergeGRM(filelist, out_fn=None, weight=None, verbose=True, device=0):
    """R/IBD.R:624-741 -> gnrGRMMerge (src/genPCA.cpp:1721-1853): combine the GRMs that snpgdsGRM(out_fn=) stored
    for disjoint SNP sets.  weight: None (by SNP count), a bool per file (False = subtract that SNP set) or numbers."""
    if isinstance(filelist, str) or len(filelist) == 0:
        raise ValueError("'filelist' should be a non-empty list of file names")
    if weight is not None and len(weight) != len(filelist):
        raise ValueError("length(weight) == length(filelist) is not TRUE")
    _cat(verbose, "GRM merging:")
    files = []
    for fn in filelist:
        f = _gds.read_output(fn)
        files.append(f)
        _cat(verbose, "    open '%s' (%s variants)" % (fn, format(len(f["snp.id"]), ",")))
    sampid = files[0]["sample.id"]
    dm = files[0]["grm"].shape
    if len(dm) != 2 or dm[0] != dm[1]:
        raise ValueError("'%s' has an invalid GRM matrix." % filelist[0])
    cmd = [str(x) for x in files[0]["command"]]
    if cmd[0] != "snpgdsGRM":
        raise ValueError("The GDS files should be created by snpgdsGRM()")
    for fn, f in zip(filelist, files):
        if [str(x) for x in f["command"]] != cmd:
            raise ValueError("'%s' has a different command." % fn)
        if f["grm"].shape != dm:
            raise ValueError("'%s' has a different GRM matrix." % fn)
    if weight is None or np.asarray(weight).dtype == np.bool_:
        num = np.array([float(len(f["snp.id"])) for f in files])
        if weight is not None:
            num[~np.asarray(weight, bool)] *= -1
        weight = num / num.sum()
    weight = np.ascontiguousarray(weight, np.float64)
    _cat(verbose, "Weight: " + ", ".join("%g" % w for w in weight))
    sid = np.array([], dtype=files[0]["snp.id"].dtype)
    for w, f in zip(weight, files):                             # R/IBD.R:704-712
        sid = np.concatenate([sid, f["snp.id"]]) if w >= 0 else sid[~np.isin(sid, f["snp.id"])]
    beta = cmd[1] == ":method = IndivBeta"
    out, avg = _lib.grm_merge([f["grm"] for f in files], weight, cmd[1], [float(f["avg_val"]) for f in files] if beta else None,
                              device=device)
    if out_fn is not None:
        _cat(verbose, "Output: " + out_fn)
        nodes = {"command": np.array(cmd), "sample.id": sampid, "snp.id": sid, "grm": out}
        if beta:
            nodes["avg_val"] = avg
        _gds.write_output(out_fn, nodes)
        return None
    rv = dict(sample_id=sampid, snp_id=sid, grm=out)
    if beta:
        rv["avg_val"] = avg
    return rv


def snpgdsPCA(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
              maf=float("nan"), missing_rate=0.01, algorithm="exact", eigen_cnt=None, num_thread=1,
              bayesian=False, need_genmat=False, genmat_only=False, eigen_method="DSPEVX",
              aux_dim=None, iter_num=10, aux_mat=None, verbose=True, device=0):
    """R/PCA.R:12-93.  algorithm = "exact" (covariance + eigen-decomposition) or "randomized" (Galinsky's
    fast PCA, CRandomPCA); aux_mat ([aux_dim][n_samp]) replaces R's rnorm(aux.dim * n.samp) when given."""
    if algorithm not in ("exact", "randomized"):
        raise ValueError("'arg' should be one of 'exact', 'randomized'")
    if eigen_cnt is None:
        eigen_cnt = 32 if algorithm == "exact" else 16          # R/PCA.R:15
    if eigen_method not in ("DSPEVX", "DSPEV"):
        raise ValueError("'arg' should be one of 'DSPEVX', 'DSPEV'")
    ws = _init_file2("Principal Component Analysis (PCA) on genotypes:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    n = ws["n_samp"]
    if algorithm == "randomized":
        if eigen_cnt <= 0:
            eigen_cnt = n
        if aux_dim is None:
            aux_dim = int(eigen_cnt) * 2                        # R/PCA.R:16
        if aux_mat is None:
            aux_mat = np.random.standard_normal((int(aux_dim), n))
        aux_mat = np.ascontiguousarray(aux_mat, np.float64)
        if aux_mat.shape != (int(aux_dim), n):
            raise ValueError("'aux.mat' should be aux.dim x n.samp")
        _cat(verbose, "    # of principal components: %d\n    starting from a random matrix [%d x %d]"
             % (eigen_cnt, aux_dim, n))
        d = np.empty(n, np.float64)
        ev = np.empty((int(eigen_cnt), n), np.float64)
        tr2 = ctypes.c_double(0)
        _lib.check(_lib.lib().snpgpu_gnrPCA_randomized(int(eigen_cnt), int(aux_dim), int(iter_num), _lib._ptr(aux_mat),
                                                       ws["num_thread"], int(verbose), _lib._ptr(d), _lib._ptr(ev),
                                                       ctypes.byref(tr2)))
        vp = 2 * d * d / tr2.value                              # R/PCA.R:82
        return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], eigenval=(n - 1) * vp, eigenvect=ev.T,
                    varprop=vp, TraceXTX=tr2.value, Bayesian=False)
    if genmat_only:
        need_genmat = True
    if eigen_cnt <= 0:
        eigen_cnt = n
    eigen_cnt = min(int(eigen_cnt), n)
    _cat(verbose, "    # of principal components: %d" % eigen_cnt)
    genmat = np.empty((n, n), np.float64) if need_genmat else None
    tr, trv = ctypes.c_double(0), ctypes.c_double(0)
    eigval = eigvec = None
    if not genmat_only:
        eigval = np.empty(n, np.float64)
        eigvec = np.empty((eigen_cnt, n), np.float64)   # column-major n x k
    _lib.check(_lib.lib().snpgpu_gnrPCA(eigen_cnt, ws["num_thread"], int(bool(bayesian)), int(verbose),
                                        ctypes.byref(tr), _lib._ptr(genmat), _lib._ptr(eigval),
                                        _lib._ptr(eigvec), ctypes.byref(trv)))
    return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], eigenval=eigval,
                eigenvect=None if eigvec is None else eigvec.T,
                varprop=None if eigval is None else eigval / trv.value,
                TraceXTX=tr.value, Bayesian=bool(bayesian), genmat=genmat)


def _init_file(gdsobj, sample_id=None, snp_id=None, device=0):
    """.InitFile, R/Internal.R:64-160: sample / SNP selection and gnrSetGenoSpace only (no filters)."""
    return _init_file2(None, gdsobj, sample_id, snp_id, autosome_only=False, remove_monosnp=False,
                       maf=float("nan"), missing_rate=float("nan"), num_thread=1, verbose=False, device=device)


def snpgdsPCACorr(pcaobj, gdsobj, snp_id=None, eig_which=None, num_thread=1, with_id=True, outgds=None,
                  verbose=True, device=0):
    """SNP correlations with the principal components (R/PCA.R:100-180 -> gnrPCACorr, src/genPCA.cpp:1455-1484).
    pcaobj: result of snpgdsPCA / snpgdsEIGMIX, or (sample_id, eigenvect [n][k]).  Returns snpcorr [k][n_snp]."""
    if outgds is not None:
        if not isinstance(outgds, str):
            raise TypeError("is.null(outgds) | is.character(outgds) is not TRUE")
        with_id = True
    if isinstance(pcaobj, dict):
        sampid, eigenvect = pcaobj["sample_id"], np.asarray(pcaobj["eigenvect"], np.float64)
    else:
        sampid, eigenvect = pcaobj
        eigenvect = np.asarray(eigenvect, np.float64)
    ws = _init_file(gdsobj, sampid, snp_id, device)
    if len(sampid) != eigenvect.shape[0]:
        raise ValueError("Internal error: the number of samples should be equal to the number of rows in 'eigenvect'.")
    if num_thread is None or num_thread <= 0:
        raise ValueError("num.thread > 0 is not TRUE")
    if eig_which is None:
        eig_which = np.arange(eigenvect.shape[1])
    else:
        eig_which = np.asarray(eig_which, dtype=np.int64) - 1          # R indices are 1-based
    _cat(verbose, "SNP Correlation:\n    # of samples: %d\n    # of SNPs: %d" % (ws["n_samp"], ws["n_snp"]))
    ev = np.ascontiguousarray(eigenvect[:, eig_which].T)               # [k][n] = n x k column-major
    out = np.empty((ws["n_snp"], ev.shape[0]), np.float64)             # k x n_snp column-major
    _lib.check(_lib.lib().snpgpu_gnrPCACorr(ev.shape[0], _lib._ptr(ev), int(num_thread), int(verbose), _lib._ptr(out)))
    if outgds is not None:
        # R/PCA.R:152-163: nodes sample.id, snp.id and "correlation" as packedreal16 (int16 steps of 1e-4, i.e. the
        # values read back are round(corr, 4), inst/unitTests/test_rel.R:148-152); nothing is returned
        _cat(verbose, "Creating '%s' ..." % outgds)
        q = np.where(np.isnan(out.T), np.nan, np.clip(np.round(out.T / 1e-4), -32767, 32767) * 1e-4)
        _gds.write_output(outgds, {"sample.id": np.asarray(sampid), "snp.id": ws["snp_id"], "correlation": q})
        return None
    if with_id:
        return dict(sample_id=np.asarray(sampid), snp_id=ws["snp_id"], snpcorr=out.T)
    return out.T


def snpgdsPCASNPLoading(pcaobj, gdsobj, num_thread=1, verbose=True, device=0):
    """SNP loadings (R/PCA.R:187-236 -> gnrPCASNPLoading, src/genPCA.cpp:1488-1531) of a snpgdsPCA result.
    Returns snploading [k][n_snp], avgfreq [n_snp] (mean genotype), scale [n_snp]."""
    if pcaobj.get("eigenval") is None or pcaobj.get("eigenvect") is None:
        raise ValueError("!is.null(pcaobj$eigenval), !is.null(pcaobj$eigenvect) are not all TRUE")
    ws = _init_file(gdsobj, pcaobj["sample_id"], pcaobj["snp_id"], device)
    ev = np.ascontiguousarray(np.asarray(pcaobj["eigenvect"], np.float64).T)    # [k][n]
    k = ev.shape[0]
    eigval = np.ascontiguousarray(np.asarray(pcaobj["eigenval"], np.float64)[:k])
    if "afreq" in pcaobj and "TraceXTX" not in pcaobj:
        # snpgdsEigMixClass, R/PCA.R:215-229 -> gnrEigMixSNPLoading, src/genEIGMIX.cpp:739-775
        if pcaobj.get("diagadj", False):
            raise ValueError("Please run `snpgdsEIGMIX(, diagadj=FALSE)` for projecting new samples.")
        af = np.ascontiguousarray(pcaobj["afreq"], np.float64)
        load = np.empty((ws["n_snp"], k), np.float64)
        _lib.check(_lib.lib().snpgpu_gnrEigMixSNPLoading(_lib._ptr(eigval), _lib._ptr(ev), k, _lib._ptr(af), int(num_thread),
                                                         int(verbose), _lib._ptr(load)))
        return dict(sample_id=np.asarray(pcaobj["sample_id"]), snp_id=np.asarray(pcaobj["snp_id"]),
                    eigenval=np.asarray(pcaobj["eigenval"]), snploading=load.T, afreq=af)
    _cat(verbose, "SNP Loading:\n    # of samples: %d\n    # of SNPs: %d\n    using the top %d eigenvectors"
         % (ws["n_samp"], ws["n_snp"], k))
    load = np.empty((ws["n_snp"], k), np.float64)
    af = np.empty(ws["n_snp"], np.float64)
    sc = np.empty(ws["n_snp"], np.float64)
    _lib.check(_lib.lib().snpgpu_gnrPCASNPLoading(_lib._ptr(eigval), _lib._ptr(ev), k, float(pcaobj["TraceXTX"]),
                                                  int(num_thread), int(bool(pcaobj.get("Bayesian", False))), int(verbose),
                                                  _lib._ptr(load), _lib._ptr(af), _lib._ptr(sc)))
    return dict(sample_id=np.asarray(pcaobj["sample_id"]), snp_id=np.asarray(pcaobj["snp_id"]),
                eigenval=np.asarray(pcaobj["eigenval"]), snploading=load.T, TraceXTX=pcaobj["TraceXTX"],
                Bayesian=bool(pcaobj.get("Bayesian", False)), avgfreq=af, scale=sc)


def snpgdsPCASampLoading(loadobj, gdsobj, sample_id=None, num_thread=1, verbose=True, device=0):
    """Project samples onto existing principal components (R/PCA.R:245-310 -> gnrPCASampLoading,
    src/genPCA.cpp:1535-1562).  Returns eigenvect [n_samp][k] (eigenval / varprop are NaN as in the reference)."""
    ws = _init_file(gdsobj, sample_id, loadobj["snp_id"], device)
    sl = np.asarray(loadobj["snploading"], np.float64)                  # [k][n_snp]
    k = sl.shape[0]
    if "avgfreq" not in loadobj:
        # snpgdsEigMixSNPLoadingClass, R/PCA.R:288-300 -> gnrEigMixSampLoading, src/genEIGMIX.cpp:777-803
        sqrt_eigval = np.sqrt(1 / np.asarray(loadobj["eigenval"], np.float64)[:k])
        sload = np.ascontiguousarray((sl * sqrt_eigval[:, None]).T)
        af = np.ascontiguousarray(loadobj["afreq"], np.float64)
        out = np.empty((k, ws["n_samp"]), np.float64)
        _lib.check(_lib.lib().snpgpu_gnrEigMixSampLoading(k, _lib._ptr(sload), _lib._ptr(af), int(num_thread), int(verbose),
                                                          _lib._ptr(out)))
        return dict(sample_id=ws["sample_id"], snp_id=np.asarray(loadobj["snp_id"]),
                    eigenval=np.full(ws["n_samp"], np.nan), eigenvect=out.T, afreq=af)
    _cat(verbose, "Sample Loading:\n    # of samples: %d\n    # of SNPs: %d\n    using the top %d eigenvectors"
         % (ws["n_samp"], ws["n_snp"], k))
    # prepare post-eigenvectors, R/PCA.R:281-285
    ss = (len(loadobj["sample_id"]) - 1) / loadobj["TraceXTX"]
    sqrt_eigval = np.sqrt(ss / np.asarray(loadobj["eigenval"], np.float64)[:k])
    sload = np.ascontiguousarray((sl * sqrt_eigval[:, None]).T)         # [n_snp][k] = k x n_snp column-major
    af = np.ascontiguousarray(loadobj["avgfreq"], np.float64)
    sc = np.ascontiguousarray(loadobj["scale"], np.float64)
    n = ws["n_samp"]
    out = np.empty((k, n), np.float64)                                  # n x k column-major
    _lib.check(_lib.lib().snpgpu_gnrPCASampLoading(k, _lib._ptr(sload), _lib._ptr(af), _lib._ptr(sc), int(num_thread),
                                                   int(verbose), _lib._ptr(out)))
    nan = np.full(n, np.nan)
    return dict(sample_id=ws["sample_id"], snp_id=np.asarray(loadobj["snp_id"]), eigenval=nan, eigenvect=out.T,
                varprop=nan.copy(), TraceXTX=loadobj["TraceXTX"], Bayesian=loadobj.get("Bayesian", False), genmat=None)


def snpgdsIBDMoM(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                 maf=float("nan"), missing_rate=0.01, allele_freq=None, kinship=False,
                 kinship_constraint=False, num_thread=1, useMatrix=False, verbose=True, device=0):
    """PLINK method of moments (R/IBD.R:22-68 -> gnrIBD_PLINK, src/genIBS.cpp:558-639)."""
    ws = _init_file2("IBD analysis (PLINK method of moment) on genotypes:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device,
                     allele_freq=allele_freq)
    allele_freq = ws["allele_freq"]       # dataset order, filtered with gnrSelSNP_Base_Ex (R/Internal.R:355-452)
    n = ws["n_samp"]
    k0, k1 = _tri_or_full(n, useMatrix), _tri_or_full(n, useMatrix)
    af = np.empty(ws["n_snp"], np.float64)
    _lib.check(_lib.lib().snpgpu_gnrIBD_PLINK(ws["num_thread"], _lib._ptr(allele_freq), int(bool(kinship_constraint)),
                                              int(bool(useMatrix)), int(verbose), _lib._ptr(k0), _lib._ptr(k1),
                                              _lib._ptr(af)))
    af[af < 0] = np.nan
    ans = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], afreq=af, k0=k0, k1=k1)
    if kinship:
        ans["kinship"] = 0.5 * (1 - k0 - k1) + 0.25 * k1
    return ans


def snpgdsDiss(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
               maf=float("nan"), missing_rate=0.01, num_thread=1, verbose=True, device=0):
    """Individual dissimilarity (R/IBD.R:432-450 -> gnrDiss, src/genIBS.cpp:652-683): the full n x n matrix.

    R's result carries the class "snpgdsDissClass"; here it is a dict like every other result."""
    ws = _init_file2("Individual dissimilarity analysis on genotypes:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    n = ws["n_samp"]
    d = np.empty((n, n), np.float64)
    _lib.check(_lib.lib().snpgpu_gnrDiss(ws["num_thread"], int(verbose), _lib._ptr(d)))
    return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], diss=d)


def snpgdsIndivBeta(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                    maf=float("nan"), missing_rate=0.01, method="weighted", inbreeding=True, num_thread=1,
                    with_id=True, useMatrix=False, verbose=True, device=0):
    if method != "weighted":
        raise ValueError("'arg' should be one of 'weighted'")
    ws = _init_file2("Individual Inbreeding and Relatedness (beta estimator):", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
    out = _tri_or_full(ws["n_samp"], useMatrix)
    avg = ctypes.c_double(0)
    _lib.check(_lib.lib().snpgpu_gnrIBD_Beta(int(bool(inbreeding)), ws["num_thread"], int(bool(useMatrix)),
                                             int(verbose), _lib._ptr(out), ctypes.byref(avg)))
    if with_id:
        return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], inbreeding=bool(inbreeding), beta=out,
                    avg_val=avg.value)
    return out


def snpgdsEIGMIX(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                 maf=float("nan"), missing_rate=0.01, num_thread=1, eigen_cnt=32, diagadj=True, ibdmat=False,
                 verbose=True, device=0):
    ws = _init_file2("Eigen-analysis on genotypes:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp,
                     maf, missing_rate, num_thread, verbose, device)
    n = ws["n_samp"]
    if eigen_cnt < 0:
        eigen_cnt = n
    k = min(int(eigen_cnt), n)
    ibd = np.empty((n, n), np.float64) if ibdmat else None
    eigval = np.empty(n, np.float64) if k > 0 else None
    eigvec = np.empty((k, n), np.float64) if k > 0 else None
    af = np.empty(ws["n_snp"], np.float64)
    _lib.check(_lib.lib().snpgpu_gnrEigMix(k, ws["num_thread"], int(bool(diagadj)), int(verbose), _lib._ptr(ibd),
                                           _lib._ptr(eigval), _lib._ptr(eigvec), _lib._ptr(af)))
    return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], eigenval=eigval,
                eigenvect=None if eigvec is None else eigvec.T, afreq=af, ibd=ibd, diagadj=bool(diagadj))


LD_METHODS = ("composite", "r", "dprime", "corr", "cov")


def snpgdsLDMat(gdsobj, sample_id=None, snp_id=None, slide=250, method="composite", mat_trim=False, num_thread=1,
                with_id=True, verbose=True, device=0):
    """Linkage disequilibrium between SNP pairs (R/LD.R:53-92 -> gnrLDMat, src/genLD.cpp:957-1010).
    slide <= 0, None or NaN: the full n_snp x n_snp matrix; otherwise LD[k - 1, i] = LD(i, i + k), k = 1 ... slide (clamped to
    n_snp): a slide x n_snp matrix with NaN past the last SNP, or slide x (n_snp - slide) with mat_trim.  Returns
    dict(sample_id, snp_id, LD, slide), or the bare matrix with with_id=False."""
    if isinstance(slide, (bool, np.bool_)) or not isinstance(slide, (int, float, np.integer, np.floating, type(None))):
        raise TypeError("is.numeric(slide) is not TRUE")
    if num_thread is None or not isinstance(num_thread, (int, float, np.integer, np.floating)) or not num_thread > 0:
        raise ValueError("is.numeric(num.thread), num.thread > 0 is not TRUE")
    if not isinstance(mat_trim, (bool, np.bool_)):
        raise TypeError("is.logical(mat.trim) is not TRUE")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    if method not in LD_METHODS:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in LD_METHODS))
    code = LD_METHODS.index(method) + 1
    ws = _init_file(gdsobj, sample_id, snp_id, device)
    n_snp = ws["n_snp"]
    if slide is None or (isinstance(slide, (float, np.floating)) and math.isnan(slide)):
        slide = -1
    slide = int(slide)
    if slide > n_snp:
        slide = n_snp
    if verbose:
        print("Linkage Disequilibrium (LD) estimation on genotypes:")
        print("    # of samples: %d" % ws["n_samp"])
        print("    # of SNPs: %d" % n_snp)
        print("    using %d thread%s" % (int(num_thread), "" if int(num_thread) == 1 else "s"))
        if slide > 0:
            print("    sliding window size: %d" % slide)
        print("    method: %s" % ("composite", "R", "D'", "correlation", "covariance")[code - 1])
    rows, cols = _lib.ld_out_dims(n_snp, slide, mat_trim)
    out = np.empty((cols, rows), np.float64)          # rows x cols column-major
    _lib.check(_lib.lib().snpgpu_gnrLDMat(code, slide, int(bool(mat_trim)), int(num_thread), int(bool(verbose)), _lib._ptr(out)))
    m = out.T
    if with_id:
        return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], LD=m, slide=slide)
    return m


IBDMLE_METHODS = ("EM", "downhill.simplex", "Jacquard")
RELATEDNESS = {"": None, "self": (0.0, 0.0), "fullsib": (0.25, 0.5), "offspring": (0.0, 1.0), "halfsib": (0.5, 0.5),
               "cousin": (0.75, 0.25), "unrelated": (1.0, 0.0)}


def snpgdsIBDMLE(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True, maf=float("nan"),
                 missing_rate=0.01, kinship=False, kinship_constraint=False, allele_freq=None, method="EM", max_niter=1000,
                 reltol=math.sqrt(np.finfo(float).eps), coeff_correct=True, out_num_iter=True, num_thread=1, verbose=True,
                 device=0):
    """IBD coefficients by maximum likelihood (R/IBD.R:79-156 -> gnrIBD_MLE, src/genIBD.cpp:1465-1548), method "EM" only.
    Returns dict(sample_id, snp_id, afreq, k0, k1, niter[, kinship]): k0 / k1 / niter are n x n with 0 on the diagonal,
    niter is None when out_num_iter is False; afreq < 0 becomes NaN.  kinship_constraint is accepted and has no effect, as in
    the reference (Est_PLINK_Kinship is called without the constraint)."""
    if method not in IBDMLE_METHODS:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in IBDMLE_METHODS))
    if method != "EM":
        raise NotImplementedError('snpgdsIBDMLE: method "%s" is not built on the GPU path (only "EM")' % method)
    for name, v in (("kinship", kinship), ("kinship.constraint", kinship_constraint), ("coeff.correct", coeff_correct),
                    ("out.num.iter", out_num_iter)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    for name, v in (("max.niter", max_niter), ("reltol", reltol)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("is.numeric(%s) is not TRUE" % name)
    ws = _init_file2("Identity-By-Descent analysis (MLE) on genotypes:", gdsobj, sample_id, snp_id, autosome_only,
                     remove_monosnp, maf, missing_rate, num_thread, verbose, device, allele_freq=allele_freq)
    n, L = ws["n_samp"], ws["n_snp"]
    if n < 2:
        raise ValueError("snpgdsIBDMLE: at least two samples are needed")
    if L < 1:
        raise ValueError("snpgdsIBDMLE: no SNP in the working dataset")
    af_in = ws["allele_freq"]
    if verbose and af_in is not None:
        print("Specifying allele frequencies, mean: %0.3f, sd: %0.3f" % (np.nanmean(af_in), np.nanstd(af_in, ddof=1)))
    k0 = np.empty((n, n), np.float64)
    k1 = np.empty((n, n), np.float64)
    niter = np.empty((n, n), np.int32) if out_num_iter else None
    af = np.empty(L, np.float64)
    _lib.check(_lib.lib().snpgpu_gnrIBD_MLE(_lib._ptr(af_in), int(bool(kinship_constraint)), int(max_niter), float(reltol),
                                            int(bool(coeff_correct)), 0, int(bool(out_num_iter)), ws["num_thread"],
                                            int(bool(verbose)), _lib._ptr(k0), _lib._ptr(k1), _lib._ptr(af),
                                            _lib._ptr(niter)))
    af[af < 0] = np.nan
    ans = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], afreq=af, k0=k0, k1=k1, niter=niter)
    if kinship:
        ans["kinship"] = 0.5 * (1 - k0 - k1) + 0.25 * k1
    return ans


def snpgdsIBDMLELogLik(gdsobj, ibdobj, k0=float("nan"), k1=float("nan"), relatedness="", device=0):
    """Log-likelihood of IBD coefficients (R/IBD.R:162-205 -> gnrIBD_LogLik / gnrIBD_LogLik_k01, src/genIBD.cpp:1289-1330):
    n x n, diagonal included.  relatedness presets override k0 / k1; with finite k0 and k1 every pair is evaluated at them,
    otherwise at the pair's own ibdobj["k0"], ibdobj["k1"]."""
    if not isinstance(ibdobj, dict) or not {"sample_id", "snp_id", "afreq", "k0", "k1"} <= set(ibdobj):
        raise TypeError("inherits(ibdobj, \"snpgdsIBDClass\") is not TRUE")
    if relatedness not in RELATEDNESS:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in RELATEDNESS))
    for name, v in (("k0", k0), ("k1", k1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("is.numeric(%s), is.vector(%s), length(%s) == 1L is not TRUE" % (name, name, name))
    if RELATEDNESS[relatedness] is not None:
        k0, k1 = RELATEDNESS[relatedness]
    ws = _init_file(gdsobj, ibdobj["sample_id"], ibdobj["snp_id"], device)
    afreq = np.ascontiguousarray(ibdobj["afreq"], np.float64)
    n = ws["n_samp"]
    # snpgpu_gnrIBD_LogLik reads one frequency per SNP and n x n coefficients of the working space
    if afreq.ndim != 1 or afreq.shape[0] != ws["n_snp"]:
        raise ValueError("'ibdobj$afreq' should have one entry per SNP of 'ibdobj$snp.id' (%d), not %s"
                         % (ws["n_snp"], afreq.shape))
    out = np.empty((n, n), np.float64)
    if np.isfinite(k0) and np.isfinite(k1):
        _lib.check(_lib.lib().snpgpu_gnrIBD_LogLik_k01(_lib._ptr(afreq), float(k0), float(k1), _lib._ptr(out)))
    else:
        m0 = np.ascontiguousarray(ibdobj["k0"], np.float64)
        m1 = np.ascontiguousarray(ibdobj["k1"], np.float64)
        if m0.shape != (n, n) or m1.shape != (n, n):
            raise ValueError("'ibdobj$k0' and 'ibdobj$k1' should be %d x %d matrices, not %s and %s" % (n, n, m0.shape, m1.shape))
        _lib.check(_lib.lib().snpgpu_gnrIBD_LogLik(_lib._ptr(afreq), _lib._ptr(m0), _lib._ptr(m1), _lib._ptr(out)))
    return out


def _check_mle_args(logical, numeric):
    for name, v in logical:
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    for name, v in numeric:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("is.numeric(%s) is not TRUE" % name)


def snpgdsIBDMLEPairs(gdsobj, sample1_id, sample2_id, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                      maf=float("nan"), missing_rate=0.01, kinship=False, kinship_constraint=False, allele_freq=None,
                      max_niter=1000, reltol=math.sqrt(np.finfo(float).eps), coeff_correct=True, out_num_iter=True, num_thread=1,
                      verbose=True, device=0, method="EM"):
    """IBD coefficients by maximum likelihood of the listed pairs (sample1_id[t], sample2_id[t]) only.  No reference
    counterpart: each pair's k0 / k1 / niter is what snpgdsIBDMLE puts at that matrix entry, but no n x n matrix is built and one
    wave works on each pair (snpgpu_gnrIBD_MLE_Pairs), so a few hundred pairs out of 100 000 samples -- the table of
    snpgdsIBDPairs -- are refined directly.  sample_id is the population: it defines the allele frequencies and the SNP filters as
    in snpgdsIBDMLE, and both ID lists must lie in it.  Returns dict(sample_id, snp_id, afreq, ID1, ID2, k0, k1, loglik, niter
    [, kinship]); loglik is the log-likelihood of the returned coefficients (after coeff_correct); niter is None when
    out_num_iter is False.  kinship_constraint is accepted and has no effect, as in snpgdsIBDMLE.

    method: "EM" (the default), "downhill.simplex" or "Jacquard", the three of the reference's snpgdsIBDMLE.
    "downhill.simplex" runs the reference's Nelder-Mead walk from EM's start values and returns the same dictionary; niter is
    then the walk's count of function evaluations.  "Jacquard" estimates the nine condensed identity coefficients by EM from
    D1 ... D8 = 0.01: the result has D1 ... D8 (D9 = 1 - their sum), loglik and niter, no k0 / k1, and with kinship=True
    kinship = D1 + 0.5 (D3 + D5 + D7) + 0.25 D8; coeff_correct has no effect.  Jacquard's likelihood table is not symmetric in the
    two samples, and, as the reference's table does (its MM / MM entry falls through to the default and is zeroed), it leaves out
    every SNP at which both samples are homozygous for the A allele."""
    _check_mle_args((("kinship", kinship), ("kinship.constraint", kinship_constraint), ("coeff.correct", coeff_correct),
                     ("out.num.iter", out_num_iter)), (("max.niter", max_niter), ("reltol", reltol)))
    if method not in IBDMLE_METHODS:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in IBDMLE_METHODS))
    id1, id2 = np.asarray(sample1_id).ravel(), np.asarray(sample2_id).ravel()
    if id1.shape != id2.shape:
        raise ValueError("snpgdsIBDMLEPairs: 'sample1.id' and 'sample2.id' should have the same length (%d and %d)"
                         % (id1.size, id2.size))
    if id1.size < 1:
        raise ValueError("snpgdsIBDMLEPairs: no pair is listed")
    ws = _init_file2("Identity-By-Descent analysis (MLE) on genotypes, listed pairs only:", gdsobj, sample_id, snp_id,
                     autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device, allele_freq=allele_freq)
    n, L = ws["n_samp"], ws["n_snp"]
    if n < 2:
        raise ValueError("snpgdsIBDMLEPairs: at least two samples are needed")
    if L < 1:
        raise ValueError("snpgdsIBDMLEPairs: no SNP in the working dataset")
    ids = np.asarray(ws["sample_id"])
    order = np.argsort(ids, kind="stable")
    idx = []
    for name, v in (("sample1.id", id1), ("sample2.id", id2)):
        pos = np.clip(np.searchsorted(ids[order], v), 0, n - 1)
        hit = ids[order][pos] == v
        if not hit.all():
            raise ValueError("snpgdsIBDMLEPairs: '%s' has a sample that is not in the working samples: %r"
                             % (name, v[np.argmin(hit)].item()))
        idx.append(np.ascontiguousarray(order[pos], np.int32))
    af_in = ws["allele_freq"]
    P = id1.size
    ll = np.empty(P, np.float64)
    niter = np.empty(P, np.int32) if out_num_iter else None
    af = np.empty(L, np.float64)
    ans = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], afreq=af, ID1=id1, ID2=id2)
    if method == "EM":
        k0, k1 = np.empty(P, np.float64), np.empty(P, np.float64)
        _lib.check(_lib.lib().snpgpu_gnrIBD_MLE_Pairs(_lib._ptr(af_in), _lib._ptr(idx[0]), _lib._ptr(idx[1]), P, int(max_niter),
                                                      float(reltol), int(bool(coeff_correct)), ws["num_thread"], int(bool(verbose)),
                                                      _lib._ptr(k0), _lib._ptr(k1), _lib._ptr(ll), _lib._ptr(niter), _lib._ptr(af)))
    else:
        coef = np.empty((8 if method == "Jacquard" else 2, P), np.float64)
        _lib.check(_lib.lib().snpgpu_gnrIBD_MLE_PairsMethod(_lib._ptr(af_in), _lib._ptr(idx[0]), _lib._ptr(idx[1]), P,
                                                            IBDMLE_METHODS.index(method), int(max_niter), float(reltol),
                                                            int(bool(coeff_correct)), ws["num_thread"], int(bool(verbose)),
                                                            _lib._ptr(coef), _lib._ptr(ll), _lib._ptr(niter), _lib._ptr(af)))
        k0, k1 = coef[0], coef[1]
    af[af < 0] = np.nan
    if method == "Jacquard":
        ans.update(("D%d" % (t + 1), coef[t]) for t in range(8))
        ans.update(loglik=ll, niter=niter)
        if kinship:
            ans["kinship"] = coef[0] + 0.5 * (coef[2] + coef[4] + coef[6]) + 0.25 * coef[7]
        return ans
    ans.update(k0=k0, k1=k1, loglik=ll, niter=niter)
    if kinship:
        ans["kinship"] = 0.5 * (1 - k0 - k1) + 0.25 * k1
    return ans


PAIRIBD_METHODS = ("EM", "downhill.simplex", "MoM", "Jacquard")


def _pair_vectors(geno1, geno2, allele_freq, verbose):
    """the argument checks of snpgdsPairIBD / snpgdsPairIBDMLELogLik (R/IBD.R:216-241) and the SNPs they keep: integer codes with
    3 = missing and the frequencies, for the loci with a finite frequency in [0, 1]"""
    vec = []
    for name, v in (("geno1", geno1), ("geno2", geno2), ("allele.freq", allele_freq)):
        a = np.asarray(v)
        if a.ndim != 1 or a.dtype.kind not in "iuf":
            raise TypeError("is.vector(%s) & is.numeric(%s) is not TRUE" % (name, name))
        vec.append(a)
    g1, g2, af = vec
    if len(g1) != len(g2):
        raise ValueError("length(geno1) == length(geno2) is not TRUE")
    if len(g1) != len(af):
        raise ValueError("length(geno1) == length(allele.freq) is not TRUE")
    af = np.array(af, np.float64)
    af[~np.isfinite(af)] = -1
    flag = (0 <= af) & (af <= 1)
    if flag.sum() < len(g1):
        _cat(verbose, "IBD MLE for %d SNPs in total, after removing loci with invalid allele frequencies." % flag.sum())

    def codes(g):
        g = np.asarray(g, np.float64)[flag]
        ok = np.isfinite(g)
        t = np.trunc(np.where(ok, g, 3))                       # as.integer
        return np.where(ok & (t >= 0) & (t <= 2), t, 3).astype(np.uint8)
    return codes(g1), codes(g2), np.ascontiguousarray(af[flag])


def snpgdsPairIBD(geno1, geno2, allele_freq, method="EM", kinship_constraint=False, max_niter=1000,
                  reltol=math.sqrt(np.finfo(float).eps), coeff_correct=True, out_num_iter=True, verbose=True, device=0):
    """IBD coefficients of one pair of genotype vectors (R/IBD.R:210-259 -> gnrPairIBD, src/genIBD.cpp:1646-1719): "EM" and "MoM"
    on the GPU (snpgpu_ibd_mle_pairs with two samples and the caller's frequencies).  Codes outside 0..2 are missing; SNPs whose
    frequency is not a finite value in [0, 1] are dropped.  kinship_constraint acts on the start values, as in the reference.
    Returns dict(k0, k1, loglik[, niter])."""
    c1, c2, af = _pair_vectors(geno1, geno2, allele_freq, verbose)
    _check_mle_args((("kinship.constraint", kinship_constraint), ("coeff.correct", coeff_correct)), ())
    if method not in PAIRIBD_METHODS:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in PAIRIBD_METHODS))
    if method in ("downhill.simplex", "Jacquard"):
        raise NotImplementedError('snpgdsPairIBD: method "%s" is not built on the GPU path (only "EM" and "MoM")' % method)
    from .gds import pack_2bit_rows
    rows = pack_2bit_rows(np.stack([c1, c2], 1))
    k0, k1, ll, nit, _ = _lib.ibd_mle_pairs(rows, 2, [0], [1], af, 0 if method == "EM" else 1, kinship_constraint, max_niter,
                                            reltol, coeff_correct, device)
    ans = dict(k0=float(k0[0]), k1=float(k1[0]), loglik=float(ll[0]))
    if out_num_iter:
        ans["niter"] = int(nit[0])
    return ans


def snpgdsPairIBDMLELogLik(geno1, geno2, allele_freq, k0=float("nan"), k1=float("nan"), relatedness="", verbose=True):
    """Log-likelihood of one pair at (k0, k1) or a relatedness preset (R/IBD.R:267-321 -> gnrPairIBDLogLik,
    src/genIBD.cpp:1771-1808), on the host in fp64 and in SNP order.  Non-positive sums are skipped (never -Inf)."""
    c1, c2, af = _pair_vectors(geno1, geno2, allele_freq, verbose)
    for name, v in (("k0", k0), ("k1", k1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("is.numeric(%s) is not TRUE" % name)
    if not isinstance(relatedness, str):
        raise TypeError("is.character(relatedness) is not TRUE")
    if RELATEDNESS.get(relatedness) is not None:
        k0, k1 = RELATEDNESS[relatedness]
    k0, k1 = float(k0), float(k1)
    k2 = 1 - k0 - k1
    # PrIBDTable (:454-510) with its own products
    p, q = af, 1 - af
    a, b = np.minimum(c1, c2).astype(np.int64), np.maximum(c1, c2).astype(np.int64)
    t0, t1, t2 = np.zeros(len(af)), np.zeros(len(af)), np.zeros(len(af))
    ok = (0 < p) & (p < 1)
    for ga, gb, v0, v1, v2 in ((0, 0, q * q * q * q, q * q * q, q * q), (0, 1, 2 * (p * q * q) * q, p * q * q, 0 * p),
                               (0, 2, p * p * q * q, 0 * p, 0 * p), (1, 1, 4 * (p * q) * (p * q), p * q, 2 * (p * q)),
                               (1, 2, 2 * p * (p * p * q), p * p * q, 0 * p), (2, 2, p * p * p * p, p * p * p, p * p)):
        m = ok & (a == ga) & (b == gb)
        t0[m], t1[m], t2[m] = v0[m], v1[m], v2[m]
    with np.errstate(invalid="ignore"):
        s = t0 * k0 + t1 * k1 + t2 * k2
    ll = 0.0
    for v in s[s > 0]:
        ll += math.log(v)
    return ll


_IBD_NOT_PER_PAIR = ("sample_id", "snp_id", "afreq", "inbreed")


def _full_matrix(x, n, name):
    """a per-pair entry of an IBD object as an n x n matrix: full, or the packed upper triangle of useMatrix=True (symmetric)"""
    x = np.asarray(x)
    if x.shape == (n, n):
        return x
    if x.shape == (_lib.tri_size(n),):
        m = np.empty((n, n), x.dtype)
        i, j = np.triu_indices(n)
        m[i, j] = x
        m[j, i] = x
        return m
    raise ValueError("'ibdobj$%s' should be a %d x %d matrix or its packed triangle, not %s" % (name, n, n, x.shape))


def snpgdsIBDSelection(ibdobj, kinship_cutoff=float("nan"), samp_sel=None):
    """Table of the pairs of an IBD object (R/IBD.R:463-531): dict of columns ID1, ID2, every per-pair entry of `ibdobj` in its
    order and -- derived from k0 / k1 or D1..D8 when the object has none -- kinship, for the pairs with kinship >= kinship_cutoff
    (a non-finite cutoff: every pair).  Rows follow which(lower.tri & flag, arr.ind=TRUE): ID1 = the earlier sample, ascending, then
    ID2 ascending.  samp_sel: None, a logical vector over the samples, or numeric 0-based indices (which may permute, as R's
    indexing does).  Works on the dicts of snpgdsIBDKING / snpgdsIBDMoM / snpgdsIBDMLE, full matrices or useMatrix triangles."""
    if not isinstance(ibdobj, dict) or "sample_id" not in ibdobj:
        raise TypeError("inherits(ibdobj, \"snpgdsIBDClass\") is not TRUE")
    if isinstance(kinship_cutoff, (bool, np.bool_)) or not isinstance(kinship_cutoff, (int, float, np.integer, np.floating)):
        raise TypeError("is.numeric(kinship.cutoff) is not TRUE")
    ids = np.asarray(ibdobj["sample_id"])
    n = len(ids)
    sel = None
    if samp_sel is not None:
        sel = np.asarray(samp_sel)
        if sel.dtype.kind == "b":
            if sel.shape != (n,):
                raise ValueError("length(samp.sel) == length(ibdobj$sample.id) is not TRUE")
            sel = np.flatnonzero(sel)
        elif sel.dtype.kind in "iuf" and sel.ndim == 1:
            if sel.dtype.kind == "f":
                if not np.all(np.isfinite(sel)):
                    raise ValueError("'samp.sel' should not hold NA")
                sel = sel.astype(np.int64)                       # truncation, as R's numeric subscripts
            if sel.size and (sel.min() < 0 or sel.max() >= n):
                raise IndexError("subscript out of bounds")
        else:
            raise TypeError("is.null(samp.sel) | is.logical(samp.sel) | is.numeric(samp.sel) is not TRUE")
    # the variables in the output
    ns = [k for k in ibdobj if k not in _IBD_NOT_PER_PAIR and ibdobj[k] is not None]
    mats = {k: _full_matrix(ibdobj[k], n, k) for k in ns}
    if sel is not None:
        ids = ids[sel]
        mats = {k: m[np.ix_(sel, sel)] for k, m in mats.items()}
        n = len(ids)
    if "kinship" not in mats:
        if "k0" in mats and "k1" in mats:
            mats["kinship"] = (1 - mats["k0"] - mats["k1"]) * 0.5 + mats["k1"] * 0.25
            ns.append("kinship")
        elif "D1" in mats:
            mats["kinship"] = mats["D1"] + 0.5 * (mats["D3"] + mats["D5"] + mats["D7"]) + 0.25 * mats["D8"]
            ns.append("kinship")
        elif np.isfinite(kinship_cutoff):
            raise ValueError("There is no kinship coefficient.")
    flag = np.tril(np.ones((n, n), bool), -1)
    if np.isfinite(kinship_cutoff):
        with np.errstate(invalid="ignore"):
            flag &= mats["kinship"] >= kinship_cutoff           # (NaN compares FALSE: flag[is.na(flag)] <- FALSE)
    col, row = np.nonzero(flag.T)                                # column-major walk of flag: which(flag, arr.ind=TRUE)
    ans = dict(ID1=ids[col], ID2=ids[row])
    for k in ns:
        ans[k] = mats[k][row, col]
    return ans


_IBD_PAIR_METHODS = {"KING-robust": _lib.SEL_KING_ROBUST, "KING-homo": _lib.SEL_KING_HOMO, "MoM": _lib.SEL_MOM}


def snpgdsIBDPairs(gdsobj, method="KING-robust", kinship_cutoff=float("nan"), samp_sel=None, family_id=None, allele_freq=None,
                   kinship_constraint=False, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True, maf=float("nan"),
                   missing_rate=0.01, num_thread=1, verbose=True, device=0):
    """The related pairs of a KING or MoM run without its n x n matrices.  No reference counterpart; the result equals
        snpgdsIBDSelection(snpgdsIBDKING(gdsobj, type=method, family_id=...), kinship_cutoff, samp_sel)      "KING-robust", "KING-homo"
        snpgdsIBDSelection(snpgdsIBDMoM(gdsobj, allele_freq=..., kinship_constraint=...), kinship_cutoff, samp_sel)      "MoM"
    column for column and bit for bit (ID1, ID2, IBS0 / k0, k1, kinship), plus sample_id, snp_id and, for MoM, afreq.  The counters are
    accumulated once on the GPU and only the selected pairs come back (snpgpu_gnrIBDPairs): host memory is proportional to their
    number.  Here samp_sel is a logical vector over the working samples or strictly increasing 0-based indices -- a selection, not a
    permutation; for anything else build the matrices and use snpgdsIBDSelection."""
    if method not in _IBD_PAIR_METHODS:
        raise ValueError("'arg' should be one of %s" % ", ".join("'%s'" % m for m in _IBD_PAIR_METHODS))
    if isinstance(kinship_cutoff, (bool, np.bool_)) or not isinstance(kinship_cutoff, (int, float, np.integer, np.floating)):
        raise TypeError("is.numeric(kinship.cutoff) is not TRUE")
    mom = method == "MoM"
    ws = _init_file2("IBD analysis (%s) on genotypes, related pairs only:" % ("PLINK method of moment" if mom else "KING method of moment"),
                     gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device,
                     allele_freq=allele_freq if mom else None)
    n = ws["n_samp"]
    mask = _pairs_samp_sel("snpgdsIBDPairs", samp_sel, n, "snpgdsIBDKING / snpgdsIBDMoM")
    fam = _family_codes(family_id, sample_id, ws, verbose and method == "KING-robust") if method == "KING-robust" else None
    af_in = ws["allele_freq"] if mom else None
    L = _lib.lib()
    found = ctypes.c_int64(0)
    _lib.check(L.snpgpu_gnrIBDPairs(_IBD_PAIR_METHODS[method], _lib._ptr(fam), _lib._ptr(af_in), int(bool(kinship_constraint)),
                                    float(kinship_cutoff), _lib._ptr(mask), ws["num_thread"], int(bool(verbose)), ctypes.byref(found)))
    m = found.value
    i1, i2 = np.empty(m, np.int32), np.empty(m, np.int32)
    v0, v1, kin = np.empty(m, np.float64), np.empty(m, np.float64), np.empty(m, np.float64)
    _lib.check(L.snpgpu_gnrIBDPairs_get(_lib._ptr(i1), _lib._ptr(i2), _lib._ptr(v0), _lib._ptr(v1), _lib._ptr(kin)))
    ids = np.asarray(ws["sample_id"])
    ans = dict(ID1=ids[i1], ID2=ids[i2])
    if method == "KING-robust":
        ans.update(IBS0=v0, kinship=kin)
    else:
        ans.update(k0=v0, k1=v1, kinship=kin)
    ans.update(sample_id=ws["sample_id"], snp_id=ws["snp_id"])
    if mom:
        if af_in is None:                  # the frequencies snpgpu_gnrIBD_PLINK reports: allele counts of the working samples
            af = np.empty(ws["n_snp"], np.float64)
            _lib.check(L.snpgpu_ws_snp_rate_freq(_lib._ptr(af), None, None))
        else:
            af = np.array(af_in, np.float64)
            af[np.isfinite(af) & ((af < 0) | (af > 1))] = np.nan
        ans["afreq"] = af
    _cat(verbose, "%d pair%s selected" % (m, "" if m == 1 else "s"))
    return ans


LD_PRUNE_METHODS = ("composite", "r", "dprime", "corr")
LD_PRUNE_START = ("random.f500", "random", "first", "last")
_INT_MAX = 2 ** 31 - 1
_NA_INTEGER = -2 ** 31


def _is_na(x):
    return x is None or (isinstance(x, (float, np.floating)) and math.isnan(x))


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))


def _as_integer(x):
    """Rf_asInteger of a numeric scalar: truncation toward zero; NaN or a value outside the int range is NA_integer_ (INT_MIN),
    with R's warning"""
    x = float(x)
    if math.isnan(x) or x >= _INT_MAX + 1.0 or x <= _NA_INTEGER:
        warnings.warn("NAs introduced by coercion to integer range", RuntimeWarning, stacklevel=3)
        return _NA_INTEGER
    return int(x)


def _pretty(x):
    """prettyNum(x, ",", scientific=FALSE)"""
    x = float(x)
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x.is_integer():
        return "{:,}".format(int(x))
    return "{:,}".format(float("%.7g" % x))


def snpgdsLDpruning(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True, maf=0.005, missing_rate=0.01,
                    method="composite", slide_max_bp=500000, slide_max_n=float("nan"), ld_threshold=0.2, start_pos="random.f500",
                    num_thread=1, autosave=None, verbose=True, device=0, seed=None):
    """LD-based SNP pruning (R/LD.R:100-243 -> gnrLDpruning, src/genLD.cpp:1014-1035, once per chromosome): a dict
    {"chr<ch>": kept snp ids} in the order the chromosomes first appear in the file (0 / "" excluded), chromosomes without a
    selected SNP left out, as R's list.

    Per chromosome the working space is its selected SNPs in file order and Perform_LD_Pruning runs on it (snpgpu_ld_prune: the
    pair tables of the window on the GPU, the greedy scan on the host).  The window limits are coerced as R does: NA / Inf
    slide_max_n becomes .Machine$integer.max; NA / Inf slide_max_bp becomes .Machine$double.xmax, which Rf_asInteger turns into
    NA_integer_ -- no SNP is then inside any window and every selected SNP is kept (the reference's behaviour, with R's coercion
    warning); finite values are truncated toward zero.

    start_pos "random.f500" / "random" draw the 1-based start index uniformly from 1 ... min(n, 500) / 1 ... n per chromosome,
    in chromosome order, from numpy.random.default_rng(seed): the ranges are R's, the stream is not (R's sample.int cannot be
    reproduced).  autosave (saveRDS, R only) is validated as in R; a file name raises NotImplementedError."""
    # the R function's argument checks, before anything reaches the device
    if not (_is_na(slide_max_bp) or _is_number(slide_max_bp)):
        raise TypeError("is.na(slide.max.bp) | is.numeric(slide.max.bp) is not TRUE")
    if not (_is_na(slide_max_n) or _is_number(slide_max_n)):
        raise TypeError("is.na(slide.max.n) | is.numeric(slide.max.n) is not TRUE")
    if not _is_number(ld_threshold):
        raise TypeError("is.numeric(ld.threshold) is not TRUE")
    if not math.isfinite(ld_threshold):
        raise ValueError("is.finite(ld.threshold) is not TRUE")
    if not _is_number(num_thread):
        raise TypeError("is.numeric(num.thread) is not TRUE")
    if not num_thread > 0:
        raise ValueError("num.thread > 0L is not TRUE")
    if autosave is not None and not isinstance(autosave, str):
        raise TypeError("is.null(autosave) | is.character(autosave) is not TRUE")
    if isinstance(autosave, str) and autosave == "":
        raise ValueError("'autosave' should be NULL or a file name.")
    if start_pos not in LD_PRUNE_START:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in LD_PRUNE_START))
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    if method not in LD_PRUNE_METHODS:
        raise ValueError('method should be one of "composite", "r", "dprime" and "corr"')
    if autosave is not None:
        raise NotImplementedError("snpgdsLDpruning: 'autosave' writes an R object (saveRDS), which only R can do")
    if not isinstance(gdsobj, GenoFile):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    if gdsobj.snp_position is None:
        raise ValueError("GDS node 'snp.position' not found")
    code = LD_PRUNE_METHODS.index(method) + 1

    ws = _init_file2("SNP pruning based on LD:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate,
                     num_thread, verbose, device)
    bp, mn = slide_max_bp, slide_max_n
    if verbose:
        print("    sliding window: %s basepairs, %s SNPs" % (_pretty(bp if not _is_na(bp) and math.isfinite(bp) else math.inf),
                                                              _pretty(mn if not _is_na(mn) and math.isfinite(mn) else math.inf)))
        print("    |LD| threshold: %g" % ld_threshold)
        print("    method: %s" % ("composite", "R", "D'", "correlation")[code - 1])
    bp = _as_integer(np.finfo(np.float64).max if _is_na(bp) or not math.isfinite(bp) else bp)
    mn = _as_integer(_INT_MAX if _is_na(mn) or not math.isfinite(mn) else mn)

    total_ids = gdsobj.snp_id
    chrom = np.asarray(gdsobj.snp_chromosome)
    position = gdsobj.snp_position
    snp_flag = np.isin(total_ids, ws["snp_id"])
    ws_chrom = chrom[snp_flag]                       # chromosome of each working-space SNP (file order)
    _, first = np.unique(chrom, return_index=True)
    chrset = [c for c in chrom[np.sort(first)] if not (c == 0 if np.issubdtype(chrom.dtype, np.number) else c == "")]
    rng = np.random.default_rng(seed)
    L = _lib.lib()
    res, ntotal = {}, 0
    for ch in chrset:
        flag = snp_flag & (chrom == ch)
        n_tmp = int(flag.sum())
        if n_tmp <= 0:
            continue
        rows = np.ascontiguousarray(ws["packed"][ws_chrom == ch])
        _lib.check(L.snpgpu_ws_set_geno(_lib._ptr(rows), n_tmp, ws["n_samp"], _lib.GENO_PACKED2, int(device)))
        if start_pos == "random.f500":
            startidx = int(rng.integers(1, min(n_tmp, 500) + 1))
        elif start_pos == "random":
            startidx = int(rng.integers(1, n_tmp + 1))
        else:
            startidx = 1 if start_pos == "first" else n_tmp
        pos = np.ascontiguousarray(position[flag], np.int32)
        keep = np.zeros(n_tmp, np.uint8)
        _lib.check(L.snpgpu_gnrLDpruning(startidx - 1, _lib._ptr(pos), bp, mn, float(ld_threshold), code, int(num_thread),
                                         int(bool(verbose)), _lib._ptr(keep)))
        rv = keep.astype(bool)
        res["chr%s" % ch] = total_ids[flag][rv]
        ntmp = int(rv.sum())
        ntotal += ntmp
        if verbose:
            # Perform_LD_Pruning's two progress bars (CdProgression type 2: 20 '=' per pass that has SNPs to visit)
            print("Chrom %s: |%s|%s|" % (ch, "=" * 20 if n_tmp - startidx > 0 else "", "=" * 20 if startidx > 1 else ""))
            ntot = int((chrom == ch).sum())
            print("    %0.2f%%, %s / %s (%s)" % (100.0 * ntmp / ntot, _pretty(ntmp), _pretty(ntot), time.ctime()))
    if verbose:
        print("%s markers are selected in total." % _pretty(ntotal))
    return res


def snpgdsLDScore(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True, maf=float("nan"),
                  missing_rate=float("nan"), method="corr", slide_max_bp=1000000, slide_max_n=float("nan"), adjust=True,
                  include_self=True, with_id=True, num_thread=1, verbose=True, device=0):
    """LD score of every selected SNP: score[i] = sum of the squared LD values of the pairs (i, j) over the partners j of i on the
    same chromosome with |i - j| <= slide_max_n (in selected SNPs) and |pos[i] - pos[j]| <= slide_max_bp.  Not a function of the
    reference: what snpgdsLDMat's users reduce its band to, computed on the GPU without the slide x n_snp matrix (one
    snpgpu_gnrLDScore call per chromosome over its selected SNPs in file order, include/snpgpu.h section 1d).

    method: "composite", "r", "dprime" or "corr".  adjust: each squared value t becomes t - (1 - t) / (n - 2), n = the samples
    called at both SNPs (pairs with n <= 2 are then not valid); pairs whose LD value is NaN are never valid.  include_self adds
    the SNP's own term 1.  The window limits are coerced as in snpgdsLDpruning (NA / Inf slide_max_n becomes
    .Machine$integer.max, finite values go through Rf_asInteger), except that a NA / Inf slide_max_bp means no limit in base
    pairs: the positions are then not needed.  A chromosome's selected positions must not decrease.

    Returns dict(sample_id, snp_id, chromosome, position, score, n_valid, n_window) in the order of the selected SNPs (n_valid:
    valid partners, n_window: partners in the window), or the bare score with with_id=False."""
    # the argument checks, R style, before anything reaches the device
    if not (_is_na(slide_max_bp) or _is_number(slide_max_bp)):
        raise TypeError("is.na(slide.max.bp) | is.numeric(slide.max.bp) is not TRUE")
    if not (_is_na(slide_max_n) or _is_number(slide_max_n)):
        raise TypeError("is.na(slide.max.n) | is.numeric(slide.max.n) is not TRUE")
    if not _is_number(num_thread):
        raise TypeError("is.numeric(num.thread) is not TRUE")
    if not num_thread > 0:
        raise ValueError("num.thread > 0L is not TRUE")
    for name, v in (("adjust", adjust), ("include.self", include_self), ("with.id", with_id), ("verbose", verbose)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    if method not in LD_PRUNE_METHODS:
        raise ValueError('method should be one of "composite", "r", "dprime" and "corr"')
    if not isinstance(gdsobj, GenoFile):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    bp_limit = not _is_na(slide_max_bp) and math.isfinite(slide_max_bp)
    if bp_limit and gdsobj.snp_position is None:
        raise ValueError("GDS node 'snp.position' not found (needed for a finite slide.max.bp)")
    code = LD_PRUNE_METHODS.index(method) + 1

    ws = _init_file2("LD scores:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose,
                     device)
    bp, mn = slide_max_bp, slide_max_n
    if verbose:
        print("    sliding window: %s basepairs, %s SNPs" % (_pretty(bp if bp_limit else math.inf),
                                                              _pretty(mn if not _is_na(mn) and math.isfinite(mn) else math.inf)))
        print("    method: %s" % ("composite", "R", "D'", "correlation")[code - 1])
        print("    adjusted: %s, self term: %s" % (str(bool(adjust)).upper(), str(bool(include_self)).upper()))
    bp = _as_integer(bp) if bp_limit else _INT_MAX
    mn = _as_integer(_INT_MAX if _is_na(mn) or not math.isfinite(mn) else mn)
    flags = (_lib.LDSCORE_ADJUST if adjust else 0) | (_lib.LDSCORE_SELF if include_self else 0)

    snp_flag = np.isin(gdsobj.snp_id, ws["snp_id"])
    ws_chrom = np.asarray(gdsobj.snp_chromosome)[snp_flag]           # of each working-space SNP (file order)
    ws_pos = None if gdsobj.snp_position is None else np.ascontiguousarray(gdsobj.snp_position[snp_flag], np.int32)
    _, first = np.unique(ws_chrom, return_index=True)
    groups = [(ch, np.nonzero(ws_chrom == ch)[0]) for ch in ws_chrom[np.sort(first)]]
    if bp_limit:
        for ch, idx in groups:
            if np.any(np.diff(ws_pos[idx].astype(np.int64)) < 0):
                raise ValueError("snp.position decreases on chromosome %s: the SNPs of a chromosome should be sorted by position" % ch)
    n = ws["n_snp"]
    score = np.empty(n, np.float64)
    n_valid, n_window = np.empty(n, np.int32), np.empty(n, np.int32)
    L = _lib.lib()
    for ch, idx in groups:
        rows = np.ascontiguousarray(ws["packed"][idx])
        _lib.check(L.snpgpu_ws_set_geno(_lib._ptr(rows), len(idx), ws["n_samp"], _lib.GENO_PACKED2, int(device)))
        pos = np.ascontiguousarray(ws_pos[idx]) if bp_limit else None
        s = np.empty(len(idx), np.float64)
        nv, nw = np.empty(len(idx), np.int32), np.empty(len(idx), np.int32)
        _lib.check(L.snpgpu_gnrLDScore(_lib._ptr(pos), bp, mn, code, flags, int(num_thread), int(bool(verbose)), _lib._ptr(s),
                                       _lib._ptr(nv), _lib._ptr(nw)))
        score[idx], n_valid[idx], n_window[idx] = s, nv, nw
        if verbose:
            print("Chrom %s: %s SNPs, %s pairs in the window, mean LD score %.6g" % (ch, _pretty(len(idx)), _pretty(int(nw.sum()) // 2),
                                                                                    float(s.mean())))
    if not with_id:
        return score
    return dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], chromosome=ws_chrom, position=ws_pos, score=score, n_valid=n_valid,
                n_window=n_window)


# ---------------------------------------------------------------------------------------------------------------------
# population statistics: snpgdsFst (R/IBD.R:756-830) and snpgdsSlidingWindow (R/AllUtilities.R:1998-2239)
FST_METHODS = _lib.FST_METHODS
SLIDE_UNITS = ("basepair", "locus")
SLIDE_AS_IS = ("list", "numeric", "array")
SLIDE_WITH_ID = ("snp.id", "snp.id.in.window", "none")
SLIDE_FUNS = ("snpgdsFst", "snpgdsSNPRateFreq")


def _match_arg(value, choices, name):
    """match.arg: NULL or the whole default vector selects the first choice"""
    if value is None or (isinstance(value, (tuple, list)) and tuple(value) == tuple(choices)):
        return choices[0]
    if isinstance(value, str) and value in choices:
        return value
    raise ValueError("'%s' should be one of %s" % (name, ", ".join('"%s"' % c for c in choices)))


def _working_sample_ids(gdsobj, sample_id):
    """ws$sample.id of .InitFile2: the file's samples that are selected, in FILE order"""
    ids = np.asarray(gdsobj.sample_id)
    if sample_id is None:
        return ids
    return ids[np.isin(ids, np.asarray(sample_id))]


def _param_fst(sample_id, population, method, ws_sample_id):
    """.paramFst (R/IBD.R:756-795) without its verbose lines: `population` is any sequence of labels, its levels the sorted unique
    labels (as factor()); returns the 1-based codes in working sample order, the levels, their sizes and the method."""
    method = _match_arg(method, FST_METHODS, "method")
    if population is None or isinstance(population, (str, bytes)) or not hasattr(population, "__len__"):
        raise TypeError("is.factor(population) is not TRUE")
    labels = list(population)
    na = [lab is None or (isinstance(lab, (float, np.floating)) and math.isnan(lab)) for lab in labels]
    levels = sorted(set(lab for lab, m in zip(labels, na) if not m))
    if sample_id is None:
        if len(labels) != len(ws_sample_id):
            raise ValueError("The length of 'population' should be the number of samples in the GDS file.")
    else:
        want = list(np.asarray(sample_id))
        if len(labels) != len(want):
            raise ValueError("The length of 'population' should be the same as the length of 'sample.id'.")
        where = {}
        for i, s in enumerate(want):
            where.setdefault(s, i)                       # match(): the first occurrence
        pos = [where[s] for s in list(ws_sample_id)]
        labels = [labels[i] for i in pos]
        na = [na[i] for i in pos]
    if any(na):
        raise ValueError("'population' should not have missing values!")
    if len(levels) <= 1:
        raise ValueError("There should be at least two populations!")
    code = {lab: i + 1 for i, lab in enumerate(levels)}
    codes = np.array([code[lab] for lab in labels], np.int32)
    sizes = np.bincount(codes, minlength=len(levels) + 1)[1:]
    if (sizes < 1).any():
        raise ValueError("Each population should have at least one individual.")
    return dict(population=codes, npop=len(levels), method=method, levels=levels, sizes=sizes)


def _print_param_fst(v):
    print("Method: Weir & Cockerham, 1984" if v["method"] == "W&C84" else "Method: Weir & Hill, 2002")
    print("# of Populations: %d\n    %s" % (v["npop"], ", ".join("%s (%d)" % (lv, n) for lv, n in zip(v["levels"], v["sizes"]))))


def snpgdsFst(gdsobj, population, method="W&C84", sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
              maf=float("nan"), missing_rate=0.01, with_id=False, verbose=True, device=0):
    """Fixation index (R/IBD.R:797-830 -> gnrFst, src/genFst.cpp:170-242): dict(Fst, MeanFst, FstSNP[, Beta, Beta_levels]
    [, sample_id, snp_id]).  `population`: one label per sample of the file, or per entry of `sample_id` (re-ordered to the working
    sample order as .paramFst does); its levels are the sorted unique labels.  method "W&C84" (Weir & Cockerham 1984) or "W&H02"
    (Weir & Hill 2002, with the K x K matrix Beta whose rows / columns are Beta_levels).  The per-population allele counters are
    exact integers from one pass over the genotypes on the GPU (snpgpu_pop_counts); the Fst terms are fp64 in the reference's
    operation order."""
    if not isinstance(gdsobj, GenoFile) and not hasattr(gdsobj, "packed"):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    v = _param_fst(sample_id, population, method, _working_sample_ids(gdsobj, sample_id))
    ws = _init_file2("Fst estimation on genotypes:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate,
                     1, verbose, device)
    if verbose:
        _print_param_fst(v)
    k = v["npop"]
    fst = ctypes.c_double(0)
    per = np.empty(ws["n_snp"], np.float64)
    beta = np.empty((k, k), np.float64) if v["method"] == "W&H02" else None
    _lib.check(_lib.lib().snpgpu_gnrFst(_lib._ptr(v["population"]), k, v["method"].encode(), ctypes.byref(fst), _lib._ptr(per),
                                        _lib._ptr(beta)))
    rv = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"]) if with_id else {}
    rv["Fst"] = fst.value
    ok = ~np.isnan(per)
    rv["MeanFst"] = float(per[ok].mean()) if ok.any() else float("nan")
    rv["FstSNP"] = per
    if beta is not None:
        rv["Beta"] = beta
        rv["Beta_levels"] = list(v["levels"])
    return rv


def sliding_num_win(start, end, winsize, shift):
    """SlidingNumWin (src/genSlideWin.cpp:78-85): window starts start, start + shift, ... <= end - winsize, plus one"""
    e = end - winsize
    return (0 if start > e else (e - start) // shift + 1) + 1


def _window_members(lo_vals, key, winsize):
    """CSR membership of the windows lo <= key < lo + winsize in ascending SNP index order; key: one integer per SNP"""
    order = np.argsort(key, kind="stable")
    skey = key[order]
    a = np.searchsorted(skey, lo_vals, side="left")
    b = np.searchsorted(skey, lo_vals + winsize, side="left")
    offsets = np.zeros(len(lo_vals) + 1, np.int64)
    np.cumsum(b - a, out=offsets[1:])
    idx = np.empty(int(offsets[-1]), np.int32)
    in_order = bool((order[1:] > order[:-1]).all()) if len(order) > 1 else True
    for w in range(len(lo_vals)):
        seg = order[a[w]:b[w]]
        idx[offsets[w]:offsets[w + 1]] = seg if in_order else np.sort(seg)
    return offsets, idx


def _finite_mean(x):
    """GetMean (src/genSlideWin.cpp:61-75): the mean of the finite values, summed in order; 0 / 0 without any"""
    f = x[np.isfinite(x)]
    return float(np.cumsum(f)[-1]) / len(f) if len(f) else float("nan")


def snpgdsSlidingWindow(gdsobj, sample_id=None, snp_id=None, FUN=None, winsize=100000, shift=10000, unit="basepair", winstart=None,
                        autosome_only=False, remove_monosnp=True, maf=float("nan"), missing_rate=float("nan"), as_is="list",
                        with_id="snp.id", num_thread=1, verbose=True, device=0, **kwargs):
    """Sliding-window scan (R/AllUtilities.R:1998-2239, gnrSlidingWindow src/genSlideWin.cpp:101-327): a dict with sample_id,
    (snp_id,) and per chromosome -- in order of first appearance, 0 / "" left out, SNPs with a position <= 0 dropped -- the keys
    "chr<ch>.val", "chr<ch>.num" (SNPs per window), "chr<ch>.pos" (mean position, NaN for an empty window) and "chr<ch>.posrange".
    Windows: SlidingNumWin of them, starting at `winstart` (None: the first position / the first SNP; a scalar; or one value per
    chromosome) and `shift` apart, half-open x <= pos < x + winsize (unit "basepair") or index windows (unit "locus").

    FUN="snpgdsFst" (population=, method= as keyword arguments): every window's Fst from ONE pass over the chromosome's genotypes
      (snpgpu_gnrSlidingWindowFst: exact per-population counters, window sums on the device).  as_is "numeric": the window's Fst
      (NaN for an empty window); "list": [Fst, FstSNP of the window's SNPs(, Beta)] per window, None for an empty one -- the
      reference's unnamed gnrFst list.  as_is "array" raises NotImplementedError: the reference fills it from the per-SNP ratio
      vector at stride npop + 1 instead of from Beta and reads past its end in small windows, so there is no defined result.
    FUN="snpgdsSNPRateFreq": window means of the finite per-SNP allele frequency / minor allele frequency / missing rate;
      "list": the window's three per-SNP vectors, "numeric": the mean MAF, "array": 3 x windows.
    FUN callable: the host loop of the R function, FUN(sample_id, snp_ids, positions, **kwargs) per window, keys "chr<ch>" (values),
      ".num", ".pos", ".posrange" and, with with_id="snp.id.in.window", ".snpid".  As in R, basepair windows then start at the first
      position whatever `winstart` says (it only enters the window count).  One deviation: a locus window running past the last
      SNP passes only the SNPs that exist (R passes NA ids), with .num = winsize and .pos = NaN as R's NA indexing gives.
    shift must be positive (the reference would not terminate otherwise).  The argument checks of the R function run before the
    device is used; of a `winstart` with one value per chromosome only "more values than the file has chromosomes" can be known
    then -- the chromosome set is that of the SNPs the device-side filter (remove_monosnp, maf, missing_rate) keeps, so any other
    wrong length is reported after the filter, as in R.  With FUN="snpgdsFst" keyword arguments other than population / method
    are ignored, as R's list(...) lookup ignores them."""
    # the R function's argument checks, before anything reaches the device
    if not _is_number(winsize):
        raise TypeError("is.numeric(winsize) is not TRUE")
    if not _is_number(shift):
        raise TypeError("is.numeric(shift) is not TRUE")
    unit = _match_arg(unit, SLIDE_UNITS, "unit")
    as_is = _match_arg(as_is, SLIDE_AS_IS, "as.is")
    with_id = _match_arg(with_id, SLIDE_WITH_ID, "with.id")
    if not (math.isfinite(winsize) and math.isfinite(shift)) or abs(winsize) >= 2 ** 31 or abs(shift) >= 2 ** 31:
        raise ValueError("is.finite(winsize) & is.finite(shift) is not TRUE")
    winsize, shift = int(winsize), int(shift)
    if shift <= 0:
        raise ValueError("'shift' should be positive")
    if winstart is not None:
        ok = _is_number(winstart) or (isinstance(winstart, (list, tuple, np.ndarray)) and np.ndim(winstart) == 1 and
                                      all(_is_number(x) for x in winstart))
        if not ok:
            raise TypeError("is.null(winstart) | (is.numeric(winstart) & is.vector(winstart)) is not TRUE")
        winstart = [winstart] if _is_number(winstart) else list(winstart)
        if not all(math.isfinite(x) for x in winstart):
            raise ValueError("all(is.finite(winstart)) is not TRUE")
        winstart = [int(x) for x in winstart]
    if callable(FUN):
        if FUN is snpgdsFst:
            raise ValueError('Please use `FUN="snpgdsFst"` instead.')
        if FUN is snpgdsSNPRateFreq:
            raise ValueError('Please use `FUN="snpgdsSNPRateFreq"` instead.')
        fun_idx = 0
    elif isinstance(FUN, str):
        if FUN not in SLIDE_FUNS:
            raise ValueError("'FUN' should be one of %s." % ",".join(SLIDE_FUNS))
        fun_idx = SLIDE_FUNS.index(FUN) + 1
    else:
        raise TypeError("'FUN' should be a function, or a character.")
    if not isinstance(gdsobj, GenoFile) and not hasattr(gdsobj, "packed"):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    position = getattr(gdsobj, "snp_position", None)
    if position is None:
        raise ValueError("GDS node 'snp.position' not found")
    param = None
    if fun_idx == 1:
        if as_is == "array":
            raise NotImplementedError(
                'snpgdsSlidingWindow(FUN="snpgdsFst", as.is="array") has no defined result: the reference fills the array from the '
                "per-SNP ratio vector at stride npop + 1 (src/genSlideWin.cpp:284-292), not from Beta, and reads past its end in "
                'small windows; use as.is="list" or "numeric"')
        param = _param_fst(sample_id, kwargs.get("population"), kwargs.get("method"), _working_sample_ids(gdsobj, sample_id))
    elif fun_idx == 2 and kwargs:
        raise ValueError("Unused additional parameters '...'.")
    total_ids = np.asarray(gdsobj.snp_id)
    chrom = np.asarray(gdsobj.snp_chromosome)
    numeric_chr = np.issubdtype(chrom.dtype, np.number)

    def chrom_set(flag):
        c = chrom[flag]
        _, first = np.unique(c, return_index=True)
        return [x for x in c[np.sort(first)] if not (x == 0 if numeric_chr else x == "")]

    placed = np.asarray(position) > 0
    if winstart is not None and len(winstart) != 1 and len(winstart) > len(chrom_set(placed)):
        raise ValueError("'winstart' should be specified according to the chromosome set (%s)" %
                         ",".join(str(c) for c in chrom_set(placed)))

    ws = _init_file2("Sliding Window Analysis:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate,
                     num_thread, verbose, device)
    if verbose:
        print("    window size: %d, shift: %d%s" % (winsize, shift, " (basepair)" if unit == "basepair" else " (locus index)"))
        if param is not None:
            _print_param_fst(param)
    ans = dict(sample_id=ws["sample_id"])
    if with_id in ("snp.id", "snp.id.in.window"):
        ans["snp_id"] = ws["snp_id"]
    in_ws = np.isin(total_ids, ws["snp_id"])
    snp_flag = in_ws & placed
    chrset = chrom_set(snp_flag)
    if winstart is not None and len(winstart) != 1 and len(winstart) != len(chrset):
        raise ValueError("'winstart' should be specified according to the chromosome set (%s)" % ",".join(str(c) for c in chrset))
    if verbose:
        print("Chromosome Set: %s" % ",".join(str(c) for c in chrset))
    L = _lib.lib()
    for ci, ch in enumerate(chrset):
        chflag = snp_flag & (chrom == ch)
        sid = total_ids[chflag]
        chpos = np.asarray(position)[chflag].astype(np.int64)
        winst = None if winstart is None else winstart[0 if len(winstart) == 1 else ci]
        n_chr = len(chpos)
        rg = (int(chpos.min()), int(chpos.max()))
        key = "chr%s" % ch
        if fun_idx == 0:
            if unit == "basepair":
                n = sliding_num_win(rg[0] if winst is None else winst, rg[1], winsize, shift)
            else:
                n = sliding_num_win(1 if winst is None else winst, n_chr, winsize, shift)
            if verbose:
                print("%s, Chromosome %s (%d SNPs), %d windows" % (time.ctime(), ch, n_chr, n))
            rvlist = [None] * n if as_is == "list" else np.zeros(n, np.float64)
            nlist, poslist, sidlist = np.zeros(n, np.int32), np.zeros(n, np.float64), [None] * n
            x = rg[0] if unit == "basepair" else 1
            for i in range(n):
                if unit == "basepair":
                    k = (x <= chpos) & (chpos < x + winsize)
                    ssid, ppos = sid[k], chpos[k]
                    nlist[i] = len(ppos)
                    poslist[i] = ppos.mean() if len(ppos) else float("nan")
                else:
                    lo, hi = max(x - 1, 0), max(min(x - 1 + winsize, n_chr), 0)
                    ssid, ppos = sid[lo:hi], chpos[lo:hi]
                    nlist[i] = winsize
                    poslist[i] = ppos.mean() if (len(ppos) == winsize and x >= 1) else float("nan")
                v = FUN(ans["sample_id"], ssid, ppos, **kwargs)
                if as_is == "list":
                    rvlist[i] = v
                else:
                    rvlist[i] = float(np.asarray(v, np.float64).reshape(-1)[0])
                sidlist[i] = ssid
                x += shift
            ans[key] = rvlist
            ans[key + ".num"] = nlist
            ans[key + ".pos"] = poslist
            ans[key + ".posrange"] = np.array(rg, np.int32)
            if with_id == "snp.id.in.window":
                ans[key + ".snpid"] = sidlist
            continue

        # gnrSlidingWindow
        if unit == "basepair":
            start, end, wkey = (rg[0] if winst is None else winst), rg[1], chpos
        else:
            start, end, wkey = (0 if winst is None else winst - 1), n_chr - 1, np.arange(n_chr, dtype=np.int64)
        n_win = sliding_num_win(start, end, winsize, shift)
        if verbose:
            print("%s, Chromosome %s (%d SNPs), %d windows" % (time.ctime(), ch, n_chr, n_win))
        offsets, idx = _window_members(start + shift * np.arange(n_win, dtype=np.int64), wkey, winsize)
        num = np.diff(offsets).astype(np.int32)
        psum = np.concatenate([[0.0], np.cumsum(chpos[idx].astype(np.float64))])       # integers: exact in any order
        with np.errstate(invalid="ignore", divide="ignore"):
            pos = np.where(num > 0, (psum[offsets[1:]] - psum[offsets[:-1]]) / np.maximum(num, 1), np.nan)
        rows = np.ascontiguousarray(ws["packed"][chflag[in_ws]])
        _lib.check(L.snpgpu_ws_set_geno(_lib._ptr(rows), n_chr, ws["n_samp"], _lib.GENO_PACKED2, int(device)))
        if fun_idx == 1:
            k = param["npop"]
            fw = np.empty(n_win, np.float64)
            per = np.empty(n_chr, np.float64)
            want_beta = param["method"] == "W&H02" and as_is == "list"
            beta = np.empty((n_win, k, k), np.float64) if want_beta else None
            _lib.check(L.snpgpu_gnrSlidingWindowFst(_lib._ptr(param["population"]), k, param["method"].encode(), _lib._ptr(offsets),
                                                    _lib._ptr(idx), n_win, _lib._ptr(fw), _lib._ptr(beta), _lib._ptr(per)))
            if as_is == "numeric":
                val = np.where(num > 0, fw, np.nan)
            else:
                val = [None] * n_win
                for w in range(n_win):
                    if num[w] > 0:
                        val[w] = [float(fw[w]), per[idx[offsets[w]:offsets[w + 1]]]] + ([beta[w]] if want_beta else [])
        else:
            af, mf, mr = (np.empty(n_chr, np.float64) for _ in range(3))
            _lib.check(L.snpgpu_ws_snp_rate_freq(_lib._ptr(af), _lib._ptr(mf), _lib._ptr(mr)))
            seg = [idx[offsets[w]:offsets[w + 1]] for w in range(n_win)]
            if as_is == "list":
                val = [[af[s], mf[s], mr[s]] if len(s) else None for s in seg]
            elif as_is == "numeric":
                val = np.array([_finite_mean(mf[s]) if len(s) else np.nan for s in seg], np.float64)
            else:
                val = np.full((3, n_win), np.nan)
                for w, s in enumerate(seg):
                    if len(s):
                        val[:, w] = (_finite_mean(af[s]), _finite_mean(mf[s]), _finite_mean(mr[s]))
        ans[key + ".val"] = val
        ans[key + ".num"] = num
        ans[key + ".pos"] = pos
        ans[key + ".posrange"] = np.array(rg, np.int32)
    if verbose:
        print("%s\tDone." % time.ctime())
    return ans


# ---- quality-control statistics ---------------------------------------------------------------------------------------------
INB_METHODS = _lib.INB_METHODS
INB_COEF_METHODS = ("mom.weir", "mom.visscher", "mle")
_RELTOL_INB = float(np.finfo(float).eps ** 0.75)


def _scalar_reltol(reltol):
    """stopifnot(is.numeric(reltol), length(reltol) == 1L) / gnrIndInbCoef's own check (src/genIBD.cpp:1820-1821)"""
    if isinstance(reltol, (bool, np.bool_)) or not isinstance(reltol, (int, float, np.integer, np.floating)):
        raise ValueError("`reltol' should a real number.")
    return float(reltol)


def snpgdsSampMissRate(gdsobj, sample_id=None, snp_id=None, with_id=False, device=0):
    """Missing rate per sample (R/AllUtilities.R:230-248 -> gnrSampFreq -> GetSampMissingRates, src/dGenGWAS.cpp:207-248):
    float64 [n_samp] = (calls > 2) / n_snp over the selected SNPs, from the exact per-sample counters of snpgpu_geno_counts.
    with_id: R names the vector by sample; here, as snpgdsSNPRateFreq does with its ids, dict(sample_id, MissingRate)."""
    ws = _init_file(gdsobj, sample_id, snp_id, device)
    rv = np.empty(ws["n_samp"], np.float64)
    _lib.check(_lib.lib().snpgpu_gnrSampFreq(_lib._ptr(rv)))
    if with_id:
        return dict(sample_id=ws["sample_id"], MissingRate=rv)
    return rv


def snpgdsGetGeno(gdsobj, sample_id=None, snp_id=None, snpfirstdim=None, with_id=False, verbose=True, device=0):
    """A subset of the genotypes of a file (R/AllUtilities.R:1006-1025 -> gnrCopyGenoMem, src/SNPRelate.cpp:322-382).
    gdsobj: a SNP GDS object, or a file name (opened and closed here).  The selection follows FILE order whatever the order of the
    id lists, as .InitFile's flags do.  snpfirstdim None (R's NA) follows the file's layout: a snp.order file gives n_snp x n_samp,
    a sample.order file n_samp x n_snp; True / False force one.  verbose prints the reference's line.  The result is uint8 with
    3 for a missing call, as read_genotype returns it: numpy has no NA_integer_, which is what R's integer matrix holds there.
    with_id: dict(genotype, sample_id, snp_id).  Selection and layout run on the device (snpgpu_geno_select, 2 bits per genotype);
    only the final expansion to one byte per genotype is host numpy, since that part is bound by its own output."""
    if snpfirstdim is not None and not isinstance(snpfirstdim, (bool, np.bool_)):
        raise TypeError("is.logical(snpfirstdim) is not TRUE")
    if not isinstance(with_id, (bool, np.bool_)):
        raise TypeError("is.logical(with.id) is not TRUE")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    opened = isinstance(gdsobj, str)
    if opened:
        gdsobj = snpgdsOpen(gdsobj, stream=True)
    try:
        ws = _init_file(gdsobj, sample_id, snp_id, device)
    finally:
        if opened:
            snpgdsClose(gdsobj)                     # on.exit({ snpgdsClose(gdsobj) })
    if snpfirstdim is None:
        snpfirstdim = not getattr(gdsobj, "sample_order", True)
    g = _gds.unpack_2bit_rows(ws["packed"], ws["n_samp"])
    if snpfirstdim:
        _cat(verbose, "Genotype matrix: %d SNPs X %d samples" % (ws["n_snp"], ws["n_samp"]))
        g = np.ascontiguousarray(g)
    else:
        _cat(verbose, "Genotype matrix: %d samples X %d SNPs" % (ws["n_samp"], ws["n_snp"]))
        g = np.ascontiguousarray(g.T)
    if with_id:
        return dict(genotype=g, sample_id=ws["sample_id"], snp_id=ws["snp_id"])
    return g


def snpgdsOption(autosome_start=1, autosome_end=22, **chromosome_code):
    """snpgdsOption() without a file (R/AllUtilities.R:1910-1990): dict(autosome_start, autosome_end, chromosome_code), the codes
    X, XY, Y, M = MT = autosome_end + 1 ... + 4 unless others are named.  The `option` of snpgdsOpenBED."""
    return _bed.default_option(autosome_start, autosome_end, **chromosome_code)


def snpgdsOpenBED(bed_fn, fam_fn=None, bim_fn=None, family=False, option=None, cvt_chr="int", cvt_snpid="auto", verbose=True):
    """Open a PLINK binary PED file for every snpgds* function: snpgdsBED2GDS (R/Conversion.R:433-653) + snpgdsOpen in one step,
    without the GDS file in between.  Returns a bed.BedStream -- a GenoStream whose sample_id, snp_id (snp_rs_id), snp_chromosome,
    snp_position, snp_allele and sample_annot are what snpgdsBED2GDS would have stored, and whose genotypes stay in the .bed file
    (memory-mapped; a .bed.gz is inflated once) and are recoded on the device, block by block, as they are read.
    fam_fn and bim_fn both None: they are named after bed_fn (R/Conversion.R:440-446).  family: keep FamilyID, PatID, MatID in
    sample_annot.  option: snpgdsOption(...) for cvt_chr="int" (chromosome labels through its codes, non-numeric ones become 0 with
    a warning); cvt_chr="char" keeps the labels.  cvt_snpid="auto" keeps the .bim ids when they are unique, else 1 ... n_snp.
    There is no snpgdsBED2GDS here: writing the GDS container is gdsfmt's work, which this package does not restate; the
    arguments that only shape that file (out.gdsfn, snpfirstdim, compress.*) have no counterpart."""
    if not isinstance(bed_fn, str):
        raise TypeError("is.character(bed.fn) is not TRUE")
    for v, name in ((family, "family"), (verbose, "verbose")):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    if fam_fn is None and bim_fn is None:
        import re
        fn = re.sub(r"\.bed$", "", bed_fn, flags=re.IGNORECASE)
        bed_fn, fam_fn, bim_fn = fn + ".bed", fn + ".fam", fn + ".bim"
    if not isinstance(fam_fn, str):
        raise TypeError("is.character(fam.fn) is not TRUE")
    if not isinstance(bim_fn, str):
        raise TypeError("is.character(bim.fn) is not TRUE")
    _cat(verbose, "Open a PLINK BED file as a SNP GDS object ...")
    bs = _bed.BedStream(bed_fn, fam_fn, bim_fn, family=family, option=option, cvt_chr=cvt_chr, cvt_snpid=cvt_snpid)
    if verbose:
        import os
        print("    BED file: '%s'" % bed_fn)
        print("        %s, %d bytes" % ("SNP-major mode (Sample X SNP)" if bs.mode else "individual-major mode (SNP X Sample)",
                                       os.path.getsize(bed_fn)))
        print("    FAM file: '%s'" % fam_fn)
        print("    BIM file: '%s'" % bim_fn)
        print("    %d samples, %d SNPs" % (bs.n_samp, bs.n_snp))
    return bs


class VcfGenoFile(GenoFile):
    """What snpgdsOpenVCF returns: a GenoFile (packed rows in host memory) with the nodes snpgdsVCF2GDS would have stored --
    snp_rs_id, snp_allele, snp_annot["qual"] / ["filter"] and the chromosome labels as text."""

    def __init__(self, packed, n_samp, sample_id, nodes):
        GenoFile.__init__(self, packed=packed, n_samp=n_samp, sample_id=sample_id, snp_id=nodes["snp_id"],
                          snp_chromosome=nodes["snp_chromosome"], snp_position=nodes["snp_position"], snp_allele=nodes["snp_allele"])
        self.snp_rs_id = nodes["snp_rs_id"]
        self.snp_annot = {"qual": nodes["qual"], "filter": nodes["filter"]}
        # text labels, as BedStream(cvt_chr="char"): autosome_only=True keeps the labels that parse into 1 ... 22
        self.chromosome_code = {}


def snpgdsOpenVCF(vcf_fn, method="biallelic.only", ref_allele=None, ignore_chr_prefix="chr", verbose=True, device=0):
    """Open VCF files for every snpgds* function: snpgdsVCF2GDS (R/Conversion.R:972-1155 -> gnrParseVCF4,
    src/ConvToGDS.cpp:667-997) + snpgdsOpen in one step, without the GDS file in between.  vcf_fn: a file name or a list of
    them (plain or .gz) with the same sample ids.  method "biallelic.only" keeps the lines whose REF and ALT are single
    nucleotides, "copy.num.of.ref" all; the genotype is the number of copies of the reference allele (0 / 1 / 2, 3 = missing).
    ref_allele: None, or one entry per data line of all files (None entries keep REF): the allele that is counted.
    The sample cells are parsed on the device (vcf.VcfReader -> snpgpu_vcf_genotypes) and the rows are kept in host memory, at
    most SNPGPU_VCF_MAX_BYTES (default 8 GiB) of them.  Returns a VcfGenoFile.  There is no CPU fallback: without a device the
    call fails with SnpGpuError.  There is no snpgdsVCF2GDS here, for the reason there is no snpgdsBED2GDS: writing the GDS
    container is gdsfmt's work, which this package does not restate."""
    import os
    files = [vcf_fn] if isinstance(vcf_fn, str) else list(vcf_fn)
    if not files or not all(isinstance(f, str) for f in files):
        raise TypeError("is.character(vcf.fn) & is.vector(vcf.fn) is not TRUE")
    if method not in _vcf.VcfReader.METHODS:
        raise ValueError("'arg' should be one of \"biallelic.only\", \"copy.num.of.ref\"")
    if ref_allele is not None and not all(a is None or isinstance(a, str) for a in ref_allele):
        raise TypeError("is.null(ref.allele) || is.character(ref.allele) is not TRUE")
    if not isinstance(ignore_chr_prefix, str) and not all(isinstance(a, str) for a in ignore_chr_prefix):
        raise TypeError("is.character(ignore.chr.prefix) is not TRUE")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    _cat(verbose, "Open VCF as a SNP GDS object ...")
    _cat(verbose, "Method: extracting biallelic SNPs" if method == "biallelic.only"
         else "Method: dosage (0,1,2) of reference allele for all variant sites")
    samp_id = None
    for fn in files:
        ids = _vcf.sample_ids(fn)
        if samp_id is None:
            samp_id = ids
            if len(samp_id) <= 0:
                raise ValueError("No sample in the VCF file!")
        elif ids != samp_id:
            raise ValueError("'%s' has different sample id." % fn)
    _cat(verbose, "Number of samples: %d" % len(samp_id))
    if _lib.device_count() < 1:
        raise _lib.SnpGpuError("snpgdsOpenVCF: no HIP device (the VCF genotype parser has no CPU fallback)")
    budget = int(os.environ.get("SNPGPU_VCF_MAX_BYTES", 8 << 30))
    rb = (len(samp_id) + 3) // 4
    parts, readers, held = [], [], 0
    next_id, lines = 1, 0
    for fn in files:
        _cat(verbose, "Parsing \"", fn, "\" ...")
        r = _vcf.VcfReader(fn, method=method, ref_allele=ref_allele, ignore_chr_prefix=ignore_chr_prefix, snp_id_start=next_id,
                           line_start=lines)
        for _, m, rows in r.blocks(65536, device=device):
            held += m * rb
            if held > budget:
                raise ValueError("the genotypes of %s need more than the %d bytes of SNPGPU_VCF_MAX_BYTES in host memory: read the "
                                 "file block by block with snprelate_amd.vcf.VcfReader.blocks instead" % (", ".join(files), budget))
            parts.append(rows.cpu().numpy())
        _cat(verbose, "\timport %d variant%s." % (r.n_snp, "s" if r.n_snp > 1 else ""))
        next_id, lines = r.next_snp_id, r.lines_seen
        readers.append(r)
    if not sum(r.n_snp for r in readers):
        raise ValueError("No variant in the VCF file%s (method \"%s\")" % ("s" if len(files) > 1 else "", method))
    cat = lambda name: np.concatenate([getattr(r, name) for r in readers])          # noqa: E731
    nodes = dict(snp_id=cat("snp_id"), snp_chromosome=cat("snp_chromosome"), snp_position=cat("snp_position"),
                 snp_allele=cat("snp_allele"), snp_rs_id=cat("snp_rs_id"),
                 qual=np.concatenate([r.snp_annot["qual"] for r in readers]),
                 filter=np.concatenate([r.snp_annot["filter"] for r in readers]))
    return VcfGenoFile(np.concatenate(parts, 0), len(samp_id), np.array(samp_id), nodes)


def _bim_chromosomes(gdsobj, chrom):
    """the chromosome column of snpgdsGDS2BED (R/Conversion.R:354-379): labels through the object's chromosome codes, then PLINK's
    numbers for X, Y, XY, M / MT when the autosomes are 1 ... 22.  The two substitutions run one after the other as the reference
    runs them, so that with the default codes (XY = 24, Y = 25) 24 is written as 25 and 25 as 24."""
    x = np.array([str(c) for c in chrom], dtype=object)
    a0, a1 = getattr(gdsobj, "autosome_start", 1), getattr(gdsobj, "autosome_end", 22)
    code = getattr(gdsobj, "chromosome_code", None)
    if code is None:
        code = _bed.default_option(a0, a1)["chromosome_code"]
    for name, c in code.items():
        x[x == str(c)] = name
    if a0 == 1 and a1 == 22:
        for name, c in (("X", "23"), ("Y", "24"), ("XY", "25"), ("M", "26"), ("MT", "26")):
            x[x == name] = c
    return x


def snpgdsGDS2BED(gdsobj, bed_fn, sample_id=None, snp_id=None, snpfirstdim=None, verbose=True, device=0):
    """Write the selected genotypes as PLINK binary PED (R/Conversion.R:310-425): bed_fn + ".bed", ".bim", ".fam".  gdsobj: a
    SNP GDS object of any kind -- a BedStream gives BED -> BED subsetting -- or the name of a GDS file.  The selection follows FILE
    order.  snpfirstdim=True writes mode byte 0 (individual-major), False mode byte 1 (SNP-major); None follows the object's
    layout (a sample.order file gives False).  .bim: tab-separated, genetic distance 0, alleles from snp_allele or A / B with the
    reference's warning; .fam: 0, id, 0, 0, 0, -9.  The genotype bytes come from the device (snpgpu_geno_convert) in the file's
    layout, block by block; without a visible device numpy writes the same bytes."""
    opened = isinstance(gdsobj, str)
    if opened:
        gdsobj = snpgdsOpen(gdsobj, stream=True)
    if not isinstance(gdsobj, (GenoFile, _gds.GenoStream)):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    if not isinstance(bed_fn, str):
        raise TypeError("is.character(bed.fn) is not TRUE")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    if snpfirstdim is not None and not isinstance(snpfirstdim, (bool, np.bool_)):
        raise TypeError("is.logical(snpfirstdim) is not TRUE")
    flags = []
    for want, have, name, what in ((sample_id, gdsobj.sample_id, "sample.id", "sample"), (snp_id, gdsobj.snp_id, "snp.id", "SNP")):
        f = np.ones(len(have), bool)
        if want is not None:
            f = np.isin(have, np.asarray(want))
            if int(f.sum()) != len(want):
                raise ValueError("Some of %s do not exist!" % name)
            if f.sum() <= 0:
                raise ValueError("No %s in the working dataset." % what)
        flags.append(f)
    samp_flag, snp_flag = flags
    if snpfirstdim is None:
        snpfirstdim = not getattr(gdsobj, "sample_order", True)
    n, ns, Ls = gdsobj.n_samp, int(samp_flag.sum()), int(snp_flag.sum())
    _cat(verbose, "Converting from GDS to PLINK binary PED:")
    _cat(verbose, "Working space: %d samples, %d SNPs" % (ns, Ls))

    if gdsobj.snp_position is None:
        raise ValueError("the object has no snp.position, which the .bim file needs")
    allele = getattr(gdsobj, "snp_allele", None)
    if allele is not None:
        parts = [str(a).split("/") for a in np.asarray(allele)[snp_flag]]
        ref, nonref = [p[0] for p in parts], [p[1] if len(p) > 1 else "" for p in parts]
    else:
        warnings.warn("There is no allele information in the GDS file. ``A/B'' is used for the last two columns.")
        ref, nonref = ["A"] * Ls, ["B"] * Ls
    xchr = _bim_chromosomes(gdsobj, np.asarray(gdsobj.snp_chromosome)[snp_flag])
    with open(bed_fn + ".bim", "w") as f:
        for c, rs, pos, a, b in zip(xchr, gdsobj.snp_id[snp_flag], gdsobj.snp_position[snp_flag], ref, nonref):
            f.write("%s\t%s\t0\t%d\t%s\t%s\n" % (c, rs, pos, a, b))
    _cat(verbose, "Output a BIM file.")
    with open(bed_fn + ".fam", "w") as f:
        for sid in gdsobj.sample_id[samp_flag]:
            f.write("0\t%s\t0\t0\t0\t-9\n" % sid)
    _cat(verbose, "Output a BED file ...")

    # the body, in blocks of selected SNPs (a multiple of 4, so that a block is whole bytes of an individual-major row too)
    rows, cols = (ns, Ls) if snpfirstdim else (Ls, ns)
    with open(bed_fn + ".bed", "wb") as f:
        f.write(_bed.MAGIC + bytes([0 if snpfirstdim else 1]))
        f.truncate(3 + rows * ((cols + 3) // 4))
    body = np.memmap(bed_fn + ".bed", dtype=np.uint8, mode="r+", offset=3, shape=(rows, (cols + 3) // 4))
    try:
        for a, b, blk in _bed_blocks(gdsobj, samp_flag, snp_flag, bool(snpfirstdim), 65536, device):
            if snpfirstdim:
                body[:, a >> 2:(b + 3) >> 2] = blk
            else:
                body[a:b] = blk
        body.flush()
    finally:
        del body
        if opened:
            snpgdsClose(gdsobj)
    _cat(verbose, "Done.")
    return None


def _bed_blocks(gdsobj, samp_flag, snp_flag, individual_major, block, device):
    """(a, b, bytes) for the selected SNPs a ... b - 1 of snpgdsGDS2BED: their .bed bytes of the selected samples, uint8
    [b - a][ceil(n_sel / 4)], or for individual_major [n_sel][ceil((b - a) / 4)].  With a device: one snpgpu_geno_convert per block
    -- from the packed rows in host memory, or, for a stream that is read whole (no SNP selection) and not yet in memory, from
    the device rows select_blocks lays out.  Without one: numpy (bed.encode_bed)."""
    n, rb = gdsobj.n_samp, (gdsobj.n_samp + 3) // 4
    samp_index = None if samp_flag.all() else np.flatnonzero(samp_flag).astype(np.int32)
    ns = n if samp_index is None else len(samp_index)
    dm = 1 if individual_major else 0
    on_device = _device_visible()
    if on_device and isinstance(gdsobj, _gds.GenoStream) and getattr(gdsobj, "_packed", None) is None and snp_flag.all():
        for lo, m, rows in gdsobj.select_blocks(block, samp_index=samp_index, device=device, to="device"):
            rbs = (ns + 3) // 4
            yield lo, lo + m, _lib.geno_convert(int(rows.data_ptr()), 0, m, ns, dst_code=_lib.CODE_BED, dst_major=dm,
                                                row_stride_bits=8 * rbs, n_bytes=m * rbs, device=device)
        return
    packed, pos = gdsobj.packed, np.flatnonzero(snp_flag)
    for a in range(0, len(pos), block):
        b = min(a + block, len(pos))
        k0, k1 = int(pos[a]), int(pos[b - 1]) + 1
        idx = None if k1 - k0 == b - a else (pos[a:b] - k0).astype(np.int32)
        if on_device:
            src, m, cols, sel = packed[k0:k1], k1 - k0, n, samp_index
            if individual_major and sel is not None:
                # samples are the rows of dst here, and a list of them cuts the transposition into one segment per run of
                # consecutive samples: select first, then transpose all
                src = _lib.geno_select(src, 0, m, n, row_stride_bits=8 * rb, samp_index=sel, snp_index=idx, device=device)
                m, cols, sel, idx = b - a, ns, None, None
            yield a, b, _lib.geno_convert(src, 0, m, cols, dst_code=_lib.CODE_BED, dst_major=dm, row_stride_bits=8 * ((cols + 3) // 4),
                                          samp_index=sel, snp_index=idx, device=device)
        else:
            g = _gds.unpack_2bit_rows(packed[k0:k1] if idx is None else packed[k0:k1][idx], n)
            yield a, b, _bed.encode_bed(g if samp_index is None else g[:, samp_index], individual_major)


def _file_order_flags(gdsobj, sample_id, snp_id, between=None):
    """the selection flags of snpgdsGDS2PED / snpgdsGDS2Eigen (R/Conversion.R:34-64, :702-734): ids %in% the wanted ones, in FILE
    order, with the reference's messages; `between` runs after the sample check, as the reference prints its first line there"""
    flags = []
    for want, have, name, what in ((sample_id, gdsobj.sample_id, "sample.id", "sample"), (snp_id, gdsobj.snp_id, "snp.id", "SNP")):
        f = np.ones(len(have), bool)
        if want is not None:
            want = np.asarray(want).reshape(-1)
            f = np.isin(have, want)
            if int(f.sum()) != len(want):
                raise ValueError("Some of %s do not exist!" % name)
            if f.sum() <= 0:
                raise ValueError("No %s in the working dataset." % what)
        flags.append(f)
        if between is not None and len(flags) == 1:
            between()
    return flags


def _text_gdsobj(gdsobj):
    opened = isinstance(gdsobj, str)
    if opened:
        gdsobj = snpgdsOpen(gdsobj, stream=True)
    if not isinstance(gdsobj, (GenoFile, _gds.GenoStream)):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    return gdsobj


def snpgdsGDS2PED(gdsobj, ped_fn, sample_id=None, snp_id=None, use_snp_rsid=True, format="A/G/C/T", verbose=True, device=0):
    """Write the selected genotypes as PLINK text PED (R/Conversion.R:26-124 -> gnrConvGDS2PED, src/SNPRelate.cpp:685-767):
    ped_fn + ".map" and ped_fn + ".ped".  gdsobj: a SNP GDS object of any kind (GenoFile, GenoStream, BedStream, the VCF GenoFile)
    or the name of a GDS file.  The selection follows FILE order.  format "A/G/C/T" writes the alleles of snp_allele ("s1/s2":
    a third allele is ignored, an empty one is "0"; an allele may be any length) -- genotype 0 / 1 / 2 / missing is "s2 s2" /
    "s1 s2" / "s1 s1" / "0 0" --, "A/B" the letters A and B, "1/2" the digits.  .map: tab-separated chromosome (23 -> X, 25 -> Y,
    24 -> XY, 26 -> MT, the reference's four substitutions), snp_rs_id when the object has it and use_snp_rsid is set, else
    snp_id, genetic distance 0, position.  .ped: "0 ID 0 0 0 -9" and the genotypes, tab-separated, one line per sample; its bytes
    are made on the device (text.write_ped -> snpgpu_text_render) in windows of SNPGPU_TEXT_STAGE_BYTES and appended to the file.
    There is no CPU fallback: without a device the call fails with SnpGpuError."""
    from . import text as _text
    gdsobj = _text_gdsobj(gdsobj)
    if not isinstance(ped_fn, str):
        raise TypeError("is.character(ped.fn) is not TRUE")
    format = _match_arg(format, ("A/G/C/T", "A/B", "1/2"), "arg")
    samp_flag, snp_flag = _file_order_flags(gdsobj, sample_id, snp_id, lambda: _cat(verbose, "Converting from GDS to PLINK PED:"))
    alleles = None
    if format == "A/G/C/T":
        al = getattr(gdsobj, "snp_allele", None)
        if al is None:
            raise ValueError("There is no 'snp.allele' variable in the GDS file.")
        if len(al) != len(gdsobj.snp_id):
            raise ValueError("Invalid 'snp.allele' in the GDS file.")
        alleles = _text.split_alleles(np.asarray(al)[snp_flag])
    fmt = {"A/G/C/T": _lib.TEXT_PED_ALLELE, "A/B": _lib.TEXT_PED_AB, "1/2": _lib.TEXT_PED_12}[format]

    rs = gdsobj.snp_id
    if use_snp_rsid and getattr(gdsobj, "snp_rs_id", None) is not None:
        rs = gdsobj.snp_rs_id
    if gdsobj.snp_position is None:
        raise ValueError("the object has no snp.position, which the .map file needs")
    sub = {"23": "X", "25": "Y", "24": "XY", "26": "MT"}
    with open(ped_fn + ".map", "w") as f:
        for c, r, pos in zip(np.asarray(gdsobj.snp_chromosome)[snp_flag], np.asarray(rs)[snp_flag], gdsobj.snp_position[snp_flag]):
            c = str(c)
            f.write("%s\t%s\t0\t%d\n" % (sub.get(c, c), r, pos))
    _cat(verbose, "\tOutput a MAP file DONE.")
    _cat(verbose, "\tOutput a PED file ...")
    with open(ped_fn + ".ped", "wb") as f:
        _text.write_ped(f, gdsobj, samp_flag, snp_flag, [str(x) for x in np.asarray(gdsobj.sample_id)[samp_flag]], fmt, alleles, device)
    return None


def snpgdsGDS2Eigen(gdsobj, eigen_fn, sample_id=None, snp_id=None, verbose=True, device=0):
    """Write the selected genotypes in EIGENSTRAT format (R/Conversion.R:695-785 -> gnrConvGDS2EIGEN, src/SNPRelate.cpp:828-859):
    eigen_fn + ".snp" (id, chromosome, 0, position), ".ind" (id, sex, "control") and ".eigenstratgeno" (one line per SNP, one
    digit per sample: the genotype, 9 = missing).  gdsobj and the selection as snpgdsGDS2PED.  The sex column is
    sample_annot["sex"]: every value must be "M" or "F" (the reference's message otherwise), a missing value (None / NaN) is
    "U", and so is every sample when the object has no such column.  The genotype lines are made on the device
    (text.write_eigenstratgeno -> snpgpu_text_render); there is no CPU fallback."""
    from . import text as _text
    gdsobj = _text_gdsobj(gdsobj)
    if not isinstance(eigen_fn, str):
        raise TypeError("is.character(eigen.fn) is not TRUE")
    samp_flag, snp_flag = _file_order_flags(gdsobj, sample_id, snp_id, lambda: _cat(verbose, "Converting from GDS to EIGENSOFT:"))
    if gdsobj.snp_position is None:
        raise ValueError("the object has no snp.position, which the .snp file needs")
    Ls, ns = int(snp_flag.sum()), int(samp_flag.sum())
    with open(eigen_fn + ".snp", "w") as f:
        for i, c, pos in zip(np.asarray(gdsobj.snp_id)[snp_flag], np.asarray(gdsobj.snp_chromosome)[snp_flag],
                             gdsobj.snp_position[snp_flag]):
            f.write("%s\t%s\t0\t%d\n" % (i, c, pos))
    _cat(verbose, "\tsave to *.snp: %d snps" % Ls)
    sex = getattr(gdsobj, "sample_annot", {}).get("sex")
    if sex is None:
        sex = ["U"] * ns
    else:
        sex = [None if _is_na(x) else str(x) for x in np.asarray(sex, dtype=object)[samp_flag]]
        if not all(x in ("F", "M") for x in sex if x is not None):
            raise ValueError("The gender variable in GDS file should be either \"M\" or \"F\".")
        sex = ["U" if x is None else x for x in sex]
    with open(eigen_fn + ".ind", "w") as f:
        for sid, x in zip(np.asarray(gdsobj.sample_id)[samp_flag], sex):
            f.write("%s\t%s\tcontrol\n" % (sid, x))
    _cat(verbose, "\tsave to *.ind: %d samples" % ns)
    with open(eigen_fn + ".eigenstratgeno", "wb") as f:
        _text.write_eigenstratgeno(f, gdsobj, samp_flag, snp_flag, device)
    _cat(verbose, "Done.")
    return None


def snpgdsOpenPED(ped_fn, map_fn, family=True, verbose=True, device=0):
    """Open a PLINK text PED/MAP pair for every snpgds* function: snpgdsPED2GDS (R/Conversion.R:132-302 -> gnrParsePED,
    src/ConvToGDS.cpp:1175-1361) + snpgdsOpen in one step, without the GDS file in between.  ped_fn: plain or .gz.  Returns a
    GenoFile: snp_id 1 ... n_snp, snp_rs_id / snp_position / snp_chromosome the MAP columns in the order of R/Conversion.R:164-170
    (chromosome, then position; a numeric chromosome column as integers, else as text with the labels compared as bytes), snp_allele
    "ref/alt1,alt2" with the most frequent allele as the reference (ties to the smaller string, "0" for an empty side), genotypes
    the number of reference alleles (3 when either allele is "0"), sample_id column 2, and with `family` the sample_annot columns
    family, father, mother, sex ("1" -> "M", "2" -> "F", anything else kept) and phenotype.
    The allele tokens are read on the device (ped.PedReader: snpgpu_ped_tokens / _census / _codes, two sweeps over the text as the
    reference reads the file twice) in chunks of SNPGPU_TEXT_STAGE_BYTES; lines the kernel flags (alleles of several bytes,
    quoted or empty tokens) are settled on the host, and a wrong number of columns raises the reference's message with FILE:,
    LINE:, COLUMN:.  There is no CPU fallback: without a device the call fails with SnpGpuError.
    One deviation from the reference: gnrParsePED appends snp.allele in FILE order while it permutes the genotypes, rs ids and
    positions by the MAP order (src/ConvToGDS.cpp:1272-1276 against :1353-1355), so that with an unsorted MAP its alleles belong
    to other SNPs; here snp_allele is permuted with the rest.  For a sorted MAP nothing differs.
    There is no snpgdsPED2GDS here, for the reason there is no snpgdsBED2GDS: writing the GDS container is gdsfmt's work."""
    from . import ped as _ped
    if not isinstance(ped_fn, str):
        raise TypeError("is.character(ped.fn) is not TRUE")
    if not isinstance(map_fn, str):
        raise TypeError("is.character(map.fn) is not TRUE")
    for v, name in ((family, "family"), (verbose, "verbose")):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    _cat(verbose, "Open PLINK PED/MAP as a SNP GDS object ...")
    m = _ped.read_map(map_fn)
    ii = m["ii"]
    M = len(ii)
    if np.any(ii[1:] < ii[:-1]):
        print("Hint: the SNPs are sorted and merged into the GDS file.")
    _cat(verbose, "Import %d variant%s from '%s'" % (M, "s" if M > 1 else "", map_fn))
    if not _device_visible():
        raise _lib.SnpGpuError("snpgdsOpenPED: no HIP device (the PED tokeniser has no CPU fallback)")
    _cat(verbose, "Reading '", ped_fn, "'")
    r = _ped.PedReader(ped_fn, M, device=device).run()
    N, rb = r.n_samp, (M + 3) // 4
    _cat(verbose, "Import %d sample%s" % (N, "s" if N > 1 else ""))
    # sample rows in FILE order of the SNPs -> SNP rows in the MAP order
    packed = _lib.geno_convert(int(r.rows.data_ptr()), 1, N, M, row_stride_bits=8 * rb, n_bytes=N * rb, snp_index=ii.astype(np.int32),
                               device=device)
    gf = GenoFile(packed=packed, n_samp=N, sample_id=r.sample_id, snp_id=np.arange(1, M + 1, dtype=np.int32),
                  snp_chromosome=m["snp_chromosome"], snp_position=m["snp_position"], snp_allele=r.snp_allele[ii],
                  sample_annot=r.sample_annot if family else None)
    gf.snp_rs_id = m["snp_rs_id"]
    gf.ped_flagged_lines, gf.ped_windows = r.flagged_lines, r.windows
    if m["snp_chromosome"].dtype.kind == "U":
        gf.chromosome_code = {}                            # text labels, as snpgdsOpenVCF keeps them
    return gf


def snpgdsOpenGEN(gen_fn, sample_fn, chr_code=None, call_threshold=0.9, version=">=2.0", verbose=True, device=0):
    """Open Oxford GEN files (IMPUTE2, SNPTEST, SHAPEIT) and their sample file for every snpgds* function: snpgdsGEN2GDS
    (R/Conversion.R:795-964 -> gnrParseGEN, src/ConvToGDS.cpp:1015-1157) + snpgdsOpen in one step, without the GDS file in between.
    gen_fn: a file name or a list of them (plain or .gz), appended in order; chr_code: one entry per file, all numbers (integers,
    NA -> 0) or all strings.  A sample is called AA (2), AB (1) or BB (0) when the largest of its three probabilities, read as
    strtof reads them, is >= call_threshold, else it is missing (3).  version ">=2.0": the sample file has a line of column types
    under its header; "<=1.1.5": it has none.  Returns a GenoFile: sample_id the sample file's first column, all its columns in
    sample_annot under the header's names (text), snp_id column 1 of the .gen lines (text), snp_rs_id column 2, snp_position
    column 3, snp_allele "A/B" of columns 4 and 5, snp_chromosome the file's chr_code.
    The probabilities are read and called on the device (gen.GenReader -> snpgpu_gen_genotypes) in chunks of
    SNPGPU_TEXT_STAGE_BYTES; lines the kernel flags (exponents, signs, quotes, '\\r', "." ...) are settled on the host by
    snpgpu_gen_line_host, and a malformed line raises the reference's message with FILE:, LINE:, COLUMN:.  There is no CPU
    fallback: without a device the call fails with SnpGpuError.  There is no snpgdsGEN2GDS here, for the reason there is no
    snpgdsBED2GDS: writing the GDS container is gdsfmt's work."""
    from . import gen as _gen
    files = [gen_fn] if isinstance(gen_fn, str) else list(gen_fn)
    if not files or not all(isinstance(f, str) for f in files):
        raise TypeError("is.character(gen.fn) & is.vector(gen.fn) is not TRUE")
    if not isinstance(sample_fn, str):
        raise TypeError("is.character(sample.fn) & is.vector(sample.fn) is not TRUE")
    if chr_code is None:
        raise ValueError("Please specify the argument 'chr.code', e.g., 'chr.code=1'.")
    codes = [chr_code] if isinstance(chr_code, (str, int, float, np.integer, np.floating)) else list(chr_code)
    is_text = all(c is None or isinstance(c, str) for c in codes) and any(isinstance(c, str) for c in codes)
    if not is_text and not all(c is None or _is_number(c) for c in codes):
        raise TypeError("is.numeric(chr.code) | is.character(chr.code) is not TRUE")
    if len(codes) != len(files):
        raise ValueError("length(gen.fn) == length(chr.code) is not TRUE")
    if not _is_number(call_threshold) or not math.isfinite(float(call_threshold)):
        raise TypeError("is.finite(call.threshold) is not TRUE")
    if version not in _gen.VERSIONS:
        raise ValueError("'arg' should be one of \">=2.0\", \"<=1.1.5\"")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    _cat(verbose, "Oxford GEN/BGEN format ---> GDS SNP format:")
    if is_text:
        codes = ["" if c is None else c for c in codes]
    else:
        codes = [0 if c is None or _is_na(c) else int(c) for c in codes]
    samp_id, annot = _gen.read_sample(sample_fn, version)
    N, rb = len(samp_id), (len(samp_id) + 3) // 4
    _cat(verbose, "The number of samples: %d, with SNPTEST version (%s)." % (N, version))
    if not _device_visible():
        raise _lib.SnpGpuError("snpgdsOpenGEN: no HIP device (the GEN genotype caller has no CPU fallback)")
    parts, readers, chrom = [], [], []
    for fn, code in zip(files, codes):
        _cat(verbose, "Parsing \"", fn, "\" ...")
        r = _gen.GenReader(fn, N, call_threshold)
        for _, m, rows in r.blocks(4096, device=device):
            parts.append(rows.cpu().numpy())
        _cat(verbose, "\tImport %d variant%s on chromosome %s." % (r.n_snp, "s" if r.n_snp > 1 else "", code))
        chrom += [code] * r.n_snp
        readers.append(r)
    if not chrom:
        raise ValueError("No variant in the GEN file%s" % ("s" if len(files) > 1 else ""))
    cat = lambda name: np.concatenate([getattr(r, name) for r in readers])          # noqa: E731
    gf = GenoFile(packed=np.concatenate(parts, 0), n_samp=N, sample_id=samp_id, snp_id=cat("snp_id"),
                  snp_chromosome=np.array(chrom, dtype=str) if is_text else np.array(chrom, np.int32),
                  snp_position=cat("snp_position"), snp_allele=cat("snp_allele"), sample_annot=annot)
    gf.snp_rs_id = cat("snp_rs_id")
    gf.gen_flagged_lines, gf.gen_windows = sum(r.flagged_lines for r in readers), sum(r.windows for r in readers)
    if is_text:
        gf.chromosome_code = {}                            # text labels, as snpgdsOpenVCF keeps them
    return gf


def snpgdsHWE(gdsobj, sample_id=None, snp_id=None, with_id=False, device=0):
    """p-value per SNP of the exact test of Hardy-Weinberg equilibrium (R/AllUtilities.R:255-279 -> gnrHWE,
    src/genHWE.cpp:46-137; Wigginton, Cutler & Abecasis 2005) on (AA = #g==2, AB = #g==1, BB = #g==0); NaN without a call.
    with_id: dict(pvalue, sample_id, snp_id)."""
    if not isinstance(with_id, (bool, np.bool_)):
        raise TypeError("is.logical(with.id) is not TRUE")
    ws = _init_file(gdsobj, sample_id, snp_id, device)
    rv = np.empty(ws["n_snp"], np.float64)
    _lib.check(_lib.lib().snpgpu_gnrHWE(_lib._ptr(rv)))
    if with_id:
        return dict(pvalue=rv, sample_id=ws["sample_id"], snp_id=ws["snp_id"])
    return rv


def snpgdsSelectSNP(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True, maf=float("nan"),
                    missing_rate=float("nan"), verbose=True, device=0):
    """The candidate SNPs that pass the filters (R/AllUtilities.R:286-299): ws$snp.id of .InitFile2"""
    ws = _init_file2(None, gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate, 1, verbose, device)
    return ws["snp_id"]


def _inb_mle_host(g, p, reltol):
    """_inb_mle<int> (src/genIBD.cpp:1393-1438) for one individual in numpy: g int (anything outside 0 ... 2 is skipped), p the
    allele frequencies.  The sums over the SNPs are numpy's (pairwise), not the reference's sequential ones."""
    with np.errstate(all="ignore"):
        called = (g >= 0) & (g <= 2)
        gc, pc = g[called].astype(np.float64), p[called]
        F = np.float64(np.sum(gc * gc - (1 + 2 * pc) * gc + 2 * pc * pc)) / np.float64(np.sum(2 * pc * (1 - pc)))
        if not np.isfinite(F):
            return float(F)
        F = min(max(F, 0.001), 1 - 0.001)
        het, hom = gc == 1, gc != 1
        x = np.where(gc == 0, 1 - pc, pc)
        n_het = int(het.sum())

        def loglik(F):
            val = np.log(np.where(het, (1 - F) * 2 * pc * (1 - pc), (1 - F) * x * x + F * x))
            return float(np.sum(val[np.isfinite(val)]))

        L = loglik(F)
        contol = abs(L) * reltol
        for _ in range(10000):
            old = L
            tmp = (F / (F + x * (1 - F)))[hom]
            ok = np.isfinite(tmp)
            m = int(ok.sum()) + n_het
            F = np.float64(np.sum(tmp[ok])) / np.float64(m)
            L = loglik(F)
            if abs(L - old) <= contol:
                break
        return float(F)


def snpgdsIndInbCoef(x, p, method="mom.weir", reltol=_RELTOL_INB):
    """Inbreeding coefficient of one individual from genotypes x and allele frequencies p (R/AllUtilities.R:312-341).  All three
    methods run on the host in numpy: the two moment methods as the R code does, "mle" through _inb_mle_host, a numpy routine
    that follows gnrIndInbCoef -> _inb_mle<int> (src/genIBD.cpp:1393-1438, :1814-1827) step by step."""
    method = _match_arg(method, INB_COEF_METHODS, "method")
    reltol = _scalar_reltol(reltol)
    x = np.asarray(x)
    p = np.asarray(p)
    for name, v in (("x", x), ("p", p)):
        if v.ndim != 1 or v.dtype.kind not in "iuf":
            raise TypeError("is.vector(%s) & is.numeric(%s) is not TRUE" % (name, name))
    if len(x) != len(p):
        raise ValueError("length(x) == length(p) is not TRUE")
    x = x.astype(np.float64)
    p = p.astype(np.float64)
    x[~np.isin(x, (0, 1, 2))] = np.nan
    with np.errstate(all="ignore"):
        if method == "mom.weir":
            num = x * x - (1 + 2 * p) * x + 2 * p * p
            den = 2 * p * (1 - p)
            flag = np.isfinite(num) & np.isfinite(den)
            return float(np.float64(np.sum(num[flag])) / np.float64(np.sum(den[flag])))
        if method == "mom.visscher":
            d = (x * x - (1 + 2 * p) * x + 2 * p * p) / (2 * p * (1 - p))
            d = d[np.isfinite(d)]
            return float(d.mean()) if len(d) else float("nan")
    g = np.where(np.isnan(x), -1, x).astype(np.int64)
    return _inb_mle_host(g, p, reltol)


def snpgdsIndInb(gdsobj, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True, maf=float("nan"),
                 missing_rate=float("nan"), method="mom.weir", allele_freq=None, out_num_iter=True, reltol=_RELTOL_INB,
                 verbose=True, device=0):
    """Individual inbreeding coefficients (R/AllUtilities.R:349-378 -> gnrIndInb, src/genIBD.cpp:1847-2006): dict(sample_id,
    snp_id, inbreeding[, out_num_iter]).  Methods "mom.weir", "mom.visscher", "mle", "gcta1", "gcta2", "gcta3".  The moment methods
    are the reference's sequential fp64 sums bit for bit (one lane per sample walks the SNPs in order); "mle" iterates per sample on
    the GPU with sums reduced in a wave and also returns out_num_iter (int32) unless out_num_iter is False.  Without allele_freq
    the frequencies come from the selected genotypes, as in the reference (gnrSNPFreq for "mle", calc_afreq otherwise)."""
    method = _match_arg(method, INB_METHODS, "method")
    if not isinstance(out_num_iter, (bool, np.bool_)):
        raise TypeError("is.logical(out.num.iter) is not TRUE")
    reltol = _scalar_reltol(reltol)
    ws = _init_file2("Estimating individual inbreeding coefficients:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp,
                     maf, missing_rate, 1, verbose, device, allele_freq=allele_freq)
    n = ws["n_samp"]
    if ws["n_snp"] < 1:
        raise ValueError("snpgdsIndInb: no SNP in the working dataset")
    coeff = np.empty(n, np.float64)
    want_iter = method == "mle" and bool(out_num_iter)
    niter = np.empty(n, np.int32) if want_iter else None
    _lib.check(_lib.lib().snpgpu_gnrIndInb(_lib._ptr(ws["allele_freq"]), method.encode(), reltol, int(want_iter),
                                           int(bool(verbose)), _lib._ptr(coeff), _lib._ptr(niter)))
    rv = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"], inbreeding=coeff)
    if want_iter:
        rv["out_num_iter"] = niter
    return rv


# ---- genotype scores of listed sample pairs ---------------------------------------------------------------------------------------------

PAIR_METHODS = _lib.PAIR_METHODS
PAIR_TYPES = _lib.PAIR_TYPES


def _any_duplicated(x):
    x = np.asarray(x)
    return len(np.unique(x)) != len(x)


def _check_selection(gdsobj, sample_id, snp_id):
    """the refusals of .InitFile (R/Internal.R:64-160) that depend on the selection alone, with its messages"""
    if not isinstance(gdsobj, GenoFile):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    for want, have, name, what in ((sample_id, gdsobj.sample_id, "sample.id", "sample"), (snp_id, gdsobj.snp_id, "snp.id", "SNP")):
        if want is None:
            continue
        n = int(np.isin(have, np.asarray(want)).sum())
        if n != len(want):
            raise ValueError("Some of %s do not exist!" % name)
        if n <= 0:
            raise ValueError("No %s in the working dataset." % what)


def snpgdsPairScore(gdsobj, sample1_id, sample2_id, snp_id=None, method="IBS", type="per.pair", dosage=True, with_id=True,
                    output=None, verbose=True, device=0):
    """Genotype scores of the pairs (sample1_id[j], sample2_id[j]) over the SNPs (R/IBS.R:81-184 -> gnrPairScore,
    src/genIBS.cpp:690-891).  The working set is the union of the two lists with the selected SNPs, no filter.  Returns a dict:
    sample_id, snp_id (unless with_id is False) and score --
      type "per.pair"  dict of columns Avg, SD, Num (int32), Sample1, Sample2 (R's data.frame)
      type "per.snp"   float64 [3][n_snp], rows Avg / SD / Num
      type "matrix"    int32 [n_pair][n_snp], NA_integer_ (-2^31) where a genotype is missing
      type "gds.file"  nothing in the dict: the reference writes a GDS file through gdsfmt, which is not available to this Python
                       mirror; as snpgdsGRM(out_fn=) does, THE SAME NODES (sample.id = "id1-id2", snp.id, snp.position,
                       snp.chromosome, genotype) are stored in a numpy archive under the name `output`.  genotype is uint8
                       [n_pair][n_snp] holding the two bits the bit2 node keeps (3 = missing, and 3 for a score of -1); the
                       node's "sample.order" attribute is stored as an entry of its own.
    Avg, SD and Num come from exact integer tables counted on the GPU and equal the reference's sequential double sums bit for
    bit, its quirks included: the *.only methods score -1 at some cells where both genotypes are called."""
    if _any_duplicated(sample1_id):
        raise ValueError("'sample1.id' has duplicated element(s).")
    if _any_duplicated(sample2_id):
        raise ValueError("'sample2.id' has duplicated element(s).")
    s1, s2 = np.asarray(sample1_id), np.asarray(sample2_id)
    if len(s1) != len(s2):
        raise ValueError("length(sample1.id) == length(sample2.id) is not TRUE")
    union = np.concatenate([s1, s2])
    _, first = np.unique(union, return_index=True)
    union = union[np.sort(first)]
    # .InitFile comes here in R.  What it can refuse is checked now and the working space is set after the argument checks below,
    # so that R's order of errors is kept and every one of them is raised before a device is touched.
    _check_selection(gdsobj, union, snp_id)

    method = _match_arg(method, PAIR_METHODS, "method")
    type = _match_arg(type, PAIR_TYPES, "type")
    for name, v in (("with.id", with_id), ("dosage", dosage)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    if type == "gds.file":
        if not isinstance(output, str):
            raise TypeError("is.character(output) & is.vector(output) is not TRUE")
    elif output is not None:
        raise ValueError("'output' should be NULL, if 'type' is not \"gds.file\".")

    ws = _init_file(gdsobj, union, snp_id, device)
    if verbose:
        print("Pair Score Calculation:")
        print("    # of samples: %s" % _pretty(ws["n_samp"]))
        print("    # of SNPs: %s" % _pretty(ws["n_snp"]))
        print("Method: %s" % method)
        if type == "gds.file":
            print("Output: %s" % output)

    # match(sampleX.id, ws$sample.id) - 1L
    order = np.argsort(ws["sample_id"], kind="stable")
    sorted_ids = np.asarray(ws["sample_id"])[order]
    idx1 = np.ascontiguousarray(order[np.searchsorted(sorted_ids, s1)], np.int32)
    idx2 = np.ascontiguousarray(order[np.searchsorted(sorted_ids, s2)], np.int32)
    n_pair, n_snp = len(idx1), ws["n_snp"]
    if n_snp < 1:
        raise ValueError("snpgdsPairScore: no SNP in the working dataset")
    if type == "per.pair":
        out = np.empty((3, n_pair), np.float64)                       # n_pair x 3, column-major
    elif type == "per.snp":
        out = np.empty((n_snp, 3), np.float64)                        # 3 x n_snp, column-major
    else:
        out = np.empty((n_snp, n_pair), np.int32 if type == "matrix" else np.uint8)
    _lib.check(_lib.lib().snpgpu_gnrPairScore(_lib._ptr(idx1), _lib._ptr(idx2), n_pair, method.encode(), type.encode(),
                                              int(bool(dosage)), int(bool(verbose)), _lib._ptr(out)))
    ans = dict(sample_id=ws["sample_id"], snp_id=ws["snp_id"]) if with_id else {}
    if type == "per.pair":
        ans["score"] = dict(Avg=out[0], SD=out[1], Num=out[2].astype(np.int32), Sample1=s1, Sample2=s2)
    elif type == "per.snp":
        ans["score"] = out.T
    elif type == "matrix":
        ans["score"] = out.T
    else:
        flag = np.isin(gdsobj.snp_id, ws["snp_id"])
        nodes = {"sample.id": np.array(["%s-%s" % (a, b) for a, b in zip(s1, s2)]), "snp.id": ws["snp_id"],
                 "snp.chromosome": np.asarray(gdsobj.snp_chromosome)[flag], "genotype": out.T,
                 "genotype.attr": np.array(["sample.order"])}
        if gdsobj.snp_position is not None:
            nodes["snp.position"] = np.asarray(gdsobj.snp_position)[flag]
        _gds.write_output(output, nodes)
    return ans


# ---- hierarchical clustering and the permutation test of the tree ---------------------------------------------------------------------


def snpgdsHCluster(dist, sample_id=None, need_mat=True, hang=0.25):
    """Average-linkage clustering of a dissimilarity matrix (R/AllUtilities.R:386-424 -> hclust(as.dist(dist), "average"), here
    snpgpu_hclust_average on the host).

    Results in this mirror are dicts without classes: a dict with "diss" is taken as a snpgdsDiss result, one with "ibs" as a
    snpgdsIBS result (1 - ibs is clustered); a square array needs sample_id.  Returns dict(sample_id, hclust=dict(merge, height,
    order, labels, method="average"), dendrogram=None[, dist]); R's dendrogram is a plotting object and is not built, `hang` is
    stored only."""
    if isinstance(dist, dict):
        if "diss" in dist:
            sample_id, dist = dist["sample_id"], dist["diss"]
        elif "ibs" in dist:
            sample_id, dist = dist["sample_id"], 1 - np.asarray(dist["ibs"], np.float64)
        else:
            raise TypeError("is.matrix(dist) | inherits(dist, \"snpgdsDissClass\") | inherits(dist, \"snpgdsIBSClass\") is not TRUE")
    dist = np.asarray(dist, np.float64)
    if dist.ndim != 2:
        raise TypeError("is.matrix(dist) | inherits(dist, \"snpgdsDissClass\") | inherits(dist, \"snpgdsIBSClass\") is not TRUE")
    if sample_id is None:
        if dist.shape[0] != dist.shape[1]:
            raise ValueError("nrow(dist) == ncol(dist) is not TRUE")
        raise ValueError("Please specify 'sample.id'.")
    sample_id = np.asarray(sample_id)
    if dist.shape[0] != len(sample_id):
        raise ValueError("nrow(dist) == length(sample.id) is not TRUE")
    if dist.shape[1] != len(sample_id):
        raise ValueError("ncol(dist) == length(sample.id) is not TRUE")
    merge, height, order = _lib.hclust_average(dist)
    rv = dict(sample_id=sample_id, hclust=dict(merge=merge, height=height, order=order, labels=sample_id, method="average"),
              dendrogram=None, hang=hang)
    if need_mat:
        rv["dist"] = dist
    return rv


def _relabel_groups(group, outlier_n):
    """R/AllUtilities.R:485-510: names "G%03d" / "Outlier%03d" (groups of at most outlier_n members), sorted as a factor's levels
    are, renamed in that order to G001 ..., Outlier001 ...; without outlier detection when outlier_n is not finite"""
    group = np.asarray(group)
    vals, counts = np.unique(group, return_counts=True)
    if math.isfinite(outlier_n):
        small = vals[counts <= outlier_n]
        flag = np.isin(group, small)
        names = np.array([("Outlier%03d" if f else "G%03d") % g for g, f in zip(group, flag)], dtype=object)
        n_o = len(small)
        n_g = len(vals) - n_o
        new = ["G%03d" % k for k in range(1, n_g + 1)] + ["Outlier%03d" % k for k in range(1, n_o + 1)]
    else:
        names = np.array(["G%03d" % g for g in group], dtype=object)
        new = ["G%03d" % k for k in range(1, len(vals) + 1)]
    levels = sorted(set(names.tolist()))
    ren = dict(zip(levels, new))
    return np.array([ren[s] for s in names], dtype=object)


def _group_dmat(dist, samp_group, levels):
    k = len(levels)
    dmat = np.zeros((k, k), np.float64)
    sel = [samp_group == g for g in levels]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i in range(k):
            m = dist[np.ix_(sel[i], sel[i])]
            dmat[i, i] = np.nanmean(m[~np.eye(m.shape[0], dtype=bool)]) if m.shape[0] > 1 else np.nan
            for j in range(i + 1, k):
                dmat[i, j] = dmat[j, i] = np.nanmean(dist[np.ix_(sel[i], sel[j])])
    return dmat


def snpgdsCutTree(hc, z_threshold=15, outlier_n=5, n_perm=5000, samp_group=None, col_outlier="red", col_list=None, pch_outlier=4,
                  pch_list=None, label_H=False, label_Z=True, verbose=True, device=0, seed=None):
    """Groups of individuals from the tree of snpgdsHCluster by a permutation test of every merge (R/AllUtilities.R:432-623 ->
    gnrDistPerm, src/SNPRelate.cpp:502-677, here snpgpu_dist_perm on the device).

    R's checks come first and in R's order.  With samp_group given no permutation runs (merge and clust_count are None).  The
    random stream is counter-based and keyed by `seed` (None: a fresh seed from numpy.random.default_rng()), so a result is a
    function of (dist, merge, n_perm, seed).  The plotting arguments are accepted and stored only; R's dendrogram is not built.
    Returns dict(sample_id, z_threshold, outlier_n, samp_order, samp_group, dmat, dendrogram=None, merge=dict(z, n1, n2),
    clust_count); samp_group is an array of level names, `levels` their sorted list (the row / column names of dmat), clust_count a
    list of (name, count) in order of first appearance along samp_order."""
    if not (isinstance(hc, dict) and "hclust" in hc and "sample_id" in hc):
        raise TypeError("inherits(hc, \"snpgdsHCClass\") is not TRUE")
    if not (_is_number(z_threshold) and math.isfinite(z_threshold)):
        raise ValueError("is.finite(z.threshold) is not TRUE")
    if not _is_number(n_perm):
        raise ValueError("is.numeric(n.perm) is not TRUE")
    for name, v in (("label.H", label_H), ("label.Z", label_Z), ("verbose", verbose)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    if not n_perm >= 50:
        raise ValueError("n.perm >= 50 is not TRUE")
    if hc.get("dist") is None:
        raise ValueError("`hc' should have a matrix of dissimilarity.")
    auto = samp_group is None
    if verbose and auto:
        _cat(True, "Determine groups by permutation (Z threshold: %g, outlier threshold: %s):" %
             (z_threshold, "%d" % outlier_n if math.isfinite(outlier_n) else str(outlier_n)))
    dist = np.ascontiguousarray(hc["dist"], np.float64)
    sample_id = hc["sample_id"]
    order = np.asarray(hc["hclust"]["order"])
    ans = dict(sample_id=sample_id, z_threshold=z_threshold, outlier_n=outlier_n, samp_order=order)
    if not auto:
        samp_group = np.asarray(samp_group, dtype=object)
        if len(samp_group) != len(sample_id):
            raise ValueError("length(samp.group) == length(hc$sample.id) is not TRUE")
        merge = None
    else:
        if hc["hclust"].get("merge") is None:
            raise ValueError("!is.null(hc$hclust$merge) is not TRUE")
        if seed is None:
            seed = int(np.random.default_rng().integers(0, 2 ** 63))
        rv = _lib.dist_perm(dist, hc["hclust"]["merge"], n_perm=int(n_perm), z_threshold=float(z_threshold), seed=seed, device=device)
        merge = dict(z=rv["z"], n1=rv["n1"], n2=rv["n2"])
        samp_group = _relabel_groups(rv["group"], outlier_n)
        ans["seed"] = seed
    levels = sorted(set(samp_group.tolist()))
    ans["samp_group"] = samp_group
    ans["levels"] = levels
    ans["dmat"] = _group_dmat(dist, samp_group, levels)
    ans["dendrogram"] = None
    ans["plot"] = dict(col_outlier=col_outlier, col_list=col_list, pch_outlier=pch_outlier, pch_list=pch_list, label_H=label_H,
                       label_Z=label_Z)
    ans["merge"] = merge
    if merge is not None:
        cluster = samp_group[order - 1].tolist()
        seen = list(dict.fromkeys(cluster))
        ans["clust_count"] = [(c, cluster.count(c)) for c in seen]
    else:
        ans["clust_count"] = None
    if verbose:
        _cat(True, "Create %d groups." % len(levels))
    return ans


# ---- data sets put together ---------------------------------------------------------------------------------------------------------
def snpgdsSNPList(gdsobj, sample_id=None, device=0):
    """snpgdsSNPList (R/AllUtilities.R:637-658): snp_id, chromosome, position, allele and afreq (the allele frequency of
    snpgdsSNPRateFreq over the selected samples) of every SNP, as the object snpgdsSNPListIntersect takes."""
    if not isinstance(gdsobj, (GenoFile, _gds.GenoStream)):
        raise TypeError("'gdsobj' should be a SNP GDS object (snpgdsOpen / GenoFile)")
    return _merge.snp_list(gdsobj, snpgdsSNPRateFreq(gdsobj, sample_id=sample_id, device=device)["AlleleFreq"])


def snpgdsSNPListIntersect(snplist1, snplist2, *more, method="position", na_rm=True, same_strand=False, verbose=True):
    """snpgdsSNPListIntersect (R/AllUtilities.R:667-736): the SNPs all lists share -- by chromosome:position, or for "exact" by
    snp.id:chromosome:position:allele -- in the order of list 1, duplicates dropped: dict idx1, idx2, ... (0-based positions, the
    first occurrence in each list) and, for "position", flag2, ... per further list (int32; bit 1 = the list counts the other
    allele, bit 2 = other strand, bit 4 = strand decided by the allele frequencies, NA = mismatched allele names, as
    gnrAlleleStrand).  na_rm drops the SNPs with an NA flag.  Host work: strings and a hash join."""
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    return _merge.snp_list_intersect([snplist1, snplist2] + list(more), method=method, na_rm=na_rm, same_strand=same_strand)


def snpgdsCombineGeno(gds, method="position", same_strand=False, verbose=True, device=0):
    """snpgdsCombineGeno (R/AllUtilities.R:1285-1583).  gds: at least two SNP GDS objects (GenoFile, GenoStream, BedStream, what
    snpgdsOpenVCF / snpgdsOpenPED return) or file names for snpgdsOpen.  With samples common to all files their SNPs are
    concatenated over those samples; without, the samples are concatenated over the SNPs snpgdsSNPListIntersect finds, mapped to
    file 1, every other file's rows re-coded where it counts the other allele.  The genotypes are placed by snpgpu_geno_merge on the
    device, two bits each.  Returns an in-memory GenoFile: this package does not write the GDS container (that is gdsfmt's work),
    so out.fn, compress.* and snpfirstdim have no counterpart -- snpgdsGDS2BED / snpgdsGDS2PED give a file.  No CPU fallback."""
    if isinstance(gds, (str, GenoFile, _gds.GenoStream)) or len(gds) < 2:
        raise ValueError("length(gds.fn) >= 2L is not TRUE")
    method = _match_arg(method, ("position", "exact"), "method")
    for v, name in ((same_strand, "same.strand"), (verbose, "verbose")):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("is.logical(%s) is not TRUE" % name)
    _merge.need_device("snpgdsCombineGeno")
    _cat(verbose, "Merge SNP GDS files:")
    files, lists = [], []
    for g in gds:
        if isinstance(g, str):
            _cat(verbose, "    open '", g, "' ...")
            g = snpgdsOpen(g)
        elif not isinstance(g, (GenoFile, _gds.GenoStream)):
            raise TypeError("'gds' should hold SNP GDS objects or file names")
        files.append(g)
        lists.append(snpgdsSNPList(g, device=device))
        _cat(verbose, "        %d samples, %d SNPs" % (g.n_samp, g.n_snp))
    samp_id = list(dict.fromkeys(files[0].sample_id.tolist()))
    for f in files[1:]:
        have = set(f.sample_id.tolist())
        samp_id = [s for s in samp_id if s in have]
    if samp_id:
        _cat(verbose, "Concatenating SNPs ...")
        out = _merge.combine_common_samples(files, samp_id, device)
    else:
        _cat(verbose, "Concatenating samples (mapping to the first GDS file) ...")
        snp = _merge.snp_list_intersect(lists, method=method, same_strand=same_strand)
        if len(snp["idx1"]) <= 0:
            raise ValueError("There is no common SNP.")
        if verbose:
            n = len(snp["idx1"])
            print("    reference: %d SNPs (%.1f%%)" % (n, 100.0 * n / files[0].n_snp))
            for i in range(2, len(files) + 1):
                if "flag%d" % i in snp:
                    _merge.print_flags(i, snp["flag%d" % i])
        out = _merge.combine_common_snps(files, lists, snp, device)
    _cat(verbose, "    %d samples, %d SNPs" % (out.n_samp, out.n_snp))
    _cat(verbose, "Done.")
    return out


def snpgdsAlleleSwitch(gdsobj, A_allele, verbose=True, device=0):
    """snpgdsAlleleSwitch (R/AllUtilities.R:1686-1751 -> gnrStrandSwitch, src/SNPRelate.cpp:386-499): where B of a SNP's "A/B" is
    A_allele[i] the alleles become "B/A" and the SNP's genotypes 2 - g (on the device: snpgpu_geno_merge with one part).  The
    object is modified in place, so it has to be an in-memory one (GenoFile); one that streams a file is refused as a read-only GDS
    file is.  Returns the flags: int32 0 = unchanged, 1 = switched, NA (-2^31) = A_allele[i] is neither allele, or None."""
    return _merge.allele_switch(gdsobj, A_allele, verbose=verbose, device=device)


def _mds_host_matrix(d, k, sample_id):
    """the refusals of snpgdsMDS that a host matrix allows without the device; returns the matrix as float64"""
    d = np.asarray(d)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("distances must be result of 'dist' or a square matrix")
    d = np.asarray(d, np.float64)
    _mds_check_dims(d.shape[0], k, sample_id)
    if not np.isfinite(d).all():
        raise ValueError("NA values not allowed in 'd'")
    return d


def _mds_check_dims(n, k, sample_id):
    if n < 2:
        raise ValueError("'d' must have at least two rows")
    if k > n - 1:
        raise ValueError("'k' must be in {1, 2, ..  n - 1}")
    if sample_id is not None and len(sample_id) != n:
        raise ValueError("nrow(dist) == length(sample.id) is not TRUE")


def snpgdsMDS(obj, k=2, method="ibs", sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
              maf=float("nan"), missing_rate=0.01, num_thread=1, verbose=True, device=0):
    """Classical multidimensional scaling of IBS or dissimilarity distances -- the tutorial's cmdscale(1 - ibs$ibs, k) -- on the
    GPU (snpgpu_mds / snpgpu_gnrMDS; no reference counterpart: the reference leaves the step to R's cmdscale).

    obj: a dict with "diss" (a snpgdsDiss result) or "ibs" (a snpgdsIBS result: 1 - ibs is scaled, as snpgdsHCluster takes it); a
    square array or a torch tensor on a GPU (a bare distance matrix, `sample_id` its labels); or a SNP GDS object, filtered like
    snpgdsIBS, whose `method` distances ("ibs": 1 - IBS, "diss": snpgdsDiss) are made and scaled on the device without reaching the
    host.  Returns dict(sample_id, points [n][k1], eigenval [k], GOF, trace, n_pos = k1, route): points[:, i] = v_i sqrt(lambda_i)
    for the k1 of the k algebraically largest eigenvalues of B = -1/2 J (D o D) J that are positive (above the rounding of an exact
    zero, include/snpgpu.h 1q); in every eigenvector the entry of largest magnitude is positive.  GOF: cmdscale's two figures,
    sum(eigenval) / sum(|lambda|) and sum(eigenval) / sum(max(lambda, 0)), where all eigenvalues are known (route 0, the dense
    solver), else None.  Not taken: cmdscale's add = TRUE, a packed triangle."""
    if method not in ("ibs", "diss"):
        raise ValueError("'method' should be one of \"ibs\", \"diss\"")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("'k' must be in {1, 2, ..  n - 1}")
    k = int(k)
    is_tensor = not isinstance(obj, (dict, np.ndarray, list, tuple)) and hasattr(obj, "data_ptr") and hasattr(obj, "is_cuda")
    if isinstance(obj, (GenoFile, _gds.GenoStream)):
        ws = _init_file2("Multidimensional scaling of %s distances:" % ("IBS" if method == "ibs" else "dissimilarity"), obj, sample_id,
                         snp_id, autosome_only, remove_monosnp, maf, missing_rate, num_thread, verbose, device)
        _mds_check_dims(ws["n_samp"], k, None)
        sample_id = ws["sample_id"]
        r = _lib.gnr_mds(0 if method == "ibs" else 1, k, ws["n_samp"])
    elif is_tensor:
        if obj.dim() != 2 or obj.shape[0] != obj.shape[1]:
            raise ValueError("distances must be result of 'dist' or a square matrix")
        _mds_check_dims(int(obj.shape[0]), k, sample_id)
        r = _lib.mds(obj, k, device=device)
    else:
        if isinstance(obj, dict):
            if "diss" in obj:
                sample_id, d = obj["sample_id"], obj["diss"]
            elif "ibs" in obj:
                sample_id, d = obj["sample_id"], 1 - np.asarray(obj["ibs"], np.float64)
            else:
                raise TypeError("'obj' should be a snpgdsDiss or snpgdsIBS result, a square matrix or a SNP GDS object")
        else:
            d = obj
        r = _lib.mds(_mds_host_matrix(d, k, sample_id), k, device=device)
    w, v = r["eigval"], r["vectors"]
    k1 = int(np.count_nonzero(w > r["pos_tol"]))
    if k1 < k:
        warnings.warn("only %d of the first %d eigenvalues are > 0" % (k1, k))
    points = np.ascontiguousarray((v[:k1] * np.sqrt(w[:k1])[:, None]).T)
    gof = None
    if r["all_eigval"] is not None:
        a = r["all_eigval"]
        gof = np.array([w.sum() / np.abs(a).sum(), w.sum() / np.maximum(a, 0).sum()])
    return dict(sample_id=None if sample_id is None else np.asarray(sample_id), points=points, eigenval=w, GOF=gof, trace=r["trace"],
                n_pos=k1, route=r["route"])


def _pcr_match(ws, pcs, n_pcs, training_id, verbose):
    """(ids, pcs as [n][n_pcs] float64, training flags or None) of the PC-Relate calls: `pcs` and `training_id` matched to the working
    samples"""
    n = ws["n_samp"]
    ids = np.asarray(ws["sample_id"])
    if isinstance(pcs, dict):
        if "eigenvect" not in pcs or "sample_id" not in pcs or pcs["eigenvect"] is None:
            raise TypeError("'pcs' should be a snpgdsPCA / snpgdsEIGMIX result or an array with one row per sample")
        pid = np.asarray(pcs["sample_id"])
        order = np.argsort(pid, kind="stable")
        pos = np.searchsorted(pid[order], ids)
        pos[pos >= len(pid)] = 0
        if len(pid) == 0 or not np.array_equal(pid[order][pos], ids):
            raise ValueError("Some of the selected samples are not in 'pcs$sample.id'.")
        mat = np.asarray(pcs["eigenvect"], np.float64)[order[pos]]
    else:
        mat = np.asarray(pcs, np.float64)
        if mat.ndim == 1:
            mat = mat.reshape(n, -1) if mat.size else mat.reshape(n, 0)
        if mat.ndim != 2 or mat.shape[0] != n:
            raise ValueError("'pcs' should have one row per selected sample (%d)" % n)
    if n_pcs is not None:
        if isinstance(n_pcs, bool) or not isinstance(n_pcs, (int, np.integer)) or n_pcs < 0 or n_pcs > mat.shape[1]:
            raise ValueError("'n_pcs' should be in 0 .. %d" % mat.shape[1])
        mat = mat[:, :int(n_pcs)]
    mat = np.ascontiguousarray(mat)
    train = None
    if training_id is not None:
        want = np.asarray(training_id)
        train = np.isin(ids, want)
        if int(train.sum()) != len(np.unique(want)):
            raise ValueError("Some of training.id do not exist!")
    _cat(verbose, "    # of principal components: %d\n    # of training samples: %d" % (mat.shape[1], n if train is None else int(train.sum())))
    return ids, mat, train


def snpgdsPCRelate(gdsobj, pcs, n_pcs=None, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                   maf=float("nan"), missing_rate=float("nan"), training_id=None, maf_thresh=0.01, ibd_probs=True, verbose=True,
                   device=0):
    """Ancestry-adjusted relatedness by PC-Relate (Conomos, Reiner, Weir, Thornton, AJHG 2016) on the GPU (snpgpu_gnrPCRelate,
    include/snpgpu.h section 1r; no reference counterpart, and agreement with another package's output is not tested: the
    definitions of DESIGN.md 31 are the specification).  Every SNP is regressed on the leading principal components over the
    training samples; kinship, k0, k2 and inbreeding come from the residuals under individual-specific allele frequencies.

    pcs: a snpgdsPCA / snpgdsEIGMIX result (its rows are matched to the selected samples by sample_id and the first n_pcs columns
    of eigenvect are used; all of them by default) or an array with one row per selected sample, in their order (n_pcs columns of
    it; an array without columns, or n_pcs = 0, adjusts for nothing but the mean).  training_id: the samples the regression is
    fitted on (unrelated ones, as a rule), all by default.  maf_thresh: an (individual, SNP) whose individual-specific frequency
    lies outside [maf_thresh, 1 - maf_thresh] is left out.  ibd_probs=False accumulates the kinship planes only (3 of 8).
    Returns dict(sample_id, snp_id, kinship, k0, k1, k2, nsnp, inbreed): n x n matrices and inbreed [n]; k0 / k1 / k2 are None
    without ibd_probs.  The diagonal of kinship is (1 + inbreed) / 2, that of k0 / k1 / k2 carries no meaning.
    snpgdsIBDSelection(result, kinship_cutoff) tabulates it like any IBD object."""
    ws = _init_file2("PC-Relate: kinship adjusted for principal components:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp,
                     maf, missing_rate, 1, verbose, device)
    ids, mat, train = _pcr_match(ws, pcs, n_pcs, training_id, verbose)
    n = ws["n_samp"]
    r = _lib.gnr_pcrelate(n, mat if mat.shape[1] else None, train, maf_thresh=maf_thresh, ibd=bool(ibd_probs))
    k0, k2 = r.get("k0"), r.get("k2")
    return dict(sample_id=ids, snp_id=ws["snp_id"], kinship=r["kinship"], k0=k0, k1=None if k0 is None else 1.0 - k0 - k2, k2=k2,
                nsnp=r["nsnp"], inbreed=r["inbreed"])


def snpgdsPCRelatePairs(gdsobj, pcs, n_pcs=None, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                        maf=float("nan"), missing_rate=float("nan"), training_id=None, maf_thresh=0.01, ibd_probs=True,
                        kinship_cutoff=2 ** -5.5, samp_sel=None, panel_rows=None, verbose=True, device=0):
    """The related pairs of a PC-Relate run without its n x n matrices (snpgpu_gnrPCRelatePairs, include/snpgpu.h section 1r;
    DESIGN.md 31a).  The result equals snpgdsIBDSelection(snpgdsPCRelate(gdsobj, pcs, ...), kinship_cutoff, samp_sel) column for
    column and bit for bit: the sums are accumulated on the GPU one row panel at a time and only the selected pairs come back, so
    device memory is that of one panel and host memory is proportional to the number of pairs.

    pcs, n_pcs, training_id, maf_thresh, ibd_probs and the SNP / sample filters: as snpgdsPCRelate.  kinship_cutoff: pairs with
    kinship >= it are kept (the default 2^-5.5 is the lower edge of third-degree relatives; a non-finite cutoff keeps every pair).
    samp_sel: a logical vector over the working samples or strictly increasing 0-based indices, as for snpgdsIBDPairs.  panel_rows:
    rows of one panel -- a multiple of 128, or at least the number of samples for a single panel; None: as many as the device holds.
    The pairs found never depend on it.
    Returns dict(sample_id, snp_id, ID1, ID2, idx1, idx2, kinship, k0, k1, k2, nsnp, inbreed, n_panels): one entry per pair in the
    order of snpgdsIBDSelection (ID1 = sample_id[idx1] ascending, then ID2 = sample_id[idx2]), inbreed [n] for all samples; k0 / k1 /
    k2 are None without ibd_probs."""
    if isinstance(kinship_cutoff, (bool, np.bool_)) or not isinstance(kinship_cutoff, (int, float, np.integer, np.floating)):
        raise TypeError("is.numeric(kinship.cutoff) is not TRUE")
    if panel_rows is not None and (isinstance(panel_rows, bool) or not isinstance(panel_rows, (int, np.integer)) or panel_rows < 1):
        raise ValueError("'panel_rows' should be None or a positive multiple of %d" % _lib.PCR_TILE)
    ws = _init_file2("PC-Relate: kinship adjusted for principal components, related pairs only:", gdsobj, sample_id, snp_id, autosome_only,
                     remove_monosnp, maf, missing_rate, 1, verbose, device)
    ids, mat, train = _pcr_match(ws, pcs, n_pcs, training_id, verbose)
    n = ws["n_samp"]
    mask = _pairs_samp_sel("snpgdsPCRelatePairs", samp_sel, n, "snpgdsPCRelate")
    r = _lib.gnr_pcrelate_pairs(n, mat if mat.shape[1] else None, train, maf_thresh=maf_thresh, ibd=bool(ibd_probs),
                                panel_rows=0 if panel_rows is None else int(panel_rows), kinship_cutoff=float(kinship_cutoff),
                                samp_sel=mask, verbose=False)
    k0, k2 = r.get("k0"), r.get("k2")
    m = len(r["idx1"])
    _cat(verbose, "%d pair%s selected in %d panel%s" % (m, "" if m == 1 else "s", r["n_panels"], "" if r["n_panels"] == 1 else "s"))
    return dict(sample_id=ids, snp_id=ws["snp_id"], ID1=ids[r["idx1"]], ID2=ids[r["idx2"]], idx1=r["idx1"], idx2=r["idx2"],
                kinship=r["kinship"], k0=k0, k1=None if k0 is None else 1.0 - k0 - k2, k2=k2, nsnp=r["nsnp"], inbreed=r["inbreed"],
                n_panels=r["n_panels"])


def _admix_groups(groups, sample_id, what):
    """`groups` of snpgdsAdmixProp / snpgdsAdmix: an ordered dict name -> sample ids.  Returns (names, one index array into sample_id
    per group -- match(): the first occurrence -- and whether any id is in more than one group); an unknown id raises with the
    reference's message."""
    if not isinstance(groups, dict):
        raise TypeError("is.list(groups) is not TRUE")
    if len(groups) <= 1:
        raise TypeError("length(groups) > 1 is not TRUE")
    where = {}
    for i, s in enumerate(list(np.asarray(sample_id))):
        where.setdefault(s, i)
    index, seen, overlap = [], set(), False
    for i, (name, ids) in enumerate(groups.items()):
        if isinstance(ids, (str, bytes, dict)) or not hasattr(ids, "__len__"):
            raise ValueError("`groups' should be a list of sample IDs with respect to multiple groups.")
        ids = list(np.asarray(ids).ravel()) if len(ids) else []
        if any(s not in where for s in ids):
            raise ValueError("`groups[[%d]]' includes sample(s) not existing in `%s'." % (i + 1, what))
        if any(s in seen for s in ids):
            overlap = True
        seen.update(ids)
        index.append(np.array([where[s] for s in ids], np.int64))
    return list(groups.keys()), index, overlap


def snpgdsAdmixProp(eigobj, groups, bound=False):
    """Admixture proportions from an eigen-analysis (R/PCA.R:347-425; Zheng & Weir 2016): with G groups of reference samples, the
    first G - 1 eigenvectors are mapped linearly so that the mean of group g over its own samples is the unit vector e_g.
    eigobj: a snpgdsPCA / snpgdsEIGMIX result (sample_id, eigenvect [n][k]); groups: an ordered dict name -> sample ids, 2 ... k + 1
    groups (overlapping groups warn); bound=True clips to [0, 1] and renormalises the rows.  Returns dict(sample_id, groups, prop
    [n][G]) -- the reference's matrix with its dimnames.  Computed on the host, as in the reference."""
    if not isinstance(eigobj, dict) or eigobj.get("sample_id") is None:
        raise TypeError("'eigobj' should be a snpgdsPCA / snpgdsEIGMIX result with 'sample_id' and 'eigenvect'")
    vect = eigobj.get("eigenvect")
    if vect is None or np.ndim(vect) != 2:
        raise TypeError("is.matrix(eigobj$eigenvect) is not TRUE")
    vect = np.asarray(vect, np.float64)
    if not isinstance(groups, dict):
        raise TypeError("is.list(groups) is not TRUE")
    if len(groups) <= 1:
        raise TypeError("length(groups) > 1 is not TRUE")
    if len(groups) > vect.shape[1] + 1:
        raise ValueError("`eigobj' should have more eigenvectors than what is specified in `groups'.")
    names, index, overlap = _admix_groups(groups, eigobj["sample_id"], "eigobj$sample.id")
    if overlap:
        warnings.warn("There are some overlapping between group sample IDs.")
    if not isinstance(bound, (bool, np.bool_)):
        raise TypeError("is.logical(bound) is not TRUE")
    G = len(names)
    E = vect[:, :G - 1]
    mat = np.array([E[k].mean(axis=0) if len(k) else np.full(G - 1, np.nan) for k in index]).reshape(G, G - 1)
    if np.isnan(mat).any():
        raise ValueError("The eigenvectors should not have missing value!")
    t_p = mat[G - 1]
    t_r = np.linalg.inv(mat[:G - 1] - t_p[None, :])
    new_p = (E - t_p[None, :]) @ t_r
    new_p = np.column_stack([new_p, 1.0 - new_p.sum(axis=1)])
    if bound:
        new_p[new_p < 0] = 0.0
        new_p[new_p > 1] = 1.0
        new_p = new_p / new_p.sum(axis=1, keepdims=True)
    return dict(sample_id=np.asarray(eigobj["sample_id"]), groups=names, prop=new_p)


def snpgdsAdmixTable(propmat, group, sort=False):
    """Summary of admixture proportions by group (R/PCA.R:525-556).  propmat: a snpgdsAdmixProp / snpgdsAdmix result or a numeric
    [n][G] matrix; group: one label per row (None / NaN = NA: in no group).  Returns a dict with one entry per proportion column (its
    group name, or its index for a plain matrix): the reference's data frame as dict(group, num, mean, sd, min, max), one row per
    level of factor(group) -- the sorted labels -- with NaN proportions ignored (na.rm: a group whose proportions are all NaN keeps its
    row, with a NaN mean) and sd in its n - 1 form.  sort=True orders the rows by decreasing mean."""
    names = None
    if isinstance(propmat, dict):
        names = list(propmat["groups"])
        propmat = propmat["prop"]
    p = np.asarray(propmat)
    if p.ndim != 2 or p.dtype.kind not in "fiu":
        raise TypeError("is.numeric(propmat), is.matrix(propmat) are not all TRUE")
    p = p.astype(np.float64)
    if group is None or isinstance(group, (str, bytes)) or not hasattr(group, "__len__") or len(group) != p.shape[0]:
        raise TypeError("is.vector(group) | is.factor(group), nrow(propmat) == length(group) are not all TRUE")
    if not isinstance(sort, (bool, np.bool_)):
        raise TypeError("is.logical(sort) is not TRUE")
    labels = list(group)
    na = [lab is None or (isinstance(lab, (float, np.floating)) and math.isnan(lab)) for lab in labels]
    levels = sorted(set(lab for lab, m in zip(labels, na) if not m))
    if names is None:
        names = list(range(p.shape[1]))
    ans = {}
    for c, name in enumerate(names):
        rows = []
        for grp in levels:
            x = np.array([(not m) and lab == grp for lab, m in zip(labels, na)], bool)
            if not x.any():
                continue
            y = p[x, c]
            y = y[~np.isnan(y)]
            rows.append((grp, int(x.sum()), float(y.mean()) if y.size else float("nan"),
                         float(y.std(ddof=1)) if y.size > 1 else float("nan"),
                         float(y.min()) if y.size else float("inf"), float(y.max()) if y.size else float("-inf")))
        if sort:
            # order(mean, decreasing=TRUE): stable, NA last
            rows = [rows[i] for i in sorted(range(len(rows)), key=lambda i: (math.isnan(rows[i][2]), -rows[i][2] if not math.isnan(rows[i][2]) else 0.0))]
        ans[name] = dict(group=[r[0] for r in rows], num=np.array([r[1] for r in rows], np.int64),
                         mean=np.array([r[2] for r in rows], np.float64), sd=np.array([r[3] for r in rows], np.float64),
                         min=np.array([r[4] for r in rows], np.float64), max=np.array([r[5] for r in rows], np.float64))
    return ans


def admix_seeded_start(n_samp, k, p, seed, f_min):
    """The seeded start of snpgdsAdmix without groups, so that it can be restated: with numpy.random.Generator(numpy.random.Philox(seed)),
    first Q = n_samp x k uniforms on [0.5, 1.5) with normalised rows, then F = clamp(p_j + 0.2 (U - 0.5), f_min, 1 - f_min) with U
    len(p) x k uniforms on [0, 1) and p the all-sample frequencies."""
    rng = np.random.Generator(np.random.Philox(int(seed)))
    q = 0.5 + rng.random((int(n_samp), int(k)))
    q = q / q.sum(axis=1, keepdims=True)
    p = np.asarray(p, np.float64)
    f = np.clip(p[:, None] + 0.2 * (rng.random((len(p), int(k))) - 0.5), f_min, 1.0 - f_min)
    return q, f


def _admix_pop_freq(ws, pop, n_pop, device):
    """(f [m][n_pop], p [m]): allele frequencies sum g / (2 called) of the working space's SNPs per population of `pop` (exact counters
    of snpgpu_pop_counts) and over all samples; a SNP without a called sample in a population takes p_j there, or 0.5 without any"""
    acnt, cnt = _lib.pop_counts(ws["packed"], ws["n_samp"], pop, n_pop, fmt=_lib.GENO_PACKED2, device=device)
    a_all, c_all = acnt.sum(axis=1, dtype=np.int64), cnt.sum(axis=1, dtype=np.int64)
    p = np.where(c_all > 0, a_all / np.maximum(c_all, 1), 0.5)
    f = np.where(cnt > 0, acnt / np.maximum(cnt, 1), p[:, None])
    return f, p


def snpgdsAdmix(gdsobj, k=None, groups=None, supervised=False, sample_id=None, snp_id=None, autosome_only=True, remove_monosnp=True,
                maf=float("nan"), missing_rate=float("nan"), q_start=None, f_start=None, seed=1, max_iter=500, tol=1e-4, f_min=1e-6,
                with_afreq=True, verbose=True, device=0):
    """Ancestry proportions by maximum likelihood on the GPU (snpgpu_gnrAdmix, include/snpgpu.h section 1s; no reference
    counterpart, and agreement with another package's output is not tested: the definitions of DESIGN.md 32 are the specification).
    The model is that of FRAPPE (Tang et al. 2005) and ADMIXTURE: g_ij ~ Binomial(2, sum_k q_ik f_kj) over the called genotypes,
    fitted by EM in fp64 -- one pass over all genotypes per iteration, Q and F both updated from the old state.

    groups: an ordered dict name -> sample ids as for snpgdsAdmixProp, but overlapping groups are refused; k defaults to (and must
    equal) the number of groups.  F then starts from the groups' allele frequencies (exact counters; a SNP no sample of the group was
    called at takes the all-sample frequency, or 0.5) and Q at 1 / k; column c belongs to group c.  supervised=True (needs groups)
    holds F fixed: every sample is projected onto the groups' frequencies.  Without groups, k is required and the start is seeded on
    the host (admix_seeded_start: numpy.random.Philox(seed); Q rows normalised uniforms on [0.5, 1.5), F = clamp(p_j + 0.2 (U - 0.5))).
    q_start [n][k] / f_start [m][k] override either start, e.g. q_start=snpgdsAdmixProp(eig, groups, bound=True)["prop"] (in the
    order of the selected samples).  The EM stops when an iteration raises the log-likelihood by less than tol, or after max_iter.
    Returns dict(sample_id, snp_id, groups, prop [n][k], afreq [m][k] (None without with_afreq), loglik (the trace: one entry per
    iteration made, plus the likelihood of the returned state), niter, converged).

    The column labels of an unsupervised run are arbitrary (any permutation of the populations has the same likelihood).  Plain EM is
    slow to converge: hundreds of iterations are usual, and a small tol stops on slow progress rather than at the optimum.  Not
    built: acceleration (SQUAREM, quasi-Newton), cross-validation for the choice of k, multi-device objects, results in device
    memory, anything below fp64."""
    if not isinstance(supervised, (bool, np.bool_)):
        raise TypeError("is.logical(supervised) is not TRUE")
    if groups is None and supervised:
        raise ValueError("'supervised=True' needs 'groups'.")
    if groups is None and k is None:
        raise ValueError("'k' is required without 'groups'.")
    if groups is not None and (not isinstance(groups, dict) or len(groups) < 2):
        raise ValueError("'groups' should be a dict of at least two groups of sample IDs.")
    if k is None:
        k = len(groups)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 2 or k > 32:
        raise ValueError("'k' should be an integer in 2 .. 32")
    k = int(k)
    if groups is not None and k != len(groups):
        raise ValueError("'k' should be the number of groups (%d)" % len(groups))
    if not (isinstance(f_min, (int, float, np.integer, np.floating)) and 0.0 < f_min < 0.5):
        raise ValueError("'f_min' should be inside (0, 0.5)")
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError("'max_iter' should be a non-negative integer")
    if not isinstance(tol, (int, float, np.integer, np.floating)) or math.isnan(tol):
        raise ValueError("'tol' should be a number")
    ws = _init_file2("Ancestry proportions by EM:", gdsobj, sample_id, snp_id, autosome_only, remove_monosnp, maf, missing_rate, 1,
                     verbose, device)
    n, m = ws["n_samp"], ws["n_snp"]
    ids = np.asarray(ws["sample_id"])
    if m < 1:
        raise ValueError("No SNP in the working dataset.")
    names = None
    q0 = f0 = None
    if groups is not None:
        names, index, overlap = _admix_groups(groups, ids, "the selected samples")
        if overlap:
            raise ValueError("There are some overlapping between group sample IDs.")
        if any(len(ix) == 0 for ix in index):
            raise ValueError("Each group should have at least one sample.")
        pop = np.full(n, k, np.int32)                       # the rest: samples in no group
        for g, ix in enumerate(index):
            pop[ix] = g
        if f_start is None:
            f0 = _admix_pop_freq(ws, pop, k + 1 if (pop == k).any() else k, device)[0][:, :k]
        if q_start is None:
            q0 = np.full((n, k), 1.0 / k)
    elif f_start is None or q_start is None:
        # the all-sample frequencies sum g / (2 called) of the working space's SNPs, from its exact per-SNP counters; none called: 0.5
        p = np.empty(m, np.float64)
        _lib.check(_lib.lib().snpgpu_ws_snp_rate_freq(_lib._ptr(p), None, None))
        q0, f0 = admix_seeded_start(n, k, np.where(np.isnan(p), 0.5, p), seed, f_min)
    if q_start is not None:
        q0 = np.ascontiguousarray(q_start, np.float64)
        if q0.shape != (n, k):
            raise ValueError("'q_start' should be a %d x %d matrix (selected samples x k)" % (n, k))
    if f_start is not None:
        f0 = np.ascontiguousarray(f_start, np.float64)
        if f0.shape != (m, k):
            raise ValueError("'f_start' should be a %d x %d matrix (selected SNPs x k)" % (m, k))
    _cat(verbose, "    # of populations: %d%s\n    max. iterations: %d, tol: %g" % (k, " (supervised)" if supervised else "", max_iter, tol))
    q, f, ll, done = _lib.gnr_admix(n, m, q0, f0, f_min=float(f_min), max_iter=int(max_iter), tol=float(tol), fix_f=bool(supervised))
    converged = bool(done >= 2 and ll[done - 1] - ll[done - 2] < tol)
    _cat(verbose, "%d iteration%s, log-likelihood %.6f%s" % (done, "" if done == 1 else "s", ll[-1], "" if converged else " (not converged)"))
    return dict(sample_id=ids, snp_id=ws["snp_id"], groups=names, prop=q, afreq=f if with_afreq else None, loglik=ll, niter=done,
                converged=converged)
