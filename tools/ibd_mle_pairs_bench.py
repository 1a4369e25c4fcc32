#!/usr/bin/env python
"""snpgpu_ibd_mle_pairs (one wave per pair) on one GPU: one JSON line, printed and written to profiles/ibd_mle_pairs_bench.json.

Device-resident synthetic genotypes (snpgpu_synth_block, spectrum 0: p ~ U(0.05, 0.95), 1 % missing calls), M = 20 000 SNPs.
  (a) N = 279 with all 38 781 pairs listed, beside snpgpu_ibd_mle (one pair per lane) on the same rows in the same run;
  (b) N = 100 000 rows resident, P = 292, 4 096 and 100 000 random pairs -- what the matrix path cannot do at all.
Per case, after one warm-up call, the median of --reps calls: HIP-event time of the EM kernel and of all kernels
(snpgpu_ibd_mle_pairs_stats), wall time of the whole call (outputs to host memory), SNP-iterations per second (wave-sweeps x M / EM
kernel time; the candidate sweep of coeff.correct counts as one sweep), the kernel's fp64 instruction rate as a share of what a
register-only v_fma_f64 stream sustains in the same run (snpgpu_diag_fp64_rate), and the bytes of per-SNP constants a sweep
fetches.  FP64_INSTR_PER_LANE_SNP is a FIXED count, not read from the build: the fp64 VALU instructions per lane and SNP of the EM
sweep's inner loop in the gfx950 code object of csrc/kernels_ibd.hip as committed (84 per 4-SNP step: 37 mul, 32 fma, 8 add, 4 rcp,
the frexp pair of the renormalisation and one conversion).  Recount it with `hipcc --cuda-device-only -S` when the kernel or the
compiler changes.  The share counts the padded SNP slots a sweep really issues (the words are padded to 1 024 SNPs).

--method simplex | jacquard | all runs case (a) only, for the named method(s) of snpgdsIBDMLEPairs ("all": EM, downhill simplex and
Jacquard in one run), and writes profiles/ibd_methods_bench.json: per method the HIP-event time of its one-wave-per-pair kernel,
its wave-sweeps (EM iterations; function-evaluation sweeps of the simplex; the candidate sweep counts as one), SNP-evaluations per
second (wave-sweeps x M / kernel time), the fp64 instruction count per lane-SNP of its sweep loops (FP64_INSTR_METHODS, counted in
the gfx950 code object of csrc/kernels_ibd_methods.hip as committed, fp64 compares included), mean and 99th percentile of niter
(the simplex's niter is its count of function evaluations), and the kernel-time ratios simplex / EM and Jacquard / EM.  The
default --method em is everything above, unchanged."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_INSTR_PER_LANE_SNP = 84 / 4
FP64_INSTR_PER_LANE_SNP_MATRIX = 66 / 4          # tools/ibd_mle_bench.py
# per lane-SNP, from the inner loops of ibd_nm_pairs_kernel (per 8-SNP step: 140 with one point, 196 with two, 246 with three, 404 with
# the six candidates) and ibd_jacq_pairs_kernel (84 per 2-SNP step: 31 mul, 42 fma, 6 add, 2 rcp, the frexp pair, one conversion)
FP64_INSTR_METHODS = dict(em=FP64_INSTR_PER_LANE_SNP, simplex=140 / 8, simplex_2_points=196 / 8, simplex_3_points=246 / 8,
                          simplex_6_candidates=404 / 8, jacquard=84 / 2)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-snp", type=int, default=20000)
    ap.add_argument("--small", type=int, default=279, help="N of case (a)")
    ap.add_argument("--samples", type=int, default=100000, help="N of case (b)")
    ap.add_argument("--pairs", default="292,4096,100000", help="P of case (b)")
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--max-niter", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probe-seconds", type=float, default=2.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--method", default="em", choices=("em", "simplex", "jacquard", "all"),
                    help="em: the cases above (default); another value: case (a) for that method, or for all three")
    ap.add_argument("--out", default=None, help="default: profiles/ibd_mle_pairs_bench.json, or ibd_methods_bench.json with --method")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "ibd_mle_pairs_bench.json" if a.method == "em" else "ibd_methods_bench.json")

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib

    torch.cuda.set_device(a.device)
    M = a.n_snp
    wpad = (M + 1023) // 1024 * 64
    fma_tflops = _lib.diag_fp64_rate(a.probe_seconds, a.device)
    peak_instr = fma_tflops * 1e12 / 2                                    # an FMA is one instruction, two flops
    out = dict(tool="ibd_mle_pairs_bench", source_stamp=bench.source_stamp(), n_snp=M, missing=a.missing, max_niter=a.max_niter,
               reps=a.reps, fma_stream_tflops=round(fma_tflops, 2), fp64_instr_per_lane_snp=FP64_INSTR_PER_LANE_SNP,
               snp_constant_bytes_per_sweep=8 * 16 * wpad + 4 * wpad, snp_constants="p (8 B / SNP, transposed) + usable mask (4 B / word)")

    def synth(N, seed):
        rb = (N + 3) // 4
        geno = torch.empty(M * rb, dtype=torch.uint8, device="cuda")
        step = max(1, min(8192, (1 << 28) // rb))
        for i0 in range(0, M, step):
            _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, min(step, M - i0), seed=seed, missing=a.missing, spectrum=0,
                             device=a.device)
        torch.cuda.synchronize()
        return geno

    def pairs_case(geno, N, i1, i2):
        runs = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            k0, k1, ll, nit, _ = _lib.ibd_mle_pairs(None, N, i1, i2, max_niter=a.max_niter, device=a.device,
                                                    geno_dev_ptr=geno.data_ptr(), n_snp=M)
            wall = time.perf_counter() - t0
            if rep:                                                       # (the first one warms up)
                runs.append((wall,) + _lib.ibd_mle_pairs_stats())
        wall, ms_em, ms_all, sweeps, P = median(runs)
        slots = float(sweeps) * wpad * 16                                 # lane-SNP steps issued
        return dict(n_samp=N, pairs=int(P), distinct_samples=int(len(np.unique(np.concatenate([i1, i2])))),
                    em_kernel_ms=round(ms_em, 3), kernels_ms=round(ms_all, 3), call_ms=round(wall * 1e3, 3), wave_sweeps=int(sweeps),
                    snp_iterations_per_s=float(sweeps) * M / (ms_em * 1e-3), niter_mean=round(float(nit.mean()), 2),
                    niter_frac_at_max=float((nit >= a.max_niter).mean()), nan_pairs=int(np.isnan(k0).sum()),
                    fp64_fraction_of_fma_stream=round(slots * FP64_INSTR_PER_LANE_SNP / (ms_em * 1e-3) / peak_instr, 4)), (k0, k1, nit)

    def method_case(geno, N, i1, i2, method):
        runs = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            if method == "jacquard":
                nit = _lib.ibd_jacquard_pairs(None, N, i1, i2, max_niter=a.max_niter, device=a.device, geno_dev_ptr=geno.data_ptr(),
                                              n_snp=M)[2]
            else:
                nit = _lib.ibd_mle_pairs(None, N, i1, i2, mode=2 if method == "simplex" else 0, max_niter=a.max_niter,
                                         device=a.device, geno_dev_ptr=geno.data_ptr(), n_snp=M)[3]
            wall = time.perf_counter() - t0
            if rep:
                runs.append((wall,) + _lib.ibd_mle_pairs_stats())
        wall, ms_k, ms_all, sweeps, P = median(runs)
        slots = float(sweeps) * wpad * 16
        return dict(n_samp=N, pairs=int(P), kernel_ms=round(ms_k, 3), kernels_ms=round(ms_all, 3), call_ms=round(wall * 1e3, 3),
                    wave_sweeps=int(sweeps), sweeps_per_pair=round(float(sweeps) / P, 2),
                    snp_evaluations_per_s=float(sweeps) * M / (ms_k * 1e-3), fp64_instr_per_lane_snp=FP64_INSTR_METHODS[method],
                    fp64_fraction_of_fma_stream=round(slots * FP64_INSTR_METHODS[method] / (ms_k * 1e-3) / peak_instr, 4),
                    niter_mean=round(float(nit.mean()), 2), niter_p99=float(np.percentile(nit, 99)),
                    niter_frac_at_max=float((nit >= a.max_niter).mean()))

    if a.method != "em":
        N = a.small
        geno = synth(N, 2024)
        i1, i2 = np.triu_indices(N, 1)
        out = dict(tool="ibd_mle_pairs_bench --method " + a.method, source_stamp=out["source_stamp"], n_snp=M, n_samp=N,
                   missing=a.missing, max_niter=a.max_niter, reps=a.reps, fma_stream_tflops=out["fma_stream_tflops"],
                   fp64_instr_per_lane_snp=FP64_INSTR_METHODS, methods={})
        for method in (("em", "simplex", "jacquard") if a.method == "all" else (a.method,)):
            out["methods"][method] = method_case(geno, N, i1, i2, method)
        if a.method == "all":
            em_ms = out["methods"]["em"]["kernel_ms"]
            out["kernel_ms_ratio_simplex_over_em"] = round(out["methods"]["simplex"]["kernel_ms"] / em_ms, 3)
            out["kernel_ms_ratio_jacquard_over_em"] = round(out["methods"]["jacquard"]["kernel_ms"] / em_ms, 3)
        out["fma_stream_tflops_after"] = round(_lib.diag_fp64_rate(a.probe_seconds, a.device), 2)
        line = json.dumps(out)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return

    # (a) every pair of a small N, beside the matrix path
    N = a.small
    geno = synth(N, 2024)
    i1, i2 = np.triu_indices(N, 1)
    res, (k0, k1, nit) = pairs_case(geno, N, i1, i2)
    runs = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        M0, M1, MN, _ = _lib.ibd_mle(None, N, max_niter=a.max_niter, device=a.device, geno_dev_ptr=geno.data_ptr(), n_snp=M)
        wall = time.perf_counter() - t0
        if rep:
            runs.append((wall,) + _lib.ibd_mle_stats())
    wall, ms_em, ms_all, useful, issued = median(runs)
    d = np.maximum(np.abs(k0 - M0[i1, i2]), np.abs(k1 - M1[i1, i2]))
    res["matrix_path"] = dict(em_kernel_ms=round(ms_em, 3), kernels_ms=round(ms_all, 3), call_ms=round(wall * 1e3, 3),
                              lane_occupancy=round(useful / issued, 4), snp_iterations_per_s=float(useful) * M / (ms_em * 1e-3),
                              fp64_fraction_of_fma_stream=round(float(issued) * M * FP64_INSTR_PER_LANE_SNP_MATRIX
                                                                / (ms_em * 1e-3) / peak_instr, 4))
    res["against_matrix_path"] = dict(niter_differs=int((nit != MN[i1, i2]).sum()), max_abs_dk=float(np.nanmax(d)),
                                      em_kernel_speedup=round(ms_em / res["em_kernel_ms"], 3))
    out["all_pairs_small_n"] = res
    del geno

    # (b) a few pairs out of many samples
    N = a.samples
    geno = synth(N, 78)
    rng = np.random.default_rng(1)
    out["listed_pairs_large_n"] = []
    for P in [int(x) for x in a.pairs.split(",")]:
        i1 = rng.integers(0, N, P)
        i2 = (i1 + rng.integers(1, N, P)) % N
        out["listed_pairs_large_n"].append(pairs_case(geno, N, i1, i2)[0])
    out["fma_stream_tflops_after"] = round(_lib.diag_fp64_rate(a.probe_seconds, a.device), 2)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
