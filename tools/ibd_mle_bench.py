#!/usr/bin/env python
"""snpgdsIBDMLE (method "EM") throughput on one GPU: one JSON line.

The genotypes are generated on the device (snpgpu_synth_block, spectrum 0: p ~ U(0.05, 0.95), 1 % missing calls) and handed to
snpgpu_ibd_mle from device memory; the n x n results land in host memory.  Reported: wall time of the call, HIP-event time of the
EM kernel and of all the call's kernels, SNP-iterations per second (pair sweeps x SNPs / EM kernel time), the niter distribution
(mean, p99, fraction at max_niter), lane occupancy (lane-sweeps that advanced a pair / lane-sweeps issued), and the EM kernel's
fp64 instruction rate as a fraction of what a register-only v_fma_f64 stream sustains on this device in the same run
(snpgpu_diag_fp64_rate).  FP64_INSTR_PER_LANE_SNP is a FIXED count, not read from the build: the fp64 VALU instructions per lane
and SNP of ibd_em_kernel's inner loop in the gfx950 code object of csrc/kernels_ibd.hip as committed (66 per 4-SNP step: 24 mul,
32 fma, 4 add, 4 rcp and the frexp pair of the renormalisation; the loop has no SGPR spill code).  Recount it with
`hipcc --cuda-device-only -S` when the kernel or the compiler changes; the fraction is only as current as this number."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_INSTR_PER_LANE_SNP = 66 / 4


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-samp", type=int, default=279)
    ap.add_argument("--n-snp", type=int, default=8039)
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--max-niter", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=1, help="timed runs after one warm-up run; the best is reported (0: one run, reported)")
    ap.add_argument("--probe-seconds", type=float, default=2.0)
    ap.add_argument("--row-panels", type=int, default=1,
                    help="run the matrix as this many calls on row ranges of equal pair counts (the row range of snpgpu_ibd_mle); "
                         "times and counts are summed")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from snprelate_amd import _lib

    N, M = a.n_samp, a.n_snp
    rb = (N + 3) // 4
    torch.cuda.set_device(a.device)
    geno = torch.empty(M * rb, dtype=torch.uint8, device="cuda")
    for i0 in range(0, M, 8192):
        _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, min(8192, M - i0), seed=2024, missing=a.missing, spectrum=0,
                         device=a.device)
    torch.cuda.synchronize()

    # row ranges [r0, r1) with about equal numbers of pairs (row r holds N - 1 - r of them)
    per_row = np.arange(N - 1, -1, -1, dtype=np.float64)
    cum = np.concatenate([[0], np.cumsum(per_row)])
    cuts = sorted(set([0, N] + [int(np.searchsorted(cum, cum[-1] * k / a.row_panels)) for k in range(1, a.row_panels)]))

    def run():
        out = (np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N), np.int32))
        stats = np.zeros(4)
        t0 = time.perf_counter()
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            _lib.ibd_mle(None, N, max_niter=a.max_niter, rows=(r0, r1), device=a.device, geno_dev_ptr=geno.data_ptr(),
                         n_snp=M, out=out)
            stats += _lib.ibd_mle_stats()
            if len(cuts) > 2:
                print("rows %d-%d: EM kernel %.1f ms" % (r0, r1, stats[0]), file=sys.stderr, flush=True)
        return time.perf_counter() - t0, (stats[0], stats[1], int(stats[2]), int(stats[3])), out[2]

    runs = [run() for _ in range(1 + a.repeats)]
    runs = runs[1:] or runs                    # --repeats 0: the single run is the one reported
    wall, (ms_em, ms_all, useful, issued), nit = min(runs, key=lambda r: r[0])
    iu = np.triu_indices(N, 1)
    n_it = nit[iu].astype(np.float64)
    pairs = len(n_it)
    fma_tflops = _lib.diag_fp64_rate(a.probe_seconds, a.device)
    snp_it = float(useful) * M
    instr_rate = float(issued) * M * FP64_INSTR_PER_LANE_SNP / (ms_em * 1e-3)      # fp64 instructions / s, all lanes
    peak_instr = fma_tflops * 1e12 / 2                                               # an FMA is one instruction, two flops
    print(json.dumps(dict(
        tool="ibd_mle_bench", n_samp=N, n_snp=M, pairs=pairs, row_panels=len(cuts) - 1, max_niter=a.max_niter, missing=a.missing,
        wall_s=round(wall, 4), em_kernel_ms=round(ms_em, 3), kernels_ms=round(ms_all, 3),
        snp_iterations=snp_it, snp_iterations_per_s=snp_it / (ms_em * 1e-3),
        niter_mean=round(float(n_it.mean()), 2), niter_p99=float(np.percentile(n_it, 99)),
        niter_frac_at_max=float((n_it >= a.max_niter).mean()),
        lane_occupancy=round(useful / issued, 4) if issued else None,
        fp64_instr_per_lane_snp=FP64_INSTR_PER_LANE_SNP, fma_stream_tflops=round(fma_tflops, 2),
        fp64_fraction_of_fma_stream=round(instr_rate / peak_instr, 4))))


if __name__ == "__main__":
    main()
