#!/usr/bin/env python
"""Sparse GRM selected from one GCTA panel on one GPU: one JSON line.

Device-resident synthetic genotypes (snpgpu_synth_block), N = 100 000 samples, the row panel 0 .. 2 048, 8 192 SNPs, 2 % missing calls.
For the cutoffs NaN (every pair), 0.05 and 10 (no pair): the count pass, the scan, the write pass and the diagonal kernel of
snpgpu_select_grm from HIP events around the launches (snpgpu_select_grm_stats) and the wall time of the whole call, which ends with
the results in host memory (at most --max-store pairs are stored; n_found is always the total).  Beside them, IN THE SAME RUN: the
existing packed finaliser snpgpu_grm_gcta of the same panel into device memory (what a caller had to run, copy out and threshold
before), and a device-to-device copy of as many bytes as the planes the selection reads (the fp64 sums and the uint32 both-missing
counts: what either has to read at least once)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--snps", type=int, default=8192)
    ap.add_argument("--cutoffs", default="nan,0.05,10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-store", type=int, default=1 << 25, help="pairs stored per call at most (host memory: 16 bytes per pair)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import bench
    from snprelate_amd import _lib

    torch.cuda.set_device(a.device)
    N, rows, B = a.samples, min(a.rows, a.samples), a.snps
    rb = (N + 3) // 4
    geno = torch.empty(B * rb, dtype=torch.uint8, device="cuda")
    _lib.synth_block(geno.data_ptr(), N, 0, B, seed=78, missing=0.02, spectrum=0, device=a.device)
    torch.cuda.synchronize()
    acc = _lib.Accumulator(_lib.GRM_GCTA, N, device=a.device, row_begin=0, row_end=rows, max_block_snps=B)
    acc.feed_device(geno.data_ptr(), B)
    acc.sync()
    del geno
    pad = lambda x: (x + 255) // 256 * 256                                     # noqa: E731
    plane_bytes = (8 + 4) * pad(rows) * pad(N)
    src = torch.empty(plane_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def median(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    copy_ms()
    copy_med = median(copy_ms() for _ in range(a.reps))
    del src, dst
    out = {"tool": "grm_pairs_bench", "source_stamp": bench.source_stamp(), "N": N, "rows": rows, "snps": B, "missing": 0.02,
           "kind": "GCTA", "pairs_in_panel": rows * N - rows * (rows + 1) // 2, "plane_bytes": float(plane_bytes),
           "copy_ms_median": copy_med, "copy_bytes_per_s": plane_bytes / (copy_med * 1e-3)}

    # the existing finaliser of the same panel, packed, into device memory
    slab = acc.slab_size()
    fin = torch.empty(slab, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def finaliser():
        t0 = time.perf_counter()
        acc.grm_gcta(packed=True, out_ptr=fin.data_ptr())
        return (time.perf_counter() - t0) * 1e3

    finaliser()
    fin_ms = median(finaliser() for _ in range(a.reps))
    out["grm_gcta_packed_finaliser"] = {"call_ms": fin_ms, "bytes_written": 8.0 * slab, "copy_ms_over_call_ms": copy_med / fin_ms}
    del fin

    out["select"] = []
    for c in a.cutoffs.split(","):
        cutoff = float(c)
        found = acc.select_grm(_lib.SEL_GRM_GCTA, cutoff, capacity=0)[5]
        count_only = _lib.select_grm_stats()
        cap = min(found, a.max_store)
        runs = []
        for rep in range(a.reps + 1):
            acc.select_grm(_lib.SEL_GRM_GCTA, cutoff, capacity=cap)
            if rep:                                                            # (the first one warms up)
                runs.append(_lib.select_grm_stats())
        st = sorted(runs, key=lambda r: r["call_ms"])[len(runs) // 2]
        out["select"].append({"cutoff": c, "n_found": found, "stored": cap, "bytes_to_host": 16.0 * cap + 8.0 * rows, "count_ms": st["count_ms"],
                              "scan_ms": st["scan_ms"], "write_ms": st["write_ms"], "diag_ms": st["diag_ms"], "call_ms": st["call_ms"],
                              "count_only_call_ms": count_only["call_ms"],
                              "copy_ms_over_count_ms": copy_med / st["count_ms"] if st["count_ms"] > 0 else None,
                              "finaliser_ms_over_count_only_call_ms": fin_ms / count_only["call_ms"] if count_only["call_ms"] > 0 else None})
    acc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
