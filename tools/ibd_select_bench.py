#!/usr/bin/env python
"""Selection of related pairs from one KING-robust panel on one GPU: one JSON line.

Device-resident synthetic genotypes (snpgpu_synth_block), N = 100 000 samples, the row panel 0 .. 2 048, 2 % missing calls.  For the
cutoffs NaN (every pair), 0.0442 and 0.354: the count pass, the scan and the write pass of snpgpu_select_pairs from HIP events around
the launches (snpgpu_select_stats) and the wall time of the whole call, outputs in device memory with capacity = the number found.
Beside them, IN THE SAME RUN: the existing packed finaliser snpgpu_king_robust of the same panel into device memory (what a caller had
to run, and then filter, before), and a device-to-device copy of as many bytes as the panel's five uint32 counter planes (what either
has to read at least once)."""
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
    ap.add_argument("--cutoffs", default="nan,0.0442,0.354")
    ap.add_argument("--reps", type=int, default=3)
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
    acc = _lib.Accumulator(_lib.KING_ROBUST, N, device=a.device, row_begin=0, row_end=rows, max_block_snps=B)
    acc.feed_device(geno.data_ptr(), B)
    acc.sync()
    del geno
    pad = lambda x: (x + 255) // 256 * 256                                     # noqa: E731
    plane_bytes = 5 * 4 * pad(rows) * pad(N)
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
    del dst
    out = {"tool": "ibd_select_bench", "source_stamp": bench.source_stamp(), "N": N, "rows": rows, "snps": B, "missing": 0.02,
           "kind": "KING-robust", "pairs_in_panel": rows * N - rows * (rows + 1) // 2, "plane_bytes": float(plane_bytes),
           "copy_ms_median": copy_med, "copy_bytes_per_s": plane_bytes / (copy_med * 1e-3)}

    # the existing finaliser of the same panel, packed, into device memory
    slab = acc.slab_size()
    fin = [torch.empty(slab, dtype=torch.float64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()

    def finaliser():
        t0 = time.perf_counter()
        acc.king_robust(packed=True, out_ptrs=[x.data_ptr() for x in fin])
        return (time.perf_counter() - t0) * 1e3

    finaliser()
    fin_ms = median(finaliser() for _ in range(a.reps))
    out["king_robust_packed_finaliser"] = {"call_ms": fin_ms, "bytes_written": 16.0 * slab, "copy_ms_over_call_ms": copy_med / fin_ms}
    del fin

    out["select"] = []
    for c in a.cutoffs.split(","):
        cutoff = float(c)
        found = acc.select_pairs(_lib.SEL_KING_ROBUST, cutoff, capacity=0)[5]
        count_only = _lib.select_stats()
        cap = max(found, 1)
        bufs = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.empty(cap, dtype=torch.float64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        ptrs = [bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), 0, bufs[3].data_ptr()]
        runs = []
        for rep in range(a.reps + 1):
            acc.select_pairs(_lib.SEL_KING_ROBUST, cutoff, capacity=cap, out_ptrs=ptrs)
            if rep:                                                            # (the first one warms up)
                runs.append(_lib.select_stats())
        st = sorted(runs, key=lambda r: r["call_ms"])[len(runs) // 2]
        out["select"].append({"cutoff": c, "n_found": found, "bytes_written": 24.0 * found, "count_ms": st["count_ms"], "scan_ms": st["scan_ms"],
                              "write_ms": st["write_ms"], "call_ms": st["call_ms"], "count_only_call_ms": count_only["call_ms"],
                              "copy_ms_over_count_ms": copy_med / st["count_ms"] if st["count_ms"] > 0 else None,
                              "finaliser_ms_over_call_ms": fin_ms / st["call_ms"] if st["call_ms"] > 0 else None})
        del bufs
    acc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
