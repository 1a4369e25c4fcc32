#!/usr/bin/env python
"""snpgpu_geno_merge on one GPU: one JSON line (profiles/geno_merge_bench.json).

N = 100 000 samples as parts of 60 000 + 39 999 + 1, one 65 536-SNP block of synthetic genotypes per part resident on the device
(snpgpu_synth_block), every second output row flipped in parts 2 and 3.  Medians of 5 runs after a warm-up, IN THE SAME RUN:
  (a) the splice kernel (HIP events of snpgpu_geno_merge_stats) and the whole call (host clock)
  (b) a device-to-device copy of the merged block
  (c) the snpgpu_geno_select calls that bring the three parts to byte-aligned rows of their own (the copy kernel), summed
and the merged bytes are compared once with what the selections and numpy give for a few rows.  Every call runs under an alarm
of its own."""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parts", type=int, nargs="+", default=[60000, 39999, 1])
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a single call may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geno_merge_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib
    from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

    torch.cuda.set_device(a.device)
    B, sizes = a.snps, list(a.parts)
    N = sum(sizes)
    rb = (N + 3) // 4
    src = [torch.empty(B * ((n + 3) // 4), dtype=torch.uint8, device="cuda") for n in sizes]
    for i, (t, n) in enumerate(zip(src, sizes)):
        _lib.synth_block(t.data_ptr(), n, 0, B, seed=90 + i, missing=0.02, spectrum=0, device=a.device)
    merged = torch.empty(B * rb, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(merged)
    aligned = [torch.empty_like(t) for t in src]
    torch.cuda.synchronize()
    flip = (np.arange(B) % 2).astype(np.uint8)

    def limited(fn):
        signal.alarm(a.limit)                 # no handler: a call that does not return ends the process
        try:
            return fn()
        finally:
            signal.alarm(0)

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        other.copy_(merged)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def merge():
        parts = [_lib.merge_part(int(t.data_ptr()), 0, B, n, row_stride_bits=8 * ((n + 3) // 4), n_bytes=t.numel(),
                                 flip=flip if i else None) for i, (t, n) in enumerate(zip(src, sizes))]
        t0 = time.perf_counter()
        _lib.geno_merge(parts, int(merged.data_ptr()), n_snp_out=B, device=a.device)
        return (time.perf_counter() - t0) * 1e3, _lib.geno_merge_stats()

    def selects():
        ms = 0.0
        for t, n, d in zip(src, sizes, aligned):
            _lib.geno_select(int(t.data_ptr()), 0, B, n, row_stride_bits=8 * ((n + 3) // 4), out=int(d.data_ptr()), n_bytes=t.numel(),
                             device=a.device)
            ms += _lib.geno_select_stats()["copy_ms"]
        return ms

    def median(v):
        v = sorted(v)
        return v[len(v) // 2], v

    limited(copy_ms)
    limited(merge)
    limited(selects)
    copy_med, copies = median(limited(copy_ms) for _ in range(a.reps))
    runs = [limited(merge) for _ in range(a.reps)]
    call_med, calls = median(r[0] for r in runs)
    splice_med, splices = median(r[1]["splice_ms"] for r in runs)
    sel_med, sels = median(limited(selects) for _ in range(a.reps))
    copy_after = sorted(limited(copy_ms) for _ in range(a.reps))

    # a few rows against the selections' rows and numpy
    rows = [0, 1, 2, B // 2 + 1, B - 1]
    got = merged.view(B, rb)[rows].cpu().numpy()
    cols = []
    for i, (d, n) in enumerate(zip(aligned, sizes)):
        g = unpack_2bit_rows(d.view(B, (n + 3) // 4)[rows].cpu().numpy(), n)
        cols.append(np.where((flip[rows][:, None] != 0) & (i > 0), np.array([2, 1, 0, 3], np.uint8)[g], g))
    equal = bool(np.array_equal(got, pack_2bit_rows(np.concatenate(cols, 1))))

    nbytes = B * rb
    out = {"tool": "geno_merge_bench", "source_stamp": bench.source_stamp(), "N": N, "parts": sizes, "snps": B, "missing": 0.02,
           "rows_flipped": int(flip.sum()), "merged_bytes": nbytes, "measured": "once",
           "splice_ms_median": splice_med, "splice_ms_all": splices, "splice_written_bytes_per_s": nbytes / (splice_med * 1e-3),
           "whole_call_ms_median": call_med, "whole_call_ms_all": calls, "stats_of_last_call": runs[-1][1],
           "copy_ms_median": copy_med, "copy_ms_all": copies, "copy_ms_after": copy_after, "copy_bytes_per_s": nbytes / (copy_med * 1e-3),
           "splice_ms_over_copy_ms": splice_med / copy_med,
           "select_copy_kernels_ms_median": sel_med, "select_copy_kernels_ms_all": sels, "rows_equal_selections": equal}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
