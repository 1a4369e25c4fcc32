#!/usr/bin/env python
"""snpgdsPairScore on one GPU: one JSON line.

Device-resident synthetic genotypes (snpgpu_synth_block), N = 100 000 samples, one 65 536-SNP block, 2 % missing calls, 50 000
disjoint pairs (sample 2 j with sample 2 j + 1).  From HIP events around the launches (snpgpu_pair_stats): the per-SNP table
kernel, the transposition to sample-major words, the per-pair counter and the matrix kernel, each beside a device-to-device copy
of the same block IN THE SAME RUN (the genotype bytes are what every kernel has to read at least once; the matrix kernel also
writes n_pair bytes per SNP, reported with it).  Then the wall time of the whole calls as the C ABI runs them: the tables and the
host finaliser for "per.pair" and "per.snp", and the score matrix as bit2 bytes streamed to host memory (--matrix-snps of the
block: the int32 matrix of the whole block would be 13 GB)."""
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
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--pairs", type=int, default=50000)
    ap.add_argument("--matrix-snps", type=int, default=65536)
    ap.add_argument("--method", default="GVH.minor.only", help="a method that flips, so that every kernel runs")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib

    torch.cuda.set_device(a.device)
    N, B, n_pair = a.samples, a.snps, a.pairs
    if 2 * n_pair > N:
        raise SystemExit("disjoint pairs need 2 * pairs <= samples")
    rb = (N + 3) // 4
    geno = torch.empty(B * rb, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(geno)
    _lib.synth_block(geno.data_ptr(), N, 0, B, seed=78, missing=0.02, spectrum=0, device=a.device)
    torch.cuda.synchronize()
    ptr = int(geno.data_ptr())
    idx1 = np.arange(0, 2 * n_pair, 2, dtype=np.int32)
    idx2 = idx1 + 1
    major = a.method in _lib.PAIR_METHODS[3:]

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        other.copy_(geno)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    copy_ms()
    copies = sorted(copy_ms() for _ in range(a.reps))
    copy_med = copies[len(copies) // 2]
    nbytes = float(B) * rb
    out = {"tool": "pair_score_bench", "source_stamp": bench.source_stamp(), "N": N, "snps": B, "pairs": n_pair, "missing": 0.02,
           "method": a.method, "genotype_bytes": nbytes, "copy_ms_median": copy_med, "copy_bytes_per_s": nbytes / (copy_med * 1e-3)}

    def run(fn):
        """median over reps of (wall ms, stats) after one warm-up"""
        fn()
        rows = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            rows.append(((time.perf_counter() - t0) * 1e3, _lib.pair_stats()))
        rows.sort(key=lambda r: r[0])
        return rows[len(rows) // 2]

    def kernel(ms, launches=None):
        d = {"ms": ms, "copy_ms_over_kernel_ms": copy_med / ms if ms > 0 else None}
        if launches is not None:
            d["launches"] = launches
        return d

    def per_pair():
        pt, _, _ = _lib.pair_tables(ptr, N, idx1, idx2, need_major=major, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device,
                                    want_snp=False, want_flip=False)
        return _lib.pair_score_final(pt, a.method, True)

    def per_snp():
        _, st, fl = _lib.pair_tables(ptr, N, idx1, idx2, need_major=major, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device,
                                     want_pair=False)
        return _lib.pair_score_final(st, a.method, True, flip=fl)

    ms_nb = min(a.matrix_snps, B)

    def matrix():
        return _lib.pair_score_matrix(ptr, N, idx1, idx2, a.method, True, bit2=True, fmt=_lib.GENO_PACKED2, n_snp=ms_nb, device=a.device)

    wall, st = run(per_pair)
    out["per_pair"] = {"call_ms": wall, "snp_table_kernel": kernel(st["snp_table_ms"], st["snp_table_launches"]),
                       "words_kernel": kernel(st["words_ms"]), "pair_count_kernel": kernel(st["pair_count_ms"]),
                       "launches_words_and_count": st["other_launches"]}
    wall, st = run(per_snp)
    out["per_snp"] = {"call_ms": wall, "snp_table_kernel": kernel(st["snp_table_ms"], st["snp_table_launches"])}
    wall, st = run(matrix)
    frac = ms_nb / float(B)
    out["matrix"] = {"call_ms": wall, "snps": ms_nb, "element": "bit2 bytes", "host_bytes": float(ms_nb) * n_pair,
                     "snp_table_kernel": kernel(st["snp_table_ms"] / frac if frac else 0, st["snp_table_launches"]),
                     "matrix_kernel": dict(kernel(st["matrix_ms"] / frac if frac else 0), scaled_to_snps=B,
                                           bytes_written_per_s=float(ms_nb) * n_pair / (st["matrix_ms"] * 1e-3))}
    out["copy_ms_after"] = sorted(copy_ms() for _ in range(a.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
