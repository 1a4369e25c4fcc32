#!/usr/bin/env python
"""snpgdsFst / snpgdsSlidingWindow on one GPU: one JSON line.

Device-resident synthetic genotypes (snpgpu_synth_block, spectrum 3: three sub-populations, sample % 3), N = 100 000 samples,
one 65 536-SNP block, 2 % missing calls; populations K = 2, 3, 5, 26 with labels sample % K.  Per K, from HIP events around the
launches (snpgpu_pop_stats): the counter kernel's time, the genotype bytes it read per second, and that as a fraction of what a
plain device-to-device copy of the same bytes reaches IN THE SAME RUN (the roofline of a one-pass read kernel: bytes copied per
second of the copy, which reads and writes them); then the whole snpgpu_fst call (host clock around the synchronous call, W&C84 and
W&H02).  Last, a whole-chromosome scan with winsize / shift = 10 through snpgpu_fst_windows (host rows, copy included) against the
numpy restatement of tests/fst_ref.py (counters once, then every window) on the same data, at a size the CPU finishes (--scan-*)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--pops", type=int, nargs="+", default=[2, 3, 5, 26])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scan-samples", type=int, default=2000)
    ap.add_argument("--scan-snps", type=int, default=20000)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import fst_ref as R
    from oracle.synth import synth_hash_block_packed
    from snprelate_amd import _lib
    from snprelate_amd.gds import unpack_2bit_rows

    torch.cuda.set_device(a.device)
    N, B = a.samples, a.snps
    rb = (N + 3) // 4
    geno = torch.empty(B * rb, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(geno)
    _lib.synth_block(geno.data_ptr(), N, 0, B, seed=77, missing=0.02, spectrum=3, device=a.device)
    torch.cuda.synchronize()

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        other.copy_(geno)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    copy_ms()
    copies = sorted(copy_ms() for _ in range(a.reps))
    nbytes = float(B) * rb
    copy_rate = nbytes / (copies[len(copies) // 2] * 1e-3)
    cases = []
    for K in a.pops:
        pop = (np.arange(N) % K).astype(np.int32)
        _lib.pop_counts(int(geno.data_ptr()), N, pop, K, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device)     # warm-up
        ms = []
        for _ in range(a.reps):
            _lib.pop_counts(int(geno.data_ptr()), N, pop, K, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device)
            ms.append(_lib.pop_stats()[0])
        ms.sort()
        med = ms[len(ms) // 2]
        case = {"K": K, "counter_ms_median": med, "counter_ms_all": ms, "genotype_bytes": nbytes,
                "genotype_bytes_per_s": nbytes / (med * 1e-3), "fraction_of_copy_rate": nbytes / (med * 1e-3) / copy_rate}
        for name, code in (("wc84", _lib.FST_WC84), ("wh02", _lib.FST_WH02)):
            _lib.fst(int(geno.data_ptr()), N, pop, K, code, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device)
            t0 = time.perf_counter()
            f, _, _ = _lib.fst(int(geno.data_ptr()), N, pop, K, code, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device)
            case["fst_call_ms_" + name] = (time.perf_counter() - t0) * 1e3
            case["fst_kernels_ms_" + name] = _lib.pop_stats()[2]
            case["fst_" + name] = f
        cases.append(case)
    copies_after = sorted(copy_ms() for _ in range(a.reps))

    # whole-chromosome scan, winsize / shift = 10, against the numpy restatement on the same data
    n, m = a.scan_samples, a.scan_snps
    packed = synth_hash_block_packed(n, 0, m, 77, missing=0.02, spectrum=3)
    pop = (np.arange(n) % 3).astype(np.int32)
    pos = 1000 * np.arange(1, m + 1, dtype=np.int64)
    winsize, shift = 100000, 10000
    n_win = (int(pos[-1]) - winsize - int(pos[0])) // shift + 2
    lo = int(pos[0]) + shift * np.arange(n_win, dtype=np.int64)
    first, last = np.searchsorted(pos, lo, "left"), np.searchsorted(pos, lo + winsize, "left")
    offsets = np.concatenate([[0], np.cumsum(last - first)]).astype(np.int64)
    idx = np.concatenate([np.arange(x, y) for x, y in zip(first, last)]).astype(np.int32)
    _lib.fst_windows(packed, n, pop, 3, offsets, idx, _lib.FST_WC84, device=a.device)
    t0 = time.perf_counter()
    fw, _, _ = _lib.fst_windows(packed, n, pop, 3, offsets, idx, _lib.FST_WC84, device=a.device)
    gpu_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ac, cc = R.pop_counts(unpack_2bit_rows(packed, n), pop, 3)
    ref = np.array([R.fst_set(ac, cc, "W&C84", idx[offsets[w]:offsets[w + 1]])["Fst"] for w in range(n_win)])
    cpu_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({
        "tool": "fst_bench", "N": N, "snps": B, "missing": 0.02, "copy_ms_median": copies[len(copies) // 2], "copy_ms_all": copies,
        "copy_ms_after": copies_after, "copy_bytes_per_s": copy_rate, "cases": cases,
        "scan": {"samples": n, "snps": m, "windows": int(n_win), "winsize": winsize, "shift": shift, "method": "W&C84",
                 "snpgpu_fst_windows_ms": gpu_ms, "fst_ref_ms": cpu_ms, "max_abs_diff": float(np.nanmax(np.abs(fw - ref)))}}))


if __name__ == "__main__":
    main()
