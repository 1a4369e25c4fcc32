#!/usr/bin/env python
"""snpgpu_geno_select on one GPU: one JSON line (profiles/geno_select_bench.json).

All sources in device memory, N = 100 000 samples, one 65 536-SNP block of synthetic genotypes (snpgpu_synth_block; the same bytes
read as PACKED2 rows and as a snp.order stream of N sample rows).  Medians of 5 runs after a warm-up, from the HIP events of
snpgpu_geno_select_stats, each beside a device-to-device copy of the source bytes IN THE SAME RUN:
  (a) all samples and the first 80 000, from PACKED2 rows             (the copy kernel)
  (b) a random 80 000 of 100 000, from PACKED2 rows                   (the gather kernel)
  (c) the same two selections from the snp.order stream               (the transposition kernel)
Last, at N = 10 000 x 8 192 SNPs, the host path of _init_file2 (numpy unpack / select / pack) and the whole snpgpu_geno_select call
from the same host rows (copies to and from the device included), on the same data.  Every call runs under an alarm of its own."""
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
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--keep", type=int, default=80000)
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a single call may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib
    from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

    torch.cuda.set_device(a.device)
    N, K, B = a.samples, a.keep, a.snps
    assert N % 4 == 0, "the same buffer is read in both layouts: N should be a multiple of 4"
    rb = N // 4
    nbytes = B * rb
    geno = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(geno)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.synth_block(geno.data_ptr(), N, 0, B, seed=78, missing=0.02, spectrum=0, device=a.device)
    torch.cuda.synchronize()
    ptr, optr = int(geno.data_ptr()), int(dst.data_ptr())

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        other.copy_(geno)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def limited(fn):
        signal.alarm(a.limit)                 # no handler: a call that does not return ends the process
        try:
            return fn()
        finally:
            signal.alarm(0)

    copy_ms()
    copies = sorted(copy_ms() for _ in range(a.reps))
    copy_med = copies[len(copies) // 2]
    out = {"tool": "geno_select_bench", "source_stamp": bench.source_stamp(), "N": N, "keep": K, "snps": B, "missing": 0.02,
           "source_bytes": nbytes, "copy_ms_median": copy_med, "copy_ms_all": copies, "copy_bytes_per_s": nbytes / (copy_med * 1e-3)}

    rng = np.random.default_rng(5)
    first = np.arange(K, dtype=np.int32)
    rand = np.sort(rng.choice(N, K, replace=False)).astype(np.int32)
    packed = dict(major=0, n_rows=B, n_cols=N, row_stride_bits=8 * rb)
    stream = dict(major=1, n_rows=N, n_cols=B, row_stride_bits=2 * B)
    cases = [("a_identity_packed", packed, None, "copy_ms"), ("a_first_packed", packed, first, "copy_ms"),
             ("b_random_packed", packed, rand, "gather_ms"), ("c_identity_snp_order", stream, None, "transpose_ms"),
             ("c_first_snp_order", stream, first, "transpose_ms"), ("c_random_snp_order", stream, rand, "transpose_ms")]
    for name, lay, sel, key in cases:
        def run():
            _lib.geno_select(ptr, lay["major"], lay["n_rows"], lay["n_cols"], row_stride_bits=lay["row_stride_bits"], samp_index=sel,
                             out=optr, n_bytes=nbytes, device=a.device)
            return _lib.geno_select_stats()
        limited(run)
        v = sorted(limited(run)[key] for _ in range(a.reps))
        med = v[len(v) // 2]
        n_out = N if sel is None else len(sel)
        out[name] = {"kernel": key[:-3], "ms_median": med, "ms_all": v, "bytes_written": B * ((n_out + 3) // 4),
                     "source_bytes_per_s": nbytes / (med * 1e-3), "ms_over_copy_ms": med / copy_med}
    out["copy_ms_after"] = sorted(copy_ms() for _ in range(a.reps))
    del geno, other, dst

    # the host path of _init_file2 beside the whole call, on the same host rows
    n, L = 10000, 8192
    g = np.random.default_rng(6).integers(0, 3, (L, n)).astype(np.uint8)
    rows = pack_2bit_rows(g)
    flag = np.zeros(n, bool)
    flag[np.random.default_rng(7).choice(n, 8000, replace=False)] = True
    idx = np.flatnonzero(flag).astype(np.int32)
    t0 = time.perf_counter()
    want = pack_2bit_rows(unpack_2bit_rows(rows, n)[:, flag])
    host_ms = (time.perf_counter() - t0) * 1e3
    call = lambda: _lib.geno_select(rows, 0, L, n, row_stride_bits=8 * rows.shape[1], samp_index=idx, device=a.device)  # noqa: E731
    limited(call)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = limited(call)
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    st = _lib.geno_select_stats()
    out["host_path"] = {"N": n, "snps": L, "keep": int(flag.sum()), "numpy_unpack_select_pack_ms": host_ms,
                        "geno_select_whole_call_ms_median": t[len(t) // 2], "geno_select_whole_call_ms_all": t,
                        "of_which": {k: st[k] for k in ("h2d_ms", "gather_ms", "d2h_ms")}, "equal": bool(np.array_equal(got, want))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
