#!/usr/bin/env python
"""snpgpu_geno_convert on one GPU: one JSON line (profiles/bed_bench.json).

All sources in device memory, N = 100 000 samples, one 65 536-SNP block of synthetic genotypes (snpgpu_synth_block; the same bytes
read as SNP rows -- PACKED2, or a .bed body of mode 1 -- and as sample rows -- a .bed body of mode 0; what the codes mean does not
change what the kernels do).  Medians of 5 runs after a warm-up, from the HIP events of snpgpu_geno_convert_stats.  Four
conversions, each with all samples and with a random 80 000:
  bed1_to_packed2   BED mode 1 -> PACKED2          (copy / gather kernel, BED -> GDS)
  bed0_to_packed2   BED mode 0 -> PACKED2          (transposition kernel, BED -> GDS)
  packed2_to_bed1   PACKED2 -> BED mode 1          (copy / gather kernel, GDS -> BED)
  packed2_to_bed0   PACKED2 -> BED mode 0          (transposition kernel with the axes exchanged, GDS -> BED)
and beside each, IN THE SAME RUN, the identity call of the same layout (source and dst of the source's code set) and a
device-to-device copy of the block.  Last, the wall time of snpgdsOpenBED -> snpgdsIBSNum on the committed PLINK fixture (60
samples x 5 000 SNPs), recorded only.  Every call runs under an alarm of its own."""
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
    from snprelate_amd import _lib, api

    torch.cuda.set_device(a.device)
    N, K, B = a.samples, a.keep, a.snps
    assert N % 4 == 0 and B % 4 == 0, "the same buffer is read in both layouts: N and the SNPs should be multiples of 4"
    nbytes = B * (N // 4)
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

    def median(v):
        return sorted(v)[len(v) // 2]

    copy_ms()
    copies = sorted(copy_ms() for _ in range(a.reps))
    out = {"tool": "bed_bench", "source_stamp": bench.source_stamp(), "N": N, "keep": K, "snps": B, "missing": 0.02,
           "source_bytes": nbytes, "copy_ms_median": median(copies), "copy_ms_all": copies,
           "copy_bytes_per_s": nbytes / (median(copies) * 1e-3)}

    rand = np.sort(np.random.default_rng(5).choice(N, K, replace=False)).astype(np.int32)
    snp_rows = dict(major=0, n_rows=B, n_cols=N, row_stride_bits=2 * N)
    samp_rows = dict(major=1, n_rows=N, n_cols=B, row_stride_bits=2 * B)
    G, D = _lib.CODE_GDS, _lib.CODE_BED
    # name, source layout, source code, dst code, dst_major, the kernel's field with all samples / with the list
    cases = [("bed1_to_packed2", snp_rows, D, G, 0, ("copy_ms", "gather_ms")),
             ("bed0_to_packed2", samp_rows, D, G, 0, ("transpose_ms", "transpose_ms")),
             ("packed2_to_bed1", snp_rows, G, D, 0, ("copy_ms", "gather_ms")),
             ("packed2_to_bed0", snp_rows, G, D, 1, ("transpose_ms", "transpose_ms"))]
    for name, lay, sc, dc, dm, keys in cases:
        for sel, key, tag in ((None, keys[0], "all"), (rand, keys[1], "random")):
            def run(dst_code):
                _lib.geno_convert(ptr, lay["major"], lay["n_rows"], lay["n_cols"], src_code=sc, dst_code=dst_code, dst_major=dm,
                                  row_stride_bits=lay["row_stride_bits"], samp_index=sel, out=optr, n_bytes=nbytes, device=a.device)
                return _lib.geno_convert_stats()[key]
            limited(lambda: run(dc))
            limited(lambda: run(sc))
            # recoded and identity runs alternate, so that a drift of the clocks meets both
            v, w = [], []
            for _ in range(a.reps):
                v.append(limited(lambda: run(dc)))
                w.append(limited(lambda: run(sc)))
            v.sort()
            w.sort()
            out["%s_%s" % (name, tag)] = {
                "kernel": key[:-3], "ms_median": median(v), "ms_all": v, "identity_ms_median": median(w), "identity_ms_all": w,
                "ms_over_identity_ms": median(v) / median(w), "ms_over_copy_ms": median(v) / median(copies),
                "source_bytes_per_s": nbytes / (median(v) * 1e-3)}
    out["copy_ms_after"] = sorted(copy_ms() for _ in range(a.reps))
    del geno, other, dst

    # the whole call on the fixture: open the three files, select, count
    fix = [os.path.join(ROOT, "tests", "golden", "plinkhapmap.%s.gz" % e) for e in ("bed", "fam", "bim")]

    def whole():
        t0 = time.perf_counter()
        api.snpgdsIBSNum(api.snpgdsOpenBED(*fix, verbose=False), verbose=False, device=a.device)
        return (time.perf_counter() - t0) * 1e3
    limited(whole)
    t = sorted(limited(whole) for _ in range(a.reps))
    out["fixture_open_bed_ibsnum"] = {"samples": 60, "snps": 5000, "wall_ms_median": median(t), "wall_ms_all": t}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
