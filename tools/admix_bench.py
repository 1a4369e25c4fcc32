#!/usr/bin/env python
"""The EM for ancestry proportions on one GPU: one JSON line (profiles/admix_bench.json).  Runs on an MI355X; no test runs it.

The seeded synthetic data set (snpgpu_synth_block: --n samples x --snps SNPs, --missing missing calls) is made on the device feed
block by feed block and fed as 2-bit device rows to a snpgpu_admix object with one internal block, once per K of --k.  Per K: the
HIP-event time of --iters iterations from the seeded start (snpgpu_admix_stats; the likelihood-only pass that ends a run is timed
apart, by a run of no iteration, and taken off), ms per iteration, genotypes per second, and the fp64 VALU instructions the two
owners issue per genotype -- a fixed count from the gfx950 code object of their inner loops (FP64_PER_GENOTYPE below; DESIGN.md 32
says how it was counted), not a measured counter -- as a share of what a register-only v_fma_f64 stream issues in the same time.
Beside it two yardsticks from the same run: that stream's rate (snpgpu_diag_fp64_rate) and a device-to-device copy of the resident
2-bit block."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# fp64 VALU instructions per genotype in the loop bodies of (admix_snp_kernel<KP, true>, admix_samp_kernel<KP>), counted in the
# gfx950 assembly: all v_*_f64 between the loop's label and its back edge, both sides of the `called` branch
FP64_PER_GENOTYPE = {3: (191, 39), 8: (212, 64), 16: (243, 104)}
# ... of the tree with this source stamp.  The count is static: it goes stale with any change of the kernels or of the compiler, so the
# JSON line says which tree it was taken from and whether that is the tree measured; a K outside the table gets no such figure.
FP64_COUNTED_AT_STAMP = "a008ca7a753ce529"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--k", type=int, nargs="+", default=[3, 8, 16])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--feed", type=int, default=8192, help="SNPs per feed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admix_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib, api

    n, m = a.n, a.snps
    fma_tflops = _lib.diag_fp64_rate(1.0)
    out = {"tool": "admix_bench", "source_stamp": bench.source_stamp(), "device": torch.cuda.get_device_name(0), "n": n, "snps": m,
           "missing": a.missing, "iters": a.iters, "feed_snps": a.feed, "fp64_fma_stream_tflops": fma_tflops,
           "fp64_instructions_per_genotype_is": "a static count from the gfx950 code object of the tree with source stamp %s, not a counter"
                                                % FP64_COUNTED_AT_STAMP,
           "fp64_count_is_of_this_tree": bench.source_stamp() == FP64_COUNTED_AT_STAMP, "runs": []}
    rows = torch.empty((a.feed, (n + 3) // 4), dtype=torch.uint8, device="cuda")
    for k in a.k:
        with _lib.Admix(n, k, m, block_snps=0) as ad:
            t0 = time.perf_counter()
            for s0 in range(0, m, a.feed):
                nb = min(a.feed, m - s0)
                _lib.synth_block(rows.data_ptr(), n, s0, nb, 20240601, missing=a.missing)
                torch.cuda.synchronize()
                ad.feed(int(rows.data_ptr()), fmt=_lib.GENO_PACKED2, n_snp=nb)
            feed_s = time.perf_counter() - t0
            q0, f0 = api.admix_seeded_start(n, k, np.full(m, 0.3), 1, 1e-6)
            ad.set(q0, f0)
            ll0, _ = ad.run(0)                                   # warm-up and the likelihood-only pass on its own
            ms_l = ad.stats()["pass_ms"]
            ll0, _ = ad.run(0)
            ms_l = ad.stats()["pass_ms"] - ms_l
            before = ad.stats()["pass_ms"]
            t0 = time.perf_counter()
            ll, done = ad.run(a.iters, float("-inf"))
            wall = time.perf_counter() - t0
            st = ad.stats()
            ms_iter = (st["pass_ms"] - before - ms_l) / a.iters
            rec = {"k": k, "feed_wall_s": feed_s, "ms_per_iteration": ms_iter, "likelihood_pass_ms": ms_l, "run_wall_s": wall,
                   "genotypes_per_s": n * m / (ms_iter * 1e-3), "loglik": [float(x) for x in ll], "blocks": st["blocks"],
                   "block_snps": st["block_snps"], "resident_bytes": st["resident_bytes"], "launches": st["launches"]}
            if k in FP64_PER_GENOTYPE:
                per = sum(FP64_PER_GENOTYPE[k])
                rec["fp64_instructions_per_genotype"] = per
                # a v_fma_f64 stream of fma_tflops issues fma_tflops / 2 lane-instructions per second
                rec["fp64_issue_share_of_fma_stream"] = per * n * m / (ms_iter * 1e-3) / (fma_tflops * 1e12 / 2)
            del q0, f0
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    # yardstick: a device-to-device copy of the resident block
    rb = (n + 3) // 4
    src = torch.empty((m, rb), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    best = float("inf")
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        dst.copy_(src)
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1))
    out["d2d_copy_of_the_block"] = {"bytes": m * rb, "ms": best, "gb_per_s": 2.0 * m * rb / (best * 1e-3) / 1e9}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
