#!/usr/bin/env python
"""snpgdsDiss on one GPU: one JSON line.

Synthetic 65 536-SNP blocks generated on the device (snpgpu_synth_block) at 0 % and 2 % missing calls, fed from device memory to
an SNPGPU_DISS context: N = 10 000 (whole matrix) and N = 100 000 (a row panel of --panel-rows rows).  Reported per case, from HIP
events around each launch group (snpgpu_set_timing): the counter kernels (SumGeno: MX-fp4 general kernel, or the two-product
kernel for a block without missing calls), the weight product (the one-weight fp16 product of blocks with missing calls), the
finaliser (packed output to device memory, host clock around a synchronised call); the whole call (feed + finaliser, host clock).
Rates: pair-genotypes per second of the counter kernels and their MX-fp4 rate (2 products x 2 flops per pair-genotype) as a
fraction of what a register-only stream of the same instruction sustains in the same run (snpgpu_diag_mfma_rate, mode 3).

In the same run and on the same data: the IBS counters (SNPGPU_IBS, the 4-product general kernel) for reference, and the obvious
composition of the dissimilarity -- a KING-robust context (SumGeno = SumSq + N1_Aa + N2_Aa) plus a KING-homo context (8 x its first
weight sum) -- whole calls of both."""
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
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--panel-rows", type=int, default=2048)
    ap.add_argument("--probe-seconds", type=float, default=2.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    from snprelate_amd import _lib

    torch.cuda.set_device(a.device)
    B = a.snps

    def call(kind, N, geno, r1, out):
        """one whole call: context, device feed, finaliser(s) into device memory; (wall ms, counter ms, weight ms, finaliser ms)"""
        with _lib.Accumulator(kind, N, device=a.device, row_begin=0, row_end=r1, max_block_snps=B) as c:
            c.set_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.feed_device(geno.data_ptr(), B, _lib.GENO_PACKED2)
            c.sync()
            t1 = time.perf_counter()
            if kind == _lib.DISS:
                c.diss(packed=True, out_ptr=out[0].data_ptr())
            elif kind == _lib.KING_ROBUST:
                c.king_robust(packed=True, out_ptrs=(out[0].data_ptr(), out[1].data_ptr()))
            elif kind == _lib.KING_HOMO:
                c.king_homo(packed=True, out_ptrs=(out[0].data_ptr(), out[1].data_ptr()))
            else:
                c.ibs_num(packed=True, out_ptrs=(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))
            c.sync()
            t2 = time.perf_counter()
            pair_ms, _ = c.get_timing(0)
            w_ms, _ = c.get_timing(1)
            return dict(wall_ms=(t2 - t0) * 1e3, counter_ms=pair_ms, weight_ms=w_ms, finaliser_ms=(t2 - t1) * 1e3, slab=c.slab_size())

    probe_before, _ = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    cases = []
    for N, r1 in ((10000, 0), (100000, a.panel_rows)):
        rb = (N + 3) // 4
        geno = torch.empty(B * rb, dtype=torch.uint8, device="cuda")
        slab = (r1 or N) * N - (r1 or N) * ((r1 or N) - 1) // 2
        out = [torch.empty(slab * 8, dtype=torch.uint8, device="cuda") for _ in range(3)]
        for missing in (0.0, 0.02):
            _lib.synth_block(geno.data_ptr(), N, 0, B, seed=77, missing=missing, device=a.device)
            torch.cuda.synchronize()
            call(_lib.DISS, N, geno, r1, out)                       # warm-up (code objects, allocations)
            d = call(_lib.DISS, N, geno, r1, out)
            ibs = call(_lib.IBS, N, geno, r1, out)
            kr = call(_lib.KING_ROBUST, N, geno, r1, out)
            kh = call(_lib.KING_HOMO, N, geno, r1, out)
            pg = d["slab"] * B
            cases.append({
                "N": N, "panel_rows": r1 or N, "snps": B, "missing": missing, "pairs": d["slab"],
                "diss": d, "ibs": ibs, "king_robust": kr, "king_homo": kh,
                "counter_pair_genotypes_per_s": pg / (d["counter_ms"] * 1e-3),
                "counter_tflops_useful": 4.0 * pg / (d["counter_ms"] * 1e-3) / 1e12,
                "ibs_counter_pair_genotypes_per_s": pg / (ibs["counter_ms"] * 1e-3),
                "call_pair_genotypes_per_s": pg / (d["wall_ms"] * 1e-3),
                "composition_wall_ms": kr["wall_ms"] + kh["wall_ms"],
                "speedup_vs_composition": (kr["wall_ms"] + kh["wall_ms"]) / d["wall_ms"],
            })
        del geno, out
        torch.cuda.empty_cache()
    probe_after, mhz = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    sustained = 0.5 * (probe_before + probe_after)
    for c in cases:
        c["counter_fraction_of_sustained_fp4"] = c["counter_tflops_useful"] / sustained if sustained > 0 else None
    print(json.dumps({"tool": "diss_bench", "cases": cases, "mfma_fp4_sustained_tflops": sustained,
                      "mfma_fp4_probe_tflops": [probe_before, probe_after], "implied_mhz": mhz}))


if __name__ == "__main__":
    main()
