#!/usr/bin/env python
"""snpgdsLDMat throughput on one GPU: one JSON line.

The genotypes are generated on the device (snpgpu_synth_block, spectrum 4 = 48-SNP LD blocks) and fed from device memory in
blocks, so the line measures the LD object itself: create -> feed -> result (the finished matrix in host memory).  Reported:
wall time of that sequence, HIP-event kernel time of the table (count) kernel and of the finaliser, pair-sample-genotypes per
second (pairs * N / wall time, and pairs * N / count-kernel time), the wall time by phase (create / feed / result) with the
HIP-event time of the device -> result copies inside it, and the count kernel's MX-fp4 rate as a fraction of what a register-only stream of the same
instruction sustains on this device in the same run (snpgpu_diag_mfma_rate, mode 3)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METHODS = ("composite", "r", "dprime", "corr", "cov")
MFMA_FLOP = 2 * 32 * 32 * 64          # one v_mfma_scale_f32_32x32x64_f8f6f4
# csrc/ld.hip's sizing of the sliding-window blocks (LD_BLOCK_DEFAULT, LD_TABLE_BUDGET): rows per table launch
LD_BLOCK_DEFAULT, LD_TABLE_BUDGET = 16384, 1 << 30


def band_block(slide, max_block_snps=0):
    want = max_block_snps if max_block_snps > 0 else LD_BLOCK_DEFAULT
    fit = LD_TABLE_BUDGET // (slide * 44)
    return max(64, min((want + 63) // 64 * 64, fit // 64 * 64))


def band_tile_waves(L, slide, blk, feed):
    """64 x 64 tiles the band launches compute (ld.hip's schedule: row buffers of slide + blk rows, chunks of blk columns)"""
    cap = min(slide + blk, L)
    base = n_res = done = fed = tiles = 0
    while fed < L:
        m = min(feed, L - fed)
        while m > 0:
            t = min(m, cap - n_res)
            n_res += t; fed += t; m -= t
            if n_res == cap or fed == L:
                last = fed == L
                i_end = L if last else base + n_res - slide
                for i0 in range(done, i_end, blk):
                    n_i = min(blk, i_end - i0)
                    n_b = n_res - (i0 - base)
                    for x in range((n_i + 63) // 64):
                        for y in range((63 + slide) // 64 + 1):
                            if 64 * y - 63 <= slide and 64 * x + 64 * y < n_b:
                                tiles += 1
                done = i_end
                if not last:
                    keep = base + n_res - i_end
                    base, n_res = i_end, keep
    return tiles


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-samp", type=int, default=100000)
    ap.add_argument("--n-snp", type=int, default=65536)
    ap.add_argument("--slide", type=int, default=250)
    ap.add_argument("--method", default="composite", choices=METHODS)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--feed-block", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=2, help="timed runs after one warm-up run; the best is reported")
    ap.add_argument("--probe-seconds", type=float, default=2.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    from snprelate_amd import _lib

    N, L, slide = a.n_samp, a.n_snp, a.slide
    rb = (N + 3) // 4
    torch.cuda.set_device(a.device)
    geno = torch.empty(L * rb, dtype=torch.uint8, device="cuda")
    for i0 in range(0, L, 8192):
        n = min(8192, L - i0)
        _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, n, seed=2024, missing=a.missing, spectrum=4, device=a.device)
    torch.cuda.synchronize()

    def run(timing):
        t0 = time.perf_counter()
        with _lib.LDMatrix(N, L, METHODS.index(a.method) + 1, slide, False, device=a.device) as ld:
            t1 = time.perf_counter()
            ld.set_timing(timing)
            t2 = time.perf_counter()
            for i0 in range(0, L, a.feed_block):
                ld.feed_device(geno.data_ptr() + i0 * rb, min(a.feed_block, L - i0))
            t3 = time.perf_counter()
            out = ld.result()
            t4 = time.perf_counter()
            tm = [ld.get_timing(w) if timing else (0.0, 0) for w in range(3)]
        t5 = time.perf_counter()
        phases = {"create_s": t1 - t0, "feed_s": t3 - t2, "result_s": t4 - t3, "destroy_s": t5 - t4}
        return t4 - t0, tm, phases, out

    probe_before, _ = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    run(False)
    best = None
    for _ in range(max(1, a.repeats)):
        r = run(True)
        if best is None or r[0] < best[0]:
            best = r
    probe_after, mhz = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    wall, ((kms, kl), (fms, fl), (cms, cl)), phases, out = best
    s = min(slide, L) if slide > 0 else L
    pairs = (L * s - s * (s + 1) // 2) if slide > 0 else L * (L + 1) // 2
    nz = float(out[~(out != out)].size)
    sustained = 0.5 * (probe_before + probe_after)
    rec = {"tool": "ld_bench", "N": N, "L": L, "slide": slide, "method": a.method, "missing": a.missing,
           "wall_s": wall, "count_kernel_ms": kms, "count_launches": kl, "final_kernel_ms": fms, "final_launches": fl,
           "result_copy_ms": cms, "result_copies": cl, "phases_s": phases,
           "pairs": pairs, "pair_sample_genotypes_per_s": pairs * N / wall,
           "count_kernel_pair_sample_genotypes_per_s": pairs * N / (kms * 1e-3) if kms > 0 else None,
           "finite_values": int(nz)}
    rbp = (rb + 31) // 32 * 32
    if slide > 0:
        tiles = band_tile_waves(L, s, band_block(s), a.feed_block)
        flop = tiles * 4 * (rbp // 32) * 2 * 9 * MFMA_FLOP
        rec["count_tiles"] = tiles
        rec["count_kernel_tflops_executed"] = flop / (kms * 1e-3) / 1e12 if kms > 0 else None
        rec["count_kernel_tflops_useful"] = pairs * 9 * 2 * 4 * rbp / (kms * 1e-3) / 1e12 if kms > 0 else None
        rec["mfma_fp4_sustained_tflops"] = sustained
        rec["mfma_fp4_probe_tflops"] = [probe_before, probe_after]
        rec["fraction_of_sustained"] = rec["count_kernel_tflops_executed"] / sustained if kms > 0 and sustained > 0 else None
    rec["rest_of_wall_over_count_kernel"] = (wall * 1e3 - kms) / kms if kms > 0 else None
    rec["implied_mhz"] = mhz
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
