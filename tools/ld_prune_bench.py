#!/usr/bin/env python
"""snpgdsLDpruning on one GPU: one JSON line.

Synthetic run: N samples generated on the device (snpgpu_synth_block, spectrum 4 = 48-SNP LD blocks, 2 % missing), several
chromosomes of M SNPs with uneven positions (mean gap about 3 kb, 30 % of the gaps 50 times shorter: dense stretches), each
pruned by one snpgpu_ld_prune call fed from device memory.  Reported per chromosome: the band width W, band pairs, kept
fraction, the call's wall time and its phase times (snpgpu_ld_prune_info: HIP events for staging, tables, bits and the bit
copies; host clock for the scan).  Totals: pair-sample-genotypes per second of the table launches (band pairs x N over table
kernel time) and of the whole calls (over wall time), and the table kernel's MX-fp4 rate as a fraction of what a register-only
stream of the same instruction sustains on this device in the same run (snpgpu_diag_mfma_rate, mode 3).

--hapmap: also times api.snpgdsLDpruning on tests/golden/hapmap_geno.gds (22 autosomes, defaults, start_pos "first") next
to the CPU restatement of tests/ld_prune_ref.py (numpy LD values of the band, then the loop transcription) on the same input."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_FLOP = 2 * 32 * 32 * 64          # one v_mfma_scale_f32_32x32x64_f8f6f4
INT_MAX = 2 ** 31 - 1


def positions(M, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    gaps = rng.exponential(3000, M).astype(np.int64)
    gaps[rng.random(M) < 0.3] //= 50
    return np.cumsum(gaps).astype(np.int32)


def hapmap_run(device):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ld_prune_ref
    from snprelate_amd import api
    from snprelate_amd.gds import open_gds, unpack_2bit_rows
    h = open_gds(os.path.join(ROOT, "tests", "golden", "hapmap_geno.gds"))
    api.snpgdsLDpruning(h, verbose=False, start_pos="first", device=device)        # warm-up
    t0 = time.perf_counter()
    res = api.snpgdsLDpruning(h, verbose=False, start_pos="first", device=device)
    gpu_s = time.perf_counter() - t0
    ws = api._init_file2(None, h, None, None, True, True, 0.005, 0.01, 1, False, device)
    flag = np.isin(h.snp_id, ws["snp_id"])
    chrom, pos = h.snp_chromosome[flag], h.snp_position[flag]
    t0 = time.perf_counter()
    same = True
    for ch in range(1, 23):
        sel = chrom == ch
        M = int(sel.sum())
        g = unpack_2bit_rows(ws["packed"][sel], ws["n_samp"])
        W = ld_prune_ref.band_width(M, 0, pos[sel], 500000, INT_MAX)
        r = ld_prune_ref.prune(M, 0, pos[sel], 500000, INT_MAX, 0.2, ld_prune_ref.ld_from_geno(g, "composite", W))
        same &= bool(np.array_equal(ws["snp_id"][sel][r.keep], res["chr%d" % ch]))
    cpu_s = time.perf_counter() - t0
    return {"snps": int(flag.sum()), "kept": int(sum(len(v) for v in res.values())), "gpu_call_s": gpu_s,
            "cpu_restatement_s": cpu_s, "kept_sets_equal": same}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-samp", type=int, default=100000)
    ap.add_argument("--n-chrom", type=int, default=4)
    ap.add_argument("--snps-per-chrom", type=int, default=65536)
    ap.add_argument("--slide-max-bp", type=int, default=500000)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--probe-seconds", type=float, default=2.0)
    ap.add_argument("--hapmap", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    from snprelate_amd import _lib

    N, M, C = a.n_samp, a.snps_per_chrom, a.n_chrom
    rb = (N + 3) // 4
    rbp = (rb + 31) // 32 * 32
    torch.cuda.set_device(a.device)
    geno = torch.empty(C * M * rb, dtype=torch.uint8, device="cuda")
    for i0 in range(0, C * M, 8192):
        n = min(8192, C * M - i0)
        _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, n, seed=2024, missing=a.missing, spectrum=4, device=a.device)
    torch.cuda.synchronize()
    pos = [positions(M, 100 + c) for c in range(C)]

    def run(c):
        t0 = time.perf_counter()
        keep, info = _lib.ld_prune(geno.data_ptr() + c * M * rb, N, pos[c], 0, a.slide_max_bp, INT_MAX, a.threshold, _lib.LD_COMPOSITE,
                                   fmt=_lib.GENO_PACKED2, n_snp=M, device=a.device)
        return time.perf_counter() - t0, keep, info

    probe_before, _ = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    run(0)                                                   # warm-up
    chroms = []
    for c in range(C):
        wall, keep, info = run(c)
        chroms.append(dict(info, wall_ms=wall * 1e3, kept_fraction=float(keep.mean())))
    probe_after, mhz = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    sustained = 0.5 * (probe_before + probe_after)
    tot = {k: sum(c[k] for c in chroms) for k in ("band_pairs", "table_tiles", "ms_stage", "ms_tables", "ms_bits", "ms_copy",
                                                   "ms_scan", "wall_ms")}
    flop = tot["table_tiles"] * 4 * (rbp // 32) * 2 * 9 * MFMA_FLOP
    rec = {"tool": "ld_prune_bench", "N": N, "chromosomes": C, "snps": C * M, "slide_max_bp": a.slide_max_bp,
           "threshold": a.threshold, "missing": a.missing, "per_chrom": chroms, "totals": tot,
           "table_pair_sample_genotypes_per_s": tot["band_pairs"] * N / (tot["ms_tables"] * 1e-3),
           "call_pair_sample_genotypes_per_s": tot["band_pairs"] * N / (tot["wall_ms"] * 1e-3),
           "table_kernel_tflops_executed": flop / (tot["ms_tables"] * 1e-3) / 1e12,
           "mfma_fp4_sustained_tflops": sustained, "mfma_fp4_probe_tflops": [probe_before, probe_after], "implied_mhz": mhz,
           "share_of_wall": {k: tot[k] / tot["wall_ms"] for k in ("ms_stage", "ms_tables", "ms_bits", "ms_copy", "ms_scan")}}
    rec["fraction_of_sustained"] = rec["table_kernel_tflops_executed"] / sustained if sustained > 0 else None
    if a.hapmap:
        rec["hapmap"] = hapmap_run(a.device)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
