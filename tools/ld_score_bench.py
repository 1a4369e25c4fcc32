#!/usr/bin/env python
"""snpgdsLDScore on one GPU: one JSON line (profiles/ld_score_bench.json).

N samples generated on the device (snpgpu_synth_block, spectrum 4 = 48-SNP LD blocks, 2 % missing), one block of L SNPs in device
memory, scored by snpgpu_ld_score with the methods corr and composite under two windows: 250 SNPs (no positions) and 500 kb on
uneven positions (mean gap about 3 kb, 30 % of the gaps 50 times shorter: dense stretches, as tools/ld_prune_bench.py).  Per
configuration: the band width W, the pair counts, the best whole-call wall time of the timed repeats and that call's phase times
(snpgpu_ld_score_info: HIP events for staging, the table kernel, the terms kernel, the fold kernel and the result copies).

Beside them, in the same run: snpgpu_ld_create -> feed -> result (snpgdsLDMat's slide x L matrix to the host) at slide 250 for
both methods, the ratio of the whole-call times at the 250-SNP window, and what a register-only stream of the table kernel's MFMA
sustains on this device (snpgpu_diag_mfma_rate, mode 3) before and after."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INT_MAX = 2 ** 31 - 1
METHODS = ("composite", "r", "dprime", "corr")


def positions(M, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    gaps = rng.exponential(3000, M).astype(np.int64)
    gaps[rng.random(M) < 0.3] //= 50
    return np.cumsum(gaps).astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-samp", type=int, default=100000)
    ap.add_argument("--n-snp", type=int, default=65536)
    ap.add_argument("--slide", type=int, default=250)
    ap.add_argument("--slide-max-bp", type=int, default=500000)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--methods", default="corr,composite")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls after one warm-up call; the best is reported")
    ap.add_argument("--probe-seconds", type=float, default=2.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from snprelate_amd import _lib

    N, L = a.n_samp, a.n_snp
    rb = (N + 3) // 4
    torch.cuda.set_device(a.device)
    geno = torch.empty(L * rb, dtype=torch.uint8, device="cuda")
    for i0 in range(0, L, 8192):
        _lib.synth_block(geno.data_ptr() + i0 * rb, N, i0, min(8192, L - i0), seed=2024, missing=a.missing, spectrum=4, device=a.device)
    torch.cuda.synchronize()
    pos = positions(L, 100)
    windows = {"%d_snps" % a.slide: (None, INT_MAX, a.slide), "%d_bp" % a.slide_max_bp: (pos, a.slide_max_bp, INT_MAX)}

    def score_call(method, window):
        p, bp, n = windows[window]
        t0 = time.perf_counter()
        score, n_valid, n_window, info = _lib.ld_score(geno.data_ptr(), N, p, bp, n, METHODS.index(method) + 1, True, True,
                                                       fmt=_lib.GENO_PACKED2, n_snp=L, device=a.device)
        return time.perf_counter() - t0, score, n_valid, info

    def ldmat_call(method):
        t0 = time.perf_counter()
        with _lib.LDMatrix(N, L, METHODS.index(method) + 1, a.slide, False, device=a.device) as ld:
            ld.set_timing(True)
            ld.feed_device(geno.data_ptr(), L)
            out = ld.result()
            wall = time.perf_counter() - t0
            tm = [ld.get_timing(w)[0] for w in range(3)]
        return wall, tm, out

    probe_before, _ = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    configs, ldmat = [], {}
    for method in a.methods.split(","):
        for window in windows:
            score_call(method, window)                                   # warm-up
            best = min((score_call(method, window) for _ in range(max(1, a.repeats))), key=lambda r: r[0])
            wall, score, n_valid, info = best
            configs.append(dict(info, method=method, window=window, wall_ms=wall * 1e3, mean_score=float(np.mean(score)),
                                mean_valid_partners=float(n_valid.mean()), result_bytes=int(score.nbytes + 2 * n_valid.nbytes)))
        ldmat_call(method)                                               # warm-up
        wall, tm, out = min((ldmat_call(method) for _ in range(max(1, a.repeats))), key=lambda r: r[0])
        ldmat[method] = {"slide": a.slide, "wall_ms": wall * 1e3, "count_kernel_ms": tm[0], "final_kernel_ms": tm[1],
                         "result_copy_ms": tm[2], "result_bytes": int(out.nbytes)}
    probe_after, mhz = _lib.diag_mfma_rate(_lib.DIAG_FP4, a.probe_seconds, a.device)
    ratio = {c["method"]: c["wall_ms"] / ldmat[c["method"]]["wall_ms"] for c in configs if c["window"] == "%d_snps" % a.slide}
    rec = {"tool": "ld_score_bench", "N": N, "L": L, "missing": a.missing, "repeats": a.repeats, "configs": configs,
           "ld_create_feed_result": ldmat, "score_call_over_ldmat_call_wall": ratio,
           "mfma_fp4_probe_tflops": [probe_before, probe_after], "implied_mhz": mhz}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
