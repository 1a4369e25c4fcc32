#!/usr/bin/env python
"""PC-Relate on one GPU: one JSON line (profiles/pcrelate_bench.json).  Runs on an MI355X; no test runs it.

The seeded synthetic data set (snpgpu_synth_block: --n samples x --snps SNPs, --missing missing calls) is made on the device feed
block by feed block and fed as 2-bit device rows to a snpgpu_pcr object with --pcs random principal components, once with
SNPGPU_PCR_IBD (eight planes) and once without (three).  Per setting: the phases of snpgpu_pcr_stats (HIP events), the wall time
of the feeds and of the result, and the product kernel's fp64 rate -- 2 n^2 m flops per full plane, half that for a plane of
which the tiles I <= J are computed: 5.5 plane equivalents with the flag (RR, SS, NS, DD, CC triangular, DC full, IBS0 and K0D
two triangular launches each), 1.5 without.  Beside it two yardsticks from the same run: the sustained v_mfma_f64_16x16x4_f64 rate
of tools/ubench/mfma_f64_rate (a register-only stream, run as a child process before the device is used here; "unmeasured" when
the binary has not been built) and the same X^T X of one internal block by torch.matmul in fp64."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def mfma_f64_probe():
    exe = os.path.join(ROOT, "tools", "ubench", "mfma_f64_rate")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    rates = [float(x) for x in re.findall(r"([0-9.]+) TFLOP/s", out)]
    return max(rates) if rates else None


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=65536)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--pcs", type=int, default=4)
    ap.add_argument("--feed", type=int, default=8192, help="SNPs per feed")
    ap.add_argument("--no-result", action="store_true", help="leave out the finaliser and the copies of its n x n results")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcrelate_bench.json"))
    a = ap.parse_args()

    probe = mfma_f64_probe()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib

    n, m_all = a.n, a.snps
    pcs = np.random.default_rng(1).normal(0, 1 / np.sqrt(n), (n, a.pcs))
    rows = torch.empty((a.feed, (n + 3) // 4), dtype=torch.uint8, device="cuda")
    out = {"tool": "pcrelate_bench", "source_stamp": bench.source_stamp(), "device": torch.cuda.get_device_name(0), "n": n, "snps": m_all,
           "missing": a.missing, "pcs": a.pcs, "feed_snps": a.feed,
           "mfma_f64_16x16x4_sustained_tflops": probe if probe is not None else "unmeasured", "runs": []}
    for ibd in (True, False):
        with _lib.PCRelate(n, pcs=pcs if a.pcs else None, ibd=ibd) as p:
            t0 = time.perf_counter()
            for s0 in range(0, m_all, a.feed):
                nb = min(a.feed, m_all - s0)
                _lib.synth_block(rows.data_ptr(), n, s0, nb, 20240601, missing=a.missing)
                torch.cuda.synchronize()
                p.feed(int(rows.data_ptr()), fmt=_lib.GENO_PACKED2, n_snp=nb)
            feed_s = time.perf_counter() - t0
            st = p.stats()
            rec = {"ibd": ibd, "feed_wall_s": feed_s}
            rec.update(st)
            planes = 5.5 if ibd else 1.5
            rec["product_flop"] = 2.0 * n * n * m_all * planes
            rec["product_tflops"] = rec["product_flop"] / (st["product_ms"] * 1e-3) / 1e12
            if probe is not None:
                rec["product_share_of_sustained_mfma"] = rec["product_tflops"] / probe
            if not a.no_result:
                t0 = time.perf_counter()
                r = p.result()
                rec["result_wall_s"] = time.perf_counter() - t0
                rec["final_ms"] = p.stats()["final_ms"]
                k = r["kinship"]
                off = k[np.triu_indices(min(n, 2000), 1)]
                rec["kinship_offdiag_mean_first2000"] = float(np.nanmean(off))
                rec["kinship_offdiag_sd_first2000"] = float(np.nanstd(off))
                rec["inbreed_mean"] = float(np.nanmean(r["inbreed"]))
                del r, k
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    # yardstick: X^T X of one internal block by torch in fp64
    mb = out["runs"][0]["block_snps"]
    x = torch.randn((mb, n), dtype=torch.float64, device="cuda")
    best = float("inf")
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        c = x.T @ x
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1))
    del c, x
    out["torch_fp64_xtx"] = {"block_snps": mb, "ms": best, "tflops": 2.0 * n * n * mb / (best * 1e-3) / 1e12}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
