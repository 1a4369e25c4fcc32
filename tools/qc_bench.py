#!/usr/bin/env python
"""snpgdsSampMissRate / snpgdsHWE / snpgdsIndInb on one GPU: one JSON line.

Device-resident synthetic genotypes (snpgpu_synth_block), N = 100 000 samples, one 65 536-SNP block, 2 % missing calls.  From HIP
events around the launches (snpgpu_qc_stats): the counter kernel and the moment kernel (table kernel included) as genotype bytes
per second and as a fraction of what a device-to-device copy of the same block reaches IN THE SAME RUN; the MLE kernel and the HWE
kernel as fp64 operations per second (counted from the source: 16 additions / multiplications and one division per SNP, sample and
sweep of the MLE; 9 and 2 per recurrence step and pass of the test, two passes) beside snpgpu_diag_fp64_rate of the same run, which
counts an FMA as two.  Last, whole API calls on the HapMap fixture against the numpy restatements of tests/ on the same data."""
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
    ap.add_argument("--mle-samples", type=int, default=100000, help="samples of the MLE case (its words take 4 bytes per 16 SNPs and sample)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import hwe_ref as H
    import inb_ref as R
    from snprelate_amd import _lib, api
    from snprelate_amd.gds import open_gds, unpack_2bit_rows

    torch.cuda.set_device(a.device)
    N, B = a.samples, a.snps
    rb = (N + 3) // 4
    geno = torch.empty(B * rb, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(geno)
    _lib.synth_block(geno.data_ptr(), N, 0, B, seed=78, missing=0.02, spectrum=0, device=a.device)
    torch.cuda.synchronize()
    ptr = int(geno.data_ptr())

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
    fp64 = _lib.diag_fp64_rate(1.0, a.device)
    out = {"tool": "qc_bench", "N": N, "snps": B, "missing": 0.02, "copy_ms_median": copies[len(copies) // 2],
           "copy_bytes_per_s": copy_rate, "fp64_tflops_measured": fp64}

    def median_stat(fn, key):
        fn()
        v = []
        for _ in range(a.reps):
            fn()
            v.append(_lib.qc_stats()[key])
        v.sort()
        return v[len(v) // 2], v

    med, allv = median_stat(lambda: _lib.geno_counts(ptr, N, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device), "count_ms")
    out["counter"] = {"ms_median": med, "ms_all": allv, "genotype_bytes_per_s": nbytes / (med * 1e-3),
                      "fraction_of_copy_rate": nbytes / (med * 1e-3) / copy_rate}
    for method in ("mom.weir", "gcta1"):
        med, allv = median_stat(lambda: _lib.ind_inb(ptr, N, method, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device), "mom_ms")
        out["moment_" + method] = {"ms_median": med, "ms_all": allv, "genotype_bytes_per_s": nbytes / (med * 1e-3),
                                   "fraction_of_copy_rate": nbytes / (med * 1e-3) / copy_rate}
    med, allv = median_stat(lambda: _lib.hwe(ptr, N, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device), "hwe_ms")
    cnt, _ = _lib.geno_counts(ptr, N, fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device, want_samp=False)
    steps = float(((2 * np.minimum(cnt[:, 0], cnt[:, 2]) + cnt[:, 1]) // 2).sum())
    out["hwe"] = {"ms_median": med, "ms_all": allv, "recurrence_steps": steps, "fp64_ops_per_s": 2 * 11 * steps / (med * 1e-3),
                  "fraction_of_fp64_rate": 2 * 11 * steps / (med * 1e-3) / (fp64 * 1e12)}

    n_mle = min(a.mle_samples, N)
    if n_mle == N:
        mptr = ptr
    else:
        small = torch.empty(B * ((n_mle + 3) // 4), dtype=torch.uint8, device="cuda")
        _lib.synth_block(small.data_ptr(), n_mle, 0, B, seed=78, missing=0.02, spectrum=0, device=a.device)
        torch.cuda.synchronize()
        mptr = int(small.data_ptr())
    _, nit, _ = _lib.ind_inb(mptr, n_mle, "mle", fmt=_lib.GENO_PACKED2, n_snp=B, device=a.device)
    st = _lib.qc_stats()
    snp_steps = 16.0 * st["mle_lane_steps_useful"]                  # a lane-step is one word of 16 SNPs
    out["mle"] = {"samples": n_mle, "ms": st["mle_ms"], "niter_mean": float(nit[nit > 0].mean()), "niter_max": int(nit.max()),
                  "last_stride_fill": st["mle_lane_steps_useful"] / max(st["mle_lane_steps_issued"], 1),
                  "fp64_ops_per_s": 17 * snp_steps / (st["mle_ms"] * 1e-3),
                  "fraction_of_fp64_rate": 17 * snp_steps / (st["mle_ms"] * 1e-3) / (fp64 * 1e12)}
    out["copy_ms_after"] = sorted(copy_ms() for _ in range(a.reps))

    hm = open_gds(os.path.join(ROOT, "tests", "golden", "hapmap_geno.gds"))
    g = unpack_2bit_rows(hm.packed, hm.n_samp)
    whole = {}

    def clock(fn):
        fn()
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    _, whole["snpgdsSampMissRate_ms"] = clock(lambda: api.snpgdsSampMissRate(hm, device=a.device))
    t0 = time.perf_counter()
    (g > 2).sum(0) / float(g.shape[0])
    whole["numpy_missrate_ms"] = (time.perf_counter() - t0) * 1e3
    _, whole["snpgdsHWE_ms"] = clock(lambda: api.snpgdsHWE(hm, device=a.device))
    t0 = time.perf_counter()
    H.hwe_ref(np.stack([(g == k).sum(1) for k in range(3)], 1))
    whole["hwe_ref_ms"] = (time.perf_counter() - t0) * 1e3
    for method in ("mom.weir", "mle"):
        r, whole["snpgdsIndInb_%s_ms" % method] = clock(lambda: api.snpgdsIndInb(hm, method=method, verbose=False, device=a.device))
        gs = g[np.isin(hm.snp_id, r["snp_id"])]
        t0 = time.perf_counter()
        if method == "mle":
            p = R.snp_freq(gs)
            for j in range(gs.shape[1]):
                R.mle_ref(gs[:, j], p, float(np.finfo(float).eps ** 0.75))
        else:
            R.ind_inb_moment_ref(gs, method)
        whole["inb_ref_%s_ms" % method] = (time.perf_counter() - t0) * 1e3
    out["hapmap"] = whole
    print(json.dumps(out))


if __name__ == "__main__":
    main()
