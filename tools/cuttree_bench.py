#!/usr/bin/env python
"""snpgdsHCluster / snpgdsCutTree on one GPU: one JSON line.

Synthetic three-population genotypes (Balding-Nichols frequencies, drawn on the host) through snpgdsDiss's kernel give the
dissimilarity matrix; snpgpu_hclust_average clusters it on the host; snpgpu_dist_perm runs the permutation test.  Reported per
size: the host clustering time, the phases of snpgpu_tree_stats (gather / row-sum pass, permutation kernels, their launches), matrix
elements gathered per second beside a device-to-device copy of the matrix in the same run (elements per second), the whole call,
and at the smallest size the sequential procedure of tests/tree_ref.py on the same matrix with fewer permutations, scaled."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def three_populations(n, n_snp, seed, fst=0.05):
    import numpy as np
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(0.1, 0.9, n_snp)
    a = p0 * (1 - fst) / fst
    b = (1 - p0) * (1 - fst) / fst
    pop = rng.integers(0, 3, n)
    freq = rng.beta(a[None, :], b[None, :], (3, n_snp))
    return rng.binomial(2, freq[pop].T).astype(np.uint8), pop


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 10000])
    ap.add_argument("--snps", type=int, default=2048)
    ap.add_argument("--n-perm", type=int, default=5000)
    ap.add_argument("--cpu-perm", type=int, default=50, help="permutations of the sequential CPU procedure at the smallest size (0: skip)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import tree_ref as T
    from snprelate_amd import _lib

    torch.cuda.set_device(a.device)
    out = {"tool": "cuttree_bench", "n_perm": a.n_perm, "snps": a.snps, "cases": []}
    for k, n in enumerate(a.sizes):
        g, pop = three_populations(n, a.snps, seed=n)
        with _lib.Accumulator(_lib.DISS, n, device=a.device) as acc:
            acc.feed(g)
            d = acc.diss()
        t0 = time.perf_counter()
        merge, height, order = _lib.hclust_average(d)
        t_hc = time.perf_counter() - t0
        dd = torch.from_numpy(d).cuda()
        other = torch.empty_like(dd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        other.copy_(dd)
        e0.record()
        other.copy_(dd)
        e1.record()
        torch.cuda.synchronize()
        copy_ms = e0.elapsed_time(e1)
        del other
        t0 = time.perf_counter()
        rv = _lib.dist_perm(int(dd.data_ptr()), merge, n_perm=a.n_perm, z_threshold=15.0, seed=1, device=a.device, n=n)
        t_call = time.perf_counter() - t0
        st = _lib.tree_stats()
        ns1 = np.minimum(rv["n1"], rv["n2"])
        groups = len(set(rv["group"].tolist()))
        case = {"n": n, "hclust_s": t_hc, "call_s": t_call, "stats": st, "copy_ms": copy_ms,
                "copy_elements_per_s": n * n / (copy_ms * 1e-3), "gathered_per_s": st["gathered"] / (st["perm_ms"] * 1e-3),
                "groups": groups, "z_max": float(rv["z"].max()), "nsub1_max": int(ns1.max()), "nsub1_eq_1": int((ns1 == 1).sum()),
                "tree_depth_sum": int((rv["n1"] + rv["n2"]).sum())}
        if k == 0 and a.cpu_perm >= 50:
            t0 = time.perf_counter()
            ref = T.dist_perm_sequential(d, merge, a.cpu_perm, 15.0, np.random.default_rng(1))
            t_cpu = time.perf_counter() - t0
            case["cpu_sequential_numpy_s_scaled"] = t_cpu * a.n_perm / a.cpu_perm
            case["cpu_groups_equal"] = bool(np.array_equal(ref["group"], rv["group"]))
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
