#!/usr/bin/env python
"""snpgdsMDS on one GPU: one JSON line (profiles/mds_bench.json).  Runs on an MI355X; no test runs it.

The distance matrix is made on the device with torch from random points in 8 dimensions, at n = 20 000 and 50 000, and at 100 000
where the device holds two such matrices (the copy yardstick) beside the solver's work.  The distances are city-block ones,
sum_d |x_id - x_jd| -- what an IBS distance is, sum |g - g'| -- so that B has negative eigenvalues and more than 16 positive ones;
Euclidean distances of 8-dimensional points give B the rank 8, and a call for 16 eigenvalues is then refused by design.  They are
accumulated dimension by dimension in place: |a - b| = |b - a| to the bit, so the matrix is exactly symmetric, as the scan demands.

Per size, for b = 16 and 48 vectors: one operator product q -> B q (snpgpu_mds_apply on the device matrix; the time is the HIP
events around the product's four kernels, best of --reps), its largest deviation from the same product made by torch in fp64, and
two yardsticks from the same run: a device-to-device copy of the matrix bytes, and snpgpu_pca_panel_matmul on a PCA_COV context of
the same n and b (the existing fp64 product, which reads one triangle of its panel and adds with atomics).  Then the whole
snpgpu_mds call at k = 2 and k = 16 (wall time and snpgpu_mds_stats).  A call whose worst case -- 60 restart cycles of 24 products
at the measured product time -- exceeds --max-solve-s is not started; the line says so."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIMS = 8


def make_matrix(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, DIMS), dtype=torch.float64, device="cuda", generator=g)
    d = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    rows = max(1, (1 << 28) // n)
    for r0 in range(0, n, rows):
        blk = d[r0:r0 + rows]
        for k in range(DIMS):
            blk += (x[r0:r0 + rows, k, None] - x[None, :, k]).abs_()
    return d


def torch_product(torch, d, q):
    """B q in torch, fp64, D o D made in row blocks"""
    n = d.shape[0]
    w = q - q.mean(dim=1, keepdim=True)
    z = torch.zeros_like(q)
    rows = max(1, (1 << 28) // n)
    for r0 in range(0, n, rows):
        blk = d[r0:r0 + rows]
        z += w[:, r0:r0 + rows] @ (blk * blk)
    return -0.5 * (z - z.mean(dim=1, keepdim=True))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 50000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-solve-s", type=float, default=150.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mds_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib

    out = {"tool": "mds_bench", "source_stamp": bench.source_stamp(), "device": torch.cuda.get_device_name(0), "dims": DIMS,
           "distance": "city-block", "reps": a.reps, "sizes": []}
    for n in a.sizes:
        torch.cuda.empty_cache()
        free, _total = torch.cuda.mem_get_info()
        nn = 8 * n * n
        if 2 * nn + (16 << 30) > free:
            out["sizes"].append({"n": n, "skipped": "two matrices of %.0f GB and the solver's work do not fit %.0f GB free" % (nn / 1e9, free / 1e9)})
            continue
        d = make_matrix(torch, n, 1000 + n)
        torch.cuda.synchronize()
        rec = {"n": n, "matrix_bytes": nn, "products": [], "calls": []}
        # yardstick 1: a device-to-device copy of the matrix bytes
        d2 = torch.empty_like(d)
        best = float("inf")
        for _ in range(a.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            d2.copy_(d)
            t1.record()
            t1.synchronize()
            best = min(best, t0.elapsed_time(t1))
        del d2
        torch.cuda.empty_cache()
        rec.update(copy_ms=best, copy_TBps=nn / best / 1e9)
        # yardstick 2: the fp64 panel product of a PCA_COV context of the same n
        panel = {}
        with _lib.Accumulator(_lib.PCA_COV, n, max_block_snps=1024) as acc:
            g = torch.empty((1024, (n + 3) // 4), dtype=torch.uint8, device="cuda")
            _lib.synth_block(g.data_ptr(), n, 0, 1024, 20240601, missing=0.02)
            acc.feed_device(g.data_ptr(), 1024)
            acc.sync()
            panel_bytes = 8 * acc.slab_size()
            for b in (16, 48):
                q = torch.randn((b, n), dtype=torch.float64, device="cuda")
                y = torch.zeros_like(q)
                best = float("inf")
                for _ in range(a.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    acc.pca_panel_matmul(1.0, q.data_ptr(), b, y.data_ptr())
                    torch.cuda.synchronize()
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                panel[b] = best
            del g
        torch.cuda.empty_cache()
        rec["panel_bytes"] = panel_bytes
        # the operator
        for b in (16, 48):
            q = np.random.default_rng(b).standard_normal((b, n))
            best = float("inf")
            for _ in range(a.reps + 1):
                y = _lib.mds_apply(d.data_ptr(), q, n=n)
                best = min(best, _lib.mds_stats()["product_ms"])
            y_t = torch_product(torch, d, torch.from_numpy(q).cuda()).cpu().numpy()
            rec["products"].append({
                "b": b, "mds_ms": best, "mds_TBps": nn / best / 1e9, "panel_ms": panel[b], "panel_TBps": panel_bytes / panel[b] / 1e9,
                "mds_over_panel_per_byte": (best / nn) / (panel[b] / panel_bytes), "mds_over_copy": best / rec["copy_ms"],
                "max_abs_dev_from_torch_over_max_abs": float(np.abs(y - y_t).max() / np.abs(y_t).max())})
            rec["scan_ms"] = _lib.mds_stats()["scan_ms"]
        worst_s = 60 * 24 * rec["products"][-1]["mds_ms"] / 1e3
        for k in (2, 16):
            if worst_s > a.max_solve_s:
                rec["calls"].append({"k": k, "skipped": "worst case %.0f s of products exceeds --max-solve-s %.0f" % (worst_s, a.max_solve_s)})
                continue
            t0 = time.perf_counter()
            try:
                r = _lib.mds(d.data_ptr(), k, n=n)
                call = {"k": k, "wall_ms": (time.perf_counter() - t0) * 1e3, "eigval_first": float(r["eigval"][0]),
                        "eigval_last": float(r["eigval"][-1]), "trace": r["trace"]}
            except _lib.SnpGpuError as e:
                call = {"k": k, "wall_ms": (time.perf_counter() - t0) * 1e3, "refused": str(e)[:200]}
            call.update(_lib.mds_stats())
            rec["calls"].append(call)
        out["sizes"].append(rec)
        print(json.dumps(rec), flush=True)
        del d
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
