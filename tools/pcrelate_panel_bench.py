#!/usr/bin/env python
"""PC-Relate row panels on one GPU: one JSON line (profiles/pcrelate_panel_bench.json).  Runs on an MI355X; no test runs it.

Seeded synthetic 2-bit device rows (snpgpu_synth_block, --missing missing calls) and --pcs random principal components, as
tools/pcrelate_bench.py.  Three measurements:
  1. n = --n: the panel [0, --rows) against the full object in the same run, --snps SNPs each.  The product phase's fp64 rate of
     both counts the 128 x 128 tiles that were executed (2 * 128 * 128 * m flop each); the panel's CD job (DC's other half, stored
     transposed) and its strips of diagonal tiles are timed on their own.  The CD job against the DC launch's share of the rest is
     where a slow transposed epilogue would show.
  2. n = --big-n: one panel of --rows rows, --big-snps SNPs: the phases, the bytes resident, the SNPs of an internal block -- under
     the default staging and under SNPGPU_PCR_STAGE_BYTES of 4 GiB (more SNPs per C += acc).
  3. snpgpu_pcr_select on that panel at the cutoffs 2^-5.5, NaN (every pair; at most --capacity pairs are stored) and above every
     kinship: count pass, scan and write pass, beside a device-to-device copy of the bytes the count pass reads (the RR and SS
     slabs) in the same run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE = 128


def tiles(n, r0, r1, ibd=True, panel=True):
    """128 x 128 tiles one SNP block executes: (in the slabs without CD, in the CD job, in the strips)"""
    nt = (n + TILE - 1) // TILE
    t0, t1 = r0 // TILE, (r1 + TILE - 1) // TILE
    tri = sum(nt - i for i in range(t0, t1))
    full = (t1 - t0) * (nt - t0)
    slabs = (9 * tri + full) if ibd else 3 * tri
    return slabs, ((t1 - t0) * (nt - t1) if panel and ibd else 0), (2 * nt if panel else 0)       # CD: the columns right of the block


def run(obj, n, m_all, feed, rows, missing, _lib, torch):
    t0 = time.perf_counter()
    for s0 in range(0, m_all, feed):
        nb = min(feed, m_all - s0)
        _lib.synth_block(rows.data_ptr(), n, s0, nb, 20240601, missing=missing)
        torch.cuda.synchronize()
        obj.feed(int(rows.data_ptr()), fmt=_lib.GENO_PACKED2, n_snp=nb)
    rec = {"feed_wall_s": time.perf_counter() - t0}
    rec.update(obj.stats())
    rec.update(obj.panel_stats())
    return rec


def rates(rec, n, r0, r1, m_all, panel):
    slabs, cd, strips = tiles(n, r0, r1, True, panel)
    flop = 2.0 * TILE * TILE * m_all
    rec["tiles_per_block"] = {"slabs": slabs, "cd": cd, "strips": strips}
    rec["product_tflops"] = (slabs + cd + strips) * flop / (rec["product_ms"] * 1e-3) / 1e12
    rest = rec["product_ms"] - rec["cd_ms"] - rec["strip_ms"]
    rec["slab_tflops"] = slabs * flop / (rest * 1e-3) / 1e12
    if cd:
        rec["cd_tflops"] = cd * flop / (rec["cd_ms"] * 1e-3) / 1e12
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=8192)
    ap.add_argument("--big-n", type=int, default=100000)
    ap.add_argument("--big-snps", type=int, default=8192)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--pcs", type=int, default=4)
    ap.add_argument("--feed", type=int, default=8192, help="SNPs per feed")
    ap.add_argument("--capacity", type=int, default=1 << 25, help="pairs stored at most by one selection")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcrelate_panel_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib

    out = {"tool": "pcrelate_panel_bench", "source_stamp": bench.source_stamp(), "device": torch.cuda.get_device_name(0), "missing": a.missing,
           "pcs": a.pcs, "feed_snps": a.feed, "rows": a.rows}

    # 1. the panel against the full object
    n = a.n
    pcs = np.random.default_rng(1).normal(0, 1 / np.sqrt(n), (n, a.pcs))
    rows = torch.empty((a.feed, (n + 3) // 4), dtype=torch.uint8, device="cuda")
    with _lib.PCRelate(n, pcs=pcs) as p:
        full = rates(run(p, n, a.snps, a.feed, rows, a.missing, _lib, torch), n, 0, n, a.snps, False)
    with _lib.PCRelatePanel(n, rows=(0, a.rows), pcs=pcs) as p:
        panel = rates(run(p, n, a.snps, a.feed, rows, a.missing, _lib, torch), n, 0, a.rows, a.snps, True)
    out["panel_vs_full"] = {"n": n, "snps": a.snps, "full": full, "panel": panel,
                            "panel_over_full_product_rate": panel["product_tflops"] / full["product_tflops"],
                            "cd_over_slab_rate": panel["cd_tflops"] / panel["slab_tflops"]}
    print(json.dumps(out["panel_vs_full"]), flush=True)
    del rows

    # 2. one panel at the headline size, under two staging sizes;  3. the selection on it
    n = a.big_n
    pcs = np.random.default_rng(1).normal(0, 1 / np.sqrt(n), (n, a.pcs))
    rows = torch.empty((a.feed, (n + 3) // 4), dtype=torch.uint8, device="cuda")
    big = {"n": n, "snps": a.big_snps, "runs": []}
    for stage in (None, 4 << 30):
        if stage is None:
            os.environ.pop("SNPGPU_PCR_STAGE_BYTES", None)
        else:
            os.environ["SNPGPU_PCR_STAGE_BYTES"] = str(stage)
        with _lib.PCRelatePanel(n, rows=(0, a.rows), pcs=pcs) as p:
            rec = rates(run(p, n, a.big_snps, a.feed, rows, a.missing, _lib, torch), n, 0, a.rows, a.big_snps, True)
            rec["stage_bytes"] = stage if stage else "default"
            big["runs"].append(rec)
            print(json.dumps(rec), flush=True)
            if stage is not None:
                continue
            p.select(10.0, capacity=0)                                      # (the first launch of the selection's kernels)
            sel = []
            for name, cut in (("2^-5.5", 2 ** -5.5), ("nan", float("nan")), ("above", 10.0)):
                t0 = time.perf_counter()
                s = p.select(cut, capacity=a.capacity)
                r = {"cutoff": name, "n_found": s["n_found"], "stored": len(s["idx1"]), "wall_s": time.perf_counter() - t0}
                r.update(_lib.pcr_select_stats())
                sel.append(r)
                del s
            read = 2 * 8 * a.rows * n                                       # the count pass reads the RR and SS slabs
            src = torch.empty(read // 8, dtype=torch.float64, device="cuda")
            dst = torch.empty_like(src)
            best = float("inf")
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
            del src, dst
            big["select"] = {"runs": sel, "capacity": a.capacity, "count_pass_read_bytes": read, "d2d_copy_of_those_bytes_ms": best}
            print(json.dumps(big["select"]), flush=True)
    os.environ.pop("SNPGPU_PCR_STAGE_BYTES", None)
    out["big_panel"] = big
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
