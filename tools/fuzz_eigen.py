#!/usr/bin/env python3
"""Randomised sweep of the top-k eigen solver (GPU): random sample counts (not multiples of anything), SNP counts, missing rates,
row-panel splits, matrix kinds (PCA covariance, GCTA GRM / EIGMIX matrix finalised in place) and k; the block-Krylov solver
behind snpgpu_panels_topk_eigen against numpy's eigh (LAPACK) of the device's OWN gathered matrix: eigenvalues, residuals.
The cases come from tests/eigen_spectra.py (fuzz_case), which tests/test_gpu_eigen_spectra.py runs twelve of with fixed seeds.
    tools/fuzz_eigen.py [n_cases] [seed]"""
import sys

import numpy as np

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path[:0] = [ROOT, ROOT + "/tests"]
import eigen_spectra as E  # noqa: E402
from oracle.synth import synth_geno  # noqa: E402
from snprelate_amd import _lib  # noqa: E402
from snprelate_amd.dist import panel_rows  # noqa: E402
from snprelate_amd.eigen import PanelOperator, topk_eigen  # noqa: E402

import torch  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
dev = torch.device("cuda", 0)
bad = 0
for case in range(cases):
    c = E.fuzz_case(rng, synth_geno)
    n, L, k, kind, world = c["n"], c["L"], c["k"], c["kind"], c["world"]
    panels, rows = E.open_panels(_lib, kind, c["g"], panel_rows(n, world) if world > 1 else None, c["blk"])
    full = E.gathered(kind, panels, rows, n)          # the device's own matrix; GRM / EIGMIX contexts finalised in place
    ok = np.isfinite(full).all()
    err = res = float("nan")
    if ok:
        op = PanelOperator(panels, n, dev, normalize=(kind == "PCA_COV"))
        w, v, info = topk_eigen(op, k)
        w, v = w.cpu().numpy(), v.cpu().numpy()
        wr = np.linalg.eigvalsh(full)[::-1][:k]
        err = float(np.max(np.abs(w - wr) / np.abs(wr[0])))
        res = float(np.max(np.linalg.norm(full @ v - v * w, axis=0) / np.abs(w)))
        ok = err < E.EIGENVALUE_BOUND and res < E.RESIDUAL_BOUND
    for a in panels:
        a.close()
    print("case %2d %-8s n=%4d L=%4d k=%2d miss=%.2f panels=%d  eigenvalues %.1e residual %.1e fp32 products %d of %d  %s" %
          (case, kind, n, L, k, c["miss"], world, err, res, info["matmuls_fp32"] if ok or err == err else -1, info["matmuls"] if ok or err == err else -1,
           "ok" if ok else "FAILED"), flush=True)
    bad += not ok
print("FAILED cases: %d" % bad)
