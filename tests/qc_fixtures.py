"""Inputs shared by tests/test_cpu_qc.py and tests/test_gpu_qc.py, and the two figures of the MLE comparison.

MLE_F_TOL and MLE_FIRM were MEASURED ON THE CPU from the restatement alone (tests/inb_ref.py), before any GPU run: for every
sample of every fixture below (HapMap, the synthetic set with given and with estimated frequencies, the slow sample, the
never-stopping set) the iteration was evaluated with its sums over the SNPs taken sequentially, reversed, pairwise
and in np.longdouble, and the largest differences from the sequential run over all iterations were taken
(test_cpu_qc.py::test_mle_spread_and_firmness re-measures them and checks the figures below against 10 x the spread):

    largest |F_k(order) - F_k(sequential)|                      : 1.4e-14 (synthetic, estimated frequencies)
    largest | |dLogLik_k|(order) - |dLogLik_k|(sequential) |    : 2.1e-10 (HapMap; the slow sample: 2.0e-10)

A wave reduction is one more reordering of the same kind, so the GPU is allowed 10 x these.  They are not tuned to its output."""
import numpy as np

RELTOL = 1e-9                # HapMap and the synthetic set; fixtures run at this reltol: the stop test of the default eps^0.75 sits inside the rounding of the sums
MLE_SPREAD_F = 2.0e-14      # measured: largest spread of F over the fixtures (absolute)
MLE_SPREAD_D = 2.5e-10      # measured: largest spread of |dLogLik| over the fixtures
MLE_F_TOL = 10 * MLE_SPREAD_F
MLE_FIRM = 10 * MLE_SPREAD_D


def simulate_inbred(n, m, f, missing, seed):
    """uint8 [m][n]: sample j has inbreeding coefficient f[j]; allele frequencies uniform in [0.05, 0.95]"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, m)
    f = np.broadcast_to(np.asarray(f, np.float64), (n,))
    a = rng.random((m, n)) < p[:, None]
    b = np.where(rng.random((m, n)) < f[None, :], a, rng.random((m, n)) < p[:, None])
    g = (a.astype(np.uint8) + b.astype(np.uint8))
    g[rng.random((m, n)) < missing] = 3
    return g, p


def hapmap_autosomal(hapmap):
    """the HapMap fixture's autosomal, polymorphic SNPs: uint8 [~8000][279]"""
    from snprelate_amd.gds import unpack_2bit_rows
    g = unpack_2bit_rows(hapmap.packed, hapmap.n_samp)
    chrom = np.asarray(hapmap.snp_chromosome)
    called = g <= 2
    s = np.where(called, g, 0).sum(1)
    keep = (chrom >= 1) & (chrom <= 22) & (s > 0) & (s < 2 * called.sum(1))
    return np.ascontiguousarray(g[keep])


def synthetic_mle():
    """uint8 [3000][20] and frequencies: inbred samples (F = 0.25, 0.5), outbred ones, a sample with excess heterozygosity (its
    estimate runs down to the boundary F = 0), and an all-missing sample (non-finite start: niter -1)"""
    n, m = 20, 3000
    f = np.array([0.25] * 7 + [0.5] * 7 + [0.0] * 6)
    g, p = simulate_inbred(n, m, f, 0.02, seed=20)
    rng = np.random.default_rng(21)
    col = g[:, 18]
    flip = (col != 1) & (col <= 2) & (rng.random(m) < 0.04)       # a few homozygotes turned heterozygous: F < 0
    col[flip] = 1
    g[:, 19] = 3
    return g, p


SLOW_RELTOL = 3.3736e-10
NEVER_RELTOL = -1e-9


def slow_mle():
    """One sample at the lower clamp that runs more than a thousand sweeps: uint8 [12000][1] and frequencies.

    Near F = 0 the update is F' = c F with c = 1 + S / m, S = sum over the homozygotes of (1 - x) / x minus the number of
    heterozygotes (the score at F = 0; x the frequency of the homozygote's allele) and m the called SNPs.  Homozygotes of an
    outbred sample are turned heterozygous until S <= -35: the estimate is negative, the iteration starts at the clamp 0.001 and
    shrinks F by 0.3 % per sweep, and |dLogLik| falls by about 1.2e-8 per sweep around sweep 1 000.  SLOW_RELTOL puts the stop
    threshold (reltol |loglik| = 3.26e-6) midway between two consecutive |dLogLik| there, as computed from the restatement alone:
    the stop falls on sweep 1 021 with a margin of about 5.8e-9, above MLE_FIRM."""
    m = 12000
    rng = np.random.default_rng(51)
    p = rng.uniform(0.05, 0.95, m)
    col = (rng.random(m) < p).astype(np.uint8) + (rng.random(m) < p).astype(np.uint8)
    col[rng.random(m) < 0.02] = 3
    x = np.where(col == 0, 1 - p, p)
    hom = (col == 0) | (col == 2)
    score = float(((1 - x[hom]) / x[hom]).sum() - (col == 1).sum())
    for i in rng.permutation(m):
        if score <= -35.0:
            break
        if col[i] in (0, 2):
            xi = (1 - p[i]) if col[i] == 0 else p[i]
            col[i] = 1
            score -= (1 - xi) / xi + 1
    return col[:, None].copy(), p


def never_stopping_mle():
    """uint8 [400][6] and frequencies, run at NEVER_RELTOL < 0: the stop threshold reltol |loglik| is negative, no |dLogLik| is
    below it, so every sample runs all 10 000 updates and reports 10 001; the margin is at least |threshold| (about 2.5e-7)"""
    return simulate_inbred(6, 400, [0.0, 0.0, 0.1, 0.25, 0.5, 0.9], 0.02, seed=61)
