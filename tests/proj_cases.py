"""The shapes at which the PCA projection kernels are tested (tests/test_gpu_proj_shapes.py), each with the launch geometry it is there
for.  tests/test_cpu_proj_grid.py asks csrc/proj_grid.h (through tests/proj_grid_check.cpp) for the geometry of every case and holds
it to the `want` written here by hand from the rules of launch_proj_snp / launch_proj_samp, so a case that stops reaching its
geometry -- another clamp, another pass width -- fails on the CPU.

What `want` may name (facts(case, gx, gy, split, per) derives all of them):
  gx, gy, split, per   the launch's grid (workgroups of four 64-row groups, column passes, parts) and the length of a part
  last                 reduction length of the last part (SNP side: up to n4 = N rounded up to 4, the padding codes included)
  n4                   SNP side: where the sample loop ends
  cols                 columns of the last pass (8 or 16: full)
  fill                 output rows of the last 64-row group (64: full)
  idle                 64-row groups of the last workgroup without an output row
  tail_only            sample side: parts shorter than 4 SNPs, which the scalar tail loop alone serves
  off4                 sample side: parts that begin off a multiple of 4
  kp_eq_k              sample side: k is a multiple of 16, so the padded loadings are not zeroed first"""
import collections
import functools

import numpy as np

from oracle.synth import synth_geno

Case = collections.namedtuple("Case", "side name N n_snp k bmax want")


def _snp(name, N, n_snp, k, bmax=1024, **want):
    return Case("snp", "%s-N%d-L%d-k%d" % (name, N, n_snp, k), N, n_snp, k, bmax, want)


def _samp(name, N, n_snp, k, bmax=1024, **want):
    return Case("samp", "%s-N%d-L%d-k%d" % (name, N, n_snp, k), N, n_snp, k, bmax, want)


# A: column passes 1 ... 8 and a part-filled last pass; 200 SNPs = three full 64-SNP groups and one of 8; two sample parts (256 + 80)
A = [_snp("A", 333, 200, k, gx=1, gy=gy, cols=cols, fill=8, idle=0, split=2, per=256, last=80)
     for k, gy, cols in ((1, 1, 1), (7, 1, 7), (8, 1, 8), (9, 2, 1), (15, 2, 7), (16, 2, 8), (17, 3, 1), (31, 4, 7), (32, 4, 8), (33, 5, 1),
                         (64, 8, 8))]
# B: the sample loop ends at n4; one part up to 256 samples, then parts of 256 (per at its clamp), the last one down to 4 samples
B = [_snp("B", N, 64, 3, gy=1, per=256, n4=n4, split=split, last=last)
     for N, n4, split, last in ((1, 4, 1, 4), (2, 4, 1, 4), (3, 4, 1, 4), (4, 4, 1, 4), (5, 8, 1, 8), (63, 64, 1, 64), (64, 64, 1, 64),
                                (65, 68, 1, 68), (255, 256, 1, 256), (256, 256, 1, 256), (257, 260, 2, 4), (260, 260, 2, 4),
                                (511, 512, 2, 256), (512, 512, 2, 256), (513, 516, 3, 4), (1030, 1032, 5, 8))]
# C: 64 parts asked for -> 257 samples each, rounded up to 264 and above the clamp -> 63 parts, the last one 16 400 - 62 * 264 = 32
C = [_snp("C", 16400, 64, 3, gy=1, per=264, split=63, last=32, n4=16400)]
# D: SNP groups and workgroups up to the projector's max_block_snps = 1024; groups of the last workgroup idle
D = [_snp("D", 333, L, 11, gx=gx, gy=2, cols=3, fill=fill, idle=idle, split=2)
     for L, gx, fill, idle in ((1, 1, 1, 3), (63, 1, 63, 3), (64, 1, 64, 3), (65, 1, 1, 2), (255, 1, 63, 0), (256, 1, 64, 0), (257, 2, 1, 3),
                               (1023, 4, 63, 0), (1024, 4, 64, 0))]
SNP_CASES = A + B + C + D

# E: column passes 1 ... 4, part-filled and full; 300 SNPs in five parts (4 * 64 + 44)
E = [_samp("E", 333, 300, k, gx=2, gy=gy, cols=cols, kp_eq_k=eq, split=5, per=64, last=44, fill=13, idle=2)
     for k, gy, cols, eq in ((1, 1, 1, False), (15, 1, 15, False), (16, 1, 16, True), (17, 2, 1, False), (32, 2, 16, True), (33, 3, 1, False),
                             (64, 4, 16, True))]
# F: one part served by the tail loop alone, by both loops, a second part of 1 ... 3 SNPs; 4097 SNPs: 64 parts of 65, the last one 2
F = [_samp("F", 333, L, 3, bmax=8192, split=split, per=per, last=last, tail_only=tail, off4=off4)
     for L, split, per, last, tail, off4 in ((1, 1, 64, 1, 1, 0), (2, 1, 64, 2, 1, 0), (3, 1, 64, 3, 1, 0), (4, 1, 64, 4, 0, 0), (5, 1, 64, 5, 0, 0),
                                             (63, 1, 64, 63, 0, 0), (64, 1, 64, 64, 0, 0), (65, 2, 64, 1, 1, 0), (66, 2, 64, 2, 1, 0),
                                             (67, 2, 64, 3, 1, 0), (129, 3, 64, 1, 1, 0), (4097, 64, 65, 2, 1, 48))]
# G: 257 sample groups in 65 workgroups (the last one holds one group); 16 parts asked for -> 9 SNPs each, clamped to 64 -> 3 parts
G = [_samp("G", 16400, 130, 3, gx=65, idle=3, fill=16, split=3, per=64, last=2, tail_only=1)]
# H: sample groups and workgroups
H = [_samp("H", N, 130, 3, gx=gx, fill=fill, idle=idle, split=3, last=2)
     for N, gx, fill, idle in ((1, 1, 1, 3), (63, 1, 63, 3), (64, 1, 64, 3), (65, 1, 1, 2), (255, 1, 63, 0), (256, 1, 64, 0), (257, 2, 1, 3),
                               (1030, 5, 6, 3))]
SAMP_CASES = E + F + G + H

STAGE_N, STAGE_L, STAGE_K = 333, 513, 11        # the staging tests: one block, two SNP-side workgroups, two column passes
EIGVAL_HI, EIGVAL_LO, TRACE = 3.0, 0.5, 123.4   # the loadings' eigenvalues run from 3 down to 0.5


def facts(case, gx, gy, split, per):
    """everything `want` may name, from the launch geometry and the kernels' own index rules"""
    rows, red, kc = (case.n_snp, case.N, 8) if case.side == "snp" else (case.N, case.n_snp, 16)
    groups = (rows + 63) // 64
    f = dict(gx=gx, gy=gy, split=split, per=per, cols=case.k - (gy - 1) * kc, fill=rows - (groups - 1) * 64, idle=gx * 4 - groups)
    if case.side == "snp":
        red = f["n4"] = (case.N + 3) & ~3
    parts = [(z * per, min(z * per + per, red)) for z in range(split)]
    f["parts"] = parts
    f["last"] = parts[-1][1] - parts[-1][0]
    if case.side == "samp":
        f["tail_only"] = sum(1 for a, b in parts if b - a < 4)
        f["off4"] = sum(1 for a, b in parts if a % 4)
        f["kp_eq_k"] = case.k % 16 == 0
    return f


def eigenvalues(k):
    return np.linspace(EIGVAL_HI, EIGVAL_LO, k)


@functools.lru_cache(maxsize=None)
def inputs(N, n_snp, k, seed=0):
    """(g uint8 [n_snp][N], ev [k][N], sload [n_snp][k]): synth_geno with 6 % missing calls and, where there is room, its planted SNPs
    (3 and 5 monomorphic, 7 without a call, 11 with one call, 13 all heterozygous), SNP 9 with five calls and one sample without a
    call; seeded normal eigenvectors and loadings, eigenvector 3 constant 1.  Read-only: the arrays are shared between tests."""
    g = synth_geno(N, n_snp, missing=0.06, seed=1000 + 7 * N + 3 * n_snp + seed)
    if N >= 16:
        if n_snp >= 16:
            g[9, :5] = (0, 1, 2, 1, 0)
            g[9, 5:] = 3
        g[:, N // 2] = 3
    rng = np.random.default_rng(17 * N + n_snp + 131 * k + seed)
    ev, sload = rng.normal(size=(k, N)), rng.normal(size=(n_snp, k))
    if k >= 4:
        ev[3] = 1.0
        sload[:, 3] = 1.0
    for x in (g, ev, sload):
        x.setflags(write=False)
    return g, ev, sload
