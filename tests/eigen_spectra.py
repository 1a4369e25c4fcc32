"""Degenerate and clustered spectra for the top-k eigen solver, and the comparison every eigen route is held to
(tests/test_cpu_eigen_spectra.py without a GPU, tests/test_gpu_eigen_spectra.py with one; tools/fuzz_eigen.py draws its cases here).
Nothing here imports the HIP library or torch: the functions that open contexts take the binding module as an argument.

Multiple eigenvalues made exactly from genotypes.  X is L1 x m without missing calls, every row with as many 0s as 2s and 1s
elsewhere: the row mean is exactly 1, p exactly 0.5.  For c copies g is (c L1) x (c m) with X in every diagonal block and 1 everywhere
else; the constant part centres to exactly 0, so the PCA covariance and the GCTA GRM are blockdiag(C_X, ..., C_X): every eigenvalue of
C_X has multiplicity c.  The samples are permuted, so that no block coincides with a row panel.  On the device the fp32 parts of the
accumulation split each cluster by 1e-7 to 1e-6 of the largest eigenvalue: copies that a Krylov space cannot tell apart, which is the
regime in which a block method misses a copy, returns a vector twice or loses orthogonality inside a cluster.

The near-degenerate form changes two or three genotypes and removes a call in ONE copy: the clusters spread, to a size that
near_figures() measures and tests/test_cpu_eigen_spectra.py holds ten times below the smallest cluster gap.

check_topk() is the comparison: numpy's eigh of the DEVICE's own gathered matrix in fp64 is the reference (that isolates the solver
from the accumulation), eigenvalues WITH multiplicity, residuals, orthonormality, and cluster SUBSPACES in place of vectors -- no
vector is skipped because its eigenvalue has a close neighbour."""
import numpy as np

from snprelate_amd.dist import slab_range

EIGENVALUE_BOUND = 1e-9        # max |w - w_ref| / |w_ref[0]|   (tools/fuzz_eigen.py)
RESIDUAL_BOUND = 1e-7          # max ||full v - w v|| / |w|      (tools/fuzz_eigen.py)
ORTHO_FACTOR = 1000.0          # max |V^T V - I| against numpy's own figure on the same matrix
SUBSPACE_BOUND = 1e-6          # ||P_cluster v|| >= 1 - this; smallest singular value of P_cluster V_cluster >= 1 - this
# Eigenvalues closer than CLUSTER_REL |w_ref[0]| share a cluster.  With a residual of at most RESIDUAL_BOUND |w| and every other
# eigenvalue at least CLUSTER_REL |w_ref[0]| away from the cluster, the sine between a returned vector and the cluster's subspace is at
# most 1e-7 / 1e-4 = 1e-3 (Davis-Kahan), i.e. 1 - cosine <= 5e-7 < SUBSPACE_BOUND: the subspace check asks nothing the residual bound
# does not promise, and the constructions' gaps (>= 5e-3) and device-side splits (<= 1e-6) lie far on either side of it.
CLUSTER_REL = 1e-4

SIZES = {                       # name: (m, L1, copies, seed) of the GPU tests; seeds with cluster gaps >= 5e-3 of the largest eigenvalue
    "n140": (70, 400, 2, 12),
    "n210": (70, 400, 3, 12),
    "n540": (180, 600, 3, 4),
}
TOP = 16                        # the largest k of the tests: the clusters that matter are those of the leading TOP + 1 eigenvalues
ODDS_0 = (1.5, 1.0, 1.0)         # odds of the three sample sub-groups to carry a row's 0s ...
ODDS_2 = (1.0, 1.5, 1.0)         # ... and its 2s
NEAR = {                        # name: (genotypes changed in copy 0, calls removed there, seed of the places)
    "n140": (2, 1, 2013),       # chosen on the CPU oracle so that the clusters spread at least ten times less than the smallest
    "n210": (3, 1, 2012),       # gap between them (tests/test_cpu_eigen_spectra.py asserts it and prints the figures)
    "n540": (3, 1, 2005),
}


# ---- the constructions ---------------------------------------------------------------------------------------------------------------

def balanced_block(m, L1, seed):
    """uint8 [L1][m]: every row holds q 0s, q 2s (q drawn from 1 ... m // 2) and 1s elsewhere.  Three sub-groups of the samples carry
    the 0s and the 2s with different odds, so the block has structural eigenvalues over its bulk."""
    rng = np.random.default_rng(seed)
    grp = np.arange(m) * 3 // m
    odds0 = np.array(ODDS_0)[grp]
    odds2 = np.array(ODDS_2)[grp]
    x = np.ones((L1, m), np.uint8)
    for s in range(L1):
        q = int(rng.integers(1, m // 2 + 1))
        zeros = rng.choice(m, q, replace=False, p=odds0 / odds0.sum())
        w = odds2.copy()
        w[zeros] = 0.0
        twos = rng.choice(m, q, replace=False, p=w / w.sum())
        x[s, zeros] = 0
        x[s, twos] = 2
    return x


def degenerate_geno(m, L1, copies, seed):
    """(g uint8 [copies L1][copies m], perm): the block construction of the module text; sample perm[j] of the block layout is column
    j of g.  The permutation is drawn from `seed` alone."""
    x = balanced_block(m, L1, seed)
    g = np.ones((copies * L1, copies * m), np.uint8)
    for c in range(copies):
        g[c * L1:(c + 1) * L1, c * m:(c + 1) * m] = x
    perm = np.random.default_rng(seed + 1000).permutation(copies * m)
    return np.ascontiguousarray(g[:, perm]), perm


def near_degenerate_geno(m, L1, copies, seed, edits, missing, near_seed):
    """The exact form with `edits` genotypes of copy 0 moved to another call and `missing` of its calls removed (3), at places drawn
    from near_seed.  One changed call moves its SNP's mean for every sample and with it the eigenvalues of its copy by a few 1e-4 of
    the largest; measured on the CPU oracle at n = 140, 36 changed genotypes and 1 % removed calls spread the clusters by 1.9e-2 of
    the largest eigenvalue, across gaps of 4e-3.  A spread ten times below the smallest gap leaves room for a handful of changes."""
    g, perm = degenerate_geno(m, L1, copies, seed)
    rng = np.random.default_rng(near_seed)
    cols = np.nonzero(perm < m)[0]                      # the columns of copy 0
    cells = rng.choice(L1 * m, edits + missing, replace=False)
    for t, cell in enumerate(cells):
        r, c = int(cell) // m, cols[int(cell) % m]
        g[r, c] = 3 if t >= edits else (g[r, c] + 1 + int(rng.integers(2))) % 3
    return g, perm


def size_geno(name, near=False):
    """(g, perm) of a named size, exact or near-degenerate"""
    m, L1, copies, seed = SIZES[name]
    return near_degenerate_geno(m, L1, copies, seed, *NEAR[name]) if near else degenerate_geno(m, L1, copies, seed)


def near_figures(w_exact, w_near, top=TOP):
    """(largest spread of a cluster, smallest gap between neighbouring clusters) of the near-degenerate eigenvalues, the clusters
    being those of the exact form by position, as fractions of |w_near[0]|"""
    cl, _ = clusters(w_exact, top + 1)
    spread = max(w_near[lo] - w_near[hi - 1] for lo, hi in cl) / abs(w_near[0])
    gap = min(w_near[hi - 1] - w_near[hi] for lo, hi in cl) / abs(w_near[0])
    return float(spread), float(gap)


def off_block_max(full, perm, m):
    """largest |entry| between samples of different copies"""
    blk = perm // m
    return float(np.abs(full[blk[:, None] != blk[None, :]]).max())


# ---- clusters ------------------------------------------------------------------------------------------------------------------------

def clusters(w_ref, k, rel=CLUSTER_REL):
    """Groups the descending reference eigenvalues into clusters: neighbours closer than rel |w_ref[0]| share one.  Returns
    ([(lo, hi)] of the clusters that reach into the top k, hi exclusive, and whether k cuts the last of them)."""
    w_ref = np.asarray(w_ref)
    assert 0 < k <= w_ref.size and np.all(np.diff(w_ref) <= 0)
    brk = np.nonzero(-np.diff(w_ref) >= rel * abs(w_ref[0]))[0] + 1
    edges = np.r_[0, brk, w_ref.size]
    out = [(int(lo), int(hi)) for lo, hi in zip(edges[:-1], edges[1:]) if lo < k]
    return out, out[-1][1] > k


def cluster_figures(w_ref, top=TOP, rel=CLUSTER_REL):
    """(largest spread inside a cluster, smallest gap between neighbouring clusters, multiplicities) over the clusters that reach
    into the leading top + 1 eigenvalues, spread and gap as fractions of |w_ref[0]|"""
    cl, _ = clusters(w_ref, min(top + 1, len(w_ref) - 1), rel)
    spread = max(w_ref[lo] - w_ref[hi - 1] for lo, hi in cl) / abs(w_ref[0])
    gap = min(w_ref[hi - 1] - w_ref[hi] for lo, hi in cl if hi < len(w_ref)) / abs(w_ref[0])
    return float(spread), float(gap), [hi - lo for lo, hi in cl]


# ---- the comparison ------------------------------------------------------------------------------------------------------------------

def reference(full):
    """(eigenvalues descending, eigenvectors in that order, numpy's own max |Q^T Q - I| over ALL n vectors) of a symmetric matrix"""
    w, q = np.linalg.eigh(full)
    w, q = w[::-1], q[:, ::-1]
    return w, q, float(np.abs(q.T @ q - np.eye(len(w))).max())


def figures(w, V, full, k, ref=None):
    """the figures of check_topk as a dict, nothing asserted"""
    w = np.asarray(w, np.float64)
    V = np.asarray(V, np.float64)
    n = full.shape[0]
    assert w.shape == (k,) and V.shape == (n, k), (w.shape, V.shape, n, k)
    w_ref, q, ortho_np = ref if ref is not None else reference(full)
    f = {"eigenvalues": float(np.abs(w - w_ref[:k]).max() / abs(w_ref[0])),
         "descending": bool(np.all(np.diff(w) <= 0)),
         "residual": float((np.linalg.norm(full @ V - V * w, axis=0) / np.abs(w)).max()),
         "ortho": float(np.abs(V.T @ V - np.eye(k)).max()), "ortho_numpy": ortho_np}
    cl, cut = clusters(w_ref, k)
    inside, span = 1.0, 1.0
    for lo, hi in cl:
        qc = q[:, lo:hi]
        coef = qc.T @ V[:, lo:min(hi, k)]               # the cluster's own coordinates of the vectors assigned to it
        inside = min(inside, float(np.linalg.norm(coef, axis=0).min()))
        if hi <= k:                                     # a whole cluster: its vectors must span it
            span = min(span, float(np.linalg.svd(coef, compute_uv=False).min()))
    f.update(inside=inside, span=span, clusters=len(cl), cut=cut, largest_cluster=max(hi - lo for lo, hi in cl))
    return f


def report(name, f):
    print("%s: eigenvalues %.1e residual %.1e orthonormality %.1e (numpy %.1e) in-cluster %.1e span %.1e; %d clusters, largest %d%s" %
          (name, f["eigenvalues"], f["residual"], f["ortho"], f["ortho_numpy"], 1 - f["inside"], 1 - f["span"], f["clusters"],
           f["largest_cluster"], ", k cuts the last" if f["cut"] else ""), flush=True)


def check_topk(w, V, full, k, name="top-k", ref=None):
    """The k largest eigenpairs (w [k] descending, V [n][k]) against numpy's eigh of `full` in fp64; prints, then asserts.
    ref: reference(full), where several calls share one matrix."""
    f = figures(w, V, full, k, ref)
    report(name, f)
    assert f["descending"], (name, "eigenvalues not in descending order", np.asarray(w))
    assert f["eigenvalues"] < EIGENVALUE_BOUND, (name, "eigenvalues (with multiplicity)", f)
    assert f["residual"] < RESIDUAL_BOUND, (name, "residual", f)
    assert f["ortho"] <= ORTHO_FACTOR * f["ortho_numpy"], (name, "orthonormality", f)
    assert f["inside"] >= 1 - SUBSPACE_BOUND, (name, "a vector leaves its cluster's subspace", f)
    assert f["span"] >= 1 - SUBSPACE_BOUND, (name, "the vectors of a cluster do not span it", f)
    return f


# ---- contexts (the binding module is the caller's) -----------------------------------------------------------------------------------

def three_panels(n):
    """row bounds of three 256-aligned panels (n = 540: 0-256, 256-512, 512-540, cutting through the permuted copies); below 513
    samples there are fewer non-empty ones"""
    return [0, min(256, n), min(512, n), n]


def open_panels(lib, kind, g, bounds=None, blk=1024):
    """([contexts], [(row_begin, row_end)]): one context per non-empty panel of the row bounds (None: one full context), each fed all
    of g in blocks of blk SNPs"""
    n = g.shape[1]
    b = list(bounds) if bounds is not None else [0, n]
    panels, rows = [], []
    for r0, r1 in zip(b[:-1], b[1:]):
        if r1 > r0:
            a = lib.Accumulator(getattr(lib, kind), n, row_begin=r0, row_end=r1 if len(b) > 2 else 0, max_block_snps=max(blk, 64))
            for i in range(0, g.shape[0], blk):
                a.feed(g[i:i + blk])
            panels.append(a)
            rows.append((r0, r1))
    return panels, rows


def gathered(kind, panels, rows, n):
    """The device's own matrix as the solver will see it, full [n][n] in fp64: the PCA covariance trace-normalised on the host, the
    GCTA GRM and the EIGMIX matrix as finalised -- and those contexts finalised in place afterwards, ready for the solver."""
    tri = np.zeros(n * (n + 1) // 2)
    for a, (r0, r1) in zip(panels, rows):
        lo, hi = slab_range(n, r0, r1)
        if kind == "PCA_COV":
            tri[lo:hi] = a.pca_cov(packed=True, normalize=False)[0]
        elif kind == "GRM_GCTA":
            tri[lo:hi] = a.grm_gcta(packed=True)
        else:
            tri[lo:hi] = a.eigmix(packed=True)
    full = np.empty((n, n))
    iu = np.triu_indices(n)
    full[iu] = tri
    full.T[iu] = tri
    if kind == "PCA_COV":
        full *= (n - 1) / np.trace(full)
    else:
        for a in panels:
            a.finalize_inplace()
    return full


# ---- the generic spectra of tools/fuzz_eigen.py ----------------------------------------------------------------------------------------

def fuzz_case(rng, synth_geno):
    """One case of the randomised sweep, drawn from rng: sample and SNP counts that are multiples of nothing, a missing rate, the
    matrix kind, row panels, k, the feed block -- and the genotypes (synth_geno: oracle.synth.synth_geno), with the allele
    frequencies of a third of the samples shifted on half of the SNPs."""
    n = int(rng.integers(40, 2600))
    L = int(rng.integers(200, 2500))
    miss = float(rng.choice([0.0, 0.02, 0.2]))
    kind = str(rng.choice(["PCA_COV", "GRM_GCTA", "EIGMIX"]))
    world = int(rng.choice([1, 1, 2, 3]))
    k = int(rng.integers(1, max(2, min(33, n // 3))))
    blk = int(rng.choice([256, 1000, 4096]))
    g = synth_geno(n, L, missing=miss, seed=int(rng.integers(1 << 30)))
    grp = rng.random(n) < 0.33
    flip = rng.random(L) < 0.5
    sub = g[np.ix_(flip, grp)]
    sub[(sub == 0) & (rng.random(sub.shape) < 0.4)] = 1
    g[np.ix_(flip, grp)] = sub
    return dict(n=n, L=L, miss=miss, kind=kind, world=world, k=k, blk=blk, g=g)
