"""Classical multidimensional scaling restated in numpy, and the distance matrices the MDS tests run on (tests/test_cpu_mds.py without
a GPU, tests/test_gpu_mds.py with one).  Nothing here imports the HIP library or torch.

For a symmetric n x n distance matrix D:  B = -1/2 J (D o D) J,  J = I - 1 1^T / n,  D o D = D with every entry squared.  The k
algebraically largest eigenpairs (lambda_i, v_i) of B, k1 = #{i <= k: lambda_i > 0}, points[:, i] = v_i sqrt(lambda_i) for i < k1.
B always has the eigenpair (0, 1), and n - p - 1 more zeros for points in p dimensions: "> 0" is read as "above what rounding makes
of an exact zero", pos_tol(D) = n 2^-52 max_i sum_j d_ij^2 / 2 (|B|_2 <= |D o D|_inf / 2) -- the library's rule, on both routes.
Sign rule: in every vector the entry of largest magnitude (the lowest index on ties) is positive."""
import numpy as np

SEED = 7


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def b_matrix(D):
    """B = -1/2 J (D o D) J, formed explicitly"""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    J = np.eye(n) - np.full((n, n), 1.0 / n)
    B = -0.5 * (J @ (D * D) @ J)
    return (B + B.T) / 2


def apply_ref(D, Q):
    """Y = B Q for Q [b][n] (vector-major), centre -> multiply -> centre, and the bound's |D o D| |J q| per vector"""
    D = np.asarray(D, np.float64)
    W = Q - Q.mean(axis=1, keepdims=True)
    Z = W @ (D * D)                                   # D symmetric
    return -0.5 * (Z - Z.mean(axis=1, keepdims=True)), np.abs(W) @ (D * D)


def pos_tol(D):
    D = np.asarray(D, np.float64)
    return D.shape[0] * 2.0 ** -52 * (D * D).sum(axis=1).max() / 2


def trace_b(D):
    D = np.asarray(D, np.float64)
    return ((D * D).sum() / D.shape[0] - (np.diag(D) ** 2).sum()) / 2


def sign_rule(V):
    """columns of V with the entry of largest magnitude (lowest index on ties) made positive"""
    V = np.array(V, np.float64)
    for j in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, j])), j] < 0:
            V[:, j] = -V[:, j]
    return V


def eigh_desc(B):
    w, q = np.linalg.eigh(B)
    return w[::-1], q[:, ::-1]


def cmdscale(D, k, eig=None):
    """dict(eigenval [k], vectors [n][k], points [n][k1], all_eigval [n], GOF [2], trace, n_pos); eig: eigh_desc(b_matrix(D))"""
    w, q = eig if eig is not None else eigh_desc(b_matrix(D))
    ev, V = w[:k], sign_rule(q[:, :k])
    k1 = int(np.count_nonzero(ev > pos_tol(D)))
    return dict(eigenval=ev, vectors=V, points=V[:, :k1] * np.sqrt(ev[:k1]), all_eigval=w,
                GOF=np.array([ev.sum() / np.abs(w).sum(), ev.sum() / np.maximum(w, 0).sum()]), trace=trace_b(D), n_pos=k1)


def pairwise(points):
    """Euclidean distances between the rows"""
    d = points[:, None, :] - points[None, :, :]
    return np.sqrt((d * d).sum(axis=-1))


# ---- the inputs, each a function of (n, seed) ----------------------------------------------------------------------------------------

def euclid(n, p, seed=SEED):
    """(D, X): n points in p <= 3 dimensions with axis scales 3, 2, 1, centred; D their Euclidean distances.  B = X X^T."""
    assert 1 <= p <= 3
    X = np.random.default_rng(seed).standard_normal((n, p)) * np.array([3.0, 2.0, 1.0])[:p]
    X = X - X.mean(axis=0)
    return pairwise(X), X


def ibs_like(n, L=2000, seed=SEED):
    """D = sum |g - g'| / 2L over L genotypes 0 / 1 / 2 of three populations of n // 3 (the last takes the rest): population allele
    frequencies drawn around a common one (Balding-Nichols, Fst 0.02 / 0.05 / 0.10).  Integer sums: exactly symmetric."""
    rng = np.random.default_rng(seed)
    pop = np.minimum(np.arange(n) * 3 // n, 2)
    p0 = rng.uniform(0.1, 0.9, L)
    fst = (0.02, 0.05, 0.10)
    freq = np.stack([rng.beta(p0 * (1 - f) / f, (1 - p0) * (1 - f) / f) for f in fst])
    g = rng.binomial(2, freq[pop]).astype(np.float64)                     # [n][L]
    s = (g * g).sum(axis=1)
    sq = s[:, None] + s[None, :] - 2 * (g @ g.T)                          # sum (a - b)^2: 0, 1, 4 per SNP
    i0, i2 = (g == 0).astype(np.float64), (g == 2).astype(np.float64)
    two = i0 @ i2.T
    absdiff = sq - 2 * (two + two.T)                                      # |a - b|: 0, 1, 2
    return absdiff / (2.0 * L)


def nonmetric(n, seed=SEED):
    """uniform random symmetric, zero diagonal: no metric at all"""
    u = np.triu(np.random.default_rng(seed).random((n, n)), 1)
    return u + u.T


def planted(n, seed=SEED):
    """d_ij^2 = 1 + 0.9 u_i u_j with u = +-1, zero diagonal: B = 0.95 J - 0.45 (J u)(J u)^T has the eigenvalue 0.95 with multiplicity
    n - 2, the eigenvalue 0, and 0.95 - 0.45 |J u|^2, a large negative one (-140 at n = 300)"""
    u = np.where(np.random.default_rng(seed).random(n) < 0.5, -1.0, 1.0)
    d2 = 1.0 + 0.9 * np.outer(u, u)
    np.fill_diagonal(d2, 0.0)
    return np.sqrt(d2)


def spectrum_figures(D):
    """dict(negative: count of eigenvalues below -pos_tol, smallest / lambda_1, gaps: (lambda_i - lambda_{i+1}) / lambda_1 of the
    leading eight) of B"""
    w, _ = eigh_desc(b_matrix(D))
    return dict(n=len(w), negative=int(np.count_nonzero(w < -pos_tol(D))), smallest=float(w[-1] / w[0]),
                gaps=[float(x) for x in (w[:8] - w[1:9]) / w[0]], w=w)
