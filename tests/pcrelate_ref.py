"""PC-Relate restated in numpy from the definitions of include/snpgpu.h section 1r / DESIGN.md 31, not from the kernels: the
regression matrix W (the host's Cholesky loops, operation for operation, so that float64 gives the library's bits), beta, the
individual-specific frequencies, the nine operands, the eight accumulated planes and the finaliser -- in float64 or, with
dtype=np.longdouble, in extended precision -- and the error bounds the tests hold the device to.  Also a generator of small
two-way admixed data sets with planted relatives.

Genotypes are uint8 [n_snp][n_samp], 0 / 1 / 2 and 3 = missing, as pack_2bit_rows takes them."""
import numpy as np

PLANES = ("RR", "SS", "DD", "DC", "CC", "IBS0", "K0D", "NS")
KIN_SPLIT = 2.0 ** -2.5
EPS = 2.0 ** -53


# ---- data ----------------------------------------------------------------------------------------------------------------------

def admixed_families(n_samp, n_snp, seed, missing=0.03, empty_sample=None, training=None):
    """A two-way admixed data set: two ancestral frequency vectors, an admixture fraction per founder, nuclear families of two
    founders and two children (children inherit one allele of each parent per SNP; their admixture is their parents' mean),
    single founders for what four do not divide, and -- from two samples on -- the last sample a duplicate of the first.  Calls
    are missing at rate `missing`; with three SNPs or more the last but one is monomorphic and the last has no called training
    sample (training: a mask, the founders by default); with empty_sample (default: from 17 samples on) the last but one sample has no call at all.

    dict(geno [n_snp][n_samp] uint8, admix [n_samp], founder [n_samp] bool, pairs: dict of index arrays [k][2] for "po", "sibs",
    "spouses", "unrelated" (founders of different families) and "dup")"""
    rng = np.random.default_rng(seed)
    n, m = int(n_samp), int(n_snp)
    if empty_sample is None:
        empty_sample = n >= 17
    p1 = rng.uniform(0.1, 0.9, m)
    p2 = np.clip(p1 + rng.normal(0, 0.2, m), 0.05, 0.95)
    n_core = n - 1 if n >= 2 else n
    hap = np.zeros((n, 2, m), np.uint8)
    admix = np.zeros(n)
    founder = np.zeros(n, bool)
    po, sibs, spouses = [], [], []
    family = np.full(n, -1)
    i = fam = 0
    while i < n_core:
        if n_core - i >= 4:
            f0, f1, c0, c1 = i, i + 1, i + 2, i + 3
            for f in (f0, f1):
                admix[f] = rng.uniform(0, 1)
                hap[f] = rng.random((2, m)) < admix[f] * p1 + (1 - admix[f]) * p2
                founder[f] = True
            for c in (c0, c1):
                admix[c] = (admix[f0] + admix[f1]) / 2
                pick0, pick1 = rng.integers(0, 2, m), rng.integers(0, 2, m)
                hap[c, 0] = np.where(pick0 == 0, hap[f0, 0], hap[f0, 1])
                hap[c, 1] = np.where(pick1 == 0, hap[f1, 0], hap[f1, 1])
                po += [(f0, c), (f1, c)]
            sibs.append((c0, c1))
            spouses.append((f0, f1))
            family[i:i + 4] = fam
            i += 4
        else:
            admix[i] = rng.uniform(0, 1)
            hap[i] = rng.random((2, m)) < admix[i] * p1 + (1 - admix[i]) * p2
            founder[i] = True
            family[i] = fam
            i += 1
        fam += 1
    geno = (hap[:, 0] + hap[:, 1]).T.astype(np.uint8).copy()          # [m][n]
    if m >= 3:
        geno[m - 2] = 0                                                  # monomorphic
    dup = []
    if n >= 2:
        geno[:, n - 1] = geno[:, 0]
        admix[n - 1] = admix[0]
        family[n - 1] = family[0]
        dup.append((0, n - 1))
    geno[rng.random((m, n)) < missing] = 3
    if m >= 3:
        geno[m - 1, founder if training is None else np.asarray(training, bool)] = 3      # no called training sample
    if empty_sample and n >= 3:
        geno[:, n - 2] = 3
    fidx = np.flatnonzero(founder)
    unrelated = [(a, b) for k, a in enumerate(fidx) for b in fidx[k + 1:] if family[a] != family[b]]
    arr = lambda x: np.array(x, np.int64).reshape(-1, 2)
    return dict(geno=geno, admix=admix, founder=founder,
                pairs=dict(po=arr(po), sibs=arr(sibs), spouses=arr(spouses), unrelated=arr(unrelated), dup=arr(dup)))


# ---- the regression matrix -------------------------------------------------------------------------------------------------------

def design(pcs, n_samp, dtype=np.float64):
    """V = [1, pcs], n x (D + 1)"""
    pcs = np.zeros((n_samp, 0)) if pcs is None or np.size(pcs) == 0 else np.asarray(pcs, np.float64).reshape(n_samp, -1)
    return np.concatenate([np.ones((n_samp, 1)), pcs], 1).astype(dtype)


def regression_matrix(V, training=None):
    """W = V_T (V_T^T V_T)^-1 as n x (D + 1) with zero rows outside T, by Cholesky: the sums over the training samples and over
    the factor's columns run in index order, one rounding per operation.  ValueError where the library refuses."""
    V = np.asarray(V)
    n, d1 = V.shape
    T = np.ones(n, bool) if training is None else np.asarray(training, bool)
    zero = V.dtype.type(0)
    G = np.zeros((d1, d1), V.dtype)
    for i in np.flatnonzero(T):
        G += np.tril(np.outer(V[i], V[i]))
    L = np.zeros((d1, d1), V.dtype)
    for a in range(d1):
        for b in range(a + 1):
            s = G[a, b]
            for k in range(b):
                s = s - L[a, k] * L[b, k]
            if a == b:
                if not s > np.ldexp(G[a, a], -40):
                    raise ValueError("the principal components are collinear in the training set")
                L[a, a] = np.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    Y = V[T].copy()                                                      # rows: L y = v, then L^T w = y
    for a in range(d1):
        s = Y[:, a].copy()
        for k in range(a):
            s = s - L[a, k] * Y[:, k]
        Y[:, a] = s / L[a, a]
    for a in range(d1 - 1, -1, -1):
        s = Y[:, a].copy()
        for k in range(a + 1, d1):
            s = s - L[k, a] * Y[:, k]
        Y[:, a] = s / L[a, a]
    W = np.full((n, d1), zero)
    W[T] = Y
    return W


# ---- beta ------------------------------------------------------------------------------------------------------------------------

def beta(geno, W, training=None, dtype=np.float64):
    """(beta [m][D + 1], used [m] bool, bound [m][D + 1]): beta_s = sum_{i in T} g~_is W_i in `dtype`, whether SNP s has a called
    training sample (else its beta is zero), and 2 (n_T + 8) 2^-53 sum_{i in T} |g~_is W_id|"""
    g = np.asarray(geno)
    m, n = g.shape
    T = np.ones(n, bool) if training is None else np.asarray(training, bool)
    called = g < 3
    ct = called & T[None, :]
    cnt = ct.sum(1)
    sm = np.where(ct, g, 0).sum(1)
    used = cnt > 0
    f2 = np.zeros(m, dtype)
    f2[used] = 2 * (sm[used].astype(dtype) / (2 * cnt[used]).astype(dtype))
    gt = np.where(called, g.astype(dtype), f2[:, None])[:, T]
    Wt = np.asarray(W)[T].astype(dtype)
    b = gt @ Wt
    bound = 2 * (int(T.sum()) + 8) * EPS * (np.abs(gt) @ np.abs(Wt)).astype(np.float64)
    b[~used] = 0
    return b, used, bound


# ---- operands, planes ------------------------------------------------------------------------------------------------------------

def operands(geno, b, used, V, maf_thresh=0.01, dtype=np.float64):
    """dict of the nine operands [m][n] (zero where (i, s) is not valid), plus mu and valid"""
    g = np.asarray(geno)
    b = np.asarray(b).astype(dtype)
    V = np.asarray(V).astype(dtype)
    mu = b[:, :1] + np.zeros((1, V.shape[0]), dtype)
    for d in range(1, V.shape[1]):
        mu = mu + b[:, d:d + 1] * V[None, :, d]
    mu = mu / 2
    lo, hi = dtype(maf_thresh), dtype(1.0 - maf_thresh)                  # the bounds are the library's doubles
    valid = (g < 3) & np.asarray(used)[:, None] & (mu >= lo) & (mu <= hi)
    z = lambda x: np.where(valid, x, dtype(0)).astype(dtype)
    gd = g.astype(dtype)
    c = mu * (1 - mu)
    ops = dict(R=z(gd - 2 * mu), c=z(c), S=z(np.sqrt(np.where(valid, c, 0))), gD=z(np.where(g == 0, mu, np.where(g == 2, 1 - mu, 0))),
               I0=z(g == 0), I2=z(g == 2), A=z(mu * mu), B=z((1 - mu) * (1 - mu)), O=z(1))
    ops["mu"], ops["valid"] = mu, valid
    return ops


_PRODUCTS = dict(RR=[("R", "R")], SS=[("S", "S")], DD=[("gD", "gD")], DC=[("gD", "c")], CC=[("c", "c")],
                 IBS0=[("I0", "I2"), ("I2", "I0")], K0D=[("A", "B"), ("B", "A")], NS=[("O", "O")])


def planes(ops, names=PLANES):
    """(dict plane -> n x n sums, dict plane -> max_ij sum_s |x_is| |y_js|)"""
    out, mag = {}, {}
    for name in names:
        out[name] = sum(ops[x].T @ ops[y] for x, y in _PRODUCTS[name])
        mag[name] = float(sum(np.abs(ops[x]).T @ np.abs(ops[y]) for x, y in _PRODUCTS[name]).max()) if out[name].size else 0.0
    return out, mag


def plane_bound(mag, n_snp, n_pc):
    """2 (M + 8 (D + 2)) 2^-53 max_ij sum_s |x_is| |y_js|: M - 1 additions in any order, at most 8 (D + 2) roundings per term for
    mu's FMAs, the operand arithmetic and the square root, a factor 2"""
    return 2 * (n_snp + 8 * (n_pc + 2)) * EPS * mag


# ---- the finaliser -----------------------------------------------------------------------------------------------------------------

def finalise(P):
    """dict(kinship, inbreed, nsnp and -- where the IBD planes are given -- k0, k1, k2) from the planes, in their dtype"""
    with np.errstate(divide="ignore", invalid="ignore"):
        kin = P["RR"] / (4 * P["SS"])
        inb = 2 * np.diag(kin) - 1
        r = dict(kinship=kin, inbreed=inb, nsnp=P["NS"])
        if "DD" in P:
            e = 1 + inb
            ei, ej = e[:, None], e[None, :]
            k2 = (P["DD"] - ej * P["DC"] - ei * P["DC"].T + ei * ej * P["CC"]) / P["CC"]
            k0 = np.where(kin < KIN_SPLIT, P["IBS0"] / P["K0D"], 1 - 4 * kin + k2)
            r.update(k0=k0, k2=k2, k1=1 - k0 - k2)
    return r


def pcrelate(geno, pcs=None, training=None, maf_thresh=0.01, dtype=np.float64, b=None, ibd=True):
    """The whole estimator: dict(W, beta, used, beta_bound, ops, planes, mag, result).  b: use these coefficients (the device's)
    instead of the restated ones."""
    g = np.asarray(geno)
    V = design(pcs, g.shape[1])
    W = regression_matrix(V, training)
    b_ref, used, bb = beta(g, W, training, dtype)
    ops = operands(g, b_ref if b is None else b, used, V, maf_thresh, dtype)
    P, mag = planes(ops, PLANES if ibd else ("RR", "SS", "NS"))
    return dict(W=W, beta=b_ref, used=used, beta_bound=bb, ops=ops, planes=P, mag=mag, result=finalise(P))
