"""numpy restatements of what snpgdsHCluster / snpgdsCutTree compute, written from their stated semantics (include/snpgpu.h
section 1h) and not from the kernels: average-linkage clustering with its tie rule, the counter-based random stream
and the draw rule, the permutation test as the device defines it (`dist_perm_counter`, direct double sums) and as the reference
runs it (`dist_perm_sequential`: the arrangement carried over, uniforms from a numpy Generator), the group pass and R's relabelling."""
import numpy as np

# ---- hclust(method = "average") ------------------------------------------------------------------------------------------------


def upgma(dist):
    """(merge int32 [n - 1][2], height, order int32 [n]) of the lower triangle of `dist` in R's conventions.  Every row keeps its
    nearest neighbour among the later rows, the globally closest pair is merged into the row of lower index, strict < in both
    scans: of tied distances the one of lowest index wins."""
    d = np.array(dist, np.float64)
    n = d.shape[0]
    d = np.tril(d, -1)
    d = d + d.T                                   # only the lower triangle is read
    alive = np.ones(n, bool)
    memb = np.ones(n)
    label = -(np.arange(n) + 1)
    nn = np.full(n, -1)
    dnn = np.full(n, np.inf)

    def scan(i):
        nn[i], dnn[i] = -1, np.inf
        for j in range(i + 1, n):
            if alive[j] and d[j, i] < dnn[i]:
                nn[i], dnn[i] = j, d[j, i]

    for i in range(n - 1):
        scan(i)
    merge = np.zeros((n - 1, 2), np.int32)
    height = np.zeros(n - 1)
    for step in range(n - 1):
        im, dm = -1, np.inf
        for i in range(n - 1):
            if alive[i] and nn[i] >= 0 and dnn[i] < dm:
                im, dm = i, dnn[i]
        i2, j2 = im, nn[im]
        a, b = label[i2], label[j2]
        if (a > 0 and b < 0) or (a > 0 and b > 0 and b < a):
            a, b = b, a
        merge[step] = (a, b)
        height[step] = dm
        label[i2] = step + 1
        alive[j2] = False
        for k in range(n):
            if alive[k] and k != i2:
                v = (memb[i2] * d[i2, k] + memb[j2] * d[j2, k]) / (memb[i2] + memb[j2])
                d[i2, k] = d[k, i2] = v
        memb[i2] += memb[j2]
        for i in range(n - 1):
            if alive[i] and (i == i2 or nn[i] == i2 or nn[i] == j2):
                scan(i)
    return merge, height, merge_to_order(merge)


def merge_members(merge):
    """list per merge: (members 0-based, first column's then second column's, n1, n2) -- the reference's A, :576-602"""
    out = []
    for a, b in np.asarray(merge):
        ma = [-a - 1] if a < 0 else list(out[a - 1][0])
        mb = [-b - 1] if b < 0 else list(out[b - 1][0])
        out.append((ma + mb, len(ma), len(mb)))
    return out


def merge_to_order(merge):
    """1-based leaves with the first column of every merge to the left"""
    return np.asarray(merge_members(merge)[-1][0], np.int32) + 1


# ---- the counter-based stream and the draw rule ------------------------------------------------------------------------------------

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32(key, c0, c1, c2, c3):
    """Philox4x32-10 on arrays of counters: four uint32 arrays"""
    m32 = np.uint64(0xFFFFFFFF)
    x = [np.asarray(c, np.uint64) & m32 for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_M0) * x[0]
        p1 = np.uint64(_M1) * x[2]
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ x[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return x


def uniform(seed, merge_idx, perm, draw):
    """u = (x + 0.5) 2^-32 of word draw & 3 of the block with counter (draw >> 2, perm, merge, 0)"""
    w = philox4x32(seed, np.asarray(draw) >> 2, perm, merge_idx, 0)
    x = np.choose(np.asarray(draw) & 3, w)
    return (x.astype(np.float64) + 0.5) * 2.0 ** -32


def draw_offset(u, rng_size):
    """the reference's _RandomNum(Range): (int)(u (Range - 1) + 0.5), at most Range - 1 (product and sum rounded separately)"""
    return np.minimum(rng_size - 1, (u * np.float64(rng_size - 1) + 0.5).astype(np.int64))


def rotation(seed, merge_idx, perm, N):
    """the offset by which a permutation rotates the member order before its shuffle: floor(u N), u from word 0 of the block with
    counter (2^32 - 1, perm, merge, 0)"""
    x = philox4x32(seed, 0xFFFFFFFF, perm, merge_idx, 0)[0]
    return np.minimum(N - 1, ((x.astype(np.float64) + 0.5) * 2.0 ** -32 * np.float64(N)).astype(np.int64))


def arrangements(seed, merge_idx, n_perm, N, ns1):
    """int [n_perm][N]: every permutation's arrangement of the members 0 ... N - 1 after the partial shuffle of its first ns1 slots,
    each started from the member order rotated by its own offset"""
    arr = (np.arange(N)[None, :] + rotation(seed, merge_idx, np.arange(n_perm), N)[:, None]) % N
    rows = np.arange(n_perm)
    for i in range(ns1):
        j = i + draw_offset(uniform(seed, merge_idx, rows, i), N - i)
        vi, vj = arr[rows, i].copy(), arr[rows, j].copy()
        arr[rows, i], arr[rows, j] = vj, vi
    return arr


def _z(obs, vals):
    mean = vals.sum() / len(vals)
    var = ((vals - mean) ** 2).sum() / (len(vals) - 1)
    sd = np.sqrt(var)
    return (float((obs - mean) / sd) if var > 0 else 0.0), float(mean), float(sd)


def dist_perm_counter(dist, merge, n_perm, z_threshold, seed):
    """what snpgpu_dist_perm computes, with direct double sums: dict(z, n1, n2, group, obs, perm_mean, perm_sd)"""
    dist = np.asarray(dist, np.float64)
    nm = len(merge)
    out = dict(z=np.zeros(nm), n1=np.zeros(nm, np.int32), n2=np.zeros(nm, np.int32), obs=np.zeros(nm), perm_mean=np.full(nm, np.nan),
               perm_sd=np.full(nm, np.nan))
    for m, (A, n1, n2) in enumerate(merge_members(merge)):
        out["n1"][m], out["n2"][m] = n1, n2
        sub = dist[np.ix_(A, A)]
        out["obs"][m] = sub[:n1, n1:].sum() / (n1 * n2)
        if n1 == 1 and n2 == 1:
            continue
        N, ns1 = n1 + n2, min(n1, n2)
        arr = arrangements(seed, m, n_perm, N, ns1)
        vals = np.empty(n_perm)
        step = max(1, 2_000_000 // (ns1 * (N - ns1)))
        for p0 in range(0, n_perm, step):
            a = arr[p0:p0 + step]
            vals[p0:p0 + step] = sub[a[:, :ns1, None], a[:, None, ns1:]].sum(axis=(1, 2)) / (ns1 * (N - ns1))
        with np.errstate(all="ignore"):
            out["z"][m], out["perm_mean"][m], out["perm_sd"][m] = _z(out["obs"][m], vals)
    out["group"] = group_pass(merge, out["z"], z_threshold)
    return out


def caterpillar_obs(dist, merge):
    """(n1, n2, obs) of dist_perm_counter for a caterpillar -- the first merge joins two samples, every later one a new sample
    (first column) to the cluster before it (second column) -- without the loop over merges: with the matrix reordered by the
    order in which the samples join, the observed value of merge k >= 1 is the mean of row k + 1 over its first k + 1 columns."""
    dist = np.asarray(dist, np.float64)
    merge = np.asarray(merge)
    nm = len(merge)
    assert (merge[0] < 0).all() and (merge[1:, 0] < 0).all() and np.array_equal(merge[1:, 1], np.arange(1, nm))
    join = np.concatenate([-merge[0] - 1, -merge[1:, 0] - 1])
    dp = dist[np.ix_(join, join)]
    obs = np.tril(dp, -1).sum(1)[1:] / np.arange(1, nm + 1)
    obs[0] = dp[0, 1]                                     # the first merge reads (first column, second column)
    return np.ones(nm, np.int32), np.arange(1, nm + 1, dtype=np.int32), obs


def dist_perm_sequential(dist, merge, n_perm, z_threshold, rng):
    """the reference's procedure as it stands (:526-626): within a merge the arrangement is carried over from permutation to
    permutation, the uniforms come from rng.random() in call order"""
    dist = np.asarray(dist, np.float64)
    nm = len(merge)
    out = dict(z=np.zeros(nm), n1=np.zeros(nm, np.int32), n2=np.zeros(nm, np.int32))
    for m, (A, n1, n2) in enumerate(merge_members(merge)):
        out["n1"][m], out["n2"][m] = n1, n2
        if n1 <= 1 and n2 <= 1:
            continue
        sub = dist[np.ix_(A, A)]
        obs = sub[:n1, n1:].sum() / (n1 * n2)
        N, ns1 = n1 + n2, min(n1, n2)
        idx = list(range(N))
        vals = np.empty(n_perm)
        for p in range(n_perm):
            u = rng.random(ns1)
            for i in range(ns1):
                k = min(N - i - 1, int(u[i] * (N - i - 1) + 0.5))
                idx[i], idx[i + k] = idx[i + k], idx[i]
            vals[p] = sub[np.ix_(idx[:ns1], idx[ns1:])].sum() / (ns1 * (N - ns1))
        out["z"][m] = _z(obs, vals)[0]
    out["group"] = group_pass(merge, out["z"], z_threshold)
    return out


# ---- groups --------------------------------------------------------------------------------------------------------------------------


def group_pass(merge, z, z_threshold):
    """reference :628-664: int32 [n] group numbers"""
    members = merge_members(merge)
    n = len(merge) + 1
    grp = np.ones(n, np.int32)
    flag = np.zeros(len(merge), bool)
    for m, (a, b) in enumerate(np.asarray(merge)):
        split = z[m] >= z_threshold or (a > 0 and flag[a - 1]) or (b > 0 and flag[b - 1])
        if split:
            flag[m] = True
            A, n1, _ = members[m]
            grp[A[n1:]] += grp[A[:n1]].max()
    return grp


def relabel(group, outlier_n):
    """R/AllUtilities.R:485-510: the factor of group names per sample, as a list of strings"""
    group = np.asarray(group)
    vals, counts = np.unique(group, return_counts=True)
    if np.isfinite(outlier_n):
        small = set(vals[counts <= outlier_n].tolist())
        names = ["Outlier%03d" % g if g in small else "G%03d" % g for g in group]
        n_g, n_o = len(vals) - len(small), len(small)
        new = ["G%03d" % (k + 1) for k in range(n_g)] + ["Outlier%03d" % (k + 1) for k in range(n_o)]
    else:
        names = ["G%03d" % g for g in group]
        new = ["G%03d" % (k + 1) for k in range(len(vals))]
    levels = sorted(set(names))                   # a factor's levels: sorted as strings
    ren = dict(zip(levels, new))
    return [ren[s] for s in names]


def group_dmat(dist, samp_group):
    """(levels, dmat): mean dissimilarity between groups; on the diagonal over the off-diagonal pairs within the group (NaN for a
    group of one); NaN entries dropped (na.rm)"""
    dist = np.asarray(dist, np.float64)
    sg = np.asarray(samp_group)
    levels = sorted(set(sg.tolist()))
    k = len(levels)
    out = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for i in range(k):
            si = sg == levels[i]
            m = dist[np.ix_(si, si)]
            off = m[~np.eye(m.shape[0], dtype=bool)]
            off = off[~np.isnan(off)]
            out[i, i] = off.mean() if off.size else np.nan
            for j in range(i + 1, k):
                v = dist[np.ix_(si, sg == levels[j])].ravel()
                v = v[~np.isnan(v)]
                out[i, j] = out[j, i] = v.mean() if v.size else np.nan
    return levels, out


def clust_count(samp_group, order):
    """table(cluster)[unique(cluster)] with cluster = samp.group[order]: [(name, count)] in order of first appearance"""
    cl = [samp_group[i - 1] for i in order]
    seen = []
    for c in cl:
        if c not in seen:
            seen.append(c)
    return [(c, cl.count(c)) for c in seen]
