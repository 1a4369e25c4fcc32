"""GPU tests of the second trip of the four host loops that a fixed device budget bounds and no switch shrinks: the row panels of
the full LD matrix (ld.hip), the row slabs and grid-stride loops of the GRM merge (grm_merge.hip), the window launches of the W&H02
scan (pop.hip) and the staged row copies of a host distance matrix (tree.hip).  Thin shapes reach the default budgets: few samples,
since the work of these routes grows with the sample count and not with the trip count.

Every test proves from the call's own counters that the second trip happened (snpgpu_ld_get_timing, snpgpu_grm_merge_stats, slot 4
of snpgpu_pop_stats, snpgpu_tree_stats).  No budget formula is restated here: if a budget grows and a route goes back to one trip,
the counter assertion fails instead of the test going blind."""
import numpy as np
import pytest

import fst_ref
import ld_ref
import oracle
import tree_ref
from mem_kinds import DeviceDest
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows
from test_gpu_fst import _genotypes, _within
from test_gpu_ld import CODES, _check
from test_gpu_tree import caterpillar

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_inputs():
    """inputs and references that several tests share are computed once, left unchanged, and dropped after the module"""
    yield
    _cache.clear()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. the full LD matrix in two row panels ------------------------------------------------------------------------------------------
LD_N, LD_L = 100, 4992
LD_ROWS = np.r_[0:64, 4800:4992]          # a stripe at the top and one that holds the boundary between the two panels


def _ld_case():
    """(2-bit rows, polymorphic flags, int64 tables of LD_ROWS x all SNPs with each pair oriented (lower index, higher index), as
    the reference evaluates each unordered pair once); computed once"""
    if "ld" not in _cache:
        packed = synth_hash_block_packed(LD_N, 0, LD_L, 7, 0.03, spectrum=4, special=True)
        g = unpack_2bit_rows(packed, LD_N)
        poly = np.array([len(np.unique(r[r < 3])) > 1 for r in g])
        t = ld_ref.tables(g[LD_ROWS], g)
        below = LD_ROWS[:, None] > np.arange(LD_L)[None, :]
        t[below] = t[below].transpose(0, 2, 1)
        _cache["ld"] = (packed, poly, t)
    return _cache["ld"]


def _ld_run(packed, method, out_ptr=None):
    """(matrix or None, launches of the table kernel, of the finaliser, copies of the result)"""
    with _lib.LDMatrix(LD_N, LD_L, CODES[method], -1, False) as ld:
        ld.set_timing(True)
        ld.feed(packed, _lib.GENO_PACKED2)
        m = ld.result(out_ptr=out_ptr)
        return m, [ld.get_timing(which)[1] for which in range(3)]


@pytest.mark.parametrize("method", ld_ref.METHODS)
def test_ld_full_matrix_in_two_row_panels(method):
    packed, poly, tab = _ld_case()
    assert (~poly).any() and poly[:64].any() and poly[-64:].any()      # planted monomorphic / all-missing rows; both ends polymorphic
    m, launches = _ld_run(packed, method)
    assert launches == [2, 2, 2], launches                             # the second trip
    # the whole matrix against its transpose, bit for bit: crosses the panel boundary in both directions
    base = m.T                                                         # the C-contiguous array the call wrote
    assert base.flags["C_CONTIGUOUS"] and base.shape == (LD_L, LD_L)
    nan = np.isnan(base)
    assert np.array_equal(nan, nan.T), method
    assert ((base.view(np.uint64) == base.T.view(np.uint64)) | nan).all(), method
    # the two stripes over all columns against the restatement
    _check(m[LD_ROWS], ld_ref.ld_values(tab, method), method)
    if method == "corr":
        # row 0 lies in the first panel and row L - 1 in the last whatever the panel height
        dev = np.abs(np.diag(m)[poly] - 1.0)
        print("corr: max |diagonal - 1| at %d polymorphic SNPs %.3e" % (poly.sum(), dev.max()))
        assert (dev <= 1e-12).all()
        assert np.isnan(np.diag(m)[~poly]).all()


def test_ld_two_row_panels_into_device_memory():
    packed, _, _ = _ld_case()
    host, launches = _ld_run(packed, "composite")
    assert launches == [2, 2, 2], launches
    dest = DeviceDest((LD_L, LD_L), np.float64, 1)
    none, launches = _ld_run(packed, "composite", out_ptr=dest.ptr)
    assert none is None and launches == [2, 2, 2], launches
    got = dest.read()                                                  # checks the guards before and after the result
    assert _bits_equal(got, host.T)


# ---- 2. the GRM merge: grid-stride loops and row slabs --------------------------------------------------------------------------------
BETA = ":method = IndivBeta"
# (N, weights, avg_val of the inputs, slabs per input and pass, rows that get a unique large entry)
MERGE_CASES = {
    # one slab; N^2 elements are more than one pass of the largest grid, the element after it is (2047, 1)
    2049: ((0.5, 0.75, -0.25), (0.11, 0.07, 0.2), 1, (2046, 2047, 2048)),
    # two slabs, the second of 15 rows: 5784 is the last row of the first, 5785 the first of the second
    5800: ((0.25, 0.75), (0.11, 0.07), 2, (5784, 5785, 5799)),
}


def _merge_inputs(N):
    """symmetric matrices of entries k / 256 with integer |k| <= 2^15, so that every sum of entries and every weighted sum with
    these weights is exact in fp64 in any order; + 1000 on the diagonal (a misplaced diagonal shows); a unique large entry in each
    row next to a slab boundary and in the last row; the entry that makes the global minimum of the merged matrix at (N - 1, N - 2)
    and its mirror image, both in the last rows of the last slab"""
    if ("merge", N) in _cache:
        return _cache[("merge", N)]
    weight, avg_in, _, rows = MERGE_CASES[N]
    rng = np.random.default_rng(N)
    grms = []
    for w in weight:
        r = rng.integers(-2048, 2049, (N, N), dtype=np.int32)
        r += r.T.copy()                                                 # |k| <= 4096
        sign = 1 if w > 0 else -1
        for q, i in enumerate(rows):
            r[i, 3 + 2 * q] = r[3 + 2 * q, i] = sign * (25600 + 1024 * q)      # raises M there: 100, 104, 108
        r[N - 1, N - 2] = r[N - 2, N - 1] = -sign * 32768                      # lowers M there: -128
        g = r.astype(np.float64)
        g *= 1.0 / 256
        g[np.arange(N), np.arange(N)] += 1000.0
        g.setflags(write=False)
        grms.append(g)
    _cache[("merge", N)] = (grms, np.array(weight), np.array(avg_in))
    return _cache[("merge", N)]


def _merge_beta_bounds(grms, weight, avg_in):
    """(bound on |got - ref| per element, bound on the merged avg_val) of the beta merge, from the restatement's own values.

    Mb of an input is a sum of entries k / 256: exact on both sides, the same bits.  Each term w (x + a) of an element of the merged
    M, x = (g / 2 - Mb) / (1 - Mb) (1 - a), takes at most 9 roundings on the device (g / 2 - Mb; 1 - Mb and its reciprocal; two
    products; 1 - a; + a; the weight; the accumulation) and 8 in numpy, each relative to a magnitude of at most
    mag = sum |w| (|x| + |a|) over the inputs: dM <= 20 u mag, the spare 3 u for the second-order terms.  The minimum mn is the
    planted entry on both sides (asserted: it is far below every other), so its error is dM there.  Through the final map
    v = (M - mn) 2 / (1 - mn): scale (dM + dmn) for the difference, |v| (dmn / (1 - mn) + 4 u) for the scale's own error and the
    roundings, and the diagonal's v / 2 + 1 halves that and rounds once more.
    avg_val is the one reduction whose order the device does not fix (atomic partial sums over the N (N - 1) entries off the
    diagonal): the worst-case bound of a sum of n terms in any order, (n - 1) u sum |M|, for either side, plus the entries' dM."""
    N = grms[0].shape[0]
    diag = np.arange(N)
    m, mag = np.zeros((N, N)), np.zeros((N, N))
    for g, w, a in zip(grms, weight, avg_in):
        mb = (g.sum() - np.trace(g)) / (N * (N - 1)) * 0.5             # exact sums
        x = (g * 0.5 - mb) / (1 - mb) * (1 - a)
        x[diag, diag] = (np.diag(g) - 1 - mb) / (1 - mb) * (1 - a)
        m += (x + a) * w
        np.abs(x, out=x)
        x += abs(a)
        x *= abs(w)
        mag += x
    dM = mag
    dM *= 20 * U
    i, j = np.unravel_index(np.argmin(m), m.shape)
    assert {int(i), int(j)} == {N - 1, N - 2}
    mn, dmn = m[i, j], dM[i, j]
    m[i, j] = m[j, i] = np.inf
    assert m.min() - mn > 1.0                                          # no other entry can become the minimum
    m[i, j] = m[j, i] = mn
    scale = 2 / (1 - mn)
    bound = np.abs(m - mn) * (scale * (dmn / (1 - mn) + 4 * U)) + scale * (dM + dmn)
    bound[diag, diag] = bound[diag, diag] * 0.5 + U * (np.abs(m[diag, diag] - mn) * (scale * 0.5) + 1)
    np.abs(m, out=m)
    m[diag, diag] = 0
    dM[diag, diag] = 0
    avg_bound = (dM.sum() + 2.0 * N * N * U * m.sum()) / (N * (N - 1.0))
    return bound, avg_bound


@pytest.mark.parametrize("N", sorted(MERGE_CASES))
def test_grm_merge_weighted_sum_over_slabs_and_strides(N):
    weight, _, slabs, _ = MERGE_CASES[N]
    grms, w, _ = _merge_inputs(N)
    got, avg = _lib.grm_merge(grms, w)
    st = _lib.grm_merge_stats()
    assert st == dict(slabs=slabs * len(weight), launches=slabs * len(weight)), st      # the second trip: one pass over the inputs
    ref, _ = oracle.grm_merge(grms, w)
    assert avg is None and _bits_equal(got, ref)


@pytest.mark.parametrize("N", sorted(MERGE_CASES))
def test_grm_merge_beta_over_slabs_and_strides(N):
    weight, _, slabs, _ = MERGE_CASES[N]
    grms, w, avg_in = _merge_inputs(N)
    got, avg = _lib.grm_merge(grms, w, BETA, avg_in)
    st = _lib.grm_merge_stats()
    assert st == dict(slabs=2 * slabs * len(weight), launches=2 * slabs * len(weight) + 2), st     # two passes over the inputs
    ref, ref_avg = oracle.grm_merge(grms, w, BETA, avg_in)
    bound, avg_bound = _merge_beta_bounds(grms, w, avg_in)
    err = np.abs(got - ref)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print("N = %d: max |diff| %.3e (bound there %.3e), largest diff / bound %.3e at %s; avg_val diff %.3e, bound %.3e"
          % (N, err.max(), bound[np.unravel_index(np.argmax(err), err.shape)], (err / bound).max(), worst, abs(avg - ref_avg),
             avg_bound))
    assert np.isfinite(got).all() and (err <= bound).all()
    assert abs(avg - ref_avg) <= avg_bound
    # exactly 0 at the planted minimum and its mirror image, and at no other entry off the diagonal (the diagonal is >= 1)
    zero = {(int(i), int(j)) for i, j in np.argwhere(got == 0)}
    assert zero == {(N - 1, N - 2), (N - 2, N - 1)}, sorted(zero)[:10]
    assert (np.diag(got) >= 1).all()


# ---- 3. the W&H02 sliding windows in two launches -------------------------------------------------------------------------------------
FST_N, FST_K, FST_M = 80, 40, 5300
FST_SPLIT = 2650


def _fst_case():
    """(2-bit rows, pop, offsets, snp_index, members): window w holds SNPs [w, min(w + 3, M)), but 5241 is empty, 5242 holds one
    SNP and 5243 three SNPs far from its neighbours' and from each other (ascending, as the interface requires of every window:
    an unsorted window is an argument error), so that the index list as a whole is not sorted"""
    if "fst" not in _cache:
        g, pop = _genotypes(FST_N, FST_M, FST_K, 0.08, seed=40)
        assert np.array_equal(np.unique(pop), np.arange(FST_K))
        members = [np.arange(w, min(w + 3, FST_M)) for w in range(FST_M)]
        members[5241] = np.array([], np.int64)
        members[5242] = np.array([5242])
        members[5243] = np.array([2, 2651, 5299])
        offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
        idx = np.concatenate(members).astype(np.int32)
        assert (np.diff(idx) < 0).any()
        a, c = fst_ref.pop_counts(g, pop, FST_K)
        _cache["fst"] = (pack_2bit_rows(g), pop, offsets, idx, members, a, c)
    return _cache["fst"]


@pytest.mark.parametrize("method", ["W&C84", "W&H02"])
def test_fst_windows_in_two_launches(method):
    packed, pop, offsets, idx, members, a, c = _fst_case()
    code = _lib.FST_WC84 if method == "W&C84" else _lib.FST_WH02
    wh = method == "W&H02"

    def run(w0, w1):
        f, per, beta = _lib.fst_windows(packed, FST_N, pop, FST_K, offsets[w0:w1 + 1] - offsets[w0], idx[offsets[w0]:offsets[w1]], code)
        return f, per, beta, _lib.pop_stats()[4]

    f, per, beta, launches = run(0, FST_M)
    assert launches == (2 if wh else 0)                                # the second trip; W&C84 sums in one launch: the control
    parts = [run(0, FST_SPLIT), run(FST_SPLIT, FST_M)]
    assert [p[3] for p in parts] == ([1, 1] if wh else [0, 0])
    # the whole scan equals two single-launch scans byte for byte, the NaN of the empty window included
    assert _bits_equal(f, np.concatenate([p[0] for p in parts]))
    assert np.isnan(f[5241]) and not np.isnan(f).all()
    for p in parts:
        assert _bits_equal(per, p[1])
    if wh:
        assert beta.shape == (FST_M, FST_K, FST_K) and _bits_equal(beta, np.concatenate([p[2] for p in parts]))
    else:
        assert beta is None
    # the windows at either end of the scan, the special ones among them, against the restatement
    for w in list(range(0, 8)) + list(range(5230, FST_M)):
        r = fst_ref.fst_set(a, c, method, members[w])
        _within(f[w], r["Fst"], r["Fst_bound"], "window %d" % w)
        if wh:
            _within(beta[w], r["Beta"], r["Beta_bound"], "window %d beta" % w)


# ---- 4. the permutation test with a host matrix staged in two copies -------------------------------------------------------------------
TREE_N = 5800
TREE_PERM = 50                             # the fewest the interface accepts; every merge above the first is a light one here


def test_dist_perm_host_matrix_staged_in_two_copies():
    import torch
    n = TREE_N
    d = np.triu(np.random.default_rng(58).uniform(0.1, 0.9, (n, n)), 1)
    d += d.T.copy()
    merge = caterpillar(n, 59)
    before = d.copy()
    host = _lib.dist_perm(d, merge, n_perm=TREE_PERM, z_threshold=15.0, seed=11)
    assert _lib.tree_stats()["prep_launches"] == 3                     # the second trip: two gathers and the row sums
    t = torch.from_numpy(d).cuda()
    dev = _lib.dist_perm(int(t.data_ptr()), merge, n_perm=TREE_PERM, z_threshold=15.0, seed=11, n=n)
    assert _lib.tree_stats()["prep_launches"] == 2                     # a device matrix is gathered where it lies
    for k in host:
        assert _bits_equal(host[k], dev[k]), k
    assert np.array_equal(d, before) and torch.equal(t.cpu(), torch.from_numpy(before))
    del t, before
    n1, n2, obs = tree_ref.caterpillar_obs(d, merge)
    assert np.array_equal(host["n1"], n1) and np.array_equal(host["n2"], n2)
    tol = 4.0 * n * n * U * np.abs(obs)
    err = np.abs(host["obs"] - obs)
    print("n = %d: max |obs diff| %.3e, bound there %.3e, largest diff / bound %.3e"
          % (n, err.max(), tol[np.argmax(err)], (err / tol).max()))
    assert (err <= tol).all()
    heavy = (n1 + n2) > 2
    assert np.isfinite(host["z"]).all() and np.isfinite(host["perm_mean"][heavy]).all() and np.isfinite(host["perm_sd"][heavy]).all()
