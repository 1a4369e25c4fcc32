"""The inputs and the comparison of tests/test_gpu_eigen_spectra.py cannot pass vacuously (no GPU): the constructions of
tests/eigen_spectra.py give exactly block-diagonal matrices with exactly multiple eigenvalues and wide gaps between the clusters in the
CPU oracle, the near-degenerate form spreads the clusters far less than the gaps, and check_topk passes on numpy's own eigenpairs and
fails on each of the block-Lanczos failures it is there for -- a missed copy of a multiple eigenvalue, a vector returned twice,
vectors of a cluster that are not orthogonal -- every one of them made of eigenpairs with tiny residuals."""
import functools

import numpy as np
import pytest

import eigen_spectra as E
import oracle as orc

KINDS = ("PCA_COV", "GRM_GCTA")


@functools.lru_cache(maxsize=None)
def _matrix(name, kind, near=False):
    g, perm = E.size_geno(name, near)
    n = g.shape[1]
    if kind == "PCA_COV":
        tri = orc.pca_cov(g)
        orc.trace_normalize(tri, n)
    else:
        tri = orc.grm_gcta(g)
    full = orc.tri_to_full(tri, n)
    full.setflags(write=False)
    return full, perm


@functools.lru_cache(maxsize=None)
def _reference(name, kind, near=False):
    return E.reference(_matrix(name, kind, near)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(E.SIZES))
def test_exact_construction(name, kind):
    m, L1, copies, _ = E.SIZES[name]
    g, perm = E.size_geno(name)
    assert g.shape == (copies * L1, copies * m) and g.max() == 2
    assert np.all((g == 0).sum(1) == (g == 2).sum(1)) and np.all((g != 1).any(1))          # p = 0.5, every SNP polymorphic
    assert sorted(perm.tolist()) == list(range(copies * m))
    blk = perm // m                     # the copies are interleaved: every row panel of 256 samples holds samples of every copy
    assert all(len(set(blk[r0:r0 + 256].tolist())) == copies for r0 in range(0, copies * m, 256) if copies * m - r0 >= 16)
    full, _ = _matrix(name, kind)
    assert E.off_block_max(full, perm, m) == 0.0
    w = _reference(name, kind)[0]
    spread, gap, mult = E.cluster_figures(w)
    print("%s %s: multiplicities %s, spread inside a cluster %.1e, smallest gap between clusters %.2e of the largest eigenvalue"
          % (name, kind, mult, spread, gap))
    assert set(mult) == {copies} and spread <= 1e-12 and gap >= 5e-3
    # every k of the GPU tests against these clusters: ends of clusters and inside them
    cuts = [E.clusters(w, k)[1] for k in (1, 2, 3, 4, 7, 16)]
    assert cuts == ([True, False, True, False, True, False] if copies == 2 else [True, True, False, True, True, True])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(E.SIZES))
def test_near_degenerate_construction(name, kind):
    m = E.SIZES[name][0]
    edits, missing, _ = E.NEAR[name]
    g0, perm = E.size_geno(name)
    g1, perm1 = E.size_geno(name, near=True)
    diff = g0 != g1
    assert np.array_equal(perm, perm1) and diff.sum() == edits + missing and (g1 == 3).sum() == missing
    assert set((perm[np.nonzero(diff)[1]] // m).tolist()) == {0}                           # in one copy only
    spread, gap = E.near_figures(_reference(name, kind)[0], _reference(name, kind, True)[0])
    print("%s %s near-degenerate: clusters spread by %.1e, smallest gap %.2e of the largest eigenvalue (ratio %.1f)"
          % (name, kind, spread, gap, gap / spread))
    assert 1e-6 < spread <= gap / 10


def test_clusters():
    w = np.array([5.0, 5.0 - 1e-7, 5.0 - 2e-7, 3.0, 3.0, 2.0, 1.0])
    assert E.clusters(w, 1) == ([(0, 3)], True) and E.clusters(w, 3) == ([(0, 3)], False)
    assert E.clusters(w, 4) == ([(0, 3), (3, 5)], True) and E.clusters(w, 6) == ([(0, 3), (3, 5), (5, 6)], False)
    assert E.clusters(w, 7)[0][-1] == (6, 7)
    assert E.clusters(w, 2, rel=1e-9) == ([(0, 1), (1, 2)], False)                          # a chain of close neighbours is one cluster
    assert E.clusters(np.array([5.0, 4.9996, 4.9992, 1.0]), 1) == ([(0, 3)], True)


@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(E.SIZES))
def test_check_passes_on_numpys_own_pairs(name, kind, near):
    full = _matrix(name, kind, near)[0]
    ref = _reference(name, kind, near)
    for k in (1, 2, 3, 4, 7, 16, full.shape[0] // 3):
        f = E.check_topk(ref[0][:k], ref[1][:, :k], full, k, "%s %s k=%d" % (name, kind, k), ref=ref)
        assert f["ortho"] <= ref[2]


def _triple():
    """the n = 210 covariance: triples; k = 7 holds two whole clusters and cuts the third"""
    full = _matrix("n210", "PCA_COV")[0]
    ref = _reference("n210", "PCA_COV")
    k = 7
    return full, ref, k, ref[0][:k].copy(), ref[1][:, :k].copy()


def test_check_fails_on_a_missed_copy():
    """the third copy of the first triple is missed and the next cluster's pairs move up: every returned pair is a true eigenpair,
    orthonormal, with a residual at rounding -- only the eigenvalues counted WITH multiplicity, and the subspaces, see it"""
    full, ref, k, w, V = _triple()
    w = np.r_[w[:2], ref[0][3:8]]
    V = np.c_[V[:, :2], ref[1][:, 3:8]]
    f = E.figures(w, V, full, k, ref)
    assert f["residual"] < 1e-13 and f["ortho"] <= ref[2] and f["descending"]
    assert f["eigenvalues"] >= 5e-3 and f["inside"] < 1e-6
    with pytest.raises(AssertionError, match="with multiplicity"):
        E.check_topk(w, V, full, k, ref=ref)


def test_check_fails_on_a_vector_returned_twice():
    full, ref, k, w, V = _triple()
    V[:, 2] = V[:, 1]
    f = E.figures(w, V, full, k, ref)
    assert f["eigenvalues"] < 1e-14 and f["residual"] < 1e-13 and f["inside"] > 1 - 1e-12         # nothing else notices
    assert f["ortho"] > 0.99 and f["span"] < 1e-6
    with pytest.raises(AssertionError, match="orthonormality"):
        E.check_topk(w, V, full, k, ref=ref)


@pytest.mark.parametrize("factor", [10.0, 0.1])
def test_orthonormality_bound_bites(factor):
    """two vectors of the second triple replaced by mixtures of each other with an inner product of `factor` times the bound: ten
    times the bound fails, on orthonormality alone; a tenth of it passes"""
    full, ref, k, w, V = _triple()
    eps = 0.5 * factor * E.ORTHO_FACTOR * ref[2]
    a, b = V[:, 3].copy(), V[:, 4].copy()
    V[:, 3] = (a + eps * b) / np.sqrt(1 + eps * eps)
    V[:, 4] = (b + eps * a) / np.sqrt(1 + eps * eps)
    f = E.figures(w, V, full, k, ref)
    assert f["eigenvalues"] < 1e-14 and f["residual"] < 1e-10 and f["inside"] > 1 - 1e-12 and f["span"] > 1 - 1e-9
    assert abs(f["ortho"] / (factor * E.ORTHO_FACTOR * ref[2]) - 1) < 0.05
    if factor > 1:
        with pytest.raises(AssertionError, match="orthonormality"):
            E.check_topk(w, V, full, k, ref=ref)
    else:
        E.check_topk(w, V, full, k, ref=ref)


def test_check_fails_on_values_out_of_order_and_on_a_vector_of_the_wrong_cluster():
    full, ref, k, w, V = _triple()
    with pytest.raises(AssertionError, match="descending"):
        E.check_topk(w[::-1], V[:, ::-1], full, k, ref=ref)
    # the last vector belongs to the cluster that k cuts: one of the NEXT cluster in its place has the right residual, not the subspace
    w[6], V[:, 6] = ref[0][9], ref[1][:, 9]
    f = E.figures(w, V, full, k, ref)
    assert f["residual"] < 1e-13 and f["inside"] < 1e-6 and f["cut"]


def test_fuzz_generator_is_deterministic():
    from oracle.synth import synth_geno
    a = E.fuzz_case(np.random.default_rng(5), synth_geno)
    b = E.fuzz_case(np.random.default_rng(5), synth_geno)
    assert a["g"].shape == (a["L"], a["n"]) and np.array_equal(a["g"], b["g"]) and a["kind"] == b["kind"] and 1 <= a["k"] <= 32
