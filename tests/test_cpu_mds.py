"""snpgdsMDS without a GPU: the numpy restatement of classical scaling (tests/mds_ref.py) on inputs whose answer is known, the
properties of the four inputs that the GPU tests lean on (so that another seed which breaks them fails here), the host-side refusals
of snpgdsMDS -- none of which may touch the library -- and the new names in the header and the binding."""
import os

import numpy as np
import pytest

import mds_ref as R
import mem_kinds as M
from conftest import ROOT
from snprelate_amd import _lib, api, snpgdsMDS

HEADER = os.path.join(ROOT, "include", "snpgpu.h")
NAMES = ("snpgpu_mds", "snpgpu_mds_apply", "snpgpu_gnrMDS", "snpgpu_mds_stats")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 17, 257, 540])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_restatement_recovers_euclidean_points(n, p):
    D, X = R.euclid(n, p)
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    B = R.b_matrix(D)
    assert np.abs(B - X @ X.T).max() <= 1e-12 * np.abs(B).max()
    w, q = R.eigh_desc(B)
    c = R.cmdscale(D, p, (w, q))
    assert c["n_pos"] == p and c["points"].shape == (n, p)
    err = np.abs(R.pairwise(c["points"]) - D).max() / D.max()
    print("n %d p %d: distances reproduced to %.1e of max D, eigenvalue p + 1 = %.1e lambda_1" % (n, p, err, w[p] / w[0]))
    assert err <= 1e-12
    assert abs(w[p]) <= 1e-12 * w[0]
    assert abs(c["trace"] - np.trace(B)) <= 1e-12 * abs(np.trace(B))
    # both figures of the goodness of fit are 1 at k = p
    assert np.abs(c["GOF"] - 1).max() <= 1e-12


def test_one_more_than_the_rank_is_not_positive():
    D, _ = R.euclid(257, 3)
    c = R.cmdscale(D, 4)
    assert c["n_pos"] == 3 and c["points"].shape == (257, 3) and c["eigenval"].shape == (4,)
    assert abs(c["eigenval"][3]) <= R.pos_tol(D)           # whatever its sign


def test_sign_rule():
    V = np.array([[0.5, -0.5, 0.1], [-0.7, 0.5, -0.9], [0.2, 0.1, 0.9]])
    S = R.sign_rule(V)
    assert np.array_equal(S[:, 0], -V[:, 0])                 # largest magnitude -0.7: flipped
    assert np.array_equal(S[:, 1], -V[:, 1])                 # a tie of -0.5 (index 0) and 0.5: the lowest index decides
    assert np.array_equal(S[:, 2], -V[:, 2])                 # a tie of -0.9 (index 1) and 0.9
    assert np.array_equal(R.sign_rule(S), S)
    D = R.ibs_like(60, 300)
    c = R.cmdscale(D, 3)
    for j in range(3):
        assert c["vectors"][np.argmax(np.abs(c["vectors"][:, j])), j] > 0


def test_apply_ref_is_b_times_q():
    D = R.nonmetric(65)
    Q = np.random.default_rng(3).standard_normal((5, 65))
    y, bound = R.apply_ref(D, Q)
    assert np.abs(y - Q @ R.b_matrix(D)).max() <= 1e-12 * np.abs(y).max()
    assert bound.shape == y.shape and (bound > 0).all()


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------

def test_ibs_like_is_not_euclidean_and_has_two_leading_eigenvalues():
    D = R.ibs_like(540)
    assert np.array_equal(D, D.T) and not D.diagonal().any() and np.isfinite(D).all()
    f = R.spectrum_figures(D)
    print("ibs_like(540): %d of %d eigenvalues negative, smallest %.2e lambda_1, leading gaps %s" %
          (f["negative"], f["n"], f["smallest"], " ".join("%.1e" % g for g in f["gaps"])))
    assert f["negative"] >= 50 and f["smallest"] <= -5e-3
    assert min(f["gaps"][:2]) >= 0.1                          # two population axes stand clear ...
    assert 2e-4 <= min(f["gaps"][2:6]) and max(f["gaps"][2:6]) <= 5e-3      # ... of a crowded bulk, no gap at eigen_spectra's 1e-4


def test_nonmetric_is_half_negative():
    for n in (300, 540):
        D = R.nonmetric(n)
        assert np.array_equal(D, D.T) and not D.diagonal().any()
        f = R.spectrum_figures(D)
        print("nonmetric(%d): %d negative, smallest %.2f lambda_1, leading gaps %s" %
              (n, f["negative"], f["smallest"], " ".join("%.1e" % g for g in f["gaps"][:5])))
        assert f["negative"] >= n // 3 and f["smallest"] <= -0.5
        assert min(f["gaps"][:5]) >= 1e-3


def test_planted_has_one_positive_eigenvalue_of_multiplicity_n_minus_2():
    for n in (300, 540):
        D = R.planted(n)
        w = R.spectrum_figures(D)["w"]
        assert np.abs(w[:n - 2] - 0.95).max() <= 1e-12 and abs(w[n - 2]) <= 1e-10 and w[n - 1] < -100
        print("planted(%d): 0.95 x %d, %.1e, %.1f" % (n, n - 2, w[n - 2], w[n - 1]))


# ---- host-side refusals: before the library is touched -------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "mds", boom)
    monkeypatch.setattr(_lib, "gnr_mds", boom)
    monkeypatch.setattr(api, "_init_file2", boom)


K_TEXT = r"'k' must be in \{1, 2, \.\.  n - 1\}"
D5 = R.nonmetric(5)


def _with(i, j, v):
    d = D5.copy()
    d[i, j] = v
    return d


@pytest.mark.parametrize("kwargs, exc, text", [
    (dict(obj=np.zeros((4, 5))), ValueError, "square matrix"),
    (dict(obj=np.zeros(9)), ValueError, "square matrix"),
    (dict(obj=np.zeros((1, 1)), k=1), ValueError, "'d' must have at least two rows"),
    (dict(obj=D5, k=0), ValueError, K_TEXT),
    (dict(obj=D5, k=5), ValueError, K_TEXT),
    (dict(obj=D5, k=-1), ValueError, K_TEXT),
    (dict(obj=D5, k=1.5), ValueError, K_TEXT),
    (dict(obj=D5, method="king"), ValueError, "'method' should be one of \"ibs\", \"diss\""),
    (dict(obj=D5, sample_id=list("abcd")), ValueError, r"nrow\(dist\) == length\(sample.id\) is not TRUE"),
    (dict(obj=_with(1, 2, np.nan)), ValueError, "NA values not allowed in 'd'"),
    (dict(obj=_with(4, 0, np.inf)), ValueError, "NA values not allowed in 'd'"),
    (dict(obj=dict(sample_id=list("abcde"), ibs=_with(0, 3, np.nan))), ValueError, "NA values not allowed in 'd'"),
    (dict(obj=dict(sample_id=list("abcde"), diss=D5), k=5), ValueError, K_TEXT),
    (dict(obj=dict(sample_id=list("abcde"), kinship=D5)), TypeError, "snpgdsDiss or snpgdsIBS result"),
])
def test_host_side_refusals(no_library, kwargs, exc, text):
    with pytest.raises(exc, match=text):
        snpgdsMDS(**kwargs)


def test_refusals_of_a_gds_object_come_before_the_working_space(no_library):
    from snprelate_amd.gds import GenoFile
    g = GenoFile.__new__(GenoFile)
    with pytest.raises(ValueError, match="'method' should be one of"):
        snpgdsMDS(g, method="IBS")
    with pytest.raises(ValueError, match=K_TEXT):
        snpgdsMDS(g, k=0)


# ---- the header and the binding ------------------------------------------------------------------------------------------------------

def test_names_in_header_and_exports():
    protos = M.header_prototypes(open(HEADER).read())
    for f in NAMES:
        assert f in protos and f in _lib.EXPORTS, f
    assert protos["snpgpu_mds"] == ["dist", "n", "ld", "mem", "k", "eigval", "vectors", "all_eigval", "trace_b", "route", "device"]
    assert protos["snpgpu_mds_apply"] == ["dist", "n", "ld", "mem", "Q", "b", "Y", "device"]
    assert protos["snpgpu_gnrMDS"] == ["what", "k", "eigval", "vectors", "all_eigval", "trace_b", "route"]
    assert protos["snpgpu_mds_stats"] == ["stats"]


def test_results_are_host_memory_only():
    protos = M.header_prototypes(open(HEADER).read())
    for f in NAMES:
        assert "out_mem" not in protos[f] and "dst_mem" not in protos[f]
        assert protos[f][0] not in ("ctx", "m")
    assert "#define SNPGPU_ABI_VERSION 2\n" in open(HEADER).read()          # additions only: the version stays
    assert snpgdsMDS.__defaults__[:2] == (2, "ibs")
