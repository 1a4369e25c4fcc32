"""snpgdsMDS on the GPU: the operator q -> B q alone, the dense route, the Krylov route, staging, the ABI's refusals and the API
(tests/mds_ref.py holds the numpy restatement and the inputs; tests/test_cpu_mds.py asserts the inputs' spectra).

Largest deviations seen on one MI355X (the bound in brackets):
  operator      |y - y_ref| 0.034 of its bound 8 n 2^-53 max(|D o D| |J q|), over all sizes, widths, both inputs and memory kinds
  dense route   eigenvalues 1.5e-15 [1e-9], residual 4.7e-15 [1e-7]; planted: 6.2e-14 from 0.95 [1e-9], residual 9.7e-14 [1e-7];
                all eigenvalues 3.4e-13 of lambda_1 (planted, whose other end is -140; else 2.6e-15) [1e-9]; distances of the points
                7.7e-16 of max D [1e-9]; trace 2.7e-16 [1e-12]; GOF 1.1e-15 [4.8e-9 at the least]
  Krylov route  eigenvalues 2.1e-15 [1e-9], residual 6.8e-10 [1e-7]; planted: 4.8e-14, residual 7.9e-14; distances of the points
                1.2e-15 [1e-9]; the two routes' points differ by 4.7e-15 of max |points| [1e-6]
  API           a SNP GDS object against its own snpgdsIBS / snpgdsDiss result: eigenvalues and points equal to the bit [1e-9]"""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import mds_ref as R
from eigen_spectra import EIGENVALUE_BOUND, ORTHO_FACTOR, RESIDUAL_BOUND, SUBSPACE_BOUND, check_topk, reference
from snprelate_amd import _lib, api, snpgdsMDS

pytestmark = pytest.mark.gpu

assert ORTHO_FACTOR > 0 and SUBSPACE_BOUND > 0      # (asserted inside check_topk; imported so that they are not restated)
NOT_POSITIVE = "fewer than k = %d eigenvalues appear to be positive"


# ---- inputs and references, made once ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    D = {"euclid": lambda: R.euclid(n, 3)[0], "ibs_like": lambda: R.ibs_like(n), "nonmetric": lambda: R.nonmetric(n),
         "planted": lambda: R.planted(n)}[kind]()
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def explicit_b(kind, n):
    """(B, eigen_spectra.reference(B)) in numpy"""
    B = R.b_matrix(matrix(kind, n))
    B.setflags(write=False)
    return B, reference(B)


def device_matrix(D, ld, guard=2048):
    """(tensor that owns the memory, address of the matrix, a function that checks matrix and guard words afterwards): the matrix
    with leading dimension ld in device memory, NaN in the padding columns, the last row n long, guard words on either side"""
    import torch
    n = D.shape[0]
    body = np.full((n, ld), np.nan)
    body[:, :n] = D
    body = body.reshape(-1)[:(n - 1) * ld + n]
    raw = np.concatenate([np.full(guard, -7.25), body, np.full(guard, -7.25)])
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()

    def unchanged():
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), raw.view(np.uint64)), "the caller's matrix or its guard words were written"
    return t, int(t.data_ptr()) + 8 * guard, unchanged


def wide_host(D, ld):
    n = D.shape[0]
    w = np.full((n, ld), np.nan)
    w[:, :n] = D
    return w[:, :n]


# ---- 1. the operator alone -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["nonmetric", "ibs_like"])
@pytest.mark.parametrize("n", [2, 3, 15, 16, 17, 63, 64, 65, 257])
def test_operator(kind, n):
    D = matrix(kind, n)
    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for ld in (n, n + 3):
        t, addr, unchanged = device_matrix(D, ld)
        host = wide_host(D, ld)
        assert host.strides[0] == 8 * ld
        for b in (1, 3, 16, 17, 48):
            Q = rng.standard_normal((b, n)) + rng.standard_normal((b, 1))
            y_ref, scale = R.apply_ref(D, Q)
            bound = 8 * n * 2.0 ** -53 * scale.max(axis=1)
            results = [_lib.mds_apply(host, Q), _lib.mds_apply(host, Q), _lib.mds_apply(addr, Q, n=n, ld=ld), _lib.mds_apply(addr, Q, n=n, ld=ld)]
            for y in results:
                err = np.abs(y - y_ref).max(axis=1)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (kind, n, ld, b, float((err / bound).max()))
                assert np.array_equal(y, results[0]), "two products of the same input differ (host / device, first / second run)"
        unchanged()
        del t
    print("operator %s n %d: worst |y - y_ref| / bound %.3f" % (kind, n, worst))


def test_operator_takes_more_vectors_than_one_launch():
    D = matrix("nonmetric", 65)
    Q = np.random.default_rng(5).standard_normal((50, 65))
    y = _lib.mds_apply(D, Q)
    assert np.array_equal(y[:48], _lib.mds_apply(D, Q[:48])) and np.array_equal(y[48:], _lib.mds_apply(D, Q[48:]))


# ---- the checks shared by the two routes ---------------------------------------------------------------------------------------------

def run(kind, n, k, route):
    r = _lib.mds(matrix(kind, n), k)
    assert r["route"] == route, "route %d taken, %d wanted" % (r["route"], route)
    return r


def check_points(kind, n, r):
    D = matrix(kind, n)
    pts = r["vectors"].T * np.sqrt(r["eigval"])
    err = np.abs(R.pairwise(pts) - D).max() / D.max()
    print("%s n %d route %d: distances of the points off by %.1e of max D" % (kind, n, r["route"], err))
    assert err <= 1e-9


def check_planted(n, r):
    B, _ = explicit_b("planted", n)
    w, V = r["eigval"], r["vectors"].T
    dev = np.abs(w - 0.95).max() / 0.95
    res = (np.linalg.norm(B @ V - V * w, axis=0) / np.abs(w)).max()
    print("planted n %d route %d: eigenvalues %.1e from 0.95, residual %.1e" % (n, r["route"], dev, res))
    assert dev <= EIGENVALUE_BOUND and res <= RESIDUAL_BOUND
    assert np.abs(V.T @ V - np.eye(len(w))).max() <= 1e-10


def check_sign_rule(r):
    V = r["vectors"]
    at = np.argmax(np.abs(V), axis=1)
    assert (V[np.arange(len(V)), at] > 0).all()


def check_case(kind, n, k, route):
    r = run(kind, n, k, route)
    check_sign_rule(r)
    tr = R.trace_b(matrix(kind, n))
    print("%s n %d: trace off by %.1e of itself" % (kind, n, abs(r["trace"] - tr) / abs(tr)))
    assert abs(r["trace"] - tr) <= 1e-12 * abs(tr)
    if kind == "euclid":
        check_points(kind, n, r)
    elif kind == "planted":
        check_planted(n, r)
    else:
        B, ref = explicit_b(kind, n)
        check_topk(r["eigval"], r["vectors"].T, B, k, "%s n %d k %d route %d" % (kind, n, k, route), ref)
    return r


DENSE_CASES = [("euclid", 4, 3), ("euclid", 17, 3), ("euclid", 257, 3), ("euclid", 540, 3), ("ibs_like", 540, 1), ("ibs_like", 540, 2),
               ("ibs_like", 540, 5), ("nonmetric", 300, 1), ("nonmetric", 300, 4), ("planted", 300, 3)]
KRYLOV_CASES = [(kind, n, k) for n in (300, 540) for kind, k in
                (("euclid", 3), ("ibs_like", 1), ("ibs_like", 2), ("ibs_like", 5), ("nonmetric", 1), ("nonmetric", 4), ("planted", 3))]


# ---- 2. the dense route --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind, n, k", DENSE_CASES)
def test_dense_route(kind, n, k):
    r = check_case(kind, n, k, 0)
    _, (w_ref, _, _) = explicit_b(kind, n)
    err = np.abs(r["all_eigval"] - w_ref).max() / abs(w_ref[0])
    print("all eigenvalues off by %.1e of lambda_1" % err)
    assert err <= EIGENVALUE_BOUND
    assert np.array_equal(r["all_eigval"][:k], r["eigval"])
    assert r["pos_tol"] == R.pos_tol(matrix(kind, n)) or abs(r["pos_tol"] - R.pos_tol(matrix(kind, n))) <= 1e-12 * r["pos_tol"]


@pytest.mark.parametrize("kind, n, k", [("euclid", 257, 3), ("ibs_like", 540, 2), ("nonmetric", 300, 4)])
def test_dense_api_figures(kind, n, k):
    D = matrix(kind, n)
    c = R.cmdscale(D, k, explicit_b(kind, n)[1][:2])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = snpgdsMDS(D, k=k, verbose=False)
    assert r["route"] == 0 and r["n_pos"] == c["n_pos"] == k and r["points"].shape == (n, k) and r["sample_id"] is None
    assert np.abs(r["eigenval"] - c["eigenval"]).max() <= EIGENVALUE_BOUND * c["eigenval"][0]
    assert abs(r["trace"] - c["trace"]) <= 1e-12 * abs(c["trace"])
    # numerator off by at most k E lambda_1, denominator by n E lambda_1 (E = EIGENVALUE_BOUND): GOF, at most 1, by 2 n E lambda_1 / denominator
    w = c["all_eigval"]
    for i, den in enumerate((np.abs(w).sum(), np.maximum(w, 0).sum())):
        print("%s n %d: GOF[%d] off by %.1e, allowed %.1e" % (kind, n, i, abs(r["GOF"][i] - c["GOF"][i]), 2 * n * EIGENVALUE_BOUND * w[0] / den))
        assert abs(r["GOF"][i] - c["GOF"][i]) <= 2 * n * EIGENVALUE_BOUND * w[0] / den
    scale = np.abs(c["points"]).max()
    assert np.abs(r["points"] - c["points"]).max() <= 1e-6 * scale


def test_dense_one_eigenvalue_more_than_the_rank():
    D = matrix("euclid", 257)
    with pytest.warns(UserWarning, match="only 3 of the first 4 eigenvalues are > 0"):
        r = snpgdsMDS(D, k=4, sample_id=np.arange(257), verbose=False)
    assert r["route"] == 0 and r["n_pos"] == 3 and r["points"].shape == (257, 3) and r["eigenval"].shape == (4,)
    assert np.abs(R.pairwise(r["points"]) - D).max() <= 1e-9 * D.max()
    assert np.abs(r["GOF"] - 1).max() <= 1e-9


def test_dense_all_but_one():
    n = 17
    D = matrix("ibs_like", n)
    r = run("ibs_like", n, n - 1, 0)
    B, (w_ref, _, _) = explicit_b("ibs_like", n)
    V = r["vectors"].T
    assert np.abs(r["eigval"] - w_ref[:n - 1]).max() <= EIGENVALUE_BOUND * w_ref[0]
    assert np.linalg.norm(B @ V - V * r["eigval"], axis=0).max() <= RESIDUAL_BOUND * w_ref[0]      # (one of them is the eigenvalue 0)
    assert np.abs(V.T @ V - np.eye(n - 1)).max() <= 1e-12
    check_sign_rule(r)
    assert D.shape == (n, n)


# ---- 3. the Krylov route -------------------------------------------------------------------------------------------------------------

@pytest.fixture
def krylov(monkeypatch):
    monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "0")


@pytest.mark.parametrize("kind, n, k", KRYLOV_CASES)
def test_krylov_route(krylov, kind, n, k):
    r = check_case(kind, n, k, 1)
    assert r["all_eigval"] is None
    if kind in ("nonmetric", "planted"):
        assert (r["eigval"] > 0).all(), "largest by value, not by magnitude"
    s = _lib.mds_stats()
    assert s["route"] == 1 and s["products"] >= 1 and s["product_ms"] > 0


def test_krylov_fills_all_eigval_with_nan(krylov):
    D = matrix("ibs_like", 300)
    n = 300
    w, v, a = np.zeros(2), np.zeros((2, n)), np.zeros(n)
    route = ctypes.c_int(-1)
    _lib.check(_lib.lib().snpgpu_mds(_lib._ptr(D), n, n, _lib.HOST, 2, _lib._ptr(w), _lib._ptr(v), _lib._ptr(a), None, ctypes.byref(route), 0))
    assert route.value == 1 and np.isnan(a).all()


def test_routes_agree(monkeypatch):
    dense = run("ibs_like", 540, 2, 0)
    monkeypatch.setenv("SNPGPU_EIG_DENSE_MAX", "0")
    kry = run("ibs_like", 540, 2, 1)
    assert np.abs(dense["eigval"] - kry["eigval"]).max() <= EIGENVALUE_BOUND * dense["eigval"][0]
    pd, pk = (r["vectors"].T * np.sqrt(r["eigval"]) for r in (dense, kry))
    err = np.abs(pd - pk).max() / np.abs(pd).max()
    print("the routes' points differ by %.1e of max |points|" % err)
    assert err <= 1e-6


def test_krylov_refuses_an_eigenvalue_that_is_not_positive(krylov):
    D = matrix("euclid", 300)
    with pytest.raises(_lib.SnpGpuError, match=NOT_POSITIVE % 4) as e:
        _lib.mds(D, 4)
    assert "smaller k" in str(e.value)
    check_points("euclid", 300, run("euclid", 300, 3, 1))         # the process and the device stay usable


# ---- 4. staging ----------------------------------------------------------------------------------------------------------------------

def test_staging_windows(monkeypatch):
    n = 257
    D = matrix("ibs_like", n)
    one = _lib.mds(D, 3)
    assert _lib.mds_stats()["windows"] == 1
    Q = np.random.default_rng(9).standard_normal((5, n))
    y_one = _lib.mds_apply(D, Q)
    monkeypatch.setenv("SNPGPU_MDS_STAGE_BYTES", str(8 * n * 100))
    for d in (D, wide_host(D, n + 3)):
        r = _lib.mds(d, 3)
        s = _lib.mds_stats()
        assert s["windows"] >= 2 and s["windows"] == 3
        for key in ("eigval", "vectors", "all_eigval"):
            assert np.array_equal(r[key], one[key]), key
        assert r["trace"] == one["trace"] and r["route"] == one["route"]
        assert np.array_equal(_lib.mds_apply(d, Q), y_one)


# ---- 5. the ABI's refusals -----------------------------------------------------------------------------------------------------------

def raw_mds(D, n, ld, k, mem=_lib.HOST):
    w, v = np.zeros(max(k, 1)), np.zeros((max(k, 1), max(n, 1)))
    return _lib.lib().snpgpu_mds(_lib._ptr(D), n, ld, mem, k, _lib._ptr(w), _lib._ptr(v), None, None, None, 0)


def last_error():
    return _lib.lib().snpgpu_last_error().decode()


@pytest.mark.parametrize("case, text", [
    ("nan", "NA values not allowed in 'd'"), ("inf", "NA values not allowed in 'd'"), ("asym", "must be exactly symmetric"),
    ("k0", "'k' must be in {1, 2, ..  n - 1}"), ("kn", "'k' must be in {1, 2, ..  n - 1}"), ("ld", "ld < n"), ("n1", "at least two"),
    ("null", "NULL argument")])
def test_abi_refusals(case, text):
    n = 70
    D = np.array(matrix("nonmetric", n))
    k, ld, nn = 2, n, n
    if case == "nan":
        D[69, 3] = D[3, 69] = np.nan
    elif case == "inf":
        D[5, 66] = D[66, 5] = np.inf
    elif case == "asym":
        D[68, 1] = np.nextafter(D[1, 68], 2.0)
    elif case == "k0":
        k = 0
    elif case == "kn":
        k = n
    elif case == "ld":
        ld = n - 1
    elif case == "n1":
        nn, ld, k = 1, 1, 1
    rc = raw_mds(None if case == "null" else D, nn, ld, k)
    assert rc != 0 and text in last_error(), last_error()
    if case in ("nan", "inf", "asym"):
        rc = _lib.lib().snpgpu_mds_apply(_lib._ptr(D), n, n, _lib.HOST, _lib._ptr(np.ones((1, n))), 1, _lib._ptr(np.zeros((1, n))), 0)
        assert rc != 0 and text in last_error()
    assert _lib.mds(matrix("nonmetric", n), 2)["route"] == 0              # a following call succeeds


# ---- 6. the API ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["ibs", "diss"])
def test_api_gds_object_against_its_matrix(hapmap, method):
    direct = snpgdsMDS(hapmap, method=method, verbose=False)
    via = snpgdsMDS(api.snpgdsIBS(hapmap, verbose=False) if method == "ibs" else api.snpgdsDiss(hapmap, verbose=False), verbose=False)
    assert direct["route"] == via["route"] == 0 and direct["n_pos"] == via["n_pos"] == 2
    assert np.array_equal(direct["sample_id"], via["sample_id"]) and len(direct["sample_id"]) == direct["points"].shape[0] == 279
    dev = np.abs(direct["eigenval"] - via["eigenval"]).max() / via["eigenval"][0]
    err = np.abs(direct["points"] - via["points"]).max() / np.abs(via["points"]).max()
    print("%s: eigenvalues differ by %.1e of lambda_1, points by %.1e of max |points|" % (method, dev, err))
    assert dev <= EIGENVALUE_BOUND and err <= 1e-9
    assert abs(direct["trace"] - via["trace"]) <= 1e-12 * abs(via["trace"]) and np.abs(direct["GOF"] - via["GOF"]).max() <= 1e-9


def test_api_device_tensor_and_numpy_array():
    import torch
    D = matrix("ibs_like", 257)
    a = snpgdsMDS(D, k=3, sample_id=np.arange(257), verbose=False)
    t = torch.from_numpy(np.array(D)).cuda()
    b = snpgdsMDS(t, k=3, sample_id=np.arange(257), verbose=False)
    for key in ("points", "eigenval", "GOF", "sample_id"):
        assert np.array_equal(a[key], b[key]), key
    assert a["trace"] == b["trace"] and a["n_pos"] == b["n_pos"] == 3 and a["route"] == b["route"] == 0
    assert torch.equal(t.cpu(), torch.from_numpy(np.array(D)))           # the caller's tensor is unchanged
