"""What the GPU tests of the EM for ancestry proportions lean on, shown without a GPU: the numpy restatement (tests/admix_ref.py) on
its own -- float64 against long double under a permuted summation order, a likelihood that never decreases, supervised estimates
nearer the truth than 1 / K --, snpgdsAdmixProp against a line-by-line restatement of R/PCA.R:389-422, snpgdsAdmixTable on a
hand-made matrix, and every refusal of include/snpgpu.h section 1s and of snpgdsAdmix that is made before any HIP call."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import admix_ref as R
import mem_kinds as M
from conftest import GOLDEN, ROOT
from snprelate_amd import _lib, api

LD = np.longdouble
HEADER = os.path.join(ROOT, "include", "snpgpu.h")
NAMES = ["snpgpu_admix_create", "snpgpu_admix_feed", "snpgpu_admix_set", "snpgpu_admix_run", "snpgpu_admix_get", "snpgpu_admix_stats",
         "snpgpu_admix_destroy", "snpgpu_gnrAdmix"]
F_MIN = 1e-6


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_150():
    c = R.admixed_case(150, 700, 3, 5)
    c["geno"].setflags(write=False)
    return c


@pytest.mark.parametrize("shape", [(150, 700, 3), (257, 17, 5), (15, 700, 16), (4, 4, 2)])
def test_float64_against_long_double_under_a_permutation(shape):
    n, m, K = shape
    G = R.admixed_case(n, m, K, 11 + n + m)["geno"]
    Q, F = R.awkward_state(n, m, K, 9, F_MIN)
    rng = np.random.default_rng(3)
    a = R.em_step(G, Q, F, F_MIN, np.float64, order=(rng.permutation(n), rng.permutation(m)))
    b = R.em_step(G, Q, F, F_MIN, LD)
    Ti, Tj, T = R.called_counts(G)
    assert R.worst(a["a"], b["a"], R.sum_bound(Ti, K)[:, None]) <= 1.0
    assert R.worst(a["u"], b["u"], R.sum_bound(Tj, K)[:, None]) <= 1.0
    assert R.worst(a["v"], b["v"], R.sum_bound(Tj, K)[:, None]) <= 1.0
    assert R.worst(a["Q"], b["Q"], R.q_bound(Ti, K)[:, None]) <= 1.0
    assert R.worst(a["F"], b["F"], R.f_bound(Tj, K)[:, None], scale=b["Fraw"]) <= 1.0
    kept = np.isnan(b["Fraw"])
    assert np.array_equal(a["F"][kept], F[kept])
    assert abs(LD(a["L"]) - b["L"]) <= R.sum_bound(T, K) * b["Labs"]
    assert float(np.abs(a["Q"].astype(LD).sum(axis=1) - 1).max()) <= R.row_sum_bound(K)
    assert a["F"].min() >= F_MIN and a["F"].max() <= 1.0 - F_MIN


def test_the_planted_rows_stay():
    c = case_150()
    Q, F = R.awkward_state(150, 700, 3, 9, F_MIN)
    r = R.em_step(c["geno"], Q, F, F_MIN)
    assert c["none_sample"] == 149 and c["none_snp"] == 699 and c["mono_snp"] == 698
    assert np.array_equal(r["Q"][149], Q[149]) and np.array_equal(r["F"][699], F[699])
    assert np.all(r["F"][698] == F_MIN)                            # a monomorphic SNP goes to the lower clamp at once
    assert (Q == 0).sum() >= 50 and (F == F_MIN).sum() >= 100 and (F == 1 - F_MIN).sum() >= 100
    assert np.all(r["Q"][Q == 0] == 0)


def test_likelihood_never_decreases_over_60_iterations():
    c = case_150()
    Q0, F0 = R.prepare_start(*R.awkward_state(150, 700, 3, 21, F_MIN), F_MIN)
    Q, F, trace, done = R.em_run(c["geno"], Q0, F0, F_MIN, 60, -np.inf)
    assert done == 60 and len(trace) == 61
    assert np.all(np.diff(trace) > 0)
    assert trace[-1] - trace[0] > 1000


def test_supervised_estimates_are_nearer_the_truth_than_one_over_k():
    K = 3
    c = R.admixed_case(150, 700, K, 8, missing=0.05, fst=0.3)             # well separated populations
    Q0 = np.full((150, K), 1.0 / K)
    Q, F, trace, done = R.em_run(c["geno"], Q0, np.clip(c["F"], F_MIN, 1 - F_MIN), F_MIN, 100, 1e-6, fix_f=True)
    assert np.array_equal(F, np.clip(c["F"], F_MIN, 1 - F_MIN))
    live = np.arange(150) != c["none_sample"]
    err = np.abs(Q - c["Q"])[live].mean()
    flat = np.abs(Q0 - c["Q"])[live].mean()
    assert err < 0.25 * flat, (err, flat)
    assert np.array_equal(Q[c["none_sample"]], Q0[c["none_sample"]])


def test_a_tol_between_two_increments_stops_where_the_trace_says():
    """The choice the GPU test of the stopping rule makes, checked on the reference alone.  Plain EM slows down gently -- consecutive
    increments of L differ by a sixth here -- so "well between" is measured against what can move the device's increments: twice the
    bound of L.  The margins on both sides are more than a million times that."""
    G, Q0, F0 = R.stop_case()
    _, _, full, _ = R.em_run(G, Q0, F0, F_MIN, 40, -np.inf, fix_f=True)
    inc = np.diff(full[:-1])                                       # inc[t - 1] = L_t - L_(t - 1), what the rule sees after iteration t
    assert np.all(inc[1:] < inc[:-1])                              # decreasing: one crossing
    t, tol = R.stop_choice(inc)
    T = R.called_counts(G)[2]
    l_bound = R.sum_bound(T, 3) * R.loglik(G, Q0, F0)[1]
    assert inc[t - 1] < tol < inc[t - 2] and min(inc[t - 2] - tol, tol - inc[t - 1]) > 1e6 * 2 * l_bound
    _, _, trace, done = R.em_run(G, Q0, F0, F_MIN, 40, tol, fix_f=True)
    assert done == t + 1 and len(trace) == t + 2 and np.array_equal(trace[:t + 1], full[:t + 1])


# ---- snpgdsAdmixProp ---------------------------------------------------------------------------------------------------------------

def admix_prop_restated(sample_id, eigenvect, groups, bound):
    """R/PCA.R:389-422 line by line"""
    ids = list(sample_id)
    G = len(groups)
    E = eigenvect[:, 0:G - 1]                                       # E <- eigobj$eigenvect[, 1:(length(groups)-1)]
    if E.ndim == 1:
        E = E.reshape(-1, 1)
    mat = []
    for name in groups:
        k = [ids.index(s) for s in groups[name]]                    # match(groups[[i]], eigobj$sample.id)
        mat.append(E[k, :].mean(axis=0))                            # colMeans(Ek)
    mat = np.array(mat).reshape(G, G - 1)
    if np.isnan(mat).any():
        raise ValueError("The eigenvectors should not have missing value!")
    T_P = mat[G - 1, :]
    T_R = np.linalg.inv(mat[:G - 1, :] - np.tile(T_P, (G - 1, 1)))
    new_p = (E - np.tile(T_P, (E.shape[0], 1))) @ T_R
    new_p = np.column_stack([new_p, 1 - new_p.sum(axis=1)])
    if bound:
        new_p[new_p < 0] = 0
        new_p[new_p > 1] = 1
        new_p = new_p / new_p.sum(axis=1, keepdims=True)
    return new_p


def _synthetic_eig(n, k, seed):
    rng = np.random.default_rng(seed)
    ids = np.array(["S%03d" % i for i in rng.permutation(n)])
    return dict(sample_id=ids, eigenvect=rng.normal(0, 0.1, (n, k)), eigenval=np.ones(k))


def _groups_of(ids, G, seed, size=6):
    pick = np.random.default_rng(seed).permutation(len(ids))
    return {"g%d" % g: list(ids[pick[g * size:(g + 1) * size]]) for g in range(G)}


@pytest.mark.parametrize("G,k", [(2, 1), (2, 4), (3, 4), (5, 4), (5, 8)])
def test_admixprop_against_the_restatement(G, k):
    eig = _synthetic_eig(60, k, 7 * G + k)
    groups = _groups_of(eig["sample_id"], G, G)
    for bound in (False, True):
        r = api.snpgdsAdmixProp(eig, groups, bound=bound)
        ref = admix_prop_restated(eig["sample_id"], eig["eigenvect"], groups, bound)
        assert list(r) == ["sample_id", "groups", "prop"] and r["groups"] == list(groups) and r["prop"].shape == (60, G)
        assert np.array_equal(r["sample_id"], eig["sample_id"])
        assert np.allclose(r["prop"], ref, rtol=0, atol=1e-12 * max(1.0, float(np.abs(ref).max())))
        if bound:
            assert r["prop"].min() >= 0 and r["prop"].max() <= 1 and np.allclose(r["prop"].sum(axis=1), 1, rtol=0, atol=4e-16)
    # the identity: the mean proportion of group g over its own samples is the unit vector e_g
    p = api.snpgdsAdmixProp(eig, groups)["prop"]
    ids = list(eig["sample_id"])
    scale = float(np.abs(p).max())
    for g, name in enumerate(groups):
        mean = p[[ids.index(s) for s in groups[name]]].mean(axis=0)
        assert np.allclose(mean, np.eye(G)[g], rtol=0, atol=1e-11 * max(1.0, scale)), (g, mean)
    assert np.allclose(p.sum(axis=1), 1, rtol=0, atol=1e-12 * max(1.0, scale))


def test_admixprop_on_the_eigenvectors_of_the_eigmix_fixture():
    ibd = np.load(os.path.join(GOLDEN, "validate_eigmix.npz"))["ibd"]
    w, v = np.linalg.eigh(ibd)
    vect = v[:, np.argsort(-w)][:, :8]
    ids = np.arange(1000, 1000 + len(ibd))
    eig = dict(sample_id=ids, eigenvect=vect, eigenval=np.sort(w)[::-1][:8])
    # three groups at the extremes of the first two axes
    order = np.argsort(vect[:, 0])
    rest = [i for i in np.argsort(vect[:, 1]) if i not in set(order[:8]) | set(order[-8:])]
    groups = {"low": list(ids[order[:8]]), "high": list(ids[order[-8:]]), "third": list(ids[rest[:8]])}
    for bound in (False, True):
        r = api.snpgdsAdmixProp(eig, groups, bound=bound)
        ref = admix_prop_restated(ids, vect, groups, bound)
        assert np.allclose(r["prop"], ref, rtol=0, atol=1e-12 * max(1.0, float(np.abs(ref).max())))
    p = api.snpgdsAdmixProp(eig, groups)["prop"]
    for g, name in enumerate(groups):
        mean = p[[list(ids).index(s) for s in groups[name]]].mean(axis=0)
        assert np.allclose(mean, np.eye(3)[g], rtol=0, atol=1e-11 * max(1.0, float(np.abs(p).max())))


def test_admixprop_refusals_and_the_overlap_warning():
    eig = _synthetic_eig(30, 2, 1)
    ids = eig["sample_id"]
    groups = _groups_of(ids, 3, 2)
    with pytest.raises(TypeError, match="sample_id"):
        api.snpgdsAdmixProp(dict(eigenvect=eig["eigenvect"]), groups)
    with pytest.raises(TypeError, match="is.matrix"):
        api.snpgdsAdmixProp(dict(sample_id=ids, eigenvect=eig["eigenvect"][:, 0]), groups)
    with pytest.raises(TypeError, match="is.list"):
        api.snpgdsAdmixProp(eig, [list(ids[:3]), list(ids[3:6])])
    with pytest.raises(TypeError, match="length\\(groups\\) > 1"):
        api.snpgdsAdmixProp(eig, {"a": list(ids[:3])})
    with pytest.raises(ValueError, match="`eigobj' should have more eigenvectors than what is specified in `groups'."):
        api.snpgdsAdmixProp(eig, _groups_of(ids, 4, 2))
    with pytest.raises(ValueError, match="`groups' should be a list of sample IDs with respect to multiple groups."):
        api.snpgdsAdmixProp(eig, {"a": list(ids[:3]), "b": 5})
    bad = dict(groups)
    bad["g1"] = list(groups["g1"]) + ["nobody"]
    with pytest.raises(ValueError, match="`groups\\[\\[2\\]\\]' includes sample\\(s\\) not existing in `eigobj\\$sample.id'."):
        api.snpgdsAdmixProp(eig, bad)
    with pytest.raises(TypeError, match="is.logical"):
        api.snpgdsAdmixProp(eig, groups, bound=1)
    nan = dict(eig, eigenvect=eig["eigenvect"].copy())
    nan["eigenvect"][list(ids).index(groups["g2"][0]), 1] = np.nan
    with pytest.raises(ValueError, match="The eigenvectors should not have missing value!"):
        api.snpgdsAdmixProp(nan, groups)
    over = dict(groups)
    over["g2"] = list(groups["g2"]) + [groups["g0"][0]]
    with pytest.warns(UserWarning, match="There are some overlapping between group sample IDs."):
        r = api.snpgdsAdmixProp(eig, over)
    assert np.allclose(r["prop"], admix_prop_restated(ids, eig["eigenvect"], over, False), rtol=0, atol=1e-10)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        api.snpgdsAdmixProp(eig, groups)


# ---- snpgdsAdmixTable --------------------------------------------------------------------------------------------------------------

def test_admixtable_on_a_hand_made_matrix():
    nan = float("nan")
    p = np.array([[0.10, 0.90],
                  [0.30, 0.70],
                  [nan, 1.00],
                  [0.80, 0.20],
                  [0.60, nan],
                  [0.50, 0.50]])
    group = ["b", "a", "b", "c", "c", None]
    t = api.snpgdsAdmixTable(p, group)
    assert list(t) == [0, 1]
    assert t[0]["group"] == ["a", "b", "c"] and list(t[0]["num"]) == [1, 2, 2]
    assert np.allclose(t[0]["mean"], [0.30, 0.10, 0.70]) and np.allclose(t[0]["min"], [0.30, 0.10, 0.60]) and np.allclose(t[0]["max"], [0.30, 0.10, 0.80])
    assert np.isnan(t[0]["sd"][0]) and np.isnan(t[0]["sd"][1]) and np.isclose(t[0]["sd"][2], np.sqrt(0.02))        # n - 1
    assert np.allclose(t[1]["mean"], [0.70, 0.95, 0.20]) and np.isclose(t[1]["sd"][1], np.sqrt(0.005)) and np.isnan(t[1]["sd"][2])
    # A level without a sample cannot reach the table: levels(factor(group)) drops it (an NA label makes none).  A level that is empty
    # of values in a column -- every proportion NaN -- keeps its row, as mean(numeric(0)) and sd do in R
    p2 = np.vstack([p, [nan, 0.25]])
    t = api.snpgdsAdmixTable(p2, group + ["d"])
    assert t[0]["group"] == ["a", "b", "c", "d"] and list(t[0]["num"]) == [1, 2, 2, 1]
    assert np.isnan(t[0]["mean"][3]) and np.isnan(t[0]["sd"][3]) and t[0]["min"][3] == np.inf and t[0]["max"][3] == -np.inf
    assert t[1]["mean"][3] == 0.25 and np.isnan(t[1]["sd"][3])
    assert api.snpgdsAdmixTable(p2, group + ["d"], sort=True)[0]["group"] == ["c", "a", "b", "d"]           # NA means last
    # sort: by decreasing mean, per column
    t = api.snpgdsAdmixTable(dict(sample_id=np.arange(6), groups=["P", "Q"], prop=p), group, sort=True)
    assert list(t) == ["P", "Q"]
    assert t["P"]["group"] == ["c", "a", "b"] and t["Q"]["group"] == ["b", "a", "c"]
    assert np.all(np.diff(t["P"]["mean"]) <= 0) and np.all(np.diff(t["Q"]["mean"]) <= 0)
    with pytest.raises(TypeError, match="is.matrix"):
        api.snpgdsAdmixTable(p[:, 0], group)
    with pytest.raises(TypeError, match="length\\(group\\)"):
        api.snpgdsAdmixTable(p, group[:5])
    with pytest.raises(TypeError, match="is.logical"):
        api.snpgdsAdmixTable(p, group, sort="yes")


# ---- the header and the binding ----------------------------------------------------------------------------------------------------

def test_header_declares_the_eight_functions():
    text = open(HEADER).read()
    protos = M.header_prototypes(text)
    L = _lib.lib()
    for f in NAMES:
        assert f in protos and f in _lib.EXPORTS and hasattr(L, f), f
        assert "out_mem" not in protos[f] and "dst_mem" not in protos[f] and protos[f][0] not in ("ctx", "m")
    assert protos["snpgpu_admix_create"] == ["n_samp", "n_pop", "max_snps", "f_min", "block_snps", "opts", "out"]
    assert protos["snpgpu_admix_feed"] == ["ad", "geno", "n_snp", "format", "mem"]
    assert protos["snpgpu_admix_set"] == ["ad", "q", "f"]
    assert protos["snpgpu_admix_run"] == ["ad", "max_iter", "tol", "flags", "loglik", "n_done"]
    assert protos["snpgpu_admix_get"] == ["ad", "q", "f"]
    assert protos["snpgpu_admix_stats"] == ["ad", "stats"]
    assert "enum { SNPGPU_ADMIX_FIX_F = 1 };" in text and _lib.ADMIX_FIX_F == 1
    assert "#define SNPGPU_ABI_VERSION 2\n" in text                      # additions only: the version stays
    assert text.index("1s. Ancestry proportions") > text.index("snpgpu_gnrPCRelatePairs_get")


def test_no_new_environment_variable():
    csrc = os.path.join(ROOT, "snprelate_amd", "csrc")
    for name in ("admix.hip", "kernels_admix.hip", "admix_device.h"):
        assert '"SNPGPU_' not in open(os.path.join(csrc, name)).read(), name


def test_python_interface():
    import inspect
    import snprelate_amd
    assert snprelate_amd.snpgdsAdmix is api.snpgdsAdmix and snprelate_amd.snpgdsAdmixProp is api.snpgdsAdmixProp
    assert snprelate_amd.snpgdsAdmixTable is api.snpgdsAdmixTable
    sig = inspect.signature(api.snpgdsAdmix)
    assert list(sig.parameters) == ["gdsobj", "k", "groups", "supervised", "sample_id", "snp_id", "autosome_only", "remove_monosnp", "maf",
                                    "missing_rate", "q_start", "f_start", "seed", "max_iter", "tol", "f_min", "with_afreq", "verbose", "device"]
    p = sig.parameters
    assert p["k"].default is None and p["supervised"].default is False and p["seed"].default == 1 and p["max_iter"].default == 500
    assert p["tol"].default == 1e-4 and p["f_min"].default == 1e-6 and p["with_afreq"].default is True
    assert list(inspect.signature(api.snpgdsAdmixProp).parameters) == ["eigobj", "groups", "bound"]
    doc = api.snpgdsAdmix.__doc__
    for words in ("arbitrary", "slow to converge", "SQUAREM", "cross-validation", "multi-device", "device\n    memory", "below fp64"):
        assert words in doc, words


def test_the_seeded_start_is_restated():
    p = np.linspace(0.01, 0.99, 40)
    q, f = api.admix_seeded_start(25, 4, p, 1, F_MIN)
    rng = np.random.Generator(np.random.Philox(1))
    q2 = 0.5 + rng.random((25, 4))
    q2 = q2 / q2.sum(axis=1, keepdims=True)
    f2 = np.clip(p[:, None] + 0.2 * (rng.random((40, 4)) - 0.5), F_MIN, 1 - F_MIN)
    assert np.array_equal(q, q2) and np.array_equal(f, f2)
    assert not np.array_equal(q, api.admix_seeded_start(25, 4, p, 2, F_MIN)[0])


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------

def _refused(rc, fn, text):
    assert rc != 0
    msg = _lib.lib().snpgpu_last_error().decode()
    assert msg.startswith(fn + ": ") and text in msg, msg


def _create(n=20, k=3, max_snps=64, f_min=F_MIN, block=0):
    h = ctypes.c_void_p()
    rc = _lib.lib().snpgpu_admix_create(n, k, max_snps, f_min, block, None, ctypes.byref(h))
    return rc, h


def test_create_refusals():
    fn = "snpgpu_admix_create"
    L = _lib.lib()
    _refused(L.snpgpu_admix_create(20, 3, 64, F_MIN, 0, None, None), fn, "out is NULL")
    for k in (1, 33, 0, -2):
        rc, h = _create(k=k)
        _refused(rc, fn, "n_pop must be in 2 ... 32")
        assert not h.value
    for bad in (0.0, 0.5, -0.1, 0.7, float("nan")):
        _refused(_create(f_min=bad)[0], fn, "f_min must be inside (0, 0.5)")
    for bad in (8, 17, 100, -16, (1 << 20) + 16, 1 << 27):
        _refused(_create(block=bad)[0], fn, "block_snps must be 0 or a positive multiple of 16, at most 2^20")
    rc, h = _create(block=1 << 20)
    assert rc == 0 and _lib.lib().snpgpu_admix_destroy(h) == 0
    _refused(_create(n=0)[0], fn, "invalid number of samples")
    _refused(_create(n=1 << 23)[0], fn, "invalid number of samples")
    _refused(_create(max_snps=0)[0], fn, "invalid max_snps")


def test_a_handle_refuses_without_a_device_call():
    """snpgpu_admix_create makes no HIP call, so the refusals that need a handle are reached here, where no device need exist"""
    L = _lib.lib()
    rc, h = _create(n=20, k=3, max_snps=64, block=16)
    assert rc == 0 and h.value
    try:
        st = np.zeros(6)
        _lib.check(L.snpgpu_admix_stats(h, _lib._ptr(st)))
        assert st[4] == 16 and st[0] == 0 and st[5] == 0
        g = np.zeros((80, 5), np.uint8)
        _refused(L.snpgpu_admix_feed(h, _lib._ptr(g), 65, _lib.GENO_PACKED2, _lib.HOST), "snpgpu_admix_feed", "more rows than max_snps: 0 fed, 65 more, max_snps 64")
        _refused(L.snpgpu_admix_feed(h, _lib._ptr(g), 2, 7, _lib.HOST), "snpgpu_admix_feed", "invalid genotype format")
        _refused(L.snpgpu_admix_feed(h, _lib._ptr(g), 2, _lib.GENO_U8, 5), "snpgpu_admix_feed", "invalid memory kind")
        _refused(L.snpgpu_admix_feed(h, _lib._ptr(g), -1, _lib.GENO_U8, _lib.HOST), "snpgpu_admix_feed", "invalid number of SNPs")
        _refused(L.snpgpu_admix_feed(h, None, 2, _lib.GENO_U8, _lib.HOST), "snpgpu_admix_feed", "geno is NULL")
        ll = np.zeros(4)
        done = ctypes.c_int(0)
        _refused(L.snpgpu_admix_run(h, 2, 1e-4, 0, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "run before set")
        _refused(L.snpgpu_admix_run(h, -1, 1e-4, 0, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "negative max_iter")
        _refused(L.snpgpu_admix_run(h, 2, 1e-4, 2, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "unknown flags")
        _refused(L.snpgpu_admix_run(h, 2, float("nan"), 0, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "tol is NaN")
        _refused(L.snpgpu_admix_run(h, 2, 1e-4, 0, None, ctypes.byref(done)), "snpgpu_admix_run", "loglik is NULL")
        q = np.full((20, 3), 1 / 3)
        q[7] = 0.0
        _refused(L.snpgpu_admix_set(h, _lib._ptr(q), None), "snpgpu_admix_set", "a row of q has no positive sum (sample 7)")
        q[7] = [0.5, -0.1, 0.6]
        _refused(L.snpgpu_admix_set(h, _lib._ptr(q), None), "snpgpu_admix_set", "q must be finite and non-negative (sample 7)")
        q[7] = [0.5, np.inf, 0.6]
        _refused(L.snpgpu_admix_set(h, _lib._ptr(q), None), "snpgpu_admix_set", "q must be finite and non-negative (sample 7)")
        _refused(L.snpgpu_admix_set(h, None, _lib._ptr(np.full((4, 3), 0.5))), "snpgpu_admix_set", "f before any row was fed")
        _refused(L.snpgpu_admix_get(h, _lib._ptr(q), None), "snpgpu_admix_get", "Q has no values")
        assert L.snpgpu_admix_set(h, None, None) == 0 and L.snpgpu_admix_get(h, None, None) == 0
        assert L.snpgpu_admix_feed(h, _lib._ptr(g), 0, _lib.GENO_PACKED2, _lib.HOST) == 0
    finally:
        assert L.snpgpu_admix_destroy(h) == 0


def test_run_before_set_and_a_non_finite_f():
    """host rows fed before the device is open wait in the object, so the refusals that need fed rows are reached without a device"""
    L = _lib.lib()
    rc, h = _create(n=20, k=3, max_snps=64)
    assert rc == 0
    try:
        ll = np.zeros(4)
        done = ctypes.c_int(0)
        _refused(L.snpgpu_admix_run(h, 2, 1e-4, 0, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "run before set")
        g = np.zeros((4, 5), np.uint8)
        assert L.snpgpu_admix_feed(h, _lib._ptr(g), 4, _lib.GENO_PACKED2, _lib.HOST) == 0
        assert L.snpgpu_admix_feed(h, _lib._ptr(np.zeros((60, 20), np.uint8)), 60, _lib.GENO_U8, _lib.HOST) == 0
        _refused(L.snpgpu_admix_feed(h, _lib._ptr(g), 1, _lib.GENO_PACKED2, _lib.HOST), "snpgpu_admix_feed",
                 "more rows than max_snps: 64 fed, 1 more, max_snps 64")
        _refused(L.snpgpu_admix_run(h, 2, 1e-4, 0, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "run before set")
        q = np.full((20, 3), 1 / 3)
        assert L.snpgpu_admix_set(h, _lib._ptr(q), None) == 0
        _refused(L.snpgpu_admix_run(h, 2, 1e-4, 0, _lib._ptr(ll), ctypes.byref(done)), "snpgpu_admix_run", "run before set")   # F has no values yet
        for bad in (np.nan, np.inf, -np.inf):
            f = np.full((64, 3), 0.5)
            f[40, 1] = bad
            _refused(L.snpgpu_admix_set(h, None, _lib._ptr(f)), "snpgpu_admix_set", "f must be finite")
        _refused(L.snpgpu_admix_get(h, None, _lib._ptr(np.zeros((64, 3)))), "snpgpu_admix_get", "F has no values")
    finally:
        assert L.snpgpu_admix_destroy(h) == 0


def test_other_refusals():
    L = _lib.lib()
    buf = np.zeros(16, np.float64)
    g = np.zeros((2, 5), np.uint8)
    done = ctypes.c_int(0)
    _refused(L.snpgpu_admix_feed(None, _lib._ptr(g), 2, _lib.GENO_U8, _lib.HOST), "snpgpu_admix_feed", "ad is NULL")
    _refused(L.snpgpu_admix_set(None, _lib._ptr(buf), None), "snpgpu_admix_set", "ad is NULL")
    _refused(L.snpgpu_admix_run(None, 1, 0.0, 0, _lib._ptr(buf), ctypes.byref(done)), "snpgpu_admix_run", "ad is NULL")
    _refused(L.snpgpu_admix_get(None, _lib._ptr(buf), None), "snpgpu_admix_get", "ad is NULL")
    _refused(L.snpgpu_admix_stats(None, _lib._ptr(buf)), "snpgpu_admix_stats", "NULL argument")
    assert L.snpgpu_admix_destroy(None) == 0
    _lib.check(L.snpgpu_ws_clear())
    _refused(L.snpgpu_gnrAdmix(3, F_MIN, 0, _lib._ptr(buf), _lib._ptr(buf), 1, 0.0, 0, _lib._ptr(buf), ctypes.byref(done), None, None),
             "snpgpu_gnrAdmix", "no genotype working space")
    _refused(L.snpgpu_gnrAdmix(3, F_MIN, 0, None, _lib._ptr(buf), 1, 0.0, 0, _lib._ptr(buf), ctypes.byref(done), None, None),
             "snpgpu_gnrAdmix", "the starting values q and f")
    with pytest.raises(_lib.SnpGpuError, match="n_pop must be in 2 ... 32"):
        _lib.Admix(20, 33, 64)
    with pytest.raises(_lib.SnpGpuError, match="f_min"):
        _lib.Admix(20, 3, 64, f_min=0.5)
    with _lib.Admix(20, 3, 64) as a:
        with pytest.raises(ValueError, match="'q' should be a 20 x 3 matrix"):
            a.set(q=np.zeros((19, 3)))
        with pytest.raises(ValueError, match="non-negative"):
            a.run(-1)
        with pytest.raises(ValueError, match="wrong shape"):
            a.feed(np.zeros((4, 7), np.uint8))


def test_snpgdsadmix_argument_errors(hapmap):
    with pytest.raises(ValueError, match="'k' is required without 'groups'"):
        api.snpgdsAdmix(hapmap)
    with pytest.raises(ValueError, match="'supervised=True' needs 'groups'"):
        api.snpgdsAdmix(hapmap, k=3, supervised=True)
    for k in (1, 33, 2.5, True):
        with pytest.raises(ValueError, match="'k' should be an integer in 2 .. 32"):
            api.snpgdsAdmix(hapmap, k=k)
    ids = hapmap.sample_id
    groups = {"a": list(ids[:5]), "b": list(ids[5:10])}
    with pytest.raises(ValueError, match="'k' should be the number of groups \\(2\\)"):
        api.snpgdsAdmix(hapmap, k=3, groups=groups)
    with pytest.raises(ValueError, match="at least two groups"):
        api.snpgdsAdmix(hapmap, groups={"a": list(ids[:5])})
    for bad in (0.0, 0.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="'f_min' should be inside \\(0, 0.5\\)"):
            api.snpgdsAdmix(hapmap, k=3, f_min=bad)
    with pytest.raises(ValueError, match="'max_iter'"):
        api.snpgdsAdmix(hapmap, k=3, max_iter=-1)
    with pytest.raises(ValueError, match="'tol'"):
        api.snpgdsAdmix(hapmap, k=3, tol=float("nan"))
    with pytest.raises(TypeError, match="is.logical"):
        api.snpgdsAdmix(hapmap, k=3, supervised="yes")
    with pytest.raises(TypeError, match="SNP GDS object"):
        api.snpgdsAdmix("a file name", k=3)
    # the groups are matched before any genotype is touched: an unknown id, an overlap
    names, index, overlap = api._admix_groups(groups, ids, "x")
    assert names == ["a", "b"] and [list(i) for i in index] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]] and not overlap
    assert api._admix_groups({"a": list(ids[:5]), "b": list(ids[4:10])}, ids, "x")[2]
    with pytest.raises(ValueError, match="`groups\\[\\[2\\]\\]' includes sample\\(s\\) not existing in `the selected samples'."):
        api._admix_groups({"a": list(ids[:5]), "b": ["nobody"]}, ids, "the selected samples")
