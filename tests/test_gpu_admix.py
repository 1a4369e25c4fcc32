"""The EM for ancestry proportions on the GPU (snpgpu_admix_*, snpgpu_gnrAdmix, snpgdsAdmix) against the numpy restatement of its
definitions (tests/admix_ref.py, whose docstring derives the bounds; tests/test_cpu_admix.py shows the conditions leaned on here
for the restatement alone).

The shapes stand at the edges of the kernels: n in {1, 15, 150, 257} (one lane, less than a 16-sample genotype word, three 64-sample
loads of the per-SNP owner with a ragged end, one 256-sample workgroup of the per-sample owner plus one sample; 257 is no multiple
of 4, so the last byte of a row is ragged too), m in {1, 17, 700} (one SNP, more than a 16-SNP block, 22 LDS steps of the
per-sample owner with a ragged end), K in {2, 3, 5, 16, 32} (the instantiations 2, 3, 6 -- padded --, 16 and 32).  Two shapes beyond
these lists take the paths those cannot reach: n = 4100 (a second 4096-sample segment of the per-SNP sums) and m = 1100 (a
second 1024-SNP segment of the per-sample sums, and with block_snps = 48 an internal block that straddles the two).

Every comparison starts from the state the device itself reports (get() after set(), or the previous iteration's get()), so the
restatement and the device work from the same float64 numbers.  Observed on an MI355X (the worst case of each, as a share of its
bound, over every case and test of this file): Q' 0.030, F' 0.030, L 0.024; rows of Q' sum to 1 within 0.2 of (K + 2) eps."""
import functools
import os

import numpy as np
import pytest

import admix_ref as R
from conftest import GOLDEN
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows

pytestmark = pytest.mark.gpu

LD = np.longdouble
F_MIN = 1e-6
NEVER = float("-inf")       # a tol that never stops
#        n     m    K  missing
CASES = [(1, 17, 3, 0.0),
         (1, 1, 2, 0.0),
         (15, 1, 2, 0.0),
         (15, 700, 16, 0.3),
         (150, 700, 3, 0.05),
         (150, 700, 3, 0.3),
         (150, 700, 3, 0.0),
         (150, 17, 32, 0.3),
         (257, 700, 5, 0.3),
         (257, 17, 2, 0.0),
         (4100, 17, 2, 0.05),
         (15, 1100, 3, 0.05)]
IDS = ["n%d-m%d-K%d-miss%g" % c for c in CASES]
MAIN = (150, 700, 3, 0.05)


def test_the_cases_cover_every_value():
    assert {1, 15, 150, 257} <= {c[0] for c in CASES} and {1, 17, 700} <= {c[1] for c in CASES}
    assert {c[2] for c in CASES} == {2, 3, 5, 16, 32} and {c[3] for c in CASES} >= {0.0, 0.3}
    assert _lib.device_count() >= 1


@functools.lru_cache(maxsize=None)
def inputs(case):
    n, m, K, miss = case
    c = R.admixed_case(n, m, K, 100 + 3 * n + m + K, missing=miss)
    Q, F = R.awkward_state(n, m, K, 7 + n + m, F_MIN)
    g = c["geno"]
    for a in (g, Q, F):
        a.setflags(write=False)
    return dict(c, geno=g, packed=pack_2bit_rows(g), Q0=Q, F0=F)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def one_step(case, block=0, fix_f=False):
    """the device's state after set(), after run(1), its trace and statistics; the long-double restatement from the state after set()"""
    n, m, K, _ = case
    i = inputs(case)
    with _lib.Admix(n, K, m, f_min=F_MIN, block_snps=block) as a:
        a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        a.set(i["Q0"], i["F0"])
        q0, f0 = a.get()
        ll, done = a.run(1, NEVER, fix_f=fix_f)
        q1, f1 = a.get()
        st = a.stats()
    assert done == 1 and ll.shape == (2,)
    _frozen(q0, f0, q1, f1, ll)
    return dict(q0=q0, f0=f0, q1=q1, f1=f1, ll=ll, stats=st, ref=R.em_step(i["geno"], q0, f0, F_MIN, LD, fix_f=fix_f))


def _check_step(G, K, q0, f0, q1, f1, L0, ref, fix_f=False):
    """the device's (q1, f1, L0) against the restatement `ref` of one step from (q0, f0); returns the shares of the bounds"""
    Ti, Tj, T = R.called_counts(G)
    share = dict(Q=R.worst(q1, ref["Q"], R.q_bound(Ti, K)[:, None]),
                 L=float(abs(LD(L0) - ref["L"]) / (R.sum_bound(T, K) * ref["Labs"])) if T else 0.0,
                 rows=float(np.abs(q1.astype(LD).sum(axis=1) - 1).max() / R.row_sum_bound(K)))
    if fix_f:
        assert np.array_equal(f1, f0)
    else:
        share["F"] = R.worst(f1, ref["F"], R.f_bound(Tj, K)[:, None], scale=ref["Fraw"])
        kept = np.isnan(ref["Fraw"])                                        # u + v = 0: the row of F stays, bit for bit
        assert np.array_equal(f1[kept], f0[kept])
    print("shares of the bounds:", share)
    assert all(v <= 1.0 for v in share.values()), share
    assert f1.min() >= F_MIN and f1.max() <= 1.0 - F_MIN
    assert np.array_equal(q1[Ti == 0], q0[Ti == 0])                         # no called SNP: the row of Q stays, bit for bit
    assert np.all(q1[q0 == 0] == 0) and q1.min() >= 0
    return share


# ---- 1. one step against the restatement --------------------------------------------------------------------------------------------

def test_set_normalises_and_clamps():
    i = inputs(MAIN)
    with _lib.Admix(150, 3, 700, f_min=F_MIN) as a:
        a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        f = i["F0"].copy()
        f[3, 0], f[4, 1] = -2.0, 7.0
        a.set(5.0 * i["Q0"], f)
        q, f2 = a.get()
    assert float(np.abs(q - i["Q0"]).max()) <= 4 * R.EPS and np.all(q[i["Q0"] == 0] == 0)
    assert f2[3, 0] == F_MIN and f2[4, 1] == 1 - F_MIN
    f[3, 0], f[4, 1] = F_MIN, 1 - F_MIN
    assert np.array_equal(f2, f)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_step(case):
    n, m, K, miss = case
    i, r = inputs(case), one_step(case)
    assert np.array_equal(r["f0"], i["F0"]) and float(np.abs(r["q0"] - i["Q0"]).max()) <= 4 * R.EPS
    _check_step(i["geno"], K, r["q0"], r["f0"], r["q1"], r["f1"], r["ll"][0], r["ref"])
    # the likelihood of the state that is returned
    Ti, Tj, T = R.called_counts(i["geno"])
    L1, L1abs = R.loglik(i["geno"], r["q1"], r["f1"], LD)
    assert abs(LD(r["ll"][1]) - L1) <= R.sum_bound(T, K) * L1abs
    if i["none_sample"] is not None:
        s, j = i["none_sample"], i["none_snp"]
        assert Ti[s] == 0 and Tj[j] == 0
        assert np.array_equal(r["q1"][s], r["q0"][s]) and np.array_equal(r["f1"][j], r["f0"][j])
        assert np.all(r["f1"][i["mono_snp"]] == F_MIN)
    if n >= 15 and m >= 17:
        assert (r["q0"] == 0).any() and (r["f0"] == F_MIN).any() and (r["f0"] == 1 - F_MIN).any()
    st = r["stats"]
    assert st["blocks"] == 1 and st["iterations"] == 1 and st["block_snps"] == (m + 15) // 16 * 16 and st["pass_ms"] > 0
    assert st["launches"] == 2 + 3 + 1 + 2                                  # the iteration, then the likelihood-only pass


# ---- 2. many steps without amplification --------------------------------------------------------------------------------------------

def test_25_iterations_each_within_the_one_step_bound_of_the_previous_device_state():
    n, m, K, _ = MAIN
    i = inputs(MAIN)
    G = i["geno"]
    T = R.called_counts(G)[2]
    worst = {}
    with _lib.Admix(n, K, m, f_min=F_MIN) as a:
        a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        a.set(i["Q0"], i["F0"])
        q0, f0 = a.get()
        last = None
        for t in range(25):
            ll, done = a.run(1, NEVER)
            q1, f1 = a.get()
            ref = R.em_step(G, q0, f0, F_MIN, LD)
            for k, v in _check_step(G, K, q0, f0, q1, f1, ll[0], ref).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if last is not None:
                assert ll[0] == last                                        # the same state, the same pass: the same bits
                assert ll[1] - ll[0] >= -2 * R.sum_bound(T, K) * float(ref["Labs"])
            last = ll[1]
            q0, f0 = q1, f1
        assert a.stats()["iterations"] == 25
    print("worst shares over 25 iterations:", worst)


# ---- 3. run(T) is T x run(1) --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [MAIN, (257, 700, 5, 0.3)])
def test_run_t_is_t_times_run_1_bit_for_bit(case):
    n, m, K, _ = case
    i = inputs(case)
    T = 6

    def fresh():
        a = _lib.Admix(n, K, m, f_min=F_MIN)
        a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        a.set(i["Q0"], i["F0"])
        return a

    with fresh() as a:
        ll, done = a.run(T, NEVER)
        q, f = a.get()
    assert done == T and len(ll) == T + 1
    with fresh() as b:
        trace = []
        for t in range(T):
            l1, d1 = b.run(1, NEVER)
            trace.append(l1[0])
        trace.append(l1[1])
        q2, f2 = b.get()
    assert np.array_equal(q, q2) and np.array_equal(f, f2) and np.array_equal(ll, np.array(trace))
    with fresh() as c:                                                      # another object, the same data: the same bits
        ll3, _ = c.run(T, NEVER)
        q3, f3 = c.get()
    assert np.array_equal(q, q3) and np.array_equal(f, f3) and np.array_equal(ll, ll3)
    assert np.all(np.diff(ll) > 0)


def test_max_iter_0_evaluates_the_likelihood():
    r = one_step(MAIN)
    i = inputs(MAIN)
    with _lib.Admix(150, 3, 700, f_min=F_MIN) as a:
        a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        a.set(i["Q0"], i["F0"])
        ll, done = a.run(0)
        q, f = a.get()
        assert a.stats()["iterations"] == 0
    assert done == 0 and ll.shape == (1,) and ll[0] == r["ll"][0]
    assert np.array_equal(q, r["q0"]) and np.array_equal(f, r["f0"])


# ---- 4. feeds -----------------------------------------------------------------------------------------------------------------------

def _fed(case, feeder, iters=2, block=0):
    n, m, K, _ = case
    i = inputs(case)
    with _lib.Admix(n, K, m, f_min=F_MIN, block_snps=block) as a:
        feeder(a)
        a.set(i["Q0"], i["F0"])
        ll, _ = a.run(iters, NEVER)
        q, f = a.get()
        return q, f, ll, a.stats()


@pytest.mark.parametrize("case", [(257, 700, 5, 0.3), MAIN])
def test_every_cut_form_and_memory_of_the_feeds_gives_the_same_bits(case):
    import torch
    n, m, K, _ = case
    i = inputs(case)
    packed, g = i["packed"], np.ascontiguousarray(i["geno"])

    def in_feeds(rows, size, fmt):
        def feeder(a):
            for s in range(0, m, size):
                a.feed(rows[s:s + size], fmt=fmt)
        return feeder

    def from_device(rows, size, fmt):
        dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        def feeder(a):
            for s in range(0, m, size):
                nb = min(size, m - s)
                a.feed(int(dev.data_ptr()) + s * rows.shape[1], fmt=fmt, n_snp=nb)
            torch.cuda.synchronize()
        return feeder

    def host_after_the_device_is_open(a):
        a.feed(packed[:100], fmt=_lib.GENO_PACKED2)
        a.set(i["Q0"], None)
        a.get()                                                             # opens the device: the rest is fed straight to it
        a.feed(g[100:], fmt=_lib.GENO_U8)

    base = _fed(case, in_feeds(packed, m, _lib.GENO_PACKED2))
    others = {"1": in_feeds(packed, 1, _lib.GENO_PACKED2), "16": in_feeds(packed, 16, _lib.GENO_PACKED2),
              "333": in_feeds(packed, 333, _lib.GENO_PACKED2), "u8": in_feeds(g, m, _lib.GENO_U8), "u8-333": in_feeds(g, 333, _lib.GENO_U8),
              "dev": from_device(packed, m, _lib.GENO_PACKED2), "dev-333": from_device(packed, 333, _lib.GENO_PACKED2),
              "dev-u8-16": from_device(g, 16, _lib.GENO_U8), "mixed": host_after_the_device_is_open}
    for name, feeder in others.items():
        q, f, ll, _ = _fed(case, feeder)
        assert np.array_equal(q, base[0]) and np.array_equal(f, base[1]) and np.array_equal(ll, base[2]), name


def test_rows_fed_after_f_was_set_need_f_again():
    i = inputs(MAIN)
    with _lib.Admix(150, 3, 700, f_min=F_MIN) as a:
        a.feed(i["packed"][:400], fmt=_lib.GENO_PACKED2)
        a.set(i["Q0"], i["F0"][:400])
        a.run(1, NEVER)
        a.feed(i["packed"][400:], fmt=_lib.GENO_PACKED2)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_admix_run: rows were fed after F was set: F holds 400 of 700 SNPs"):
            a.run(1, NEVER)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_admix_feed: more rows than max_snps: 700 fed, 1 more, max_snps 700"):
            a.feed(i["packed"][:1], fmt=_lib.GENO_PACKED2)
        a.set(None, i["F0"])
        ll, done = a.run(1, NEVER)
        assert done == 1 and np.isfinite(ll).all()
        f = i["F0"].copy()
        f[5, 1] = np.nan
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_admix_set: f must be finite"):
            a.set(None, f)
    with _lib.Admix(150, 3, 700, f_min=F_MIN) as a:
        a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_admix_run: run before set"):
            a.run(1)


# ---- 5. the second trip of the internal block loop ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case,block,trips", [(MAIN, 16, 44), ((257, 700, 5, 0.3), 48, 15), ((15, 1100, 3, 0.05), 48, 23),
                                              ((15, 1100, 3, 0.05), 1024, 2)])
def test_internal_blocks_give_the_same_bits(case, block, trips):
    """The sums are cut at fixed absolute indices, not at the internal blocks: a_ik is carried across the blocks in SNP
    order, so the results are equal bit for bit whatever block_snps is -- also where a block straddles two 1024-SNP segments
    (m = 1100, 48-SNP blocks) or ends exactly on one (1024)."""
    i = inputs(case)
    feeder = lambda a: a.feed(i["packed"], fmt=_lib.GENO_PACKED2)
    q, f, ll, st = _fed(case, feeder, iters=3)
    q2, f2, ll2, st2 = _fed(case, feeder, iters=3, block=block)
    assert st["blocks"] == 1 and st["block_snps"] >= case[1]
    assert st2["blocks"] == trips == -(-case[1] // block) and st2["block_snps"] == block
    assert st2["launches"] == 3 * (2 * trips + 3) + (trips + 2)
    assert np.array_equal(q, q2) and np.array_equal(f, f2) and np.array_equal(ll, ll2)
    assert st["resident_bytes"] == st2["resident_bytes"] > 0


# ---- 6. SNPGPU_ADMIX_FIX_F ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [MAIN, (15, 700, 16, 0.3), (150, 17, 32, 0.3)])
def test_fix_f_moves_q_only(case):
    n, m, K, _ = case
    i, r = inputs(case), one_step(case, fix_f=True)
    assert np.array_equal(r["f1"], r["f0"])
    _check_step(i["geno"], K, r["q0"], r["f0"], r["q1"], r["f1"], r["ll"][0], r["ref"], fix_f=True)
    assert r["ll"][0] == one_step(case)["ll"][0]                            # the same likelihood, with and without u and v
    assert r["stats"]["launches"] == 2 + 3 + 1 + 2


def test_the_stopping_rule_stops_where_the_restated_trace_says():
    G, Q0, F0 = R.stop_case(F_MIN)
    _, _, full, _ = R.em_run(G, Q0, F0, F_MIN, 40, NEVER, fix_f=True)
    t, tol = R.stop_choice(np.diff(full[:-1]))
    _, _, ref, ref_done = R.em_run(G, Q0, F0, F_MIN, 40, tol, fix_f=True)
    assert ref_done == t + 1 == 7
    with _lib.Admix(150, 3, 700, f_min=F_MIN) as a:
        a.feed(pack_2bit_rows(G), fmt=_lib.GENO_PACKED2)
        a.set(Q0, F0)
        q0, f0 = a.get()
        assert np.array_equal(q0, Q0) and np.array_equal(f0, F0)
        ll, done = a.run(40, tol, fix_f=True)
        q, f = a.get()
        assert a.stats()["iterations"] == 7
    assert done == ref_done and len(ll) == done + 1
    T = R.called_counts(G)[2]
    l_bound = R.sum_bound(T, 3) * float(R.loglik(G, Q0, F0)[1])
    assert float(np.abs(ll - ref).max()) <= 8 * l_bound                      # seven steps of a contraction-free bound, generously
    assert np.array_equal(f, F0)
    inc = np.diff(ll[:-1])
    assert inc[-1] < tol < inc[-2]


# ---- 7. snpgdsAdmix -----------------------------------------------------------------------------------------------------------------

def hapmap_groups(f):
    pop = np.asarray(f.sample_annot["pop.group"])
    ids = np.asarray(f.sample_id)
    east = (pop == "HCB") | (pop == "CHB") | (pop == "JPT")                   # the fixture spells Han Chinese in Beijing "HCB"
    return {"YRI": list(ids[pop == "YRI"]), "CEU": list(ids[pop == "CEU"]), "CHB+JPT": list(ids[east])}


@functools.lru_cache(maxsize=None)
def hapmap_file():
    from snprelate_amd.gds import open_gds
    return open_gds(os.path.join(GOLDEN, "hapmap_geno.gds"))


def test_snpgdsadmix_supervised_on_hapmap():
    """The float64 restatement on the same data (279 samples, the 8722 polymorphic autosomal SNPs; F at the groups' frequencies and
    fixed, Q from 1 / 3, 500 iterations, which tol = 1e-4 does not cut short) gives mean proportions of the groups in their own
    columns of 0.9980 (YRI), 0.9951 (CEU) and 0.9993 (CHB + JPT), the smallest single own proportion 0.973: the 0.9 asserted below stands."""
    f = hapmap_file()
    groups = hapmap_groups(f)
    assert [len(v) for v in groups.values()] == [93, 92, 94]
    r = api.snpgdsAdmix(f, groups=groups, supervised=True, verbose=False)
    assert list(r) == ["sample_id", "snp_id", "groups", "prop", "afreq", "loglik", "niter", "converged"]
    assert r["groups"] == ["YRI", "CEU", "CHB+JPT"] and r["prop"].shape == (279, 3) and r["afreq"].shape == (len(r["snp_id"]), 3)
    assert len(r["snp_id"]) > 8000 and r["niter"] >= 2 and len(r["loglik"]) == r["niter"] + 1
    assert np.all(np.diff(r["loglik"]) > -1e-6) and float(np.abs(r["prop"].sum(axis=1) - 1).max()) <= 5 * R.EPS
    ids = list(r["sample_id"])
    means = [float(r["prop"][[ids.index(s) for s in groups[g]], c].mean()) for c, g in enumerate(groups)]
    print("own-column means:", means, "niter", r["niter"], "converged", r["converged"])
    assert all(m > 0.9 for m in means), means
    # supervised: the frequencies are the groups' own, sum g / 2 called
    g = api.snpgdsGetGeno(f, snp_id=r["snp_id"], snpfirstdim=True, verbose=False)
    for c, name in enumerate(groups):
        sub = g[:, [ids.index(s) for s in groups[name]]]
        called = sub != 3
        ok = called.sum(axis=1) > 0
        freq = np.where(called, sub, 0).sum(axis=1)[ok] / (2.0 * called.sum(axis=1)[ok])
        assert np.array_equal(r["afreq"][ok, c], np.clip(freq, 1e-6, 1 - 1e-6)), name
    t = api.snpgdsAdmixTable(r, np.asarray(f.sample_annot["pop.group"]))
    assert list(t) == ["YRI", "CEU", "CHB+JPT"] and t["YRI"]["group"] == ["CEU", "HCB", "JPT", "YRI"] and t["YRI"]["mean"][3] > 0.9


def test_snpgdsadmix_seeded_twice_and_other_starts():
    f = hapmap_file()
    a = api.snpgdsAdmix(f, k=3, seed=1, max_iter=12, verbose=False)
    b = api.snpgdsAdmix(f, k=3, seed=1, max_iter=12, verbose=False)
    assert a["groups"] is None and a["niter"] == 12 and not a["converged"]
    for k in ("prop", "afreq", "loglik"):
        assert np.array_equal(a[k], b[k]), k
    c = api.snpgdsAdmix(f, k=3, seed=2, max_iter=12, verbose=False)
    assert not np.array_equal(a["prop"], c["prop"])
    assert np.all(np.diff(a["loglik"]) > 0)
    # the seeded start is the documented one: one likelihood evaluation from it equals the run's first entry
    g = api.snpgdsGetGeno(f, snp_id=a["snp_id"], snpfirstdim=True, verbose=False)
    called = g != 3
    p = np.where(called, g, 0).sum(axis=1) / (2.0 * called.sum(axis=1))
    q0, f0 = api.admix_seeded_start(279, 3, p, 1, 1e-6)
    with _lib.Admix(279, 3, len(g)) as obj:
        obj.feed(pack_2bit_rows(g), fmt=_lib.GENO_PACKED2)
        obj.set(q0, f0)
        ll, _ = obj.run(0)
    assert ll[0] == a["loglik"][0]
    # q_start from the eigen-analysis
    groups = hapmap_groups(f)
    eig = api.snpgdsEIGMIX(f, verbose=False)
    prop = api.snpgdsAdmixProp(eig, groups, bound=True)
    assert np.array_equal(prop["sample_id"], a["sample_id"])
    d = api.snpgdsAdmix(f, groups=groups, q_start=prop["prop"], max_iter=5, with_afreq=False, verbose=False)
    assert d["afreq"] is None and d["niter"] == 5 and np.all(np.diff(d["loglik"]) > 0)
    e = api.snpgdsAdmix(f, groups=groups, max_iter=5, verbose=False)
    assert d["loglik"][0] > e["loglik"][0]                                  # a better start than 1 / K
    with pytest.raises(ValueError, match="There are some overlapping between group sample IDs."):
        api.snpgdsAdmix(f, groups=dict(groups, CEU=groups["CEU"] + groups["YRI"][:1]), verbose=False)
    with pytest.raises(ValueError, match="not existing in `the selected samples'"):
        api.snpgdsAdmix(f, groups=groups, sample_id=a["sample_id"][5:], verbose=False)
    with pytest.raises(ValueError, match="'q_start' should be a 279 x 3 matrix"):
        api.snpgdsAdmix(f, k=3, q_start=np.ones((278, 3)), verbose=False)


def test_snpgdsadmix_on_a_bedstream():
    bs = api.snpgdsOpenBED(*[os.path.join(GOLDEN, "plinkhapmap.%s.gz" % e) for e in ("bed", "fam", "bim")], verbose=False)
    r = api.snpgdsAdmix(bs, k=2, max_iter=8, verbose=False)
    n = len(bs.sample_id)
    assert n > 50 and r["prop"].shape == (n, 2) and r["niter"] == 8 and np.all(np.diff(r["loglik"]) > 0)
    assert float(np.abs(r["prop"].sum(axis=1) - 1).max()) <= 4 * R.EPS and r["afreq"].shape == (len(r["snp_id"]), 2)
