"""Related pairs straight from the GPU panels: snpgpu_select_pairs / snpgpu_multi_select_pairs / snpgpu_gnrIBDPairs against the reference's
snpgdsIBDSelection (tests/ibd_selection_ref.py, R/IBD.R:463-531) applied to the matrices that the EXISTING finalisers return for the
same context -- those are held to the CPU oracle by test_gpu_panel_finalisers.py / test_gpu_parity.py.  Everything is compared exactly:
indices, order, values bit for bit, NaN positions.  Inputs are tests/panel_streams.py (read-only): n = 531 cut into the panels
0 / 256 / 512 / 531, n = 513 whose last panel is one diagonal entry; the streams `mixed` and `holes`, fed in their blocks.

One comparison is not bit for bit, and cannot be: KING-homo's three panels concatenated against the full context (see
_panels_against_whole -- the fp64 weight sums of a panel and of the full context differ in the last bit in the accumulators themselves;
one run: k0 1.0285857984399236 against 1.0285857984399234 at the first pair).  KING-robust and MoM are held to equality there too.

Counts of one run are printed as SELECT-FIGURE lines (`pytest -s`)."""
import contextlib
import ctypes

import numpy as np
import pytest

import ibd_selection_ref as R
import panel_streams as P
from conftest import synth_geno

pytestmark = pytest.mark.gpu

NAN = float("nan")
# what to select: (name, context kind, selection kind, keyword arguments of select_pairs / the finaliser)
VARIANTS = ["robust", "robust_fam", "homo", "mom", "mom_constraint"]


def _variant(name, s):
    from snprelate_amd import _lib
    if name.startswith("robust"):
        fam = s.fam if name == "robust_fam" else None
        return "KING_ROBUST", _lib.SEL_KING_ROBUST, dict(family=fam), ("IBS0", None)
    if name == "homo":
        return "KING_HOMO", _lib.SEL_KING_HOMO, {}, ("k0", "k1")
    return "IBS", _lib.SEL_MOM, dict(e=s.mom_expect(), constraint=name == "mom_constraint"), ("k0", "k1")


@contextlib.contextmanager
def _context(kind, n, blocks, rows=None, bmax=P.BMAX):
    from snprelate_amd import _lib
    kw = {} if rows is None else dict(row_begin=rows[0], row_end=rows[1])
    with _lib.Accumulator(getattr(_lib, kind), n, max_block_snps=bmax, **kw) as a:
        for b in blocks:
            a.feed(b)
        yield a


def _finaliser(a, name, args):
    """the packed slabs of the context's existing finaliser, as the per-pair entries of an IBD object"""
    if name.startswith("robust"):
        i0, k = a.king_robust(family=args["family"], packed=True)
        return dict(IBS0=i0, kinship=k)
    if name == "homo":
        k0, k1 = a.king_homo(packed=True)
    else:
        k0, k1 = a.ibd_mom(args["e"], constraint=args["constraint"], packed=True)
    return dict(k0=k0, k1=k1)


def _obj(slabs, n, rows):
    """full n x n matrices (NaN outside the panel's rows) with sample ids 0 .. n-1"""
    o = dict(sample_id=np.arange(n), snp_id=None, afreq=None)
    for k, v in slabs.items():
        o[k] = R.slab_to_rows(v, n, *rows)
    return o


def _table(res, cols):
    """select_pairs' tuple as the reference's table"""
    i1, i2, v0, v1, kin, found = res
    t = dict(ID1=i1.astype(np.int64), ID2=i2.astype(np.int64))
    t[cols[0]] = v0
    if cols[1]:
        t[cols[1]] = v1
    else:
        assert v1 is None
    t["kinship"] = kin
    return t, found


def _same(got, ref, what):
    msg = R.same_table(got, ref)
    assert msg is None, "%s: %s" % (what, msg)


def _concat(tables):
    return {k: np.concatenate([t[k] for t in tables]) for k in tables[0]}


def _realised(kin):
    """one kinship value that occurs: the median of the finite entries' upper half, so that `>=` must keep its own pair"""
    v = np.sort(kin[np.isfinite(kin)])
    return float(v[(3 * v.size) // 4])


def _panels_against_whole(variant, parts, whole, cutoff):
    """The three panels' results concatenated equal the full context's: exactly, for the kinds whose accumulators are integer counters
    (KING-robust, MoM).  KING-homo's fp64 weight sums of a row panel and of the full context are accumulated over different tiles and
    differ in the last bits before any finaliser or selection runs (test_gpu_panel_finalisers holds k0 / k1 of a panel to rtol 1e-5,
    atol 1e-7 / 2e-5 against the oracle, and only the counter kinds to equality with the full context), so a pair within that
    distance of the cutoff may be selected on one side only.  For KING-homo: with a non-finite cutoff the same pairs in the same
    order and values within twice those tolerances; with a finite cutoff the pairs found on one side only lie within the kinship
    tolerance (1e-5 relative + 1e-5 absolute: the k0 / k1 bounds through (1 - k0 - k1) / 2 + k1 / 4) of the cutoff."""
    if variant != "homo":
        return _same(parts, whole, "the three panels concatenated against the full context")
    key = lambda t: t["ID1"] * (1 << 20) + t["ID2"]                             # noqa: E731
    kp, kw = key(parts), key(whole)
    assert (np.diff(kp) > 0).all() and (np.diff(kw) > 0).all(), "order"
    if not np.isfinite(cutoff):
        assert np.array_equal(kp, kw)
        for col, atol in (("k0", 2e-7), ("k1", 4e-5), ("kinship", 2e-5)):
            np.testing.assert_allclose(parts[col], whole[col], rtol=2e-5, atol=atol, equal_nan=True)
        return None
    only_p, only_w = ~np.isin(kp, kw), ~np.isin(kw, kp)
    for t, only in ((parts, only_p), (whole, only_w)):
        assert (np.abs(t["kinship"][only] - cutoff) <= 1e-5 * abs(cutoff) + 1e-5).all(), "a pair far from the cutoff is on one side only"
    both_p, both_w = ~only_p, ~only_w
    for col, atol in (("k0", 2e-7), ("k1", 4e-5), ("kinship", 2e-5)):
        np.testing.assert_allclose(parts[col][both_p], whole[col][both_w], rtol=2e-5, atol=atol)
    return None


# ---- 1, 2: every kind x full context and the three panels x the cutoffs ---------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("mixed", 531), ("holes", 531)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_kind_panel_and_cutoff(variant, name, n):
    s = P.stream(name, n)
    kind, what, args, cols = _variant(variant, s)
    contexts = [(0, n)] + P.panels(n)
    failed = []
    with contextlib.ExitStack() as st:
        ctx = [(st.enter_context(_context(kind, n, s.blocks(), None if rows == (0, n) else rows)), rows) for rows in contexts]
        objs = [_obj(_finaliser(a, variant, args), n, rows) for a, rows in ctx]
        kin_full = objs[0]["kinship"] if "kinship" in objs[0] else (1 - objs[0]["k0"] - objs[0]["k1"]) * 0.5 + objs[0]["k1"] * 0.25
        cutoffs = [NAN, float("inf"), 0.0, 0.0442, _realised(kin_full[np.triu_indices(n, 1)]), 10.0]
        oracle = None
        if variant.startswith("robust"):                   # the oracle's whole matrices
            o0, ok = s.king_robust("fam" if variant == "robust_fam" else None)
            oracle = dict(sample_id=np.arange(n), IBS0=R.packed_to_full(o0, n), kinship=R.packed_to_full(ok, n))
        for cutoff in cutoffs:
            got = []
            for (a, rows), obj in zip(ctx, objs):
                t, found = _table(a.select_pairs(what, cutoff, **args), cols)
                ref = R.panel_selection(obj, n, rows[0], rows[1], cutoff)
                print("SELECT-FIGURE %-14s %-5s rows %3d..%3d cutoff %-8.4g: %d pairs" % (variant, name, rows[0], rows[1], cutoff, found))
                try:
                    assert found == ref["ID1"].size == t["ID1"].size, "n_found %d, %d rows, the reference has %d" % (found, t["ID1"].size, ref["ID1"].size)
                    _same(t, ref, "against the finaliser's matrices")
                    if oracle is not None:
                        _same(t, R.panel_selection(oracle, n, rows[0], rows[1], cutoff), "against the oracle")
                except AssertionError as e:
                    failed.append("rows %d..%d cutoff %r: %s" % (rows[0], rows[1], cutoff, e))
                got.append(t)
            try:
                _panels_against_whole(variant, _concat(got[1:]), got[0], cutoff)
            except AssertionError as e:
                failed.append("cutoff %r: %s" % (cutoff, e))
            n_pairs = n * (n - 1) // 2
            if not np.isfinite(cutoff):
                assert got[0]["ID1"].size == n_pairs                     # every pair, NaN pairs included
                if name == "holes" and variant.startswith("robust"):
                    assert np.isnan(got[0]["kinship"]).sum() == len(P.holes_nan_pairs(n, False)) == 531
            elif cutoff == 10.0:
                assert got[0]["ID1"].size == 0
            else:
                assert not np.isnan(got[0]["kinship"]).any() and (got[0]["kinship"] >= cutoff).all()
            if variant == "robust" and cutoff == 0.0442:                  # the oracle's counts for these streams
                assert got[0]["ID1"].size == {"holes": 5577, "mixed": 686}[name]
            if variant == "robust" and cutoff == 0.0 and name == "holes":
                assert got[0]["ID1"].size == 52254
    assert not failed, "\n".join(failed)


def test_one_entry_panel_selects_nothing():
    """n = 513: the last panel is the diagonal entry (512, 512) alone"""
    from snprelate_amd import _lib
    n = 513
    s = P.stream("mixed", n)
    with _context("KING_ROBUST", n, s.blocks(), (512, 513)) as a:
        for cutoff in (NAN, 0.0):
            res = a.select_pairs(_lib.SEL_KING_ROBUST, cutoff)
            assert res[5] == 0 and res[0].size == 0
        out = [np.full(4, -9, np.int32), np.full(4, -9, np.int32)] + [np.full(4, -9.0) for _ in range(3)]
        o = _lib.SelOpts(_lib.SEL_KING_ROBUST, 0, None, None, NAN, None)
        found = ctypes.c_int64(-1)
        _lib.check(_lib.lib().snpgpu_select_pairs(a._h, ctypes.byref(o), 4, *[_lib._ptr(x) for x in out], _lib.HOST, ctypes.byref(found)))
        assert found.value == 0 and all((x == -9).all() for x in out)
    with _context("KING_ROBUST", n, s.blocks()) as a, _context("KING_ROBUST", n, s.blocks(), (0, 256)) as p0, \
            _context("KING_ROBUST", n, s.blocks(), (256, 512)) as p1:
        full, _ = _table(a.select_pairs(_lib.SEL_KING_ROBUST, 0.0), ("IBS0", None))
        parts = [_table(p.select_pairs(_lib.SEL_KING_ROBUST, 0.0), ("IBS0", None))[0] for p in (p0, p1)]
        _same(_concat(parts), full, "panels 0 and 1 of n = 513 against the full context")
        assert full["ID1"].size > 1000


# ---- 3: the sample mask ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["robust_fam", "homo"])
def test_sample_mask(variant):
    n = 531
    s = P.stream("holes", n)
    kind, what, args, cols = _variant(variant, s)
    mask = np.random.default_rng(17).random(n) < 0.5
    for lo, hi in ((0, 256), (256, 512), (512, n)):
        assert mask[lo:hi].any() and not mask[lo:hi].all()
    for rows in [(0, n)] + P.panels(n):
        with _context(kind, n, s.blocks(), None if rows == (0, n) else rows) as a:
            obj = _obj(_finaliser(a, variant, args), n, rows)
            for cutoff in (NAN, 0.0):
                t, found = _table(a.select_pairs(what, cutoff, samp_sel=mask, **args), cols)
                ref = R.panel_selection(obj, n, rows[0], rows[1], cutoff, mask)      # sample_id = context indices: mapped back by the ids
                assert found == ref["ID1"].size and found > 0
                _same(t, ref, "rows %d..%d cutoff %r with a mask" % (rows[0], rows[1], cutoff))
                assert mask[t["ID1"]].all() and mask[t["ID2"]].all()
                t8, _ = _table(a.select_pairs(what, cutoff, samp_sel=mask.astype(np.uint8) * 7, **args), cols)    # nonzero = selected
                _same(t8, t, "uint8 mask")


# ---- 4, 6: capacity, sentinels, host and device outputs, determinism ------------------------------------------------------------------------

def _raw(a, what, cutoff, capacity, size, args, device=False):
    """snpgpu_select_pairs with outputs of `size` elements filled with sentinels; -> (arrays, n_found)"""
    from snprelate_amd import _lib
    fam = None if args.get("family") is None else np.ascontiguousarray(args["family"], np.int32)
    e = None if args.get("e") is None else np.ascontiguousarray(args["e"], np.float64)
    o = _lib.SelOpts(what, int(bool(args.get("constraint"))), _lib._ptr(fam), _lib._ptr(e), cutoff, None)
    found = ctypes.c_int64(-1)
    if device:
        import torch
        out = [torch.full((size,), -9, dtype=torch.int32, device="cuda") for _ in range(2)] + \
              [torch.full((size,), -9.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        _lib.check(_lib.lib().snpgpu_select_pairs(a._h, ctypes.byref(o), capacity, *[ctypes.c_void_p(x.data_ptr()) for x in out], _lib.DEVICE,
                                                  ctypes.byref(found)))
        return [x.cpu().numpy() for x in out], found.value
    out = [np.full(size, -9, np.int32), np.full(size, -9, np.int32)] + [np.full(size, -9.0) for _ in range(3)]
    _lib.check(_lib.lib().snpgpu_select_pairs(a._h, ctypes.byref(o), capacity, *[_lib._ptr(x) for x in out], _lib.HOST, ctypes.byref(found)))
    return out, found.value


@pytest.mark.parametrize("variant,rows", [("robust", (0, 531)), ("mom", (256, 512)), ("homo", (0, 256))])
def test_capacity_sentinels_host_and_device(variant, rows):
    n = 531
    s = P.stream("mixed", n)
    kind, what, args, cols = _variant(variant, s)
    with _context(kind, n, s.blocks(), None if rows == (0, n) else rows) as a:
        whole = a.select_pairs(what, 0.0, **args)
        total = whole[5]
        assert total > 300
        # count only
        res = a.select_pairs(what, 0.0, capacity=0, **args)
        assert res[5] == total and res[0].size == 0
        cap = total // 3
        for device in (False, True):
            out, found = _raw(a, what, 0.0, cap, cap + 64, args, device)
            assert found == total
            for k, x in enumerate(out):
                full_col = whole[k]
                if full_col is None:                                      # KING-robust: v1 is not written at all
                    assert (x == -9).all()
                    continue
                assert np.array_equal(x[:cap].view(np.int64 if x.dtype == np.float64 else np.int32),
                                      full_col[:cap].view(np.int64 if x.dtype == np.float64 else np.int32)), "output %d, device %s" % (k, device)
                assert (x[cap:] == -9).all(), "output %d written behind the capacity (device %s)" % (k, device)
            # a capacity above the number found: everything, and nothing behind it
            out, found = _raw(a, what, 0.0, total + 50, total + 64, args, device)
            assert found == total
            for k, x in enumerate(out):
                if whole[k] is not None:
                    assert np.array_equal(x[:total], whole[k]) and (x[total:] == -9).all()
        # some outputs absent
        from snprelate_amd import _lib
        o = _lib.SelOpts(what, int(bool(args.get("constraint"))), _lib._ptr(args.get("family")), _lib._ptr(args.get("e")), 0.0, None)
        kin = np.full(cap + 8, -9.0)
        found = ctypes.c_int64(0)
        _lib.check(_lib.lib().snpgpu_select_pairs(a._h, ctypes.byref(o), cap, None, None, None, None, _lib._ptr(kin), _lib.HOST, ctypes.byref(found)))
        assert found.value == total and np.array_equal(kin[:cap], whole[4][:cap]) and (kin[cap:] == -9).all()
        # the wrong kind of context is refused
        wrong = _lib.SEL_KING_HOMO if what != _lib.SEL_KING_HOMO else _lib.SEL_KING_ROBUST
        with pytest.raises(_lib.SnpGpuError, match="does not match the context kind"):
            a.select_pairs(wrong, 0.0)


def test_same_call_twice_gives_identical_arrays():
    n = 531
    s = P.stream("holes", n)
    for variant in ("robust", "mom_constraint"):
        kind, what, args, cols = _variant(variant, s)
        with _context(kind, n, s.blocks()) as a:
            for cutoff in (NAN, 0.0):
                r1 = a.select_pairs(what, cutoff, **args)
                r2 = a.select_pairs(what, cutoff, **args)
                assert r1[5] == r2[5] > 0
                for x, y in zip(r1[:5], r2[:5]):
                    assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ---- 5: planted relatives ---------------------------------------------------------------------------------------------------------------

PLANTED = [(10, 30), (100, 520), (260, 400), (310, 525)]      # inside panel 0, panel 0 -> column >= 512, inside panel 1, panel 1 -> column >= 512


def test_planted_duplicates_are_exactly_what_comes_back():
    from snprelate_amd import _lib
    n = 531
    s = P.stream("mixed", n)
    g = s.g.copy()
    for a_, b_ in PLANTED:
        g[:, b_] = g[:, a_]
    blocks = [g[a_:b_] for a_, b_ in zip(s.cuts[:-1], s.cuts[1:])]
    got = []
    for rows in [(0, n)] + P.panels(n):
        with _context("KING_ROBUST", n, blocks, None if rows == (0, n) else rows) as a:
            i1, i2, ibs0, _, kin, found = a.select_pairs(_lib.SEL_KING_ROBUST, 0.354)
            want = [p for p in PLANTED if rows[0] <= p[0] < rows[1]]
            assert list(zip(i1.tolist(), i2.tolist())) == want and found == len(want), (rows, i1, i2)
            assert (kin == 0.5).all() and (ibs0 == 0.0).all()
            got.append(found)
            if rows == (0, n):                                            # nothing else in this stream reaches 0.13
                assert a.select_pairs(_lib.SEL_KING_ROBUST, 0.13)[5] == len(PLANTED)
    assert got == [4, 2, 2, 0]


# ---- 7: long rows, large indices ------------------------------------------------------------------------------------------------------------

def _slab_selection(n, r0, r1, slabs, cutoff):
    """the reference on a packed slab: its entries are already in the order i ascending, j ascending (test_cpu_ibd_selection shows that
    this is the reference's column-major lower-triangle walk); off-diagonal, kinship >= cutoff"""
    rows = np.arange(r0, r1)
    i = np.repeat(rows, n - rows)
    start = np.cumsum(np.concatenate([[0], (n - rows)[:-1]]))
    j = np.arange(i.size) - np.repeat(start, n - rows) + i
    keep = j > i
    if np.isfinite(cutoff):
        with np.errstate(invalid="ignore"):
            keep &= slabs["kinship"] >= cutoff
    t = dict(ID1=i[keep], ID2=j[keep])
    for k, v in slabs.items():
        t[k] = v[keep]
    return t


@pytest.mark.parametrize("n,rows,n_snp,cutoffs", [(20000, (0, 256), 256, (0.0,)), (70000, (69632, 70000), 128, (0.0, NAN))])
def test_long_rows_and_large_indices(n, rows, n_snp, cutoffs):
    """20 000 columns: about 78 chunks of 64 columns per wave and row; rows 69 632 .. 70 000: absolute indices beyond 65 535"""
    from snprelate_amd import _lib
    g = synth_geno(n, n_snp, missing=0.03, seed=n)
    with _context("KING_ROBUST", n, [g], rows, bmax=n_snp) as a:
        slabs = _finaliser(a, "robust", dict(family=None))
        for cutoff in cutoffs:
            t, found = _table(a.select_pairs(_lib.SEL_KING_ROBUST, cutoff), ("IBS0", None))
            ref = _slab_selection(n, rows[0], rows[1], slabs, cutoff)
            print("SELECT-FIGURE n %d rows %d..%d cutoff %g: %d pairs" % (n, rows[0], rows[1], cutoff, found))
            assert found == ref["ID1"].size > 1000
            _same(t, ref, "n %d rows %d..%d" % (n, rows[0], rows[1]))
            assert t["ID2"].max() > 65535 or n < 65536


# ---- 8: several devices -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices,ppd", [((0, 0, 0), 1), ((0, 0), 2)])
def test_multi_device_selection_equals_the_full_context(devices, ppd):
    from snprelate_amd import _lib
    import oracle as orc
    n, L, blk = 1300, 1500, 1024
    g = synth_geno(n, L, missing=0.03, seed=41)
    e = orc.mom_expect(g)[0]
    for kind, what, args in (("KING_ROBUST", _lib.SEL_KING_ROBUST, {}), ("IBS", _lib.SEL_MOM, dict(e=e, constraint=False))):
        blocks = [g[k:k + blk] for k in range(0, L, blk)]
        with _context(kind, n, blocks, bmax=blk) as a:
            whole = a.select_pairs(what, 0.05, **args)
        total = whole[5]
        assert total > 100
        with _lib.MultiAccumulator(getattr(_lib, kind), n, devices=devices, panels_per_device=ppd, max_block_snps=blk) as m:
            assert m.info()["n_panels"] > 1
            for b in blocks:
                m.feed(b)
            for cap in (None, total // 2, total + 10, 0):
                res = m.select_pairs(what, 0.05, capacity=cap, **args)
                assert res[5] == total
                keep = total if cap is None else min(cap, total)
                for x, y in zip(res[:5], whole[:5]):
                    assert (x is None and y is None) or (x.size == keep and x.tobytes() == y[:keep].tobytes()), (kind, cap)


# ---- 9: the API on the HapMap golden file ---------------------------------------------------------------------------------------------------------

def _api_table(rv):
    return {k: rv[k] for k in rv if k not in ("sample_id", "snp_id", "afreq")}


@pytest.mark.parametrize("method", ["KING-robust", "KING-homo", "MoM"])
def test_api_pairs_equal_selection_of_the_matrices(hapmap, method):
    from snprelate_amd import api
    n = hapmap.n_samp
    fam = np.arange(n) // 3
    mask = np.random.default_rng(5).random(n) < 0.6
    subset = hapmap.sample_id[np.random.default_rng(6).random(n) < 0.7]

    def matrices(**kw):
        if method == "MoM":
            return api.snpgdsIBDMoM(hapmap, verbose=False, **kw)
        return api.snpgdsIBDKING(hapmap, type=method, verbose=False, **kw)

    cases = [dict(), dict(samp_sel=mask), dict(sample_id=subset)]
    if method == "KING-robust":
        cases.append(dict(family_id=fam))
    if method == "MoM":
        cases.append(dict(kinship_constraint=True))
    for kw in cases:
        sel = kw.get("samp_sel")
        mkw = {k: v for k, v in kw.items() if k != "samp_sel"}
        obj = matrices(**mkw)
        for cutoff in (NAN, 0.05):
            got = api.snpgdsIBDPairs(hapmap, method=method, kinship_cutoff=cutoff, verbose=False, **kw)
            ref = api.snpgdsIBDSelection(obj, cutoff, sel)
            _same(_api_table(got), ref, "%s %s cutoff %r" % (method, sorted(kw), cutoff))
            assert got["ID1"].size > 0 and np.isin(got["ID1"], hapmap.sample_id).all() and np.isin(got["ID2"], hapmap.sample_id).all()
            assert np.array_equal(got["sample_id"], obj["sample_id"]) and np.array_equal(got["snp_id"], obj["snp_id"])
            if method == "MoM":
                assert np.array_equal(got["afreq"], obj["afreq"], equal_nan=True)
            else:
                assert "afreq" not in got
    # a permuting numeric selection: refused here, accepted on the matrices
    perm = np.random.default_rng(9).permutation(n)[:40]
    with pytest.raises(ValueError, match="snpgdsIBDSelection"):
        api.snpgdsIBDPairs(hapmap, method=method, samp_sel=perm, verbose=False)
    t = api.snpgdsIBDSelection(matrices(), NAN, perm)
    assert t["ID1"].size == 40 * 39 // 2 and t["ID1"][0] == hapmap.sample_id[perm[0]]
    inc = np.sort(perm)
    _same(_api_table(api.snpgdsIBDPairs(hapmap, method=method, kinship_cutoff=0.05, samp_sel=inc, verbose=False)),
          api.snpgdsIBDSelection(matrices(), 0.05, inc), "increasing indices")
