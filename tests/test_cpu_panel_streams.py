"""The inputs of tests/test_gpu_panel_finalisers.py cannot pass vacuously: assertions on tests/panel_streams.py and its references alone
(no GPU).  The block kinds are as declared, the NaN entries lie where the holes were cut, the family vector and `diagadj` change entries of
every panel, and a result computed with a panel-relative index in place of an absolute one -- emulated in numpy on the references --
fails the very comparison functions the GPU tests call."""
import numpy as np
import pytest

import oracle as orc
import panel_streams as P

CASES = [(name, n) for n in P.SAMPLE_COUNTS for name in ("mixed", "holes")]


@pytest.mark.parametrize("name,n", CASES)
def test_streams_are_what_they_are_declared_to_be(name, n):
    s = P.stream(name, n)
    blocks = s.blocks()
    assert [(len(b), bool((b > 2).any())) for b in blocks] == list(P.BLOCKS[name])
    assert all(len(b) <= P.BMAX for b in blocks) and s.g.shape == (sum(len(b) for b in blocks), n) and s.g.shape[0] <= 2088
    assert P.panels(n)[-1] == (512, n) and all(r0 % P.PANEL_ALIGN == 0 for r0, _ in P.panels(n))
    called = s.g < 3
    if name == "mixed":
        mono = np.flatnonzero((np.where(called, s.g, 0).sum(1) == 2 * called.sum(1)) & called.all(1))
        assert mono.size and all(s.cuts[1] <= k < s.cuts[2] for k in mono)           # monomorphic, in the block without missing calls
        gone = np.flatnonzero(~called.any(1))
        assert gone.tolist() == [int(s.cuts[0]) + 9]                                 # all-missing, in a block with them
    else:
        hi, half = P.second_half_only(n), s.g.shape[0] // 2
        assert not called[:, P.NEVER_CALLED].any()
        assert not called[half:, P.FIRST_HALF_ONLY].any() and called[:half, P.FIRST_HALF_ONLY].mean() > 0.9
        assert not called[:half, hi].any() and called[half:, hi].mean() > 0.9
        assert P.FIRST_HALF_ONLY < 256 <= P.NEVER_CALLED < 512 <= hi < n


def _pairs_where(mask, n):
    i, j = P.slab_rc(n, 0, n)
    return set(zip(i[mask].tolist(), j[mask].tolist()))


@pytest.mark.parametrize("n", P.SAMPLE_COUNTS)
def test_holes_put_nan_at_the_listed_pairs_and_nowhere_else(n):
    s = P.stream("holes", n)
    assert _pairs_where(np.isnan(s.ibs_ave()), n) == P.holes_nan_pairs(n, diagonal=True)
    ibs0, kin = s.king_robust(None)
    for fam in (None, "fam"):
        for x in s.king_robust(fam):
            assert _pairs_where(np.isnan(x), n) == P.holes_nan_pairs(n, diagonal=False) and not np.isinf(x).any()
    k0, k1 = s.king_homo()
    # (KING-homo's own diagonal is 0; every pair without a shared call is NaN there too)
    assert P.holes_nan_pairs(n, diagonal=False) <= _pairs_where(np.isnan(k0), n)
    # panels 0 and 1: a NaN and a finite entry within one 32-row group of the finalisers
    hi = P.second_half_only(n)
    for rows, nan_pair in (((0, 256), (P.FIRST_HALF_ONLY, hi)), ((256, 512), (P.NEVER_CALLED, hi))):
        i, j = P.slab_rc(n, *rows)
        x = P.slab(s.ibs_ave(), n, *rows)
        grp = (i - rows[0]) // P.FIN_ROWS == (nan_pair[0] - rows[0]) // P.FIN_ROWS
        assert np.isnan(x[(i == nan_pair[0]) & (j == nan_pair[1])]).all()
        assert np.isnan(x[grp]).any() and np.isfinite(x[grp]).any()
    assert not np.isnan(P.stream("mixed", n).ibs_ave()).any()


@pytest.mark.parametrize("name,n", CASES)
def test_family_vector_changes_entries_of_every_panel(name, n):
    s, fam = P.stream(name, n), P.family_vector(n)
    assert 0.3 < (fam < 0).mean() < 0.37
    sizes = np.unique(fam[fam >= 0], return_counts=True)[1]
    assert set(sizes.tolist()) == {2, 3, 4}
    with_fam, without = s.king_robust("fam")[1], s.king_robust(None)[1]
    for name_, (i, j) in P.family_pairs(n).items():
        row0 = i // P.PANEL_ALIGN * P.PANEL_ALIGN
        assert fam[i] == fam[j] >= 0, name_
        if row0:
            assert fam[i - row0] != fam[j] and not (fam[i - row0] == fam[j - row0] >= 0), name_     # relative row, or both relative
        k = P.tri_idx(n, i, j)
        assert abs(with_fam[k] - without[k]) > 1e-3, (name_, with_fam[k], without[k])
    rows_of = {"inside_panel_0": 0, "panel_0_to_last": 0, "inside_panel_1": 1, "panel_1_to_last": 1, "inside_panel_2": 2}
    assert {rows_of[k] for k in P.family_pairs(n)} == ({0, 1, 2} if n == 531 else {0, 1})
    for p, rows in enumerate(P.panels(n)):
        d = np.abs(P.slab(with_fam, n, *rows) - P.slab(without, n, *rows))
        if (n, p) == (513, 2):
            assert d.size == 1                     # its diagonal entry alone: 0.5 whatever the families
        else:
            assert np.nanmax(d) > 1e-3


@pytest.mark.parametrize("n", P.SAMPLE_COUNTS)
def test_diagadj_changes_the_diagonal_of_every_panel(n):
    """by more than 100 x the 1e-5 the GPU test holds EIGMIX to, in the same figure"""
    s = P.stream("mixed", n)
    for rows in P.panels(n):
        e = P.rel_err(P.slab(s.eigmix(True), n, *rows), P.slab(s.eigmix(False), n, *rows), s.eigmix(False))
        d = P.diag_offsets(n, *rows)
        assert e[d].min() > 100 * 1e-5
        off = np.ones(e.size, bool)
        off[d] = False
        assert not e[off].any()


# ---- a panel-relative index in place of an absolute one, emulated on the references --------------------------------------------------

def _later_panels(n):
    return [rows for rows in P.panels(n) if rows[0] > 0]


@pytest.mark.parametrize("name,n", CASES)
def test_relative_family_lookup_fails_the_gpu_comparison(name, n):
    """fam[i - row0] for the row sample (the column lookup stays absolute): both branches of every pair come from the oracle, the
    emulation picks between them"""
    s, fam = P.stream(name, n), P.family_vector(n)
    branch_fam, branch_none = s.king_robust("one")[1], s.king_robust(None)[1]
    i, j = P.slab_rc(n, 0, n)

    def pick(row0):
        f1, f2 = fam[(i - row0) % n], fam[j]
        return np.where((i != j) & (f1 == f2) & (f1 >= 0), branch_fam, branch_none)
    assert np.array_equal(pick(0), s.king_robust("fam")[1], equal_nan=True)          # the emulation with the true lookup IS the oracle
    for rows in _later_panels(n):
        got = (P.slab(s.king_robust("fam")[0], n, *rows), P.slab(pick(rows[0]), n, *rows))
        if (n, rows) == (513, (512, 513)):
            P.check_king_robust(got, "fam", s, rows)                                 # one diagonal entry: nothing to look up
            continue
        with pytest.raises(AssertionError, match="kinship differs at"):
            P.check_king_robust(got, "fam", s, rows)
        P.check_king_robust((got[0], P.slab(s.king_robust("fam")[1], n, *rows)), "fam", s, rows)


@pytest.mark.parametrize("n", P.SAMPLE_COUNTS)
@pytest.mark.parametrize("diagadj", [True, False])
def test_relative_diagonal_terms_fail_the_gpu_comparison(diagadj, n):
    """EIGMIX's diagonal comes from per-sample sums (dsq[i], het[i]): read at i - row0, entry (i, i) is that of sample i - row0"""
    s = P.stream("mixed", n)
    whole = s.eigmix(diagadj)
    for rows in _later_panels(n):
        got = P.slab(whole, n, *rows).copy()
        P.check_eigmix(got, diagadj, s, rows)
        i = np.arange(*rows)
        got[P.diag_offsets(n, *rows)] = whole[P.tri_idx(n, i - rows[0], i - rows[0])]
        with pytest.raises(AssertionError, match="eigmix.*rel err"):
            P.check_eigmix(got, diagadj, s, rows)
        # all entries together and the diagonal alone each catch it
        with pytest.raises(AssertionError):
            P.check_rel("eigmix", got, P.slab(whole, n, *rows), whole, s, rows, only=P.diag_offsets(n, *rows))


@pytest.mark.parametrize("n", P.SAMPLE_COUNTS)
def test_relative_missing_counts_fail_the_gpu_comparison(n):
    """GCTA divides by 2 (nLocus - Denom), Denom(i, j) = M(i, i) + M(j, j) - M(i, j) with M the both-missing counts over the polymorphic
    SNPs; M(i, i) read at i - row0 changes the divisor of the whole row.  On the holes stream M(s, s) is all, half or 6 % of the SNPs."""
    s = P.stream("holes", n)
    called = s.g < 3
    tot = np.where(called, s.g, 0).sum(1)
    poly = (tot > 0) & (tot < 2 * called.sum(1))
    m = (~called[poly]).astype(np.float64)
    nl, diag, both = float(poly.sum()), m.sum(0), m.T @ m
    i, j = P.slab_rc(n, 0, n)
    grm = s.grm()
    fin = np.isfinite(grm)
    assert _pairs_where(~fin, n) == P.holes_nan_pairs(n, diagonal=True)        # one of the two is missing at every SNP: 0 / 0
    for rows in _later_panels(n):
        P.check_gcta(P.slab(grm, n, *rows), s, rows)
        if (n, rows) == (513, (512, 513)):
            continue                               # one entry: i - row0 = 0, whose count differs by chance only
        with np.errstate(divide="ignore", invalid="ignore"):
            wrong = grm * (nl - (diag[i] + diag[j] - both[i, j])) / (nl - (diag[(i - rows[0]) % n] + diag[j] - both[i, j]))
        wrong = np.where(fin, wrong, grm)
        with pytest.raises(AssertionError, match="grm_gcta"):
            P.check_gcta(P.slab(wrong, n, *rows), s, rows)


def test_comparisons_name_the_pattern():
    s = P.stream("mixed", 531)
    rows = (256, 512)
    ref = P.slab(s.ibs_ave(), 531, *rows)
    got = ref.copy()
    got[P.diag_offsets(531, *rows)[3:5]] += 1.0
    with pytest.raises(AssertionError, match=r"2 of \d+ entries of rows 256..512 .*2 on the diagonal; first \(row, column\): \[\(259, 259\), \(260, 260\)\]"):
        P.check_exact("ibs_ave", got, ref, s, rows)
    with pytest.raises(AssertionError, match="NaN / Inf placement"):
        P.check_close("x", np.where(np.arange(ref.size) == 7, np.nan, ref), ref, s, rows, rtol=1e-5)
    P.check_close("x", ref * (1 + 5e-6), ref, s, rows, rtol=1e-5)
    with pytest.raises(AssertionError, match="beyond rtol"):
        P.check_close("x", ref * (1 + 2e-5), ref, s, rows, rtol=1e-5)
    h = P.stream("holes", 531)
    nan_ref = P.slab(h.ibs_ave(), 531, *rows)
    assert np.isnan(nan_ref).any()
    P.check_close("x", nan_ref.copy(), nan_ref, h, rows, rtol=1e-12)                 # NaN where the reference has NaN is agreement
    P.check_exact("x", nan_ref.copy(), nan_ref, h, rows)
    with pytest.raises(AssertionError, match="NaN / Inf placement"):
        P.check_close("x", np.nan_to_num(nan_ref), nan_ref, h, rows, rtol=1e-12)
    assert orc.tri_size(531) ==P.slab_rc(531, 0, 531)[0].size
