"""GPU tests of snpgdsPairScore.  Every comparison is exact (np.array_equal, NaN positions equal): the kernels count integers and the
host finaliser runs the reference's fp64 operations on them, so there is nothing to tolerate.  The expected values come from the
vectorised restatement of tests/pair_score_ref.py (itself checked against the loop form on the CPU) and, for IBS, from
snpgdsIBSNum, which shares no code with the feature."""
import numpy as np
import pytest

import pair_score_ref as P
from input_forms import scramble_padding as _scramble_padding
from oracle.synth import synth_hash_block_packed
from snprelate_amd import _lib, api, gds
from snprelate_amd.gds import pack_2bit_rows, unpack_2bit_rows

pytestmark = pytest.mark.gpu
CASES = [(m, d) for m in P.METHODS for d in (True, False)]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _pairs(n_samp, n_pair, seed):
    """two lists without duplicates; with room for them, pair 0 is a self pair and pair 1's first member is also pair 2's second"""
    rng = np.random.default_rng(seed)
    a, b = rng.permutation(n_samp)[:n_pair], rng.permutation(n_samp)[:n_pair]
    if n_pair >= 3:
        def put(lst, pos, val):                                      # lst[pos] = val, keeping the list free of duplicates
            at = np.flatnonzero(lst == val)
            if len(at):
                lst[at[0]] = lst[pos]
            lst[pos] = val
        put(b, 0, a[0])
        put(b, 2, a[1])
    return a.astype(np.int32), b.astype(np.int32)


def _edge_case(n_samp, n_pair, n_snp, missing, seed):
    g = unpack_2bit_rows(synth_hash_block_packed(n_samp, 0, n_snp, seed, missing=missing), n_samp)
    idx1, idx2 = _pairs(n_samp, n_pair, seed)
    if n_snp > 2:
        g[1] = 3                                                     # an all-missing SNP
        g[n_snp - 1] = 1                                             # gsum == n: the tie, no flip
    if n_samp > 2:
        g[:, idx1[-1]] = 3                                           # an all-missing listed sample
    if n_snp > 4:
        g[3] = np.where(np.arange(n_samp) % 5 == 0, 1, 0)            # mostly 0: gsum < n for all but the smallest lists, flipped
        g[3, idx1[-1]] = 3 if n_samp > 2 else g[3, idx1[-1]]
    return g, idx1, idx2


def _check_all(g, idx1, idx2, src, n_samp, fmt, n_snp, what):
    """every method x dosage x type through the C ABI wrappers on one input"""
    want_tab = {mj: P.tables(g, idx1, idx2, mj) for mj in (False, True)}
    for mj in (False, True):
        pt, st, fl = _lib.pair_tables(src, n_samp, idx1, idx2, need_major=mj, fmt=fmt, n_snp=n_snp)
        assert _same(pt, want_tab[mj][0]) and _same(st, want_tab[mj][1]) and _same(fl, want_tab[mj][2]), (what, mj)
        for method, dosage in CASES:
            if P.score_map(method, dosage)[1] != mj:
                continue
            got = _lib.pair_score_final(pt, method, dosage)
            want = P.pair_score_ref(g, idx1, idx2, method, "per.pair", dosage)
            assert all(_same(a, b) for a, b in zip(got, want)), (what, method, dosage, "per.pair")
            got = np.stack(_lib.pair_score_final(st, method, dosage, flip=fl))
            assert _same(got, P.pair_score_ref(g, idx1, idx2, method, "per.snp", dosage)), (what, method, dosage, "per.snp")
    for method, dosage in CASES:
        want = P.pair_score_ref(g, idx1, idx2, method, "matrix", dosage)
        got = _lib.pair_score_matrix(src, n_samp, idx1, idx2, method, dosage, fmt=fmt, n_snp=n_snp)
        assert got.dtype == np.int32 and _same(got.T, want), (what, method, dosage, "matrix")
        got = _lib.pair_score_matrix(src, n_samp, idx1, idx2, method, dosage, bit2=True, fmt=fmt, n_snp=n_snp)
        assert got.dtype == np.uint8 and _same(got.T, P.bit2(want)), (what, method, dosage, "bit2")


@pytest.mark.parametrize("n_samp,n_pair,n_snp,missing", [(2, 1, 1, 0.0), (5, 1, 15, 0.3), (63, 63, 16, 0.05), (130, 64, 17, 0.3),
                                                         (130, 65, 33, 0.0), (130, 130, 1000, 0.05)])
def test_edge_shapes(n_samp, n_pair, n_snp, missing, monkeypatch):
    import torch
    g, idx1, idx2 = _edge_case(n_samp, n_pair, n_snp, missing, seed=n_samp + n_pair + n_snp)
    packed = _scramble_padding(pack_2bit_rows(g), n_samp)
    raw = g.copy()
    raw[(g == 3) & (np.random.default_rng(1).random(g.shape) < 0.5)] = 200
    dev = torch.from_numpy(packed).cuda()
    dev8 = torch.from_numpy(raw).cuda()
    shifted = torch.full((packed.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    shifted[5:5 + packed.size] = dev.reshape(-1)
    torch.cuda.synchronize()
    inputs = (("packed host", packed, _lib.GENO_PACKED2, None), ("u8 host", raw, _lib.GENO_U8, None),
              ("packed device", int(dev.data_ptr()), _lib.GENO_PACKED2, n_snp), ("u8 device", int(dev8.data_ptr()), _lib.GENO_U8, n_snp),
              ("packed device + 5 bytes", int(shifted.data_ptr()) + 5, _lib.GENO_PACKED2, n_snp))
    for block in (None, "16"):
        if block is None:
            monkeypatch.delenv("SNPGPU_PAIR_BLOCK_SNPS", raising=False)
        elif n_snp <= 16:
            continue
        else:
            monkeypatch.setenv("SNPGPU_PAIR_BLOCK_SNPS", block)
        for name, src, fmt, m in inputs if block is None else inputs[:3]:
            _check_all(g, idx1, idx2, src, n_samp, fmt, m, (name, block))
            if block == "16" and name == "packed host":
                _lib.pair_tables(src, n_samp, idx1, idx2, fmt=fmt, want_pair=False)
                assert _lib.pair_stats()["snp_table_launches"] == (n_snp + 15) // 16


def test_tables_directly():
    n_samp, n_snp = 77, 210
    g, idx1, idx2 = _edge_case(n_samp, 70, n_snp, 0.1, seed=21)
    packed = _scramble_padding(pack_2bit_rows(g), n_samp)
    for mj in (False, True):
        want = P.tables(g, idx1, idx2, mj)
        assert want[2].any() and not want[2].all()
        for sel in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, False, True)):
            got = _lib.pair_tables(packed, n_samp, idx1, idx2, need_major=mj, fmt=_lib.GENO_PACKED2, want_pair=sel[0], want_snp=sel[1],
                                   want_flip=sel[2])
            for k in range(3):
                assert (got[k] is None) if not sel[k] else _same(got[k], want[k]), (mj, sel, k)
    # the two pair tables differ exactly where a flipped SNP is called
    assert not _same(P.tables(g, idx1, idx2, False)[0], P.tables(g, idx1, idx2, True)[0])


def test_row_longer_than_the_lds_stage():
    """rows of more than 60 KiB are gathered from global memory: another kernel instance"""
    import torch
    n_samp, n_snp, n_pair = 250001, 5, 130
    rng = np.random.default_rng(12)
    g = rng.integers(0, 4, (n_snp, n_samp)).astype(np.uint8)
    idx1, idx2 = _pairs(n_samp, n_pair, 4)
    idx1[5], idx2[6] = n_samp - 1, n_samp - 1
    g[3, idx1] = 0
    g[3, idx2] = np.where(np.arange(n_pair) % 7 == 0, 1, 0)          # flipped
    packed = _scramble_padding(pack_2bit_rows(g), n_samp)
    dev = torch.from_numpy(packed).cuda()
    torch.cuda.synchronize()
    for src, m in ((packed, None), (int(dev.data_ptr()), n_snp)):
        for mj in (False, True):
            got = _lib.pair_tables(src, n_samp, idx1, idx2, need_major=mj, fmt=_lib.GENO_PACKED2, n_snp=m)
            assert all(_same(a, b) for a, b in zip(got, P.tables(g, idx1, idx2, mj)))
        for method in ("IBS", "GVH.minor.only"):
            got = _lib.pair_score_matrix(src, n_samp, idx1, idx2, method, fmt=_lib.GENO_PACKED2, n_snp=m)
            assert _same(got.T, P.pair_score_ref(g, idx1, idx2, method, "matrix"))


@pytest.fixture(scope="module")
def hapmap_pairs(hapmap):
    rng = np.random.default_rng(40)
    sid = np.asarray(hapmap.sample_id)
    s1, s2 = sid[rng.permutation(len(sid))[:40]].copy(), sid[rng.permutation(len(sid))[:40]].copy()
    if s1[0] not in s2:
        s2[0] = s1[0]                                                # a self pair
    snp = np.asarray(hapmap.snp_id)[200:4200:3]
    union = np.isin(sid, np.concatenate([s1, s2]))
    wsid = sid[union]
    g = unpack_2bit_rows(hapmap.packed, hapmap.n_samp)[np.isin(hapmap.snp_id, snp)][:, union]
    pos = {s: i for i, s in enumerate(wsid)}
    idx1, idx2 = np.array([pos[s] for s in s1], np.int32), np.array([pos[s] for s in s2], np.int32)
    return dict(s1=s1, s2=s2, snp=snp, wsid=wsid, g=g, idx1=idx1, idx2=idx2)


@pytest.mark.parametrize("method,dosage", CASES)
def test_hapmap_api(hapmap, hapmap_pairs, method, dosage, capsys):
    h = hapmap_pairs
    g, idx1, idx2 = h["g"], h["idx1"], h["idx2"]
    r = api.snpgdsPairScore(hapmap, h["s1"], h["s2"], snp_id=h["snp"], method=method, type="per.pair", dosage=dosage, verbose=False)
    assert list(r["sample_id"]) == list(h["wsid"]) and list(r["snp_id"]) == list(h["snp"])
    avg, sd, num = P.pair_score_ref(g, idx1, idx2, method, "per.pair", dosage)
    sc = r["score"]
    assert list(sc) == ["Avg", "SD", "Num", "Sample1", "Sample2"] and sc["Num"].dtype == np.int32
    assert _same(sc["Avg"], avg) and _same(sc["SD"], sd) and _same(sc["Num"], num)
    assert list(sc["Sample1"]) == list(h["s1"]) and list(sc["Sample2"]) == list(h["s2"])
    r = api.snpgdsPairScore(hapmap, h["s1"], h["s2"], snp_id=h["snp"], method=method, type="per.snp", dosage=dosage, with_id=False,
                            verbose=False)
    assert list(r) == ["score"] and r["score"].shape == (3, len(h["snp"]))
    assert _same(r["score"], P.pair_score_ref(g, idx1, idx2, method, "per.snp", dosage))
    capsys.readouterr()
    r = api.snpgdsPairScore(hapmap, h["s1"], h["s2"], snp_id=h["snp"], method=method, type="matrix", dosage=dosage)
    want = P.pair_score_ref(g, idx1, idx2, method, "matrix", dosage)
    assert r["score"].dtype == np.int32 and r["score"].shape == (40, len(h["snp"])) and _same(r["score"], want)
    assert (r["score"] == api._NA_INTEGER).any()
    assert capsys.readouterr().out == ("Pair Score Calculation:\n    # of samples: %d\n    # of SNPs: %s\nMethod: %s\n" %
                                       (len(h["wsid"]), "{:,}".format(len(h["snp"])), method))


def test_hapmap_gds_file(hapmap, hapmap_pairs, tmp_path):
    h = hapmap_pairs
    fn = str(tmp_path / "score.gds")
    for method in ("HVG", "GVH.major.only"):
        r = api.snpgdsPairScore(hapmap, h["s1"], h["s2"], snp_id=h["snp"], method=method, type="gds.file", output=fn, verbose=False)
        assert list(r) == ["sample_id", "snp_id"]
        nodes = gds.read_output(fn)
        want = P.pair_score_ref(h["g"], h["idx1"], h["idx2"], method, "matrix")
        assert nodes["genotype"].dtype == np.uint8 and _same(nodes["genotype"], P.bit2(want))
        assert list(nodes["genotype.attr"]) == ["sample.order"]
        assert list(nodes["sample.id"]) == ["%s-%s" % (a, b) for a, b in zip(h["s1"], h["s2"])]
        flag = np.isin(hapmap.snp_id, h["snp"])
        assert _same(nodes["snp.id"], h["snp"]) and _same(nodes["snp.chromosome"], np.asarray(hapmap.snp_chromosome)[flag])
        assert _same(nodes["snp.position"], np.asarray(hapmap.snp_position)[flag])
    assert (P.bit2(want) == 3).sum() > (want == P.NA_INTEGER).sum()  # scores of -1 are kept as 3, as a bit2 node keeps them


def test_ibs_against_ibsnum(hapmap, hapmap_pairs):
    """independent of the restatement: Avg Num = 2 ibs2 + ibs1 and Num = ibs0 + ibs1 + ibs2 of snpgdsIBSNum, filters off"""
    h = hapmap_pairs
    r = api.snpgdsPairScore(hapmap, h["s1"], h["s2"], snp_id=h["snp"], method="IBS", type="per.pair", dosage=True, verbose=False)
    c = api.snpgdsIBSNum(hapmap, sample_id=h["wsid"], snp_id=h["snp"], autosome_only=False, remove_monosnp=False, missing_rate=float("nan"),
                         verbose=False)
    assert list(c["sample_id"]) == list(r["sample_id"]) and list(c["snp_id"]) == list(r["snp_id"])
    i0, i1, i2 = (c[k][h["idx1"], h["idx2"]].astype(np.int64) for k in ("ibs0", "ibs1", "ibs2"))
    sc = r["score"]
    assert np.array_equal(sc["Num"], i0 + i1 + i2) and (sc["Num"] > 1).all()
    # Avg is the one fp64 division Sum / Num, so it is compared as that quotient, bit for bit; Avg Num is within Sum 2^-52 < 1/2 of
    # the integer Sum, which it therefore rounds to
    assert np.array_equal(sc["Avg"], (2 * i2 + i1) / (i0 + i1 + i2).astype(np.float64))
    assert np.array_equal(np.rint(sc["Avg"] * sc["Num"]).astype(np.int64), 2 * i2 + i1)


def test_scale_device_rows():
    import torch
    N, M, n_pair = 2000, 20000, 1000
    rb = (N + 3) // 4
    dev = torch.empty(M * rb, dtype=torch.uint8, device="cuda")
    _lib.synth_block(dev.data_ptr(), N, 0, M, seed=31, missing=0.01)
    torch.cuda.synchronize()
    g = unpack_2bit_rows(dev.cpu().numpy().reshape(M, rb), N)
    idx1, idx2 = _pairs(N, n_pair, 9)
    ptr = int(dev.data_ptr())
    for method in ("IBS", "GVH.minor.only"):
        mj = P.score_map(method, True)[1]
        pt, st, fl = _lib.pair_tables(ptr, N, idx1, idx2, need_major=mj, fmt=_lib.GENO_PACKED2, n_snp=M)
        stats = _lib.pair_stats()
        assert stats["snp_table_launches"] == 1 and stats["snp_table_bytes"] == M * rb and stats["pair_count_ms"] > 0
        got = _lib.pair_score_final(pt, method, True)
        assert all(_same(a, b) for a, b in zip(got, P.pair_score_ref(g, idx1, idx2, method, "per.pair")))
        got = np.stack(_lib.pair_score_final(st, method, True, flip=fl))
        assert _same(got, P.pair_score_ref(g, idx1, idx2, method, "per.snp"))
        assert 0 < fl.sum() < M
        sl = slice(7000, 7512)
        got = _lib.pair_score_matrix(ptr + sl.start * rb, N, idx1, idx2, method, fmt=_lib.GENO_PACKED2, n_snp=512)
        assert _same(got.T, P.pair_score_ref(g[sl], idx1, idx2, method, "matrix"))


def test_errors_with_a_device():
    g = np.zeros((4, 5), np.uint8)
    a = np.array([0, 1], np.int32)
    for bad in (np.array([2, 5], np.int32), np.array([-1, 2], np.int32)):
        with pytest.raises(_lib.SnpGpuError, match="out of range"):
            _lib.pair_tables(g, 5, a, bad)
        with pytest.raises(_lib.SnpGpuError, match="out of range"):
            _lib.pair_score_matrix(g, 5, bad, a)
    with pytest.raises(_lib.SnpGpuError, match="no pair"):
        _lib.pair_tables(g, 5, a[:0], a[:0])
    with pytest.raises(_lib.SnpGpuError, match="all NULL"):
        _lib.pair_tables(g, 5, a, a, want_pair=False, want_snp=False, want_flip=False)
    with pytest.raises(ValueError, match="'method' should be one of"):
        _lib.pair_score_matrix(g, 5, a, a, method="IBD")
    L = _lib.lib()
    out = np.zeros(8, np.float64)
    assert L.snpgpu_gnrPairScore(_lib._ptr(a), _lib._ptr(a), 2, b"IBS", b"per.sample", 1, 0, _lib._ptr(out)) == 1
    assert b"Invalid 'type'." in L.snpgpu_last_error()
    assert L.snpgpu_gnrPairScore(_lib._ptr(a), _lib._ptr(a), 2, b"IBS", b"per.pair", 1, 0, None) == 1
    # a valid call still works afterwards
    pt, st, fl = _lib.pair_tables(g, 5, a, a)
    assert pt[:, 0, 0].tolist() == [4, 4] and st[:, 0, 0].tolist() == [2] * 4 and fl.tolist() == [1] * 4
