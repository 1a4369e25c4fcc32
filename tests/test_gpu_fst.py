"""GPU tests of snpgdsFst / snpgdsSlidingWindow: the per-population counters bit-exact against numpy, the HapMap fixture through
the API against the restatement (tests/fst_ref.py) within its derived rounding bounds -- the only tolerance used -- and the
one-pass window scan against snpgdsFst called on each window's SNPs.  No case is skipped or masked: every compared entry counts and
NaN patterns must be equal."""
import numpy as np
import pytest

import fst_ref as R
from input_forms import scramble_padding as _scramble_padding
from oracle.synth import synth_hash_geno
from snprelate_amd import _lib, api
from snprelate_amd.gds import pack_2bit_rows

pytestmark = pytest.mark.gpu
METHODS = ("W&C84", "W&H02")


def _genotypes(n, m, n_pop, missing, seed):
    rng = np.random.default_rng(seed)
    pop = rng.integers(0, n_pop, n).astype(np.int32)
    pop[rng.permutation(n)[:min(n, n_pop)]] = np.arange(min(n, n_pop))          # every population present when n >= n_pop
    g = rng.integers(0, 3, (m, n)).astype(np.uint8)
    g[rng.random((m, n)) < missing] = 3
    for s in range(0, m, 7):                                                    # a population entirely missing at some SNPs
        g[s][pop == (s // 7) % n_pop] = 3
    return g, pop


def _within(got, want, bound, what):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN pattern"
    ok = ~np.isnan(want)
    inf = ok & np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    fin = ok & ~inf
    err = np.abs(got[fin] - want[fin])
    print("%s: max |diff| %.3e, max bound %.3e, entries %d" % (what, err.max() if err.size else 0.0,
                                                               bound[fin].max() if err.size else 0.0, int(fin.sum())))
    assert (err <= bound[fin]).all(), what


def _check_fst_result(res, want, method, levels):
    """Fst, MeanFst, FstSNP (NaN pattern equal) and Beta of an api.snpgdsFst result against the restatement within its bounds"""
    _within(res["Fst"], want["Fst"], want["Fst_bound"], "Fst")
    _within(res["FstSNP"], want["FstSNP"], want["FstSNP_bound"], "FstSNP")
    ok = ~np.isnan(want["FstSNP"])
    # a mean of values each within its bound, plus the rounding of the mean's own sum
    _within(res["MeanFst"], want["MeanFst"], float(np.mean(want["FstSNP_bound"][ok])) + 4 * ok.sum() * R.U * float(
        np.mean(np.abs(want["FstSNP"][ok]))), "MeanFst")
    if method == "W&H02":
        _within(res["Beta"], want["Beta"], want["Beta_bound"], "Beta")
        assert np.array_equal(res["Beta"], res["Beta"].T) and res["Beta_levels"] == levels
        assert res["Beta"].shape == (len(levels), len(levels))
    else:
        assert "Beta" not in res and "Beta_levels" not in res


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 130, 2049])
@pytest.mark.parametrize("n_pop", [2, 3, 7, 26, 40])
def test_pop_counts_bit_exact(n, n_pop):
    import torch
    if n < n_pop:
        n_pop_eff = n                      # fewer samples than populations cannot fill them: the largest count that can
    else:
        n_pop_eff = n_pop
    for missing in (0.0, 0.05, 0.30):
        g, pop = _genotypes(n, 53, n_pop_eff, missing, seed=n * 100 + n_pop)
        wa, wc = R.pop_counts(g, pop, n_pop_eff)
        packed = _scramble_padding(pack_2bit_rows(g), n)
        raw = g.copy()
        raw[(g == 3) & (np.random.default_rng(1).random(g.shape) < 0.5)] = 200      # any byte > 2 is missing
        dev = torch.from_numpy(packed).cuda()
        dev_u8 = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        inputs = (("packed host", packed, _lib.GENO_PACKED2, None), ("u8 host", raw, _lib.GENO_U8, None),
                  ("packed device", int(dev.data_ptr()), _lib.GENO_PACKED2, g.shape[0]),
                  ("u8 device", int(dev_u8.data_ptr()), _lib.GENO_U8, g.shape[0]))
        for name, src, fmt, n_snp in inputs:
            a, c = _lib.pop_counts(src, n, pop, n_pop_eff, fmt=fmt, n_snp=n_snp)
            assert np.array_equal(a, wa) and np.array_equal(c, wc), (name, n, n_pop_eff, missing)
        assert (wc == 0).any()                                                   # a population without a call at some SNPs


@pytest.mark.parametrize("n", [8, 16, 69, 80, 40, 96])
@pytest.mark.parametrize("n_pop", [2, 5])
def test_pop_counts_row_lengths_of_every_line_period(n, n_pop):
    """rb = 2, 4, 18, 20, 10, 24 bytes: gcd(rb, 16) = 2, 4, 2, 4, 2, 8, i.e. 8, 4 or 2 mask variants, with 131 SNPs so that every
    variant has several workgroups (the other tests run gcd 1, 8 and 16)"""
    import torch
    g, pop = _genotypes(n, 131, n_pop, 0.1, seed=n + n_pop)
    wa, wc = R.pop_counts(g, pop, n_pop)
    packed = _scramble_padding(pack_2bit_rows(g), n)
    for shift in (0, 6):
        buf = torch.full((packed.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        buf[shift:shift + packed.size] = torch.from_numpy(packed.reshape(-1)).cuda()
        torch.cuda.synchronize()
        a, c = _lib.pop_counts(int(buf.data_ptr()) + shift, n, pop, n_pop, fmt=_lib.GENO_PACKED2, n_snp=g.shape[0])
        assert np.array_equal(a, wa) and np.array_equal(c, wc), (n, shift)
    a, c = _lib.pop_counts(packed, n, pop, n_pop)
    assert np.array_equal(a, wa) and np.array_equal(c, wc)


def test_pop_counts_unaligned_device_rows_and_blocks(monkeypatch):
    """rows that start anywhere inside a 16-byte line (device pointer offset by 1 ... 15 bytes) and several streamed blocks"""
    import torch
    n, n_pop = 131, 5
    g, pop = _genotypes(n, 97, n_pop, 0.1, seed=7)
    wa, wc = R.pop_counts(g, pop, n_pop)
    packed = _scramble_padding(pack_2bit_rows(g), n)
    monkeypatch.setenv("SNPGPU_POP_BLOCK_SNPS", "32")
    for shift in (0, 1, 5, 8, 15):
        buf = torch.full((packed.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")        # called genotypes around the rows
        buf[shift:shift + packed.size] = torch.from_numpy(packed.reshape(-1)).cuda()
        torch.cuda.synchronize()
        a, c = _lib.pop_counts(int(buf.data_ptr()) + shift, n, pop, n_pop, fmt=_lib.GENO_PACKED2, n_snp=g.shape[0])
        assert np.array_equal(a, wa) and np.array_equal(c, wc), shift
    a, c = _lib.pop_counts(packed, n, pop, n_pop)
    assert np.array_equal(a, wa) and np.array_equal(c, wc)
    assert _lib.pop_stats()[1] == 4                                                         # 97 SNPs in blocks of 32


@pytest.mark.parametrize("method", METHODS)
def test_c_abi_fst_and_windows_match_restatement(method):
    n, n_pop = 77, 4
    g, pop = _genotypes(n, 211, n_pop, 0.08, seed=21)
    a, c = R.pop_counts(g, pop, n_pop)
    code = _lib.FST_WC84 if method == "W&C84" else _lib.FST_WH02
    f, per, beta = _lib.fst(pack_2bit_rows(g), n, pop, n_pop, code)
    want = R.snpgds_fst(g, pop, n_pop, method)
    _within(f, want["Fst"], want["Fst_bound"], "Fst")
    _within(per, want["FstSNP"], want["FstSNP_bound"], "FstSNP")
    if method == "W&H02":
        _within(beta, want["Beta"], want["Beta_bound"], "Beta")
        assert np.array_equal(beta, beta.T)
    sets = [np.arange(0, 50), np.arange(40, 41), np.array([], np.int64), np.arange(7, 211, 7), np.arange(100, 211)]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    fw, per_w, beta_w = _lib.fst_windows(pack_2bit_rows(g), n, pop, n_pop, offsets, np.concatenate(sets), code)
    assert np.array_equal(per_w, per, equal_nan=True)
    for w, s in enumerate(sets):
        r = R.fst_set(a, c, method, s)
        _within(fw[w], r["Fst"], r["Fst_bound"], "window %d" % w)
        if method == "W&H02":
            _within(beta_w[w], r["Beta"], r["Beta_bound"], "window %d beta" % w)
    assert np.isnan(fw[2])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("remove_monosnp", [True, False])
def test_hapmap_fst_against_restatement(hapmap, method, remove_monosnp):
    group = hapmap.sample_annot["pop.group"]
    res = api.snpgdsFst(hapmap, group, method=method, remove_monosnp=remove_monosnp, with_id=True, verbose=False)
    levels = sorted(set(group))
    assert len(levels) == 4
    g = hapmap.read_genotype(np.isin(hapmap.snp_id, res["snp_id"]))
    pop = np.array([levels.index(x) for x in group], np.int32)
    want = R.snpgds_fst(g, pop, 4, method)
    _check_fst_result(res, want, method, levels)


@pytest.mark.parametrize("method", METHODS)
def test_hapmap_fst_sample_id_in_another_order(hapmap, method):
    group = hapmap.sample_annot["pop.group"]
    rng = np.random.default_rng(5)
    order = rng.permutation(hapmap.n_samp)[:200]
    sid = hapmap.sample_id[order]
    res = api.snpgdsFst(hapmap, group[order], method=method, sample_id=sid, with_id=True, verbose=False)
    samp_sel = np.isin(hapmap.sample_id, sid)
    assert np.array_equal(res["sample_id"], hapmap.sample_id[samp_sel])                  # working order = file order
    levels = sorted(set(group[order]))
    g = hapmap.read_genotype(np.isin(hapmap.snp_id, res["snp_id"]), samp_sel)
    pop = np.array([levels.index(x) for x in group[samp_sel]], np.int32)
    assert len(levels) == 4 and len(set(np.bincount(pop))) > 1           # all four populations, of different sizes
    want = R.snpgds_fst(g, pop, len(levels), method)
    _check_fst_result(res, want, method, levels)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("as_is", ["list", "numeric"])
@pytest.mark.parametrize("unit,winsize,shift", [("basepair", 5000000, 1000000), ("locus", 40, 15)])
@pytest.mark.parametrize("winstart", [None, 3])
def test_hapmap_sliding_window_fst(hapmap, method, as_is, unit, winsize, shift, winstart):
    group = hapmap.sample_annot["pop.group"]
    levels = sorted(set(group))
    pop = np.array([levels.index(x) for x in group], np.int32)
    res = api.snpgdsSlidingWindow(hapmap, FUN="snpgdsFst", winsize=winsize, shift=shift, unit=unit, winstart=winstart, as_is=as_is,
                                  verbose=False, population=group, method=method)
    in_ws = np.isin(hapmap.snp_id, res["snp_id"])
    flag = in_ws & (hapmap.snp_position > 0)
    chrset = R.chromosome_set(hapmap.snp_chromosome, flag)
    assert [k[:-4] for k in res if k.endswith(".val")] == ["chr%s" % c for c in chrset] and len(chrset) >= 2
    rng = np.random.default_rng(11)
    direct, direct_chr = 0, chrset[:20]                     # one window of each of up to 20 chromosomes against snpgdsFst
    for ch in chrset:
        chflag = flag & (hapmap.snp_chromosome == ch)
        chpos = hapmap.snp_position[chflag]
        members, num, pos, posrange = R.sliding_windows(chpos, winsize, shift, unit, winstart)
        key = "chr%s" % ch
        assert np.array_equal(res[key + ".num"], num) and tuple(res[key + ".posrange"]) == posrange
        assert np.array_equal(res[key + ".pos"], pos, equal_nan=True)
        a, c = R.pop_counts(hapmap.read_genotype(chflag), pop, 4)
        val = res[key + ".val"]
        assert len(val) == len(members)
        for w, m in enumerate(members):
            if len(m) == 0:
                assert (val[w] is None) if as_is == "list" else np.isnan(val[w])
                continue
            r = R.fst_set(a, c, method, m)
            got = val[w][0] if as_is == "list" else val[w]
            _within(got, r["Fst"], r["Fst_bound"], "%s window %d" % (key, w))
            if as_is == "list":
                per, bound = R.fst_snp(a[m], c[m], method)
                _within(val[w][1], per, bound, "%s window %d FstSNP" % (key, w))
                assert len(val[w]) == (3 if method == "W&H02" else 2)
                if method == "W&H02":
                    _within(val[w][2], r["Beta"], r["Beta_bound"], "%s window %d Beta" % (key, w))
        # the property the one-pass design must preserve: a window equals snpgdsFst on its SNPs
        # (same counters, same per-SNP terms, the same sequential sum: EQUAL, bit for bit)
        filled = [w for w, m in enumerate(members) if len(m)]
        if ch not in direct_chr or not filled:
            continue
        w = int(rng.choice(filled))
        ids = hapmap.snp_id[chflag][members[w]]
        one = api.snpgdsFst(hapmap, group, method=method, snp_id=ids, autosome_only=False, remove_monosnp=False,
                            missing_rate=float("nan"), with_id=True, verbose=False)
        assert np.array_equal(one["snp_id"], ids)
        got = val[w][0] if as_is == "list" else val[w]
        assert np.array_equal(got, one["Fst"], equal_nan=True), (key, w, got, one["Fst"])
        if as_is == "list":
            assert np.array_equal(val[w][1], one["FstSNP"], equal_nan=True), (key, w)
            if method == "W&H02":
                assert np.array_equal(val[w][2], one["Beta"], equal_nan=True), (key, w)
        direct += 1
    assert 10 <= direct <= 20


@pytest.mark.parametrize("as_is", ["list", "numeric", "array"])
def test_hapmap_sliding_window_rate_freq(hapmap, as_is):
    res = api.snpgdsSlidingWindow(hapmap, FUN="snpgdsSNPRateFreq", winsize=8000000, shift=2000000, as_is=as_is, verbose=False)
    flag = np.isin(hapmap.snp_id, res["snp_id"]) & (hapmap.snp_position > 0)
    for ch in R.chromosome_set(hapmap.snp_chromosome, flag):
        chflag = flag & (hapmap.snp_chromosome == ch)
        members, num, pos, posrange = R.sliding_windows(hapmap.snp_position[chflag], 8000000, 2000000)
        g = hapmap.read_genotype(chflag)
        called = (g <= 2).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            af = np.where(g <= 2, g, 0).sum(1) / (2.0 * called)
        mf = np.minimum(af, 1 - af)
        mr = 1 - called / float(g.shape[1])
        key = "chr%s" % ch
        val = res[key + ".val"]
        assert np.array_equal(res[key + ".num"], num) and np.array_equal(res[key + ".pos"], pos, equal_nan=True)
        assert tuple(res[key + ".posrange"]) == posrange and len(val if as_is != "array" else val.T) == len(members)
        for w, m in enumerate(members):
            if as_is == "list":
                if len(m) == 0:
                    assert val[w] is None
                else:
                    assert all(np.array_equal(x, y[m], equal_nan=True) for x, y in zip(val[w], (af, mf, mr)))
            elif as_is == "numeric":
                assert np.array_equal(val[w], R.get_mean(mf[m]) if len(m) else np.nan, equal_nan=True)
            else:
                want = [R.get_mean(x[m]) if len(m) else np.nan for x in (af, mf, mr)]
                assert val.shape == (3, len(members)) and np.array_equal(val[:, w], want, equal_nan=True)


def test_hapmap_sliding_window_fst_array_refused(hapmap):
    with pytest.raises(NotImplementedError):
        api.snpgdsSlidingWindow(hapmap, FUN="snpgdsFst", as_is="array", verbose=False, population=hapmap.sample_annot["pop.group"])


def test_scale_synthetic_three_populations(monkeypatch):
    """N = 20 000 x M = 40 000 from the device generator (spectrum 3: sample % 3 with Fst ~ 0.1), 1 % missing, streamed in blocks of
    16 384 SNPs.  The two thresholds are conditions on the generator (a direct W&C84 loop on its CPU twin at N = 3 000 x M = 4 000,
    seed 99: 0.0921 with sample % 3, 3.6e-5 with the labels permuted), not measurements."""
    import torch
    N, M, seed, block = 20000, 40000, 99, 16384
    rb = (N + 3) // 4
    geno = torch.empty(M * rb, dtype=torch.uint8, device="cuda")
    _lib.synth_block(geno.data_ptr(), N, 0, M, seed=seed, missing=0.01, spectrum=3)
    torch.cuda.synchronize()
    monkeypatch.setenv("SNPGPU_POP_BLOCK_SNPS", str(block))
    pop = (np.arange(N) % 3).astype(np.int32)
    a, c = _lib.pop_counts(int(geno.data_ptr()), N, pop, 3, fmt=_lib.GENO_PACKED2, n_snp=M)
    assert _lib.pop_stats()[1] == 3
    edges = [0, block - 1, block, 2 * block - 1, 2 * block, M - 1]
    snps = np.unique(np.concatenate([edges, np.random.default_rng(1).choice(M, 494, replace=False)]))
    for s in snps:
        g = synth_hash_geno(np.arange(N), int(s), 1, seed, missing=0.01, spectrum=3)
        wa, wc = R.pop_counts(g, pop, 3)
        assert np.array_equal(a[s], wa[0]) and np.array_equal(c[s], wc[0]), s
    f, per, _ = _lib.fst(int(geno.data_ptr()), N, pop, 3, _lib.FST_WC84, fmt=_lib.GENO_PACKED2, n_snp=M)
    want = R.fst_set(a, c, "W&C84")
    _within(f, want["Fst"], want["Fst_bound"], "Fst at scale")
    assert f > 0.05
    perm = np.random.default_rng(2).permutation(pop).astype(np.int32)
    f2, _, _ = _lib.fst(int(geno.data_ptr()), N, perm, 3, _lib.FST_WC84, fmt=_lib.GENO_PACKED2, n_snp=M)
    assert abs(f2) < 0.01
