"""GPU tests of the PLINK BED path (snpgpu_geno_convert, BedStream.select_blocks, snpgdsOpenBED, snpgdsGDS2BED).  Everything is
asserted EQUAL, byte for byte, to the numpy restatement (tests/bed_ref.py): these are integer moves, there is no tolerance."""
import gzip
import os

import numpy as np
import pytest

import bed_ref as B
import geno_select_ref as R
from conftest import GOLDEN
from snprelate_amd import _lib, api, bed
from snprelate_amd.gds import GenoFile, open_gds_stream

pytestmark = pytest.mark.gpu

FIX = [os.path.join(GOLDEN, "plinkhapmap.%s.gz" % e) for e in ("bed", "fam", "bim")]
# (src_code, dst_code, dst_major)
COMBOS = [(s, d, m) for s in (B.GDS, B.BED) for d in (B.GDS, B.BED) for m in (0, 1)]


def _convert(data, kw, combo, samp=None, snp=None, **more):
    sc, dc, dm = combo
    return _lib.geno_convert(data, kw["major"], kw["n_rows"], kw["n_cols"], src_code=sc, dst_code=dc, dst_major=dm, bit0=kw["bit0"],
                             row_stride_bits=kw.get("row_stride_bits"), row_bit=kw.get("row_bit"), samp_index=samp, snp_index=snp, **more)


def _check(data, kw, combo, samp=None, snp=None, codes=None, tag=None, **more):
    sc, dc, dm = combo
    got = _convert(data, kw, combo, samp, snp, **more)
    want = B.convert_ref(data, kw, sc, dc, dm, samp, snp, codes=codes)
    assert got.shape == want.shape and np.array_equal(got, want), (combo, tag)
    n_samp_out = (kw["n_rows"] if kw["major"] else kw["n_cols"]) if samp is None else len(samp)
    n_snp_out = (kw["n_cols"] if kw["major"] else kw["n_rows"]) if snp is None else len(snp)
    assert B.padding_ok(got, n_snp_out if dm else n_samp_out, dc), (combo, tag)
    return got


@pytest.mark.parametrize("n", B.SAMPLES)
def test_every_code_pair_layout_shape_and_phase(n):
    """source samples x source SNPs x the three raw layouts x the four code pairs x both layouts of dst, bit0 cycling through
    0, 2, 4, 6, 0 / 5 / 30 % missing; the sample list cycles through all / random / a run, the SNP list through snp_lists.  The
    bits of a stream outside its elements are random, so a source's padding that is read as a genotype shows."""
    lists = R.sample_lists(n)
    runs = sorted(k for k in lists if k.startswith("run"))
    for i, L in enumerate(B.SNPS):
        g = R.codes(L, n, B.MISSING[(i + n) % 3], seed=100 * n + L)
        snps = R.snp_lists(L)
        knames = sorted(snps)
        for j, layout in enumerate(B.LAYOUTS):
            data, kw = R.make_stream(g, layout, bit0=2 * ((i + j) % 4), seed=i + j)
            codes = B.source_codes(data, kw)
            for c, combo in enumerate(COMBOS):
                sname = ("all", "random", runs[(i + j + c) % len(runs)])[(i + j + c // 2) % 3]
                kname = knames[(i + 2 * j + c) % len(knames)]
                _check(data, kw, combo, lists[sname], snps[kname], codes, tag=(n, L, layout, sname, kname))


@pytest.mark.parametrize("shape", [(279, 257), (65, 1000), (5, 3)])
def test_padding_of_both_code_sets_on_both_axes(shape):
    """sizes that leave 1, 2 and 3 unused codes on the packed axis, through the copy, the gather and the transposition: zero
    bits for a dst of BED code, all ones for GDS, along the samples for dst_major 0 and along the SNPs for dst_major 1"""
    n, L = shape
    g = R.codes(L, n, 0.05, seed=n + L)
    samps, snps = R.sample_lists(n), R.snp_lists(L)
    samp_sel = [None, samps["random"]] + [samps[k] for k in ("run2+65", "perm66") if k in samps]
    snp_sel = [None, snps["descending"]] + [snps[k] for k in ("window", "window1", "scattered") if k in snps]
    seen = set()
    for layout in B.LAYOUTS:
        data, kw = R.make_stream(g, layout, bit0=2, seed=5)
        codes = B.source_codes(data, kw)
        for combo in COMBOS:
            for a in samp_sel:
                for b in (snp_sel if combo[2] else snp_sel[:2]):
                    got = _check(data, kw, combo, a, b, codes, tag=(shape, layout))
                    packed = (L if b is None else len(b)) if combo[2] else (n if a is None else len(a))
                    seen.add(packed % 4)
                    if packed % 4:
                        tail = got[:, -1] >> (2 * (packed % 4))
                        assert (tail == (0 if combo[1] == B.BED else 0xFF >> (2 * (packed % 4)))).all(), (combo, layout)
    assert seen >= {1, 2, 3}


def test_identity_call_equals_geno_select():
    n, L = 279, 257
    g = R.codes(L, n, 0.05, seed=7)
    lists, snps = R.sample_lists(n), R.snp_lists(L)
    for layout in B.LAYOUTS + ("row_bit0", "row_bit1"):
        data, kw = R.make_stream(g, layout, bit0=4, seed=2)
        for sname, kname in (("all", "all"), ("random", "scattered"), ("run3+64", "window"), ("second", "descending")):
            a = _convert(data, kw, (B.GDS, B.GDS, 0), lists[sname], snps[kname])
            b = _lib.geno_select(data, kw["major"], kw["n_rows"], kw["n_cols"], bit0=kw["bit0"], row_stride_bits=kw.get("row_stride_bits"),
                                 row_bit=kw.get("row_bit"), samp_index=lists[sname], snp_index=snps[kname])
            assert np.array_equal(a, b) and np.array_equal(a, R.ref_of(data, kw, lists[sname], snps[kname])), (layout, sname, kname)
            assert _lib.geno_convert_stats() == _lib.geno_select_stats()


@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_destination_in_a_larger_buffer(layout):
    """dst in device and in host memory inside a 0xA5-filled buffer, at every byte alignment: the bytes before and after the
    result are unchanged, for every code pair and both layouts of dst"""
    import torch
    n, L = 130, 65
    g = R.codes(L, n, 0.05, seed=6)
    data, kw = R.make_stream(g, layout, bit0=2, seed=3)
    codes = B.source_codes(data, kw)
    lists, snps = R.sample_lists(n), R.snp_lists(L)
    names = ("all", "random", "run1+64", "perm67", "one", "run3+126")
    for c, combo in enumerate(COMBOS):
        for t in range(2):
            sel, ksel = lists[names[(c + 3 * t) % len(names)]], (None, snps["scattered"], snps["window1"])[(c + t) % 3]
            want = B.convert_ref(data, kw, combo[0], combo[1], combo[2], sel, ksel, codes=codes)
            for off in range(4):
                host = np.full(want.size + 64, 0xA5, np.uint8)
                _convert(data, kw, combo, sel, ksel, out=host[16 + off:16 + off + want.size])
                assert np.array_equal(host[16 + off:16 + off + want.size].reshape(want.shape), want), (combo, t, off)
                assert (host[:16 + off] == 0xA5).all() and (host[16 + off + want.size:] == 0xA5).all(), (combo, t, off)
                dev = torch.full((want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                _convert(data, kw, combo, sel, ksel, out=int(dev.data_ptr()) + 16 + off)
                h = dev.cpu().numpy()
                assert np.array_equal(h[16 + off:16 + off + want.size].reshape(want.shape), want), (combo, t, off, "device")
                assert (h[:16 + off] == 0xA5).all() and (h[16 + off + want.size:] == 0xA5).all(), (combo, t, off, "device")


def test_gather_with_rows_in_global_memory_and_small_lds(monkeypatch):
    """the gather runs when the source's major equals dst_major and the packed axis has a list: a sample list over SNP rows for
    dst_major 0, a SNP list over sample rows for dst_major 1 -- with the LDS budget forced to none, 1, 2 and 7 rows"""
    n, L = 2049, 65
    g = R.codes(L, n, 0.05, seed=4)
    lists = R.sample_lists(n)
    cases = []
    for layout in ("packed", "sample.order", "row_bit0"):
        data, kw = R.make_stream(g, layout, bit0=2, seed=2)
        cases.append((data, kw, 0, [(lists[k], R.snp_lists(L)["scattered"]) for k in ("random", "reversed", "perm129")]))
    gt = np.ascontiguousarray(g.T)                                      # 2049 SNPs x 65 samples, as sample rows
    for layout in ("snp.order", "row_bit1"):
        data, kw = R.make_stream(gt, layout, bit0=2, seed=2)
        cases.append((data, kw, 1, [(R.sample_lists(65)["second"], lists[k]) for k in ("random", "reversed", "perm129")]))
    for data, kw, dm, sels in cases:
        codes = B.source_codes(data, kw)
        for words in (0, 130, 300, 1000):
            monkeypatch.setenv("SNPGPU_SELECT_LDS_WORDS", str(words))
            for c, (a, b) in enumerate(sels):
                for sc, dc in ((B.BED, B.GDS), (B.GDS, B.BED), ((B.GDS, B.GDS), (B.BED, B.BED))[c % 2]):
                    _check(data, kw, (sc, dc, dm), a, b, codes, tag=(dm, words, c))
                    assert _lib.geno_convert_stats()["gather_ms"] > 0


@pytest.mark.parametrize("layout", B.LAYOUTS + ("row_bit0", "row_bit1"))
def test_host_source_through_several_staging_windows(layout, monkeypatch):
    n, L = 279, 257
    g = R.codes(L, n, 0.05, seed=9)
    data, kw = R.make_stream(g, layout, bit0=4, seed=1)
    codes = B.source_codes(data, kw)
    lists, snps = R.sample_lists(n), R.snp_lists(L)
    for stage in (1500, 100):
        monkeypatch.setenv("SNPGPU_SELECT_STAGE_BYTES", str(stage))
        for c, combo in enumerate(COMBOS):
            for sname, kname in (("all", "all"), (("random", "run2+65")[c % 2], ("scattered", "descending", "window")[c % 3])):
                _check(data, kw, combo, lists[sname], snps[kname], codes, tag=(layout, stage, sname, kname))
                st = _lib.geno_convert_stats()
                assert st["source_bytes"] > 0 and st["windows"] >= 1, (layout, stage, combo, st)
                if sname == "all":                                  # data.size > stage: never one window
                    assert st["windows"] > 1, (layout, stage, combo, st)


# ---- the reader ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_codes():
    with gzip.open(FIX[0], "rb") as f:
        return B.bed_codes(f.read(), 1, 5000, 60)


def _read_all(bs, block, sel, to, **kw):
    rows = []
    for lo, m, r in bs.select_blocks(block, samp_index=sel, to=to, **kw):
        assert r.shape[0] == m
        rows.append(r.cpu().numpy() if to == "device" else r.copy())
    return np.concatenate(rows, 0)


@pytest.mark.parametrize("to", ["device", "host"])
def test_select_blocks_on_the_fixture_and_on_an_individual_major_file(fixture_codes, tmp_path, to):
    rng = np.random.default_rng(8)
    g0 = R.codes(1000, 65, 0.05, seed=10)
    fn = str(tmp_path / "m0")
    with open(fn + ".bed", "wb") as f:
        f.write(B.bed_file(g0, 0))
    with open(fn + ".fam", "w") as f:
        f.write("".join("0 s%d 0 0 0 -9\n" % i for i in range(65)))
    with open(fn + ".bim", "w") as f:
        f.write("".join("1\tr%d\t0\t%d\tA\tC\n" % (k, k + 1) for k in range(1000)))
    for bs, g in ((bed.BedStream(*FIX), fixture_codes), (bed.BedStream(fn + ".bed", fn + ".fam", fn + ".bim"), g0)):
        L, n = g.shape
        sels = {"all": None, "shuffled": rng.permutation(n)[:n // 2 + 1].astype(np.int32), "repeats": rng.integers(0, n, n + 5).astype(np.int32)}
        for name, block in (("all", 333), ("shuffled", 1000), ("repeats", L + 50), ("shuffled", 7 * 64 + 1)):
            sel = sels[name]
            want = R.pack_ref(g if sel is None else g[:, sel])
            assert np.array_equal(_read_all(bs, block, sel, to), want), (bs.mode, name, block)
        # equal to blocks(), the host path, over a window off every multiple and one SNP per block
        host = np.concatenate([r.copy() for _, _, r in bs.blocks(5, snp_begin=L - 21, snp_end=L - 1)], 0)
        assert np.array_equal(_read_all(bs, 1, None, to, snp_begin=L - 21, snp_end=L - 1), host), bs.mode
        assert np.array_equal(_read_all(bs, 4096, None, to), bs.packed), bs.mode


# ---- the public interface ----------------------------------------------------------------------------------------------------------
def test_analysis_functions_on_an_opened_bed(fixture_codes, monkeypatch):
    """snpgdsIBSNum and snpgdsSNPRateFreq of snpgdsOpenBED(fixture) equal those of a GenoFile built from the restatement's codes;
    sample_id= on the BedStream (selected on the device) equals the numpy fallback"""
    bs = api.snpgdsOpenBED(*FIX, verbose=False)
    gf = GenoFile(genotype=fixture_codes, sample_id=bs.sample_id, snp_id=bs.snp_id, snp_chromosome=bs.snp_chromosome)
    a, b = api.snpgdsIBSNum(bs, verbose=False), api.snpgdsIBSNum(gf, verbose=False)
    assert np.array_equal(a["sample_id"], b["sample_id"]) and np.array_equal(a["snp_id"], b["snp_id"]) and len(a["snp_id"]) > 4000
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(a[k], b[k]), k
    a, b = api.snpgdsSNPRateFreq(bs), api.snpgdsSNPRateFreq(gf)
    for k in ("AlleleFreq", "MinorFreq", "MissingRate"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    pick = bs.sample_id[np.random.default_rng(3).permutation(60)[:37]]
    fresh = api.snpgdsOpenBED(*FIX, verbose=False)                      # not yet in memory: the selection reads the file
    a = api.snpgdsIBSNum(fresh, sample_id=pick, verbose=False)
    assert getattr(fresh, "_packed", None) is None
    monkeypatch.setattr(api, "_device_visible", lambda: False)
    b = api.snpgdsIBSNum(api.snpgdsOpenBED(*FIX, verbose=False), sample_id=pick, verbose=False)
    assert np.array_equal(a["sample_id"], b["sample_id"]) and np.array_equal(a["snp_id"], b["snp_id"])
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(a[k], b[k]), k
    # chromosome labels kept as text: autosome_only keeps what parses into 1 ... 22
    monkeypatch.undo()
    ch = api.snpgdsOpenBED(*FIX, cvt_chr="char", verbose=False)
    assert ch.snp_chromosome.dtype.kind == "U"
    assert np.array_equal(api.snpgdsSelectSNP(ch, verbose=False), api.snpgdsSelectSNP(bs, verbose=False))


@pytest.mark.parametrize("snpfirstdim", [False, True])
def test_round_trip_of_the_hapmap_gds(hapmap, tmp_path, snpfirstdim):
    """279 samples (padding on the sample axis), 100 samples x 1 001 SNPs selected: .bed bytes equal the restatement's, and the
    opened copy reads the same genotypes; the same from a stream that is read block by block, and from a BedStream"""
    rng = np.random.default_rng(11)
    samp, snps = np.sort(rng.permutation(hapmap.n_samp)[:100]), np.sort(rng.permutation(hapmap.n_snp)[:1001])
    mode = 0 if snpfirstdim else 1
    out = str(tmp_path / "rt")
    api.snpgdsGDS2BED(hapmap, out, sample_id=hapmap.sample_id[samp], snp_id=hapmap.snp_id[snps], snpfirstdim=snpfirstdim, verbose=False)
    want = hapmap.read_genotype(snps, samp)
    with open(out + ".bed", "rb") as f:
        assert f.read() == B.bed_file(want, mode)
    back = api.snpgdsOpenBED(out + ".bed", verbose=False)
    assert back.mode == mode and np.array_equal(back.read_genotype(), want)
    assert np.array_equal(back.sample_id, hapmap.sample_id[samp]) and np.array_equal(back.snp_id, hapmap.snp_id[snps])
    # a stream, all SNPs: the rows select_blocks lays out on the device are recoded there
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    api.snpgdsGDS2BED(gs, out + "s", sample_id=hapmap.sample_id[samp], snpfirstdim=snpfirstdim, verbose=False)
    assert getattr(gs, "_packed", None) is None
    with open(out + "s.bed", "rb") as f:
        assert f.read() == B.bed_file(hapmap.read_genotype(None, samp), mode)
    # BED -> BED: the copy written above, a subset of it, in the other mode
    fresh = api.snpgdsOpenBED(out + ".bed", verbose=False)              # not in memory: read through select_blocks
    api.snpgdsGDS2BED(fresh, out + "b", sample_id=back.sample_id[3:70], snpfirstdim=not snpfirstdim, verbose=False)
    assert getattr(fresh, "_packed", None) is None
    with open(out + "b.bed", "rb") as f:
        assert f.read() == B.bed_file(want[:, 3:70], 1 - mode)
