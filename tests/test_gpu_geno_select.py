"""GPU tests of the genotype selection (snpgpu_geno_select, GenoStream.select_blocks, snpgdsGetGeno and the sample selection of
_init_file2).  Everything is asserted EQUAL, byte for byte, to the numpy restatement (tests/geno_select_ref.py): these are integer
moves, there is no tolerance."""
import os

import numpy as np
import pytest

import geno_select_ref as R
from conftest import GOLDEN
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoFile, GenoStream, open_gds_stream, pack_2bit_rows

pytestmark = pytest.mark.gpu


def _select(data, kw, samp=None, snp=None, **more):
    return _lib.geno_select(data, kw["major"], kw["n_rows"], kw["n_cols"], bit0=kw["bit0"], row_stride_bits=kw.get("row_stride_bits"),
                            row_bit=kw.get("row_bit"), samp_index=samp, snp_index=snp, **more)


def _check(data, kw, samp=None, snp=None, tag=None, **more):
    got = _select(data, kw, samp, snp, **more)
    want = R.ref_of(data, kw, samp, snp)
    assert got.shape == want.shape and np.array_equal(got, want), tag
    return got


@pytest.mark.parametrize("n", R.SAMPLES)
def test_every_shape_layout_and_phase(n):
    """source samples x source SNPs x the three raw layouts, bit0 cycling through 0, 2, 4, 6 (odd products put the rows of the
    continuous streams at phases 2, 4 and 6 anyway), 0 / 5 / 30 % missing, all samples and two lists per case"""
    for i, L in enumerate(R.SNPS):
        g = R.codes(L, n, R.MISSING[(i + n) % 3], seed=100 * n + L)
        lists = R.sample_lists(n)
        names = sorted(lists)
        for j, layout in enumerate(R.LAYOUTS):
            data, kw = R.make_stream(g, layout, bit0=2 * ((i + j) % 4), seed=i + j)
            for name in ("all", "random", names[(3 * i + j) % len(names)]):
                _check(data, kw, lists[name], tag=(n, L, layout, name))


@pytest.mark.parametrize("shape", [(279, 257), (2049, 65), (130, 1000), (65, 64)])
@pytest.mark.parametrize("layout", R.LAYOUTS + ("row_bit0", "row_bit1"))
def test_every_sample_list(shape, layout):
    n, L = shape
    g = R.codes(L, n, 0.05, seed=n + L)
    data, kw = R.make_stream(g, layout, bit0=2, seed=5)
    lists = R.sample_lists(n)
    sizes = {n if v is None else len(v) for v in lists.values()}
    if n >= 279:
        assert {s % 4 for s in sizes} == {0, 1, 2, 3} and {0, 1, 63} <= {s % 64 for s in sizes}
    for name, sel in lists.items():
        got = _check(data, kw, sel, tag=(shape, layout, name))
        n_out = n if sel is None else len(sel)
        if n_out % 4:                                                   # the padding codes are 3
            assert ((got[:, -1] >> (2 * (n_out % 4))) == (0xFF >> (2 * (n_out % 4)))).all(), name


@pytest.mark.parametrize("shape", [(279, 257), (65, 1000), (2049, 130)])
@pytest.mark.parametrize("layout", R.LAYOUTS + ("row_bit0", "row_bit1"))
def test_every_snp_list(shape, layout):
    n, L = shape
    g = R.codes(L, n, 0.30, seed=n * L)
    data, kw = R.make_stream(g, layout, bit0=6, seed=7)
    lists = R.sample_lists(n)
    for sname in ("all", "random", "run1+64", "second"):
        for name, snp in R.snp_lists(L).items():
            _check(data, kw, lists[sname], snp, tag=(shape, layout, sname, name))


def _device_copy(block, offset):
    import torch
    buf = torch.full((block.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    buf[offset:offset + block.size] = torch.from_numpy(np.ascontiguousarray(block).reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 256 == 0
    return buf, int(buf.data_ptr()) + offset


@pytest.mark.parametrize("layout", R.LAYOUTS + ("row_bit0", "row_bit1"))
def test_sources_in_host_pinned_and_device_memory(layout):
    """device sources at byte offsets 0 .. 3 inside a 0x5A-filled buffer, bit0 in {0, 2, 4, 6}"""
    n, L = 279, 130
    g = R.codes(L, n, 0.05, seed=3)
    lists = R.sample_lists(n)
    snps = R.snp_lists(L)
    for bit0 in (0, 2, 4, 6):
        data, kw = R.make_stream(g, layout, bit0=bit0, seed=bit0)
        cases = [(None, None), (lists["random"], snps["scattered"]), (lists["run3+64"], snps["window"]), (lists["one"], snps["descending"])]
        want = [R.ref_of(data, kw, a, b) for a, b in cases]
        pb = _lib.PinnedBuffer((data.size,))
        try:
            pb.array[:] = data
            for (a, b), w in zip(cases, want):
                got = _lib.geno_select(pb.ptr, kw["major"], kw["n_rows"], kw["n_cols"], bit0=bit0, row_stride_bits=kw.get("row_stride_bits"),
                                       row_bit=kw.get("row_bit"), samp_index=a, snp_index=b, n_bytes=data.size, mem=_lib.HOST_PINNED)
                assert np.array_equal(got, w), (layout, bit0, "pinned")
        finally:
            pb.free()
        for off in range(4):
            keep, ptr = _device_copy(data, off)
            for (a, b), w in zip(cases, want):
                got = _lib.geno_select(ptr, kw["major"], kw["n_rows"], kw["n_cols"], bit0=bit0, row_stride_bits=kw.get("row_stride_bits"),
                                       row_bit=kw.get("row_bit"), samp_index=a, snp_index=b, n_bytes=data.size)
                assert np.array_equal(got, w), (layout, bit0, off)
            del keep


@pytest.mark.parametrize("layout", R.LAYOUTS + ("row_bit0", "row_bit1"))
def test_host_source_through_several_staging_windows(layout, monkeypatch):
    n, L = 279, 257
    g = R.codes(L, n, 0.05, seed=9)
    data, kw = R.make_stream(g, layout, bit0=4, seed=1)
    lists, snps = R.sample_lists(n), R.snp_lists(L)
    for stage in (4096, 1500, 100):
        monkeypatch.setenv("SNPGPU_SELECT_STAGE_BYTES", str(stage))
        for sname, kname in (("all", "all"), ("random", "all"), ("run2+65", "window"), ("second", "scattered"), ("all", "descending")):
            _check(data, kw, lists[sname], snps[kname], tag=(layout, stage, sname, kname))
            st = _lib.geno_select_stats()
            # (a short sample list can fit one window of a larger staging size; all samples, or 100 bytes, never do)
            assert st["source_bytes"] > 0 and st["windows"] >= 1, (layout, stage, sname, kname, st)
            if stage == 100 or sname == "all":
                assert st["windows"] > 1, (layout, stage, sname, kname, st)
    monkeypatch.delenv("SNPGPU_SELECT_STAGE_BYTES")
    _check(data, kw, lists["random"], None)
    assert _lib.geno_select_stats()["windows"] == 1


def test_gather_with_rows_in_global_memory_and_small_lds(monkeypatch):
    """the LDS budget of the gather kernel decides the rows per workgroup and whether the source rows stay in global memory"""
    n, L = 2049, 65
    g = R.codes(L, n, 0.05, seed=4)
    lists = R.sample_lists(n)
    for layout in ("packed", "sample.order", "row_bit0"):
        data, kw = R.make_stream(g, layout, bit0=2, seed=2)
        for words in (0, 130, 300, 1000):                     # none; 1, 2 and 7 rows of 130 dwords
            monkeypatch.setenv("SNPGPU_SELECT_LDS_WORDS", str(words))
            for name in ("random", "reversed", "perm129"):
                _check(data, kw, lists[name], R.snp_lists(L)["scattered"], tag=(layout, words, name))
                assert _lib.geno_select_stats()["gather_ms"] > 0


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_destination_in_a_larger_buffer(layout):
    """dst in device and in host memory inside a 0xA5-filled buffer, at every byte alignment: the bytes before and after the
    result are unchanged"""
    import torch
    n, L = 130, 65
    g = R.codes(L, n, 0.05, seed=6)
    data, kw = R.make_stream(g, layout, bit0=2, seed=3)
    lists = R.sample_lists(n)
    for name in ("all", "random", "run1+64", "perm67", "one", "run3+126"):
        sel = lists[name]
        want = R.ref_of(data, kw, sel)
        for off in range(4):
            host = np.full(want.size + 64, 0xA5, np.uint8)
            _select(data, kw, sel, out=host[16 + off:16 + off + want.size])
            assert np.array_equal(host[16 + off:16 + off + want.size].reshape(want.shape), want), (name, off)
            assert (host[:16 + off] == 0xA5).all() and (host[16 + off + want.size:] == 0xA5).all(), (name, off)
            dev = torch.full((want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _select(data, kw, sel, out=int(dev.data_ptr()) + 16 + off)
            h = dev.cpu().numpy()
            assert np.array_equal(h[16 + off:16 + off + want.size].reshape(want.shape), want), (name, off, "device")
            assert (h[:16 + off] == 0xA5).all() and (h[16 + off + want.size:] == 0xA5).all(), (name, off, "device")


# ---- the reader ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_cases(hapmap):
    """selections of the HapMap fixture and their rows, computed once: the restatement applied to the packed rows"""
    n, L = hapmap.n_samp, hapmap.n_snp
    rng = np.random.default_rng(8)
    sels = {"all": None, "shuffled100": rng.permutation(n)[:100].astype(np.int32), "first200": np.arange(200, dtype=np.int32),
            "repeats": rng.integers(0, n, n + 5).astype(np.int32)}
    rb = (n + 3) // 4
    want = {k: R.select_ref(hapmap.packed, 0, L, n, stride=8 * rb, samp_index=v) for k, v in sels.items()}
    return sels, want


def _read_all(gs, block, sel, to, **kw):
    rows = []
    for lo, m, r in gs.select_blocks(block, samp_index=sel, to=to, **kw):
        assert r.shape[0] == m
        rows.append(r.cpu().numpy() if to == "device" else r)
    return np.concatenate(rows, 0)


def _transposed_stream(hapmap, tmp_path):
    """the fixture in the layout it does NOT have, as a raw file with a GenoStream built on it directly"""
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    g = hapmap.read_genotype()
    layout = "snp.order" if gs.sample_order else "sample.order"
    data, _ = R.make_stream(g, layout, bit0=0)
    fn = tmp_path / "other_layout.bin"
    fn.write_bytes(data.tobytes())
    dims = [hapmap.n_samp, hapmap.n_snp] if gs.sample_order else [hapmap.n_snp, hapmap.n_samp]
    other = GenoStream(str(fn), hapmap.sample_id, hapmap.snp_id, hapmap.snp_chromosome, dims, [(0, data.size)], data.size, False,
                       not gs.sample_order)
    return gs, other


@pytest.mark.parametrize("to", ["device", "host"])
def test_select_blocks_on_the_fixture_in_both_layouts(hapmap, fixture_cases, tmp_path, to):
    sels, want = fixture_cases
    L = hapmap.n_snp
    for gs in _transposed_stream(hapmap, tmp_path):
        for name, block in (("shuffled100", 1000), ("all", 4096), ("repeats", L + 50), ("first200", 4096), ("shuffled100", 3333)):
            got = _read_all(gs, block, sels[name], to)
            assert np.array_equal(got, want[name]), (gs.sample_order, name, block)
        # one SNP per block, over a window off every multiple
        got = _read_all(gs, 1, sels["shuffled100"], to, snp_begin=1001, snp_end=1031)
        assert np.array_equal(got, want["shuffled100"][1001:1031]), gs.sample_order
        got = _read_all(gs, 7, None, to, snp_begin=L - 20)
        assert np.array_equal(got, want["all"][L - 20:]), gs.sample_order


def test_device_blocks_alternate_between_two_buffers(hapmap, fixture_cases):
    sels, want = fixture_cases
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    it = gs.select_blocks(500, samp_index=sels["shuffled100"], to="device", snp_end=1500)
    lo0, m0, r0 = next(it)
    lo1, m1, r1 = next(it)
    assert r0.data_ptr() != r1.data_ptr()
    assert np.array_equal(r0.cpu().numpy(), want["shuffled100"][lo0:lo0 + m0])          # still valid after the next next()
    lo2, m2, r2 = next(it)
    assert r2.data_ptr() == r0.data_ptr()
    assert np.array_equal(r1.cpu().numpy(), want["shuffled100"][lo1:lo1 + m1])
    assert np.array_equal(r2.cpu().numpy(), want["shuffled100"][lo2:lo2 + m2])


# ---- the public interface ----------------------------------------------------------------------------------------------------------
def test_getgeno_against_read_genotype(hapmap, capsys):
    rng = np.random.default_rng(12)
    samp = rng.permutation(hapmap.n_samp)[:77]
    snps = rng.permutation(hapmap.n_snp)[:501]
    want = hapmap.read_genotype(np.sort(snps), np.sort(samp))                             # [snp][sample], file order
    got = api.snpgdsGetGeno(hapmap, sample_id=hapmap.sample_id[samp], snp_id=hapmap.snp_id[snps], snpfirstdim=True, verbose=True)
    assert "Genotype matrix: 501 SNPs X 77 samples" in capsys.readouterr().out
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    got = api.snpgdsGetGeno(hapmap, sample_id=hapmap.sample_id[samp], snp_id=hapmap.snp_id[snps], snpfirstdim=False, verbose=True)
    assert "Genotype matrix: 77 samples X 501 SNPs" in capsys.readouterr().out
    assert np.array_equal(got, want.T)
    path = os.path.join(GOLDEN, "hapmap_geno.gds")
    rv = api.snpgdsGetGeno(path, sample_id=hapmap.sample_id[samp], snpfirstdim=None, with_id=True, verbose=False)
    full = hapmap.read_genotype(None, np.sort(samp))
    assert np.array_equal(rv["genotype"], full.T if hapmap.sample_order else full)
    assert np.array_equal(rv["sample_id"], hapmap.sample_id[np.sort(samp)]) and np.array_equal(rv["snp_id"], hapmap.snp_id)
    assert capsys.readouterr().out == ""
    # no selection at all, and a stream object
    assert np.array_equal(api.snpgdsGetGeno(hapmap, snpfirstdim=True, verbose=False), hapmap.read_genotype())
    gs = open_gds_stream(path)
    got = api.snpgdsGetGeno(gs, sample_id=hapmap.sample_id[samp], snp_id=hapmap.snp_id[snps], snpfirstdim=True, verbose=False)
    assert np.array_equal(got, want)


def test_sample_id_selection_of_the_analysis_functions(hapmap):
    """snpgdsIBSNum and snpgdsSampMissRate with sample_id= of 100 shuffled samples (now selected on the device) equal the same
    calls on a GenoFile built from the host-selected matrix, bit for bit"""
    rng = np.random.default_rng(21)
    pick = rng.permutation(hapmap.n_samp)[:100]
    keep = np.sort(pick)
    sub = GenoFile(genotype=hapmap.read_genotype(None, keep), sample_id=hapmap.sample_id[keep], snp_id=hapmap.snp_id,
                   snp_chromosome=hapmap.snp_chromosome)
    a = api.snpgdsIBSNum(hapmap, sample_id=hapmap.sample_id[pick], verbose=False)
    b = api.snpgdsIBSNum(sub, verbose=False)
    assert np.array_equal(a["sample_id"], b["sample_id"]) and np.array_equal(a["snp_id"], b["snp_id"])
    for k in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(a[k], b[k]), k
    a = api.snpgdsSampMissRate(hapmap, sample_id=hapmap.sample_id[pick])
    b = api.snpgdsSampMissRate(sub)
    assert np.array_equal(a, b)


def test_streaming_accumulator_fed_from_select_blocks(hapmap):
    rng = np.random.default_rng(22)
    sel = rng.permutation(hapmap.n_samp)[:150].astype(np.int32)
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    host_rows = pack_2bit_rows(hapmap.read_genotype(None, sel))
    with _lib.Accumulator(_lib.IBS, len(sel), max_block_snps=2048) as acc:
        for lo in range(0, hapmap.n_snp, 2048):
            acc.feed(host_rows[lo:lo + 2048], _lib.GENO_PACKED2)
        want = acc.ibs_num(packed=True)
    with _lib.Accumulator(_lib.IBS, len(sel), max_block_snps=2048) as acc:
        for lo, m, rows in gs.select_blocks(2048, samp_index=sel, to="device"):
            acc.feed_device(rows.data_ptr(), m, _lib.GENO_PACKED2)
        got = acc.ibs_num(packed=True)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
