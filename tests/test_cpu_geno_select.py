"""CPU tests of the genotype selection (snpgpu_geno_select, GenoStream.select_blocks, snpgdsGetGeno): the numpy restatement
(tests/geno_select_ref.py) against the existing host paths, the exports, and every argument refusal -- none needs a device."""
import ctypes
import os

import numpy as np
import pytest

import geno_select_ref as R
import snprelate_amd
from conftest import GOLDEN
from snprelate_amd import _lib, api
from snprelate_amd.gds import GenoStream, open_gds_stream, pack_2bit_rows, realign_bit2_rows, unpack_2bit_rows

NEW_SYMBOLS = ("snpgpu_geno_select", "snpgpu_geno_select_stats")


def test_exports():
    L = _lib.lib()
    assert L.snpgpu_abi_version() == 2
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s), s
    assert callable(_lib.geno_select) and callable(_lib.geno_select_stats)
    assert callable(GenoStream.select_blocks)
    assert snprelate_amd.snpgdsGetGeno is api.snpgdsGetGeno


@pytest.mark.parametrize("n", R.SAMPLES)
def test_restatement_equals_the_host_paths(n, tmp_path):
    """On the shapes of the GPU tests: the restatement of a packed-row source with a sample list is unpack -> [:, sel] -> pack,
    of the raw sample.order stream it is realign_bit2_rows (windows at any phase included), of the raw snp.order stream it is
    _blocks_snp_order."""
    for i, L in enumerate(R.SNPS):
        g = R.codes(L, n, R.MISSING[(i + n) % 3], seed=100 * n + L)
        lists = R.sample_lists(n)
        names = sorted(lists)
        for name in (names[i % len(names)], "random", "all"):
            sel = lists[name]
            data, kw = R.make_stream(g, "packed", bit0=0)
            want = pack_2bit_rows(unpack_2bit_rows(pack_2bit_rows(g), n)[:, sel] if sel is not None else g)
            assert np.array_equal(R.ref_of(data, kw, samp_index=sel), want), (L, name)
        data, kw = R.make_stream(g, "sample.order", bit0=0)
        assert np.array_equal(R.ref_of(data, kw), realign_bit2_rows(data.tobytes(), 0, n, 0, L))
        lo, hi = L // 3, L
        b0 = (2 * n * lo) >> 3
        win = dict(kw, n_rows=hi - lo, bit0=2 * n * lo - 8 * b0)
        assert np.array_equal(R.ref_of(data[b0:], win), realign_bit2_rows(data[b0:].tobytes(), 8 * b0, n, lo, hi))
        data, kw = R.make_stream(g, "snp.order", bit0=0)
        fn = tmp_path / ("snp_order_%d_%d.bin" % (n, L))
        fn.write_bytes(data.tobytes())
        gs = GenoStream(str(fn), np.arange(n), np.arange(L), np.ones(L, np.int32), [n, L], [(0, len(data))], len(data), False, False)
        got = np.concatenate([r.copy() for _, _, r in gs._blocks_snp_order(100, None, 0, L)], 0)
        assert np.array_equal(R.ref_of(data, kw), got), L
        # every layout and the row_bit forms describe the same matrix
        for layout in ("row_bit0", "row_bit1"):
            for bit0 in (0, 2, 4, 6):
                data, kw = R.make_stream(g, layout, bit0=bit0, seed=bit0)
                assert np.array_equal(R.ref_of(data, kw), pack_2bit_rows(g)), (layout, bit0)


def test_fixture_node_through_the_stream_reader(hapmap):
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    assert np.array_equal(gs.read_packed(4096), hapmap.packed)
    assert hapmap.sample_order == gs.sample_order
    # the node's own bytes, described as a source, are the same rows
    assert len(gs._extents) == 1 and not gs._zipped
    with open(gs.path, "rb") as f:
        f.seek(gs._extents[0][0])
        node = np.frombuffer(f.read(gs._extents[0][1]), np.uint8)
    if gs.sample_order:
        got = R.select_ref(node, 0, gs.n_snp, gs.n_samp)
    else:
        got = R.select_ref(node, 1, gs.n_samp, gs.n_snp)
    assert np.array_equal(got, hapmap.packed)


def _call(src, samp=None, n_samp_out=None, snp=None, n_snp_out=None, dst=True, dst_mem=_lib.HOST):
    L = _lib.lib()
    out = np.zeros(1 << 12, np.uint8)
    n_so = (src.n_rows if src.major else src.n_cols) if n_samp_out is None else n_samp_out
    n_ko = (src.n_cols if src.major else src.n_rows) if n_snp_out is None else n_snp_out
    rc = L.snpgpu_geno_select(ctypes.byref(src) if src is not None else None, _lib._ptr(samp), n_so, _lib._ptr(snp), n_ko,
                              _lib._ptr(out) if dst else None, dst_mem, 0, None)
    return rc, L.snpgpu_last_error().decode()


def test_argument_errors_are_refused_without_a_device():
    L = _lib.lib()
    bits = np.zeros(64, np.uint8)

    def src(**kw):
        d = dict(bits=bits.ctypes.data, mem=_lib.HOST, major=0, n_rows=4, n_cols=10, bit0=0, row_stride_bits=20, row_bit=None, n_bytes=64)
        d.update(kw)
        return _lib.GenoSrc(*[d[k] for k, _ in _lib.GenoSrc._fields_])

    out = np.zeros(64, np.uint8)
    rc = L.snpgpu_geno_select(None, None, 10, None, 4, _lib._ptr(out), _lib.HOST, 0, None)
    assert rc == 1 and "src is NULL" in L.snpgpu_last_error().decode()
    rb = np.array([0, 20, 41, 60], np.int64)
    cases = [
        (src(bits=None), {}, "bits is NULL"),
        (src(), dict(dst=False), "dst is NULL"),
        (src(bit0=1), {}, "odd or negative bit position: bit0"),
        (src(bit0=-2), {}, "odd or negative bit position: bit0"),
        (src(row_stride_bits=21), {}, "odd or negative bit position: row_stride_bits"),
        (src(row_bit=rb.ctypes.data), {}, r"odd or negative bit position: row_bit[2]"),
        (src(major=2), {}, "invalid major"),
        (src(), dict(samp=np.array([0, 10], np.int32), n_samp_out=2), "an index outside the source: samp_index[1]"),
        (src(), dict(samp=np.array([-1], np.int32), n_samp_out=1), "an index outside the source: samp_index[0]"),
        (src(), dict(snp=np.array([3, 4], np.int32), n_snp_out=2), "an index outside the source: snp_index[1]"),
        (src(major=1), dict(samp=np.array([4], np.int32), n_samp_out=1), "an index outside the source: samp_index[0]"),
        (src(n_bytes=9), {}, "an element outside n_bytes: row 3"),
        (src(bit0=440), {}, "an element outside n_bytes"),
        (src(row_bit=np.array([0, 20, 40, 500], np.int64).ctypes.data), {}, "an element outside n_bytes: row 3"),
        (src(n_bytes=0), {}, "invalid n_bytes"),
        (src(n_cols=1 << 30, row_stride_bits=0, n_rows=1), {}, "invalid number of samples"),
        (src(major=1, n_cols=1 << 31, n_rows=1, row_stride_bits=0), {}, "too many SNPs"),
        (src(n_rows=0), {}, "no SNP in the working dataset"),
        (src(), dict(n_samp_out=9), "samp_index is NULL"),
        (src(), dict(n_snp_out=3), "snp_index is NULL"),
        (src(mem=7), {}, "invalid memory kind"),
        (src(), dict(dst_mem=5), "invalid dst_mem"),
    ]
    for s, kw, msg in cases:
        rc, err = _call(s, **kw)
        assert rc == 1 and msg in err and err.startswith("snpgpu_geno_select: "), (msg, err)
        assert "HIP" not in err and "hip" not in err, err              # refused before any device is asked for
    assert L.snpgpu_geno_select_stats(None) == 1
    # the binding's own checks
    with pytest.raises(ValueError, match="needs n_bytes"):
        _lib.geno_select(12345, 0, 1, 4)
    with pytest.raises(ValueError, match="one bit position per source row"):
        _lib.geno_select(bits, 0, 4, 10, row_bit=[0, 20])
    with pytest.raises(ValueError, match="out should be"):
        _lib.geno_select(bits, 0, 4, 10, out=np.zeros(5, np.uint8))
    with pytest.raises(_lib.SnpGpuError, match="odd or negative"):
        _lib.geno_select(bits, 0, 4, 10, bit0=3)


def test_reader_and_getgeno_argument_checks(hapmap):
    gs = open_gds_stream(os.path.join(GOLDEN, "hapmap_geno.gds"))
    with pytest.raises(ValueError, match="'to' should be"):
        next(gs.select_blocks(100, to="disk"))
    with pytest.raises(ValueError, match="block_snps should be positive"):
        next(gs.select_blocks(0, to="host"))
    with pytest.raises(ValueError, match="samp_index should hold positions"):
        next(gs.select_blocks(100, samp_index=[0, gs.n_samp], to="host"))
    with pytest.raises(ValueError, match="samp_index should hold positions"):
        next(gs.select_blocks(100, samp_index=[], to="host"))
    with pytest.raises(TypeError, match="snpfirstdim"):
        api.snpgdsGetGeno(hapmap, snpfirstdim=1, verbose=False)
    with pytest.raises(TypeError, match="with.id"):
        api.snpgdsGetGeno(hapmap, with_id="yes", verbose=False)
    with pytest.raises(TypeError, match="verbose"):
        api.snpgdsGetGeno(hapmap, verbose=None)
    with pytest.raises(ValueError, match="Some of sample.id do not exist!"):
        api.snpgdsGetGeno(hapmap, sample_id=["nobody"], verbose=False)
    with pytest.raises(ValueError, match="Some of snp.id do not exist!"):
        api.snpgdsGetGeno(hapmap, snp_id=[-5], verbose=False)
    with pytest.raises(TypeError, match="SNP GDS object"):
        api.snpgdsGetGeno(12, verbose=False)


@pytest.mark.parametrize("w,rows", [(4096, 1000), (300, 2000), (100, 5000), (1, 3000)])
def test_gather_segments_touches_only_the_segments(w, rows, tmp_path):
    """The reader's gather of a snp.order node copies rows x w bytes and nothing that grows with the node: on a 256 MiB memory
    map (a sparse file with a few marked bytes) its temporaries stay below 2 MiB -- the index blocks are 2^17 int64 entries,
    1 MiB -- where a materialised window view of the node would take node length x w bytes."""
    import tracemalloc
    from snprelate_amd.gds import gather_segments
    size = 256 << 20
    fn = tmp_path / "node.bin"
    rng = np.random.default_rng(w)
    start = np.sort(rng.integers(0, size - w, rows)).astype(np.int64)
    start[-1] = size - w                                   # a segment that ends with the node
    with open(fn, "wb") as f:
        f.truncate(size)
        for a in start[::97]:
            f.seek(int(a))
            f.write(bytes([1 + int(a) % 251]) * w)
    mm = np.memmap(str(fn), dtype=np.uint8, mode="r", shape=(size,))
    out = np.full((rows, w), 0xEE, np.uint8)
    tracemalloc.start()
    gather_segments(mm, start, w, out)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < (2 << 20), peak
    for j in list(range(0, rows, 97)) + [rows - 1, 1, rows // 2]:
        assert np.array_equal(out[j], mm[start[j]:start[j] + w]), j
    # and the same bytes from an array in memory, every row
    a = rng.integers(0, 256, 1 << 16).astype(np.uint8)
    st = rng.integers(0, len(a) - w + 1, 500).astype(np.int64)
    got = gather_segments(a, st, w, np.empty((500, w), np.uint8))
    assert np.array_equal(got, np.stack([a[s:s + w] for s in st]))
