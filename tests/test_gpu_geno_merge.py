"""snpgpu_geno_merge on the device, byte for byte against the numpy restatement (tests/geno_merge_ref.py), padding included: parts
at column offsets of every phase mod 4 and dwords of dst that hold several parts, rows that start off a dword between guard bytes,
permuted and repeated SNP lists, flips per part, every kind of source, several windows, nine parts, a caller's stream."""
import numpy as np
import pytest

import geno_merge_ref as R
import geno_select_ref as S
import mem_kinds as M
from snprelate_amd import _lib

pytestmark = pytest.mark.gpu


def _part(g, layout="packed", bit0=0, seed=0, **kw):
    """a part of the restatement (data, kw, lists) from codes g [n_snp][n_samp] written as a stream of `layout`"""
    data, d = S.make_stream(g, layout, bit0=bit0, seed=seed)
    return dict(data=data, kw=d, **kw)


def _lib_part(p, device_src=None):
    d = p["kw"]
    src = p["data"] if device_src is None else int(device_src.data_ptr())
    return _lib.merge_part(src, d["major"], d["n_rows"], d["n_cols"], bit0=d["bit0"], row_stride_bits=d.get("row_stride_bits"),
                           row_bit=d.get("row_bit"), samp_index=p.get("samp_index"), snp_index=p.get("snp_index"), flip=p.get("flip"),
                           n_bytes=None if device_src is None else len(p["data"]))


def _run(parts, offset=0, stream=None, device_src=None):
    """the merged rows of the library for the restatement's parts, written `offset` bytes past an aligned address between guards"""
    want = R.merge_ref(parts)
    dest = M.DeviceDest(want.shape, np.uint8, offset)
    dims = _lib.geno_merge([_lib_part(p, (device_src or {}).get(i)) for i, p in enumerate(parts)], dest.ptr, n_snp_out=want.shape[0],
                           stream=stream)
    got = dest.read()                                            # (checks both guards)
    assert dims[0] == want.shape[0] and (dims[1] + 3) // 4 == want.shape[1]
    return got, want


def _same(got, want):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d bytes differ, the first at row %d byte %d: %#x for %#x" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def _parts_of(sizes, L, missing=0.0, seed=3):
    return [_part(S.codes(L, n, missing, seed + i)) for i, n in enumerate(sizes)]


def test_offsets_of_every_phase_and_a_dword_of_four_parts():
    sizes = (1, 3, 5, 17, 64, 2, 3)                              # N = 95; offsets 0 1 4 9 26 90 92; codes 0 ... 15 hold four parts
    assert sum(sizes) == 95 and {o % 4 for o in np.cumsum((0,) + sizes[:-1])} == {0, 1, 2}
    parts = _parts_of(sizes, 5)
    _same(*_run(parts))
    parts = _parts_of((2, 1, 4, 64, 17, 5, 2), 5)                # offsets 0 2 3 7 71 88 93: phase 3 as well
    assert {o % 4 for o in np.cumsum([0, 2, 1, 4, 64, 17, 5])} == {0, 1, 2, 3}
    _same(*_run(parts))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_rows_that_start_off_a_dword_between_guards(offset):
    sizes = (1, 3, 5, 17, 6, 2, 3)                               # N = 37: rows of 10 bytes, every second one starts at 2 mod 4
    assert sum(sizes) == 37
    parts = _parts_of(sizes, 6, missing=0.1)
    for p, f in zip(parts, (None, [1] * 6, [0, 1] * 3, None, [1, 0] * 3, [1] * 6, None)):
        p["flip"] = f
    _same(*_run(parts, offset=offset))
    _same(*_run(_parts_of((1, 3, 5, 17, 64, 2, 3), 3), offset=offset))


def test_permuted_and_repeated_snps_flips_and_missing_codes():
    L, order = 9, np.array([4, 0, 8, 8, 2, 7, 1], np.int32)      # 7 output rows, one repeated
    sizes = (5, 18, 1, 33, 7)
    parts = _parts_of(sizes, L, missing=0.10)
    flips = (None, np.ones(7, np.uint8), np.arange(7) % 2, 1 - np.arange(7) % 2, 5 * np.ones(7, np.uint8))   # (any non-zero byte flips)
    rng = np.random.default_rng(5)
    for p, f in zip(parts, flips):
        p["snp_index"] = rng.permutation(order)
        p["flip"] = f
    got, want = _run(parts)
    _same(got, want)
    codes = R.unpack_ref(got, sum(sizes))
    assert (codes == 3).any() and (codes[:, 5:23] == 3).any()    # missing codes went through the flipped part as 3


def test_one_source_of_each_kind():
    import torch
    L = 11
    g = [S.codes(L, n, 0.05, 20 + i) for i, n in enumerate((6, 7, 13, 9, 21, 10, 5))]
    dirty = _part(g[0])                                          # byte-aligned host rows, the padding bits of every row dirty
    for pattern in (0x00, 0xAA):
        rows = dirty["data"].reshape(L, 2).copy()
        rows[:, 1] = (rows[:, 1] & 0x0F) | (pattern & 0xF0)
        dirty = dict(dirty, data=rows.reshape(-1))
        raw = _part(g[1], "sample.order", bit0=6, seed=1)       # the continuous stream with an odd number of samples
        major1 = _part(g[2], "snp.order", bit0=2, seed=2, flip=np.arange(L) % 2)
        onrows = _part(g[3], "row_bit0", seed=3)
        dev = _part(g[4], "sample.order", bit0=4, seed=4, snp_index=np.arange(L, dtype=np.int32)[::-1], flip=np.arange(L) % 3)
        listed = _part(g[5], samp_index=np.array([9, 0, 3, 3, 7], np.int32))
        run = _part(g[6], samp_index=np.array([1, 2, 3], np.int32))           # a run of consecutive samples: read where it lies
        parts = [dirty, raw, major1, onrows, dev, listed, run]
        on_device = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), dev["data"]])).cuda()[3:]     # (and off a dword)
        torch.cuda.synchronize()
        _same(*_run(parts, device_src={4: on_device}))
    # a sample list against NULL
    a, b = _part(g[5], samp_index=np.arange(10, dtype=np.int32)[::-1]), _part(g[5])
    got, want = _run([a, b])
    _same(got, want)
    c = R.unpack_ref(got, 20)
    assert np.array_equal(c[:, :10], c[:, 10:][:, ::-1])


def test_several_windows_give_the_single_window_result(monkeypatch):
    L = 50
    g = [S.codes(L, n, 0.05, 40 + i) for i, n in enumerate((9, 14, 3, 22, 6))]
    perm = np.random.default_rng(8).permutation(L).astype(np.int32)
    parts = [_part(g[0], flip=np.arange(L) % 2),                                         # in order, where it lies
             _part(g[1], "sample.order", bit0=2, snp_index=perm),                        # a list, where it lies
             _part(g[2], "snp.order", seed=1),                                           # staged: windows of columns
             _part(g[3], "row_bit0", seed=2, flip=np.arange(L) % 3),                     # staged: windows of row_bit
             _part(g[4], samp_index=np.array([5, 0, 2], np.int32))]                      # staged: windows of byte-aligned rows
    one, want = _run(parts)
    assert _lib.geno_merge_stats()["windows"] == 1
    _same(one, want)
    row_bytes = sum((n + 3) // 4 for n in (3, 22, 3))                                     # of the staged parts: 16 rows a window
    monkeypatch.setenv("SNPGPU_MERGE_STAGE_BYTES", str(16 * row_bytes))
    many, _ = _run(parts, offset=1)
    st = _lib.geno_merge_stats()
    assert st["windows"] == 4 and st["launches"] == 4 and st["bytes_written"] == want.size
    _same(many, want)
    monkeypatch.setenv("SNPGPU_MERGE_STAGE_BYTES", "1")                                   # at least one row per window
    rows1, _ = _run(parts)
    assert _lib.geno_merge_stats()["windows"] == L
    _same(rows1, want)


def test_one_part_with_flip_and_nine_parts():
    g = S.codes(23, 37, 0.1, 60)
    flip = (np.arange(23) % 3 == 0).astype(np.uint8)
    got, want = _run([_part(g, flip=flip)])                      # the snpgdsAlleleSwitch path
    _same(got, want)
    assert np.array_equal(R.unpack_ref(got, 37), np.where(flip[:, None] != 0, R.flip_codes(g), g))
    twice, _ = _run([dict(data=got.reshape(-1), kw=dict(major=0, n_rows=23, n_cols=37, bit0=0, row_stride_bits=80), flip=flip)])
    _same(twice, S.pack_ref(g))                                  # flipping twice restores the bytes
    sizes = (3, 1, 1, 2, 30, 1, 16, 15, 4)
    parts = _parts_of(sizes, 8, missing=0.05, seed=70)
    for i, p in enumerate(parts):
        p["flip"] = None if i % 3 == 0 else (np.arange(8) + i) % 2
    assert len(parts) == 9
    _same(*_run(parts, offset=3))


def test_more_parts_than_the_kernel_keeps_in_lds():
    sizes = [(1, 2, 3, 5, 18)[i % 5] for i in range(70)]         # (the kernel reads up to 64 descriptions from LDS, more from memory)
    parts = _parts_of(sizes, 4, missing=0.05, seed=100)
    for i, p in enumerate(parts):
        p["flip"] = None if i % 4 == 0 else (np.arange(4) + i) % 2
    _same(*_run(parts, offset=1))
    _same(*_run(parts[:64]))
    _same(*_run(parts[:65], offset=2))


def test_three_parts_of_300_snps_on_a_callers_stream():
    import torch
    L = 300
    parts = _parts_of((1000, 1, 2049), L, missing=0.02, seed=80)
    parts[2]["flip"] = np.arange(L) % 2
    parts[0]["samp_index"] = np.random.default_rng(9).permutation(1000).astype(np.int32)
    s = torch.cuda.Stream()
    got, want = _run(parts, offset=2, stream=s.cuda_stream)
    _same(got, want)
