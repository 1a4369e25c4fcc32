"""The input forms of tests/input_forms.py on the CPU: every form is the canonical matrix again once decoded, the dirty forms are
dirty where tests/test_gpu_input_forms.py needs them to be, and the shared scramble_padding is the function the GPU test files
used to carry privately."""
import numpy as np
import pytest

import input_forms as F
from oracle.synth import synth_geno
from snprelate_amd.gds import pack_2bit_rows

CUTS = [0, 256, 556, 700]
SIZES = [61, 62, 63, 64, 65, 333, 1037, 1040, 1041]


def _geno(n):
    g = synth_geno(n, CUTS[-1], missing=0.04, seed=n, special=True)
    mid = g[CUTS[1]:CUTS[2]]
    mid[mid > 2] = 1                       # a block without missing calls
    return g


@pytest.mark.parametrize("n", SIZES)
def test_every_form_decodes_to_the_canonical_matrix(n):
    g = _geno(n)
    fs = F.forms(g, CUTS)
    assert [f.name for f in fs] == ["u8_clean", "u8_dirty", "packed_dirty", "packed_dirty device + 0", "packed_dirty device + 1",
                                    "packed_dirty device + 2", "packed_dirty device + 3", "u8_dirty device + 0", "u8_dirty device + 1",
                                    "u8_dirty pinned", "packed_dirty pinned", "u8_dirty stats", "packed_dirty stats"]
    for f in fs:
        assert [b.shape[0] for b in f.blocks] == [256, 300, 144]
        assert all(b.dtype == np.uint8 and b.flags.c_contiguous for b in f.blocks)
        assert all(b.shape[1] == (n if f.fmt == F.GENO_U8 else (n + 3) // 4) for b in f.blocks)
        back = np.concatenate([F.decode(b, f.fmt, n) for b in f.blocks])
        assert np.array_equal(back, g), f.name
    assert np.array_equal(fs[0].blocks[0], g[:256])
    assert len(F.forms(g, CUTS, device=False, pinned=False, stats=False)) == 3


@pytest.mark.parametrize("n", SIZES)
def test_dirty_forms_are_dirty(n):
    g = _geno(n)
    fs = {f.name: f for f in F.forms(g, CUTS)}
    d = np.concatenate(fs["u8_dirty"].blocks)
    assert np.array_equal(d > 2, g > 2) and np.array_equal(d[g < 3], g[g < 3])
    assert not (np.concatenate(fs["u8_dirty"].blocks[1:2]) > 2).any()          # the middle block stays without missing calls
    col = np.broadcast_to(np.arange(n)[None, :], g.shape)
    for v in F.DIRTY_BYTES:
        for pos in range(4):                                                    # every value at every byte position of a dword
            assert ((d == v) & (col % 4 == pos)).any(), (v, pos)
    # ... in the part of a row that repack_stats_kernel converts 16 samples at a time, and in its scalar tail (n % 16 != 0)
    tail0 = n // 16 * 16
    for v in F.DIRTY_BYTES:
        assert (d[:, :tail0] == v).any()
        assert n - tail0 < 13 or (d[:, tail0:] == v).any(), v                   # (a tail of 13 .. 15 samples has room for all)
    assert tail0 == n or (d[:, tail0:] > 3).any()
    # the cells of one dword differ: a row that is missing everywhere (SNP 7 of synth_geno's planted rows)
    assert (g[7] == 3).all() and len(set(d[7, :4])) == 4
    for blk, p in zip(fs["u8_clean"].blocks, fs["packed_dirty"].blocks):
        bits = F.padding_bits(p, n)
        if n % 4:
            assert bits.any() and len(set(bits.tolist())) > 1                   # not zero, and not one constant either
            assert not np.array_equal(p, pack_2bit_rows(blk))
        else:
            assert np.array_equal(p, pack_2bit_rows(blk))
    assert fs["packed_dirty device + 3"].offset == 3 and fs["u8_dirty device + 1"].offset == 1


def test_dirty_byte_cycle_is_a_function_of_the_cell_alone():
    """a block cut out of the matrix gets the bytes the whole matrix would get (row0), so the forms do not depend on the cuts"""
    g = _geno(65)
    assert np.array_equal(F.dirty_u8(g)[256:556], F.dirty_u8(g[256:556], 256))
    assert np.array_equal(F.dirty_u8(g)[600:], F.dirty_u8(g[600:], 600))
    assert sorted(set(F.dirty_u8(g)[g > 2].tolist())) == sorted(F.DIRTY_BYTES)


# what the private _scramble_padding of tests/test_gpu_qc.py, test_gpu_ld.py, test_gpu_ibd_mle.py, test_gpu_pair_score.py and
# test_gpu_fst.py gave (recorded from it before it moved) for 8 rows of two bytes {0xA5, 9 r}: the last byte per sample count,
# with the default seed 3 and with seed 4
_RECORDED = {5: ([204, 21, 46, 63, 44, 205, 222, 151], [184, 241, 226, 131, 240, 249, 250, 23]),
             6: ([192, 25, 34, 59, 36, 205, 214, 159], [176, 249, 226, 139, 244, 253, 246, 31]),
             7: ([192, 9, 18, 27, 36, 237, 246, 191], [128, 201, 210, 155, 228, 237, 246, 63]),
             8: ([0, 9, 18, 27, 36, 45, 54, 63], [0, 9, 18, 27, 36, 45, 54, 63])}


@pytest.mark.parametrize("n", sorted(_RECORDED))
def test_shared_scramble_padding_equals_the_private_copies(n):
    p = np.empty((8, 2), np.uint8)
    p[:, 0] = 0xA5
    p[:, 1] = np.arange(8) * 9
    p0 = p.copy()
    for kw, want in zip(({}, {"seed": 4}), _RECORDED[n]):
        got = F.scramble_padding(p, n, **kw)
        assert got.dtype == np.uint8 and got[:, 1].tolist() == want and np.array_equal(got[:, 0], p0[:, 0])
        assert np.array_equal(F.decode(got, F.GENO_PACKED2, n), F.decode(p0, F.GENO_PACKED2, n))      # the samples keep their codes
    assert np.array_equal(p, p0)                                                                    # the input is left alone


def test_snp_stats_reference():
    g = _geno(63)
    s, c = F.snp_stats(g)
    assert s.dtype == np.int32 and c.dtype == np.int32
    assert s[7] == 0 and c[7] == 0 and c[11] == 1 and s[11] == 1 and s[5] == 2 * 63 and c[5] == 63
    assert np.array_equal(s, np.array([int(r[r < 3].sum()) for r in g])) and np.array_equal(c, np.array([int((r < 3).sum()) for r in g]))
