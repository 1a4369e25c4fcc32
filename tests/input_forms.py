"""The ways a caller can hand ONE genotype matrix to a streaming context (snpgpu_feed and its siblings), as named forms.

From a canonical matrix g (uint8 [L][n], codes 0 / 1 / 2 and 3 = missing) and the block boundaries of the feeds, forms() builds
  u8_clean       g itself
  u8_dirty       every missing cell holds another byte of DIRTY_BYTES (include/snpgpu.h: U8 bytes 3..255 are all missing calls)
  packed_dirty   2-bit rows whose last byte carries random bits in the codes of samples >= n (they are ignored whatever they hold)
each from host memory, the two dirty ones also from device memory at byte offsets (2-bit rows: 0 .. 3, U8 rows: 0 and 1 -- rows that
were 16-byte aligned stop being aligned and the reverse), through two page-locked buffers used alternately, and through
snpgpu_block_stats + snpgpu_feed_stats.  decode() is the CPU inverse (tests/test_cpu_input_forms.py: every form is g again);
feed() drives an Accumulator, LDMatrix or MultiAccumulator with a form and needs a GPU.  Nothing here imports the HIP library
before feed() is called."""
from collections import namedtuple

import numpy as np

from snprelate_amd.gds import pack_2bit_rows

GENO_U8, GENO_PACKED2 = 0, 1           # enum snpgpu_geno_format

# one byte with only bit 2, 3, ... 7 set, the smallest and the largest byte above 3, and mixtures
DIRTY_BYTES = (3, 4, 5, 7, 8, 16, 32, 64, 128, 129, 252, 255)

Form = namedtuple("Form", "name fmt mem offset blocks")      # mem: host | device | pinned | stats; blocks: one uint8 array per feed


def scramble_padding(p, n_samp, seed=3):
    """random bits in the codes of samples >= n_samp of the last byte: they must not count whatever they hold"""
    p = p.copy()
    tail = (n_samp + 3) // 4 * 4 - n_samp
    if tail:
        keep = (1 << (2 * (4 - tail))) - 1
        r = np.random.default_rng(seed).integers(0, 256, p.shape[0]).astype(np.uint8)
        p[:, -1] = (p[:, -1] & keep) | (r & ~np.uint8(keep))
    return p


def dirty_u8(g, row0=0):
    """g with every missing cell (row r, column c; r counted from row0) replaced by DIRTY_BYTES[(r + c // 4 + 5 (c % 4)) % 12]: a
    cycle over the cell index in which, for each byte position c % 4 of a dword, the value moves on by one per row and per dword
    -- so every value turns up at every byte position, and the cells of one dword differ"""
    g = np.asarray(g, dtype=np.uint8)
    r = np.arange(row0, row0 + g.shape[0])[:, None]
    c = np.arange(g.shape[1])[None, :]
    pick = np.asarray(DIRTY_BYTES, np.uint8)[(r + c // 4 + 5 * (c % 4)) % len(DIRTY_BYTES)]
    return np.where(g > 2, pick, g).astype(np.uint8)


def decode(block, fmt, n_samp):
    """what a context must read from a block: 2-bit rows unpacked, the samples >= n_samp dropped, bytes above 3 clamped to 3"""
    b = np.asarray(block, dtype=np.uint8)
    if fmt == GENO_PACKED2:
        out = np.empty((b.shape[0], b.shape[1], 4), np.uint8)
        for k in range(4):
            out[:, :, k] = (b >> (2 * k)) & 3
        b = out.reshape(b.shape[0], -1)[:, :n_samp]
    return np.minimum(b, 3)


def padding_bits(packed, n_samp):
    """the bits of the unused codes of every row's last byte (all zero rows of a matrix with n_samp % 4 == 0)"""
    tail = (n_samp + 3) // 4 * 4 - n_samp
    return (np.asarray(packed)[:, -1] >> (2 * (4 - tail))) if tail else np.zeros(len(packed), np.uint8)


def forms(g, cuts, device=True, pinned=True, stats=True):
    """the list of Forms of g fed as the blocks cuts[i] .. cuts[i + 1]; device / pinned / stats: include those variants"""
    g = np.ascontiguousarray(g, dtype=np.uint8)
    n = g.shape[1]
    spans = list(zip(cuts[:-1], cuts[1:]))
    clean = [np.ascontiguousarray(g[a:b]) for a, b in spans]
    dirty = [dirty_u8(g[a:b], a) for a, b in spans]
    packed = [scramble_padding(pack_2bit_rows(g[a:b]), n, seed=3 + i) for i, (a, b) in enumerate(spans)]
    out = [Form("u8_clean", GENO_U8, "host", 0, clean), Form("u8_dirty", GENO_U8, "host", 0, dirty),
           Form("packed_dirty", GENO_PACKED2, "host", 0, packed)]
    if device:
        out += [Form("packed_dirty device + %d" % o, GENO_PACKED2, "device", o, packed) for o in range(4)]
        out += [Form("u8_dirty device + %d" % o, GENO_U8, "device", o, dirty) for o in range(2)]
    if pinned:
        out += [Form("u8_dirty pinned", GENO_U8, "pinned", 0, dirty), Form("packed_dirty pinned", GENO_PACKED2, "pinned", 0, packed)]
    if stats:
        out += [Form("u8_dirty stats", GENO_U8, "stats", 0, dirty), Form("packed_dirty stats", GENO_PACKED2, "stats", 0, packed)]
    return out


def snp_stats(g):
    """(sum, num) int32 per SNP: the sum of the called genotypes and their number (what snpgpu_block_stats returns)"""
    g = np.asarray(g)
    called = g < 3
    return np.where(called, g, 0).sum(axis=1).astype(np.int32), called.sum(axis=1).astype(np.int32)


def _device_copy(block, offset):
    """(tensor, address): the block's bytes at `offset` inside a larger device buffer of called genotypes (0x5A); the allocation
    itself is 256-byte aligned, so the address is `offset` past such a boundary"""
    import torch
    buf = torch.full((block.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    buf[offset:offset + block.size] = torch.from_numpy(np.ascontiguousarray(block).reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 256 == 0
    return buf, int(buf.data_ptr()) + offset


def feed(acc, form):
    """feed every block of `form` to acc (Accumulator; LDMatrix and MultiAccumulator for host and device forms).  Returns None, or
    for a stats form the (sum, num) int32 arrays snpgpu_block_stats produced for all blocks."""
    if form.mem == "host":
        for b in form.blocks:
            acc.feed(b, form.fmt)
        return None
    if form.mem == "device":
        for b in form.blocks:
            keep, ptr = _device_copy(b, form.offset)
            acc.feed_device(ptr, b.shape[0], form.fmt)
            if hasattr(acc, "sync"):                     # the buffer goes away with `keep` (snpgpu_ld_feed has read its rows
                acc.sync()                               # when it returns: LDMatrix has nothing to wait for)
            del keep
        return None
    if form.mem == "pinned":
        from snprelate_amd import _lib
        rows = max(b.shape[0] for b in form.blocks)
        bufs = [_lib.PinnedBuffer((rows, form.blocks[0].shape[1])) for _ in range(2)]
        try:
            for k, b in enumerate(form.blocks):
                pb = bufs[k & 1]
                acc.host_wait(pb)                        # the copy of the block this buffer held before has left it
                pb.array[:b.shape[0]] = b
                acc.feed_pinned(pb, b.shape[0], form.fmt)
            acc.sync()
        finally:
            for pb in bufs:
                pb.free()
        return None
    assert form.mem == "stats"
    import torch
    sums, nums = [], []
    for b in form.blocks:
        keep, ptr = _device_copy(b, form.offset)
        st = torch.full((2, b.shape[0]), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        acc.block_stats_device(ptr, b.shape[0], st[0].data_ptr(), st[1].data_ptr(), form.fmt)
        acc.feed_device_stats(ptr, b.shape[0], st[0].data_ptr(), st[1].data_ptr(), form.fmt)
        acc.sync()
        h = st.cpu().numpy()
        sums.append(h[0].copy()); nums.append(h[1].copy())
        del keep, st
    return np.concatenate(sums), np.concatenate(nums)
