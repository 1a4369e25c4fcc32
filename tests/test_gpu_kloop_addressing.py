"""Where syrk_uv16c_kernel's genotype-word addresses can go wrong.  The K loop keeps ONE running 64-bit base per run -- set from the
run's first chunk in the prologue, advanced by the constant stride of a 32-SNP group once per group -- plus a 32-bit lane offset per
operand side.  Each case below is a place where such a base starts or ends somewhere else than at a block's first word:

  * a partial last chunk and an odd block size (the last chunk holds fewer than 32 groups), two such blocks;
  * tiles split along K (a work item's base starts at its own first chunk, not at the run's);
  * the fused (tile, run) launch (SNPGPU_SYRK_UV16=2: every work item starts at its run's first chunk);
  * row panels (row and column offsets differ, the word array starts at the panel's first column);
  * a word array of more than 4 GiB, whose last groups lie beyond what 32 bits reach.

Every small case is GCTA against the CPU oracle with the project's two figures (tests/norms.py, < 1e-5); the large one against
tests/fp64_anchor.py as tests/test_gpu_fullsize.py uses it."""
import numpy as np
import pytest

import oracle as orc
from conftest import synth_geno

gpu = pytest.mark.gpu

N, L = 700, 10000                     # 3 x 3 tiles of 256, the last ones ending in padding rows
ODD = 5000                            # an odd block size: five table chunks, the last one partial; L = two such blocks


@pytest.fixture(scope="module")
def data():
    g = synth_geno(N, L, missing=0.0, seed=5179, special=False)      # (special plants all-missing SNPs)
    g.setflags(write=False)
    ref = orc.grm_gcta(g)
    ref.setflags(write=False)
    return g, ref


def _figures(got, ref):
    """tests/norms.py: the contract figure and the off-diagonal-floor figure"""
    from norms import error_figures, tri_diag_scale
    f = error_figures(got, ref, tri_diag_scale(ref, N))
    return f["contract"], f["offdiag"]


def _env(monkeypatch, form="3", promote=1024, whole_tiles=True):
    monkeypatch.setenv("SNPGPU_SYRK", "f16")
    monkeypatch.setenv("SNPGPU_SYRK_UV16", form)
    for name, v in (("SNPGPU_H3_PROMOTE", promote), ("SNPGPU_I8_TAIL_PARTS", 1 if whole_tiles else None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    for name in ("SNPGPU_UVC_CARRY_ALL", "SNPGPU_UVC_CARRY_SLOTS", "SNPGPU_UVC_PACE", "SNPGPU_SYRK_UV"):
        monkeypatch.delenv(name, raising=False)


def _grm(g, block, bounds=None):
    """(packed GCTA GRM fed in blocks of `block` SNPs as one context or as row panels, work items that found no carry slot)"""
    from snprelate_amd import _lib
    from snprelate_amd.dist import slab_range
    bounds = bounds or [0, N]
    got = np.zeros(N * (N + 1) // 2)
    fell = 0
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        with _lib.Accumulator(_lib.GRM_GCTA, N, row_begin=r0, row_end=r1 if len(bounds) > 2 else 0, max_block_snps=block) as a:
            for i in range(0, g.shape[0], block):
                a.feed(g[i:i + block])
            lo, hi = slab_range(N, r0, r1)
            got[lo:hi] = a.grm_gcta(packed=True)
            fell += a.carry_fallbacks()
    return got, fell


def _plan(block):
    from snprelate_amd import _lib
    return _lib.diag_plan(_lib.GRM_GCTA, N, block_snps=block, max_block_snps=block)


@gpu
def test_partial_last_chunk_and_odd_block(data, monkeypatch):
    """blocks of 5000 SNPs as five 1024-slot runs, the last chunk with fewer than 32 groups; whole tiles, so that every work item walks
    all five runs and sets its base five times"""
    _env(monkeypatch)
    d = _plan(ODD)
    assert (d["uv_form"], int(d["uv_runs"]), int(d["uv_chunks"])) == ("converted_carry", 5, 5)
    g, ref = data
    got, fell = _grm(g, ODD)
    contract, offdiag = _figures(got, ref)
    print("odd blocks: contract %.3g, off-diagonal %.3g, fallbacks %d" % (contract, offdiag, fell))
    assert contract < 1e-5 and offdiag < 1e-5
    assert fell == 0


@gpu
@pytest.mark.parametrize("promote", [1024, None])
def test_tiles_split_along_k(data, promote, monkeypatch):
    """The same data without SNPGPU_I8_TAIL_PARTS=1: six tiles fill a fraction of one round of the device, so the work list splits each
    along K (tail_parts = 0 in the plan: chosen per list, worklist.h) and the parts start at their own c_beg.  With 1024-slot runs a run is
    one chunk and only part 0 has work; at the default run length a run holds three chunks (two runs per block) and parts 1 and 2
    start in the middle of it.  That the split path ran shows in the sums: K parts meet in the fp64 panel instead of in one fp32
    accumulator, so some of the 245 350 entries round differently from the whole-tile walk."""
    g, ref = data
    _env(monkeypatch, promote=promote, whole_tiles=True)
    whole, _ = _grm(g, ODD)
    _env(monkeypatch, promote=promote, whole_tiles=False)
    d = _plan(ODD)
    assert (d["uv_form"], d["tail_parts"]) == ("converted_carry", "0")
    assert int(d["uv_runs"]) == (5 if promote else 2) and int(d["uv_cpr"]) == (1 if promote else 3)
    split, fell = _grm(g, ODD)
    contract, offdiag = _figures(split, ref)
    print("split along K (promote %s): contract %.3g, off-diagonal %.3g" % (promote, contract, offdiag))
    assert contract < 1e-5 and offdiag < 1e-5
    assert fell == 0                      # (a split tile carries nothing: it never asks for a slot)
    if promote is None:
        assert not np.array_equal(split, whole)


@gpu
def test_fused_tile_run_items(data, monkeypatch):
    """SNPGPU_SYRK_UV16=2: one launch of (tile, run) items, six runs per 6144-SNP block; an item's base starts at its run's first chunk"""
    _env(monkeypatch, form="2")
    d = _plan(6144)
    assert (d["uv_form"], int(d["uv_runs"])) == ("converted", 6)
    g, ref = data
    got, _ = _grm(g, 6144)
    contract, offdiag = _figures(got, ref)
    print("fused items: contract %.3g, off-diagonal %.3g" % (contract, offdiag))
    assert contract < 1e-5 and offdiag < 1e-5


@gpu
def test_row_panels(data, monkeypatch):
    """three row panels, six runs: the row offset counts from the panel's first row, the column offset from its first column, and the
    word array is as wide as the panel's columns"""
    _env(monkeypatch)
    assert int(_plan(6144)["uv_runs"]) == 6
    g, ref = data
    got, fell = _grm(g, 6144, bounds=[0, 256, 512, N])
    contract, offdiag = _figures(got, ref)
    print("row panels: contract %.3g, off-diagonal %.3g, fallbacks %d" % (contract, offdiag, fell))
    assert contract < 1e-5 and offdiag < 1e-5
    assert fell == 0


N_BIG, B_BIG, SEED_BIG = 132096, 65536, 20240601      # 516 tile rows; one block of the headline's size


@gpu
def test_word_array_beyond_4_gib(monkeypatch):
    """One 65 536-SNP block at N = 132 096 on 256-row panels.  A panel's word array spans its COLUMNS (first row to last sample) x B / 2
    bytes: for the panel of the first tile row that is 132 096 x 32 768 = 4.33 GB, and the words of the block's last 16 groups lie
    beyond 4 GiB; the panel of the last whole tile row has the largest row and column offsets of the sample range (its own word array
    is 256 columns wide).  Every entry sums over all SNPs, so a base or an offset that wraps in the last groups shows in all of them.
    Data from the device generator, per-SNP statistics by torch, a few hundred entries per panel recomputed in fp64 on the CPU."""
    import torch
    from snprelate_amd import _lib
    from fp64_anchor import Fp64Anchor, block_stats_torch
    from norms import error_figures
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip("needs 16 GB of free device memory, has %.1f" % (free / 2.0 ** 30))
    for k in ("SNPGPU_SYRK", "SNPGPU_SYRK_UV16", "SNPGPU_SYRK_UV", "SNPGPU_H3_PROMOTE", "SNPGPU_I8_TAIL_PARTS"):      # the default path
        monkeypatch.delenv(k, raising=False)
    n, B = N_BIG, B_BIG
    panels = [(0, 256), (n - 256, n)]
    d = _lib.diag_plan(_lib.GRM_GCTA, n, block_snps=B, max_block_snps=B, rows=panels[0])
    assert d["syrk_kernel_nomiss"] == "syrk_uv16c_kernel" and d["uv_form"] == "converted_carry"
    assert int(d["ncols_pad"]) * (B // 2) > 1 << 32
    blk = torch.empty((B, (n + 3) // 4), dtype=torch.uint8, device="cuda")
    _lib.synth_block(blk.data_ptr(), n, 0, B, SEED_BIG, missing=0.0)
    s, c = [np.concatenate(x) for x in zip(*(block_stats_torch(blk[i:i + 8192]) for i in range(0, B, 8192)))]
    for r0, r1 in panels:
        anchor = Fp64Anchor(n, r0, r1, 16, 64, "GRM_GCTA", SEED_BIG, 0.0, 0)      # (entries left of the diagonal drop out)
        anchor.add(0, B, s, c)
        with _lib.Accumulator(_lib.GRM_GCTA, n, row_begin=r0, row_end=r1, max_block_snps=B) as a:
            a.feed_device(blk.data_ptr(), B)
            out = torch.empty(a.slab_size(), dtype=torch.float64, device="cuda")
            a.grm_gcta(packed=True, out_ptr=out.data_ptr())
        torch.cuda.synchronize()
        idx, want = anchor.finish()
        got = out[torch.from_numpy(idx).to("cuda")].cpu().numpy()
        diag = (anchor.cols[None, :] == anchor.rows[:, None])[anchor.cols[None, :] >= anchor.rows[:, None]]      # (finish()'s order)
        assert diag.sum() >= 2 and idx.size >= 300
        f = error_figures(got, want, float(np.median(want[diag])))
        print("panel rows %d .. %d: %d entries, contract %.3g, off-diagonal %.3g" % (r0, r1, idx.size, f["contract"], f["offdiag"]))
        assert f["contract"] < 1e-5 and f["offdiag"] < 1e-5, f
        del out
