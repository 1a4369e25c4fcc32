"""syrk_uv16c_kernel with EVERY sub-tile sum carried between the fp32 runs of a block: 35 of a wave's 64 in LDS as before, the other 29 in
a scratch slot of device memory that the work item takes from its XCD's pool (SNPGPU_UVC_CARRY_ALL, default on; SNPGPU_UVC_CARRY_SLOTS
slots per pool).  A work item that finds no free slot adds those 29 sub-tiles to the panel after every run, as before the scratch existed.

Every GPU case checks GCTA against the CPU oracle with the project's figure (< 1e-5); the data holds no missing calls and the tiles are whole
(SNPGPU_I8_TAIL_PARTS=1), so that every work item walks its runs itself.  Which path ran is read from the kernel's fallback count."""
import numpy as np
import pytest

import oracle as orc
from conftest import synth_geno

gpu = pytest.mark.gpu

N_SMALL, L_SMALL = 700, 9000          # 3 x 3 tiles of 256, the last ones ending in padding rows
N_POOL, L_POOL = 4000, 4096           # 16 tile rows: 136 tiles, ~17 per XCD


@pytest.fixture(scope="module")
def small():
    g = synth_geno(N_SMALL, L_SMALL, missing=0.0, seed=4177, special=False)      # (special plants all-missing SNPs)
    g.setflags(write=False)
    ref = orc.grm_gcta(g)
    ref.setflags(write=False)
    return g, ref


@pytest.fixture(scope="module")
def pool():
    g = synth_geno(N_POOL, L_POOL, missing=0.0, seed=4178, special=False)
    g.setflags(write=False)
    ref = orc.grm_gcta(g)
    ref.setflags(write=False)
    return g, ref


def _rel_err(got, ref):
    """tests/norms.py: the larger of the contract figure and the off-diagonal-floor figure (as tests/test_gpu_parity.py)"""
    from norms import error_figures, tri_diag_scale
    n = int((np.sqrt(8 * ref.size + 1) - 1) / 2 + 0.5)
    f = error_figures(got, ref, tri_diag_scale(ref, n))
    return max(f["contract"], f["offdiag"])


def _whole_tiles(monkeypatch, promote=None, carry_all=None, slots=None):
    monkeypatch.setenv("SNPGPU_SYRK", "f16")
    monkeypatch.setenv("SNPGPU_SYRK_UV16", "3")
    monkeypatch.setenv("SNPGPU_I8_TAIL_PARTS", "1")
    for name, v in (("SNPGPU_H3_PROMOTE", promote), ("SNPGPU_UVC_CARRY_ALL", carry_all), ("SNPGPU_UVC_CARRY_SLOTS", slots)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _grm(g, block, bounds=None, packed=True):
    """(result, work items that fell back) of a GCTA GRM fed in blocks of `block` SNPs, as one context or as row panels"""
    from snprelate_amd import _lib
    from snprelate_amd.dist import slab_range
    n = g.shape[1]
    bounds = bounds or [0, n]
    got = None if not packed else np.zeros(n * (n + 1) // 2)
    fell = 0
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        with _lib.Accumulator(_lib.GRM_GCTA, n, row_begin=r0, row_end=r1 if len(bounds) > 2 else 0, max_block_snps=block) as a:
            for i in range(0, g.shape[0], block):
                a.feed(g[i:i + block])
            if packed:
                lo, hi = slab_range(n, r0, r1)
                got[lo:hi] = a.grm_gcta(packed=True)
            else:
                got = a.grm_gcta(packed=False)
            fell += a.carry_fallbacks()
    return got, fell


# runs per block: two (a 4096-SNP block = four table chunks as 2 + 2), three and six (1024-slot runs: one table chunk each; six is the
# headline's count and gives every run its own weight-target factor)
RUNS = [(2, None, 4096), (3, 1024, 3072), (6, 1024, 6144)]


@gpu
@pytest.mark.parametrize("runs,promote,block", RUNS)
def test_run_counts_vs_oracle(small, runs, promote, block, monkeypatch):
    from snprelate_amd import _lib
    _whole_tiles(monkeypatch, promote=promote)
    d = _lib.diag_plan(_lib.GRM_GCTA, N_SMALL, block_snps=block, max_block_snps=block)
    assert (d["uv_form"], d["uvc_carry_all"], int(d["uv_runs"])) == ("converted_carry", "1", runs)
    g, ref = small
    got, fell = _grm(g, block)
    err = _rel_err(got, ref)
    print("runs %d: rel err %.3g, fallbacks %d" % (runs, err, fell))
    assert err < 1e-5
    assert fell == 0              # six work items per launch, 64 slots in every pool


@gpu
def test_row_panels_vs_oracle(small, monkeypatch):
    """three row panels: a panel with a column offset, panels that end in padding rows (n_rows_real masks the flush)"""
    _whole_tiles(monkeypatch, promote=1024)
    g, ref = small
    got, fell = _grm(g, 6144, bounds=[0, 256, 512, N_SMALL])
    err = _rel_err(got, ref)
    print("row panels: rel err %.3g, fallbacks %d" % (err, fell))
    assert err < 1e-5
    assert fell == 0


@gpu
def test_slots_are_released(small, monkeypatch):
    """nine launches of six work items on pools of six slots (48 in all): wherever the work items run, a launch finds its XCD's pool
    free if and only if the launches before it gave their slots back"""
    _whole_tiles(monkeypatch, slots=6)
    g, ref = small
    got, fell = _grm(g, 1024)
    assert _rel_err(got, ref) < 1e-5
    assert fell == 0


def _lds_carried(r, c):
    """sub-tile map of syrk_uv16c_kernel: a wave owns 128 x 128 of a 256 x 256 tile as 8 x 8 sub-tiles of 16 x 16; sub-tile 8 i + j < 35
    is carried in LDS"""
    return ((r % 128) // 16) * 8 + (c % 128) // 16 < 35


@gpu
def test_lds_carried_sub_tiles_unchanged(small, monkeypatch):
    """The K loop and the LDS carry did not change, and atomics into distinct addresses do not reorder sums: with the scratch on, the
    entries of sub-tiles 0 ... 34 of every wave are bit-identical to SNPGPU_UVC_CARRY_ALL=0; the others moved (different roundings).
    Only SNPs with more than UV_SPARSE_MAC = 128 copies of the minor allele: rarer ones leave the dense product and reach the panel as
    fp64 atomics of uv_sparse_kernel, several per entry in an order that changes from run to run -- with them no two runs of EITHER
    form agree bit for bit (about nine tenths of the 9000 SNPs stay: blocks of six and of two runs)."""
    g, _ = small
    mac = np.minimum(g.sum(1, dtype=np.int64), 2 * N_SMALL - g.sum(1, dtype=np.int64))
    g = np.ascontiguousarray(g[mac > 128])
    assert g.shape[0] > 6144 + 1024
    ref = orc.grm_gcta(g)
    _whole_tiles(monkeypatch, promote=1024, carry_all=0)
    old, fell_old = _grm(g, 6144, packed=False)
    _whole_tiles(monkeypatch, promote=1024)
    new, fell_new = _grm(g, 6144, packed=False)
    assert (fell_old, fell_new) == (0, 0)          # (no scratch: nothing to fall back from)
    r, c = np.triu_indices(N_SMALL)
    # an entry of a diagonal tile may be read from either triangle of the tile: both sub-tiles must be LDS-carried there
    lds = _lds_carried(r, c) & ((r // 256 != c // 256) | _lds_carried(c, r))
    assert 0.3 < lds.mean() < 0.6
    assert np.array_equal(old[r, c][lds], new[r, c][lds])
    assert not np.array_equal(old[r, c][~lds], new[r, c][~lds])
    assert _rel_err(new[r, c], ref) < 1e-5 and _rel_err(old[r, c], ref) < 1e-5


@gpu
def test_slot_pools_reuse_and_fallback(pool, monkeypatch):
    """136 work items of four runs in one launch: pools of 64 serve all of them; pools of 2 (16 slots in all) leave most without a slot;
    pools of 0 leave all -- and that is the code path of SNPGPU_UVC_CARRY_ALL=0, bit for bit (no SNP of this data is rare enough
    for the fp64 atomics of uv_sparse_kernel, whose order is not reproducible: 8000 alleles, minor allele frequency >= 5 %)."""
    g, ref = pool
    assert np.minimum(g.sum(1, dtype=np.int64), 2 * N_POOL - g.sum(1, dtype=np.int64)).min() > 128
    items = (N_POOL + 255) // 256 * ((N_POOL + 255) // 256 + 1) // 2
    assert items == 136
    res = {}
    for name, kw in (("64", {}), ("2", dict(slots=2)), ("0", dict(slots=0)), ("off", dict(carry_all=0))):
        _whole_tiles(monkeypatch, promote=1024, **kw)
        res[name] = _grm(g, 4096)
        print("pools of %s: rel err %.3g, fallbacks %d" % (name, _rel_err(res[name][0], ref), res[name][1]))
    for name in res:
        assert _rel_err(res[name][0], ref) < 1e-5, name
    assert res["64"][1] == 0
    assert 0 < res["2"][1] < items
    assert res["0"][1] == items
    assert res["off"][1] == 0
    assert np.array_equal(res["0"][0], res["off"][0])


def test_switches_parse_and_show_in_the_plan(monkeypatch):
    """no GPU: SNPGPU_UVC_CARRY_ALL and SNPGPU_UVC_CARRY_SLOTS through plan_context / plan_block and the plan dump"""
    from snprelate_amd import _lib
    for k in ("SNPGPU_SYRK", "SNPGPU_SYRK_UV16", "SNPGPU_UVC_CARRY_ALL", "SNPGPU_UVC_CARRY_SLOTS", "SNPGPU_H3_PROMOTE", "SNPGPU_SYRK_UV"):
        monkeypatch.delenv(k, raising=False)

    def plan(kind=_lib.GRM_GCTA, **kw):
        return _lib.diag_plan(kind, 700, **kw)

    d = plan(block_snps=65536, max_block_snps=65536)
    assert (d["uv_form"], d["uvc_carry_all"], d["uvc_carry_slots"], d["uv_runs"]) == ("converted_carry", "1", "64", "6")
    assert plan(_lib.PCA_COV)["uvc_carry_all"] == "1"
    monkeypatch.setenv("SNPGPU_UVC_CARRY_SLOTS", "2")
    assert plan()["uvc_carry_slots"] == "2"
    monkeypatch.setenv("SNPGPU_UVC_CARRY_SLOTS", "0")
    d = plan()
    assert (d["uvc_carry_all"], d["uvc_carry_slots"]) == ("1", "0")
    for bad in ("-1", "257", "100000"):            # outside 0 ... 256: the default
        monkeypatch.setenv("SNPGPU_UVC_CARRY_SLOTS", bad)
        assert plan()["uvc_carry_slots"] == "64"
    monkeypatch.setenv("SNPGPU_UVC_CARRY_SLOTS", "8")
    monkeypatch.setenv("SNPGPU_UVC_CARRY_ALL", "0")
    d = plan()
    assert (d["uv_form"], d["uvc_carry_all"], d["uvc_carry_slots"]) == ("converted_carry", "0", "0")
    monkeypatch.setenv("SNPGPU_UVC_CARRY_ALL", "1")
    assert plan()["uvc_carry_slots"] == "8"
    # only the form that walks the runs inside has sums to carry; the other kinds have no such kernel
    monkeypatch.setenv("SNPGPU_SYRK_UV16", "2")
    d = plan()
    assert (d["uv_form"], d["uvc_carry_all"], d["uvc_carry_slots"]) == ("converted", "0", "0")
    monkeypatch.delenv("SNPGPU_SYRK_UV16")
    assert plan(_lib.EIGMIX)["uvc_carry_all"] == "0"
    assert "uvc_carry_all" not in plan(_lib.IBS)
    assert "snpgpu_diag_carry_fallbacks" in _lib.EXPORTS and hasattr(_lib.lib(), "snpgpu_diag_carry_fallbacks")
