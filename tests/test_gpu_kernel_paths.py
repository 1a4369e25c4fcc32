"""Every kernel path a switch can select, run against the oracle (tests/kernel_paths.py holds the table, tests/test_cpu_kernel_paths.py
holds it against the library): one parametrised test over CASES, then one hand-written test per switch that changes geometry or
launches without changing a kernel's name.  Every test proves the path it means to run: from the live plan, from the context's span
and launch counters, and -- where two paths differ in arithmetic -- from the bits of the result."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_paths as K
import oracle as orc
from conftest import ROOT, synth_geno

pytestmark = pytest.mark.gpu

FEEDS = (320, 256, 324)          # the outer two with 5 % missing calls, the middle one without: every quadruple runs both of its kernels
L_FEEDS = sum(FEEDS)


def _figures(got, ref, n=None):
    """(contract, off-diagonal) figure of a packed triangle or slab against its reference (tests/norms.py); diag scale from `n`-sample ref"""
    from norms import error_figures, tri_diag_scale
    f = error_figures(got, ref, tri_diag_scale(ref, n) if n else 1.0)
    return f["contract"], f["offdiag"]


def _rel_err(got, ref, n):
    """test_gpu_parity._rel_err: the larger of the contract and the off-diagonal-floor figure"""
    return max(_figures(got, ref, n))


@functools.lru_cache(maxsize=None)
def _geno(n):
    """three feeds of 320, 256 and 324 SNPs: 5 % missing calls, none, 5 %; monomorphic, all-missing and single-call SNPs in the first"""
    g = synth_geno(n, L_FEEDS, missing=0.05, seed=4000 + n, special=True)
    clean = synth_geno(n, L_FEEDS, missing=0.0, seed=5000 + n, special=False)
    lo, hi = FEEDS[0], FEEDS[0] + FEEDS[1]
    g[lo:hi] = clean[lo:hi]
    assert (g[:lo] > 2).any() and not (g[lo:hi] > 2).any() and (g[hi:] > 2).any()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _reference(kind, n):
    """the oracle's result of `kind` on _geno(n), computed once and left unchanged"""
    g = _geno(n)
    if kind == "IBS":
        ref = (orc.ibs_count(g),)
    elif kind == "KING_ROBUST":
        ref = (orc.king_robust_count(g),)
    elif kind == "INDIV_BETA":
        ref = orc.beta_final_ibd(orc.beta_count(g), n, True)
    elif kind == "KING_HOMO":
        c, fs = orc.king_homo_count(g)
        ref = orc.king_homo_final(c, fs, n)
    elif kind == "GRM_GCTA":
        ref = (orc.grm_gcta(g),)
    elif kind == "PCA_COV":
        ref = orc.pca_cov(g, False)
        orc.trace_normalize(ref, n)
        ref = (ref,)
    elif kind == "EIGMIX":
        ref = (orc.eigmix(g, True)[0],)
    else:
        import diss_ref as R
        sg, sa = R.diss_sums(g)
        ref = (R.packed_upper(sg), R.packed_upper(sa))
    for r in ref:
        if isinstance(r, np.ndarray):
            r.setflags(write=False)
    return ref


def _run(kind, n, rows=None):
    """feed _geno(n) to a context of `kind` created under the environment as it stands: (results, spans of the counter family, spans
    of the SYRK family, SYRK kernel launches)"""
    from snprelate_amd import _lib
    g = _geno(n)
    kw = dict(row_begin=rows[0], row_end=rows[1]) if rows else {}
    with _lib.Accumulator(getattr(_lib, kind), n, max_block_snps=512, **kw) as a:
        a.set_timing(True)
        lo = 0
        for m in FEEDS:
            a.feed(g[lo:lo + m])
            lo += m
        assert a.counts()[0] == L_FEEDS
        if kind == "IBS":
            out = (np.stack(a.ibs_num(packed=True), 1).astype(np.uint32),)
        elif kind == "KING_ROBUST":
            out = (a.king_robust_counts(),)
        elif kind == "INDIV_BETA":
            out = a.indiv_beta(mode=1, packed=True)
        elif kind == "KING_HOMO":
            out = a.king_homo(packed=True)
        elif kind == "GRM_GCTA":
            out = (a.grm_gcta(packed=True),)
        elif kind == "PCA_COV":
            out = (a.pca_cov(packed=True, normalize=True)[0],)
        elif kind == "EIGMIX":
            out = (a.eigmix(diagadj=True, packed=True),)
        else:
            out = a.diss_sums()
        return out, a.get_timing(0)[1], a.get_timing(1)[1], a.syrk_launches()


_default_runs = {}


def _default_run(kind, n, rows):
    """the default path's result on the same data (environment cleared by the caller), once per (kind, n, rows)"""
    key = (kind, n, rows)
    if key not in _default_runs:
        _default_runs[key] = _run(kind, n, rows)[0]
    return _default_runs[key]


def _slab(ref, n, rows):
    from snprelate_amd.dist import slab_range
    if not rows:
        return ref
    lo, hi = slab_range(n, rows[0], rows[1])
    return ref[lo:hi]


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(K.SWITCH_SPACE) + list(K.GEOMETRY_SWITCHES) + ["SNPGPU_RUN_INNER", "SNPGPU_PREP_TWO_PASS"]:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("c", K.CASES, ids=[K.case_id(c) for c in K.CASES])
def test_kernel_path(c, clean_env):
    from snprelate_amd import _lib
    kind, n, rows = c["kind"], c["n"], c["rows"]
    default = _default_run(kind, n, rows) if c["compare"] != K.REFUSAL else None       # (under the cleared environment)
    default_sig = K.signature(kind, None, n, rows)
    for name, value in c["env"].items():
        clean_env.setenv(name, value)
    # ---- proof of path, 1: the live plan is the case's
    sig = K.signature(kind, None, n, rows)
    assert sig == K.case_signature(c)
    if c["compare"] == K.REFUSAL:
        assert sig == (kind, K.REFUSED)
        with pytest.raises(_lib.SnpGpuError, match="snpgpu_create: the dissimilarity kind needs the MX-fp4 counter kernels"):
            _lib.Accumulator(getattr(_lib, kind), n)
        return
    out, spans_counter, spans_syrk, launches = _run(kind, n, rows)
    # ---- 2: spans of each family the signature names, none for a family it names `none` (one span per feed for the counters, one
    # per table and feed for the SYRK family); SYRK kernel launches exactly where it names a SYRK kernel
    names_counter = any(k != "none" for k in K.counter_kernels(sig))
    names_syrk = any(k != "none" for k in K.syrk_kernels(sig))
    assert (spans_counter >= 1) == names_counter and (spans_syrk >= 1) == names_syrk, (spans_counter, spans_syrk, sig)
    assert spans_counter == (len(FEEDS) if names_counter else 0)
    assert (launches >= len(FEEDS)) == names_syrk and (launches > 0) == names_syrk, (launches, sig)
    # ---- comparison with the oracle, in the class of the kernel family
    ref = tuple(_slab(r, n, rows) if isinstance(r, np.ndarray) and r.ndim >= 1 and r.shape[0] == n * (n + 1) // 2 else r
                for r in _reference(kind, n))
    figures = {}
    if c["compare"] == K.EXACT:
        if kind == "INDIV_BETA":                 # (the finaliser of the exact counters: test_beta_mom_eigmix_synthetic's class)
            np.testing.assert_allclose(out[0], ref[0], rtol=1e-10, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(out[1], ref[1], rtol=1e-11)
        else:
            assert np.array_equal(out[0], ref[0])
        for o, d in zip(out, default):           # ... and the default path's bits
            assert np.array_equal(o, d, equal_nan=True)
        figures["bit_exact"] = True
    elif c["compare"] == K.REL_1E5:
        fin = np.isfinite(ref[0])
        assert np.array_equal(np.isfinite(out[0]), fin) and np.array_equal(np.isnan(out[0]), np.isnan(ref[0]))
        figures["contract"], figures["offdiag"] = _figures(out[0], ref[0], n) if not rows else \
            _panel_figures(out[0], ref[0], _reference(kind, n)[0], n)
        print("%s: contract %.2e offdiag %.2e (bound 1e-5)" % (K.case_id(c), figures["contract"], figures["offdiag"]), flush=True)
        assert max(figures.values()) < 1e-5, figures
    elif c["compare"] == K.KING_HOMO_TOL:
        for o, r in zip(out, ref):
            assert np.array_equal(np.isnan(o), np.isnan(r)) and np.array_equal(np.isfinite(o), np.isfinite(r))
        e0 = np.nanmax(np.abs(out[0] - ref[0]) / (1e-7 + 1e-5 * np.abs(ref[0])))
        e1 = np.nanmax(np.abs(out[1] - ref[1]) / (2e-5 + 1e-5 * np.abs(ref[1])))
        print("%s: k0 %.3f k1 %.3f of the tolerance of test_king_homo" % (K.case_id(c), e0, e1), flush=True)
        np.testing.assert_allclose(out[0], ref[0], rtol=1e-5, atol=1e-7, equal_nan=True)
        np.testing.assert_allclose(out[1], ref[1], rtol=1e-5, atol=2e-5, equal_nan=True)
    else:
        assert c["compare"] == K.DISS_TOL
        assert np.array_equal(out[0].astype(np.int64), ref[0])
        e = np.max(np.abs(out[1] - ref[1]) / (1e-9 + 2e-6 * np.abs(ref[1])))
        print("%s: SumAFreq %.3f of the tolerance of test_sum_geno_bit_exact" % (K.case_id(c), e), flush=True)
        np.testing.assert_allclose(out[1], ref[1], rtol=2e-6, atol=1e-9)
    # ---- proof of path, 3: a SYRK kernel of another arithmetic than the default path's leaves other bits than the default path
    # (counter kernels are exact by design: for them the plan and the spans are the proof)
    arithmetic = tuple(K.SYRK_ARITHMETIC[k] for k in K.syrk_kernels(sig))
    if arithmetic != tuple(K.SYRK_ARITHMETIC[k] for k in K.syrk_kernels(default_sig)):
        diff = max(float(np.nanmax(np.abs(np.asarray(o, np.float64) - np.asarray(d, np.float64)))) for o, d in zip(out, default))
        assert diff > 0, "the result equals the default path's bit for bit: did %s run?" % (K.syrk_kernels(sig),)


def _panel_figures(got, ref_slab, ref_full, n):
    """the figures of a row panel's slab, with the diagonal scale and the off-diagonal floor of the WHOLE matrix (a slab has its own
    median; the bound was stated for the matrix)"""
    from norms import tri_diag_scale
    fin = np.isfinite(ref_slab)
    d = np.abs(got[fin] - ref_slab[fin])
    a = np.abs(ref_slab[fin])
    med = float(np.median(np.abs(ref_full[np.isfinite(ref_full)])))
    return float(np.max(d / (a + tri_diag_scale(ref_full, n)))), float(np.max(d / (a + med)))


# ---- switches that change geometry or launches, never a kernel name -------------------------------------------------------------------

def _grm(g, n, block, kind="GRM_GCTA", rows=None):
    """one context fed `g` in blocks of `block` SNPs: (packed result, SYRK spans, SYRK kernel launches)"""
    from snprelate_amd import _lib
    kw = dict(row_begin=rows[0], row_end=rows[1]) if rows else {}
    with _lib.Accumulator(getattr(_lib, kind), n, max_block_snps=block, **kw) as a:
        a.set_timing(True)
        for i in range(0, g.shape[0], block):
            a.feed(g[i:i + block])
        if kind == "GRM_GCTA":
            out = a.grm_gcta(packed=True)
        elif kind == "PCA_COV":
            out = a.pca_cov(packed=True, normalize=False)[0]
        else:
            out = a.king_homo(packed=True)
        return out, a.get_timing(1)[1], a.syrk_launches()


# SNPGPU_RUN_INNER is read once per process (syrk_device.h): every value runs in a process of its own.  The worker feeds the block
# under each of the three environments and leaves the results and the launch counts in a file.
RUN_INNER_VALUES = ("unset", "0", "1", "4")
RUN_INNER_FORMS = {
    "exact_row_missing": (0.02, {}),                                    # syrk_x1_kernel on a block with missing calls
    "lookup32_nomiss": (0.0, {"SNPGPU_SYRK_UV16": "0"}),                # syrk_uv_kernel as (tile, run) items
    "lookup16_nomiss": (0.0, {"SNPGPU_SYRK_UV16": "1"}),                # syrk_uv16_kernel as (tile, run) items
}
RUN_INNER_N, RUN_INNER_L, RUN_INNER_PROMOTE = 700, 4096 + 640, 1024      # the shape of test_grm_several_fp32_runs_per_block
_WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from oracle.synth import synth_geno
from snprelate_amd import _lib
forms, n, L, out = json.loads(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
res = {}
for name, (missing, env) in forms.items():
    for k, v in env.items():
        os.environ[k] = v
    g = synth_geno(n, L, missing=missing, seed=77)
    with _lib.Accumulator(_lib.GRM_GCTA, n, max_block_snps=8192) as a:
        a.set_timing(True)
        a.feed(g)
        res[name] = a.grm_gcta(packed=True)
        res[name + "_launches"] = np.array([a.get_timing(1)[1], a.syrk_launches()])
    for k in env:
        del os.environ[k]
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def run_inner_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_inner")
    results = {}
    for value in RUN_INNER_VALUES:
        env = {k: v for k, v in os.environ.items() if k not in K.SWITCH_SPACE and k not in K.GEOMETRY_SWITCHES}
        env.pop("SNPGPU_RUN_INNER", None)
        if value != "unset":
            env["SNPGPU_RUN_INNER"] = value
        env["SNPGPU_H3_PROMOTE"] = str(RUN_INNER_PROMOTE)
        out = str(d / ("run_inner_%s.npz" % value))
        r = subprocess.run([sys.executable, "-c", _WORKER, ROOT, json.dumps(RUN_INNER_FORMS), str(RUN_INNER_N), str(RUN_INNER_L), out],
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        results[value] = dict(np.load(out))
    return results


def _expected_launches(form, fused):
    """RunLaunches::count() for the block of this test (syrk_device.h, launch_syrk_h3, launch_syrk_uv): every block enqueues the
    exact-row kernel AND the single-product kernel, the device flag lets one of them work.  Exact-row kernel: table chunks of 512 SNPs,
    runs of H3_PROMOTE / 512 chunks, each run launched as two halves where the plan allows short runs; single-product kernel: the plan's
    runs (plan_block), walked inside the work item by the default form."""
    from snprelate_amd import _lib
    missing, env = RUN_INNER_FORMS[form]
    with K.SwitchEnv(dict(env, SNPGPU_H3_PROMOTE=str(RUN_INNER_PROMOTE))):
        d = _lib.diag_plan(_lib.GRM_GCTA, RUN_INNER_N, block_snps=RUN_INNER_L, max_block_snps=8192)
    n_chunk = (int(d["n_q"]) + 31) // 32
    run = max(1, int(d["h3_promote"]) // 512)
    short_div = 2 if (d["sparse_missing"] == "1" and d["x1_short_runs"] == "1" and run >= 2 and run % 2 == 0) else 1
    n_runs = -(-n_chunk // (run // short_div))
    x1 = 1 if (fused and n_runs > 1) else -(-n_chunk // run) * short_div
    uv_runs = int(d["uv_runs"])
    inner = d["uv_form"] == "converted_carry"
    uv = 1 if (inner or uv_runs == 1 or fused) else uv_runs
    return x1 + uv, n_runs, uv_runs


@pytest.mark.parametrize("form", list(RUN_INNER_FORMS))
def test_fp32_runs_as_one_launch_or_one_launch_per_run(form, run_inner_results):
    """SNPGPU_RUN_INNER in {0, 1, 4, unset} with SNPGPU_H3_PROMOTE=1024 on a 4736-SNP block at n = 700: the fp32 runs of the block as
    one launch per run (0), or as ONE launch of (tile, run) work items whose XCD queues are walked in groups of 1, 4 or 32 tiles.  The
    launch counts of 0 and unset are those of RunLaunches::count(), the four results agree to 1e-6 (the figure
    test_grm_several_fp32_runs_per_block holds between run lengths), each is within 1e-5 of the oracle."""
    missing, _ = RUN_INNER_FORMS[form]
    g = synth_geno(RUN_INNER_N, RUN_INNER_L, missing=missing, seed=77)
    ref = orc.grm_gcta(g)
    per_run, n_runs, uv_runs = _expected_launches(form, fused=False)
    fused = _expected_launches(form, fused=True)[0]
    assert n_runs > 1 and uv_runs > 1 and per_run > fused == 2
    counts = {v: [int(x) for x in run_inner_results[v][form + "_launches"]] for v in RUN_INNER_VALUES}
    print("%s: (spans, kernel launches) %s; expected launches: one per run %d, fused %d" % (form, counts, per_run, fused), flush=True)
    for v in RUN_INNER_VALUES:
        assert counts[v] == [1, per_run if v == "0" else fused], (v, counts[v])
    outs = [run_inner_results[v][form] for v in RUN_INNER_VALUES]
    for v, o in zip(RUN_INNER_VALUES, outs):
        e = _rel_err(o, ref, RUN_INNER_N)
        print("%s SNPGPU_RUN_INNER=%s: %.2e (bound 1e-5)" % (form, v, e), flush=True)
        assert e < 1e-5 and np.array_equal(np.isfinite(o), np.isfinite(ref))
    spread = max(float(np.nanmax(np.abs(a - b))) for a in outs for b in outs)
    print("%s: largest difference between two of the four results %.2e (bound 1e-6)" % (form, spread), flush=True)
    assert spread < 1e-6


def _short_run_geno(n, L, rare, seed):
    """3 % missing calls; rare: every fourth SNP carried by 1 ... 12 samples (one or two copies each, either allele orientation):
    weights 1 / (p (1 - p)) >= 64 and at most 128 minor copies, so such SNPs take the fp64 sparse path next to missing calls and set
    the block's short-run flag; not rare: every SNP common (p in 0.05 ... 0.95), the flag stays clear"""
    g = synth_geno(n, L, missing=0.0, seed=seed, special=False)
    rng = np.random.default_rng(seed + 1)
    if rare:
        for k in range(0, L, 4):
            g[k] = 0
            g[k, rng.choice(n, size=1 + (k // 4) % 12, replace=False)] = 1 + ((k // 4) % 5 == 0)
            if (k // 4) % 3 == 0:
                g[k] = 2 - g[k]
    g[rng.random((L, n)) < 0.03] = 3
    return g


@pytest.mark.parametrize("L,rare", [(4608, True), (4608, False), (2048, True), (2048, False)],
                         ids=["9chunks-rare", "9chunks-common", "4chunks-rare", "4chunks-common"])
def test_short_run_flag_of_the_exact_row_kernel(L, rare, clean_env):
    """Blocks with missing calls AND rare variants on the fp64 sparse path run the exact-row kernel as half-length fp32 runs: a flag
    that build_lut_kernel sets on the device and syrk_x1_kernel reads.  n = 700, 3 % missing calls, default run length (8192 SNPs = 16
    table chunks of 512).  4608 SNPs = 9 chunks, 10 with the padding of the single-product tables: ONE fused launch laid out for
    half-length runs (8 + 2 chunks), of which a block with the flag clear uses the first at full length; 2048 SNPs = 4 chunks: one
    run, launched as the two halves of launch_syrk_h3.
    SNPGPU_X1_SHORT_RUNS=0: no flag, one full-length launch.  SNPGPU_X1_SPARSE_MAC = 1 / 8: fewer SNPs on the fp64 path."""
    from snprelate_amd import _lib
    n = 700
    g = _short_run_geno(n, L, rare, 300 + L)
    ref = orc.grm_gcta(g)
    scale = np.abs(ref[np.isfinite(ref)]).max()
    out, launches = {}, {}
    for short in (None, "0"):
        for mac in (None, "1", "8"):
            for name, v in (("SNPGPU_X1_SHORT_RUNS", short), ("SNPGPU_X1_SPARSE_MAC", mac)):
                clean_env.delenv(name, raising=False)
                if v is not None:
                    clean_env.setenv(name, v)
            d = _lib.diag_plan(_lib.GRM_GCTA, n, block_snps=L, max_block_snps=8192)
            assert d["sparse_missing"] == "1" and d["x1_short_runs"] == ("0" if short else "1") and d["x1_sparse_mac"] == (mac or "128")
            out[short, mac], spans, launches[short, mac] = _grm(g, n, 8192)
            assert spans == 1
            err = float(np.nanmax(np.abs(out[short, mac] - ref))) / scale
            # every rare SNP on the fp64 path (mac unset: up to 12 copies <= 128): the sparse path's bound; some or all of them left in
            # the dense product (mac 1, 8), or no rare SNP at all: the dense product's
            bound = 2e-6 if (rare and mac is None) else 2e-5
            print("L=%d rare=%s SHORT_RUNS=%s SPARSE_MAC=%s: %.2e of the scale (bound %.0e), %d kernel launches"
                  % (L, rare, short, mac, err, bound, launches[short, mac]), flush=True)
            assert err < bound and np.array_equal(np.isfinite(out[short, mac]), np.isfinite(ref))
    # the counter: exact-row launches + the single-product launch that every block enqueues.  9 chunks: the fused launch whatever the
    # flag; 4 chunks: two half launches with the flag's pointer, one without
    for mac in (None, "1", "8"):
        assert launches[None, mac] == (2 if L == 4608 else 3) and launches["0", mac] == 2, launches
    same_runs = np.array_equal(out[None, None], out["0", None])
    print("L=%d rare=%s: bits equal with and without short runs: %s" % (L, rare, same_runs), flush=True)
    if rare:
        # the flag was set and read: two fp32 runs (8 + 2 chunks, 2 + 2 chunks) round differently from one
        assert not same_runs
        # fewer SNPs on the fp64 path: other bits, in both run geometries
        for short in (None, "0"):
            assert np.abs(out[short, "1"] - out[short, None]).max() > 0 and np.abs(out[short, "8"] - out[short, None]).max() > 0
            assert np.abs(out[short, "1"] - out[short, "8"]).max() > 0


SUPER_WORKLOADS = {
    "grm_nomiss": ("GRM_GCTA", 0.0, {}),                              # x1 list: syrk_uv16c_kernel
    "grm_missing": ("GRM_GCTA", 0.04, {}),                            # x1 list: syrk_x1_kernel
    "grm_three_products": ("GRM_GCTA", 0.04, {"SNPGPU_SYRK": "h3"}),  # h3 list: syrk_h3_kernel<3, false>
    "king_homo": ("KING_HOMO", 0.04, {}),                             # (its single-product list has a fixed super-tile edge)
    "king_homo_two_products": ("KING_HOMO", 0.04, {"SNPGPU_HOMO_UV": "0"}),   # h3 list: syrk_h3_kernel<2, false>
}


@functools.lru_cache(maxsize=None)
def _super_case(n, workload):
    kind, missing, _ = SUPER_WORKLOADS[workload]
    g = synth_geno(n, 700, missing=missing, seed=n + len(workload), special=missing > 0)
    if kind == "GRM_GCTA":
        ref = (orc.grm_gcta(g),)
    else:
        c, fs = orc.king_homo_count(g)
        ref = orc.king_homo_final(c, fs, n)
    return g, ref


@pytest.mark.parametrize("workload", list(SUPER_WORKLOADS))
@pytest.mark.parametrize("n", [1300, 1030])
@pytest.mark.parametrize("edge", ["1", "3", "32"])
def test_super_tile_edges(edge, n, workload, clean_env):
    """SNPGPU_H3_SUPER and SNPGPU_X1_SUPER: the super-tile edge of the two SYRK work lists.  n = 1300: six 256-tiles (3 divides that,
    32 exceeds it); n = 1030: five (3 does not divide it).  Every tile must still be visited exactly once: against the oracle in the
    class of the kernel family.  (The pair counters' lists have a fixed edge: no counter kind depends on these switches.)"""
    from snprelate_amd import _lib
    kind, missing, env = SUPER_WORKLOADS[workload]
    g, ref = _super_case(n, workload)
    for name, value in dict(env, SNPGPU_H3_SUPER=edge, SNPGPU_X1_SUPER=edge).items():
        clean_env.setenv(name, value)
    d = _lib.diag_plan(getattr(_lib, kind), n)
    assert d["h3_super"] == edge and d["x1_super"] == edge                     # the plan the context is created from
    out, spans, launches = _grm(g, n, 512, kind)
    assert spans >= 2 and launches >= 2
    if kind == "GRM_GCTA":
        assert np.array_equal(np.isfinite(out), np.isfinite(ref[0]))
        e = _rel_err(out, ref[0], n)
        print("%s n=%d super=%s: %.2e (bound 1e-5)" % (workload, n, edge, e), flush=True)
        assert e < 1e-5
    else:
        np.testing.assert_allclose(out[0], ref[0], rtol=1e-5, atol=1e-7, equal_nan=True)
        np.testing.assert_allclose(out[1], ref[1], rtol=1e-5, atol=2e-5, equal_nan=True)


@pytest.mark.parametrize("missing", [0.0, 0.03])
def test_one_run_one_weight_target(missing, clean_env):
    """SNPGPU_SYRK_FAST=1 (bench.py's grm_fast leg): one 32 768-SNP fp32 run per flush and ONE weight target for the single-product
    kernel.  ctx_plan.h states its price as 1.6e-5 instead of 1e-5 in the off-diagonal figure at full size; the contract figure
    (tests/norms.py) holds at 1e-5, and so does the off-diagonal figure at this size, where SNPGPU_UV_TARGETS=0 -- the same single
    target -- is held to it by test_grm_weight_targets_per_fp32_run."""
    from snprelate_amd import _lib
    n, L = 700, 5000
    g = synth_geno(n, L, missing=missing, seed=61)
    ref = orc.grm_gcta(g)
    d0 = _lib.diag_plan(_lib.GRM_GCTA, n, block_snps=L, max_block_snps=8192)
    clean_env.setenv("SNPGPU_SYRK_FAST", "1")
    d = _lib.diag_plan(_lib.GRM_GCTA, n, block_snps=L, max_block_snps=8192)
    assert (d0["h3_promote"], d0["uv_promote"], d0["uv_targets"], d0["uv_q"]) == ("8192", "11264", "1", "2")
    assert (d["h3_promote"], d["uv_promote"], d["uv_targets"], d["uv_q"], d["uv_runs"]) == ("32768", "32768", "0", "1", "1")
    out, spans, launches = _grm(g, n, 8192)
    contract, offdiag = _figures(out, ref, n)
    print("SNPGPU_SYRK_FAST=1 missing=%g: contract %.2e offdiag %.2e (bound 1e-5)" % (missing, contract, offdiag), flush=True)
    assert contract < 1e-5 and offdiag < 1e-5 and np.array_equal(np.isfinite(out), np.isfinite(ref))
