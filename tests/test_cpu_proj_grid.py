"""The launch geometry of the PCA projection kernels (csrc/proj_grid.h) at every shape of tests/test_gpu_proj_shapes.py, and the
extended-precision references of tests/proj_ref.py against the oracle's restatements of the same formulas.  No GPU is touched."""
import os
import subprocess

import numpy as np
import pytest

import oracle as orc
import proj_cases as pc
import proj_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = pc.SNP_CASES + pc.SAMP_CASES


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """tests/proj_grid_check.cpp includes only proj_grid.h; built with the host compiler under the address and undefined-behaviour
    sanitizers and run as a process of its own on the whole case table: {case name: (gx, gy, split, per)}"""
    exe = str(tmp_path_factory.mktemp("proj_grid") / "proj_grid_check")
    r = subprocess.run(["g++", "-std=gnu++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "snprelate_amd", "csrc"), os.path.join(ROOT, "tests", "proj_grid_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    text = "".join("%s %d %d %d\n" % (c.side, c.N, c.n_snp, c.k) for c in ALL_CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(ALL_CASES)
    out = {}
    for c, line in zip(ALL_CASES, lines):
        w = line.split()
        assert w[:4] == [c.side, str(c.N), str(c.n_snp), str(c.k)], line
        out[c.name] = tuple(int(x) for x in w[4:])
    r = subprocess.run([exe], input="snp 10 x 3\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "bad input line" in r.stderr       # (a line it cannot read is not skipped)
    return out


def test_the_table_is_the_issue_s():
    assert len({c.name for c in ALL_CASES}) == len(ALL_CASES) == 11 + 16 + 1 + 9 + 7 + 12 + 1 + 8
    assert sorted({c.k for c in pc.A}) == [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64]
    assert [c.N for c in pc.B] == [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 511, 512, 513, 1030]
    assert [c.n_snp for c in pc.D] == [1, 63, 64, 65, 255, 256, 257, 1023, 1024] and all(c.bmax == 1024 for c in pc.D)
    assert [c.k for c in pc.E] == [1, 15, 16, 17, 32, 33, 64]
    assert [c.n_snp for c in pc.F] == [1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 129, 4097] and all(c.bmax == 8192 for c in pc.F)
    assert [c.N for c in pc.H] == [1, 63, 64, 65, 255, 256, 257, 1030]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_case_reaches_its_geometry(geometry, case):
    f = pc.facts(case, *geometry[case.name])
    assert case.want and {k: f[k] for k in case.want} == case.want
    # what the kernels rely on at any shape: parts that tile the range without an empty one, SNP-side parts that begin on a multiple
    # of 8 (16-byte loads of 4 samples' words), a grid within the launch limits, every output row and column inside it
    red = f["n4"] if case.side == "snp" else case.n_snp
    parts = f["parts"]
    assert parts[0][0] == 0 and parts[-1][1] == red and all(a < b for a, b in parts)
    assert all(parts[i][1] == parts[i + 1][0] for i in range(len(parts) - 1))
    if case.side == "snp":
        assert f["per"] % 8 == 0 and f["per"] >= 256 and f["gx"] * 256 >= case.n_snp and f["gy"] * 8 >= case.k
    else:
        assert f["per"] >= 64 and f["gx"] * 256 >= case.N and f["gy"] * 16 >= case.k
    assert 1 <= f["split"] <= 64 and f["gy"] <= 65535 and 0 <= f["idle"] <= 3 and 1 <= f["fill"] <= 64


def test_the_cases_cover_what_they_are_named_for(geometry):
    """across the table: every geometry the kernels treat differently is reached by some case"""
    fs = {c.name: pc.facts(c, *geometry[c.name]) for c in ALL_CASES}
    snp = [fs[c.name] for c in pc.SNP_CASES]
    samp = [fs[c.name] for c in pc.SAMP_CASES]
    assert {f["gy"] for f in snp} >= {1, 2, 3, 4, 5, 8} and {f["gy"] for f in samp} == {1, 2, 3, 4}
    assert any(f["per"] > 256 and f["last"] < f["per"] for f in snp)                  # per not clamped, the last part short
    assert any(f["split"] >= 2 and f["last"] == 4 for f in snp)                        # a last part of one 4-sample step
    assert any(f["n4"] > c.N for c, f in zip(pc.SNP_CASES, snp)) and any(c.N < 4 for c in pc.SNP_CASES)
    assert any(f["fill"] < 64 and f["idle"] == 0 for f in snp) and any(f["idle"] > 0 for f in snp) and any(f["gx"] > 1 for f in snp)
    assert any(f["cols"] < 8 for f in snp) and any(f["cols"] == 8 and f["gy"] > 1 for f in snp)
    assert any(f["off4"] for f in samp) and any(f["tail_only"] and f["split"] > 1 for f in samp)
    assert any(f["split"] == 1 and f["last"] < 4 for f in samp) and any(f["last"] % 4 and f["last"] > 4 for f in samp)
    assert {f["kp_eq_k"] for f in samp} == {True, False} and any(f["kp_eq_k"] and f["gy"] > 1 for f in samp)
    assert any(f["gx"] > 64 for f in samp) and any(f["idle"] for f in samp)
    # the staging tests: more than one workgroup, pass and part on the SNP side
    f = pc.facts(pc.Case("snp", "stage", pc.STAGE_N, pc.STAGE_L, pc.STAGE_K, 1024, {}), 3, 2, 2, 256)
    assert (f["fill"], f["idle"], f["last"]) == (1, 3, 80)


@pytest.mark.parametrize("N,L,k", [(37, 50, 3), (333, 200, 11)])
def test_references_agree_with_the_oracle(N, L, k):
    """proj_ref restates in long double what oracle/__init__.py computes in double: 1e-12 relative to the largest entry"""
    g, ev, sload = pc.inputs(N, L, k)
    w = pc.eigenvalues(k)

    def same(got, ref):
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    for bayes in (False, True):
        load, avg, scale = pr.pca_snp_loading_like_oracle(g, w, ev, pc.TRACE, bayes)
        rl, ra, rs = orc.pca_snp_loading(g, w, ev, pc.TRACE, bayesian=bayes)
        same(load, rl)
        np.testing.assert_allclose(avg, ra, rtol=1e-14)
        np.testing.assert_allclose(scale, rs, rtol=1e-14)
    got, bound = pr.samp_loading(g, sload, ra, rs)
    same(got, orc.pca_samp_loading(g, sload, ra, rs))
    assert bound.shape == got.shape == (k, N) and (bound >= 0).all()
    valid = g < 3
    af = np.where(valid.any(axis=1), np.where(valid, g, 0).sum(axis=1) / np.maximum(2 * valid.sum(axis=1), 1), 0.5)
    same(pr.eigmix_snp_loading_like_oracle(g, w, ev, af), orc.eigmix_snp_loading(g, w, ev, af))
    same(pr.eigmix_samp_loading_like_oracle(g, sload, af), orc.eigmix_samp_loading(g, sload, af))


def test_bound_and_fallback():
    """the bound is the stated one, a double-precision loop lies far inside it, and the route for a platform whose long double is a
    double (exact products, math.fsum) gives the same numbers"""
    N, L, k = 333, 40, 5
    g, ev, sload = pc.inputs(N, L, k)
    load, avg, scale, bound = pr.snp_loading(g, ev)
    y = np.where(g < 3, (g - avg[:, None]) * scale[:, None], 0.0)
    np.testing.assert_allclose(bound, (N + 8) * 2.0 ** -53 * (np.abs(y) @ np.abs(ev).T), rtol=1e-12)
    plain = np.zeros((L, k))
    for i in range(N):
        plain += y[:, i:i + 1] * ev[None, :, i]
    assert (np.abs(plain - load) <= 0.25 * bound).all() and (bound[7] == 0).all() and (load[7] == 0).all()
    if pr.EXTENDED:
        alt = pr.snp_loading(g, ev, extended=False)
        assert (np.abs(alt[0] - load) <= 8 * 2.0 ** -53 * (np.abs(y) @ np.abs(ev).T)).all()
        np.testing.assert_allclose(alt[3], bound, rtol=1e-12)
        a2, b2 = pr.samp_loading(g, sload, avg, scale, extended=False)
        a1, b1 = pr.samp_loading(g, sload, avg, scale)
        assert (np.abs(a2 - a1) <= 8 * 2.0 ** -53 * (np.abs(y).T @ np.abs(sload)).T).all()


def test_corr_margin_names_the_degenerate_entries():
    g, ev, _ = pc.inputs(333, 200, 11)
    degenerate, margin = pr.corr_margin(g, ev)
    ref = orc.pca_snp_corr(g, ev)
    assert np.array_equal(np.isnan(ref), degenerate)
    assert degenerate[[3, 5, 7, 11, 13]].all() and degenerate[:, 3].all() and not degenerate[9, [0, 1, 2, 4]].any()
    assert margin.min() >= 1e-6
