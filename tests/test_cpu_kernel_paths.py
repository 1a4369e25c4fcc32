"""tests/kernel_paths.py against the library and the sources, without a GPU: every switch that Switches::from_env reads is in a table,
every environment variable the native code reads names the GPU test that sets it, every reachable kernel path has a case and every
case gives the path it claims, and no value of the two parity fixtures is a second name for another value's path."""
import ast
import glob
import os
import re

import pytest

import kernel_paths as K
from conftest import ROOT

CSRC = os.path.join(ROOT, "snprelate_amd", "csrc")
PLAN_HEADER = os.path.join(CSRC, "ctx_plan.h")
TESTS = os.path.join(ROOT, "tests")


def _from_env_names(text):
    """the SNPGPU_* names inside the body of Switches::from_env"""
    lo = text.index("static Switches from_env()")
    hi = text.index("return s;", lo)
    return re.findall(r'"(SNPGPU_[A-Z0-9_]+)"', text[lo:hi])


def _source_names():
    """every "SNPGPU_*" string literal under snprelate_amd/csrc: what getenv, the env_* helpers, RowBlocks::open and env_bytes are given"""
    names = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        with open(path, errors="replace") as f:
            for name in re.findall(r'"(SNPGPU_[A-Z0-9_]+)"', f.read()):
                names.setdefault(name, os.path.basename(path))
    return names


def _functions(path):
    """top-level function name -> its source text"""
    src = open(path).read()
    return {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}, src


def test_parsers_on_known_text():
    names = _from_env_names(open(PLAN_HEADER).read())
    assert "SNPGPU_PAIR_BACKEND" in names and "SNPGPU_I8_TAIL_PARTS" in names and len(names) == len(set(names)) >= 27
    src = _source_names()
    assert src["SNPGPU_RUN_INNER"] == "syrk_device.h" and src["SNPGPU_PCR_BLOCK_SNPS"] == "pcrelate.hip" and src["SNPGPU_EIG_FP32"] == "eigen.hip"
    assert set(names) <= set(src)


def test_every_switch_of_the_plan_is_in_a_table():
    names = set(_from_env_names(open(PLAN_HEADER).read()))
    known = set(K.SWITCH_SPACE) | set(K.GEOMETRY_SWITCHES)
    assert not names - known, "read by Switches::from_env, neither in SWITCH_SPACE nor in GEOMETRY_SWITCHES: %s" % sorted(names - known)
    assert not known - names, "in a table of tests/kernel_paths.py, not read by Switches::from_env: %s" % sorted(known - names)
    assert not set(K.SWITCH_SPACE) & set(K.GEOMETRY_SWITCHES)
    for name, values in K.SWITCH_SPACE.items():
        assert values[0] is None and len(values) == len(set(values)) >= 2, name      # unset is always one of the values


def test_every_environment_variable_of_the_sources_names_its_gpu_test():
    src = _source_names()
    assert len(src) >= 50
    missing = sorted(n for n in src if n not in K.SWITCH_TESTS and n not in K.EXEMPT)
    assert not missing, "environment variables read under snprelate_amd/csrc without a GPU test in SWITCH_TESTS (or a reason in EXEMPT): %s" \
        % ", ".join("%s (%s)" % (n, src[n]) for n in missing)
    stale = sorted(n for n in list(K.SWITCH_TESTS) + list(K.EXEMPT) if n not in src)
    assert not stale, "in SWITCH_TESTS / EXEMPT, read nowhere under snprelate_amd/csrc: %s" % stale
    assert not set(K.SWITCH_TESTS) & set(K.EXEMPT)
    assert all(len(reason) > 20 for reason in K.EXEMPT.values()) and len(K.EXEMPT) <= 3


def test_every_named_test_exists_is_a_gpu_test_and_sets_its_variable():
    in_cases = {name for c in K.CASES for name in c["env"]}
    parsed = {}
    for name, (fname, func) in K.SWITCH_TESTS.items():
        assert fname.startswith("test_gpu_"), (name, fname)
        path = os.path.join(TESTS, fname)
        assert os.path.exists(path), "%s: %s does not exist" % (name, fname)
        if fname not in parsed:
            parsed[fname] = _functions(path)
        funcs, text = parsed[fname]
        assert "pytest.mark.gpu" in text, "%s holds no GPU test" % fname
        assert func in funcs, "%s: %s has no function %s" % (name, fname, func)
        if (fname, func) == K.GPU_TEST and name in K.SWITCH_SPACE:
            # set from the cases' environments: the variable must be in one, and the test must read the cases
            assert name in in_cases, "%s is in no environment of CASES" % name
            assert "CASES" in text and 'c["env"]' in funcs[func]
        else:
            assert re.search(r"\b%s\b" % name, funcs[func]), "%s is not named in %s::%s" % (name, fname, func)


def test_cases_are_the_reachable_signatures():
    reach = K.reachable()
    assert len(reach) >= 100 and sum(1 for s in reach if s[1] == K.REFUSED) == 1
    by_sig = {}
    for c in K.CASES:
        by_sig.setdefault(K.case_signature(c), []).append(c)
    lacking = reach - set(by_sig)
    assert not lacking, "%d reachable signatures without a case, the first: %s (from %s)" % (
        len(lacking), sorted(lacking, key=str)[0], K._enumerate()[sorted(lacking, key=str)[0]])
    extra = set(by_sig) - reach
    assert not extra, "cases whose signature is not reachable over SWITCH_SPACE: %s" % [K.case_id(by_sig[s][0]) for s in extra]
    # one case per signature, beside the row panels; a panel case adds no signature of its own
    for sig, cs in by_sig.items():
        full = [c for c in cs if not c["rows"]]
        assert len(full) == 1, "signature %s has %d full-context cases: %s" % (sig, len(full), [K.case_id(c) for c in cs])
    ids = [K.case_id(c) for c in K.CASES]
    assert len(ids) == len(set(ids))


def test_cases_hold_the_smallest_environment_and_the_right_size():
    first = K._enumerate()
    for c in K.CASES:
        if c["rows"]:
            continue
        sig = K.case_signature(c)
        env, n, _ = first[sig]
        assert len(c["env"]) == len(env), "%s: %s produces the same signature" % (K.case_id(c), env)
        for name, value in c["env"].items():
            assert value in K.SWITCH_SPACE[name], (K.case_id(c), name, value)
        if c["kind"] in K.COUNTER_KINDS:
            assert c["n"] == K.N_COUNTER
        else:
            assert c["n"] == n, "%s: the signature is first met at n = %d" % (K.case_id(c), n)     # N_SMALL only where it exists only there
        assert c["compare"] == (K.REFUSAL if sig[1] == K.REFUSED else K.COMPARE[c["kind"]])
        assert c["test"] == K.GPU_TEST


def test_one_row_panel_per_pair_of_syrk_kernels():
    names = {k for s in K.reachable() for k in K.syrk_kernels(s)} - {"none"}
    assert names == set(K.SYRK_ARITHMETIC) - {"none"}
    pairs = {K.syrk_kernels(s) for s in K.reachable() if s[1] != K.REFUSED} - {("none", "none")}
    covered = [K.syrk_kernels(K.case_signature(c)) for c in K.PANEL_CASES]
    assert not pairs - set(covered), "pairs of SYRK kernels (block without, with missing calls) without a row-panel case: %s" % sorted(pairs - set(covered))
    assert len(covered) == len(set(covered)) == len(pairs) >= 14                 # one panel each: none can go unnoticed
    assert {k for p in covered for k in p} - {"none"} == names
    assert all(c["rows"] == K.PANEL_ROWS and c["n"] == K.N_LARGE for c in K.PANEL_CASES)
    assert K.CASES[-len(K.PANEL_CASES):] == K.PANEL_CASES and not any(c["rows"] for c in K.CASES[:-len(K.PANEL_CASES)])


def test_signature_tells_sizes_and_refusals():
    d = K.signature("GRM_GCTA", {}, K.N_LARGE)
    assert d[:5] == ("GRM_GCTA", "none", "pair_mfma_fp4_miss_kernel", "syrk_uv16c_kernel", "syrk_x1_kernel")
    assert d != K.signature("GRM_GCTA", {}, K.N_SMALL)                       # sparse_missing needs X1_SPARSE_MIN_N = 384 samples
    assert d == K.signature("GRM_GCTA", {}, K.N_LARGE, K.PANEL_ROWS)
    assert K.signature("DISS", {"SNPGPU_PAIR_FP4": "0"}, K.N_LARGE) == ("DISS", K.REFUSED)
    assert K.signature("IBS", {}, 279)[5:] == (None,) * (len(K.PLAN_FIELDS) - 1) + ("0",)      # no SYRK table; gcta_sparse is a counter field


def test_signature_leaves_the_environment_as_it_was(monkeypatch):
    monkeypatch.setenv("SNPGPU_SYRK", "h3")
    monkeypatch.delenv("SNPGPU_SYRK_UV16", raising=False)
    a = K.signature("GRM_GCTA", {"SNPGPU_SYRK_UV16": "0"}, K.N_LARGE)
    assert os.environ["SNPGPU_SYRK"] == "h3" and "SNPGPU_SYRK_UV16" not in os.environ
    assert a[3] == "syrk_uv_kernel"                                                  # the given environment alone counted ...
    assert K.signature("GRM_GCTA", None, K.N_LARGE)[3] == "syrk_h3_kernel<3, false>"      # ... and env=None is the live one


@pytest.mark.parametrize("envs,default,kinds", [(K.PAIR_BACKEND_ENVS, K.PAIR_BACKEND_DEFAULT, K.PAIR_BACKEND_KINDS),
                                                (K.SYRK_BACKEND_ENVS, K.SYRK_BACKEND_DEFAULT, K.SYRK_BACKEND_KINDS)],
                         ids=["pair_backend", "syrk_backend"])
def test_no_fixture_value_of_the_parity_suite_is_idle(envs, default, kinds):
    """every value of a fixture selects, for at least one kind that uses it, a path that no other value of the fixture selects; the
    default is the one value that may set nothing -- and it must"""
    assert envs[default] == {}
    sigs = {v: {k: K.signature(k, env, K.N_LARGE) for k in kinds} for v, env in envs.items()}
    for v, env in envs.items():
        if v != default:
            assert env, "%s sets nothing, as the default does" % v
        for name, value in env.items():
            assert value in K.SWITCH_SPACE[name], "%s: %s=%s is not a value the plan tells from unset" % (v, name, value)
        for w in envs:
            if w != v:
                assert any(sigs[v][k] != sigs[w][k] for k in kinds), "fixture values %s and %s select the same paths for %s" % (v, w, kinds)
    # the fixtures read this table, not a copy of it
    funcs, _ = _functions(os.path.join(TESTS, "test_gpu_parity.py"))
    assert "PAIR_BACKEND_ENVS[request.param]" in funcs["pair_backend"] and "SYRK_BACKEND_ENVS[request.param]" in funcs["syrk_backend"]
    assert "setenv(\"SNPGPU" not in funcs["pair_backend"] + funcs["syrk_backend"]
