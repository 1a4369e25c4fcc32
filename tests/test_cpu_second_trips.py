"""CPU side of tests/test_gpu_second_trips.py: the vectorised restatement its tree case is held to, pinned to the loop over merges,
and the counters it reads declared, exported and bound."""
import os

import numpy as np

import mem_kinds as M
import tree_ref as T
from snprelate_amd import _lib
from test_gpu_tree import caterpillar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_counters():
    text = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    protos = M.header_prototypes(text)
    for f in ("snpgpu_grm_merge_stats", "snpgpu_pop_stats", "snpgpu_tree_stats", "snpgpu_ld_get_timing"):
        assert f in protos and f in _lib.EXPORTS and hasattr(_lib.lib(), f)
    assert protos["snpgpu_grm_merge_stats"] == ["stats"] and _lib.lib().snpgpu_grm_merge_stats(None) != 0
    assert set(_lib.grm_merge_stats()) == {"slabs", "launches"}
    assert len(_lib.pop_stats()) == 5                      # the W&H02 launches are the slot appended at the end


def test_caterpillar_obs_is_dist_perm_counter():
    n = 300
    rng = np.random.default_rng(31)
    d = np.triu(rng.uniform(0.1, 0.9, (n, n)), 1)
    d = d + d.T
    merge = caterpillar(n, 32)
    ref = T.dist_perm_counter(d, merge, 2, 15.0, 1)
    n1, n2, obs = T.caterpillar_obs(d, merge)
    assert np.array_equal(n1, ref["n1"]) and np.array_equal(n2, ref["n2"])
    # two orders of the same at most n additions
    assert np.all(np.abs(obs - ref["obs"]) <= 4.0 * n * 2.0 ** -53 * np.abs(ref["obs"]))
    assert obs[0] == d[tuple(-merge[0] - 1)]
    # not symmetric: the rows are the joining sample's, as the loop reads them
    d2 = rng.uniform(0.1, 0.9, (n, n))
    ref2 = T.dist_perm_counter(d2, merge, 2, 15.0, 1)
    assert np.all(np.abs(T.caterpillar_obs(d2, merge)[2] - ref2["obs"]) <= 4.0 * n * 2.0 ** -53 * np.abs(ref2["obs"]))
