"""CPU restatement of LD pruning for the tests (snpgdsLDpruning, R/LD.R:100-243 -> gnrLDpruning, src/genLD.cpp:1014-1035).

prune() transcribes Perform_LD_Pruning (src/genLD.cpp:807-924) loop by loop: a list of kept SNPs with erase, the forward pass
from the start SNP, the backward pass's initial list with its `break`, push_front in the backward pass, and the test
fabs(_CalcLD(kept, candidate)) > threshold that stops testing once it fired.  LD values come from a callback, so the same loop runs
on numpy values (tests/ld_ref.py), on device tables, or on the device's threshold bits.  Test infrastructure only: nothing in
snprelate_amd imports it."""
import math

import numpy as np

import ld_ref

INT_MAX = 2 ** 31 - 1
NA_INTEGER = -2 ** 31


def as_integer(x):
    """Rf_asInteger of an R numeric scalar: NA / NaN / out of int range -> NA_integer_ (INT_MIN, with R's coercion warning),
    otherwise truncated toward zero"""
    if x is None:
        return NA_INTEGER
    x = float(x)
    if math.isnan(x) or x >= INT_MAX + 1.0 or x <= NA_INTEGER:
        return NA_INTEGER
    return int(x)


class PruneResult:
    def __init__(self, keep, margin, tests, max_dist):
        self.keep = keep              # bool [M]
        self.margin = margin          # smallest | |LD| - threshold | over the non-NaN tests made (inf: none)
        self.tests = tests            # number of LD evaluations
        self.max_dist = max_dist      # largest |i - j| of a tested pair (0: none)


def prune(M, start, pos, slide_max_bp, slide_max_n, threshold, ld):
    """Perform_LD_Pruning(StartIdx = start (0-based), pos_bp, slide_max_bp, slide_max_n, LD_threshold) on M SNPs.
    ld(j, i): LD value with j (the kept SNP) as the first argument.  Position differences are exact integers."""
    pos = [int(p) for p in pos]
    out = [False] * M
    st = {"margin": math.inf, "tests": 0, "dist": 0}

    def in_window(i, j):
        return abs(i - j) <= slide_max_n and abs(pos[i] - pos[j]) <= slide_max_bp

    def test(j, i, to_include):
        # CThreadPoolLD::TestLD with one thread: no evaluation once the SNP is excluded
        if not to_include:
            return False
        v = float(ld(j, i))
        st["tests"] += 1
        st["dist"] = max(st["dist"], abs(i - j))
        if not math.isnan(v):
            st["margin"] = min(st["margin"], abs(abs(v) - threshold))
        return not (math.fabs(v) > threshold)

    def scan(lst, i):
        to_include = True
        k = 0
        while k < len(lst):
            j = lst[k]
            if in_window(i, j):
                to_include = test(j, i, to_include)
                k += 1
            else:
                del lst[k]                 # ListGeno.erase
        return to_include

    # increasing searching: i --> i + 1
    out[start] = True
    lst = [start]
    for i in range(start + 1, M):
        out[i] = scan(lst, i)
        if out[i]:
            lst.append(i)
    # decreasing searching: i --> i - 1
    lst = []
    for i in range(start, M):
        if out[i]:
            if in_window(i, start):
                lst.append(i)
            else:
                break
    for i in range(start - 1, -1, -1):
        out[i] = scan(lst, i)
        if out[i]:
            lst.insert(0, i)               # push_front
    return PruneResult(np.array(out, bool), st["margin"], st["tests"], st["dist"])


def ld_from_geno(g, method, width=None):
    """ld(j, i) callback over uint8 genotype rows g [M][N] for prune(): every ordered pair (width None), or the pairs with
    |i - j| <= width in both orientations.  Values by tests/ld_ref.py from int64 tables."""
    g = np.asarray(g)
    M = g.shape[0]
    if width is None or width >= M - 1:
        v = ld_ref.ld_values(ld_ref.tables(g), method)          # v[j, i]: j first
        return lambda j, i: v[j, i]
    return ld_from_band(band_tables(g, width), method)


def band_tables(g, width):
    """int64 [M][width][3][3]: tables of the pairs (x, x + k), k = 1 ... width (first SNP x); zero past the last SNP"""
    g = np.asarray(g)
    M = g.shape[0]
    pc = [(g == a).astype(np.int64) for a in range(3)]
    t = np.zeros((M, width, 3, 3), np.int64)
    for k in range(1, width + 1):
        x = np.arange(0, M - k)
        for a in range(3):
            for b in range(3):
                t[x, k - 1, a, b] = (pc[a][x] * pc[b][x + k]).sum(1)
    return t


def ld_from_band(t, method):
    """ld(j, i) callback from band tables [M][W][3][3] (e.g. snpgpu_ld_pair_tables rearranged, or band_tables())"""
    fwd = ld_ref.ld_values(t, method)                          # first = x
    bwd = ld_ref.ld_values(np.swapaxes(t, -1, -2), method)     # first = x + k

    def ld(j, i):
        if j < i:
            return fwd[j, i - j - 1]
        return bwd[i, j - i - 1]
    return ld


def ld_from_bits(bits, start):
    """ld(j, i) callback over threshold bits bool [M][W] (entry [x, k - 1] for the pair (x, x + k), oriented as in
    snpgpu_ld_prune_bits): 1.0 where the bit is set, 0.0 elsewhere -- prune() with a threshold in (0, 1) then scans the bits.
    A tested pair outside the band raises."""
    W = bits.shape[1]

    def ld(j, i):
        x, y = min(i, j), max(i, j)
        k = y - x
        if not 1 <= k <= W:
            raise AssertionError("tested pair (%d, %d) lies outside the band of width %d" % (j, i, W))
        # forward pass: kept x >= start first; backward pass: kept y first -- the orientation the bits were made for
        assert (x >= start) == (j < i), (j, i, start)
        return 1.0 if bits[x, k - 1] else 0.0
    return ld


def band_width(M, start, pos, slide_max_bp, slide_max_n):
    """The band width the GPU path computes (csrc/ld_prune.hip prune_width), by brute force: the largest |i - j| over the
    (kept j, candidate i) pairs that can be listed whatever is kept"""
    pos = [int(p) for p in pos]

    def win(i, j):
        return abs(i - j) <= slide_max_n and abs(pos[i] - pos[j]) <= slide_max_bp
    W = 0
    for j in range(start, M):                   # forward: listed at j + 1 ... first miss
        i = j + 1
        while i < M and win(i, j):
            i += 1
        W = max(W, i - 1 - j)
    for j in range(0, start):                   # backward, inserted at j
        i = j - 1
        while i >= 0 and win(i, j):
            i -= 1
        W = max(W, j - (i + 1))
    for j in range(start, M):                   # backward, initial list
        if not win(j, start):
            continue
        i = start - 1
        while i >= 0 and win(i, j):
            i -= 1
        if i + 1 < start:
            W = max(W, j - (i + 1))
    return W
