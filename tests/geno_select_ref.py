"""numpy restatement of snpgpu_geno_select (include/snpgpu.h section 1j), bit by bit through np.unpackbits / np.packbits and
independent of pack_2bit_rows / unpack_2bit_rows: from a description of a 2-bit stream (bytes, major, n_rows, n_cols, bit0,
stride | row_bit) and the index lists to the packed rows uint8 [n_snp_out][ceil(n_samp_out / 4)], padding codes 3.
Also the sources the tests build: a matrix written as a stream of any layout (make_stream) and the shapes and lists they share."""
import numpy as np


def select_ref(data, major, n_rows, n_cols, bit0=0, stride=None, row_bit=None, samp_index=None, snp_index=None):
    bits = np.unpackbits(np.frombuffer(np.ascontiguousarray(data, dtype=np.uint8).tobytes(), np.uint8), bitorder="little")
    if row_bit is not None:
        start = bit0 + np.asarray(row_bit, np.int64)
    else:
        start = bit0 + np.arange(n_rows, dtype=np.int64) * (2 * n_cols if stride is None else stride)
    pos = start[:, None] + 2 * np.arange(n_cols, dtype=np.int64)[None, :]
    codes = bits[pos] | (bits[pos + 1] << 1)                   # [n_rows][n_cols]
    g = codes.T if major else codes                             # [snp][sample]
    if snp_index is not None:
        g = g[np.asarray(snp_index, np.int64)]
    if samp_index is not None:
        g = g[:, np.asarray(samp_index, np.int64)]
    return pack_ref(g)


def pack_ref(g):
    """codes [L][n] -> rows [L][ceil(n / 4)], code j at bits 2 (j % 4) of byte j // 4, the unused codes of the last byte 3"""
    L, n = g.shape
    rb = (n + 3) // 4
    b = np.ones((L, 8 * rb), np.uint8)
    b[:, 0:2 * n:2] = g & 1
    b[:, 1:2 * n:2] = g >> 1
    return np.packbits(b, axis=1, bitorder="little")


def make_stream(g, layout, bit0=0, seed=0):
    """g: codes [n_snp][n_samp].  layout "packed" (byte-aligned rows of SNPs), "sample.order" (the continuous stream of SNP rows),
    "snp.order" (the continuous stream of sample rows), "row_bit0" / "row_bit1" (rows of SNPs / samples at random even bit
    positions with gaps, in shuffled order).  Returns (bytes uint8, kwargs of the description): bits before bit0, in the gaps and
    after the last element are random."""
    rng = np.random.default_rng(seed)
    L, n = g.shape
    major = 1 if layout in ("snp.order", "row_bit1") else 0
    m = g.T if major else g
    n_rows, n_cols = m.shape
    if layout == "packed":
        stride = 8 * ((n_cols + 3) // 4)
    else:
        stride = 2 * n_cols
    row_bit = None
    if layout.startswith("row_bit"):
        gaps = 2 * rng.integers(0, 21, n_rows)
        order = rng.permutation(n_rows)
        row_bit = np.empty(n_rows, np.int64)
        at = 0
        for r in order:
            at += int(gaps[r])
            row_bit[r] = at
            at += 2 * n_cols
        total = bit0 + at
        start = bit0 + row_bit
    else:
        total = bit0 + (n_rows - 1) * stride + 2 * n_cols
        start = bit0 + np.arange(n_rows, dtype=np.int64) * stride
    nbytes = (total + 7) // 8
    bits = rng.integers(0, 2, 8 * nbytes).astype(np.uint8)
    pos = start[:, None] + 2 * np.arange(n_cols, dtype=np.int64)[None, :]
    bits[pos] = m & 1
    bits[pos + 1] = m >> 1
    kw = dict(major=major, n_rows=n_rows, n_cols=n_cols, bit0=bit0)
    if row_bit is None:
        kw["row_stride_bits"] = stride
    else:
        kw["row_bit"] = row_bit
    return np.packbits(bits, bitorder="little"), kw


def ref_of(data, kw, samp_index=None, snp_index=None):
    return select_ref(data, kw["major"], kw["n_rows"], kw["n_cols"], kw["bit0"], kw.get("row_stride_bits"), kw.get("row_bit"),
                      samp_index, snp_index)


def codes(n_snp, n_samp, missing, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, (n_snp, n_samp)).astype(np.uint8)
    if missing:
        g[rng.random((n_snp, n_samp)) < missing] = 3
    return g


SAMPLES = (1, 3, 4, 5, 63, 64, 65, 130, 279, 2049)
SNPS = (1, 3, 5, 63, 64, 65, 257, 1000)
MISSING = (0.0, 0.05, 0.30)
LAYOUTS = ("packed", "sample.order", "snp.order")


def sample_lists(n, seed=1):
    """name -> list (None = all): every second, reversed, one sample, a random list with repeats longer than the source, runs of
    consecutive samples from 0, 1, 2, 3 whose lengths give n_out % 4 in {0, 1, 2, 3} and n_out % 64 in {0, 1, 63} where n allows"""
    rng = np.random.default_rng(seed)
    out = {"all": None, "second": np.arange(0, n, 2), "reversed": np.arange(n)[::-1], "one": np.array([n // 2]),
           "random": rng.integers(0, n, n + 7)}
    for s0 in range(4):
        if s0 >= n:
            continue
        for ln in (n - s0, n - s0 - 1, 64, 65, 127, 63 + s0, 6):
            if 1 <= ln <= n - s0:
                out["run%d+%d" % (s0, ln)] = np.arange(s0, s0 + ln)
    for ln in (128, 129, 191, 66, 67):          # lists (not runs) of those sizes
        if ln <= n:
            out["perm%d" % ln] = rng.permutation(n)[:ln]
    return {k: (None if v is None else v.astype(np.int32)) for k, v in out.items()}


def snp_lists(L, seed=2):
    """None, one SNP, a window starting off a multiple of 4 and of 64, a scattered ascending list, a descending list"""
    rng = np.random.default_rng(seed)
    out = {"all": None, "one": np.array([L // 3])}
    if L > 70:
        out["window"] = np.arange(67, min(L, 67 + 130))
    if L > 2:
        out["window1"] = np.arange(1, L)
        out["scattered"] = np.sort(rng.choice(L, max(1, L // 3), replace=False))
    out["descending"] = np.arange(L)[::-1]
    return {k: (None if v is None else v.astype(np.int32)) for k, v in out.items()}
