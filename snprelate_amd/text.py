"""Genotypes as text files: the bodies of snpgdsGDS2PED's .ped and snpgdsGDS2Eigen's .eigenstratgeno.

The 2-bit rows of the selected rectangle go to the device, ``snpgpu_text_render`` turns every row into one line of the file in
device memory, and the host appends that buffer to the file.  Nothing per genotype exists on the host.  A file is built in
windows of whole lines: as many as fit SNPGPU_TEXT_STAGE_BYTES (default 256 MiB) by the longest line the format can give, and at
least one.  A window is: select (and for .ped transpose) its rows with snpgpu_geno_select / snpgpu_geno_convert, render, copy to
page-locked memory, append.  There is no CPU fallback: without a device the calls fail with ``SnpGpuError``.
"""
import numpy as np

from . import _lib
from .textio import stage_bytes


def split_alleles(allele):
    """s1, s2 per entry of snp.allele as gnrConvGDS2PED splits it (src/SNPRelate.cpp:720-734): the text before the first '/' and
    the text between the first and the second; a third allele is ignored, an empty one is "0".  Returns the 2 n pieces s1, s2,
    s1, s2, ... as bytes."""
    out = []
    for a in allele:
        p = str(a).split("/")
        s1, s2 = p[0], (p[1] if len(p) > 1 else "")
        out.append((s1 or "0").encode("latin1"))
        out.append((s2 or "0").encode("latin1"))
    return out


def _span(pos):
    """(k0, k1, idx) of ascending source positions: the rows [k0, k1) and the positions inside them, None when they are all"""
    k0, k1 = int(pos[0]), int(pos[-1]) + 1
    return k0, k1, (None if k1 - k0 == len(pos) else (pos - k0).astype(np.int32))


class _Writer:
    """the device and page-locked buffers of one file, and the append of a rendered window"""

    def __init__(self, f, cap, device):
        import torch
        self.f, self.device, self.torch = f, int(device), torch
        self.text = torch.empty(int(cap), dtype=torch.uint8, device="cuda:%d" % self.device)
        self.host = torch.empty(int(cap), dtype=torch.uint8, pin_memory=True)
        self.windows = 0

    def rows(self, shape):
        return self.torch.empty(shape, dtype=self.torch.uint8, device="cuda:%d" % self.device)

    def render(self, rows, n_rows, n_cols, fmt, alleles, prefixes):
        off = _lib.text_render(int(rows.data_ptr()), n_rows, n_cols, fmt, alleles=alleles, prefixes=prefixes,
                               text=int(self.text.data_ptr()), device=self.device)
        n = int(off[-1])
        self.host[:n].copy_(self.text[:n])
        self.f.write(self.host[:n].numpy())
        self.windows += 1
        return off


def device_visible():
    try:
        return _lib.device_count() > 0
    except _lib.SnpGpuError:
        return False


def _need_device(what):
    if not device_visible():
        raise _lib.SnpGpuError("%s: no HIP device (the text renderer has no CPU fallback)" % what)


def write_eigenstratgeno(f, gdsobj, samp_flag, snp_flag, device=0):
    """the lines of .eigenstratgeno for the selected SNPs (one line each, a digit per selected sample) appended to the binary file
    object f; returns the number of windows"""
    _need_device("snpgdsGDS2Eigen")
    n, rb = gdsobj.n_samp, (gdsobj.n_samp + 3) // 4
    samp_index = None if samp_flag.all() else np.flatnonzero(samp_flag).astype(np.int32)
    ns = n if samp_index is None else len(samp_index)
    pos = np.flatnonzero(snp_flag)
    line = ns + 1
    per = max(1, stage_bytes() // line)
    w = _Writer(f, line * min(per, len(pos)), device)
    packed = gdsobj.packed
    for a in range(0, len(pos), per):
        b = min(a + per, len(pos))
        k0, k1, idx = _span(pos[a:b])
        rows = w.rows((b - a, (ns + 3) // 4))
        _lib.geno_select(packed[k0:k1], 0, k1 - k0, n, row_stride_bits=8 * rb, samp_index=samp_index, snp_index=idx,
                         out=int(rows.data_ptr()), device=device)
        w.render(rows, b - a, ns, _lib.TEXT_DIGIT, None, None)
    return w.windows


def write_ped(f, gdsobj, samp_flag, snp_flag, sample_ids, fmt, alleles=None, device=0):
    """the lines of .ped for the selected samples appended to the binary file object f: "0\\tID\\t0\\t0\\t0\\t-9" and one piece per
    selected SNP.  fmt: _lib.TEXT_PED_AB / TEXT_PED_12 / TEXT_PED_ALLELE with alleles = split_alleles(...) of the selected SNPs.
    Returns the number of windows."""
    _need_device("snpgdsGDS2PED")
    n, rb = gdsobj.n_samp, (gdsobj.n_samp + 3) // 4
    samp = np.flatnonzero(samp_flag).astype(np.int32)
    pos = np.flatnonzero(snp_flag)
    Ls = len(pos)
    k0, k1, idx = _span(pos)
    prefixes = [("0\t%s\t0\t0\t0\t-9" % s).encode("latin1") for s in sample_ids]
    apool = None
    if fmt == _lib.TEXT_PED_ALLELE:
        apool = _lib._pool(alleles)
        la = np.diff(apool[1])
        body = int(np.sum(2 + 2 * np.maximum(np.maximum(la[0::2], la[1::2]), 1)))
    else:
        body = 4 * Ls
    line = max(len(p) for p in prefixes) + body + 1                             # the longest line the format can give
    per = max(1, stage_bytes() // line)
    w = _Writer(f, line * min(per, len(samp)), device)
    src = gdsobj.packed[k0:k1]
    for a in range(0, len(samp), per):
        b = min(a + per, len(samp))
        m = b - a
        # the window's samples as columns of the selected SNP rows, then transposed: the samples become the rows
        sel = w.rows((Ls, (m + 3) // 4))
        _lib.geno_select(src, 0, k1 - k0, n, row_stride_bits=8 * rb, samp_index=samp[a:b], snp_index=idx, out=int(sel.data_ptr()),
                         device=device)
        rows = w.rows((m, (Ls + 3) // 4))
        _lib.geno_convert(int(sel.data_ptr()), 0, Ls, m, dst_major=1, row_stride_bits=8 * ((m + 3) // 4), n_bytes=sel.numel(),
                          out=int(rows.data_ptr()), device=device)
        w.render(rows, m, Ls, fmt, apool, prefixes[a:b])
    return w.windows
