"""Objects created on a CALLER'S stream (snpgpu_opts.stream and the `stream` argument of the one-shot calls): what bench.py and
snprelate_amd/multigpu.py run on -- several contexts on one torch stream, device blocks in, device results out.

The stream is kept busy by mem_kinds.delayed_write(): about 50 ms of matrix products, then the copy that puts the REAL block where a
DECOY (another valid block) lay.  The library call is issued at once.  A call that did not order itself after the caller's stream
would read the decoy; a call that read its block later than stream order allows would read what the caller wrote afterwards.  Every
test asserts that its own delay was in effect (mem_kinds.still_pending: `not ev.query()`): right after the call where the call is
asynchronous (snpgpu_feed of a device block, pinned feeds, snpgpu_synth_block, the projector's device-to-device calls), and right
before it where the call blocks until it has read its input (snpgpu_ld_feed, the one-shot calls) -- if that assertion fails the delay
was too short on this machine and the test says so; it does not blame the library.

Shapes: 333 samples, 1500 SNPs in blocks of 1024 (and row panels 256..512 of 600 samples for the two contexts on one stream).
References: the CPU oracle (counters bit for bit; GRM in test_gpu_parity.py's norm below 1e-5; LD values with test_gpu_ld.py's
tolerance), and for the one-shot calls the same call on host memory, which their own tests hold against their references."""
import functools

import numpy as np
import pytest

import mem_kinds as M
import oracle as orc
from conftest import synth_geno

pytestmark = pytest.mark.gpu

N, L, BLK = 333, 1500, 1024
SPANS = [(0, 1024), (1024, 1500)]


@functools.lru_cache(maxsize=None)
def _data(n=N):
    """(real matrix, decoy matrix) uint8 [L][n] and their 2-bit rows"""
    from snprelate_amd.gds import pack_2bit_rows
    g = synth_geno(n, L, missing=0.03, seed=n)
    d = synth_geno(n, L, missing=0.03, seed=n + 4000)
    return g, d, pack_2bit_rows(g), pack_2bit_rows(d)


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.current_stream().synchronize()
    return t


def _rel_err(got, ref):
    """test_gpu_parity.py's figure: the larger of the contract and the off-diagonal-floor errors of a packed triangle"""
    from norms import error_figures, tri_diag_scale
    n = int((np.sqrt(8 * ref.size + 1) - 1) / 2 + 0.5)
    f = error_figures(got, ref, tri_diag_scale(ref, n))
    return max(f["contract"], f["offdiag"])


def _check_acc(kind, a, g):
    """the context's result against the oracle of g: counters bit for bit, GRM below 1e-5"""
    if kind == "IBS":
        ref = orc.ibs_count(g)
        for k, got in enumerate(a.ibs_num(packed=True)):
            assert np.array_equal(got, ref[:, k].astype(np.int32)), "ibs%d differs from the real block's counters" % k
    else:
        err = _rel_err(a.grm_gcta(packed=True), orc.grm_gcta(g))
        assert err < 1e-5, err


def _delayed_blocks(stream, real, decoy):
    """[(device buffer holding the decoy block, event)]: the real block arrives on `stream` after the delay"""
    out = []
    for lo, hi in SPANS:
        buf = _cuda(decoy[lo:hi])
        src = _cuda(real[lo:hi])
        out.append((buf, src, lo, hi))
    return out


@pytest.mark.parametrize("kind", ["IBS", "GRM_GCTA"])
def test_input_ordered_after_the_callers_work(kind):
    """the block is complete only in stream order: snpgpu_feed of a device block orders itself after the caller's stream"""
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    s = torch.cuda.Stream()
    with _lib.Accumulator(getattr(_lib, kind), N, max_block_snps=BLK, stream=s.cuda_stream) as a:
        keep = _delayed_blocks(s, pg, pd)
        for buf, src, lo, hi in keep:
            ev = M.delayed_write(s, buf, src)
            a.feed_device(buf.data_ptr(), hi - lo)
            M.still_pending(ev)
        _check_acc(kind, a, g)
        s.synchronize()


@pytest.mark.parametrize("kind", ["IBS", "GRM_GCTA"])
def test_input_read_before_later_work_of_the_caller(kind):
    """include/snpgpu.h: the block stays unchanged "until the pre-pass has read it -- snpgpu_sync, or any call that orders after the
    context's stream".  The caller's overwrite of the block, enqueued on the same stream right after the feed, is such a call."""
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    s = torch.cuda.Stream()
    with _lib.Accumulator(getattr(_lib, kind), N, max_block_snps=BLK, stream=s.cuda_stream) as a:
        keep = _delayed_blocks(s, pg, pd)
        alive = []                                                 # (until the stream has run)
        for buf, src, lo, hi in keep:
            decoy = _cuda(pd[lo:hi])
            alive.append(decoy)
            ev = M.delayed_write(s, buf, src)
            a.feed_device(buf.data_ptr(), hi - lo)
            with torch.cuda.stream(s):
                buf.copy_(decoy, non_blocking=True)               # the caller reuses its buffer, in stream order
            M.still_pending(ev)
        _check_acc(kind, a, g)
        s.synchronize()
        for buf, src, lo, hi in keep:
            assert np.array_equal(buf.cpu().numpy(), pd[lo:hi])   # the overwrite did happen


@pytest.mark.parametrize("kind", ["IBS", "GRM_GCTA"])
def test_result_complete_at_return(kind):
    """a finaliser into device memory on a context whose stream is still busy when it is called: the result is there, whole, when
    the call returns -- read through a side stream that waits for nothing"""
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    s = torch.cuda.Stream()
    with _lib.Accumulator(getattr(_lib, kind), N, max_block_snps=BLK, stream=s.cuda_stream) as a:
        keep = _delayed_blocks(s, pg, pd)
        for buf, src, lo, hi in keep:
            ev = M.delayed_write(s, buf, src)
            a.feed_device(buf.data_ptr(), hi - lo)
        M.still_pending(ev)
        for off in M.OFFSETS:
            if kind == "IBS":
                dest = M.DeviceDest((a.slab_size(),), np.float64, off)
                a.ibs_ave(packed=True, out_ptr=dest.ptr)
                got, host = dest.read(), a.ibs_ave(packed=True)
            else:
                dest = M.DeviceDest((N, N), np.float64, off)
                a.grm_gcta(packed=False, out_ptr=dest.ptr)
                got, host = dest.read(), a.grm_gcta(packed=False)
            assert got.tobytes() == host.tobytes()
        _check_acc(kind, a, g)


def _run_two(stream_handle, n, rows, blocks):
    """an IBS and a GRM_GCTA panel fed the device blocks alternately, as multigpu.py's shared stream does: (ibs_num, grm) bytes"""
    from snprelate_amd import _lib
    kw = dict(row_begin=rows[0], row_end=rows[1], max_block_snps=BLK)
    if stream_handle:
        kw["stream"] = stream_handle
    with _lib.Accumulator(_lib.IBS, n, **kw) as a, _lib.Accumulator(_lib.GRM_GCTA, n, **kw) as b:
        for t in blocks:
            a.feed_device(t.data_ptr(), t.shape[0])
            b.feed_device(t.data_ptr(), t.shape[0])
        ibs = a.ibs_num(packed=True)
        grm = b.grm_gcta(packed=True)
        a.sync()
        b.sync()
    return ibs, grm


def test_two_contexts_on_one_caller_stream():
    """IBS and GRM_GCTA panels (rows 256..512 of 600) on ONE caller stream with alternating feeds equal each context's own-stream
    run: counters and GRM byte for byte; the counters also equal the oracle's slab"""
    import torch
    n, rows = 600, (256, 512)
    g, d, pg, pd = _data(n)
    blocks = [_cuda(pg[lo:hi]) for lo, hi in SPANS]
    own = _run_two(None, n, rows, blocks)
    s = torch.cuda.Stream()
    scratch, src = _cuda(pd[:8]), _cuda(pg[:8])
    from snprelate_amd import _lib
    kw = dict(row_begin=rows[0], row_end=rows[1], max_block_snps=BLK, stream=s.cuda_stream)
    with _lib.Accumulator(_lib.IBS, n, **kw) as a, _lib.Accumulator(_lib.GRM_GCTA, n, **kw) as b:
        # (snpgpu_create clears its accumulators on the stream and waits for that: the delay starts once both contexts exist)
        ev = M.delayed_write(s, scratch, src)                     # the caller's stream is busy while the feeds are issued
        for t in blocks:
            a.feed_device(t.data_ptr(), t.shape[0])
            b.feed_device(t.data_ptr(), t.shape[0])
        M.still_pending(ev)
        ibs = a.ibs_num(packed=True)
        grm = b.grm_gcta(packed=True)
    s.synchronize()
    for k in range(3):
        assert ibs[k].tobytes() == own[0][k].tobytes(), "ibs%d on the shared stream differs from the own-stream run" % k
    assert grm.tobytes() == own[1].tobytes(), "GRM on the shared stream differs from the own-stream run"
    lo, hi = rows[0] * n - rows[0] * (rows[0] - 1) // 2, rows[1] * n - rows[1] * (rows[1] - 1) // 2
    ref = orc.ibs_count(g)
    for k in range(3):
        assert np.array_equal(ibs[k], ref[lo:hi, k].astype(np.int32))


@pytest.mark.parametrize("kind", ["IBS", "GRM_GCTA"])
@pytest.mark.parametrize("fmt", ["u8", "packed"])
def test_pinned_feeds_on_a_caller_stream(kind, fmt):
    """the two-buffer loop of input_forms.feed on a context created on a caller's stream: the copies run on the context's copy
    stream, ordered against the caller's stream by events (hipStreamWaitEvent in ctx_feed.hip), while that stream is busy.  The first
    feed out of either buffer allocates its staging copy on the device and waits for the stream, so the delay starts after two
    blocks; the four that follow reuse both buffers while the kernels that read their staging copies are still held up behind it."""
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    rows, code = (g, _lib.GENO_U8) if fmt == "u8" else (pg, _lib.GENO_PACKED2)
    s = torch.cuda.Stream()
    scratch, src = _cuda(pd[:8]), _cuda(pg[:8])
    bufs = [_lib.PinnedBuffer((BLK, rows.shape[1])) for _ in range(2)]
    try:
        with _lib.Accumulator(getattr(_lib, kind), N, max_block_snps=BLK, stream=s.cuda_stream) as a:
            cuts = [0, 256, 512, 768, 1024, 1280, L]
            for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                if k == 2:
                    ev = M.delayed_write(s, scratch, src)
                pb = bufs[k & 1]
                a.host_wait(pb)                              # the copy of the block this buffer held before has left it
                pb.array[:hi - lo] = rows[lo:hi]
                a.feed_pinned(pb, hi - lo, code)
            M.still_pending(ev)
            a.sync()
            _check_acc(kind, a, g)
    finally:
        for pb in bufs:
            pb.free()


# ---- the other objects and one-shot calls that take a stream -------------------------------------------------------------------------------

def test_ld_matrix_on_a_caller_stream():
    """snpgpu_ld_feed of a device block on an object created on the caller's stream: ordered after that stream's work; the call
    returns when the block has been read, so the delay is asserted before it"""
    import torch
    import ld_ref
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    s = torch.cuda.Stream()
    with _lib.LDMatrix(N, L, method=_lib.LD_COMPOSITE, slide=7, max_block_snps=BLK, stream=s.cuda_stream) as ld:
        keep = _delayed_blocks(s, pg, pd)
        for buf, src, lo, hi in keep:
            decoy = _cuda(pd[lo:hi])
            ev = M.delayed_write(s, buf, src)
            M.still_pending(ev)
            ld.feed_device(buf.data_ptr(), hi - lo)
            buf.copy_(decoy)                                       # the block has been read: the caller may reuse it at once
        got = ld.result()
    s.synchronize()
    ref = ld_ref.ld_mat(g, "composite", 7, False)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12, equal_nan=True)


def test_projector_on_a_caller_stream():
    """Projector(stream=): a device block that arrives late on the caller's stream, the correlations into device memory
    (stream-ordered: the delay is still running when the call returns), sync(), read"""
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    k = 5
    ev_mat = np.random.default_rng(8).normal(size=(k, N))
    ref = orc.pca_snp_corr(g, ev_mat)
    s = torch.cuda.Stream()
    with _lib.Projector(N, k, max_block_snps=BLK, stream=s.cuda_stream) as p:
        p.set_eigvec(ev_mat)
        keep = _delayed_blocks(s, pg, pd)
        for buf, src, lo, hi in keep:
            dest = M.DeviceDest((hi - lo, k), np.float64, 1)
            ev = M.delayed_write(s, buf, src)
            p.snp_corr(buf.data_ptr(), n_snp=hi - lo, out_ptr=dest.ptr)
            M.still_pending(ev)
            p.sync()
            got = dest.read()
            assert np.array_equal(np.isnan(got), np.isnan(ref[lo:hi]))
            np.testing.assert_allclose(got, ref[lo:hi], rtol=1e-9, atol=1e-12, equal_nan=True)


def _late_matrix(s):
    """(device buffer of all L rows holding the decoy, event): the real rows arrive on `s` after the delay"""
    g, d, pg, pd = _data()
    buf, src = _cuda(pd), _cuda(pg)
    ev = M.delayed_write(s, buf, src)
    M.still_pending(ev)                                            # (the calls below block until they have their result)
    return buf, src


def test_ld_prune_and_ld_score_on_a_caller_stream():
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    pos = np.cumsum(np.random.default_rng(3).integers(1, 4000, L)).astype(np.int32)
    prune = lambda x, **kw: _lib.ld_prune(x, N, pos, 0, 500000, 50, 0.2, method=_lib.LD_COMPOSITE, fmt=_lib.GENO_PACKED2, **kw)[0]   # noqa: E731
    score = lambda x, **kw: _lib.ld_score(x, N, pos, 500000, 50, method=_lib.LD_CORR, fmt=_lib.GENO_PACKED2, **kw)[:3]               # noqa: E731
    want_keep, decoy_keep = prune(pg), prune(pd)
    want_score, decoy_score = score(pg), score(pd)
    assert not np.array_equal(want_keep, decoy_keep) and not np.array_equal(want_score[0], decoy_score[0])
    s = torch.cuda.Stream()
    buf, src = _late_matrix(s)
    got = prune(int(buf.data_ptr()), n_snp=L, max_block_snps=BLK, stream=s.cuda_stream)
    assert np.array_equal(got, want_keep), "ld_prune read its device rows before the caller's stream had written them"
    buf2, src2 = _late_matrix(s)
    got = score(int(buf2.data_ptr()), n_snp=L, max_block_snps=BLK, stream=s.cuda_stream)
    for a, b in zip(got, want_score):
        assert a.tobytes() == b.tobytes(), "ld_score read its device rows before the caller's stream had written them"
    s.synchronize()


def test_geno_select_on_a_caller_stream():
    """a device source that arrives late on the caller's stream, a device destination: complete when the call returns"""
    import torch
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    rb = pg.shape[1]
    samp = np.random.default_rng(2).permutation(N)[:101].astype(np.int32)
    kw = dict(row_stride_bits=8 * rb, samp_index=samp)
    want = _lib.geno_select(pg, 0, L, N, **kw)
    assert not np.array_equal(want, _lib.geno_select(pd, 0, L, N, **kw))
    s = torch.cuda.Stream()
    buf, src = _late_matrix(s)
    dest = M.DeviceDest(want.shape, np.uint8, 3)
    _lib.geno_select(int(buf.data_ptr()), 0, L, N, n_bytes=pg.size, out=dest.ptr, stream=s.cuda_stream, **kw)
    assert np.array_equal(dest.read(), want)
    s.synchronize()


def test_synth_block_on_a_caller_stream():
    """snpgpu_synth_block with a stream is enqueued behind the caller's work on it: the block it writes is what the buffer holds
    at the end, not the decoy the caller's delayed copy put there before it -- and a feed on the same stream reads that block"""
    import torch
    from oracle.synth import synth_hash_block_packed, synth_hash_geno
    from snprelate_amd import _lib
    g, d, pg, pd = _data()
    n_snp, seed = 1024, 77
    want = synth_hash_block_packed(N, 0, n_snp, seed, 0.02)
    s = torch.cuda.Stream()
    buf = _cuda(np.zeros_like(pd[:n_snp]))
    decoy = _cuda(pd[:n_snp])
    with _lib.Accumulator(_lib.IBS, N, max_block_snps=BLK, stream=s.cuda_stream) as a:
        ev = M.delayed_write(s, buf, decoy)
        _lib.synth_block(buf.data_ptr(), N, 0, n_snp, seed, missing=0.02, stream=s.cuda_stream)
        a.feed_device(buf.data_ptr(), n_snp)
        M.still_pending(ev)
        ref = orc.ibs_count(synth_hash_geno(np.arange(N), 0, n_snp, seed, 0.02))
        for k, got in enumerate(a.ibs_num(packed=True)):
            assert np.array_equal(got, ref[:, k].astype(np.int32))
    s.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
