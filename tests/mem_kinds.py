"""Device-memory destinations and caller streams for the calls of include/snpgpu.h that take a result memory kind.

DestLayout places a result `offset_elems` elements past a 256-byte boundary inside one buffer filled with FILL, with GUARD bytes of
the fill before and after it: with offsets 1 and 3 a double result is 8-byte but not 16-byte aligned and an int32 result 4-byte
aligned, and a kernel that stores one element (or one tile row) outside its result changes a guard.  check() works on the raw bytes
of such a buffer, wherever they live: tests/test_cpu_mem_kinds.py runs it on numpy buffers, DeviceDest on a torch allocation read
back through a side stream.  RESULT_CALLS names, for every C function with a result memory kind, the parameter that carries it and
the GPU tests that hand it a device destination; the CPU test holds the table against the header, so an entry point with a result
memory kind cannot be added without such a test.  delayed_write() keeps a caller's stream busy for about 50 ms before a copy, for
the stream-ordering tests.  Nothing here imports the HIP library, and torch only inside the functions that need a GPU."""
import numpy as np

FILL = 0xA5
GUARD = 16384                 # bytes of fill on either side of a result (at least 4096; a multiple of 256)
OFFSETS = (1, 3)              # elements past the 256-byte boundary


class DestLayout:
    """where a result of `shape` / `dtype` lies in a buffer of `total` bytes: [begin, end), guards before and after"""

    def __init__(self, shape, dtype, offset_elems, guard=GUARD):
        assert guard >= 4096 and guard % 256 == 0
        self.shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.begin = guard + int(offset_elems) * self.dtype.itemsize
        self.end = self.begin + self.nbytes
        self.total = (self.end + guard + 255) // 256 * 256

    def new_buffer(self):
        return np.full(self.total, FILL, np.uint8)

    def result(self, raw):
        """the result's elements, a view of the raw bytes"""
        return np.asarray(raw)[self.begin:self.end].view(self.dtype).reshape(self.shape)

    def check(self, raw):
        """assert that both guards still hold the fill; returns the result (a view)"""
        raw = np.asarray(raw)
        assert raw.dtype == np.uint8 and raw.shape == (self.total,)
        before = np.flatnonzero(raw[:self.begin] != FILL)
        after = np.flatnonzero(raw[self.end:] != FILL)
        msg = []
        if before.size:
            msg.append("%d bytes written BEFORE the result, the nearest %d bytes (%g elements) in front of it"
                       % (before.size, self.begin - before[-1], (self.begin - before[-1]) / self.dtype.itemsize))
        if after.size:
            msg.append("%d bytes written AFTER the result, the nearest %d bytes (%g elements) behind its end"
                       % (after.size, after[0], after[0] / self.dtype.itemsize))
        assert not msg, "write outside a result of %s %s: %s" % (self.shape, self.dtype, "; ".join(msg))
        return self.result(raw)

    def untouched(self, raw, mask):
        """assert that the result elements chosen by `mask` (boolean, the result's shape) still hold the fill"""
        r = self.result(raw)
        m = np.broadcast_to(np.asarray(mask, bool), self.shape)
        fill = np.full(1, FILL, np.uint8).repeat(self.dtype.itemsize).view(self.dtype)[0]
        bad = m & (r.view(np.uint8).reshape(self.shape + (self.dtype.itemsize,)) != FILL).any(axis=-1)
        assert not bad.any(), "%d elements that should have been left as they were have been written, the first at %s (fill %r)" \
            % (bad.sum(), tuple(int(x) for x in np.argwhere(bad)[0]), fill)


class DeviceDest:
    """A device destination of `shape` / `dtype`, `offset_elems` elements past a 256-byte boundary inside one torch uint8 allocation
    filled with FILL.  ptr: the destination address.  read(): the result as numpy after checking both guards; the bytes come through
    a side stream created beforehand, and nothing synchronises the device: a side-stream copy waits for no other non-blocking stream,
    so it sees what is in memory when the library call has returned."""

    def __init__(self, shape, dtype, offset_elems):
        import torch
        self.layout = DestLayout(shape, dtype, offset_elems)
        self.buf = torch.full((self.layout.total,), FILL, dtype=torch.uint8, device="cuda")
        self._host = torch.empty(self.layout.total, dtype=torch.uint8).pin_memory()
        self._side = torch.cuda.Stream()
        torch.cuda.current_stream().synchronize()          # the fill is in memory before any library stream writes
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = int(self.buf.data_ptr()) + self.layout.begin
        assert (self.ptr - offset_elems * self.layout.dtype.itemsize) % 256 == 0

    def view(self):
        """the destination as a torch uint8 tensor (to place inputs there, or as the target of a caller's copy)"""
        return self.buf[self.layout.begin:self.layout.end]

    def put(self, array):
        """place `array` (the result's shape and dtype) in the destination: inputs that live in the result's memory kind"""
        import torch
        a = np.ascontiguousarray(array, self.layout.dtype)
        assert a.shape == self.layout.shape
        self.view().copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)).cuda())
        torch.cuda.current_stream().synchronize()

    def _raw(self):
        import torch
        with torch.cuda.stream(self._side):
            self._host.copy_(self.buf, non_blocking=True)
        self._side.synchronize()
        return self._host.numpy()

    def read(self):
        return self.layout.check(self._raw()).copy()

    def untouched(self, mask):
        self.layout.untouched(self._raw(), mask)


# ---- a caller's stream kept busy ------------------------------------------------------------------------------------------------------
_DELAY = {}
DELAY_MS = 50.0


def _delay_plan():
    """(a, b, repetitions): torch.mm(a, a, out=b) repeated `repetitions` times lasts about DELAY_MS; sized once per session"""
    import torch
    if not _DELAY:
        a = torch.randn(4096, 4096, device="cuda")
        b = torch.empty_like(a)
        for _ in range(3):
            torch.mm(a, a, out=b)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(8):
            torch.mm(a, a, out=b)
        t1.record()
        t1.synchronize()
        per = max(t0.elapsed_time(t1) / 8, 1e-3)
        _DELAY.update(a=a, b=b, reps=max(4, int(np.ceil(DELAY_MS / per))))
    return _DELAY["a"], _DELAY["b"], _DELAY["reps"]


def delayed_write(stream, dst_tensor, src_tensor):
    """Enqueue on `stream` (torch.cuda.Stream) about DELAY_MS of matrix products and then dst_tensor.copy_(src_tensor); returns an
    event recorded after the copy.  Right after issuing the library call under test the caller asserts `not ev.query()`
    (still_pending): if that fails the delay was too short for this machine -- the test proved nothing, the library is not to blame."""
    import torch
    a, b, reps = _delay_plan()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(reps):
            torch.mm(a, a, out=b)
        dst_tensor.copy_(src_tensor, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def still_pending(ev):
    assert not ev.query(), ("the caller's delayed work had already finished when the library call returned: the test's delay "
                            "(mem_kinds.DELAY_MS) was too short to show any ordering; this says nothing about the library")


# ---- every C function with a result memory kind ----------------------------------------------------------------------------------------
# compare: BYTES = the device result has the host result's bytes (two host calls must agree, or the test fails and asks for an
# oracle); "oracle: ..." = both forms are held to the named tolerance, and to each other's bytes as well whenever two host calls
# agree.  One run on an MI355X: two host calls differed for the Krylov solvers only (snpgpu_panels_topk_eigen, snpgpu_multi_topk_eigen);
# the projector's sums use fp64 atomics, which promise no order, and agreed byte for byte at these shapes.
BYTES = "bytes"
ORACLE_PROJ = "oracle: test_projector_vs_oracle_synthetic's rtol 1e-9 / 1e-10 (fp64 atomics: two host calls need not agree)"
ORACLE_EIG = "oracle: the eigen tests' rtol 2e-5 on eigenvalues and 1e-8 residual (the iterative solver is not reproducible)"


def _e(param, compare, *tests):
    return dict(param=param, compare=compare, tests=tuple(tests))


RESULT_CALLS = {
    # accumulator finalisers
    "snpgpu_ibs_num": _e("mem", BYTES, "test_ibs_finalisers"),
    "snpgpu_ibs_ave": _e("mem", BYTES, "test_ibs_finalisers"),
    "snpgpu_ibd_mom": _e("mem", BYTES, "test_ibs_finalisers"),
    "snpgpu_king_robust_counts": _e("mem", BYTES, "test_king_robust_finalisers"),
    "snpgpu_king_robust": _e("mem", BYTES, "test_king_robust_finalisers"),
    "snpgpu_king_homo": _e("mem", BYTES, "test_king_homo_finaliser"),
    "snpgpu_diss": _e("mem", BYTES, "test_diss_finalisers"),
    "snpgpu_diss_sums": _e("mem", BYTES, "test_diss_finalisers"),
    "snpgpu_grm_gcta": _e("mem", BYTES, "test_grm_gcta_finaliser"),
    "snpgpu_pca_cov": _e("mem", BYTES, "test_pca_cov_finaliser"),
    "snpgpu_eigmix": _e("mem", BYTES, "test_eigmix_finaliser"),
    "snpgpu_indiv_beta": _e("mem", BYTES, "test_indiv_beta_finaliser"),
    "snpgpu_pca_eigen": _e("mem", ORACLE_EIG, "test_pca_eigen"),
    "snpgpu_select_pairs": _e("mem", BYTES, "test_select_pairs"),
    "snpgpu_panels_topk_eigen": _e("mem", ORACLE_EIG, "test_panels_topk_eigen"),
    # gathers over several panels
    "snpgpu_multi_ibs_num": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_ibs_ave": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_king_robust": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_king_robust_counts": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_king_homo": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_diss": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_grm_gcta": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_eigmix": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_pca_cov": _e("mem", BYTES, "test_multi_gathers"),
    "snpgpu_multi_topk_eigen": _e("mem", ORACLE_EIG, "test_multi_topk_eigen"),
    # projector
    "snpgpu_proj_snp_corr": _e("out_mem", ORACLE_PROJ, "test_projector_device"),
    "snpgpu_proj_snp_loading": _e("out_mem", ORACLE_PROJ, "test_projector_device"),
    "snpgpu_proj_snp_loading_ext": _e("out_mem", ORACLE_PROJ, "test_projector_device"),
    "snpgpu_proj_samp_loading": _e("out_mem", ORACLE_PROJ, "test_projector_samp_loading"),
    # LD, IBD-MLE, one-shots
    "snpgpu_ld_result": _e("out_mem", BYTES, "test_ld_result"),
    "snpgpu_ibd_mle": _e("out_mem", BYTES, "test_ibd_mle"),
    "snpgpu_ibd_loglik": _e("out_mem", BYTES, "test_ibd_loglik"),
    "snpgpu_ibd_mle_pairs": _e("out_mem", BYTES, "test_ibd_mle_pairs"),
    "snpgpu_ibd_jacquard_pairs": _e("out_mem", BYTES, "test_ibd_jacquard_pairs"),
    "snpgpu_pop_counts": _e("out_mem", BYTES, "test_pop_counts"),
    "snpgpu_geno_counts": _e("out_mem", BYTES, "test_geno_counts"),
    "snpgpu_hwe_counts": _e("mem", BYTES, "test_hwe_counts"),
    "snpgpu_ind_inb": _e("out_mem", BYTES, "test_ind_inb"),
    "snpgpu_pair_tables": _e("out_mem", BYTES, "test_pair_tables"),
    "snpgpu_geno_select": _e("dst_mem", BYTES, "test_geno_select_convert"),
    "snpgpu_geno_convert": _e("dst_mem", BYTES, "test_geno_select_convert"),
}


def header_prototypes(text):
    """{function name: [parameter names]} of the `int snpgpu_...(...)` prototypes of a header text (comments removed)"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"\bint\s+(snpgpu_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        params = []
        for p in m.group(2).split(","):
            names = re.findall(r"[A-Za-z_]\w*", p)
            if names and names != ["void"]:
                params.append(names[-1])
        out[m.group(1)] = params
    return out
