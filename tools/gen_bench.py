#!/usr/bin/env python
"""snpgpu_gen_genotypes on one GPU: one JSON line, printed and written to profiles/gen_bench.json.

N = 100 000 samples, 512 data lines, in two cell styles: "1 0 0" (2 bytes per number with its separator) and "0.973" (6 bytes per
number).  Sixteen different lines are drawn per style and tiled in numpy to the 512; the text is resident on the device.  Per style,
medians of 5 runs after a warm-up:
  kernel     ms of the kernel from the HIP events of snpgpu_gen_stats, and the text bytes per second that is
  copy       a device-to-device copy of the same bytes IN THE SAME RUN, alternating with the kernel runs
  pinned     the whole call (host clock) with the text in page-locked host memory: staging copies, kernel, flags back
No threshold is applied to any of it: the tool records.  Every call runs under an alarm of its own."""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# one sample's three numbers, each with its separator
STYLES = {
    "cells_2_bytes": ["1 0 0 ", "0 1 0 ", "0 0 1 ", "1 0 0 ", "0 1 0 ", "0 0 0 "],
    "cells_6_bytes": ["0.973 0.021 0.006 ", "0.004 0.951 0.045 ", "0.012 0.033 0.955 ", "0.998 0.001 0.001 ", "0.412 0.335 0.253 ",
                      "0.090 0.905 0.005 "],
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--lines", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a single call may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from snprelate_amd import _lib

    torch.cuda.set_device(a.device)
    N, L = a.samples, a.lines
    assert L % 16 == 0, "sixteen different lines are tiled"
    rb = (N + 3) // 4

    def limited(fn):
        signal.alarm(a.limit)                 # no handler: a call that does not return ends the process
        try:
            return fn()
        finally:
            signal.alarm(0)

    def median(v):
        return sorted(v)[len(v) // 2]

    out = {"tool": "gen_bench", "source_stamp": bench.source_stamp(), "N": N, "lines": L, "reps": a.reps, "call_threshold": 0.9, "styles": {}}
    rows = torch.empty((L, rb), dtype=torch.uint8, device="cuda")
    for style, pool in STYLES.items():
        w = len(pool[0])
        assert all(len(c) == w for c in pool)
        rng = np.random.default_rng(len(style))
        cells = np.array([c.encode() for c in pool], "S%d" % w)
        head = np.frombuffer(b"SNP_A-1234567 rs1234567 10000 A C ", np.uint8)
        sixteen = []
        for _ in range(16):
            body = cells[rng.integers(0, len(pool), N)].view(np.uint8).copy()
            body[-1] = 10                                                       # the last number's space becomes the line end
            sixteen.append(np.concatenate([head, body]))
        text = np.tile(np.concatenate(sixteen), L // 16)
        line_bytes = len(head) + N * w
        assert text.size == L * line_bytes
        cb = np.arange(L, dtype=np.int64) * line_bytes + len(head)
        le = np.arange(1, L + 1, dtype=np.int64) * line_bytes - 1
        res = {"number_bytes_with_separator": w // 3, "text_bytes": int(text.size), "cell_text_bytes": int((le - cb).sum())}

        dtext = torch.from_numpy(text).cuda()
        other = torch.empty_like(dtext)
        torch.cuda.synchronize()

        def copy_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            other.copy_(dtext)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def kernel_ms():
            flags, ncell = _lib.gen_genotypes(int(dtext.data_ptr()), cb, le, N, 0.9, int(rows.data_ptr()), n_bytes=text.size, device=a.device)
            assert not flags.any() and (ncell == 3 * N).all()
            return _lib.gen_stats()["kernel_ms"]

        limited(kernel_ms)
        copy_ms()
        k, c = [], []
        for _ in range(a.reps):                                                 # alternating, so that a drift of the clocks meets both
            k.append(limited(kernel_ms))
            c.append(copy_ms())
        k.sort()
        c.sort()
        first = rows[:16].cpu().numpy().copy()
        res.update(kernel_ms_median=median(k), kernel_ms_all=k, kernel_text_bytes_per_s=text.size / (median(k) * 1e-3),
                   kernel_samples_per_s=N * L / (median(k) * 1e-3), copy_ms_median=median(c), copy_ms_all=c,
                   copy_bytes_per_s=text.size / (median(c) * 1e-3), kernel_ms_over_copy_ms=median(k) / median(c))
        del other, dtext
        torch.cuda.empty_cache()

        # the whole call from page-locked host text
        pinned = _lib.PinnedBuffer((text.size,))
        pinned.array[:] = text

        def whole_ms():
            t0 = time.perf_counter()
            flags, _ = _lib.gen_genotypes(pinned.ptr, cb, le, N, 0.9, int(rows.data_ptr()), n_bytes=text.size, text_mem=_lib.HOST_PINNED,
                                          device=a.device)
            ms = (time.perf_counter() - t0) * 1e3
            assert not flags.any()
            return ms, _lib.gen_stats()
        limited(whole_ms)
        runs = sorted((limited(whole_ms) for _ in range(a.reps)), key=lambda r: r[0])
        ms, st = runs[len(runs) // 2]
        assert np.array_equal(rows[:16].cpu().numpy(), first)
        res.update(pinned_call_ms_median=ms, pinned_call_ms_all=[r[0] for r in runs], pinned_h2d_ms=st["h2d_ms"],
                   pinned_kernel_ms=st["kernel_ms"], pinned_launches=st["launches"], pinned_text_bytes_per_s=text.size / (ms * 1e-3))
        pinned.free()
        out["styles"][style] = res
        del text
    s = _lib.gen_stats()
    out.update(chunk_bytes=s["chunk_bytes"], segment_bytes=s["segment_bytes"], halo_bytes=s["halo_bytes"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
