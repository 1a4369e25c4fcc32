#!/usr/bin/env python
"""The text formats on one GPU: one JSON line, printed and written to profiles/text_bench.json.

A window of 2 048 rows of N = 100 000 2-bit codes, resident on the device.  Medians of 5 runs after a warm-up, each kernel figure
next to a device-to-device copy of as many bytes as the text IN THE SAME RUN, alternating with the kernel runs:
  out        snpgpu_text_render for the digit format, PED "A/B", PED "1/2", PED alleles of one byte (the fixed-width kernel with
             its table) and PED alleles of several lengths (the length pass and the write pass), ms from the HIP events of
             snpgpu_text_stats
  in         the tokeniser's two sweeps over the one-byte PED text rendered above, resident on the device: snpgpu_ped_tokens +
             snpgpu_ped_census, and snpgpu_ped_tokens + snpgpu_ped_codes, ms from snpgpu_ped_stats
  calls      snpgdsGDS2PED of a 2 048-sample x N-SNP GenoFile to a file and snpgdsOpenPED of that file, host clock
No threshold is applied to any of it: the tool records.  Every call runs under an alarm of its own."""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--columns", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a single call may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    import snprelate_amd as S
    from snprelate_amd import _lib
    from snprelate_amd.gds import GenoFile

    torch.cuda.set_device(a.device)
    N, L = a.columns, a.rows
    rb = (N + 3) // 4

    def limited(fn):
        signal.alarm(a.limit)                 # no handler: a call that does not return ends the process
        try:
            return fn()
        finally:
            signal.alarm(0)

    def median(v):
        return sorted(v)[len(v) // 2]

    rng = np.random.default_rng(1)
    packed = rng.integers(0, 256, (L, rb), dtype=np.uint8)
    rows = torch.from_numpy(packed).cuda()
    prefixes = _lib._pool([("0\tsample%05d\t0\t0\t0\t-9" % i).encode() for i in range(L)])
    letters = np.frombuffer(b"ACGT", np.uint8)
    one = [bytes(x) for x in rng.choice(letters, (2 * N, 1))]
    mixed = list(one)
    for k in rng.choice(2 * N, N // 10, replace=False):                         # a twentieth of the alleles are indels of 2 ... 10 bytes
        mixed[int(k)] = bytes(rng.choice(letters, int(rng.integers(2, 11))))
    formats = {"digit": (_lib.TEXT_DIGIT, None, None), "ped_ab": (_lib.TEXT_PED_AB, None, prefixes),
               "ped_12": (_lib.TEXT_PED_12, None, prefixes), "ped_allele_1byte": (_lib.TEXT_PED_ALLELE, _lib._pool(one), prefixes),
               "ped_allele_mixed": (_lib.TEXT_PED_ALLELE, _lib._pool(mixed), prefixes)}

    out = {"tool": "text_bench", "source_stamp": bench.source_stamp(), "columns": N, "rows": L, "reps": a.reps, "out": {}, "in": {},
           "calls": {}}
    keep = None
    for name, (fmt, alleles, pre) in formats.items():
        off = limited(lambda: _lib.text_render(int(rows.data_ptr()), L, N, fmt, alleles=alleles, prefixes=pre, device=a.device))
        nbytes = int(off[-1])
        text, other = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def copy_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            other.copy_(text)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def kernel_ms():
            _lib.text_render(int(rows.data_ptr()), L, N, fmt, alleles=alleles, prefixes=pre, text=int(text.data_ptr()), device=a.device)
            return _lib.text_stats()

        limited(kernel_ms)
        copy_ms()
        k, c = [], []
        for _ in range(a.reps):                                                 # alternating, so that a drift of the clocks meets both
            k.append(limited(kernel_ms))
            c.append(copy_ms())
        wr, ln = sorted(s["write_ms"] for s in k), sorted(s["lengths_ms"] for s in k)
        c.sort()
        out["out"][name] = dict(text_bytes=nbytes, write_ms_median=median(wr), write_ms_all=wr, lengths_ms_median=median(ln),
                                launches=k[0]["launches"], copy_ms_median=median(c), copy_ms_all=c,
                                text_bytes_per_s=nbytes / (median(wr) * 1e-3), copy_bytes_per_s=nbytes / (median(c) * 1e-3),
                                write_ms_over_copy_ms=median(wr) / median(c),
                                kernels_ms_over_copy_ms=(median(wr) + median(ln)) / median(c))
        if name == "ped_allele_1byte":
            keep = (text, off, other)
        else:
            del text, other
        torch.cuda.empty_cache()

    # ---- the tokeniser's two sweeps over the one-byte PED text ----------------------------------------------------------------------
    text, off, other = keep
    nbytes = int(off[-1])
    cb = off[:-1] + np.diff(prefixes[1]) + 1
    le = off[1:] - 1
    tokens = torch.empty(L * 2 * N, dtype=torch.uint8, device="cuda")
    table = torch.zeros((N, _lib.PED_ALLELES), dtype=torch.int32, device="cuda")
    codes = torch.empty((L, rb), dtype=torch.uint8, device="cuda")

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        other.copy_(text)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def sweeps():
        flags, count = _lib.ped_tokens(int(text.data_ptr()), nbytes, cb, le, N, int(tokens.data_ptr()), device=a.device)
        assert not flags.any() and (count == 2 * N).all()
        table.zero_()
        _lib.ped_census(int(tokens.data_ptr()), flags, N, int(table.data_ptr()), device=a.device)
        ref = (table.argmax(1) + 0x21).to(torch.uint8).cpu().numpy()
        _lib.ped_codes(int(tokens.data_ptr()), L, N, ref, int(codes.data_ptr()), device=a.device)
        return _lib.ped_stats()

    limited(sweeps)
    copy_ms()
    k, c = [], []
    for _ in range(a.reps):
        k.append(limited(sweeps))
        c.append(copy_ms())
    c.sort()
    res = dict(text_bytes=nbytes, copy_ms_median=median(c), copy_ms_all=c)
    for key in ("tokens_ms", "census_ms", "codes_ms"):
        v = sorted(s[key] for s in k)
        res[key + "_median"], res[key + "_all"] = median(v), v
    res["census_sweep_ms"] = res["tokens_ms_median"] + res["census_ms_median"]
    res["coding_sweep_ms"] = res["tokens_ms_median"] + res["codes_ms_median"]
    res["census_sweep_over_copy"] = res["census_sweep_ms"] / median(c)
    res["coding_sweep_over_copy"] = res["coding_sweep_ms"] / median(c)
    res["tokens_text_bytes_per_s"] = nbytes / (res["tokens_ms_median"] * 1e-3)
    out["in"] = res
    del text, other, tokens, table, codes, keep
    torch.cuda.empty_cache()

    # ---- the two whole calls -------------------------------------------------------------------------------------------------------
    g = GenoFile(packed=np.ascontiguousarray(rng.integers(0, 256, (N, (L + 3) // 4), dtype=np.uint8)), n_samp=L,
                 sample_id=np.array(["sample%05d" % i for i in range(L)]), snp_position=np.arange(1, N + 1),
                 snp_allele=np.array([x.decode() + "/" + y.decode() for x, y in zip(one[0::2], one[1::2])]))
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "b")
        t0 = time.perf_counter()
        limited(lambda: S.snpgdsGDS2PED(g, fn, verbose=False, device=a.device))
        t1 = time.perf_counter()
        gf = limited(lambda: S.snpgdsOpenPED(fn + ".ped", fn + ".map", verbose=False, device=a.device))
        t2 = time.perf_counter()
        size = os.path.getsize(fn + ".ped")
    assert gf.n_samp == L and gf.n_snp == N and gf.ped_flagged_lines == 0
    out["calls"] = dict(ped_bytes=size, gds2ped_s=t1 - t0, openped_s=t2 - t1, gds2ped_bytes_per_s=size / (t1 - t0),
                        openped_bytes_per_s=size / (t2 - t1), openped_windows=gf.ped_windows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
