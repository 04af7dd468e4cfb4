"""Time the [shuffle] epoch gather kernels (csrc/gpu/kernels_shuffle.hip) against a
hipMemcpyAsync device-to-device copy of the same byte count, in one process, alternating.

  python scripts/shuffle_bench.py [--iters 50] [--rounds 5] [--quick]

Shapes: MNIST 60 000 x 800 uint8 -> fragment-major (the tile front's input), RRUFF-shaped
16 384 x 4096 bf16 row-major, plus the label and dense-target gathers of an MNIST epoch and
the permutation kernel.  Times are device-event times per call (us), median over rounds of
`iters` back-to-back calls; bytes = read + written.  One JSON line per shape.
--quick: 2 rounds of 3 calls (for a profiler run)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hpnn_amd import ops  # noqa: E402

HIP = ctypes.CDLL("libamdhip64.so")
HIP.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
D2D = 3


def memcpy(dst, src):
    rc = HIP.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), D2D,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.iters, a.rounds = 3, 2
    if not torch.cuda.is_available():
        raise SystemExit("shuffle_bench: no GPU")
    dev = "cuda"
    cases = []

    def add(name, n, fn, src, dst):
        cases.append((name, n, fn, src, dst))

    n = 60000
    perm = ops.epoch_perm(n, 10958, 0, dev)
    x8 = torch.randint(0, 256, (n, 800), dtype=torch.uint8, device=dev)
    rows_p = ops.pad_to(n, 4096)
    f8 = torch.empty(rows_p // 32, 50, 64, 8, dtype=torch.uint8, device=dev)
    add("gather_fm u8 60000x800 (MNIST)", n, lambda: ops.gather_fragment_major(x8, perm, f8), x8, f8)
    lab = torch.randint(0, 10, (n, 1), dtype=torch.int32, device=dev)
    lab_o = torch.empty(rows_p, 1, dtype=torch.int32, device=dev)
    add("gather_rows labels 60000x4B", n, lambda: ops.gather_rows(lab, perm, lab_o), lab, lab_o)
    tgt = torch.rand(n, 10, device=dev)
    tgt_o = torch.empty(rows_p, 10, device=dev)
    add("gather_rows targets 60000x40B", n, lambda: ops.gather_rows(tgt, perm, tgt_o), tgt, tgt_o)
    word, err = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    add("epoch_perm 60000 (+ word advance)", n,
        lambda: ops.epoch_perm(n, 10958, word, dev, out=perm2, err=err, advance=True), None, None)
    perm2 = torch.empty(n, dtype=torch.int32, device=dev)
    nr = 16384
    permr = ops.epoch_perm(nr, 10958, 0, dev)
    xr = torch.randn(nr, 4096, device=dev).bfloat16()
    xo = torch.empty(nr, 4096, dtype=torch.bfloat16, device=dev)
    add("gather_rows bf16 16384x4096 (RRUFF)", nr, lambda: ops.gather_rows(xr, permr, xo), xr, xo)
    fr = torch.empty(nr // 32, 256, 64, 8, dtype=torch.bfloat16, device=dev)
    add("gather_fm bf16 16384x4096", nr, lambda: ops.gather_fragment_major(xr, permr, fr), xr, fr)

    for name, n_, fn, src, dst in cases:
        cp = None
        if src is not None:
            flat_s, flat_d = src.view(-1), torch.empty_like(src).view(-1)
            cp = lambda: memcpy(flat_d, flat_s)  # noqa: E731
        for f in (fn, cp):  # warm up: code objects, copy engine paths
            if f:
                timed(f, 3)
        tk, tc = [], []
        for _ in range(a.rounds):  # alternate kernel and copy
            tk.append(timed(fn, a.iters))
            if cp:
                tc.append(timed(cp, a.iters))
        rec = {"case": name, "kernel_us": round(statistics.median(tk), 2), "kernel_us_min_max": [round(min(tk), 2),
                                                                                                 round(max(tk), 2)]}
        if cp:
            nbytes = src.numel() * src.element_size()
            c = statistics.median(tc)
            rec.update({"bytes_one_way": nbytes, "memcpy_us": round(c, 2),
                        "memcpy_us_min_max": [round(min(tc), 2), round(max(tc), 2)],
                        "ratio": round(statistics.median(tk) / c, 3),
                        "kernel_GBps_read_plus_write": round(2 * nbytes / statistics.median(tk) / 1e3, 1),
                        "memcpy_GBps_read_plus_write": round(2 * nbytes / c / 1e3, 1)})
        print(json.dumps(rec), flush=True)
    assert int(err.item()) == 0


if __name__ == "__main__":
    main()
