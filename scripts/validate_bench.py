"""Time one validation pass of the BF16 plan (MLP.evaluate) on the fused tile path
(hpnn_mlp3_eval, csrc/gpu/kernels_mlp3t.hip) against the per-layer path (HPNN_EVAL_FUSED=0:
forward GEMMs + the output kernel in chunks of Bp rows), in one process, alternating.

  python scripts/validate_bench.py [--iters 50] [--rounds 5] [--batch 4096] [--quick]

MNIST-shaped 784-128-64-10 SNN on 8-bit pixels with labels, held-out sets of 10 240 and
65 536 rows.  The fused path reads the set fragment-major as bytes; the per-layer path reads a
row-major BF16 copy (its conversion is setup, not timed).  Times are device-event times per
pass (us), median over rounds of `iters` back-to-back passes.  One JSON line per set size.
--quick: 2 rounds of 3 passes (for a profiler run)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hpnn_amd.models import MLP  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.iters, a.rounds = 3, 2
    if not torch.cuda.is_available():
        raise SystemExit("validate_bench: no GPU")
    fused = MLP([784, 128, 64, 10], "SNN", batch=a.batch, momentum=True, fused="t")
    layer = MLP([784, 128, 64, 10], "SNN", batch=a.batch, momentum=True, fused="t")
    layer.plan.eval_fused = False
    assert fused.plan.eval_is_fused() and not layer.plan.eval_is_fused()
    g = torch.Generator().manual_seed(1)
    for n in (10240, 65536):
        X = torch.randint(0, 256, (n, 784), dtype=torch.uint8, generator=g).cuda()
        lab = torch.randint(0, 10, (n,), dtype=torch.int32, generator=g).cuda()
        Xf = fused.prepare_input(X)
        Xr = layer._rowmajor(layer.prepare_input(X))  # what evaluate would convert per call, in whole chunks
        pad = -Xr.shape[0] % layer.Bp
        Xr = torch.cat([Xr, Xr.new_zeros(pad, Xr.shape[1])]).contiguous() if pad else Xr.contiguous()
        f = lambda: fused.evaluate(Xf, labels=lab, n_valid=n)  # noqa: E731
        p = lambda: layer.evaluate(Xr, labels=lab, n_valid=n)  # noqa: E731
        for fn in (f, p):
            timed(fn, 3)
        fused.reset_eval_stats()
        layer.reset_eval_stats()
        f()
        p()
        sf, sp = fused.read_eval_stats(), layer.read_eval_stats()
        tf, tp = [], []
        for _ in range(a.rounds):  # alternate the two paths
            tf.append(timed(f, a.iters))
            tp.append(timed(p, a.iters))
        print(json.dumps({"rows": n, "batch": a.batch, "fused_us": round(statistics.median(tf), 2),
                          "fused_us_min_max": [round(min(tf), 2), round(max(tf), 2)],
                          "per_layer_us": round(statistics.median(tp), 2),
                          "per_layer_us_min_max": [round(min(tp), 2), round(max(tp), 2)],
                          "per_layer_launches": 4 * ((n + layer.Bp - 1) // layer.Bp),
                          "ratio_per_layer_over_fused": round(statistics.median(tp) / statistics.median(tf), 2),
                          "fused_loss_hits": sf, "per_layer_loss_hits": sp}), flush=True)


if __name__ == "__main__":
    main()
