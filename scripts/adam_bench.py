#!/usr/bin/env python3
"""Time the Adam step of the BF16 plan beside the BPM steps it is built on (profiles/adam/README.md).

One process, the MNIST net 784-128-64-10 at batch 65 536 with 8-bit pixels (bench.py's flagship
shape), three models stepped in turn, round after round, so that clock and cache state are shared:

    (a) bpm        BPM as the plan runs it: front, then G0 with its split-K reduction and every
                   layer's step in the same launch (2 launches)
    (b) bpm_3l     BPM with plan.g0_fused = False: front -> g0_reduce -> one update launch (3
                   launches), the sequence Adam builds on
    (c) adam       optimizer="adam": that sequence with the one-thread advance and
                   hpnn_adam_update_multi in place of hpnn_sgd_update_multi (4 launches)

Every model is warmed up, then timed with device events over --steps steps (at least 200) in
rounds of --round steps.  Prints one JSON line: ms per step of each, the differences (b) - (a) and
(c) - (b), and the bytes the update launch of (b) and (c) moves.

    python scripts/adam_bench.py --steps 400
    python scripts/adam_bench.py --rehearse     # CPU: tiny shapes through the emulation, no timing claims
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpnn_amd.models import MLP  # noqa: E402

SIZES = [784, 128, 64, 10]


def update_bytes(m, adam):
    """bytes one update launch reads and writes: the S slabs of every layer, the FP32 masters and
    moments read and written, the BF16 W and W^T (and W0f) written"""
    total = 0
    for l in range(m.L):
        n = m.Np[l] * m.Kp[l]
        slabs = (m.S[l] if l == 0 else m.mid_groups) if m.fused else m.S[l]
        total += 4 * n * slabs + 2 * 4 * n * (3 if adam else 2) + 2 * 2 * n + (2 * n if l == 0 and m.W0f is not None else 0)
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=400, help="timed steps per model (>= 200)")
    ap.add_argument("--round", type=int, default=20, help="steps of one model before the next takes its turn")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rehearse", action="store_true", help="CPU emulation at batch 256, 4 steps: checks the script")
    a = ap.parse_args()
    dev = "cpu" if a.rehearse else "cuda"
    if a.rehearse:
        a.batch, a.steps, a.round, a.warmup = 256, 4, 2, 1
    elif a.steps < 200:
        ap.error("--steps must be at least 200")
    torch.manual_seed(0)
    X = torch.randint(0, 256, (a.batch, SIZES[0]), dtype=torch.uint8)
    labels = torch.randint(0, SIZES[-1], (a.batch,), dtype=torch.int32)
    models = {
        "bpm": MLP(SIZES, "SNN", batch=a.batch, device=dev, momentum=True, init="fast"),
        "bpm_3l": MLP(SIZES, "SNN", batch=a.batch, device=dev, momentum=True, init="fast"),
        "adam": MLP(SIZES, "SNN", batch=a.batch, device=dev, optimizer="adam", init="fast"),
    }
    models["bpm_3l"].plan.g0_fused = False
    inputs = {k: m.prepare_input(X) for k, m in models.items()}
    lab = labels.to(dev)
    if a.rehearse:  # the emulation takes dense targets
        T = torch.zeros(models["adam"].Bp, SIZES[-1])
        T[torch.arange(a.batch), labels.long()] = 1.0

    def step(k):
        if a.rehearse:
            models[k].train_step(inputs[k], T=T, n_valid=a.batch, lr=0.01, alpha=0.2)
        else:
            models[k].train_step(inputs[k], labels=lab, lr=0.01, alpha=0.2)

    for k in models:
        for _ in range(a.warmup):
            step(k)
    ms = {k: 0.0 for k in models}
    done = 0
    while done < a.steps:
        r = min(a.round, a.steps - done)
        for k in models:
            if a.rehearse:
                t0 = time.perf_counter()
                for _ in range(r):
                    step(k)
                ms[k] += 1e3 * (time.perf_counter() - t0)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(r):
                step(k)
            e1.record()
            e1.synchronize()
            ms[k] += e0.elapsed_time(e1)
        done += r
    out = {"sizes": SIZES, "batch": a.batch, "steps": a.steps, "device": dev, "mode": models["adam"].fused_mode,
           "S": models["adam"].S, "ms_per_step": {k: v / a.steps for k, v in ms.items()}}
    out["bpm_3l_minus_bpm_us"] = 1e3 * (out["ms_per_step"]["bpm_3l"] - out["ms_per_step"]["bpm"])
    out["adam_minus_bpm_3l_us"] = 1e3 * (out["ms_per_step"]["adam"] - out["ms_per_step"]["bpm_3l"])
    out["update_bytes"] = {"bpm_3l": update_bytes(models["bpm_3l"], False), "adam": update_bytes(models["adam"], True)}
    out["adam_launches_per_step"] = models["adam"].plan.adam_launches / (a.steps + a.warmup) if not a.rehearse else None
    for k, m in models.items():
        if not m.healthy():
            out["unhealthy"] = k
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
