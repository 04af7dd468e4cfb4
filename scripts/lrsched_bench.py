#!/usr/bin/env python3
"""Time the scheduled (unfused, device-rate) step beside the steps it replaces
(profiles/lr_schedule/README.md).

One process, models stepped in turn, round after round, so that clock and cache state are shared:

  mnist   784-128-64-10, mode t, batch 65 536, 8-bit pixels, BPM (bench.py's flagship shape)
            fused      the plan as it runs without a schedule: front, then G0 with every layer's
                       step in the same launch (2 launches)
            unfused    plan.g0_fused = False: front -> g0_reduce -> hpnn_sgd_update_multi (3)
            sched      lr_schedule constant: front -> g0_reduce -> hpnn_sgd_sched_multi (3)
  rruff   4096-230-230, mode w, batch 16 384, BPM
            fused      layer 0's step in its gradient launch, layer 1's as its side job
            sched      the gradients into slabs, then hpnn_sgd_sched_multi
  f32     the FP32 engine of train_nn on 784-128-64-10 (8192 samples, batch 1024, --epochs epochs),
          with and without [lr_schedule] constant: seconds of the training loop as train_nn prints
          them, three runs each in turn
  launch  the one-thread advance and plateau launches, back to back

Every model is warmed up, then timed with device events over --steps steps in rounds of --round.
Prints one JSON line.

    python scripts/lrsched_bench.py --steps 400
    python scripts/lrsched_bench.py --rehearse     # CPU: tiny shapes through the emulation, no timing claims
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpnn_amd import capi, ops  # noqa: E402
from hpnn_amd.models import MLP  # noqa: E402
from hpnn_amd.utils import formats  # noqa: E402

MNIST, RRUFF = [784, 128, 64, 10], [4096, 230, 230]
SCHED = dict(kind="constant", lr=0.01)


def time_models(models, step, steps, rnd, warmup, rehearse):
    for k in models:
        for _ in range(warmup):
            step(k)
    ms = {k: 0.0 for k in models}
    done = 0
    while done < steps:
        r = min(rnd, steps - done)
        for k in models:
            if rehearse:
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
    return {k: 1e3 * v / steps for k, v in ms.items()}  # us per step


def plan_case(sizes, batch, pixels, variants, a, dev):
    torch.manual_seed(0)
    if pixels:
        X = torch.randint(0, 256, (batch, sizes[0]), dtype=torch.uint8)
    else:
        X = torch.rand(batch, sizes[0]) * 2 - 1
    labels = torch.randint(0, sizes[-1], (batch,), dtype=torch.int32)
    models = {}
    for k in variants:
        models[k] = MLP(sizes, "SNN", batch=batch, device=dev, momentum=True, init="fast",
                        lr_schedule=SCHED if k == "sched" else None)
        if k == "unfused":
            models[k].plan.g0_fused = False
        if k == "sched":
            models[k].advance_schedule()
    inputs = {k: m.prepare_input(X) for k, m in models.items()}
    lab = labels.to(dev)
    T = None
    if a.rehearse:  # the emulation takes dense targets
        T = torch.zeros(models["sched"].Bp, sizes[-1])
        T[torch.arange(batch), labels.long()] = 1.0

    def step(k):
        if a.rehearse:
            models[k].train_step(inputs[k], T=T, n_valid=batch, lr=0.01, alpha=0.2)
        else:
            models[k].train_step(inputs[k], labels=lab, lr=0.01, alpha=0.2)

    us = time_models(models, step, a.steps, a.round, a.warmup, a.rehearse)
    out = {"sizes": sizes, "batch": batch, "mode": models["sched"].fused_mode, "S": models["sched"].S, "us_per_step": us}
    for k, m in models.items():
        if not m.healthy():
            out["unhealthy"] = k
    return out


def launch_case(a, dev):
    st = ops.lr_state("plateau", lr0=0.01, patience=2).to(dev)
    hist = torch.zeros(4, dtype=torch.float64, device=dev)
    cur = torch.zeros(1, dtype=torch.int32, device=dev)
    vh = torch.ones(4, 2, dtype=torch.float64, device=dev)
    vc = torch.ones(1, dtype=torch.int32, device=dev)
    calls = {"advance": lambda: ops.lr_advance(st, None, hist, cur), "plateau": lambda: ops.lr_plateau(vh, vc, st)}
    return time_models(calls, lambda k: calls[k](), 10 * a.steps, 10 * a.round, a.warmup, a.rehearse)


def f32_case(a):
    """train_nn -d f32 with and without [lr_schedule] constant, in turn; the seconds it prints"""
    n, B = (8192, 1024) if not a.rehearse else (64, 32)
    sizes = MNIST if not a.rehearse else [12, 8, 4]
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (n, sizes[0]))
    T = np.zeros((n, sizes[-1]))
    T[np.arange(n), rng.integers(0, sizes[-1], n)] = 1.0
    out = {"sizes": sizes, "n": n, "batch": B, "epochs": a.epochs, "seconds": {"plain": [], "sched": []}}
    with tempfile.TemporaryDirectory() as d:
        capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
        formats.write_conf(os.path.join(d, "nn.conf"), name="b", type="SNN", seed=1, inputs=sizes[0], hiddens=sizes[1:-1],
                           outputs=sizes[-1], train="BPM", sample_dir="./train.hpnb", test_dir="./train.hpnb",
                           mode="batched", batch=B, epochs=a.epochs, dtype="f32", lr=0.01)
        for _ in range(3):
            for k, extra in (("plain", []), ("sched", ["-L", "constant"])):
                cmd = [os.path.join(ROOT, "bin", "train_nn"), "-vv"] + (["-c"] if a.rehearse else []) + extra + ["nn.conf"]
                r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=600)
                m = re.search(r"BATCHED TRAINING: \d+ samples in ([0-9.]+) s", r.stdout)
                if r.returncode or not m:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                out["seconds"][k].append(float(m.group(1)))
    steps = a.epochs * ((n + B - 1) // B)
    out["us_per_step"] = {k: 1e6 * min(v) / steps for k, v in out["seconds"].items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=400, help="timed steps per model")
    ap.add_argument("--round", type=int, default=20, help="steps of one model before the next takes its turn")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=50, help="epochs of the f32 engine runs")
    ap.add_argument("--rehearse", action="store_true", help="CPU emulation at batch 256, 4 steps: checks the script")
    a = ap.parse_args()
    dev = "cpu" if a.rehearse else "cuda"
    if a.rehearse:
        a.steps, a.round, a.warmup, a.epochs = 4, 2, 1, 2
    out = {"device": dev, "steps": a.steps}
    out["mnist"] = plan_case(MNIST, 65536 if not a.rehearse else 256, True, ("fused", "unfused", "sched"), a, dev)
    out["rruff"] = plan_case(RRUFF, 16384 if not a.rehearse else 256, False, ("fused", "sched"), a, dev)
    out["launch_us"] = launch_case(a, dev)
    out["f32"] = f32_case(a)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
