#!/usr/bin/env python3
"""Time the clipped step beside the scheduled (unfused, device-rate) step it is built on
(profiles/clip/README.md).

One process, models stepped in turn, round after round, so that clock and cache state are shared:

  mnist   784-128-64-10, mode t, batch 65 536, 8-bit pixels, BPM (bench.py's flagship shape)
            sched      lr_schedule constant: front -> g0_reduce -> hpnn_sgd_sched_multi (3 launches)
            clip       clip: front -> g0_reduce -> hpnn_gnorm_partials -> hpnn_clip_finalize_dev ->
                       hpnn_sgd_sched_multi with the factor (5 launches)
  rruff   4096-230-230, mode w, batch 16 384, BPM: sched and clip
  f32     the FP32 engine of train_nn on 784-128-64-10 (8192 samples, batch 1024, --epochs epochs),
          -L constant against -C: seconds of the training loop as train_nn prints them, three runs
          each in turn
  launch  hpnn_gnorm_partials over the MNIST plan's slabs, the finalize and the commit, back to back

--root DIR times the package and the train_nn of another checkout (the parent commit's build, which
knows --variants sched only): the parent's scheduled step on the same machine.

Every model is warmed up, then timed with device events over --steps steps in rounds of --round.
Prints one JSON line.

    python scripts/clip_bench.py --steps 400
    python scripts/clip_bench.py --steps 400 --root ../parent --variants sched
    python scripts/clip_bench.py --rehearse     # CPU: tiny shapes through the emulation, no timing claims
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

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MNIST, RRUFF = [784, 128, 64, 10], [4096, 230, 230]
SCHED = dict(kind="constant", lr=0.01)
CLIP = 1.0


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


def plan_case(MLP, ops, sizes, batch, pixels, variants, a, dev):
    torch.manual_seed(0)
    if pixels:
        X = torch.randint(0, 256, (batch, sizes[0]), dtype=torch.uint8)
    else:
        X = torch.rand(batch, sizes[0]) * 2 - 1
    labels = torch.randint(0, sizes[-1], (batch,), dtype=torch.int32)
    models = {}
    for k in variants:
        kw = dict(lr_schedule=SCHED) if k == "sched" else dict(clip=CLIP, lr=0.01)
        models[k] = MLP(sizes, "SNN", batch=batch, device=dev, momentum=True, init="fast", **kw)
        if k == "sched":
            models[k].advance_schedule()
    inputs = {k: m.prepare_input(X) for k, m in models.items()}
    lab = labels.to(dev)
    T = None
    first = models[variants[0]]
    if a.rehearse:  # the emulation takes dense targets
        T = torch.zeros(first.Bp, sizes[-1])
        T[torch.arange(batch), labels.long()] = 1.0

    def step(k):
        if a.rehearse:
            models[k].train_step(inputs[k], T=T, n_valid=batch, lr=0.01, alpha=0.2)
        else:
            models[k].train_step(inputs[k], labels=lab, lr=0.01, alpha=0.2)

    us = time_models(models, step, a.steps, a.round, a.warmup, a.rehearse)
    out = {"sizes": sizes, "batch": batch, "mode": first.fused_mode, "S": first.S, "us_per_step": us}
    if "clip" in models:
        if dev == "cuda":
            torch.cuda.synchronize()
        r = ops.read_clip_state(models["clip"].clip_state)
        out["clip_state"] = {k: r[k] for k in ("norm", "factor", "steps", "clipped")}
        out["partials"] = models["clip"].plan.clip_count
    for k, m in models.items():
        if not m.healthy():
            out["unhealthy"] = k
    return out


def launch_case(MLP, ops, a, dev):
    """the three launches of kernels_clip.hip alone, over the slabs of the MNIST plan"""
    m = MLP(MNIST, "SNN", batch=65536 if not a.rehearse else 256, device=dev, momentum=True, init="fast", clip=CLIP,
            lr=0.01)
    tab = ops.GnormTable([m.slab[l].reshape(m.slab[l].shape[0], -1) for l in range(m.L)], interleaved=True)
    part = torch.zeros(tab.count, dtype=torch.float64, device=dev)
    st = ops.clip_state(CLIP).to(dev)
    hist, cur = ops.clip_history(4, dev)
    calls = {"partials": lambda: ops.gnorm_partials(tab, part, 1.0 / 65536),
             "finalize": lambda: ops.clip_finalize(part, tab.count, st),
             "commit": lambda: ops.clip_commit(st, hist, cur)}
    return time_models(calls, lambda k: calls[k](), 10 * a.steps, 10 * a.round, a.warmup, a.rehearse)


def f32_case(capi, formats, root, variants, a):
    """train_nn -d f32 under -L constant and under -C, in turn; the seconds it prints"""
    n, B = (8192, 1024) if not a.rehearse else (64, 32)
    sizes = MNIST if not a.rehearse else [12, 8, 4]
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (n, sizes[0]))
    T = np.zeros((n, sizes[-1]))
    T[np.arange(n), rng.integers(0, sizes[-1], n)] = 1.0
    flags = {"sched": ["-L", "constant"], "clip": ["-C", str(CLIP)]}
    out = {"sizes": sizes, "n": n, "batch": B, "epochs": a.epochs, "seconds": {k: [] for k in variants}}
    with tempfile.TemporaryDirectory() as d:
        capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
        formats.write_conf(os.path.join(d, "nn.conf"), name="b", type="SNN", seed=1, inputs=sizes[0],
                           hiddens=sizes[1:-1], outputs=sizes[-1], train="BPM", sample_dir="./train.hpnb",
                           test_dir="./train.hpnb", mode="batched", batch=B, epochs=a.epochs, dtype="f32", lr=0.01)
        for _ in range(3):
            for k in variants:
                cmd = [os.path.join(root, "bin", "train_nn"), "-vv"] + (["-c"] if a.rehearse else []) + flags[k]
                cmd.append("nn.conf")
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
    ap.add_argument("--root", default=HERE, help="the checkout whose package and train_nn are timed")
    ap.add_argument("--variants", default="sched,clip", help="sched, clip or both")
    ap.add_argument("--rehearse", action="store_true", help="CPU emulation at batch 256, 4 steps: checks the script")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from hpnn_amd import capi, ops
    from hpnn_amd.models import MLP
    from hpnn_amd.utils import formats
    variants = tuple(a.variants.split(","))
    dev = "cpu" if a.rehearse else "cuda"
    if a.rehearse:
        a.steps, a.round, a.warmup, a.epochs = 4, 2, 1, 2
    out = {"device": dev, "steps": a.steps, "root": os.path.relpath(root, HERE), "variants": variants}
    out["mnist"] = plan_case(MLP, ops, MNIST, 65536 if not a.rehearse else 256, True, variants, a, dev)
    out["rruff"] = plan_case(MLP, ops, RRUFF, 16384 if not a.rehearse else 256, False, variants, a, dev)
    if "clip" in variants:
        out["launch_us"] = launch_case(MLP, ops, a, dev)
    out["f32"] = f32_case(capi, formats, root, variants, a)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
