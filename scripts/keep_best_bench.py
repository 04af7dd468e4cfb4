"""What [keep_best] costs on one MI355X: the two launches it adds behind every validation pass
(hpnn_best_commit, hpnn_snapshot_if; csrc/gpu/kernels_best.hip) timed alone, and train_nn
-V 1 with -K loss against the same run without it, interleaved.

  python scripts/keep_best_bench.py [--rounds 3] [--epochs 50] [--parent DIR] [--skip-train]

Part 1, per net (MNIST 784-128-64-10 and the synthetic 8 x 4096, FP32 masters + momentum):
`reps` passes captured in one graph, device-event time per pass (us), median over rounds, the
variants alternating:
  empty2      two empty one-thread launches (the yardstick for a pass that copies nothing)
  flag0       best_commit + snapshot_if on a pass that does not improve (flag 0)
  flag1       best_commit + snapshot_if on a pass that improves (flag 1: the copy runs)
  copy        snapshot_if alone with the flag set (bytes / time = the copy's rate)
Part 2: a 60 000 x 784 MNIST-shaped set (8-bit prototypes plus noise, 10 000 held out), SNN
784-128-64-10 BPM bf16, B 4096, -V 1: seconds of the BATCHED TRAINING line for -K loss on, off,
and (--parent DIR: a build of the parent commit) the parent's train_nn, `rounds` rounds
alternating.  One JSON line per measurement."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpnn_amd import capi, ops  # noqa: E402
from hpnn_amd._lib import native  # noqa: E402
from hpnn_amd.utils import formats  # noqa: E402


def stream():
    return torch.cuda.current_stream().cuda_stream


def graph_time(fn, reps, iters=20):
    """us per call of fn, `reps` calls captured in one graph, `iters` replays timed"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (iters * reps)


def launches(name, shapes, rounds, reps):
    src = [torch.rand(s, device="cuda") for s in shapes for _ in range(2)]  # masters and momentum
    dst = [torch.empty_like(t) for t in src]
    table = ops.snapshot_table(list(zip(src, dst)))
    nbytes = sum(t.numel() * 4 for t in src)
    hist = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    hist[:, 0] = torch.tensor([5.0, 5.0, 5.0, 5.0])
    cur = torch.ones(1, dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    nat = native()

    def empty2():
        nat.best_empty_launch(stream())
        nat.best_empty_launch(stream())

    def state(valid):
        st = ops.best_state("cuda")
        if valid:  # a best of 5.0 is held: another 5.0 is a tie, flag 0
            ops.best_commit(hist, cur, st, "loss", 0)
        return st

    st0 = state(True)

    def flag0():
        ops.best_commit(hist, cur, st0, "loss", 0)
        ops.snapshot_if(table, st0[7:8])

    # flag 1 on every pass: metric acc takes the first pass; valid is cleared behind the copy
    st1 = state(False)

    def flag1():
        ops.best_commit(hist, cur, st1, "acc", 0)
        ops.snapshot_if(table, st1[7:8])
        st1[6:7].zero_()

    def zero_only():
        st1[6:7].zero_()

    def copy():
        ops.snapshot_if(table, one)

    fns = dict(empty2=empty2, flag0=flag0, flag1=flag1, zero_only=zero_only, copy=copy)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(graph_time(fn, reps))
    assert int(st0.cpu()[7]) == 0 and all(torch.equal(a, b) for a, b in zip(src, dst))
    med = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps({"net": name, "snapshot_bytes": nbytes, "segments": len(src), "reps_per_graph": reps,
                      **{f"{k}_us": round(v, 3) for k, v in med.items()},
                      **{f"{k}_us_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
                      "flag1_minus_zero_us": round(med["flag1"] - med["zero_only"], 3),
                      "copy_GBps_read_plus_write": round(2 * nbytes / med["copy"] / 1e3, 1)}), flush=True)


TRAIN_RE = re.compile(r"BATCHED TRAINING: (\d+) samples in ([0-9.]+) s")
VAL_RE = re.compile(r"VALIDATION: epoch (\d+) loss=([0-9.eE+-]+) acc=(\d+)/(\d+)")


def training(rounds, epochs, parent):
    rng = np.random.default_rng(4)
    with tempfile.TemporaryDirectory() as d:
        P = rng.integers(0, 256, (10, 784)).astype(np.float64)
        for fn, n in (("train.hpnb", 60000), ("val.hpnb", 10000)):
            cls = rng.integers(0, 10, n)
            X = np.clip(np.rint(P[cls] + 64.0 * rng.standard_normal((n, 784))), 0, 255)
            lab = np.where(rng.random(n) < 0.1, rng.integers(0, 10, n), cls)
            T = np.zeros((n, 10))
            T[np.arange(n), lab] = 1.0
            capi.pack_arrays(os.path.join(d, fn), X, T)
        formats.write_conf(os.path.join(d, "nn.conf"), name="kb", type="SNN", seed=10958, inputs=784,
                           hiddens=[128, 64], outputs=10, train="BPM", sample_dir="./train.hpnb",
                           test_dir="./val.hpnb", mode="batched", batch=4096, epochs=epochs, dtype="bf16")
        variants = [("K_on", ROOT, ["-K", "loss"]), ("K_off", ROOT, [])]
        if parent:
            variants.append(("parent", os.path.abspath(parent), []))
        secs = {v[0]: [] for v in variants}
        info = {}
        for r in range(rounds):
            for tag, root, flags in variants:
                out = subprocess.run([os.path.join(root, "bin", "train_nn"), "-vv", "-V", "1", *flags, "nn.conf"],
                                     cwd=d, capture_output=True, text=True, timeout=600, check=True).stdout
                secs[tag].append(float(TRAIN_RE.search(out).group(2)))
                recs = [(float(l), int(c)) for _, l, c, _ in VAL_RE.findall(out)]
                best, improving = None, 0
                for loss, _ in recs:
                    if best is None or loss < best:
                        best, improving = loss, improving + 1
                info[tag] = {"records": len(recs), "improving_passes": improving,
                             "best_line": (re.findall(r"BEST: .*", out) or [None])[0],
                             "last_record": VAL_RE.findall(out)[-1] if recs else None}
        for tag in secs:
            print(json.dumps({"train": tag, "epochs": epochs, "seconds": secs[tag],
                              "median_s": statistics.median(secs[tag]), **info[tag]}), flush=True)
        on, off = statistics.median(secs["K_on"]), statistics.median(secs["K_off"])
        print(json.dumps({"K_on_minus_K_off_us_per_epoch": round((on - off) / epochs * 1e6, 2),
                          "epoch_us_K_off": round(off / epochs * 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("keep_best_bench: no GPU")
    launches("mnist 784-128-64-10", [(128, 800), (64, 128), (32, 64)], a.rounds, 200)
    launches("synthetic 8 x 4096", [(4096, 4096)] * 8, a.rounds, 10)
    if not a.skip_train:
        training(a.rounds, a.epochs, a.parent)


if __name__ == "__main__":
    main()
