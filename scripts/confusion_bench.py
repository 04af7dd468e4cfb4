"""What [confusion] costs on one MI355X (csrc/gpu/kernels_confusion.hip): the tally kernel alone,
and one validation pass of the Python plan with the key off and on.

  python scripts/confusion_bench.py [--rounds 5] [--root DIR] [--pass-only]

Part 1: hpnn_confusion_add on 65 536 rows, device-event time per launch (us) of `reps` launches
captured in one graph, median over rounds, the variants alternating: every row in one cell (the
worst contention: 65 536 atomic adds on one address) and uniformly random rows, int labels, at
n_out = 10, 63 and 230.
Part 2: one validation pass (evaluate + validate_commit; with the key on also the tally launches
and confusion_commit) over 10 000 held-out rows: the MNIST plan 784-128-64-10 (fused evaluation,
10 classes) and the RRUFF-shaped plan 4096-230-230 (per-layer evaluation, 230 classes), key off
and on alternating.  --root DIR imports hpnn_amd from another build (the parent commit: it has no
key, so only "off" is timed); --pass-only skips part 1.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--root", default=None)
ap.add_argument("--pass-only", action="store_true")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root) if ARGS.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpnn_amd import ops  # noqa: E402
from hpnn_amd.models import MLP  # noqa: E402


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


def report(tag, t, **extra):
    print(json.dumps({**tag, **{f"{k}_us": round(statistics.median(v), 3) for k, v in t.items()},
                      **{f"{k}_us_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}, **extra}),
          flush=True)


def tally(rounds, rows=65536):
    g = torch.Generator().manual_seed(1)
    for n_out in (10, 63, 230):
        for shape in ("one-cell", "uniform"):
            if shape == "one-cell":
                guess = torch.full((rows,), n_out - 1, dtype=torch.int32, device="cuda")
                lab = torch.zeros(rows, dtype=torch.int32, device="cuda")
            else:
                guess = torch.randint(0, n_out, (rows,), dtype=torch.int32, generator=g).cuda()
                lab = torch.randint(0, n_out, (rows,), dtype=torch.int32, generator=g).cuda()
            M = ops.confusion_matrix(n_out, "cuda")
            fns = {"add": lambda: ops.confusion_add(guess, M, labels=lab)}
            t = {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():
                    t[k].append(graph_time(fn, 50))
            report({"tally": shape, "n_out": n_out, "rows": rows}, t)


def validation_pass(rounds, name, sizes, batch, fused, nv=10000):
    n_out = sizes[-1]
    g = torch.Generator().manual_seed(2)
    m = MLP(sizes, "SNN", batch=batch, momentum=True, seed=3, fused=fused)
    X = m.prepare_input((torch.rand(nv, sizes[0], generator=g) - 0.5).cuda())
    lab = torch.randint(0, n_out, (nv,), dtype=torch.int32, generator=g).cuda()
    vst = m.buf[("vstats", -1)]
    hist = torch.zeros(1, 2, dtype=torch.float64, device="cuda")
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")
    has_key = hasattr(m, "confusion")

    def off():
        m.evaluate(X, labels=lab, n_valid=nv)
        ops.validate_commit(vst, hist, cur)

    def on():
        m.evaluate(X, labels=lab, n_valid=nv)
        m.commit_confusion(cur)
        ops.validate_commit(vst, hist, cur)

    t = {"off": []} if not has_key else {"off": [], "on": []}
    for _ in range(rounds):
        for k in t:
            if has_key:
                m.confusion(k == "on", passes=1)
            t[k].append(graph_time(on if k == "on" else off, 5))
    report({"pass": name, "held_out": nv, "classes": n_out, "fused_eval": bool(m.plan.eval_is_fused()), "root": ROOT}, t)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("confusion_bench: no GPU")
    if not ARGS.pass_only:
        tally(ARGS.rounds)
    validation_pass(ARGS.rounds, "mnist 784-128-64-10", [784, 128, 64, 10], 256, "t")
    validation_pass(ARGS.rounds, "rruff-shaped 4096-230-230", [4096, 230, 230], 256, False)


if __name__ == "__main__":
    main()
