#!/usr/bin/env python3
"""Time one [train] CG iteration beside one BP epoch of the same conf (profiles/cg/README.md).

Writes an MNIST-shaped synthetic pack (n x 784 pixels k/255, 10 classes), runs bin/train_nn
twice in child processes -- [train] CG for --cg-epochs and [train] BP for --bp-epochs -- and reads
the training-loop seconds from the "BATCHED TRAINING:" line (data upload, layout conversion and
graph capture are outside it).  Prints one JSON line.

    python scripts/cg_bench.py --n 60000 --batch 4096 --dtype f32
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpnn_amd import capi  # noqa: E402
from hpnn_amd.utils import formats  # noqa: E402

LINE = re.compile(r"BATCHED TRAINING: (\d+) samples in ([0-9.]+) s")


def launches(n, batch, layers):
    """launches of one CG iteration and of one BP epoch, from the launch sequences of
    BatchedFP::iterate_cg and BatchedFP::step (csrc/gpu/batched_net.h)"""
    nb = (n + batch - 1) // batch
    grad = layers + 1 + (layers - 1) + layers + 1 + 1  # forward, output, deltas, gradients, loss, accumulate
    search = 7 * (nb * (layers + 1) + 1) + 8           # seven passes (forward + loss, file) and eight steps
    return nb * grad + 5 + search, nb * (layers + 1 + (layers - 1) + layers + layers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--hidden", type=int, nargs="*", default=[128, 64])
    ap.add_argument("--cg-epochs", type=int, default=4)
    ap.add_argument("--bp-epochs", type=int, default=12)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    out = {"n": a.n, "batch": a.batch, "dtype": a.dtype, "sizes": [784] + a.hidden + [10]}
    with tempfile.TemporaryDirectory() as d:
        P = rng.uniform(0.0, 1.0, (10, 784))
        cls = rng.integers(0, 10, a.n)
        X = np.round(np.clip(P[cls] + 0.3 * rng.standard_normal((a.n, 784)), 0.0, 1.0) * 255.0) / 255.0
        T = np.zeros((a.n, 10))
        T[np.arange(a.n), cls] = 1.0
        capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
        for train, epochs in (("CG", a.cg_epochs), ("BP", a.bp_epochs)):
            formats.write_conf(os.path.join(d, "nn.conf"), name="cgb", type="SNN", seed=10958, inputs=784,
                               hiddens=a.hidden, outputs=10, train=train, sample_dir="./train.hpnb",
                               test_dir="./train.hpnb", mode="batched", batch=a.batch, epochs=epochs, lr=0.1,
                               dtype=a.dtype)
            r = subprocess.run([os.path.join(ROOT, "bin", "train_nn"), "-vv", "-x", "nn.conf"], cwd=d,
                               capture_output=True, text=True, timeout=a.timeout)
            m = LINE.search(r.stdout)
            if r.returncode != 0 or not m:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                return 1
            out[train] = {"epochs": epochs, "seconds": float(m.group(2)), "ms_per_epoch": 1e3 * float(m.group(2)) / epochs}
            if train == "CG":
                out["CG"]["records"] = re.findall(r"CG: epoch \d+ (.*)", r.stdout)
    cg, bp = launches(a.n, a.batch, len(a.hidden) + 1)
    out["launches"] = {"cg_iteration": cg, "bp_epoch": bp}
    out["cg_over_bp"] = out["CG"]["ms_per_epoch"] / out["BP"]["ms_per_epoch"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
