"""Shared pieces of the [confusion] tests: the rule of include/libhpnn/confusion.h written out in
numpy (first-maximum target, the cell rule, the per-class record, balanced accuracy in the stated
operation order), the hand-made rule cases, the two small seeded nets and the train_nn / run_nn
plumbing.

Every expected value is an integer count, so every comparison in these tests is exact."""
import json
import os
import re

import numpy as np
import torch

from hpnn_amd import capi
from hpnn_amd.models import reference
from hpnn_amd.utils import formats
from tests import keep_best_common as kb

GUESS_PAD, GUESS_NONE = -1, 1 << 30
CLASSES_RE = re.compile(r"CLASSES: epoch (\d+) bacc=([0-9.]+) worst=(-?\d+) recall=(\d+)/(\d+)")
RUN_RE = re.compile(r"\[(PASS)\]|\[FAIL idx=(\d+)\]")
BESTCLASS_RE = re.compile(r"BEST CLASS idx=(\d+)")


# ------------------------------------------------------------------ the rule in numpy
def target_class(T):
    """the lowest index of the largest value of every row, the serial rule: tr = 0, then t[i] >
    t[tr] moves tr (a NaN never compares)"""
    T = np.asarray(T)
    out = np.zeros(T.shape[0], dtype=np.int64)
    for r in range(T.shape[0]):
        tr = 0
        for i in range(1, T.shape[1]):
            if T[r, i] > T[r, tr]:
                tr = i
        out[r] = tr
    return out


def matrix(guess, target, n_out, M=None):
    """M[t, g] += 1 per row; guess < 0: not a sample; guess >= n_out: the "none" column n_out; a
    target outside [0, n_out): the row is skipped"""
    M = np.zeros((n_out, n_out + 1), dtype=np.uint32) if M is None else M
    for g, t in zip(np.asarray(guess).tolist(), np.asarray(target).tolist()):
        if g < 0 or t < 0 or t >= n_out:
            continue
        M[t, min(g, n_out)] += 1
    return M


def class_record(M):
    n = M.shape[0]
    return {"support": M.sum(1, dtype=np.uint32), "hit": np.diagonal(M).astype(np.uint32),
            "predicted": M[:, :n].sum(0, dtype=np.uint32)}


def balanced_accuracy(support, hit):
    total, classes = np.float64(0.0), np.float64(0.0)
    for s, h in zip(support, hit):
        if int(s):
            total = total + np.float64(int(h)) / np.float64(int(s))
            classes = classes + np.float64(1.0)
    return float(total / classes) if classes > 0 else 0.0


def worst_class(support, hit):
    w = -1
    for c, (s, h) in enumerate(zip(support, hit)):
        if int(s) and (w < 0 or int(h) * int(support[w]) < int(hit[w]) * int(s)):
            w = c
    return w


# ------------------------------------------------------------------ hand-made rule cases
# (name, n_out, guess, dense targets, expected matrix rows)
RULE_CASES = [
    ("ties in the target row", 3,
     [0, 1, 2, 2],
     [[1.0, 1.0, 0.0], [0.0, 0.5, 0.5], [0.2, 0.2, 0.2], [0.0, 0.0, 1.0]],
     [[1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 1, 0]]),
    ("a class without support", 4,
     [0, 0, 3, 1],
     [[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1]],
     [[2, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 1, 0, 1, 0]]),
    ("a none guess and a pad row", 2,
     [GUESS_NONE, 1, GUESS_PAD, 0],
     [[0, 1], [0, 1], [1, 0], [1, 0]],
     [[1, 0, 0], [0, 1, 1]]),
    ("NaN targets never compare", 3,
     [1, 1, 1],
     [[float("nan"), 5.0, 1.0], [0.0, float("nan"), 1.0], [float("-inf"), float("-inf"), float("-inf")]],
     [[0, 2, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]),
]


def read_matrix_file(path):
    """the -X file: "# n_out", then one row of n_out + 1 counts per target class"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# "), lines[:2]
    n = int(lines[0][2:])
    M = np.array([[int(v) for v in ln.split(" ")] for ln in lines[1:-1]], dtype=np.uint32)
    assert M.shape == (n, n + 1), (M.shape, n)
    return M


# ------------------------------------------------------------------ the two small nets
SEED = 7
NETS = {
    # one-hot targets: the engines take their label form
    "S": dict(type="SNN", sizes=[16, 12, 4], n=53, nv=37, B=16, lr=0.6, onehot=True),
    # soft dense targets (0.8 at the class, the rest spread unevenly): the dense form everywhere
    "L": dict(type="LNN", sizes=[33, 17, 5], n=61, nv=45, B=16, lr=0.05, onehot=False),
}


def make_net(d, name):
    """train.hpnb / val.hpnb of net `name` in d; returns (f, Xv, Tv)"""
    f = NETS[name]
    n_in, n_out = f["sizes"][0], f["sizes"][-1]
    rng = np.random.default_rng(23)
    P = rng.uniform(-1.0, 1.0, (n_out, n_in))
    held = None
    for fn, n in (("train.hpnb", f["n"]), ("val.hpnb", f["nv"])):
        cls = rng.integers(0, n_out, n)
        X = np.clip(P[cls] + 0.7 * rng.standard_normal((n, n_in)), -1.0, 1.0)
        if f["onehot"]:
            T = np.zeros((n, n_out))
            T[np.arange(n), cls] = 1.0
        else:
            T = 0.05 * rng.random((n, n_out))
            T[np.arange(n), cls] = 0.8
        capi.pack_arrays(os.path.join(d, fn), X, T)
        held = (X, T)
    return f, held[0], held[1]


def write_conf(d, name, dtype="f64", epochs=4, **extra):
    f = NETS[name]
    kw = dict(mode="batched", batch=f["B"], epochs=epochs, lr=f["lr"], dtype=dtype)
    kw.update(extra)
    formats.write_conf(os.path.join(d, "nn.conf"), name="cf", type=f["type"], seed=SEED, inputs=f["sizes"][0],
                       hiddens=f["sizes"][1:-1], outputs=f["sizes"][-1], train="BPM",
                       sample_dir=os.path.join(d, "train.hpnb"), test_dir=os.path.join(d, "val.hpnb"), **kw)


run = kb.run


def oracle_outputs(d, name, Xv):
    """the held-out outputs of d/kernel.opt (written with %.17g) through the FP64 PyTorch forward"""
    k = formats.read_kernel(os.path.join(d, "kernel.opt"))
    W = [torch.tensor(np.asarray(w), dtype=torch.float64) for w in k["weights"]]
    return reference.forward(W, torch.tensor(Xv, dtype=torch.float64), NETS[name]["type"])[-1].numpy()


def top2_gap(O):
    s = np.sort(O, axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def oracle_matrix(d, name, Xv, Tv, gap=1e-9):
    """the matrix numpy builds from the independent forward; the fixture's precondition: every
    sample's two largest outputs differ by more than `gap`, so a summation order cannot move a guess"""
    O = oracle_outputs(d, name, Xv)
    assert top2_gap(O) > gap, f"fixture {name}, not the feature, is at fault: a near tie among the outputs"
    return matrix(O.argmax(1), target_class(Tv), O.shape[1])


def keep_best_held_out(name):
    """the held-out arrays (X, labels) kb.make_fixture(d, name) packs into val.hpnb: the same draws
    from the same generator, in the same order"""
    f = kb.FIXTURES[name]
    n_in, n_out = f["sizes"][0], f["sizes"][-1]
    rng = np.random.default_rng(4)
    P = rng.uniform(f["lo"], f["hi"], (n_out, n_in))
    for n in (f["n"], f["nv"]):
        cls = rng.integers(0, n_out, n)
        X = np.clip(P[cls] + f["noise"] * rng.standard_normal((n, n_in)), f["lo"], f["hi"])
        if f.get("pixels"):
            X = np.round(X * 255.0) / 255.0
        lab = np.where(rng.random(n) < f["flip"], rng.integers(0, n_out, n), cls)
    return X, lab


def classes_events(path):
    return [json.loads(ln) for ln in open(path) if '"event": "classes"' in ln]
