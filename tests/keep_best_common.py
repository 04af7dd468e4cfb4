"""Shared pieces of the [keep_best] / [patience] tests: the four overfitting fixtures, the
improvement rule written out in Python, and the train_nn runner.

Every fixture comes from one recipe on numpy.default_rng(4): class prototypes P ~ U(lo, hi) per
class, X = P[class] + noise * N(0, 1) (clipped to [lo, hi]; fixture D rounded to k/255), and a
fraction of the labels redrawn at random.  The nets memorise the flipped labels of the small
training set, so the held-out loss has an interior minimum and rises from there."""
import os
import re
import subprocess

import numpy as np

from hpnn_amd import capi
from hpnn_amd.utils import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
SEED = 11
VAL_RE = re.compile(r"VALIDATION: epoch (\d+) loss=([0-9.eE+-]+|-?nan) acc=(\d+)/(\d+)")
BEST_RE = re.compile(r"BEST: epoch (\d+) loss=([0-9.eE+-]+) acc=(\d+)/(\d+)")
STOP_RE = re.compile(r"EARLY STOP: epoch (\d+) \(no improvement in (\d+) passes\)")

SMALL = [20, 16, 8, 5]
FIXTURES = {
    "A": dict(sizes=SMALL, n=37, nv=23, lo=-1.0, hi=1.0, noise=0.6, flip=0.25, B=8, epochs=24, lr=0.5),
    "B": dict(sizes=SMALL, n=150, nv=90, lo=-1.0, hi=1.0, noise=0.6, flip=0.25, B=32, epochs=24, lr=1.0),
    "C": dict(sizes=SMALL, n=37, nv=23, lo=-1.0, hi=1.0, noise=0.6, flip=0.25, B=64, epochs=32, lr=2.0),
    "D": dict(sizes=[784, 128, 64, 10], n=600, nv=300, lo=0.0, hi=1.0, noise=0.5, flip=0.3, B=256, epochs=16,
              lr=1.0, pixels=True),
}


def make_fixture(d, name):
    """write train.hpnb / val.hpnb of fixture `name` into d and a conf per call of conf()"""
    f = FIXTURES[name]
    n_in, n_out = f["sizes"][0], f["sizes"][-1]
    rng = np.random.default_rng(4)
    P = rng.uniform(f["lo"], f["hi"], (n_out, n_in))
    for fn, n in (("train.hpnb", f["n"]), ("val.hpnb", f["nv"])):
        cls = rng.integers(0, n_out, n)
        X = np.clip(P[cls] + f["noise"] * rng.standard_normal((n, n_in)), f["lo"], f["hi"])
        if f.get("pixels"):
            X = np.round(X * 255.0) / 255.0
        lab = np.where(rng.random(n) < f["flip"], rng.integers(0, n_out, n), cls)
        T = np.zeros((n, n_out))
        T[np.arange(n), lab] = 1.0
        capi.pack_arrays(os.path.join(d, fn), X, T)
    return f


def write_conf(d, name, dtype="f64", data=None, **extra):
    f = FIXTURES[name]
    data = data or d
    kw = dict(mode="batched", batch=f["B"], epochs=f["epochs"], lr=f["lr"], dtype=dtype)
    kw.update(extra)
    formats.write_conf(os.path.join(d, "nn.conf"), name="kb", type="SNN", seed=SEED, inputs=f["sizes"][0],
                       hiddens=f["sizes"][1:-1], outputs=f["sizes"][-1], train="BPM",
                       sample_dir=os.path.join(data, "train.hpnb"), test_dir=os.path.join(data, "val.hpnb"), **kw)


def run(d, *flags, cpu=True, env=None, tool="train_nn", check=True):
    e = dict(os.environ, HPNN_KERNEL_EXACT="1")
    if not cpu:
        e.pop("HPNN_FORCE_CPU", None)
    e.update(env or {})
    cmd = [os.path.join(BIN, tool)] + (["-c"] if cpu else []) + ["-vv", *flags, "nn.conf"]
    r = subprocess.run(cmd, cwd=d, env=e, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def records(out):
    return [(int(e), float(l), int(c), int(n)) for e, l, c, n in VAL_RE.findall(out)]


def kernel(d):
    return open(os.path.join(d, "kernel.opt"), "rb").read()


def rule(recs, metric="loss", patience=0):
    """the improvement rule on (epoch, loss, hits, n) records: (index of the best pass or None,
    index of the stopping pass or None).  loss: strictly smaller; acc: more hits, the loss
    breaking ties; the first pass is taken (under loss: the first whose loss is not a NaN); an
    improving pass zeroes stale, any other adds one; stale == patience stops."""
    best, stale = None, 0
    for i, (_, loss, hits, _) in enumerate(recs):
        if best is None:
            better = metric == "acc" or loss == loss
        elif metric == "acc":
            better = hits > recs[best][2] or (hits == recs[best][2] and loss < recs[best][1])
        else:
            better = loss < recs[best][1]
        if better:
            best, stale = i, 0
        else:
            stale += 1
        if patience and stale == patience:
            return best, i
    return best, None


def check_interior(name, recs, metric="loss", patience=0, need_stop=False):
    """the fixture's precondition: the best pass is neither the first nor the last one, it is
    clear of the runner-up beyond the ten printed decimals, and (need_stop) patience stops the
    run before its last pass"""
    b, s = rule(recs, metric, patience)
    last = len(recs) - 1
    assert b is not None and 1 <= b < last, \
        f"fixture {name}, not the feature, is at fault: best pass {b} of 0..{last} is not interior: {recs}"
    if metric == "loss":
        others = sorted(r[1] for i, r in enumerate(recs) if i != b)
        assert others[0] - recs[b][1] > 1e-9, f"fixture {name} is at fault: the best loss is not clear of the rest"
    if need_stop:
        assert s is not None and s < last, \
            f"fixture {name}, not the feature, is at fault: patience {patience} does not stop before the end: {recs}"
    return b, s
