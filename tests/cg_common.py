"""Shared pieces of the [train] CG tests: the two fixtures, the in-process trainer, the FP64 /
FP32 PyTorch reference runs and the preconditions on them.

A fixture is one recipe on numpy.default_rng(data seed): class prototypes P ~ U(-1, 1), X =
P[class] + 0.6 N(0, 1) clipped to [-1, 1], 20 % of the labels redrawn at random; the targets are
one-hot (the other entries 0 for SNN, -1 for ANN).  The data seeds were picked so that every one
of the ten iterations of the FP64 reference takes its decisions with room to spare (check_gaps):
an engine that differs from the reference by rounding then takes the same ones."""
import ctypes
import ctypes.util
import os

import numpy as np
import torch

from hpnn_amd import capi
from hpnn_amd.models import reference
from hpnn_amd.utils import formats

ITERS = 10
SEED = 11  # [seed]: the initial weights and the sample order
LR = 0.5   # the first a_init
GAP = 1e-4
NETS = {
    "8-6-4": dict(sizes=[8, 6, 4], n=100, nv=40, B=32),        # four chunks, the last of 4 rows
    "20-16-12-5": dict(sizes=[20, 16, 12, 5], n=70, nv=30, B=128),  # B >= n
}
DATA_SEED = {("8-6-4", "ANN"): 5, ("8-6-4", "SNN"): 1, ("20-16-12-5", "ANN"): 4, ("20-16-12-5", "SNN"): 2}
FAILING = ("20-16-12-5", "SNN", 1)  # a data seed whose third iteration overshoots: a failed search, then a restart
CASES = [(net, t) for net in NETS for t in ("ANN", "SNN")]


def order(n, seed=SEED):
    """nn_train_kernel's seeded sample order"""
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.random.restype = ctypes.c_long
    libc.srandom(ctypes.c_uint(seed))
    used, out = set(), []
    while len(out) < n:
        idx = int(float(libc.random()) * n / 2147483647.0)
        if idx >= n or idx in used:
            continue
        used.add(idx)
        out.append(idx)
    return out


def make_data(d, net, net_type, data_seed=None):
    """write train.hpnb / val.hpnb into d; returns X, T, Xv, Tv (float64 numpy)"""
    f = NETS[net]
    n_in, n_out = f["sizes"][0], f["sizes"][-1]
    rng = np.random.default_rng(DATA_SEED[(net, net_type)] if data_seed is None else data_seed)
    P = rng.uniform(-1.0, 1.0, (n_out, n_in))
    out = []
    for fn, n in (("train.hpnb", f["n"]), ("val.hpnb", f["nv"])):
        cls = rng.integers(0, n_out, n)
        X = np.clip(P[cls] + 0.6 * rng.standard_normal((n, n_in)), -1.0, 1.0)
        lab = np.where(rng.random(n) < 0.2, rng.integers(0, n_out, n), cls)
        T = np.full((n, n_out), 0.0 if net_type == "SNN" else -1.0)
        T[np.arange(n), lab] = 1.0
        capi.pack_arrays(os.path.join(d, fn), X, T)
        out += [X, T]
    return out


def write_conf(d, net, net_type, dtype="f64", train="CG", **extra):
    f = NETS[net]
    kw = dict(mode="batched", batch=f["B"], epochs=ITERS, lr=LR, dtype=dtype)
    kw.update(extra)
    formats.write_conf(os.path.join(d, "nn.conf"), name="cg", type=net_type, seed=SEED, inputs=f["sizes"][0],
                       hiddens=f["sizes"][1:-1], outputs=f["sizes"][-1], train=train,
                       sample_dir=os.path.join(d, "train.hpnb"), test_dir=os.path.join(d, "val.hpnb"), **kw)


def weights_of(net, d, name):
    p = os.path.join(d, name)
    net.dump_kernel(p, exact=True)
    return [np.array(w, dtype=np.float64) for w in formats.read_kernel(p)["weights"]]


def train(d, device="cpu", env=None, **set_kw):
    """train nn.conf of d in this process; returns a dict: ok, w0, w (lists of float64 arrays),
    hist (Network.cg_history()), val (validation records), best, epochs_done"""
    capi.init(0)
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        net = capi.Network(os.path.join(d, "nn.conf"))
        net.set(device=device, **set_kw)
        w0 = weights_of(net, d, "k0.opt")
        ok = net.train()
        out = dict(ok=ok, w0=w0, w=weights_of(net, d, "k1.opt"), hist=net.cg_history(), val=net.validation(),
                   best=net.best(), epochs_done=net.epochs_done)
        net.close()
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def reference_run(w0, X, T, net_type, B, iters=ITERS, perm=None, dtype=torch.float64, lr=LR):
    """`iters` iterations of reference.cg_iteration from w0 on the samples in the seeded order
    (perm: a further permutation of them, which changes only summation orders); returns
    (records, weights as float64 arrays)"""
    o = np.array(order(X.shape[0]))
    if perm is not None:
        o = o[perm]
    Xo, To = torch.tensor(X[o], dtype=dtype), torch.tensor(T[o], dtype=dtype)
    W = [torch.tensor(w, dtype=dtype) for w in w0]
    st = reference.cg_state(W, lr)
    recs = [reference.cg_iteration(W, Xo, To, net_type, st, batch=B) for _ in range(iters)]
    return recs, [w.double().numpy() for w in W]


def spread(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b))


def order_spread(w0, X, T, net_type, B, dtype=torch.float64, iters=ITERS):
    """the largest weight difference between two reference runs that differ only in the sample
    order: the size of a legitimate summation-order effect after `iters` iterations"""
    n = X.shape[0]
    _, wa = reference_run(w0, X, T, net_type, B, iters, None, dtype)
    _, wb = reference_run(w0, X, T, net_type, B, iters, np.random.default_rng(5).permutation(n), dtype)
    return spread(wa, wb)


def check_gaps(recs, who):
    """the fixture's precondition, on the reference alone: at every iteration the best trial is
    clear of the second best, the seventh trial of b (when it is another point) and f0 of the best
    trial, each by more than GAP relative -- far above FP32 rounding of a mean loss"""
    for i, r in enumerate(recs):
        assert r["trial"] is not None and not r["flags"] & reference.CG_FAILED, f"{who}: iteration {i} failed: {r}"
        phi = r["phi"][:reference.CG_TRIALS]
        best = phi[r["trial"]]
        second = min(p for j, p in enumerate(phi) if j != r["trial"])
        assert (second - best) / best > GAP, f"fixture {who} is at fault: iteration {i}, best vs second best: {phi}"
        assert (r["f0"] - best) / r["f0"] > GAP, f"fixture {who} is at fault: iteration {i}, f0 vs best trial"
        if r["flags"] & reference.CG_VERTEX:
            assert abs(r["phi"][6] - best) / best > GAP, \
                f"fixture {who} is at fault: iteration {i}, parabola point vs b: {r['phi'][6]} {best}"


def decisions(recs):
    return [(r["trial"], r["flags"]) for r in recs]


# ------------------------------------------------------------------ rule edges of cg.h
from hpnn_amd import ops  # noqa: E402

NAN, INF, TINY = float("nan"), float("inf"), 5e-324
_F, _R, _V, _T = ops.CG_FAILED, ops.CG_RESTART, ops.CG_VERTEX, ops.CG_TOOK7
# state: fields set before the direction (first = 0: a previous iteration exists); f0, phi: the
# losses filed (n = 1, so a mean is its sum); expect: beta, j*, flags, the seventh point, a*, and
# the a_init / first the next iteration starts from.  a_init = 1: a = .25 .5 1 2 4 8.
EDGES = [
    dict(name="tie: the lowest index wins", state=dict(first=1), f0=10.0, phi=[3, 2, 2, 5, 6, 7], phi7=1.5,
         expect=dict(beta=0.0, jstar=1, flags=_R | _V | _T, a7=0.75, alpha=0.75, a_init=0.75, first=0)),
    dict(name="tie with the seventh trial keeps b", state=dict(first=1), f0=10.0, phi=[3, 2, 2, 5, 6, 7], phi7=2.0,
         expect=dict(beta=0.0, jstar=1, flags=_R | _V, a7=0.75, alpha=0.5, a_init=0.5, first=0)),
    dict(name="NaN trials are skipped, a NaN neighbour gives no vertex", state=dict(first=1), f0=10.0,
         phi=[NAN, 4, 3, NAN, 6, 7], phi7=3.0,
         expect=dict(beta=0.0, jstar=2, flags=_R, a7=1.0, alpha=1.0, a_init=1.0, first=0)),
    dict(name="j* = 0 brackets with (0, f0)", state=dict(first=1), f0=10.0, phi=[1, 2, 3, 4, 5, 6], phi7=0.5,
         expect=dict(beta=0.0, jstar=0, flags=_R | _V | _T, a7=0.35, alpha=0.35, a_init=0.35, first=0)),
    dict(name="j* = K-1 has no parabola", state=dict(first=1), f0=10.0, phi=[6, 5, 4, 3, 2, 1], phi7=1.0,
         expect=dict(beta=0.0, jstar=5, flags=_R, a7=8.0, alpha=8.0, a_init=8.0, first=0)),
    dict(name="zero denominator (both products underflow)", state=dict(first=1, a_init=0.125), f0=1.0,
         phi=[1, TINY, 0.0, TINY, 1, 1], phi7=0.0,
         expect=dict(beta=0.0, jstar=2, flags=_R, a7=0.125, alpha=0.125, a_init=0.125, first=0)),
    # a strictly convex triple has its vertex inside (a, c): the bracket test is reached through
    # values that are not finite
    dict(name="vertex not finite / outside the bracket", state=dict(first=1), f0=10.0, phi=[5, 2, INF, 9, 9, 9],
         phi7=2.0, expect=dict(beta=0.0, jstar=1, flags=_R, a7=0.5, alpha=0.5, a_init=0.5, first=0)),
    dict(name="failed search: no trial below f0", state=dict(first=0, gg=2.0, gp=0.5, gd=1.0, gg_prev=1.0), f0=10.0,
         phi=[10, 11, 12, 13, 14, 15], phi7=10.0,
         expect=dict(beta=1.5, jstar=0, flags=_F, a7=0.0, alpha=0.0, a_init=1.0 / 16, first=1)),
    dict(name="failed search: every trial a NaN", state=dict(first=1), f0=10.0, phi=[NAN] * 6, phi7=NAN,
         expect=dict(beta=0.0, jstar=ops.CG_NONE, flags=_R | _F, a7=0.0, alpha=0.0, a_init=1.0 / 16, first=1)),
    dict(name="failed search: f0 itself a NaN", state=dict(first=1), f0=NAN, phi=[1, 2, 3, 4, 5, 6], phi7=1.0,
         expect=dict(beta=0.0, jstar=0, flags=_R | _F, a7=0.0, alpha=0.0, a_init=1.0 / 16, first=1)),
    dict(name="Polak-Ribiere+ beta", state=dict(first=0, gg=2.0, gp=0.5, gd=1.0, gg_prev=1.0), f0=10.0,
         phi=[9, 8, 7, 8, 9, 9], phi7=6.0,
         expect=dict(beta=1.5, jstar=2, flags=_V | _T, a7=1.25, alpha=1.25, a_init=1.25, first=0)),
    dict(name="negative beta is clamped", state=dict(first=0, gg=1.0, gp=3.0, gd=1.0, gg_prev=1.0), f0=10.0,
         phi=[9, 8, 7, 8, 9, 9], phi7=9.0,
         expect=dict(beta=0.0, jstar=2, flags=_V, a7=1.25, alpha=1.0, a_init=1.0, first=0)),
    dict(name="no descent along g + beta d: restart", state=dict(first=0, gg=2.0, gp=0.5, gd=-2.0, gg_prev=1.0),
         f0=10.0, phi=[9, 8, 7, 8, 9, 9], phi7=9.0,
         expect=dict(beta=0.0, jstar=2, flags=_R | _V, a7=1.25, alpha=1.0, a_init=1.0, first=0)),
    dict(name="gg = 0: nothing to descend along", state=dict(first=0, gg=0.0, gp=0.0, gd=0.0, gg_prev=1.0), f0=10.0,
         phi=[10.0] * 6, phi7=10.0,
         expect=dict(beta=0.0, jstar=0, flags=_R | _F, a7=0.0, alpha=0.0, a_init=1.0 / 16, first=1)),
    dict(name="gg_prev = 0: restart", state=dict(first=0, gg=1.0, gp=0.0, gd=0.0, gg_prev=0.0), f0=10.0,
         phi=[9, 8, 7, 8, 9, 9], phi7=9.0,
         expect=dict(beta=0.0, jstar=2, flags=_R | _V, a7=1.25, alpha=1.0, a_init=1.0, first=0)),
]


def slots_with(loss, hits=0, device="cpu"):
    """64 stat slots holding one pass's loss (the FP64 form, floats 2..3 of slot 0) and hits"""
    s = torch.zeros(64, 16, dtype=torch.float32)
    s[0, 2:4].view(torch.float64)[0] = loss
    s[0, 1:2].view(torch.int32)[0] = hits
    return s.to(device)


def run_edge(case, device="cpu"):
    """direction, f0, the six trials and the seventh of one EDGES case through ops; returns the
    state after the choice (trial K-1) and at the end, and the history, as CPU tensors"""
    st = ops.cg_state(1.0, 1, 2)
    ops.write_cg_state(st, **case["state"])
    st = st.to(device)
    hist = ops.cg_history(2, device)
    ops.cg_direction(st)
    ops.cg_file(slots_with(case["f0"], 7, device), st, hist, ops.CG_FINAL)
    for j in range(ops.CG_TRIALS):
        ops.cg_file(slots_with(float(case["phi"][j]), j, device), st, hist, j)
    mid = st.cpu().clone()
    ops.cg_file(slots_with(case["phi7"], 0, device), st, hist, ops.CG_PARABOLA)
    return mid, st.cpu().clone(), hist.cpu().clone()
