"""Shared pieces of the [clip] tests: a restatement of the rule of include/libhpnn/clip.h in numpy
(every sum in the stated order, one IEEE operation per line), the integer-exact gradient sets, the
fixture (that of tests/lrsched_common.py: a 12-8-4 net, three minibatches per epoch), the
in-process trainer and the independent PyTorch runs."""
import math
import os
import struct

import numpy as np
import torch

from hpnn_amd import capi
from hpnn_amd.models import reference
from tests import adam_common as A
from tests import lrsched_common as K

BLOCK, LANES = 1024, 256
NP = {torch.float64: np.float64, torch.float32: np.float32}
SIZES = (1, 3, 1023, 1024, 1025, 4099)  # one element, under a lane's four, one block +- 1, five blocks
SLABS = (1, 2, 3, 9, 17)                # 9 and 17: the second round of the 8-way order


def bits(x):
    return struct.pack("<d", float(x))


# ------------------------------------------------------------------ the restatement
def slab_sum(slabs, interleaved):
    """slabs: numpy [S, n] of the engine's type T.  Sequential: slabs 0 .. S-1 added in order to 0.
    Interleaved: p_w = slabs w, w + 8, ... added in order to 0, then ((p0 + p1) + ...) + p7."""
    S, n = slabs.shape
    T = slabs.dtype.type
    if not interleaved:
        a = np.zeros(n, dtype=T)
        for s in range(S):
            a = a + slabs[s]
        return a
    p = []
    for w in range(8):
        pw = np.zeros(n, dtype=T)
        for s in range(w, S, 8):
            pw = pw + slabs[s]
        p.append(pw)
    a = p[0]
    for w in range(1, 8):
        a = a + p[w]
    return a


def tree(p):
    """p[t] += p[t + s] for s = 128, 64, ..., 1 on 256 float64; returns p[0]"""
    p = p.copy()
    s = LANES // 2
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def block_sums(slabs, scale, interleaved):
    """the partials of one segment: per block of 1024 elements, lane t adds the q of the elements
    4t .. 4t + 3 in that order to 0 (elements past n add nothing), then the tree"""
    T = slabs.dtype.type
    gs = slab_sum(slabs, interleaved) * T(scale)
    g64 = gs.astype(np.float64)
    q = g64 * g64
    n = q.shape[0]
    out = []
    for b in range((n + BLOCK - 1) // BLOCK):
        blk = np.zeros(BLOCK, dtype=np.float64)  # q >= 0 or NaN: adding +0 is adding nothing
        blk[:min(BLOCK, n - b * BLOCK)] = q[b * BLOCK:(b + 1) * BLOCK]
        lanes = blk.reshape(LANES, 4)
        p = np.zeros(LANES, dtype=np.float64)
        for k in range(4):
            p = p + lanes[:, k]
        out.append(tree(p))
    return np.array(out, dtype=np.float64)


def total(partials):
    """lane t adds partials[t], partials[t + 256], ... in order to 0, then the tree"""
    p = np.zeros(LANES, dtype=np.float64)
    for i0 in range(0, len(partials), LANES):
        chunk = np.zeros(LANES, dtype=np.float64)
        chunk[:len(partials[i0:i0 + LANES])] = partials[i0:i0 + LANES]
        p = p + chunk
    return tree(p)


class Clip:
    """the state and the finalize / commit, restated on Python floats"""

    def __init__(self, max_norm):
        self.max_norm = float(max_norm)
        self.sumsq = self.norm = 0.0
        self.factor = 1.0
        self.norm_max = self.norm_last = 0.0
        self.steps = self.clipped = 0

    def finalize(self, sumsq):
        sumsq = float(sumsq)
        norm = math.sqrt(sumsq) if sumsq >= 0.0 else float("nan")  # correctly rounded; a NaN stays a NaN
        factor = self.max_norm / norm if norm > self.max_norm else 1.0
        self.sumsq, self.norm, self.factor = sumsq, norm, factor
        self.steps += 1
        if factor != 1.0:
            self.clipped += 1
        if norm > self.norm_max:
            self.norm_max = norm
        self.norm_last = norm

    def commit(self):
        rec = dict(steps=self.steps, clipped=self.clipped, norm_max=self.norm_max, norm_last=self.norm_last)
        self.steps = self.clipped = 0
        self.norm_max = self.norm_last = 0.0
        return rec

    def as_dict(self):
        return dict(max_norm=self.max_norm, sumsq=self.sumsq, norm=self.norm, factor=self.factor,
                    norm_max=self.norm_max, norm_last=self.norm_last, steps=self.steps, clipped=self.clipped)


def same_state(got, want):
    """a read_clip_state dict against Clip.as_dict(), the floats bit for bit (NaN-safe)"""
    return all(bits(got[k]) == bits(v) if isinstance(v, float) else got[k] == v for k, v in want.items())


# ------------------------------------------------------------------ gradient sets
def random_slabs(n, S, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 4.0 - 2.0)
    return (scale * torch.randn(S, n, generator=g, dtype=torch.float64)).to(dtype)


def integer_set(n, S, j, dtype, seed):
    """integer slabs [S, n] whose sum over the slabs has j^2 elements of 3, j^2 of -4 and zeros
    elsewhere, in a seeded order: the sum of squares is 25 j^2 and the norm 5 j in any order of
    summation (every partial sum is a small integer)"""
    assert 2 * j * j <= n
    g = torch.Generator().manual_seed(seed)
    tgt = torch.zeros(n, dtype=torch.int64)
    tgt[:j * j], tgt[j * j:2 * j * j] = 3, -4
    tgt = tgt[torch.randperm(n, generator=g)]
    sl = torch.randint(-5, 6, (S, n), generator=g)
    sl[S - 1] = tgt - sl[:S - 1].sum(0)
    assert int((sl.sum(0) ** 2).sum()) == 25 * j * j
    return sl.to(dtype), 25 * j * j


# ------------------------------------------------------------------ the engines
make_data = K.make_data
write_conf = K.write_conf
NET, LR, SEED = K.NET, K.LR, K.SEED


def train(d, device="cpu", load=None, dump="state.bin", verbose=0, env=None, **set_kw):
    """K.train plus clip: Network.clip_history() of the call"""
    capi.init(verbose)
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        net = capi.Network(os.path.join(d, "nn.conf"))
        net.set(device=device, **set_kw)
        if load:
            net.load_state(os.path.join(d, load))
        w0 = K.C.weights_of(net, d, "k0.opt")
        ok = net.train()
        out = dict(ok=ok, w0=w0, w=K.C.weights_of(net, d, "k1.opt"), clip=net.clip_history(), lr=net.lr_history(),
                   val=net.validation(), best=net.best(), epochs_done=net.epochs_done, raw=None)
        if ok and dump:
            net.dump_state(os.path.join(d, dump))
            out["raw"] = open(os.path.join(d, dump), "rb").read()
        net.close()
        return out
    finally:
        if verbose:
            capi.init(0)
            capi._LIBC.fflush(None)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def reference_run(w0, X, T, net_type, B, epochs, train_kind, lr=LR, alpha=0.2, clip=None, perm=None,
                  dtype=torch.float64):
    """`epochs` epochs of reference.batched_step (BP | BPM | ADAM) from w0 on the samples in the
    seeded order (perm: a further permutation inside the minibatches), clipped to `clip` when given;
    returns (weights as float64 arrays, the gradient norm of every step)"""
    o = np.array(A.order(X.shape[0]))
    if perm is not None:
        o = o[perm]
    Xo, To = torch.tensor(X[o], dtype=dtype), torch.tensor(T[o], dtype=dtype)
    W = [torch.tensor(w, dtype=dtype) for w in w0]
    mom = [torch.zeros_like(w) for w in W] if train_kind == "BPM" else None
    adam = None
    if train_kind == "ADAM":
        adam = ([torch.zeros_like(w) for w in W], [torch.zeros_like(w) for w in W], reference.adam_new_state(lr=lr))
    norms = []
    for _ in range(epochs):
        for s in range(0, Xo.shape[0], B):
            reference.batched_step(W, Xo[s:s + B], To[s:s + B], net_type, lr, momentum=mom, alpha=alpha, adam=adam,
                                   clip=clip, norms=norms)
    return [w.double().numpy() for w in W], norms


def order_spread(w0, X, T, net_type, B, epochs, train_kind, lr=LR, alpha=0.2, clip=None, dtype=torch.float64):
    """A.order_spread for a clipped run of train_kind: the largest weight difference between two
    reference runs that differ only in the order of the samples inside every minibatch"""
    n = X.shape[0]
    rng = np.random.default_rng(5)
    perm = np.concatenate([s + rng.permutation(min(B, n - s)) for s in range(0, n, B)])
    wa = reference_run(w0, X, T, net_type, B, epochs, train_kind, lr, alpha, clip, None, dtype)[0]
    wb = reference_run(w0, X, T, net_type, B, epochs, train_kind, lr, alpha, clip, perm, dtype)[0]
    return A.spread(wa, wb)


def median_norm(w0, X, T, net_type, B, epochs, train_kind, lr=LR, alpha=0.2):
    """the bound of a run that must clip, and not always: the median of the per-step gradient norms
    of the UNCLIPPED run of the same configuration"""
    norms = reference_run(w0, X, T, net_type, B, epochs, train_kind, lr, alpha, None)[1]
    return float(np.median(norms)), norms
