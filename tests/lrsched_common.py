"""Shared pieces of the [lr_schedule] tests: an independent restatement of the rule of
include/libhpnn/lrsched.h in plain Python floats (products in the stated order), its mutants, the
fixture (the recipe of tests/cg_common.py on a 12-8-4 net), the in-process trainer and a reader
of the state file's schedule block."""
import math
import os
import struct

import numpy as np

from hpnn_amd import capi
from hpnn_amd.utils import formats
from tests import cg_common as C

SEED = C.SEED
LR = 0.05
NET = dict(sizes=[12, 8, 4], n=96, nv=40, B=32)  # three full minibatches per epoch
DATA_SEED = 3


# ------------------------------------------------------------------ the restatement
class Sched:
    """the rule, restated.  mutant: None or one of MUTANTS (each a deliberate mistake)"""

    def __init__(self, kind, lr0, gamma=0.5, period=10, span=0, lr_end=0.0, lr_min=0.0, patience=2, warmup=0, epoch=0,
                 mutant=None):
        self.kind, self.lr0, self.gamma, self.period, self.span = kind, float(lr0), float(gamma), period, span
        self.lr_end, self.lr_min, self.patience, self.warmup = float(lr_end), float(lr_min), patience, warmup
        self.epoch, self.scale, self.best, self.stale, self.cuts, self.valid = epoch, 1.0, 0.0, 0, 0, 0
        self.lr = float(lr0)
        self.mutant = mutant
        self.pending = None  # mutant "cut_same_epoch" only

    def advance(self):
        e, m = self.epoch, self.mutant
        if self.kind == "constant":
            base = self.lr0
        elif self.kind == "step":
            f = 1.0
            for _ in range((e + 1 if m == "period_off_by_one" else e) // self.period):
                f = f * self.gamma
            base = self.lr0 * f
        elif self.kind == "linear":
            base = self.lr0 + (self.lr_end - self.lr0) * (float(e) / float(self.span)) if e < self.span else self.lr_end
        else:
            base = self.lr0 * self.scale
            if m != "clamp_after_warmup" and base < self.lr_min:
                base = self.lr_min
        if e < self.warmup:
            base = base * (float(e) / float(self.warmup) if m == "warmup_e_over_w" else float(e + 1) / float(self.warmup))
        if self.kind == "plateau" and m == "clamp_after_warmup" and base < self.lr_min:
            base = self.lr_min
        self.lr = base
        self.epoch = e + 1
        return base

    def plateau(self, loss):
        if self.kind != "plateau":
            return
        m = self.mutant
        better = (loss <= self.best) if m == "le_for_lt" else (loss < self.best)
        if loss == loss and (not self.valid or better):
            self.best, self.valid, self.stale = loss, 1, 0
        else:
            self.stale += 1
        if self.stale == self.patience:
            self.scale = self.scale * self.gamma
            if m != "stale_not_reset":
                self.stale = 0
            self.cuts += 1
            if m == "cut_same_epoch":  # the rate of the epoch just trained is rewritten
                base = self.lr0 * self.scale
                self.lr = self.lr_min if base < self.lr_min else base

    def running(self):
        return dict(scale=self.scale, best=self.best, stale=self.stale, cuts=self.cuts, valid=self.valid)

    def resume(self, other):
        """continue from another run's running fields at its epoch (a state file)"""
        self.epoch = other.epoch
        if self.mutant != "scale_restarted":
            self.scale = other.scale
        self.best, self.stale, self.cuts, self.valid = other.best, other.stale, other.cuts, other.valid


MUTANTS = ("period_off_by_one", "le_for_lt", "clamp_after_warmup", "stale_not_reset", "cut_same_epoch",
           "warmup_e_over_w", "scale_restarted")


def trace(cfg, losses=None, epochs=None, mutant=None, resume_at=None):
    """the numbers a run compares: per epoch the rate used (read after the epoch's validation pass,
    as a history filed per epoch would show it) and the running fields.  losses: one validation
    loss per epoch (None: no pass).  resume_at: split into two runs joined through resume()."""
    n = epochs if epochs is not None else len(losses)
    s = Sched(mutant=mutant, **cfg)
    out = []
    for e in range(n):
        if resume_at is not None and e == resume_at:
            t = Sched(mutant=mutant, **cfg)
            t.resume(s)
            s = t
        s.advance()
        if losses is not None and losses[e] is not None:
            s.plateau(losses[e])
        out.append((s.lr, s.scale, s.best, s.stale, s.cuts, s.valid))
    return out


def bits(x):
    return struct.pack("<d", x)


def same(a, b):
    """two traces equal bit for bit (NaN-safe)"""
    return len(a) == len(b) and all(
        all((bits(float(x)) == bits(float(y))) for x, y in zip(ra, rb)) for ra, rb in zip(a, b))


NAN = float("nan")
# hand-made validation losses, one per epoch: ties, a NaN first, a NaN later, enough stale passes to
# reach the lr_min clamp, cuts at patience 1 and 3
PLATEAU_CASES = [
    dict(name="ties do not improve", cfg=dict(kind="plateau", lr0=0.1, gamma=0.5, patience=2),
         losses=[5.0, 5.0, 5.0, 4.0, 4.0, 4.0, 4.0, 3.0]),
    dict(name="a NaN first", cfg=dict(kind="plateau", lr0=0.1, gamma=0.5, patience=2),
         losses=[NAN, 7.0, 8.0, 9.0, 6.0, 6.5, 6.5]),
    dict(name="a NaN later", cfg=dict(kind="plateau", lr0=0.1, gamma=0.9, patience=2),
         losses=[5.0, NAN, 4.0, NAN, NAN, 3.0, 3.0, 3.0]),
    dict(name="the lr_min clamp", cfg=dict(kind="plateau", lr0=0.1, gamma=0.5, patience=1, lr_min=0.03),
         losses=[5.0, 6.0, 6.0, 6.0, 6.0, 4.0, 6.0]),
    dict(name="patience 1", cfg=dict(kind="plateau", lr0=0.3, gamma=0.9, patience=1),
         losses=[3.0, 2.0, 2.5, 2.0, 1.0, 1.5, 1.5]),
    dict(name="patience 3", cfg=dict(kind="plateau", lr0=0.3, gamma=0.9, patience=3),
         losses=[3.0, 3.5, 3.5, 3.5, 3.5, 2.0, 2.5, 2.5, 2.5, 2.5]),
    dict(name="clamp under warmup", cfg=dict(kind="plateau", lr0=0.1, gamma=0.5, patience=1, lr_min=0.08, warmup=4),
         losses=[5.0, 6.0, 6.0, 6.0, 6.0, 6.0]),
]


# ------------------------------------------------------------------ the fixture and the trainer
def make_data(d):
    """write train.hpnb / val.hpnb into d (the recipe of tests/cg_common.py); returns X, T, Xv, Tv"""
    n_in, n_out = NET["sizes"][0], NET["sizes"][-1]
    rng = np.random.default_rng(DATA_SEED)
    P = rng.uniform(-1.0, 1.0, (n_out, n_in))
    out = []
    for fn, n in (("train.hpnb", NET["n"]), ("val.hpnb", NET["nv"])):
        cls = rng.integers(0, n_out, n)
        X = np.clip(P[cls] + 0.6 * rng.standard_normal((n, n_in)), -1.0, 1.0)
        lab = np.where(rng.random(n) < 0.2, rng.integers(0, n_out, n), cls)
        T = np.full((n, n_out), 0.0)
        T[np.arange(n), lab] = 1.0
        capi.pack_arrays(os.path.join(d, fn), X, T)
        out += [X, T]
    return out


def write_conf(d, train="BP", dtype="f64", net_type="SNN", **extra):
    kw = dict(mode="batched", batch=NET["B"], epochs=4, lr=LR, dtype=dtype)
    kw.update(extra)
    kw = {k: v for k, v in kw.items() if v is not None}
    formats.write_conf(os.path.join(d, "nn.conf"), name="lrs", type=net_type, seed=SEED, inputs=NET["sizes"][0],
                       hiddens=NET["sizes"][1:-1], outputs=NET["sizes"][-1], train=train,
                       sample_dir=os.path.join(d, "train.hpnb"), test_dir=os.path.join(d, "val.hpnb"), **kw)


def read_state(path):
    """the state file (csrc/core/state.cpp) as a dict: header words, the raw bytes of the weight /
    momentum / Adam payload, the schedule block (has_sched) and the file's length"""
    b = open(path, "rb").read()
    assert b[:8] == b"HPNNSTA1"
    typ, train, L, has_mom = struct.unpack_from("<4I", b, 8)
    dims = struct.unpack_from(f"<{L + 1}I", b, 24)
    off = 24 + 4 * (L + 1)
    seed, epochs, has_adam, has_sched = struct.unpack_from("<4I", b, off)
    off += 24
    nw = sum(dims[l] * dims[l + 1] for l in range(L))
    pay = 8 * nw * (1 + has_mom + has_adam) + (24 if has_adam else 0)
    out = dict(train=train, has_momentum=has_mom, has_adam=has_adam, has_sched=has_sched, epochs_done=epochs,
               payload=b[off:off + pay], length=len(b), expected_plain=off + pay + 8, sched=None)
    off += pay
    if has_sched:
        scale, best, stale, cuts, valid, pad = struct.unpack_from("<ddIIII", b, off)
        out["sched"] = dict(scale=scale, best=best, stale=stale, cuts=cuts, valid=valid, pad=pad)
        off += 32
    assert off + 8 == len(b), "state file: bytes left over"
    return out


def train(d, device="cpu", load=None, dump="state.bin", verbose=0, env=None, **set_kw):
    """train nn.conf of d in this process (after load_state(load) when given); returns a dict: ok,
    w (list of float64 arrays), lr (Network.lr_history()), val, best, epochs_done, state
    (read_state of the file dumped afterwards) and raw (its bytes)"""
    capi.init(verbose)
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        net = capi.Network(os.path.join(d, "nn.conf"))
        net.set(device=device, **set_kw)
        if load:
            net.load_state(os.path.join(d, load))
        w0 = C.weights_of(net, d, "k0.opt")
        ok = net.train()
        out = dict(ok=ok, w0=w0, w=C.weights_of(net, d, "k1.opt"), lr=net.lr_history(), val=net.validation(),
                   best=net.best(), epochs_done=net.epochs_done, state=None, raw=None, sched=net.lr_schedule)
        if ok and dump:
            net.dump_state(os.path.join(d, dump))
            out["state"] = read_state(os.path.join(d, dump))
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


def wbytes(ws):
    return [np.ascontiguousarray(w).tobytes() for w in ws]


__all__ = ["math"]
