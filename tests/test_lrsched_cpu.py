"""[lr_schedule] on the host: the rule of include/libhpnn/lrsched.h against an independent
restatement (tests/lrsched_common.py) bit for bit, mutants of that restatement, the FP64 CPU engine
(bit-exact chaining, resume and the state file) and the interface (conf keys, C API, CLI, metrics,
refusals).  No GPU."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.utils import formats
from tests import lrsched_common as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def header_trace(cfg, losses=None, epochs=None, resume_at=None):
    """the trace of lrsched_common.trace, run by the header's host entry points (ops on CPU tensors)"""
    n = epochs if epochs is not None else len(losses)
    s = ops.lr_state(**cfg)
    vh = torch.zeros(1, 2, dtype=torch.float64)
    one = torch.ones(1, dtype=torch.int32)
    out = []
    for e in range(n):
        if resume_at is not None and e == resume_at:
            r = ops.read_lr_state(s)
            s = ops.lr_state(**dict(cfg, epoch=r["epoch"]))
            ops.write_lr_state(s, **{k: r[k] for k in ("scale", "best", "stale", "cuts", "valid")})
        ops.lr_advance(s)
        if losses is not None and losses[e] is not None:
            vh[0, 0] = losses[e]
            ops.lr_plateau(vh, one, s)
        r = ops.read_lr_state(s)
        assert r["epoch"] == cfg.get("epoch", 0) + e + 1
        out.append((r["lr"], r["scale"], r["best"], r["stale"], r["cuts"], r["valid"]))
    return out


STEP_LINEAR = ([dict(kind="step", lr0=0.1, gamma=g, period=p, warmup=w) for g in (0.5, 0.9) for p in (1, 3)
                for w in (0, 1, 4)] +
               [dict(kind="linear", lr0=0.3, lr_end=e, span=sp, warmup=w) for e in (0.0, 0.01) for sp in (1, 7)
                for w in (0, 1, 4)] +
               [dict(kind="constant", lr0=0.07, warmup=w) for w in (0, 1, 4)])


@pytest.mark.parametrize("cfg", STEP_LINEAR, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_header_equals_restatement(cfg):
    # epochs 0..40: before, at and far beyond every period, span and warmup
    assert K.same(header_trace(cfg, epochs=41), K.trace(cfg, epochs=41))
    # a run that starts at epoch 5 (a resumed call) continues the same function of the absolute epoch
    late = dict(cfg, epoch=5)
    assert K.same(header_trace(late, epochs=36), K.trace(late, epochs=36))
    assert K.same(header_trace(late, epochs=36), K.trace(cfg, epochs=41)[5:])


def test_step_is_successive_products():
    """gamma^(e / period) is e / period multiplications of a factor that starts at 1.0"""
    s = ops.lr_state("step", lr0=0.1, gamma=0.9, period=1)
    f = 1.0
    for e in range(41):
        ops.lr_advance(s)
        assert K.bits(ops.read_lr_state(s)["lr"]) == K.bits(0.1 * f)
        f = f * 0.9


@pytest.mark.parametrize("case", K.PLATEAU_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("warmup", [0, 1, 4])
def test_plateau_equals_restatement(case, warmup):
    cfg = dict(case["cfg"])
    cfg.setdefault("warmup", warmup)
    got = header_trace(cfg, case["losses"])
    assert K.same(got, K.trace(cfg, case["losses"]))
    # through a state file's fields: split anywhere, the same trace
    for at in range(1, len(case["losses"])):
        assert K.same(header_trace(cfg, case["losses"], resume_at=at), got)
        assert K.same(K.trace(cfg, case["losses"], resume_at=at), got)


def test_plateau_cases_cover_their_edges():
    """the hand-made sequences do what their names say (on the restatement)"""
    by = {c["name"]: K.trace(c["cfg"], c["losses"]) for c in K.PLATEAU_CASES}
    assert [r[4] for r in by["ties do not improve"]] == [0, 0, 1, 1, 1, 2, 2, 2]
    assert by["a NaN first"][0][5] == 0 and by["a NaN first"][1][5] == 1 and by["a NaN first"][1][2] == 7.0
    assert by["a NaN later"][-1][4] >= 2
    assert [r[0] for r in by["the lr_min clamp"]][3:5] == [0.03, 0.03]
    assert [r[4] for r in by["patience 1"]] == [0, 0, 1, 2, 2, 3, 4]
    assert [r[4] for r in by["patience 3"]] == [0, 0, 0, 1, 1, 1, 1, 1, 2, 2]
    # the cut behind epoch 1's pass acts at epoch 2: max(lr_min, lr0 scale) = 0.08 first, then (e + 1) / W
    assert by["clamp under warmup"][2][0] == 0.08 * (3.0 / 4.0)


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_mutants_change_a_compared_number(mutant):
    cases = [(c["cfg"], c["losses"], None) for c in K.PLATEAU_CASES]
    cases += [(c, None, 41) for c in STEP_LINEAR]
    changed = 0
    for cfg, losses, epochs in cases:
        good = K.trace(cfg, losses, epochs)
        assert K.same(good, header_trace(cfg, losses, epochs))
        changed += not K.same(good, K.trace(cfg, losses, epochs, mutant=mutant))
        if losses:
            for at in range(1, len(losses)):
                changed += not K.same(good, K.trace(cfg, losses, epochs, mutant=mutant, resume_at=at))
    assert changed, f"mutant {mutant} changes nothing the tests compare"


@pytest.mark.parametrize("bad", [dict(lr0=float("inf")), dict(lr0=float("nan")), dict(lr_end=float("inf")),
                                 dict(gamma=0.0), dict(gamma=1.5), dict(gamma=float("nan")), dict(period=0),
                                 dict(kind="linear", span=0), dict(lr_min=-1e-9), dict(lr_min=float("nan")),
                                 dict(kind="plateau", patience=0), dict(kind=4)])
def test_valid_refuses_each_bad_field(bad):
    good = dict(kind="step", lr0=0.1, gamma=0.5, period=1, span=3, lr_end=0.0, lr_min=0.0, patience=2)
    for k in ("step", "linear", "plateau", "constant"):
        assert ops.lr_valid(ops.lr_state(**dict(good, kind=k)))
    with pytest.raises(ValueError):
        ops.lr_state(**dict(good, **bad))


def test_state_layout():
    from hpnn_amd._lib import native
    assert native().LR_STATE_BYTES == 96 and native().LR_STATE_BYTES % 16 == 0
    s = ops.lr_state("plateau", lr0=0.25, gamma=0.75, period=3, span=5, lr_end=0.5, lr_min=0.125, patience=7,
                     warmup=9, epoch=11)
    assert s.tolist()[:7] == [0.25, 0.75, 0.5, 0.125, 1.0, 0.0, 0.25]
    assert s.view(torch.int32)[14:].tolist() == [3, 3, 5, 7, 9, 11, 0, 0, 0, 0]


# ------------------------------------------------------------------ the element rule
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("momentum", [False, True])
def test_host_update_is_the_stated_rule(dtype, momentum):
    g = torch.Generator().manual_seed(3)
    n, S = 37, 3
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    v = torch.randn(n, generator=g, dtype=torch.float64).to(dtype) * 0.1
    slab = torch.randn(S, n, generator=g, dtype=torch.float64).to(dtype)
    w[-3:], v[-3:], slab[:, -3:] = 0.5, 0.0, 0.0
    st = ops.lr_state("step", lr0=0.3, gamma=0.9, period=1)
    ops.lr_advance(st), ops.lr_advance(st)
    lr, alpha, scale = torch.tensor(0.3 * 0.9, dtype=torch.float64).to(dtype), torch.tensor(0.2, dtype=dtype), \
        torch.tensor(1.0 / 7.0, dtype=torch.float64).to(dtype)
    gs = ((slab[0] + slab[1]) + slab[2]) * scale  # slab order, then (T)scale
    w1, v1 = w.clone(), v.clone()
    ops.sgd_sched_fp(ops.SgdSchedTable([dict(w=w1, v=v1, slab=slab)], momentum=momentum), st, scale=1.0 / 7.0,
                     alpha=0.2)
    if momentum:
        vv = v + lr * gs
        assert torch.equal(w1, w + vv) and torch.equal(v1, vv * alpha)
    else:
        assert torch.equal(w1, w + lr * gs) and torch.equal(v1, v)
    assert w1[-3:].view(torch.int64 if dtype == torch.float64 else torch.int32).tolist() == \
        w[-3:].view(torch.int64 if dtype == torch.float64 else torch.int32).tolist()  # g = 0, v = 0: w's bits


# ------------------------------------------------------------------ the FP64 CPU engine
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lrs"))
    K.make_data(d)
    return d


@pytest.mark.parametrize("tr", ["BP", "BPM"])
def test_step_equals_chained_calls(data, tr):
    """period 1 over 3 epochs == three one-epoch calls through the state file with -l set per epoch"""
    K.write_conf(data, train=tr, epochs=3)
    a = K.train(data, lr_schedule=dict(kind="step", gamma=0.5, period=1))
    assert a["ok"] and [K.bits(x) for x in a["lr"]] == [K.bits(K.LR), K.bits(K.LR * 0.5), K.bits(K.LR * 0.5 * 0.5)]
    K.write_conf(data, train=tr, epochs=1)
    r, prev = None, None
    for i, lr in enumerate(a["lr"]):
        r = K.train(data, lr=lr, load=prev, dump=f"c{i}.bin")
        prev = f"c{i}.bin"
    assert K.wbytes(r["w"]) == K.wbytes(a["w"])
    assert r["raw"] == a["raw"]  # weights, momentum, progress, checksum: the same file


@pytest.mark.parametrize("tr", ["BP", "BPM"])
def test_gamma_one_equals_unscheduled(data, tr):
    K.write_conf(data, train=tr, epochs=3)
    plain = K.train(data)
    assert plain["lr"] == [] and plain["sched"]["kind"] is None
    for kind in ("constant", "step"):
        s = K.train(data, lr_schedule=dict(kind=kind, gamma=1.0, period=1))
        assert s["raw"] == plain["raw"] and K.wbytes(s["w"]) == K.wbytes(plain["w"])
        assert s["lr"] == [K.LR] * 3
    # a non-plateau file has the parent's length and a zero has_sched word
    assert plain["state"]["has_sched"] == 0 and plain["state"]["length"] == plain["state"]["expected_plain"]


KINDS = [dict(kind="constant", warmup=3), dict(kind="step", gamma=0.5, period=3), dict(kind="step", gamma=0.9, period=1, warmup=2),
         dict(kind="linear", span=3, lr_end=0.001), dict(kind="plateau", gamma=0.5, patience=1)]


@pytest.mark.parametrize("tr", ["BP", "BPM", "ADAM"])
@pytest.mark.parametrize("sched", KINDS, ids=lambda s: s["kind"] + str(s.get("warmup", "")))
def test_four_epochs_equal_two_plus_two(data, tr, sched):
    plateau = sched["kind"] == "plateau"
    lr = 8.0 if plateau and tr != "ADAM" else (0.5 if plateau else None)  # plateau: a rate at which the loss stalls
    extra = dict(validate=1) if plateau else {}
    K.write_conf(data, train=tr, epochs=4, **extra)
    kw = dict(lr_schedule=sched, **({"lr": lr} if lr else {}))
    full = K.train(data, **kw)
    K.write_conf(data, train=tr, epochs=2, **extra)
    h1 = K.train(data, dump="h1.bin", **kw)
    h2 = K.train(data, load="h1.bin", dump="h2.bin", **kw)
    assert full["ok"] and h1["ok"] and h2["ok"]
    assert [K.bits(x) for x in h1["lr"] + h2["lr"]] == [K.bits(x) for x in full["lr"]]
    assert K.wbytes(h2["w"]) == K.wbytes(full["w"]) and h2["raw"] == full["raw"]
    assert len(set(full["lr"])) > 1, "the fixture is at fault: the rate never changed"
    st = full["state"]
    assert st["has_sched"] == (1 if plateau else 0)
    assert st["length"] == st["expected_plain"] + (32 if plateau else 0)
    if plateau:
        assert h1["state"]["sched"]["cuts"] >= 1, "the fixture is at fault: no cut before the split"
        assert st["sched"]["pad"] == 0 and st["sched"]["valid"] == 1


def test_plateau_follows_the_validation_losses(data):
    """the engine's rates are those of the restatement fed the engine's own validation loss sums"""
    K.write_conf(data, train="BP", epochs=8, validate=1, lr=2.0)
    cfg = dict(kind="plateau", gamma=0.5, patience=1, lr_min=0.2)
    r = K.train(data, lr_schedule=cfg)
    sums = [v["loss"] * v["n"] for v in r["val"]]
    t = K.trace(dict(cfg, lr0=2.0), sums)
    assert [K.bits(x) for x in r["lr"]] == [K.bits(row[0]) for row in t]
    assert min(r["lr"]) == 0.2 and r["state"]["sched"]["cuts"] == t[-1][4] >= 4
    assert abs(r["state"]["sched"]["best"] - min(sums)) <= 1e-12 * min(sums)


def test_keep_best_returns_the_best_epochs_state(data):
    """-K loss with plateau: the kernel AND the schedule state of -e <best epoch>"""
    cfg = dict(kind="plateau", gamma=0.5, patience=1)
    K.write_conf(data, train="BPM", epochs=10, validate=1, lr=2.0)
    kb = K.train(data, lr_schedule=cfg, keep_best="loss", patience=3)
    b = kb["best"]["epoch"]
    assert 1 < b < 10 and kb["epochs_done"] == b and len(kb["val"]) == b + 3
    assert len(kb["lr"]) == b + 3  # reported up to the stopping pass's epoch
    K.write_conf(data, train="BPM", epochs=b, validate=1, lr=2.0)
    e = K.train(data, lr_schedule=cfg)
    assert e["raw"] == kb["raw"] and K.wbytes(e["w"]) == K.wbytes(kb["w"])
    assert kb["state"]["sched"] == e["state"]["sched"]


# ------------------------------------------------------------------ interface
def test_conf_round_trip(data, tmp_path):
    K.write_conf(data, lr_schedule="plateau", lr_gamma=0.25, lr_period=3, lr_span=7, lr_end=0.001, lr_min=0.0005,
                 lr_patience=4, warmup=2)
    net = capi.Network(os.path.join(data, "nn.conf"))
    want = dict(kind="plateau", gamma=0.25, period=3, span=7, lr_end=0.001, lr_min=0.0005, patience=4, warmup=2)
    assert net.lr_schedule == want
    p = str(tmp_path / "out.conf")
    net.dump_conf(p)
    txt = open(p).read()
    for key in ("lr_schedule] plateau", "lr_gamma] 0.25", "lr_period] 3", "lr_span] 7", "lr_end] 0.001",
                "lr_min] 0.0005", "lr_patience] 4", "warmup] 2"):
        assert "[" + key in txt
    assert "[lr] " in txt  # [lr] itself is still read, not swallowed by a prefix
    net.close()
    net2 = capi.Network(p)
    assert net2.lr_schedule == want
    net2.close()
    # nothing set: nothing written, the defaults returned
    K.write_conf(data)
    net = capi.Network(os.path.join(data, "nn.conf"))
    assert net.lr_schedule == dict(kind=None, gamma=0.5, period=10, span=0, lr_end=0.0, lr_min=0.0, patience=2, warmup=0)
    net.dump_conf(p)
    assert "lr_" not in open(p).read() and "warmup" not in open(p).read()
    net.set(lr_schedule=dict(warmup=3))  # [warmup] alone schedules a constant rate
    assert net.lr_schedule["kind"] == "constant"
    net.close()


@pytest.mark.parametrize("key,val", [("lr_schedule", "cosine"), ("lr_gamma", "0"), ("lr_gamma", "1.5"), ("lr_period", "0"),
                                     ("lr_span", "x"), ("lr_min", "-1"), ("lr_end", "inf"), ("lr_patience", "0")])
def test_conf_value_errors(data, capfd, key, val):
    K.write_conf(data, **{key: val})
    with pytest.raises(RuntimeError):
        capi.Network(os.path.join(data, "nn.conf"))
    assert f"[{key}]" in capfd.readouterr().err


def _refused(data, capfd, needle, **set_kw):
    capi.init(0)
    net = capi.Network(os.path.join(data, "nn.conf"))
    net.set(device="cpu", **set_kw)
    assert not net.train()
    capi._LIBC.fflush(None)
    assert needle in capfd.readouterr().err
    net.close()


def test_refusals(data, capfd):
    K.write_conf(data, train="BP", epochs=2)
    _refused(data, capfd, "plateau needs [validate]", lr_schedule=dict(kind="plateau"))
    _refused(data, capfd, "[lr_span] >= 1 for linear", lr_schedule=dict(kind="linear"))
    K.write_conf(data, train="CG", epochs=2)
    _refused(data, capfd, "not supported by [train] CG", lr_schedule=dict(kind="step"))


def test_online_mode_warns_once(data, capfd):
    K.write_conf(data, train="BP", mode="online", batch=None, epochs=None)
    capi.init(1)
    try:
        net = capi.Network(os.path.join(data, "nn.conf"))
        net.set(device="cpu", lr_schedule=dict(kind="step"))
        assert net.train() and net.lr_history() == []
        net.close()
    finally:
        capi.init(0)
        capi._LIBC.fflush(None)
    assert capfd.readouterr().err.count("[lr_schedule] has no effect in online mode") == 1


def test_python_multi_device_refusal():
    from hpnn_amd.models import MLP
    from hpnn_amd.parallel.dp import DataParallel
    m = MLP([32, 32, 32], "SNN", batch=32, device="cpu", lr_schedule=dict(kind="step", lr=0.1))
    with pytest.raises(ValueError, match="one device only"):
        DataParallel(m)
    with pytest.raises(RuntimeError, match="one launch"):
        m.update_layer(0, 0.1, 0.0, 1.0)


@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
def test_mlp_emulation_applies_the_epochs_rate(momentum):
    """the CPU emulation of the scheduled plan: gamma 1 is the unscheduled plan bit for bit (one
    slab per layer at this batch, so both sum in the same order), and under step every epoch's
    weight change is that epoch's rate times the same gradient"""
    from hpnn_amd.models import MLP
    torch.manual_seed(1)
    sizes, B = [40, 64, 8], 32
    X = torch.rand(B, sizes[0]) * 2 - 1
    T = torch.full((B, sizes[-1]), -1.0)
    T[torch.arange(B), torch.randint(0, sizes[-1], (B,))] = 1.0

    def run(sched, lr):
        m = MLP(sizes, "ANN", batch=B, device="cpu", momentum=momentum, seed=5, lr_schedule=sched)
        assert all(s == 1 for s in m.S)
        Tp = torch.zeros(m.Bp, sizes[-1])
        Tp[:B] = T
        for _ in range(3):
            if sched:
                m.advance_schedule()
            m.train_step(m.prepare_input(X), T=Tp, n_valid=B, lr=lr, alpha=0.25)
        return m

    plain = run(None, 0.125)
    same = run(dict(kind="step", lr=0.125, gamma=1.0, period=1), 99.0)
    for l in range(2):
        assert torch.equal(plain.W32[l], same.W32[l]) and torch.equal(plain.Wb[l], same.Wb[l])
        assert torch.equal(plain.Wt[l], same.Wt[l])
        if momentum:
            assert torch.equal(plain.V32[l], same.V32[l])
    cut = run(dict(kind="step", lr=0.125, gamma=0.5, period=1), 99.0)
    assert ops.read_lr_state(cut.lr_state)["lr"] == 0.125 * 0.25 and ops.read_lr_state(cut.lr_state)["epoch"] == 3
    assert not torch.equal(cut.W32[0], plain.W32[0])


def test_cli_history_lines_and_metrics(data):
    """train_nn -L step: the schedule line, one LR line per epoch at -vv, one "lr" event per epoch"""
    K.write_conf(data, train="BPM", epochs=3, lr_gamma=0.5, lr_period=1)
    m = os.path.join(data, "m.jsonl")
    if os.path.exists(m):
        os.remove(m)
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-vv", "-c", "-L", "step", "-M", "m.jsonl", "nn.conf"], cwd=data,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("training: learning rate schedule step") == 1
    lines = [ln for ln in r.stdout.splitlines() if "LR: epoch" in ln]
    assert [ln.split("LR: ")[1] for ln in lines] == [f"epoch {e + 1} lr={K.LR * 0.5 ** e:.17g}" for e in range(3)]
    ev = [json.loads(ln) for ln in open(m)]
    lr = [e for e in ev if e.get("event") == "lr"]
    assert [(e["epoch"], e["lr"], e["engine"]) for e in lr] == [(e + 1, K.LR * 0.5 ** e, "cpu") for e in range(3)]
    # without -L: no line, no event, the parent's output
    os.remove(m)
    r2 = subprocess.run([os.path.join(BIN, "train_nn"), "-vv", "-c", "-M", "m.jsonl", "nn.conf"], cwd=data,
                        capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0 and "LR:" not in r2.stdout and "learning rate schedule" not in r2.stdout
    assert not [ln for ln in open(m) if '"lr"' in ln.split(",")[0]]
    bad = subprocess.run([os.path.join(BIN, "train_nn"), "-L", "cosine", "nn.conf"], cwd=data, capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode != 0 and "bad -L parameter" in bad.stderr
