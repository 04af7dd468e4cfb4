"""[validate] N on the CPU: the conf key and the -V flag, the FP64 CPU batched engine's
validation records against an independent FP64 PyTorch reference, training left bit for bit
unchanged by validation, record numbering across an exact resume, the metrics events, the
refusals, and the PyTorch emulation of the forward-only tile kernel against FP64."""
import ctypes
import ctypes.util
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP, reference
from hpnn_amd.utils import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")

N_TRAIN, N_VAL, B, SEED, LR = 37, 23, 8, 11, 0.05
VAL_RE = re.compile(r"VALIDATION: epoch (\d+) loss=([0-9.eE+-]+) acc=(\d+)/(\d+)")


def _order(n, seed):
    """nn_train_kernel's seeded sample order (the helper of tests/test_bplan_gpu.py)"""
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.random.restype = ctypes.c_long
    libc.srandom(ctypes.c_uint(seed))
    used, order = set(), []
    while len(order) < n:
        idx = int(float(libc.random()) * n / 2147483647.0)
        if idx >= n or idx in used:
            continue
        used.add(idx)
        order.append(idx)
    return order


def _records(out):
    return [(int(e), float(l), int(c), int(n)) for e, l, c, n in VAL_RE.findall(out)]


def _dataset(d, n_in, n_out, net_type, n_val=N_VAL):
    rng = np.random.default_rng(4)
    lo = 0.0 if net_type == "SNN" else -1.0
    sets = []
    for name, n in (("train.hpnb", N_TRAIN), ("val.hpnb", n_val)):
        X = rng.uniform(-1, 1, (n, n_in))
        T = np.full((n, n_out), lo)
        T[np.arange(n), rng.integers(0, n_out, n)] = 1.0
        capi.pack_arrays(os.path.join(d, name), X, T)
        sets += [X, T]
    return sets


def _conf(d, n_in, hid, n_out, net_type="SNN", train="BPM", epochs=5, test_dir="./val.hpnb", **extra):
    formats.write_conf(os.path.join(d, "nn.conf"), name="v", type=net_type, seed=SEED, inputs=n_in, hiddens=hid,
                       outputs=n_out, train=train, sample_dir="./train.hpnb", test_dir=test_dir, mode="batched",
                       batch=B, epochs=epochs, lr=LR, dtype="f64", **extra)


def _run(d, *flags, tool="train_nn", env=None):
    e = dict(os.environ, HPNN_KERNEL_EXACT="1", **(env or {}))
    return subprocess.run([os.path.join(BIN, tool), "-c", "-vv", *flags, "nn.conf"], cwd=d, env=e,
                          capture_output=True, text=True, timeout=300)


def _train(d, *flags, env=None):
    r = _run(d, *flags, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


# ------------------------------------------------------------------ conf and CLI
def test_conf_validate_round_trip(tmp_path):
    d = str(tmp_path)
    kw = dict(name="s", type="SNN", seed=3, inputs=6, hiddens=[4], outputs=3, train="BP", sample_dir="./s",
              test_dir="./s", mode="batched")
    capi.init(0)
    formats.write_conf(os.path.join(d, "a.conf"), validate=5, **kw)
    net = capi.Network(os.path.join(d, "a.conf"))
    assert net.validate == 5
    net.dump_conf(os.path.join(d, "a2.conf"))
    net.close()
    assert "[validate] 5\n" in open(os.path.join(d, "a2.conf")).read()
    net = capi.Network(os.path.join(d, "a2.conf"))
    assert net.validate == 5
    net.set(validate=0)
    assert net.validate == 0
    assert net.validation() == []
    net.close()
    formats.write_conf(os.path.join(d, "b.conf"), **kw)
    net = capi.Network(os.path.join(d, "b.conf"))
    assert net.validate == 0
    net.dump_conf(os.path.join(d, "b2.conf"))
    net.set(validate=3)
    assert net.validate == 3
    net.close()
    assert "validate" not in open(os.path.join(d, "b2.conf")).read()
    for bad in ("0", "x"):
        formats.write_conf(os.path.join(d, "c.conf"), validate=bad, **kw)
        with pytest.raises(RuntimeError):
            capi.Network(os.path.join(d, "c.conf"))


def test_cli_validate_flag(tmp_path):
    d = str(tmp_path)
    _dataset(d, 4, 4, "SNN")
    _conf(d, 4, [8], 4)
    for flags in (("-V",), ("-V", "x"), ("-V", "0")):
        r = subprocess.run([os.path.join(BIN, "train_nn"), "-c", *flags], cwd=d, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode != 0 and "syntax error" in r.stderr, (flags, r.stdout, r.stderr)
    r = _run(d, "-V", "2", tool="run_nn")
    assert r.returncode != 0 and "syntax error" in r.stderr, r.stdout + r.stderr
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-h"], cwd=d, capture_output=True, text=True, timeout=60)
    assert "-V N" in r.stdout


# ------------------------------------------------------------------ CPU engine vs FP64 PyTorch
def _reference_records(w0, X, T, Xv, Tv, net_type, momentum, epochs, every, epoch0=0):
    order = _order(N_TRAIN, SEED)
    Xo, To = torch.tensor(X[order]), torch.tensor(T[order])
    W = [torch.tensor(w) for w in w0]
    V = [torch.zeros_like(w) for w in W] if momentum else None
    Xv, Tv = torch.tensor(Xv), torch.tensor(Tv)
    recs = []
    for e in range(epochs):
        for s in range(0, N_TRAIN, B):
            reference.batched_step(W, Xo[s:s + B], To[s:s + B], net_type, LR, momentum=V, alpha=0.2)
        a = epoch0 + e + 1
        if a % every == 0 or e + 1 == epochs:
            o = reference.forward(W, Xv, net_type)[-1]
            loss = float(reference.loss_per_sample(o, Tv, net_type).mean())
            hits = int((o.argmax(1) == Tv.argmax(1)).sum())
            recs.append((a, loss, hits, Xv.shape[0]))
    return recs


@pytest.mark.parametrize("train", ["BP", "BPM"])
@pytest.mark.parametrize("net_type", ["ANN", "LNN", "SNN"])
@pytest.mark.parametrize("dims", [(4, [8], 4), (20, [16, 8], 5)], ids=["4-8-4", "20-16-8-5"])
def test_cpu_engine_validation_matches_reference(tmp_path, dims, net_type, train):
    n_in, hid, n_out = dims
    d = str(tmp_path)
    X, T, Xv, Tv = _dataset(d, n_in, n_out, net_type)
    _conf(d, n_in, hid, n_out, net_type, train, epochs=5)
    got = _records(_train(d, "-V", "2"))
    w0 = formats.read_kernel(os.path.join(d, "kernel.tmp"))["weights"]
    want = _reference_records(w0, X, T, Xv, Tv, net_type, train == "BPM", 5, 2)
    assert [r[0] for r in got] == [2, 4, 5] and [r[0] for r in want] == [2, 4, 5], got
    for g, w in zip(got, want):
        print("epoch", g[0], "loss", g[1], "reference", w[1], "hits", g[2], w[2])
        assert g[2] == w[2] and g[3] == w[3] == N_VAL
        # the line prints ten decimals of a loss the two FP64 engines agree on to 1e-12 relative
        assert abs(g[1] - w[1]) <= 1e-12 * abs(w[1]) + 0.5e-10, (g, w)


def test_network_api_records_match_the_printed_lines(tmp_path):
    d = str(tmp_path)
    X, T, Xv, Tv = _dataset(d, 20, 5, "SNN")
    _conf(d, 20, [16, 8], 5, epochs=5, device="cpu")
    capi.init(0)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        net = capi.Network("nn.conf")
        net.dump_kernel("k0.txt", exact=True)
        w0 = formats.read_kernel("k0.txt")["weights"]
        net.set(validate=2)
        assert net.train()
        recs = net.validation()
        net.close()
    finally:
        os.chdir(cwd)
    assert [r["epoch"] for r in recs] == [2, 4, 5]
    assert all(r["n"] == N_VAL and 0 <= r["correct"] <= N_VAL for r in recs)
    assert all(abs(r["accuracy"] - r["correct"] / N_VAL) < 1e-12 and r["loss"] > 0 for r in recs)
    want = _reference_records(w0, X, T, Xv, Tv, "SNN", True, 5, 2)
    for r, w in zip(recs, want):
        assert r["correct"] == w[2] and abs(r["loss"] - w[1]) <= 1e-12 * abs(w[1])


def test_validation_leaves_training_unchanged(tmp_path):
    outs = {}
    for tag, flags in (("with", ("-V", "1")), ("without", ())):
        d = str(tmp_path / tag)
        os.makedirs(d)
        _dataset(d, 20, 5, "SNN")
        _conf(d, 20, [16, 8], 5, epochs=3)
        out = _train(d, *flags)
        assert (len(_records(out)) == 3) == (tag == "with"), out[-2000:]
        outs[tag] = open(os.path.join(d, "kernel.opt"), "rb").read()
    assert outs["with"] == outs["without"]


def test_conf_key_validates_like_the_flag(tmp_path):
    d = str(tmp_path)
    _dataset(d, 4, 4, "SNN")
    _conf(d, 4, [8], 4, epochs=4, validate=3)
    assert [r[0] for r in _records(_train(d))] == [3, 4]


def test_resume_numbers_the_records(tmp_path):
    d = str(tmp_path)
    _dataset(d, 20, 5, "SNN")
    _conf(d, 20, [16, 8], 5, epochs=2)
    first = _records(_train(d, "-V", "2", "-r", "state.bin"))
    second = _records(_train(d, "-V", "2", "-r", "state.bin"))
    assert [r[0] for r in first] == [2] and [r[0] for r in second] == [4], (first, second)
    d4 = str(tmp_path / "four")
    os.makedirs(d4)
    _dataset(d4, 20, 5, "SNN")
    _conf(d4, 20, [16, 8], 5, epochs=4)
    whole = _records(_train(d4, "-V", "2"))
    assert [r[0] for r in whole] == [2, 4]
    assert whole[0] == first[0] and whole[1] == second[0]


def test_metrics_hold_the_validation_events(tmp_path):
    d = str(tmp_path)
    _dataset(d, 20, 5, "SNN")
    _conf(d, 20, [16, 8], 5, epochs=5)
    recs = _records(_train(d, "-V", "2", "-M", "m.jsonl"))
    ev = [json.loads(l) for l in open(os.path.join(d, "m.jsonl"))]
    val = [e for e in ev if e["event"] == "validation"]
    assert [e["epoch"] for e in val] == [2, 4, 5]
    for e, r in zip(val, recs):
        assert e["correct"] == r[2] and e["n"] == N_VAL and abs(e["loss"] - r[1]) <= 1e-9
        assert abs(e["accuracy"] - r[2] / N_VAL) < 1e-5
    # each record follows its epoch's "epoch" event, whose fields are the ones it had before
    names = [(e["event"], e.get("epoch")) for e in ev if e["event"] in ("epoch", "validation")]
    assert names == [("epoch", 1), ("epoch", 2), ("validation", 2), ("epoch", 3), ("epoch", 4), ("validation", 4),
                     ("epoch", 5), ("validation", 5)]


def test_missing_or_empty_test_dir_is_an_error(tmp_path):
    d = str(tmp_path)
    _dataset(d, 4, 4, "SNN")
    os.makedirs(os.path.join(d, "empty"))
    for test_dir in ("./nowhere", "./empty"):
        _conf(d, 4, [8], 4, test_dir=test_dir)
        r = _run(d, "-V", "1")
        assert r.returncode != 0 and "[validate]" in r.stderr and "VALIDATION:" not in r.stdout, r.stdout + r.stderr
        assert _run(d).returncode == 0  # without validation the set is not needed


def test_online_mode_warns_and_trains(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(2)
    os.makedirs(os.path.join(d, "samples"))
    for i in range(3):
        t = np.zeros(3)
        t[i] = 1.0
        formats.write_sample(os.path.join(d, "samples", f"s{i}"), rng.uniform(-1, 1, 4), t)
    formats.write_conf(os.path.join(d, "nn.conf"), name="o", type="SNN", seed=3, inputs=4, hiddens=[5], outputs=3,
                       train="BP", sample_dir="./samples", test_dir="./samples", validate=2)
    r = _run(d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[validate] has no effect in online mode" in r.stderr and "TRAINING FILE" in r.stdout
    assert "VALIDATION:" not in r.stdout


# ------------------------------------------------------------------ emulation
def _mnist_like(rows, n_valid, seed=0):
    g = torch.Generator().manual_seed(seed)
    sizes = [784, 128, 64, 10]
    W = [((torch.rand(sizes[l + 1], sizes[l], generator=g) - 0.5) * 2 / sizes[l] ** 0.5) for l in range(3)]
    X = torch.rand(rows, 784, generator=g)
    labels = torch.randint(0, 10, (rows,), generator=g, dtype=torch.int32)
    return sizes, W, X, labels


def test_emulation_matches_fp64_forward():
    rows, n_valid = 256, 250
    sizes, W, X, labels = _mnist_like(rows, n_valid)
    Wb = []
    for l, w in enumerate(W):
        p = torch.zeros(ops.pad_to(w.shape[0], 32), ops.pad_to(w.shape[1], 32))
        p[:w.shape[0], :w.shape[1]] = w
        Wb.append(p.bfloat16())
    Xb = torch.zeros(rows, 800).bfloat16()
    Xb[:, :784] = X.bfloat16()
    vst = torch.zeros(64, 16)
    guess = torch.zeros(rows, dtype=torch.int32)
    ops.mlp3_eval(ops.to_fragment_major(Xb).view(rows // 32, 50, 64, 8), 800, Wb[0], None, Wb[1], Wb[2], 10,
                  ops.TYPE_SNN, labels=labels, n_valid=n_valid, loss_acc=vst[0, 0:1], correct=vst[0, 1:2],
                  guess=guess)
    loss, hits = float(vst[0, 0]), int(vst[0, 1:2].view(torch.int32))
    # FP64 forward of the same BF16-rounded operands
    W64 = [Wb[l][:sizes[l + 1], :sizes[l] if l else 800].double() for l in range(3)]
    T = torch.zeros(rows, 10, dtype=torch.float64)
    T[torch.arange(rows), labels.long()] = 1.0
    o = reference.forward(W64, Xb.double(), "SNN")[-1]
    ref_loss = float(reference.loss_per_sample(o, T, "SNN")[:n_valid].sum())
    ref_hits = int((o.argmax(1) == labels.long())[:n_valid].sum())
    print("loss", loss, "fp64", ref_loss, "hits", hits, ref_hits)
    assert abs(loss - ref_loss) <= 2e-3 * abs(ref_loss) + 1e-3
    assert abs(hits - ref_hits) <= max(2, n_valid // 200)
    assert int((guess[n_valid:] != -1).sum()) == 0
    assert int((guess[:n_valid] == labels[:n_valid]).sum()) == hits


def test_mlp_cpu_evaluate_matches_emulation_and_leaves_stats():
    rows, n_valid = 256, 250
    sizes, W, X, labels = _mnist_like(rows, n_valid, seed=1)
    m = MLP(sizes, "SNN", batch=256, device="cpu", weights=[w.double() for w in W])
    Xp = m.prepare_input(X)
    m.stats[3, 0] = 7.0
    before = m.stats.clone()
    m.reset_eval_stats()
    g = m.evaluate(Xp, labels=labels, n_valid=n_valid, guess=True)
    loss, hits = m.read_eval_stats()
    assert torch.equal(m.stats, before) and m.read_stats()[0] == 7.0
    vst = torch.zeros(64, 16)
    guess = torch.zeros(rows, dtype=torch.int32)
    ops.mlp3_eval(ops.to_fragment_major(Xp).view(rows // 32, 50, 64, 8), 800, m.Wb[0], None, m.Wb[1], m.Wb[2], 10,
                  ops.TYPE_SNN, labels=labels, n_valid=n_valid, loss_acc=vst[0, 0:1], correct=vst[0, 1:2],
                  guess=guess)
    assert hits == int(vst[0, 1:2].view(torch.int32)) and abs(loss - float(vst[0, 0])) <= 1e-6 * abs(loss)
    assert torch.equal(g, guess)
    # a second pass accumulates; the reset clears
    m.evaluate(Xp, labels=labels, n_valid=n_valid)
    assert m.read_eval_stats()[1] == 2 * hits
    m.reset_eval_stats()
    assert m.read_eval_stats() == (0.0, 0)


def test_validate_commit_emulation_files_records_in_order():
    slots = torch.zeros(64, 16)
    hist = torch.zeros(2, 2, dtype=torch.float64)
    cur = torch.zeros(1, dtype=torch.int32)
    for k in range(3):  # the third pass finds the history full: dropped, slots still zeroed
        slots[:, 0] = 0.5 * (k + 1)
        slots[:, 1:2].view(torch.int32)[:] = k + 1
        ops.validate_commit(slots, hist, cur)
        assert int(slots.count_nonzero()) == 0
    assert int(cur[0]) == 2
    assert hist[:, 0].tolist() == [32.0, 64.0]
    assert hist[:, 1:2].view(torch.int32)[:, 0].tolist() == [64, 128]
