"""[validate] N on the GPU: the forward-only tile kernel (hpnn_mlp3_eval) against its PyTorch
emulation and against the training front's own numbers, the commit kernel inside a captured
graph, evaluate leaving a training run bit for bit alone, the fused against the per-layer
evaluation path, and train_nn -V on the FP64 / FP32 / BF16 engines against the FP64 CPU
engine and the Python plan."""
import ctypes
import ctypes.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP
from hpnn_amd.utils import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
TY = {"ANN": ops.TYPE_ANN, "LNN": ops.TYPE_LNN, "SNN": ops.TYPE_SNN}
VAL_RE = re.compile(r"VALIDATION: epoch (\d+) loss=([0-9.eE+-]+) acc=(\d+)/(\d+)")


def _records(out):
    return [(int(e), float(l), int(c), int(n)) for e, l, c, n in VAL_RE.findall(out)]


def _stats(st):
    s = st.cpu()
    return float(s[:, 0].double().sum()), int(s[:, 1].contiguous().view(torch.int32).long().sum())


def _pad_w(w, rows, cols):
    p = torch.zeros(rows, cols)
    p[:w.shape[0], :w.shape[1]] = w
    return p.bfloat16()


# ------------------------------------------------------------------ kernel against emulation
@pytest.mark.gpu
@pytest.mark.parametrize("net,n_out,dense,u8,n_in,K0,Bp,n_valid,grid", [
    ("SNN", 10, False, True, 784, 800, 256, 256, 0),   # one full tile
    ("SNN", 10, False, True, 784, 800, 256, 1, 0),     # masks: one valid row
    ("SNN", 24, True, False, 784, 800, 768, 700, 1),   # one workgroup runs three tiles (LDS images reused)
    ("ANN", 30, False, True, 784, 800, 768, 768, 2),   # uneven tiles per workgroup, two output tiles
    ("LNN", 12, True, False, 200, 256, 512, 500, 0),   # the K0 = 256 form
])
def test_eval_kernel_matches_emulation(gpu, net, n_out, dense, u8, n_in, K0, Bp, n_valid, grid):
    g = torch.Generator().manual_seed(Bp + n_out + n_valid)
    sizes = [n_in, 128, 64, n_out]
    W = [(torch.rand(sizes[l + 1], sizes[l], generator=g) - 0.5) * 2 / sizes[l] ** 0.5 for l in range(3)]
    Wb = [_pad_w(W[0], 128, K0), _pad_w(W[1], 64, 128), _pad_w(W[2], 32, 64)]
    if u8:
        X = torch.zeros(Bp, K0, dtype=torch.uint8)
        X[:, :n_in] = torch.randint(0, 256, (Bp, n_in), dtype=torch.uint8, generator=g)
        xscale = float(torch.tensor(1.0 / 255.0, dtype=torch.float32))
    else:
        X = torch.zeros(Bp, K0)
        X[:, :n_in] = torch.rand(Bp, n_in, generator=g) - 0.5
        X, xscale = X.bfloat16(), 1.0
    Xg = ops.to_fragment_major(X).view(Bp // 32, K0 // 16, 64, 8).contiguous()
    t_hi, t_lo = (1.0, 0.0) if net == "SNN" else (1.0, -1.0)
    lab = torch.randint(0, n_out, (Bp,), dtype=torch.int32, generator=g)
    T = None
    if dense:
        T = torch.full((Bp, n_out), t_lo)
        T[torch.arange(Bp), lab.long()] = t_hi

    def run(dev):
        st = torch.zeros(64, 16, device=dev)
        gs = torch.full((Bp,), -7, dtype=torch.int32, device=dev)
        kw = dict(T=T.to(dev)) if dense else dict(labels=lab.to(dev))
        W0f = ops.frag_major(Wb[0]).contiguous().to(dev) if dev == "cuda" else None
        ops.mlp3_eval(Xg.to(dev), K0, Wb[0].to(dev), W0f, Wb[1].to(dev), Wb[2].to(dev), n_out, TY[net], t_hi=t_hi,
                      t_lo=t_lo, n_valid=n_valid, loss_acc=st[0, 0:1], correct=st[0, 1:2], guess=gs, xscale=xscale,
                      grid=grid, **kw)
        if dev == "cuda":
            torch.cuda.synchronize()
        return _stats(st) + (gs.cpu(),)

    loss, hits, gs = run("cuda")
    loss_r, hits_r, gs_r = run("cpu")
    tol = max(2, n_valid // 200)
    print(f"loss {loss} emulation {loss_r}; hits {hits} / {hits_r}; guess mismatches "
          f"{int((gs[:n_valid] != gs_r[:n_valid]).sum())}")
    assert abs(loss - loss_r) <= 2e-3 * abs(loss_r) + 1e-3, (loss, loss_r)
    assert abs(hits - hits_r) <= tol, (hits, hits_r)
    assert int((gs[:n_valid] != gs_r[:n_valid]).sum()) <= tol
    assert int((gs[n_valid:] != -1).sum()) == 0 and int((gs[:n_valid] < 0).sum()) == 0
    assert int((gs[:n_valid] >= n_out).sum()) == 0


# ------------------------------------------------------------------ same numbers as training
@pytest.mark.gpu
@pytest.mark.parametrize("net,dense,u8", [("SNN", False, True), ("ANN", True, False)])
def test_evaluate_reports_the_training_fronts_numbers(gpu, net, dense, u8):
    Bp, n_out, n_valid = 1024, 10, 1000
    torch.manual_seed(5)
    m = MLP([784, 128, 64, n_out], net, batch=Bp, momentum=True, seed=5, fused="t")
    X = torch.randint(0, 256, (Bp, 784), dtype=torch.uint8) if u8 else torch.rand(Bp, 784) - 0.5
    Xg = m.prepare_input(X.cuda())
    lab = torch.randint(0, n_out, (Bp,), dtype=torch.int32)
    kw = dict(labels=lab.cuda())
    if dense:
        T = torch.full((Bp, n_out), -1.0)
        T[torch.arange(Bp), lab.long()] = 1.0
        kw = dict(T=T.cuda())
    m.reset_stats()
    m.front(Xg, n_valid=n_valid, **kw)
    tl, th = m.read_stats()
    m.reset_stats()
    m.reset_eval_stats()
    gs = m.evaluate(Xg, n_valid=n_valid, guess=True, **kw)
    el, eh = m.read_eval_stats()
    print(f"{net}: front loss {tl} hits {th}; evaluate loss {el} hits {eh}")
    assert eh == th
    # the same <= 1024 non-negative FP32 terms in another order: (n - 1) 2^-24 ~ 6e-5 at worst
    assert abs(el - tl) <= 1e-4 * abs(tl)
    assert int((gs[:n_valid].cpu() == lab[:n_valid]).sum()) == eh
    assert int((gs[n_valid:] != -1).sum()) == 0
    assert m.read_stats() == (0.0, 0)  # the training slots were not touched


@pytest.mark.gpu
def test_commit_kernel_files_records_from_a_captured_graph(gpu):
    Bp, n_out = 512, 10
    torch.manual_seed(2)
    m = MLP([784, 128, 64, n_out], "SNN", batch=Bp, momentum=True, seed=2, fused="t")
    sets = []
    for n_valid in (512, 300):
        Xg = m.prepare_input(torch.randint(0, 256, (Bp, 784), dtype=torch.uint8).cuda())
        lab = torch.randint(0, n_out, (Bp,), dtype=torch.int32).cuda()
        m.reset_eval_stats()
        m.evaluate(Xg, labels=lab, n_valid=n_valid)
        sets.append((Xg, lab, n_valid, m.read_eval_stats()))
    m.reset_eval_stats()
    vst = m.buf[("vstats", -1)]
    hist = torch.zeros(5, 2, dtype=torch.float64, device="cuda")
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.validate_commit(vst, hist, cur)  # code object loaded before the capture; files an empty record
    torch.cuda.synchronize()
    assert int(cur.item()) == 1 and float(hist[0, 0]) == 0.0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for Xg, lab, n_valid, _ in sets:
            m.evaluate(Xg, labels=lab, n_valid=n_valid)
            ops.validate_commit(vst, hist, cur)
    for _ in range(3):  # 1 + 6 passes into 5 records: the last two are dropped, nothing is overrun
        g.replay()
    torch.cuda.synchronize()
    assert int(cur.item()) == 5 and m.read_eval_stats() == (0.0, 0)
    h = hist.cpu()
    hits = h[:, 1:2].contiguous().view(torch.int32)[:, 0].tolist()
    for i in range(1, 5):
        want = sets[(i - 1) % 2][3]
        assert hits[i] == want[1] and abs(float(h[i, 0]) - want[0]) <= 1e-4 * abs(want[0]), (i, h[i], want)


# ------------------------------------------------------------------ evaluate leaves training alone
@pytest.mark.gpu
@pytest.mark.parametrize("sizes,Bp,fused,rows", [([784, 128, 64, 10], 512, "t", 768), ([20, 16, 8, 5], 128, False, 300)])
def test_evaluate_leaves_training_alone(gpu, sizes, Bp, fused, rows):
    n_out = sizes[-1]
    g = torch.Generator().manual_seed(9)
    X = [torch.rand(Bp, sizes[0], generator=g) - 0.5 for _ in range(3)]
    lab = [torch.randint(0, n_out, (Bp,), dtype=torch.int32, generator=g).cuda() for _ in range(3)]
    Xe = torch.rand(rows, sizes[0], generator=g) - 0.5
    le = torch.randint(0, n_out, (rows,), dtype=torch.int32, generator=g).cuda()
    ms = []
    for with_eval in (False, True):
        m = MLP(sizes, "SNN", batch=Bp, momentum=True, seed=4, fused=fused)
        assert m.fused_mode == (fused or None)
        Xv = m.prepare_input(Xe.cuda())
        for i in range(3):
            m.train_step(m.prepare_input(X[i].cuda()), labels=lab[i], lr=0.05)
            if with_eval:
                m.evaluate(Xv, labels=le, n_valid=rows)
        torch.cuda.synchronize()
        ms.append(m)
    a, b = ms
    for l in range(3):
        for name in ("W32", "V32", "Wb", "Wt"):
            ta, tb = getattr(a, name)[l], getattr(b, name)[l]
            assert torch.equal(ta.view(torch.int16 if ta.element_size() == 2 else torch.int32),
                               tb.view(torch.int16 if tb.element_size() == 2 else torch.int32)), (name, l)
    assert a.read_stats() == b.read_stats()
    assert a.healthy() and b.healthy()
    assert a.read_eval_stats() == (0.0, 0) and b.read_eval_stats()[0] > 0


# ------------------------------------------------------------------ fused against per-layer
@pytest.mark.gpu
def test_fused_evaluation_matches_per_layer(gpu, monkeypatch):
    n, n_out = 1000, 10
    g = torch.Generator().manual_seed(12)
    X = torch.randint(0, 256, (n, 784), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, n_out, (n,), dtype=torch.int32, generator=g).cuda()
    res = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("HPNN_EVAL_FUSED", raising=False)
        else:
            monkeypatch.setenv("HPNN_EVAL_FUSED", env)
        m = MLP([784, 128, 64, n_out], "SNN", batch=256, momentum=True, seed=6, fused="t")
        assert m.plan.eval_is_fused() == (env is None)
        gs = m.evaluate(m.prepare_input(X.cuda()), labels=lab, n_valid=n, guess=True)
        res.append(m.read_eval_stats() + (gs[:n].cpu(),))
        assert int((gs[n:] != -1).sum()) == 0
    (lf, hf, gf), (lp, hp, gp) = res
    print(f"fused loss {lf} hits {hf}; per-layer loss {lp} hits {hp}; guesses differ {int((gf != gp).sum())}")
    assert abs(hf - hp) <= 0.01 * n and abs(lf - lp) <= 1e-2 * abs(lp)
    assert int((gf != gp).sum()) <= 0.01 * n


# ------------------------------------------------------------------ train_nn
def _run(cmd, cwd, extra_env=None, check=True):
    env = dict(os.environ)
    env.pop("HPNN_FORCE_CPU", None)
    env.update(extra_env or {})
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def _pack(d, name, n, n_in, n_out, net, rng, pixels=False):
    X = rng.integers(0, 256, (n, n_in)).astype(np.float64) if pixels else rng.uniform(-1, 1, (n, n_in))
    lab = rng.integers(0, n_out, n)
    T = np.full((n, n_out), 0.0 if net == "SNN" else -1.0)
    T[np.arange(n), lab] = 1.0
    capi.pack_arrays(os.path.join(d, name), X, T)
    return X, T, lab


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-12), ("f32", 1e-4)])
@pytest.mark.parametrize("net,train", [("ANN", "BPM"), ("SNN", "BP")])
def test_train_nn_fp_validation_matches_cpu_engine(tmp_path, gpu, monkeypatch, dtype, tol, net, train):
    monkeypatch.delenv("HPNN_FORCE_CPU", raising=False)
    d = str(tmp_path)
    rng = np.random.default_rng(1)
    _pack(d, "train.hpnb", 300, 20, 5, net, rng)
    _pack(d, "val.hpnb", 100, 20, 5, net, rng)
    formats.write_conf(os.path.join(d, "nn.conf"), name="fp", type=net, seed=9, inputs=20, hiddens=[16, 8], outputs=5,
                       train=train, sample_dir=os.path.join(d, "train.hpnb"), test_dir=os.path.join(d, "val.hpnb"),
                       mode="batched", batch=64, epochs=4, lr=0.05, dtype=dtype)
    cpu = _records(_run([os.path.join(BIN, "train_nn"), "-c", "-vv", "-V", "1", "nn.conf"], d).stdout)
    out = _run([os.path.join(BIN, "train_nn"), "-vv", "-d", dtype, "-V", "1", "nn.conf"], d).stdout
    assert f"batched GPU training: {dtype}" in out, out[-2000:]
    got = _records(out)
    assert [r[0] for r in cpu] == [1, 2, 3, 4] and [r[0] for r in got] == [1, 2, 3, 4], (cpu, got)
    for g, c in zip(got, cpu):
        print(f"{net} {dtype} epoch {g[0]}: loss {g[1]} cpu {c[1]} hits {g[2]} cpu {c[2]}")
        assert g[3] == c[3] == 100
        # each line prints its loss rounded to ten decimals
        assert abs(g[1] - c[1]) <= tol * abs(c[1]) + 1e-10, (g, c)
        assert g[2] == c[2] if dtype == "f64" else abs(g[2] - c[2]) <= max(2, 100 // 200)
    if dtype != "f64":
        return
    # the full doubles through the C API, both engines in this process
    capi.init(0)
    recs = {}
    for dev in ("cpu", "gpu"):
        net_ = capi.Network(os.path.join(d, "nn.conf")).set(device=dev, validate=1)
        assert net_.train()
        recs[dev] = net_.validation()
        net_.close()
    assert [r["epoch"] for r in recs["gpu"]] == [1, 2, 3, 4]
    for g, c in zip(recs["gpu"], recs["cpu"]):
        print(f"{net} f64 epoch {g['epoch']}: loss {g['loss']!r} cpu {c['loss']!r}")
        assert g["correct"] == c["correct"] and abs(g["loss"] - c["loss"]) <= tol * abs(c["loss"]), (g, c)


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


@pytest.mark.gpu
@pytest.mark.parametrize("reshuffle", [False, True], ids=["once", "R"])
def test_train_nn_bf16_validation_equals_python_plan(tmp_path, gpu, reshuffle):
    n, nv, B, seed, epochs, n_out = 1024, 600, 256, 11, 3, 10
    d = str(tmp_path)
    rng = np.random.default_rng(5)
    X, T, _ = _pack(d, "train.hpnb", n, 784, n_out, "SNN", rng, pixels=True)
    Xv, _, labv = _pack(d, "val.hpnb", nv, 784, n_out, "SNN", rng, pixels=True)
    formats.write_conf(os.path.join(d, "nn.conf"), name="t", type="SNN", seed=seed, inputs=784, hiddens=[128, 64],
                       outputs=n_out, train="BPM", sample_dir="./train.hpnb", test_dir="./val.hpnb", mode="batched",
                       batch=B, epochs=epochs, dtype="bf16", lr=0.01)
    flags = ["-R"] if reshuffle else []
    r = _run([os.path.join(BIN, "train_nn"), "-vvv", "-V", "1", *flags, "nn.conf"], d)
    assert "batched plan: mode t" in r.stdout, r.stdout[-3000:]
    got = _records(r.stdout)
    with_v = open(os.path.join(d, "kernel.opt")).read()
    _run([os.path.join(BIN, "train_nn"), "-vvv", *flags, "nn.conf"], d)
    assert open(os.path.join(d, "kernel.opt")).read() == with_v  # validation changes no weight

    m = MLP([784, 128, 64, n_out], "SNN", batch=B, momentum=True, seed=seed)
    assert m.fused_mode == "t" and m.plan.eval_is_fused()
    order = _order(n, seed)
    Xo, To = X[order], T[order]
    Xvp = m.prepare_input(torch.tensor(Xv).to(torch.uint8), pixel_scale=1.0)
    lv = torch.tensor(labv, dtype=torch.int32).cuda()
    want = []
    for e in range(epochs):
        perm = capi.hpnn_epoch_perm(n, seed, e).astype(np.int64) if reshuffle else np.arange(n)
        Xe, Te = Xo[perm], To[perm]
        for s in range(n // B):
            Xp = m.prepare_input(torch.tensor(Xe[s * B:(s + 1) * B]).to(torch.uint8), pixel_scale=1.0)
            Tt = torch.tensor(Te[s * B:(s + 1) * B], dtype=torch.float32, device="cuda")
            m.train_step(Xp, T=Tt.contiguous(), n_valid=B, lr=0.01, alpha=0.2)
        m.reset_eval_stats()
        m.evaluate(Xvp, labels=lv, n_valid=nv)
        loss, hits = m.read_eval_stats()
        want.append((e + 1, loss / nv, hits, nv))
    assert [g[0] for g in got] == [1, 2, 3], r.stdout[-3000:]
    for g, w in zip(got, want):
        print(f"epoch {g[0]}: train_nn loss {g[1]} hits {g[2]}; plan loss {w[1]} hits {w[2]}")
        assert g[2] == w[2] and g[3] == nv
        assert abs(g[1] - w[1]) <= 1e-4 * abs(w[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_train_nn_validation_graph_equals_eager(tmp_path, gpu, dtype):
    """16 batches an epoch: replays of 2 epochs with -V 2, and a last replay of one"""
    d = str(tmp_path)
    rng = np.random.default_rng(3)
    _pack(d, "train.hpnb", 4096, 20, 5, "SNN", rng)
    _pack(d, "val.hpnb", 300, 20, 5, "SNN", rng)
    formats.write_conf(os.path.join(d, "nn.conf"), name="g", type="SNN", seed=4, inputs=20, hiddens=[16, 8], outputs=5,
                       train="BPM", sample_dir="./train.hpnb", test_dir="./val.hpnb", mode="batched", batch=256,
                       epochs=5, lr=0.05, dtype=dtype)
    hist = {}
    for tag, env in (("graph", {}), ("eager", {"HPNN_GRAPH": "0"})):
        out = _run([os.path.join(BIN, "train_nn"), "-vv", "-V", "2", "nn.conf"], d, extra_env=env).stdout
        hist[tag] = _records(out)
        assert "300 held-out samples validated every 2 epochs" in out, out[-2000:]
    assert [r[0] for r in hist["graph"]] == [2, 4, 5], hist
    assert [(r[0], r[2], r[3]) for r in hist["graph"]] == [(r[0], r[2], r[3]) for r in hist["eager"]], hist
    for a, b in zip(hist["graph"], hist["eager"]):
        assert abs(a[1] - b[1]) <= 1e-4 * abs(b[1])


@pytest.mark.gpu
def test_train_nn_validation_metrics_events(tmp_path, gpu):
    d = str(tmp_path)
    rng = np.random.default_rng(6)
    _pack(d, "train.hpnb", 512, 20, 5, "SNN", rng)
    _pack(d, "val.hpnb", 100, 20, 5, "SNN", rng)
    formats.write_conf(os.path.join(d, "nn.conf"), name="m", type="SNN", seed=4, inputs=20, hiddens=[16, 8], outputs=5,
                       train="BP", sample_dir="./train.hpnb", test_dir="./val.hpnb", mode="batched", batch=128,
                       epochs=3, lr=0.05, dtype="bf16")
    import json
    plain = _records(_run([os.path.join(BIN, "train_nn"), "-vv", "-V", "2", "nn.conf"], d).stdout)
    recs = _records(_run([os.path.join(BIN, "train_nn"), "-vv", "-V", "2", "-M", "m.jsonl", "nn.conf"], d).stdout)
    assert [(r[0], r[2]) for r in recs] == [(r[0], r[2]) for r in plain] and [r[0] for r in recs] == [2, 3]
    ev = [json.loads(l) for l in open(os.path.join(d, "m.jsonl"))]
    val = [e for e in ev if e["event"] == "validation"]
    assert [(e["epoch"], e["correct"], e["n"], e["engine"]) for e in val] == [(r[0], r[2], 100, "gpu") for r in recs]
    for e, r in zip(val, recs):
        assert abs(e["loss"] - r[1]) <= 1e-9


@pytest.mark.gpu
def test_multi_replica_engines_refuse_validation(tmp_path, gpu):
    d = str(tmp_path)
    rng = np.random.default_rng(2)
    _pack(d, "train.hpnb", 256, 20, 4, "SNN", rng)
    kw = dict(name="r", type="SNN", seed=3, inputs=20, hiddens=[16], outputs=4, train="BP",
              sample_dir="./train.hpnb", test_dir="./train.hpnb", mode="batched", batch=128, epochs=2, dtype="f32")
    formats.write_conf(os.path.join(d, "nn.conf"), **kw)
    r = _run([os.path.join(BIN, "train_nn"), "-v", "-V", "1", "nn.conf"], d, extra_env={"HPNN_LOOPBACK_RANKS": "2"},
             check=False)
    assert r.returncode != 0 and "[validate] is not supported" in r.stdout + r.stderr
    assert "VALIDATION:" not in r.stdout
    formats.write_conf(os.path.join(d, "nn.conf"), parallel="tp", **kw)
    r = _run([os.path.join(BIN, "train_nn"), "-v", "-V", "1", "nn.conf"], d, check=False)
    assert r.returncode != 0 and "[validate] is not supported" in r.stdout + r.stderr
    assert "VALIDATION:" not in r.stdout
