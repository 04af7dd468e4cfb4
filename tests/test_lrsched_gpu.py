"""[lr_schedule] on the GPU: the kernels of csrc/gpu/kernels_lrsched.hip bit for bit against the
host entry points of include/libhpnn/lrsched.h and against exact FP64 references, the rate read
from device memory inside a captured graph, the whole BF16 plan on the integer-exact fixture, the
f64 / f32 engines against the FP64 CPU oracle, train_nn -d bf16 against the Python plan, exact
resume, [keep_best], and an unscheduled plan untouched.

Every case prints what it measured."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP
from hpnn_amd.utils import formats
from tests import adam_common as A
from tests import front_exact_common as fc
from tests import lrsched_common as K
from tests import upd_common as U

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
BIG = 1_048_576 + 3  # the smallest n that enters the grid-stride loop (4096 x 256 elements per pass)


def _segment(n, S, off, goff, dtype, seed):
    """one CPU segment inside sentinel (NaN) filled buffers: w and v `off` elements from the start
    of theirs, the slabs [S, n] `goff` elements from the start of theirs with rows n + 3 apart;
    elements 0..2 (n permitting) have g = 0 and v = 0"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    v = (0.1 * torch.randn(n, generator=g, dtype=torch.float64)).to(dtype)
    sl = torch.randn(S, n, generator=g, dtype=torch.float64).to(dtype)
    if n > 3:
        sl[:, :3] = 0.0
        v[:3] = 0.0
    seg, bases = {}, {}
    bases["slab"], seg["slab"] = U.slab_window(sl, goff)
    for k, t in (("w", w), ("v", v)):
        bases[k], seg[k] = U.window(t, off)
    return seg, bases


def _state(epochs=3, **kw):
    cfg = dict(kind="step", lr0=0.3, gamma=0.9, period=1)
    cfg.update(kw)
    st = ops.lr_state(**cfg)
    for _ in range(epochs):
        ops.lr_advance(st)
    return st


def _run_fp(sizes, S, off, goff, dtype, momentum, seed):
    """the kernel on `sizes` segments in ONE launch against the host entry point: every bit of w
    and v, the sentinels around them, the slabs read only"""
    cpu = [_segment(n, S, off, goff, dtype, seed + i) for i, n in enumerate(sizes)]
    st = _state()
    dev = [U.to_cuda(seg, bases) for seg, bases in cpu]
    ops.sgd_sched_fp(ops.SgdSchedTable([d for d, _ in dev], momentum=momentum), st.cuda(), scale=1.0 / 7, alpha=0.25)
    torch.cuda.synchronize()
    for (seg, bases), (d1, b1) in zip(cpu, dev):
        hw, hv = seg["w"].clone(), seg["v"].clone()
        ops.sgd_sched_fp(ops.SgdSchedTable([dict(w=hw, v=hv, slab=seg["slab"])], momentum=momentum), st, scale=1.0 / 7,
                         alpha=0.25)
        who = f"n {seg['w'].numel()} S {S} off {off} goff {goff} {dtype} momentum {momentum}"
        assert torch.equal(U.ibits(d1["w"].cpu()), U.ibits(hw)), who
        assert torch.equal(U.ibits(d1["v"].cpu()), U.ibits(hv if momentum else seg["v"])), who
        assert not torch.equal(hw, seg["w"]), who
        for k in ("w", "v", "slab"):
            mask = torch.ones_like(bases[k], dtype=torch.bool)
            mask.as_strided(seg[k].shape, seg[k].stride(), seg[k].storage_offset()).fill_(False)
            assert torch.equal(U.ibits(b1[k].cpu())[mask], U.ibits(bases[k])[mask]), f"{who}: {k} sentinels written"
        assert torch.equal(U.ibits(d1["slab"].cpu()), U.ibits(seg["slab"])), "the slabs are read only"
        if seg["w"].numel() > 3:  # g = 0 with v = 0 keeps w's bits
            assert torch.equal(U.ibits(d1["w"].cpu()[:3]), U.ibits(seg["w"][:3]))


# ------------------------------------------------------------------ 1. hpnn_sgd_sched_fp
@pytest.mark.gpu
@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sgd_sched_fp_equals_the_host_form(gpu, dtype, momentum):
    # off 0: W on a 16-byte boundary; off 1: one element off it (the unaligned head); goff != off: G aligned
    # differently from W (every chunk element by element)
    cases = [([n], S, off, goff) for n in (1, 3, 5, 4099) for S in (1, 2, 3) for off, goff in ((0, 0), (1, 1), (0, 1))]
    cases += [([4099, 3, 5], 2, 1, 1), ([5, 4099, 1], 3, 0, 1)]  # three segments in one table
    for i, (sizes, S, off, goff) in enumerate(cases):
        _run_fp(sizes, S, off, goff, dtype, momentum, 100 + i)
    print(f"sgd_sched_fp {dtype} momentum {momentum}: {len(cases)} cases bit-equal to the host entry point")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sgd_sched_fp_grid_stride_loop(gpu, dtype):
    _run_fp([BIG], 2, 1, 1, dtype, True, 7)
    _run_fp([BIG, 5], 1, 0, 0, dtype, False, 9)


@pytest.mark.gpu
def test_sgd_sched_table_refusals_write_nothing(gpu):
    w = torch.ones(16, device="cuda")
    ok = dict(w=w, v=w.clone(), slab=torch.ones(2, 16, device="cuda"))
    ops.SgdSchedTable([ok], momentum=True)
    with pytest.raises(ValueError):
        ops.SgdSchedTable([ok] * 17, momentum=True)
    nat = ops.native()
    s = torch.cuda.current_stream().cuda_stream
    tb = torch.full((17, 7), -7, dtype=torch.int64, device="cuda")
    row = (w.data_ptr(), ok["v"].data_ptr(), ok["slab"].data_ptr(), 2, 16, 16)
    assert nat.sgd_sched_table(0, tb.data_ptr(), [row] * 17, 1, s) == -1      # 17 segments
    assert nat.sgd_sched_table(0, tb.data_ptr(), [(0,) + row[1:]], 1, s) == -1  # a null pointer
    assert nat.sgd_sched_table(0, tb.data_ptr(), [(row[0], 0) + row[2:]], 1, s) == -1  # BPM without V
    assert nat.sgd_sched_table(1, tb.data_ptr(), [(row[0] + 4,) + row[1:]], 1, s) == -1  # a misaligned double
    assert nat.sgd_sched_table(0, tb.data_ptr(), [row[:4] + (8, 16)], 1, s) == -1  # overlapping slabs
    assert nat.sgd_sched_table(0, tb.data_ptr(), [row[:5] + (0,)], 1, s) == -1  # n = 0
    torch.cuda.synchronize()
    assert bool((tb == -7).all()), "a refused table wrote something"
    st = _state().cuda()
    assert nat.sgd_sched_fp(0, tb.data_ptr(), 17, 1.0, 0.0, 1, st.data_ptr(), s) == -1
    assert nat.sgd_sched_fp(0, tb.data_ptr(), 1, 1.0, 0.0, 1, 0, s) == -1
    assert nat.lr_advance(0, 0, 0, 0, 0, s) == -1 and nat.lr_plateau(0, 0, st.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and bool((ok["v"] == 1).all())


# ------------------------------------------------------------------ 2. hpnn_sgd_sched_multi
LAYERS = {"32x32": (32, 32, False), "64x96": (64, 96, False), "128x800": (128, 800, True)}


def _check_copies(W1, Wb, Wt, Wf):
    assert torch.equal(Wb, W1.bfloat16()) and torch.equal(Wt, Wb.t())
    if Wf is not None:
        assert torch.equal(Wf, ops.frag_major(Wb).reshape(-1))  # the layout of hpnn_sgd_update_multi's Wf


@pytest.mark.gpu
@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
@pytest.mark.parametrize("S", [1, 2, 24])
@pytest.mark.parametrize("names", [["32x32"], ["64x96"], ["128x800"], ["32x32", "64x96", "128x800"]],
                         ids=["32x32", "64x96", "128x800", "all"])
def test_sgd_sched_multi_exact_on_integers(gpu, names, S, momentum):
    """integer gradients in [-3, 3], W and V multiples of 2^-6 below 4, lr = 2^-2 (step, two cuts
    from 1), alpha = 2^-1, scale = 2^-3: every sum, product and stepped value is an FP32 number, so
    any summation order gives the FP64 reference's bits"""
    st = _state(epochs=3, lr0=1.0, gamma=0.5)
    lr, alpha, scale = ops.read_lr_state(st)["lr"], 0.5, 0.125
    assert lr == 0.25
    g = torch.Generator().manual_seed(11 + S)
    cpu = []
    for n in names:
        N, Kk, frag = LAYERS[n]
        cpu.append(dict(W=torch.randint(-256, 257, (N, Kk), generator=g).float() / 64,
                        V=torch.randint(-256, 257, (N, Kk), generator=g).float() / 64 * (1.0 if momentum else 0.0),
                        G=torch.randint(-3, 4, (S, N, Kk), generator=g).float(), frag=frag))
    dev = [U.multi_dev(c, ("V",)) for c in cpu]
    ops.sgd_sched_multi(dev, st.cuda(), alpha=alpha, scale=scale, momentum=momentum)
    torch.cuda.synchronize()
    for c, d in zip(cpu, dev):
        W1, V1, G1, Wb, Wt, Wf = [None if t is None else t.cpu() for t in d]
        gs = c["G"].double().sum(0) * scale
        if momentum:
            v = c["V"].double() + lr * gs
            w_ref, v_ref = c["W"].double() + v, v * alpha
        else:
            w_ref, v_ref = c["W"].double() + lr * gs, c["V"].double()
        assert torch.equal(w_ref.float().double(), w_ref) and torch.equal(v_ref.float().double(), v_ref)
        assert torch.equal(W1, w_ref.float()) and torch.equal(V1, v_ref.float()), (tuple(c["W"].shape), S)
        assert torch.equal(G1, c["G"])
        _check_copies(W1, Wb, Wt, Wf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYERS))
def test_sgd_sched_multi_random_equals_the_host_form(gpu, name):
    """random data: the kernel's one summation order, restated on the host, bit for bit"""
    N, Kk, frag = LAYERS[name]
    st = _state()
    for S, momentum in ((1, True), (2, False), (24, True)):
        g = torch.Generator().manual_seed(S)
        c = dict(W=torch.randn(N, Kk, generator=g) / math.sqrt(Kk), V=0.1 * torch.randn(N, Kk, generator=g),
                 G=torch.randn(S, N, Kk, generator=g), frag=frag)
        c["G"][:, -3:, :] = 0.0  # rows that behave like the plan's zero padding
        c["W"][-3:], c["V"][-3:] = 0.0, 0.0
        d = U.multi_dev(c, ("V",))
        ops.sgd_sched_multi([d], st.cuda(), alpha=0.2, scale=1.0 / 5, momentum=momentum)
        torch.cuda.synchronize()
        W1, V1, G1, Wb, Wt, Wf = [None if t is None else t.cpu() for t in d]
        hw, hv = c["W"].clone(), c["V"].clone()
        ops.sgd_sched_multi([(hw, hv, c["G"], torch.empty_like(Wb), torch.empty_like(Wt), None)], st, alpha=0.2,
                            scale=1.0 / 5, momentum=momentum)
        assert torch.equal(U.ibits(W1), U.ibits(hw)) and torch.equal(U.ibits(V1), U.ibits(hv if momentum else c["V"]))
        assert not W1[-3:].any() and not V1[-3:].any()  # g = 0, v = 0 rows stay exactly 0
        _check_copies(W1, Wb, Wt, Wf)


@pytest.mark.gpu
def test_sgd_sched_multi_goes_in_groups_past_8_layers(gpu):
    st = _state(epochs=1, lr0=0.5, gamma=0.5)
    g = torch.Generator().manual_seed(3)
    cpu = [dict(W=torch.randint(-8, 9, (32, 32), generator=g).float(), V=torch.zeros(32, 32),
                G=torch.randint(-3, 4, (2, 32, 32), generator=g).float(), frag=False) for _ in range(11)]
    dev = [U.multi_dev(c, ("V",)) for c in cpu]
    ops.sgd_sched_multi(dev, st.cuda(), scale=1.0, momentum=False)
    torch.cuda.synchronize()
    for c, d in zip(cpu, dev):
        assert torch.equal(d[0].cpu(), c["W"] + 0.5 * c["G"].sum(0))
    with pytest.raises(RuntimeError):
        ops.sgd_sched_multi(dev + dev[:6], st.cuda())  # 17 layers


# ------------------------------------------------------------------ 3. the rate is read when the launch runs
@pytest.mark.gpu
@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_a_captured_epoch_reads_its_rate_when_it_runs(gpu, adam):
    """ONE captured graph [advance, update] replayed four times under step, gamma 0.5, period 1:
    every replay must apply its own, exact rate 2^-e"""
    n = 4099
    g = torch.Generator().manual_seed(2)
    w0 = torch.randint(-64, 65, (n,), generator=g).double()
    G = torch.randint(-3, 4, (1, n), generator=g).double()
    w, slab = w0.clone().cuda(), G.clone().cuda()
    sd = ops.lr_state("step", lr0=1.0, gamma=0.5, period=1).cuda()
    ad = ops.adam_state(lr=99.0).cuda() if adam else None
    hist = torch.zeros(3, dtype=torch.float64, device="cuda")  # one short of the replays: the last is dropped
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")
    tab = ops.SgdSchedTable([dict(w=w, slab=slab)])
    # load the code object before the capture
    ww = w0.clone().cuda()
    sw = ops.lr_state("constant", lr0=0.0).cuda()
    ops.lr_advance(sw)
    ops.sgd_sched_fp(ops.SgdSchedTable([dict(w=ww, slab=slab)]), sw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.lr_advance(sd, ad, hist, cur)
            ops.sgd_sched_fp(tab, sd)
    host = ops.lr_state("step", lr0=1.0, gamma=0.5, period=1)
    ref = w0.clone()
    for e in range(4):
        before = w.cpu().clone()
        graph.replay()
        torch.cuda.synchronize()
        ops.lr_advance(host)
        rate = 0.5 ** e
        assert ops.read_lr_state(sd) == ops.read_lr_state(host) and ops.read_lr_state(host)["lr"] == rate
        ref = ref + rate * G[0]
        assert torch.equal(w.cpu(), ref), e                # exact: integers times a power of two
        assert torch.equal(w.cpu() - before, rate * G[0])  # this replay's own rate, not the captured one
        if adam:
            assert ops.read_adam_state(ad)["lr"] == rate
    assert hist.cpu().tolist() == [1.0, 0.5, 0.25] and int(cur[0]) == 3  # a full history drops the record


@pytest.mark.gpu
def test_plateau_launch_equals_the_host_form(gpu):
    for case in K.PLATEAU_CASES:
        cfg, losses = case["cfg"], case["losses"]
        sd, sh = ops.lr_state(**cfg).cuda(), ops.lr_state(**cfg)
        vh = torch.zeros(len(losses), 2, dtype=torch.float64)
        vh[:, 0] = torch.tensor(losses, dtype=torch.float64)
        vhd = vh.cuda()
        cur = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.lr_plateau(vhd, cur, sd)  # an empty history: a no-op
        assert torch.equal(U.ibits(sd.cpu()), U.ibits(sh))
        for e in range(len(losses)):
            cur.fill_(e + 1)
            ops.lr_advance(sd), ops.lr_advance(sh)
            ops.lr_plateau(vhd, cur, sd)
            ops.lr_plateau(vh, torch.tensor([e + 1], dtype=torch.int32), sh)
            assert torch.equal(U.ibits(sd.cpu()), U.ibits(sh)), (case["name"], e)
        t = K.trace(cfg, losses)
        r = ops.read_lr_state(sd)
        assert K.same([(r["lr"], r["scale"], r["best"], r["stale"], r["cuts"], r["valid"])], t[-1:])


# ------------------------------------------------------------------ 4. the whole plan, exact
@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["t", False], ids=["mode-t", "mode-0"])
@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
def test_scheduled_plan_steps_exact(gpu, fused, momentum):
    """three one-step epochs under step with gamma 0.5 on the integer-exact fixture (784-128-64-10,
    batch 256): every rate is a power of two, so each epoch's step equals the FP64 reference with
    torch.equal.  A stepped weight leaves the fixture's lattice (pre-activations 0 or >= 32), so
    every epoch starts again from the fixture's weights with a zero momentum: what differs from
    epoch to epoch is the rate alone, and the three results must differ accordingly."""
    fx = fc.make_mlp3("LNN", 800, 256, 10, u8=True, seed=fc.SEED, n_in=784)
    n_valid = 128
    ref = fc.reference(fx, n_valid)
    m = MLP([784, 128, 64, 10], "LNN", batch=256, momentum=momentum, fused=fused,
            lr_schedule=dict(kind="step", lr=fc.STEP_LR, gamma=0.5, period=1))
    assert m.fused_mode == (fused or None) and m.plan.sched and not m.plan.g0_fused
    Xg = m.prepare_input(fx.X[:, :784].to(torch.uint8), pixel_scale=1.0)
    seen = []
    for e in range(3):
        for l, W in enumerate((fx.W0, fx.W1, fx.W2)):
            m.W32[l].copy_(W.float())
            if momentum:
                m.V32[l].zero_()
        m.refresh_bf16()
        m.advance_schedule()
        m.train_step(Xg, labels=fx.labels.cuda(), n_valid=n_valid, lr=77.0, alpha=fc.STEP_ALPHA)  # lr: ignored
        torch.cuda.synchronize()
        rate = fc.STEP_LR * 0.5 ** e
        assert ops.read_lr_state(m.lr_state)["lr"] == rate
        new = fc.reference_step(fx, ref, n_valid, rate, fc.STEP_ALPHA, momentum)
        for l, (W32, V32, Wb) in enumerate(new):
            assert torch.equal(m.W32[l].cpu(), W32), (e, l)
            if momentum:
                assert torch.equal(m.V32[l].cpu(), V32), (e, l)
            assert torch.equal(m.Wb[l].cpu(), Wb) and torch.equal(m.Wt[l].cpu(), Wb.t()), (e, l)
        if m.W0f is not None:  # mode t keeps the fragment-major copy of W0
            assert torch.equal(m.W0f.cpu().view(-1), ops.frag_major(new[0][2]).reshape(-1)), e
        seen.append(m.W32[0].cpu().clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert m.plan.sched_launches == 6 and m.plan.side_launches == 0  # per epoch the advance and ONE update


# ------------------------------------------------------------------ 5. f64 / f32 engines against the CPU oracle
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lrs"))
    return (d,) + tuple(K.make_data(d))


ENGINE_CASES = [("BPM", dict(kind="step", gamma=0.5, period=2)), ("BP", dict(kind="step", gamma=0.5, period=2)),
                ("ADAM", dict(kind="linear", span=6, lr_end=0.001, warmup=2))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tr,sched", ENGINE_CASES, ids=[f"{t}-{s['kind']}" for t, s in ENGINE_CASES])
def test_engine_matches_the_oracle(gpu, data, tr, sched, dtype):
    d, X, T = data[:3]
    K.write_conf(d, train=tr, dtype=dtype, epochs=6)
    cpu = K.train(d, "cpu", lr_schedule=sched)
    got = K.train(d, "gpu", lr_schedule=sched)
    assert cpu["ok"] and got["ok"]
    assert [K.bits(x) for x in got["lr"]] == [K.bits(x) for x in cpu["lr"]] and len(set(cpu["lr"])) >= 3
    tdt = torch.float64 if dtype == "f64" else torch.float32
    tol = 100.0 * A.order_spread(cpu["w0"], X, T, "SNN", K.NET["B"], dtype=tdt, epochs=6)
    err = A.spread(got["w"], cpu["w"])
    print(f"{tr} {sched['kind']} {dtype}: order spread {tol / 100:.3g}, engine - oracle {err:.3g}")
    assert tol > 0.0 and err <= tol
    assert A.spread(cpu["w"], cpu["w0"]) > 1e-3
    # the captured replays, the eager launches and a second run: the same bits
    eager = K.train(d, "gpu", env={"HPNN_GRAPH": "0"}, lr_schedule=sched)
    assert eager["raw"] == got["raw"] and K.train(d, "gpu", lr_schedule=sched)["raw"] == got["raw"]


# ------------------------------------------------------------------ 6. the BF16 engine
@pytest.mark.gpu
@pytest.mark.parametrize("net,dims,B,pixels,mode,tr", [
    ("SNN", (784, [128, 64], 10), 256, True, "t", "BPM"),
    ("SNN", (4096, [230], 230), 256, False, "w", "BP"),
    ("ANN", (100, [64, 48], 7), 128, False, None, "BPM"),
])
def test_train_nn_bf16_equals_python_plan(tmp_path, gpu, net, dims, B, pixels, mode, tr):
    """three scheduled epochs of one minibatch each (step, gamma 0.5, period 1, warmup 2)"""
    n_in, hid, n_out = dims
    n, seed, lr = B - 7, 11, 0.05
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (n, n_in)).astype(np.float64) if pixels else rng.uniform(-1, 1, (n, n_in))
    lab = rng.integers(0, n_out, n)
    T = np.full((n, n_out), 0.0 if net == "SNN" else -1.0)
    T[np.arange(n), lab] = 1.0
    d = str(tmp_path)
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    formats.write_conf(os.path.join(d, "nn.conf"), name="t", type=net, seed=seed, inputs=n_in, hiddens=hid,
                       outputs=n_out, train=tr, sample_dir="./train.hpnb", test_dir="./train.hpnb",
                       mode="batched", batch=B, epochs=3, dtype="bf16", lr=lr, momentum=0.25, lr_gamma=0.5, lr_period=1,
                       warmup=2)
    env = dict(os.environ)
    env.pop("HPNN_FORCE_CPU", None)
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-vvv", "-L", "step", "nn.conf"], cwd=d, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"batched plan: mode {mode or '-'}" in r.stdout, r.stdout[-3000:]
    rates = [float(ln.split("lr=")[1]) for ln in r.stdout.splitlines() if "LR: epoch" in ln]
    assert rates == [lr * 0.5, lr * 0.5, lr * 0.25]  # warmup 1/2, 2/2 on lr, lr/2; then lr/4
    got = formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"]
    m = MLP([n_in] + hid + [n_out], net, batch=B, seed=seed, momentum=tr == "BPM",
            lr_schedule=dict(kind="step", lr=lr, gamma=0.5, period=1, warmup=2))
    assert m.fused_mode == mode
    o = A.order(n, seed)
    xb = torch.tensor(X[o])
    Xp = m.prepare_input(xb.to(torch.uint8) if pixels else xb, pixel_scale=1.0)
    Tt = torch.zeros(m.Bp, n_out, device="cuda")
    Tt[:n] = torch.tensor(T[o], dtype=torch.float32, device="cuda")
    for _ in range(3):
        m.advance_schedule()
        m.train_step(Xp, T=Tt, n_valid=n, alpha=0.25)
    torch.cuda.synchronize()
    for a, w in zip(got, m.W32):
        ref = w[:a.shape[0], :a.shape[1]].double().cpu().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), ref), np.abs(a - ref).max()
        assert not w[a.shape[0]:].any() and not w[:, a.shape[1]:].any()


def _bpm_distance(lr_schedule, g0_fused, B=256, lr=0.01):
    """3 BPM steps of 784-128-64-10 at a constant rate: the relative Frobenius distance of the
    weight change per layer to the FP64 reference on the same BF16-rounded inputs"""
    from hpnn_amd.models import reference
    torch.manual_seed(0)
    m = MLP([784, 128, 64, 10], "SNN", batch=B, momentum=True, seed=7, lr_schedule=lr_schedule)
    if not g0_fused:
        m.plan.g0_fused = False
    W64 = [w.clone() for w in m.host_weights()]
    W0 = [w.clone() for w in W64]
    V64 = [torch.zeros_like(w) for w in W64]
    X = torch.rand(B, 784, dtype=torch.float64)
    labels = torch.randint(0, 10, (B,))
    T = torch.zeros(B, 10, dtype=torch.float64)
    T[torch.arange(B), labels] = 1.0
    Xb = X.float().bfloat16().double()
    Xd = m.prepare_input(X)
    Tf = torch.zeros(m.Bp, 10, device="cuda")
    Tf[:B] = T.float().cuda()
    for _ in range(3):
        if lr_schedule:
            m.advance_schedule()
        m.train_step(Xd, T=Tf, n_valid=B, lr=lr, alpha=0.2)
        reference.batched_step(W64, Xb, T, "SNN", lr, momentum=V64, alpha=0.2)
    torch.cuda.synchronize()
    got = m.host_weights()
    return [float(((got[l] - W0[l]) - (W64[l] - W0[l])).norm() / (W64[l] - W0[l]).norm()) for l in range(m.L)]


@pytest.mark.gpu
def test_scheduled_plan_is_as_close_to_fp64_as_the_unfused_plan(gpu):
    """the scheduled plan's distance to the FP64 reference is at most 2 x that of the unscheduled,
    unfused plan at the same constant rate"""
    plain = _bpm_distance(None, g0_fused=False)
    sched = _bpm_distance(dict(kind="constant", lr=0.01), g0_fused=True)
    for l, (s, p) in enumerate(zip(sched, plain)):
        print(f"layer {l}: distance to FP64, scheduled {s:.3g}, unscheduled unfused {p:.3g}")
    for s, p in zip(sched, plain):
        assert s <= 2.0 * p, (s, p)


# ------------------------------------------------------------------ 7. resume and keep-best
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plateau_resume_through_the_state_file_is_exact(gpu, data, dtype):
    d = data[0]
    sched = dict(kind="plateau", gamma=0.5, patience=1)
    kw = dict(train="BPM", dtype=dtype, validate=1, lr=8.0)
    K.write_conf(d, epochs=4, **kw)
    whole = K.train(d, "gpu", lr_schedule=sched)
    K.write_conf(d, epochs=2, **kw)
    h1 = K.train(d, "gpu", dump="two.bin", lr_schedule=sched)
    rest = K.train(d, "gpu", load="two.bin", lr_schedule=sched)
    assert whole["ok"] and rest["ok"] and rest["epochs_done"] == 4
    print(f"{dtype}: rates {whole['lr']}, state {whole['state']['sched']}")
    assert h1["state"]["sched"]["cuts"] >= 1, "the fixture is at fault: no cut before the split"
    assert [K.bits(x) for x in h1["lr"] + rest["lr"]] == [K.bits(x) for x in whole["lr"]]
    assert rest["raw"] == whole["raw"] and whole["state"]["has_sched"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_keep_best_with_plateau_equals_the_best_epochs_run(gpu, data, dtype):
    d = data[0]
    sched = dict(kind="plateau", gamma=0.5, patience=1)
    kw = dict(train="BPM", dtype=dtype, validate=1, lr=2.0)
    K.write_conf(d, epochs=10, **kw)
    kept = K.train(d, "gpu", lr_schedule=sched, keep_best="loss", patience=3)
    assert kept["ok"]
    b = kept["best"]["epoch"]
    print(f"{dtype}: best epoch {b}, rates {kept['lr']}")
    assert 1 < b < 10 and kept["epochs_done"] == b and len(kept["lr"]) == len(kept["val"]) == b + 3
    assert min(kept["lr"]) < 2.0, "the fixture is at fault: no cut in the whole run"
    K.write_conf(d, epochs=b, **kw)
    plain = K.train(d, "gpu", lr_schedule=sched)
    assert plain["raw"] == kept["raw"]


@pytest.mark.gpu
@pytest.mark.parametrize("env,msg", [
    ({"HPNN_LOOPBACK_RANKS": "2"}, "[lr_schedule] is not supported by data-parallel batched training; use one GPU"),
    ({"HPNN_PARALLEL": "tp"}, "[lr_schedule] is not supported by tensor-parallel batched training; use one GPU"),
])
def test_engine_refusals(gpu, data, capfd, env, msg):
    d = data[0]
    K.write_conf(d, train="BPM", dtype="f32", epochs=2)
    r = K.train(d, "gpu", env=env, dump=None, lr_schedule=dict(kind="step"))
    out = capfd.readouterr()
    assert not r["ok"] and (out.err + out.out).count(msg) == 1
    assert all(np.array_equal(a, b) for a, b in zip(r["w"], r["w0"]))


# ------------------------------------------------------------------ 8. an unscheduled plan is untouched
@pytest.mark.gpu
def test_an_unscheduled_bpm_plan_launches_no_schedule_kernel(gpu):
    torch.manual_seed(0)
    B = 256
    X = torch.rand(B, 784)
    lab = torch.randint(0, 10, (B,), dtype=torch.int32, device="cuda")
    m = MLP([784, 128, 64, 10], "SNN", batch=B, momentum=True, seed=3)
    assert not m.sched and m.lr_state is None and not m.plan.sched
    assert m.plan.g0_fused and m.plan.tn_update and m.plan.tn8_side  # the fused steps stay on
    assert not any(name == "lrs" for name, *_ in m.plan.buffers())
    Xd = m.prepare_input(X)
    for _ in range(2):
        m.train_step(Xd, labels=lab, lr=0.01, alpha=0.2)
    torch.cuda.synchronize()
    assert m.plan.sched_launches == 0
    with pytest.raises(RuntimeError):
        m.advance_schedule()
    # the two-layer net: layer 1's step still rides in layer 0's fused launch
    # (the shape and batch of tests/test_wide_gpu.py's side-job test)
    B = 16384
    w = MLP([4096, 230, 230], "SNN", batch=B, momentum=True, seed=3)
    Xw = w.prepare_input(torch.rand(B, 4096, device="cuda"))
    labw = torch.randint(0, 230, (B,), dtype=torch.int32, device="cuda")
    s = MLP([4096, 230, 230], "SNN", batch=B, momentum=True, seed=3, lr_schedule=dict(kind="constant", lr=0.01))
    for _ in range(3):
        w.train_step(Xw, labels=labw, lr=0.01, alpha=0.2)
        s.advance_schedule()
        s.train_step(Xw, labels=labw, alpha=0.2)
    torch.cuda.synchronize()
    assert w.plan.sched_launches == 0 and s.plan.sched_launches == 6 and s.plan.side_launches == 0
    print(f"unscheduled two-layer plan: side_launches {w.plan.side_launches}")
    assert w.plan.side_launches == 3  # this shape takes the side job on every step (tests/test_wide_gpu.py)
