"""[train] ADAM on the GPU: the kernels of csrc/gpu/kernels_adam.hip against the rounding bounds of
tests/adam_common.py (derived there) and bit for bit against the host form, the state read at run
time inside a captured graph, the f64 / f32 engines against the FP64 CPU oracle, the BF16 plan
against the FP64 reference and, bit for bit, against train_nn, exact resume, [keep_best], the
refusals, and BP / BPM untouched.

Every case prints what it measured."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP, reference
from hpnn_amd.utils import formats
from tests import adam_common as A
from tests import upd_common as U

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
BIG = 1_048_576 + 3  # the smallest n that enters the grid-stride loop (4096 x 256 elements per pass)


def _segment(n, S, off, dtype, seed):
    """one CPU segment: w, m, v windows `off` elements into NaN-padded buffers, slabs [S, n] with
    rows n + 3 apart (NaN between); elements 0..4 have g = m = v = 0, 5..8 a g whose square
    overflows the type (n permitting)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    m = (0.1 * torch.randn(n, generator=g, dtype=torch.float64)).to(dtype)
    v = (0.01 * torch.rand(n, generator=g, dtype=torch.float64)).to(dtype)
    scale = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 6.0 - 4.0)
    sl = (scale * torch.randn(S, n, generator=g, dtype=torch.float64)).to(dtype)
    sl[:, :5] = 0.0
    m[:5] = 0.0
    v[:5] = 0.0
    if n > 9:
        sl[0, 5:9] = 1e30 if dtype == torch.float32 else 1e200
        sl[1:, 5:9] = 0.0
    seg, bases = {}, {}
    bases["slab"], seg["slab"] = U.slab_window(sl, off)
    for k, t in (("w", w), ("m", m), ("v", v)):
        bases[k], seg[k] = U.window(t, off)
    return seg, bases


def _run_fp(sizes, S, off, dtype, t, decay, seed):
    """the kernel on `sizes` segments in one launch; checks bounds, padding, repeatability and that
    every bit equals the host form's; returns the worst error / bound ratios and that equality"""
    cpu = [_segment(n, S, off, dtype, seed + i) for i, n in enumerate(sizes)]
    st = ops.adam_state(lr=0.01, decay=decay)
    for _ in range(t):
        ops.adam_advance(st)
    sd = ops.read_adam_state(st)
    assert sd["t"] == t
    runs = []
    for _ in range(2):
        dev = [U.to_cuda(seg, bases) for seg, bases in cpu]
        ops.adam_update_fp(ops.AdamTable([d for d, _ in dev]), st.cuda(), 1.0 / 7)
        torch.cuda.synchronize()
        runs.append(dev)
    worst, same_as_host = [0.0, 0.0, 0.0], True
    for (seg, bases), (d1, b1), (d2, b2) in zip(cpu, runs[0], runs[1]):
        for k in ("w", "m", "v", "slab"):
            assert torch.equal(U.ibits(b1[k].cpu()), U.ibits(b2[k].cpu())), "two runs differ"
            # everything outside the windows (NaN padding, the gaps between slabs) is untouched
            mask = torch.ones_like(bases[k], dtype=torch.bool)
            mask.as_strided(seg[k].shape, seg[k].stride(), seg[k].storage_offset()).fill_(False)
            assert torch.equal(U.ibits(b1[k].cpu())[mask], U.ibits(bases[k])[mask]), f"{k}: padding written"
        assert torch.equal(U.ibits(d1["slab"].cpu()), U.ibits(seg["slab"])), "the slabs are read only"
        w1, m1, v1 = d1["w"].cpu(), d1["m"].cpu(), d1["v"].cpu()
        r = A.check_update(seg["w"], seg["m"], seg["v"], seg["slab"], 1.0 / 7, sd, w1, m1, v1, dtype,
                           f"n {seg['w'].numel()} S {S} off {off} t {t}")
        worst = [max(a, b) for a, b in zip(worst, r)]
        if decay == 0.0:  # g = 0, m = v = 0: not a bit changes
            assert torch.equal(U.ibits(w1[:5]), U.ibits(seg["w"][:5])) and not m1[:5].any() and not v1[:5].any()
            if seg["w"].numel() > 9:  # g^2 overflows: v = inf, the step is 0
                assert torch.isinf(v1[5:9]).all() and torch.equal(U.ibits(w1[5:9]), U.ibits(seg["w"][5:9]))
        hw, hm, hv = seg["w"].clone(), seg["m"].clone(), seg["v"].clone()
        ops.adam_update_fp(ops.AdamTable([dict(w=hw, m=hm, v=hv, slab=seg["slab"])]), st, 1.0 / 7)
        same = all(torch.equal(U.ibits(a), U.ibits(b)) for a, b in ((hw, w1), (hm, m1), (hv, v1)))
        assert same, f"n {seg['w'].numel()} S {S} off {off} t {t} {dtype}: the bits differ from the host form's"
        same_as_host &= same
    return worst, same_as_host


# ------------------------------------------------------------------ 1. hpnn_adam_fp
@pytest.mark.gpu
@pytest.mark.parametrize("decay", [0.0, 0.01])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_adam_fp_kernel_within_the_bounds(gpu, dtype, decay):
    worst, host = [0.0, 0.0, 0.0], True
    cases = [([n], S, off, t) for n in (1, 3, 255, 257) for S in (1, 3) for off in (0, 1) for t in (1, 1000)]
    cases += [([255, 3], 3, 1, 1), ([257, 1, 255], 1, 0, 1000), ([3, 257, 255], 3, 1, 1000)]
    for i, (sizes, S, off, t) in enumerate(cases):
        r, h = _run_fp(sizes, S, off, dtype, t, decay, 100 + i)
        worst = [max(a, b) for a, b in zip(worst, r)]
        host &= h
    print(f"adam_fp {dtype} decay {decay}: worst error / bound of m, v, w = {['%.3g' % x for x in worst]}; "
          f"bits equal to the host form: {host}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_adam_fp_kernel_grid_stride_loop(gpu, dtype):
    for S, off in ((1, 1), (3, 0)):
        r, h = _run_fp([BIG], S, off, dtype, 1000, 0.01, 7)
        print(f"adam_fp {dtype} n {BIG} S {S} off {off}: error / bound {['%.3g' % x for x in r]}; host bits {h}")
    r, h = _run_fp([BIG, 257], 1, 0, dtype, 1, 0.0, 9)
    print(f"adam_fp {dtype} n {BIG} + 257: error / bound {['%.3g' % x for x in r]}; host bits {h}")


@pytest.mark.gpu
def test_adam_table_refusals(gpu):
    w = torch.zeros(16, device="cuda")
    ok = dict(w=w, m=w.clone(), v=w.clone(), slab=torch.zeros(2, 16, device="cuda"))
    ops.AdamTable([ok])
    with pytest.raises(ValueError):
        ops.AdamTable([ok] * 17)
    with pytest.raises(ValueError):  # overlapping slabs
        ops.AdamTable([dict(ok, slab=torch.zeros(40, device="cuda").as_strided((2, 16), (8, 1)))])
    nat = ops.native()
    tb = torch.zeros(1, 8, dtype=torch.int64, device="cuda")
    row = (w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), 1, 16, 16)
    s = torch.cuda.current_stream().cuda_stream
    assert nat.adam_table(0, tb.data_ptr(), [row], s) == 0
    assert nat.adam_table(0, tb.data_ptr(), [(0,) + row[1:]], s) == -1        # a null pointer
    assert nat.adam_table(1, tb.data_ptr(), [(w.data_ptr() + 4,) + row[1:]], s) == -1  # a misaligned double
    assert nat.adam_table(0, tb.data_ptr(), [row[:6] + (0,)], s) == -1        # n = 0
    assert nat.adam_fp(0, tb.data_ptr(), 0, 1.0, tb.data_ptr(), s) == -1 and nat.adam_advance(0, s) == -1


# ------------------------------------------------------------------ 2. hpnn_adam_update_multi
LAYERS = {"32x32": (32, 32, False), "64x96": (64, 96, False), "128x800": (128, 800, True)}


def _multi_layer(N, K, S, frag, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    M = 0.1 * torch.randn(N, K, generator=g)
    V = 0.01 * torch.rand(N, K, generator=g)
    scale = 10.0 ** (torch.rand(N, K, generator=g, dtype=torch.float64) * 6.0 - 4.0)
    G = (scale * torch.randn(S, N, K, generator=g, dtype=torch.float64)).float()
    G[:, -3:, :] = 0.0  # rows that behave like the plan's zero padding
    W[-3:], M[-3:], V[-3:] = 0.0, 0.0, 0.0
    return dict(W=W, M=M, V=V, G=G, frag=frag)


def _run_multi(names, S, seed):
    st = ops.adam_state(lr=0.01, decay=0.01)
    for _ in range(3):
        ops.adam_advance(st)
    sd = ops.read_adam_state(st)
    cpu = [_multi_layer(*LAYERS[n][:2], S, LAYERS[n][2], seed + i) for i, n in enumerate(names)]
    outs = []
    for _ in range(2):
        dev = [U.multi_dev(c, ("M", "V")) for c in cpu]
        ops.adam_update_multi(dev, st.cuda(), 1.0 / 5)
        torch.cuda.synchronize()
        outs.append(dev)
    worst = [0.0, 0.0, 0.0]
    for c, a, b in zip(cpu, outs[0], outs[1]):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16
                                                                   else torch.int32), y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))
        W1, M1, V1, G1, Wb, Wt, Wf = [None if t is None else t.cpu() for t in a]
        n = c["W"].numel()
        r = A.check_update(c["W"].view(-1), c["M"].view(-1), c["V"].view(-1), c["G"].view(S, n), 1.0 / 5, sd,
                           W1.view(-1), M1.view(-1), V1.view(-1), torch.float32, f"{tuple(c['W'].shape)} S {S}")
        worst = [max(p, q) for p, q in zip(worst, r)]
        assert torch.equal(G1, c["G"])
        assert torch.equal(Wb, W1.bfloat16()) and torch.equal(Wt, Wb.t())
        if c["frag"]:
            assert torch.equal(Wf, ops.frag_major(Wb))  # the layout of hpnn_sgd_update_multi's Wf
        assert not W1[-3:].any() and not M1[-3:].any() and not V1[-3:].any()  # g = 0 rows stay exactly 0
        # the documented summation order, through the host form: the same bits
        hw, hm, hv = c["W"].clone(), c["M"].clone(), c["V"].clone()
        ops.adam_update_multi([(hw, hm, hv, c["G"], torch.empty_like(Wb), torch.empty_like(Wt), None)], st, 1.0 / 5)
        c["host"] = torch.equal(hw, W1) and torch.equal(hm, M1) and torch.equal(hv, V1)
        assert c["host"], f"{tuple(c['W'].shape)} S {S}: the bits differ from the host form's in the kernel's order"
    return worst, all(c["host"] for c in cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 24])
@pytest.mark.parametrize("names", [["32x32"], ["64x96"], ["128x800"], ["32x32", "64x96", "128x800"]],
                         ids=["32x32", "64x96", "128x800", "all"])
def test_adam_update_multi_within_the_bounds(gpu, names, S):
    worst, host = _run_multi(names, S, 40 + S)
    print(f"adam_update_multi {names} S {S}: worst error / bound of m, v, w = {['%.3g' % x for x in worst]}; "
          f"bits equal to the host form in the kernel's order: {host}")


# ------------------------------------------------------------------ 3. the state is read when the launch runs
@pytest.mark.gpu
def test_a_captured_step_reads_its_state_when_it_runs(gpu):
    seg, bases = _segment(257, 3, 1, torch.float32, 5)
    dev, _ = U.to_cuda(seg, bases)
    eag, _ = U.to_cuda(seg, bases)
    td, te = ops.AdamTable([dev]), ops.AdamTable([eag])
    sd = ops.adam_state(lr=0.01).cuda()
    se = ops.adam_state(lr=0.01).cuda()
    warm, _ = U.to_cuda(seg, bases)
    sw = ops.adam_state(lr=0.01).cuda()
    ops.adam_advance(sw)  # loads the code object before the capture
    ops.adam_update_fp(ops.AdamTable([warm]), sw, 0.5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.adam_advance(sd)
            ops.adam_update_fp(td, sd, 0.5)
    host = ops.adam_state(lr=0.01)
    for _ in range(5):
        graph.replay()
        ops.adam_advance(se)
        ops.adam_update_fp(te, se, 0.5)
        ops.adam_advance(host)
    torch.cuda.synchronize()
    got = ops.read_adam_state(sd)
    assert got == ops.read_adam_state(host) and got["t"] == 5  # p1, p2, c1, s2 equal as floats: the same bits
    for k in ("w", "m", "v"):
        assert torch.equal(U.ibits(dev[k].cpu()), U.ibits(eag[k].cpu())), k
    # a new lr in the device state: the next replay must use it
    for s in (sd, se):
        ops.write_adam_state(s, lr=0.5)
    before = dev["w"].cpu().clone()
    graph.replay()
    ops.adam_advance(se)
    ops.adam_update_fp(te, se, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(U.ibits(dev["w"].cpu()), U.ibits(eag["w"].cpu()))
    moved = (dev["w"].cpu() - before).abs()[9:]
    assert float(moved.max()) > 0.05, "the replay did not read the new lr"  # steps of about lr = 0.5, not 0.01


# ------------------------------------------------------------------ 4. f64 / f32 engines against the CPU oracle
def _bits(ws):
    return [w.tobytes() for w in ws]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("net,net_type", A.CASES)
def test_engine_matches_the_oracle(gpu, tmp_path, capfd, net, net_type, dtype):
    d = str(tmp_path)
    X, T, _, _ = A.make_data(d, net, net_type)
    A.write_conf(d, net, net_type, dtype=dtype, validate=1)
    B = A.NETS[net]["B"]
    cpu = A.train(d, "cpu")
    capfd.readouterr()
    got = A.train(d, "gpu", verbose=2)
    out = capfd.readouterr().out
    assert cpu["ok"] and got["ok"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    tol = 100.0 * A.order_spread(cpu["w0"], X, T, net_type, B, dtype=tdt)
    err = A.spread(got["w"], cpu["w"])
    print(f"{net} {net_type} {dtype}: order spread {tol / 100:.3g}, engine - oracle {err:.3g}")
    assert tol > 0.0 and err <= tol
    assert got["state"]["t"] == cpu["state"]["t"] and got["state"]["p1"] == cpu["state"]["p1"]
    assert A.spread(got["state"]["dW"], cpu["state"]["dW"]) <= tol and A.spread(got["state"]["V"], cpu["state"]["V"]) <= tol
    # the epoch losses: the held-out loss after every epoch, summed in FP64 by both engines
    rel = 1e-9 if dtype == "f64" else 1e-3
    assert len(got["val"]) == len(cpu["val"]) == A.EPOCHS
    for v, o_ in zip(got["val"], cpu["val"]):
        assert v["epoch"] == o_["epoch"] and v["loss"] == pytest.approx(o_["loss"], rel=rel), (v, o_)
    # the training loss of the last epoch as train_nn prints it: the output kernels add it up in
    # FP32 (n <= 100 additions of positive terms: n 2^-24 < 1e-5 relative), whatever the dtype
    loss = [float(ln.split("loss=")[1].split()[0]) for ln in out.splitlines() if "BATCHED TRAINING" in ln]
    assert len(loss) == 1
    W = [torch.tensor(w) for w in cpu["w0"]]
    o = np.array(A.order(X.shape[0]))
    Xo, To = torch.tensor(X[o]), torch.tensor(T[o])
    M_, V_ = [torch.zeros_like(w) for w in W], [torch.zeros_like(w) for w in W]
    st = reference.adam_new_state(lr=A.LR)
    for e in range(A.EPOCHS):
        tot = 0.0
        for s in range(0, Xo.shape[0], B):
            tot += float(reference.batched_step(W, Xo[s:s + B], To[s:s + B], net_type, 0.0, adam=(M_, V_, st))) * \
                min(B, Xo.shape[0] - s)
    assert loss[0] == pytest.approx(tot / X.shape[0], rel=max(rel, 1e-5))
    # the captured replays, the eager launches and a second run: the same bits
    eager = A.train(d, "gpu", env={"HPNN_GRAPH": "0"})
    again = A.train(d, "gpu")
    assert A.state_bits(eager["state"]) == A.state_bits(got["state"]) == A.state_bits(again["state"])


# ------------------------------------------------------------------ 5. the BF16 engine
BF16_NETS = [("SNN", [784, 128, 64, 10], "t"), ("ANN", [64, 96, 32], None), ("LNN", [40, 64, 8], None)]


def _weight_change_error(device, net_type, sizes, B, data_seed, lr=0.001):
    """the relative Frobenius error of the weight change per layer after 3 Adam steps against the
    FP64 reference on the same BF16-rounded inputs and initial weights"""
    torch.manual_seed(data_seed)
    m = MLP(sizes, net_type, batch=B, device=device, optimizer="adam", lr=lr, seed=7)
    W64 = [w.clone() for w in m.host_weights()]
    W0 = [w.clone() for w in W64]
    M_, V_ = [torch.zeros_like(w) for w in W64], [torch.zeros_like(w) for w in W64]
    st = reference.adam_new_state(lr=lr)
    X = torch.rand(B, sizes[0], dtype=torch.float64)
    labels = torch.randint(0, sizes[-1], (B,))
    T = torch.full((B, sizes[-1]), 0.0 if net_type == "SNN" else -1.0, dtype=torch.float64)
    T[torch.arange(B), labels] = 1.0
    Xb = X.float().bfloat16().double()
    Xd = m.prepare_input(X)
    Tf = torch.zeros(m.Bp, sizes[-1], device=m.device)
    Tf[:B] = T.float().to(m.device)
    for _ in range(3):
        m.train_step(Xd, T=Tf, n_valid=B, lr=99.0, alpha=99.0)  # ignored under Adam
        reference.batched_step(W64, Xb, T, net_type, 0.0, adam=(M_, V_, st))
    if m.device.type == "cuda":
        torch.cuda.synchronize()
    got = m.host_weights()
    err = [float(((got[l] - W0[l]) - (W64[l] - W0[l])).norm() / (W64[l] - W0[l]).norm()) for l in range(m.L)]
    return err, m


@pytest.mark.gpu
@pytest.mark.parametrize("net_type,sizes,mode", BF16_NETS, ids=[f"{t}-{'-'.join(map(str, s))}" for t, s, _ in BF16_NETS])
def test_bf16_plan_matches_the_fp64_reference(gpu, net_type, sizes, mode):
    """3 Adam steps at B = 256 against the FP64 reference; the bound of each layer is twice the
    same statistic of the CPU emulation (same rounding points, no code under test).

    Adam divides by sqrt(v): after the first steps every element moves by about lr sign(g), so
    this statistic counts the elements whose gradient sign the BF16 noise flips.  Over three data
    seeds the emulation's value is NOT stable within 20 % on the CPU -- per layer it varies by
    4.6 % .. 1000 % at B = 256 (784-128-64-10: 0.026-0.027, 0.025-0.032, 0.004-0.046; 64-96-32:
    0.009-0.026, 0.0009-0.0014; 40-64-8: 0.0005-0.002, 0.003-0.043) and no better at B = 1024,
    4096 or 16384 (one flipped element of a 40 x 64 layer is 0.013 by itself), so raising B does
    not help and B stays 256.  For ONE data seed the GPU and the emulation flip the same elements:
    measured on an MI355X at data seed 0, GPU / emulation per layer: 784-128-64-10 0.0272 / 0.0273,
    0.0254 / 0.0254, 0.0461 / 0.0461; 64-96-32 0.0221 / 0.0221, 0.00111 / 0.00111; 40-64-8 0.00211 /
    0.00211, 0.0432 / 0.0432 (profiles/adam/README.md)."""
    B = 256
    emu, _ = _weight_change_error("cpu", net_type, sizes, B, 0)
    got, m = _weight_change_error("cuda", net_type, sizes, B, 0)
    assert m.fused_mode == mode and m.plan.adam_launches == 6
    for l, (g_, e_) in enumerate(zip(got, emu)):
        print(f"{net_type} {sizes} layer {l}: relative error of the weight change, GPU {g_:.3g}, emulation {e_:.3g}")
    for l in range(m.L):
        N, K = sizes[l + 1], sizes[l]
        for t in (m.W32[l], m.V32[l], m.A32[l]):
            assert not t[N:].any() and not t[:, K:].any(), "the zero padding must stay zero"
        assert torch.equal(m.Wb[l], m.W32[l].bfloat16()) and torch.equal(m.Wt[l], m.Wb[l].t())
    assert ops.read_adam_state(m.adam_state)["t"] == 3
    for l, (g_, e_) in enumerate(zip(got, emu)):
        assert g_ <= 2.0 * e_, (l, g_, e_)


@pytest.mark.gpu
@pytest.mark.parametrize("net,dims,B,pixels,mode", [
    ("SNN", (784, [128, 64], 10), 256, True, "t"),
    ("SNN", (784, [128, 64], 10), 384, True, "x"),
    ("SNN", (4096, [230], 230), 256, False, "w"),
    ("ANN", (100, [64, 48], 7), 128, False, None),
])
def test_train_nn_adam_equals_python_plan(tmp_path, gpu, net, dims, B, pixels, mode):
    """the shapes of tests/test_bplan_gpu.py; three steps, the last minibatch half full"""
    n_in, hid, n_out = dims
    n, seed = 2 * B + B // 2, 11
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (n, n_in)).astype(np.float64) if pixels else rng.uniform(-1, 1, (n, n_in))
    lab = rng.integers(0, n_out, n)
    T = np.full((n, n_out), 0.0 if net == "SNN" else -1.0)
    T[np.arange(n), lab] = 1.0
    d = str(tmp_path)
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    formats.write_conf(os.path.join(d, "nn.conf"), name="t", type=net, seed=seed, inputs=n_in, hiddens=hid,
                       outputs=n_out, train="ADAM", sample_dir="./train.hpnb", test_dir="./train.hpnb",
                       mode="batched", batch=B, epochs=1, dtype="bf16", lr=0.002, decay=0.01)
    env = dict(os.environ)
    env.pop("HPNN_FORCE_CPU", None)
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-vvv", "nn.conf"], cwd=d, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"batched plan: mode {mode or '-'}" in r.stdout, r.stdout[-3000:]
    got = formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"]
    m = MLP([n_in] + hid + [n_out], net, batch=B, seed=seed, optimizer="adam", lr=0.002, decay=0.01)
    assert m.fused_mode == mode
    o = A.order(n, seed)
    Xo, To = X[o], T[o]
    for s in range(3):
        rows = min(B, n - s * B)
        xb = torch.tensor(Xo[s * B:s * B + rows])
        xb = xb.to(torch.uint8) if pixels else xb
        Xp = m.prepare_input(xb, pixel_scale=1.0)
        Tt = torch.zeros(m.Bp, n_out, device="cuda")
        Tt[:rows] = torch.tensor(To[s * B:s * B + rows], dtype=torch.float32, device="cuda")
        m.train_step(Xp, T=Tt, n_valid=rows)
    torch.cuda.synchronize()
    for a, w in zip(got, m.W32):
        ref = w[:a.shape[0], :a.shape[1]].double().cpu().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), ref), np.abs(a - ref).max()
        assert not w[a.shape[0]:].any() and not w[:, a.shape[1]:].any()


# ------------------------------------------------------------------ 6. exact resume
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resume_through_the_state_file_is_exact(gpu, tmp_path, dtype):
    d = str(tmp_path)
    A.make_data(d, "20-16-12-5", "SNN")
    kw = dict(dtype=dtype, decay=0.01, batch=32)
    A.write_conf(d, "20-16-12-5", "SNN", epochs=5, **kw)
    whole = A.train(d, "gpu")
    A.write_conf(d, "20-16-12-5", "SNN", epochs=2, **kw)
    A.train(d, "gpu", dump="two.bin")
    A.write_conf(d, "20-16-12-5", "SNN", epochs=3, **kw)
    rest = A.train(d, "gpu", load="two.bin")
    assert whole["ok"] and rest["ok"] and rest["epochs_done"] == 5
    assert whole["state"]["t"] == 15 and A.spread(whole["w"], whole["w0"]) > 0.01
    assert A.state_bits(rest["state"]) == A.state_bits(whole["state"])


# ------------------------------------------------------------------ 7. keep-best
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_keep_best_returns_the_state_of_the_best_epoch(gpu, tmp_path, dtype):
    d = str(tmp_path)
    A.make_data(d, A.KEEP["net"], A.KEEP["net_type"])
    A.write_keep_conf(d)
    b = A.check_keep_fixture(A.train(d, "cpu"))
    A.write_keep_conf(d, dtype=dtype)
    cpu = A.train(d, "cpu")
    kept = A.train(d, "gpu", dump="kept.bin")
    assert kept["ok"]
    if dtype == "f32":  # the same decisions as the FP64 oracle
        assert kept["best"]["epoch"] == b and kept["epochs_done"] == b
        assert [v["correct"] for v in kept["val"]] == [v["correct"] for v in cpu["val"]]
    kb = kept["best"]["epoch"]
    assert 1 < kb < A.KEEP["epochs"] and kept["epochs_done"] == kb
    A.write_keep_conf(d, dtype=dtype, epochs=kb, validate=None, keep_best=None, patience=None)
    plain = A.train(d, "gpu", dump="plain.bin")
    assert A.state_bits(kept["state"]) == A.state_bits(plain["state"])
    A.write_keep_conf(d, dtype=dtype, epochs=2, validate=None, keep_best=None, patience=None)
    a = A.train(d, "gpu", load="kept.bin")
    c = A.train(d, "gpu", load="plain.bin")
    assert a["epochs_done"] == kb + 2 and A.state_bits(a["state"]) == A.state_bits(c["state"])
    assert A.state_bits(a["state"]) != A.state_bits(kept["state"])


# ------------------------------------------------------------------ 8. refusals
@pytest.mark.gpu
@pytest.mark.parametrize("env,msg", [
    ({"HPNN_LOOPBACK_RANKS": "2"}, "[train] ADAM is not supported by data-parallel batched training"),
    ({"HPNN_PARALLEL": "tp"}, "[train] ADAM is not supported by tensor-parallel batched training"),
])
def test_engine_refusals(gpu, tmp_path, capfd, env, msg):
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "SNN")
    A.write_conf(d, "8-6-4", "SNN", dtype="f32")
    r = A.train(d, "gpu", env=env, dump=None)
    out = capfd.readouterr()
    assert not r["ok"] and msg in out.err + out.out
    assert all(np.array_equal(a, b) for a, b in zip(r["w"], r["w0"]))


# ------------------------------------------------------------------ 9. BP / BPM untouched
@pytest.mark.gpu
@pytest.mark.parametrize("sizes,net_type", [([784, 128, 64, 10], "SNN"), ([100, 64, 48, 7], "ANN")])
def test_a_bpm_plan_launches_no_adam_kernel(gpu, sizes, net_type):
    torch.manual_seed(0)
    B = 256
    X = torch.rand(B, sizes[0])
    lab = torch.randint(0, sizes[-1], (B,), dtype=torch.int32, device="cuda")
    m = MLP(sizes, net_type, batch=B, momentum=True, seed=3)
    assert not m.adam and m.A32[0] is None and m.adam_state is None and not m.plan.adam
    assert not any(name in ("A32", "adam") for name, *_ in m.plan.buffers())
    Xd = m.prepare_input(X)
    for _ in range(2):
        m.train_step(Xd, labels=lab, lr=0.01, alpha=0.2)
    torch.cuda.synchronize()
    assert m.plan.adam_launches == 0
    a = MLP(sizes, net_type, batch=B, seed=3, optimizer="adam")
    for _ in range(2):
        a.train_step(a.prepare_input(X), labels=lab)
    torch.cuda.synchronize()
    assert a.plan.adam_launches == 4  # per step the advance and ONE update over all layers
