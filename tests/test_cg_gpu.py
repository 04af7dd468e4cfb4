"""[train] CG on the GPU: the kernels of csrc/gpu/kernels_cg.hip at their edges, both dtypes
(segment sizes around the 16-byte vector and the 256-thread workgroup, tables of 1, 3 and 16
segments, unaligned tensors and gapped slabs), the decision kernels against the rule of
include/libhpnn/cg.h on the CPU bit for bit, and the f64 / f32 engines against the FP64 CPU
oracle (fixtures and preconditions: tests/cg_common.py).

Tolerances of the engine's weights: f64, 100 x the spread between two FP64 reference runs that
differ only in the sample order (as tests/test_cg_cpu.py); f32, 100 x the same spread of two FP32
PyTorch runs.  Each case prints what it measured.  On an MI355X, ten iterations: FP64 spread 2.4e-15
to 6.2e-15 with the f64 engine 4.0e-15 to 3.2e-14 from the oracle; FP32 spread 7.8e-7 to 3.3e-6
with the f32 engine 8.8e-7 to 3.0e-6 from the oracle; trial indices and flags identical in all
sixteen runs, and the captured, the eager and a repeated run equal bit for bit."""
import math

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from tests import cg_common as C
from tests import fp_ref

SIZES = [1, 3, 4, 5, 255, 256, 257, 4099]
TABLES = {1: [4099], 3: [5, 257, 4099], 16: SIZES + SIZES}
DTYPES = [torch.float64, torch.float32]
KEYS = ("w", "w0", "g", "gprev", "d")


def _ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _segments(sizes, dtype, seed, integers=False):
    """CPU segments: every tensor a window of its own buffer, odd segments one element off the
    16-byte grid; slabs [S, n] with S = 1 + i % 3 rows n + 3 elements apart, one element off too"""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        if integers:
            return torch.randint(-8, 9, shape, generator=g).to(dtype)
        return torch.randn(*shape, generator=g, dtype=dtype)

    segs = []
    for i, n in enumerate(sizes):
        off = i % 2
        s = {k: rnd(n + 4)[off:off + n] for k in KEYS}
        S = 1 + i % 3
        s["slab"] = rnd(S * (n + 3) + 1)[1:].view(S, n + 3)[:, :n]
        segs.append(s)
    return segs


def _to_cuda(segs):
    """the same windows on the device (the offsets inside the allocations are kept)"""
    out = []
    for s in segs:
        o = {}
        for k, t in s.items():
            base = torch.empty(t.untyped_storage().nbytes() // t.element_size(), dtype=t.dtype)
            base.set_(t.untyped_storage())
            o[k] = base.cuda().as_strided(t.shape, t.stride(), t.storage_offset())
        out.append(o)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n_segs", sorted(TABLES))
def test_accumulate_begin_trial_match_the_cpu_rule(gpu, dtype, n_segs):
    cpu = _segments(TABLES[n_segs], dtype, 7 + n_segs)
    dev = _to_cuda(cpu)
    tc, td = ops.CgTable(cpu), ops.CgTable(dev)
    st = ops.cg_state(1.0, 1, 1)
    ops.write_cg_state(st, beta=0.75, a=[0.0, 0.5, 1.0, 2.0, 0.3, -1.7, 1e-3, 0.0])
    sd = st.cuda()

    def same(keys):
        for a, b in zip(cpu, dev):
            for k in keys:
                assert torch.equal(_ibits(a[k]), _ibits(b[k].cpu())), k

    for first, scale in ((True, 1.0), (False, 1.0), (False, 1.0 / 100)):
        ops.cg_accumulate(tc, first, scale)
        ops.cg_accumulate(td, first, scale)
        same(("g",))
    # against plain PyTorch too: (S0 + S0 + S0) / 100 in slab order
    for s in cpu:
        acc = torch.zeros_like(s["g"])
        for _ in range(3):
            for r in range(s["slab"].shape[0]):
                acc = acc + s["slab"][r]
        assert torch.equal(s["g"], acc * torch.tensor(1.0 / 100, dtype=dtype))
    for beta in (0.75, 0.0):
        ops.write_cg_state(st, beta=beta)
        sd.copy_(st)
        ops.cg_begin(tc, st)
        ops.cg_begin(td, sd)
        same(("d", "gprev", "w0", "g", "w"))
    for j in range(8):
        ops.cg_trial(tc, st, j)
        ops.cg_trial(td, sd, j)
        same(("w", "w0", "d"))
    # a = 0 is a copy: -0 stays -0 and a d that is not finite does not leak into W
    for segs in (cpu, dev):
        for s in segs:
            s["w0"][0] = -0.0
            s["d"][0] = float("inf")
            s["d"][-1] = float("nan")
    for tb, state in ((tc, st), (td, sd)):
        ops.cg_trial(tb, state, 0)
    same(("w",))
    for s in cpu:
        assert torch.equal(_ibits(s["w"]), _ibits(s["w0"]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_trial_rounding(gpu, dtype):
    """W = W0 + a d within one unit roundoff of |W0| + |a d| (one fma), bitwise for a power of
    two, and W0 itself for a = 0"""
    u = fp_ref.U[dtype]
    cpu = _segments(TABLES[16], dtype, 3)
    dev = _to_cuda(cpu)
    td = ops.CgTable(dev)
    steps = [0.0, 0.5, 1.0, 2.0, 0.3, -1.7, 1e-3, 0.0078125]
    sd = ops.write_cg_state(ops.cg_state(1.0, 1, 1), a=steps).cuda()
    for j, a in enumerate(steps):
        ops.cg_trial(td, sd, j)
        at = torch.tensor(a, dtype=dtype)
        for s, sg in zip(cpu, dev):
            w = sg["w"].cpu()
            if a == 0.0:
                assert torch.equal(_ibits(w), _ibits(s["w0"]))
                continue
            if math.log2(abs(a)).is_integer():
                assert torch.equal(w, s["w0"] + at * s["d"])
            w0, d = s["w0"].numpy().astype(np.longdouble), s["d"].numpy().astype(np.longdouble)
            ad = np.longdouble(at.item()) * d
            err = np.abs(w.numpy().astype(np.longdouble) - (w0 + ad))
            assert (err <= u * (np.abs(w0) + np.abs(ad))).all(), (j, float(err.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n_segs", sorted(TABLES))
def test_dots(gpu, dtype, n_segs):
    # small integers: exact
    cpu = _segments(TABLES[n_segs], dtype, 11, integers=True)
    td = ops.CgTable(_to_cuda(cpu))
    sd = ops.cg_state(1.0, 1, 1).cuda()
    ops.cg_dots(td, sd)
    s = ops.read_cg_state(sd)
    want = [sum(int((x["g"].long() * x[k].long()).sum()) for x in cpu) for k in ("g", "gprev", "d")]
    assert [s["gg"], s["gp"], s["gd"]] == [float(v) for v in want]
    # random operands: within n u sum |x| |y| of the exact sum of the products, and the same bits twice
    cpu = _segments(TABLES[n_segs], dtype, 12)
    td = ops.CgTable(_to_cuda(cpu))
    ops.cg_dots(td, sd)
    first = sd.clone()
    part = torch.full((3 * 64,), float("nan"), dtype=torch.float64, device="cuda")
    ops.cg_dots(td, sd, part)
    assert torch.equal(_ibits(first[:3]), _ibits(sd[:3]))
    s = ops.read_cg_state(sd)
    n = sum(TABLES[n_segs])
    for got, k in ((s["gg"], "g"), (s["gp"], "gprev"), (s["gd"], "d")):
        prod = torch.cat([x["g"].double() * x[k].double() for x in cpu])
        ref = math.fsum(prod.tolist())
        bound = n * fp_ref.U[torch.float64] * float(prod.abs().sum())
        assert abs(got - ref) <= bound, (k, got, ref, bound)
    # the CPU form of the op: the same products in element order
    sc = ops.cg_state(1.0, 1, 1)
    ops.cg_dots(ops.CgTable(cpu), sc)
    c = ops.read_cg_state(sc)
    assert abs(c["gg"] - s["gg"]) <= n * fp_ref.U[torch.float64] * s["gg"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("net", [0, 1, 2], ids=["ANN", "LNN", "SNN"])
def test_loss_kernel(gpu, dtype, net):
    """cg_loss against the float64 output layer of tests/fp_ref.py: the hits exact, the loss added
    to what the slots held, the same bits twice, rows past n_valid not counted.  Bound of the loss
    sum: a row's loss goes through at most n_out + 8 roundings of relative size u (the softmax
    denominator's n_out terms, exp, the division, log or the squared difference, the row sum) on
    quantities no larger than max(1, loss of the row); a factor 8 covers the few-ulp exp / log of
    the device library and log's conditioning near an output of 1: 8 (n_out + 8) u sum_rows (1 +
    |loss|).  The FP64 additions of the rows and of the slot's earlier content are below that."""
    u = fp_ref.U[dtype]
    g = torch.Generator().manual_seed(17 + net)
    # (a one-output softmax is 1 whatever the logit: its loss is rounding alone, so SNN starts at 2)
    for B, n_out in ((1, 2 if net == 2 else 1), (5, 5), (257, 70), (1030, 5), (1030, 64)):
        z = (2.0 * torch.randn(B, n_out + 3, generator=g, dtype=torch.float64)).to(dtype)
        t = torch.full((B, n_out + 1), 0.0 if net == 2 else -1.0, dtype=dtype)
        t[torch.arange(B), torch.randint(0, n_out, (B,), generator=g)] = 1.0
        zd, td = z.cuda()[:, :n_out], t.cuda()[:, :n_out]
        for n_valid in sorted({0, max(B - 3, 0), B}):
            _, _, loss = fp_ref.output_ref(z[:, :n_out].double(), t[:, :n_out].double(), net, n_valid)
            o, _, _ = fp_ref.output_ref(z[:, :n_out].double(), t[:, :n_out].double(), net, B)
            hits = int((fp_ref.first_argmax(o) == fp_ref.first_argmax(t[:, :n_out].double()))[:n_valid].sum())
            slots = torch.zeros(64, 16, dtype=torch.float32, device="cuda")
            slots[3, 2:4].view(torch.float64)[0] = 1024.0  # what a chunk before this one left
            slots[3, 1:2].view(torch.int32)[0] = 5
            again = slots.clone()
            ops.cg_loss(zd, td, slots, net, n_valid)
            ops.cg_loss(zd, td, again, net, n_valid)
            assert torch.equal(slots.view(torch.int32), again.view(torch.int32))
            sl = slots.cpu()
            got = float(sl.view(torch.float64)[:, 1].sum()) - 1024.0
            assert int(sl[:, 1].contiguous().view(torch.int32).sum()) - 5 == hits, (B, n_out, n_valid)
            bound = 8.0 * (n_out + 8) * u * (n_valid + float(loss.abs().sum())) + 1024.0 * 2.0 ** -52
            assert abs(got - float(loss.sum())) <= bound, (B, n_out, n_valid, got, float(loss.sum()), bound)
            assert torch.count_nonzero(sl[:, 0]) == 0 and torch.count_nonzero(sl[:, 4:]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.EDGES, ids=[c["name"] for c in C.EDGES])
def test_decision_kernels_match_the_cpu_rule(gpu, case):
    """direction, file, choose and settle on the device against cg.h on the host, bit for bit"""
    want = C.run_edge(case, "cpu")
    got = C.run_edge(case, "cuda")
    for w, g_ in zip(want, got):
        assert torch.equal(w.view(torch.int64), g_.view(torch.int64))


@pytest.mark.gpu
def test_a_captured_trial_reads_its_step_when_it_runs(gpu):
    cpu = _segments([257], torch.float32, 5)
    dev = _to_cuda(cpu)
    td = ops.CgTable(dev)
    sd = ops.write_cg_state(ops.cg_state(1.0, 1, 4), a=[0.5] + [0.0] * 7).cuda()
    hist = ops.cg_history(4, "cuda")
    slots = torch.zeros(64, 16, dtype=torch.float32, device="cuda")
    ops.cg_trial(td, sd, 0)  # loads the code object before the capture
    ops.cg_file(slots, sd, hist, 0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.cg_trial(td, sd, 0)
            ops.cg_file(slots, sd, hist, 0)
    for a, loss in ((0.5, 3.0), (2.0, 5.0), (0.0, 7.0)):
        sd.copy_(ops.write_cg_state(sd.cpu(), a=[a] + [0.0] * 7))
        slots.copy_(C.slots_with(loss))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dev[0]["w"].cpu(), cpu[0]["w0"] + a * cpu[0]["d"] if a else cpu[0]["w0"])
        assert ops.read_cg_state(sd)["phi"][0] == loss and float(slots.abs().sum()) == 0.0


# ------------------------------------------------------------------ the engines against the oracle
def _bits(ws):
    return [w.tobytes() for w in ws]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("net,net_type", C.CASES)
def test_engine_matches_the_oracle(gpu, tmp_path, net, net_type, dtype):
    d = str(tmp_path)
    X, T, _, _ = C.make_data(d, net, net_type)
    C.write_conf(d, net, net_type, dtype=dtype)
    B = C.NETS[net]["B"]
    cpu = C.train(d, "cpu")
    got = C.train(d, "gpu")
    assert cpu["ok"] and got["ok"] and len(got["hist"]) == C.ITERS
    tdt = torch.float64 if dtype == "f64" else torch.float32
    recs, _ = C.reference_run(cpu["w0"], X, T, net_type, B, dtype=tdt)
    C.check_gaps(recs, f"{net} {net_type} {dtype}")
    tol = 100.0 * C.order_spread(cpu["w0"], X, T, net_type, B, dtype=tdt)
    err = C.spread(got["w"], cpu["w"])
    print(f"{net} {net_type} {dtype}: order spread {tol / 100:.3g}, engine - oracle {err:.3g}, "
          f"trials {[h['trial'] for h in got['hist']]}")
    assert C.decisions(got["hist"]) == C.decisions(cpu["hist"])
    assert err <= tol
    rel = 1e-9 if dtype == "f64" else 1e-3
    for h, o in zip(got["hist"], cpu["hist"]):
        for k in ("f0", "f1", "beta", "alpha"):
            assert h[k] == pytest.approx(o[k], rel=rel, abs=rel * 1e-3), (k, h, o)
    # the captured replays, the eager launches and a second run: the same bits
    eager = C.train(d, "gpu", env={"HPNN_GRAPH": "0"})
    again = C.train(d, "gpu")
    assert _bits(eager["w"]) == _bits(got["w"]) and eager["hist"] == got["hist"]
    assert _bits(again["w"]) == _bits(got["w"]) and again["hist"] == got["hist"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_engine_failed_search_and_restart(gpu, tmp_path, dtype):
    net, net_type, ds = C.FAILING
    d = str(tmp_path)
    C.make_data(d, net, net_type, ds)
    C.write_conf(d, net, net_type, dtype=dtype, epochs=2)
    two = C.train(d, "gpu")
    C.write_conf(d, net, net_type, dtype=dtype, epochs=3)
    three = C.train(d, "gpu")
    C.write_conf(d, net, net_type, dtype=dtype, epochs=4)
    cpu, four = C.train(d, "cpu"), C.train(d, "gpu")
    assert cpu["hist"][2]["flags"] & capi.CG_FAILED, "the fixture is at fault: no failed search"
    assert C.decisions(four["hist"]) == C.decisions(cpu["hist"])
    assert _bits(three["w"]) == _bits(two["w"])  # the failed iteration wrote W0 back, bit for bit
    assert three["hist"][2]["alpha"] == 0.0 and four["hist"][3]["beta"] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_engine_with_validate_keep_best_patience(gpu, tmp_path, dtype):
    net, net_type = "20-16-12-5", "SNN"
    d = str(tmp_path)
    X, T, _, _ = C.make_data(d, net, net_type)
    C.write_conf(d, net, net_type, dtype=dtype, epochs=40, validate=1, keep_best="loss", patience=2)
    cpu, got = C.train(d, "cpu"), C.train(d, "gpu")
    assert cpu["ok"] and got["ok"]
    b = cpu["best"]["epoch"]
    assert 1 < b and len(cpu["val"]) == b + 2 < 40, "the fixture is at fault: no early stop"
    assert got["best"]["epoch"] == b and got["epochs_done"] == cpu["epochs_done"] == b
    assert [v["epoch"] for v in got["val"]] == [v["epoch"] for v in cpu["val"]]
    assert [v["correct"] for v in got["val"]] == [v["correct"] for v in cpu["val"]]
    rel = 1e-9 if dtype == "f64" else 1e-3
    for v, o in zip(got["val"], cpu["val"]):
        assert v["loss"] == pytest.approx(o["loss"], rel=rel)
    assert len(got["hist"]) == len(cpu["hist"]) == b + 2
    assert C.decisions(got["hist"]) == C.decisions(cpu["hist"])
    tdt = torch.float64 if dtype == "f64" else torch.float32
    tol = 100.0 * C.order_spread(cpu["w0"], X, T, net_type, C.NETS[net]["B"], dtype=tdt, iters=b)
    err = C.spread(got["w"], cpu["w"])
    print(f"keep best {dtype}: best epoch {b}, order spread {tol / 100:.3g}, engine - oracle {err:.3g}")
    assert err <= tol
    # the kept weights are those of a run of b epochs
    C.write_conf(d, net, net_type, dtype=dtype, epochs=b)
    assert _bits(C.train(d, "gpu")["w"]) == _bits(got["w"])


@pytest.mark.gpu
@pytest.mark.parametrize("env,extra,msg", [
    ({"HPNN_LOOPBACK_RANKS": "2"}, {}, "[train] CG is not supported by data-parallel batched training"),
    ({"HPNN_PARALLEL": "tp"}, {}, "[train] CG is not supported by tensor-parallel batched training"),
    ({}, {"dtype": "bf16"}, "use [dtype] f32 or f64"),
])
def test_engine_refusals(gpu, tmp_path, capfd, env, extra, msg):
    d = str(tmp_path)
    C.make_data(d, "8-6-4", "SNN")
    C.write_conf(d, "8-6-4", "SNN", **extra)
    r = C.train(d, "gpu", env=env)
    out = capfd.readouterr()
    assert not r["ok"] and msg in out.err + out.out
    assert all(np.array_equal(a, b) for a, b in zip(r["w"], r["w0"]))
