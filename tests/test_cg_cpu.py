"""[train] CG on the CPU: the FP64 C oracle (csrc/cpu/cpu_cg.cpp) against the FP64 PyTorch
reference (hpnn_amd.models.reference.cg_iteration), the rule edges of include/libhpnn/cg.h through
hpnn_amd.ops on CPU tensors, and the conf / CLI surface (round trip, [validate] / [keep_best] /
[patience], -r, the refusals).

Tolerance of the weight comparison: 100 x the largest weight difference between two FP64
reference runs that differ only in the sample order (a legitimate summation order), measured in
the test.  Measured after ten iterations: 8-6-4 ANN 3.6e-15, SNN 3.0e-14; 20-16-12-5 ANN 4.9e-15,
SNN 1.6e-15 (largest |W| 2.3 to 5.2); the oracle is 4.4e-15 to 2.8e-14 from the reference."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import reference
from tests import cg_common as C

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin")
CG_RE = re.compile(r"CG: epoch (\d+) loss=(\S+) beta=(\S+) alpha=(\S+) trial=(-?\d+)( FAILED)?")


# ------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("net,net_type", C.CASES)
def test_oracle_matches_reference(tmp_path, net, net_type):
    d = str(tmp_path)
    X, T, _, _ = C.make_data(d, net, net_type)
    C.write_conf(d, net, net_type)
    B = C.NETS[net]["B"]
    r = C.train(d, "cpu")
    assert r["ok"] and len(r["hist"]) == C.ITERS and r["epochs_done"] == C.ITERS
    recs, w_ref = C.reference_run(r["w0"], X, T, net_type, B)
    C.check_gaps(recs, f"{net} {net_type}")
    tol = 100.0 * C.order_spread(r["w0"], X, T, net_type, B)
    err = C.spread(r["w"], w_ref)
    print(f"{net} {net_type}: order spread {tol / 100:.3g}, oracle - reference {err:.3g}, "
          f"max |W| {max(np.abs(w).max() for w in w_ref):.3g}, trials {[x['trial'] for x in recs]}")
    assert 0 < tol < 1e-9
    assert C.decisions(r["hist"]) == C.decisions(recs)
    assert err <= tol
    for h, x in zip(r["hist"], recs):
        for k in ("f0", "f1", "beta", "alpha"):
            assert h[k] == pytest.approx(x[k], rel=1e-9, abs=1e-12), (k, h, x)
    # the loss never rises: within an iteration, and from one epoch to the next
    f0 = [h["f0"] for h in r["hist"]]
    assert all(h["f1"] < h["f0"] for h in r["hist"])
    assert all(b <= a for a, b in zip(f0, f0[1:]))
    # the next iteration starts from the loss the last one settled on
    for a, b in zip(r["hist"], r["hist"][1:]):
        assert b["f0"] == pytest.approx(a["f1"], rel=1e-12)
    assert r["hist"][0]["flags"] & capi.CG_RESTART and r["hist"][0]["beta"] == 0.0
    assert any(h["beta"] > 0 for h in r["hist"][1:])


def test_oracle_failed_search_and_restart(tmp_path):
    """a fixture whose third iteration overshoots with every trial: W stays W0 bit for bit, a_init
    shrinks by 16 and the next iteration is steepest descent -- as the reference does"""
    net, net_type, ds = C.FAILING
    d = str(tmp_path)
    X, T, _, _ = C.make_data(d, net, net_type, ds)
    C.write_conf(d, net, net_type, epochs=3)
    r3 = C.train(d, "cpu")
    recs, w_ref = C.reference_run(r3["w0"], X, T, net_type, C.NETS[net]["B"], iters=4)
    assert recs[2]["flags"] & reference.CG_FAILED, "the fixture is at fault: no failed search"
    C.write_conf(d, net, net_type, epochs=2)
    r2 = C.train(d, "cpu")
    C.write_conf(d, net, net_type, epochs=4)
    r4 = C.train(d, "cpu")
    assert C.decisions(r4["hist"]) == C.decisions(recs)
    h = r3["hist"][2]
    assert h["flags"] & capi.CG_FAILED and h["alpha"] == 0.0 and h["f1"] == h["f0"]
    assert all(np.array_equal(a, b) for a, b in zip(r3["w"], r2["w"]))  # the failed iteration wrote W0 back
    h = r4["hist"][3]
    assert h["flags"] & capi.CG_RESTART and h["beta"] == 0.0 and not h["flags"] & capi.CG_FAILED
    assert h["f1"] < h["f0"]


# ------------------------------------------------------------------ rule edges through ops (CPU tensors)
@pytest.mark.parametrize("case", C.EDGES, ids=[c["name"] for c in C.EDGES])
def test_rule_edges(case):
    mid, end, hist = C.run_edge(case)
    e = case["expect"]
    m, s = ops.read_cg_state(mid), ops.read_cg_state(end)
    a0 = case["state"].get("a_init", 1.0)
    assert m["a"][:6] == [a0 * 2.0 ** (j - 2) for j in range(6)]
    assert m["beta"] == e["beta"] and m["jstar"] == e["jstar"]
    assert m["a"][6] == e["a7"]
    assert m["flags"] == e["flags"] & ~ops.CG_TOOK7
    assert s["flags"] == e["flags"] and s["a"][7] == e["alpha"]
    assert s["a_init"] == e["a_init"] and s["first"] == e["first"]
    assert s["gg_prev"] == case["state"].get("gg", 0.0)
    assert s["hits0"] == 7 and s["cursor"] == 1
    (r,) = ops.read_cg_history(hist, 1)
    assert r["flags"] == e["flags"] and r["alpha"] == e["alpha"] and r["beta"] == e["beta"]
    assert r["trial"] == (None if e["jstar"] == ops.CG_NONE else e["jstar"])
    f0 = case["f0"]
    assert r["f0"] == f0 or (f0 != f0 and r["f0"] != r["f0"])
    if e["flags"] & ops.CG_FAILED:
        assert r["f1"] == r["f0"] or f0 != f0
    else:
        assert r["f1"] == min(case["phi7"], float(case["phi"][e["jstar"]]))


def test_rule_restart_after_failure():
    """the iteration after a failed search: beta = 0 whatever the dot products say, and the steps
    start from a_init / 16"""
    case = next(c for c in C.EDGES if c["name"].startswith("failed search: no trial"))
    _, st, _ = C.run_edge(case)
    ops.write_cg_state(st, gg=3.0, gp=0.0, gd=5.0)
    ops.cg_direction(st)
    s = ops.read_cg_state(st)
    assert s["beta"] == 0.0 and s["flags"] == ops.CG_RESTART and s["gg_prev"] == 3.0
    assert s["a"][:6] == [2.0 ** (j - 2) / 16 for j in range(6)]


def test_history_capacity():
    """a full history drops the record, the decisions go on"""
    st, hist = ops.cg_state(1.0, 1, 1), ops.cg_history(1)
    for _ in range(2):
        ops.cg_direction(st)
        ops.cg_file(C.slots_with(10.0), st, hist, ops.CG_FINAL)
        for j in range(6):
            ops.cg_file(C.slots_with([9, 8, 7, 8, 9, 9][j]), st, hist, j)
        ops.cg_file(C.slots_with(6.0), st, hist, ops.CG_PARABOLA)
    assert ops.read_cg_state(st)["cursor"] == 1


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_elementwise_ops_cpu(dtype):
    g0 = torch.Generator().manual_seed(3)
    n = 37
    w0 = torch.randn(n, generator=g0, dtype=dtype)
    w0[0], w0[1] = -0.0, 0.0
    d = torch.randn(n, generator=g0, dtype=dtype)
    d[2], d[3] = float("inf"), float("nan")
    w, g, gp = torch.zeros(n, dtype=dtype), torch.randn(n, generator=g0, dtype=dtype), torch.zeros(n, dtype=dtype)
    slab = torch.randint(-8, 9, (3, n), generator=g0).to(dtype)
    tb = ops.CgTable([dict(w=w, w0=w0.clone(), g=g, gprev=gp, d=d.clone(), slab=slab)])
    st = ops.cg_state(1.0, 1, 1)
    ops.cg_direction(st)
    ops.write_cg_state(st, a=[0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 0.3, 0.0])
    # a = 0 returns W0 bit for bit: -0 stays -0, a d that is not finite does not leak
    ops.cg_trial(tb, st, 0)
    assert torch.equal(w.view(torch.int64 if dtype == torch.float64 else torch.int32),
                       w0.view(torch.int64 if dtype == torch.float64 else torch.int32))
    # a power of two is exact; any a is one fma
    ops.cg_trial(tb, st, 1)
    assert torch.equal(w[4:], w0[4:] + 0.5 * d[4:])
    ops.cg_trial(tb, st, 6)
    a = torch.tensor(0.3, dtype=dtype)
    exact = w0[4:].double() + a.double() * d[4:].double()
    assert torch.equal(w[4:], exact.to(dtype)) or dtype == torch.float64
    assert (w[4:].double() - exact).abs().max() <= C_U(dtype) * (w0[4:].abs() + (a * d[4:]).abs()).max()
    # accumulate: slab order, first, scale
    ops.cg_accumulate(tb, True, 1.0)
    assert torch.equal(g, slab.sum(0))
    ops.cg_accumulate(tb, False, 0.25)
    assert torch.equal(g, slab.sum(0) * 2 * 0.25)
    # dots on small integers are exact
    gp.copy_(torch.randint(-8, 9, (n,), generator=g0).to(dtype))
    tb.segs[0]["d"].copy_(torch.randint(-8, 9, (n,), generator=g0).to(dtype))
    ops.cg_dots(tb, st)
    s = ops.read_cg_state(st)
    assert (s["gg"], s["gp"], s["gd"]) == (float((g * g).sum()), float((g * gp).sum()),
                                           float((g * tb.segs[0]["d"]).sum()))
    # begin: d = fma(beta, d, g); beta = 0 copies g
    ops.write_cg_state(st, beta=0.0)
    ops.cg_begin(tb, st)
    assert torch.equal(tb.segs[0]["d"], g) and torch.equal(gp, g) and torch.equal(tb.segs[0]["w0"][4:], w[4:])
    ops.write_cg_state(st, beta=2.0)
    ops.cg_begin(tb, st)
    assert torch.equal(tb.segs[0]["d"], 3 * g)


def C_U(dtype):
    return 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24


# ------------------------------------------------------------------ conf and CLI
def _run(d, *flags, check=True):
    e = dict(os.environ, HPNN_KERNEL_EXACT="1")
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-c", "-vv", *flags, "nn.conf"], cwd=d, env=e,
                       capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_conf_round_trip(tmp_path):
    d = str(tmp_path)
    C.make_data(d, "8-6-4", "SNN")
    C.write_conf(d, "8-6-4", "SNN")
    capi.init(0)
    net = capi.Network(os.path.join(d, "nn.conf"))
    assert net.L.nn_return_train(net.ptr) == capi.NN_TRAIN["CG"]
    assert net.cg_history() == []
    net.dump_conf(os.path.join(d, "b.conf"))
    net.close()
    assert "[train] CG\n" in open(os.path.join(d, "b.conf")).read()
    net = capi.Network(os.path.join(d, "b.conf"))
    assert net.L.nn_return_train(net.ptr) == capi.NN_TRAIN["CG"]
    net.close()


def test_cli_log_metrics_and_samples(tmp_path):
    d = str(tmp_path)
    C.make_data(d, "8-6-4", "SNN")
    C.write_conf(d, "8-6-4", "SNN", epochs=3, shuffle="epoch")
    out = _run(d, "-M", "m.jsonl").stdout
    lines = CG_RE.findall(out)
    assert [int(x[0]) for x in lines] == [1, 2, 3] and float(lines[0][2]) == 0.0
    assert "CG sums over the whole set, no reshuffle" in out
    ev = [json.loads(x) for x in open(os.path.join(d, "m.jsonl"))]
    cg = [e for e in ev if e.get("event") == "cg" or e.get("type") == "cg" or "f0" in e]
    assert len(cg) == 3 and [e["epoch"] for e in cg] == [1, 2, 3]
    assert [e["trial"] for e in cg] == [int(x[4]) for x in lines]
    assert re.search(r"BATCHED TRAINING: 300 samples", out)  # n per iteration
    tb = [e for e in ev if "samples_per_s" in e]
    assert tb and tb[-1]["samples"] == 300 and tb[-1]["epochs_done"] == 3


def test_keep_best_patience_returns_best_epoch(tmp_path):
    """-V 1 -K loss -P 2: the weights returned are those after the best pass's iteration, bit for
    bit the kernel of a run of that many epochs"""
    d = str(tmp_path)
    C.make_data(d, "20-16-12-5", "SNN")
    C.write_conf(d, "20-16-12-5", "SNN", epochs=40)
    out = _run(d, "-V", "1", "-K", "loss", "-P", "2").stdout
    best = re.search(r"BEST: epoch (\d+)", out)
    stop = re.search(r"EARLY STOP: epoch (\d+)", out)
    assert best and stop, out[-2000:]
    b, s = int(best.group(1)), int(stop.group(1))
    assert 1 < b and s == b + 2 and s < 40, f"the fixture is at fault: best {b}, stop {s}"
    assert len(CG_RE.findall(out)) == s
    kept = open(os.path.join(d, "kernel.opt"), "rb").read()
    _run(d, "-e", str(b))
    assert open(os.path.join(d, "kernel.opt"), "rb").read() == kept


def test_resume_starts_with_steepest_descent(tmp_path):
    d = str(tmp_path)
    C.make_data(d, "8-6-4", "ANN")
    C.write_conf(d, "8-6-4", "ANN", epochs=3)
    first = CG_RE.findall(_run(d, "-r", "st.bin").stdout)
    second = CG_RE.findall(_run(d, "-e", "4", "-r", "st.bin").stdout)
    assert [int(x[0]) for x in first] == [1, 2, 3] and float(first[2][2]) > 0.0
    assert [int(x[0]) for x in second] == [4, 5, 6, 7]  # epochs_done continues
    assert float(second[0][2]) == 0.0 and any(float(x[2]) > 0.0 for x in second[1:])  # the direction does not
    assert float(second[0][1]) < float(first[2][1])  # the weights do


@pytest.mark.parametrize("extra,flags,msg", [
    (dict(mode="online"), (), r"\[train\] CG needs \[mode\] batched .*online mode trains with BP or BPM"),
    (dict(dtype="bf16"), (), r"\[train\] CG: the line search compares losses that the BF16 forward cannot resolve; "
                             r"use \[dtype\] f32 or f64"),
    (dict(), ("-d", "bf16"), r"use \[dtype\] f32 or f64"),
])
def test_refusals(tmp_path, extra, flags, msg):
    d = str(tmp_path)
    C.make_data(d, "8-6-4", "SNN")
    C.write_conf(d, "8-6-4", "SNN", **extra)
    r = _run(d, *flags, check=False)
    assert r.returncode != 0 and re.search(msg, r.stdout + r.stderr), r.stdout[-1500:] + r.stderr[-1500:]
    assert len(re.findall(r"NN\(ERR\)", r.stdout + r.stderr)) == 1  # one clear error


def test_splx_keeps_its_message(tmp_path):
    d = str(tmp_path)
    C.make_data(d, "8-6-4", "SNN")
    C.write_conf(d, "8-6-4", "SNN", train="SPLX")
    r = _run(d, check=False)
    assert r.returncode != 0 and "unimplemented training type!" in r.stdout + r.stderr
