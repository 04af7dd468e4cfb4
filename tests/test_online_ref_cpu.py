"""The reference of the online-kernel unit tests (tests/online_common.py) on the CPU: it agrees
with the existing oracles, every fixture meets the preconditions the GPU tests rely on, every
mutant of the rule is told apart by a named fixture, and the host-side grid helpers of
csrc/gpu/online.hip give the documented values."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from hpnn_amd.models import reference as ref
from hpnn_amd.utils import formats
from tests import online_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


# ----------------------------------------------------------------------------- existing oracles
@pytest.mark.parametrize("net,mom", [("ANN", True), ("ANN", False), ("SNN", False), ("SNN", True), ("LNN", True)])
def test_matches_online_step_loop(net, mom):
    """the numpy rule == a loop over hpnn_amd.models.reference.online_step with the stop rule of
    tests/test_capi_cpu.py, from a non-zero dW, to the rounding of two different summations"""
    c = oc.make_case("o", [23, 11, 7, 5], net, mom, 5, lr=0.01, delta=1e-3, min_iter=4, max_iter=60)
    r = oc.run_case(c)
    W = [torch.tensor(w) for w in c.W]
    V = [torch.tensor(v) for v in c.dW] if mom else None
    x, t = torch.tensor(c.x), torch.tensor(c.t)
    it = 0
    while True:
        it += 1
        dEp, o = ref.online_step(W, x, t, net, c.lr, V, c.alpha)
        ok = int(torch.argmax(o)) == int(torch.nonzero(t == 1.0)[-1])
        if it == 1:
            first = ok
        if it > c.max_iter:
            break
        ok = ok and it > c.min_iter
        if dEp <= c.delta and ok:
            break
    assert (r.iters, r.ok, r.first_ok) == (it, int(ok), int(first))
    assert 4 < it <= c.max_iter + 1
    for l in range(3):
        assert np.abs(r.W[l] - W[l].numpy()).max() < 1e-13
        if mom:
            assert np.abs(r.dW[l] - V[l].numpy()).max() < 1e-13
    assert abs(float(r.dEp) - float(dEp)) < 1e-13 and np.abs(r.out - o.numpy()).max() < 1e-13


def test_matches_train_nn_cpu_engine(tmp_path):
    """train_nn on the CPU engine (online mode, two samples): the weights of kernel.opt and the
    logged iteration counts, first / final verdicts equal a replay through the reference"""
    d = str(tmp_path)
    rng = np.random.default_rng(1)
    os.makedirs(os.path.join(d, "samples"))
    for i in range(2):
        x = rng.uniform(-1, 1, 4)
        t = np.full(4, -1.0)
        t[int(np.argmax(x))] = 1.0
        formats.write_sample(os.path.join(d, "samples", f"s{i:04d}.txt"), x, t)
    formats.write_conf(os.path.join(d, "nn.conf"), name="t", type="ANN", seed=10958, inputs=4, hiddens=[8], outputs=4,
                       train="BPM", sample_dir="./samples", test_dir="./samples")
    env = dict(os.environ, HPNN_FORCE_CPU="1")
    p = subprocess.run([os.path.join(BIN, "train_nn"), "-vv", "nn.conf"], cwd=d, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    order = [ln.split("TRAINING FILE:")[1].split()[0] for ln in p.stdout.splitlines() if "TRAINING FILE" in ln]
    logged = re.findall(r"(OK|NO) N_ITER=\s*(\d+) final=\s*\S+ (SUCCESS|FAIL)", p.stdout)
    assert len(order) == 2 and len(logged) == 2, p.stdout
    W = [np.array(w) for w in formats.read_kernel(os.path.join(d, "kernel.tmp"))["weights"]]
    for f, (first, n_iter, verdict) in zip(order, logged):
        x, t = formats.read_sample(os.path.join(d, "samples", f))
        r = oc.run(W, [np.zeros_like(w) for w in W], x, t, "ANN", True, 0.0005, 0.2, **oc.DEFAULTS[True])
        assert (r.iters, r.first_ok, r.ok) == (int(n_iter), int(first == "OK"), int(verdict == "SUCCESS"))
        W = r.W
    k1 = formats.read_kernel(os.path.join(d, "kernel.opt"))
    for a, b in zip(k1["weights"], W):
        assert np.abs(a - b).max() < 1e-9


def test_orders_differ_only_by_rounding():
    a = np.random.default_rng(0).uniform(-1, 1, (5, 1025))
    v = np.random.default_rng(1).uniform(-1, 1, 1025)
    exact = (a.astype(np.longdouble) * v.astype(np.longdouble)).sum(1)
    outs = [oc._dot(a, v, o) for o in oc.ORDERS[:3]]
    for o in outs:
        assert np.abs(o - exact).max() < 1e-13
    assert any(not np.array_equal(outs[0], o) for o in outs[1:])
    assert np.finfo(np.longdouble).eps < 2e-19  # the 80-bit format the tolerance reasoning assumes


# ----------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("name", oc.case_names())
def test_tolerance_is_far_below_the_update(name):
    """16 x spread + 4 ulp of every weight tensor is below 1e-6 of the largest weight update"""
    assert oc.check_precondition(name) < 1e-6
    nat = oc.reference(name)[0]
    assert nat.iters == 3  # min_iter = max_iter = 2: three iterations whatever the data


@pytest.mark.parametrize("name", list(oc.CONVERGE))
def test_convergence_fixture_is_decided_by_a_margin(name):
    oc.check_converge_precondition(name)
    oc.check_precondition(name)
    nat = oc.reference(name)[0]
    assert 100 < nat.iters < 10000 and nat.ok == 1


@pytest.mark.parametrize("name", oc.exact_names())
def test_exact_fixture_is_exact(name):
    """exact_reference asserts: pre-activations 0 or >= 64, every sum below 2^52 quanta, the four
    orders bit-equal, deltas on a fair share of rows"""
    c, r = oc.exact_reference(name)
    assert r.iters == 1
    if c.momentum:  # every element moves: W += dW0 with dW0 dense
        assert float(np.mean(r.W[0] != c.W[0])) > 0.8


def test_float64_activation_is_exact_where_the_fixtures_need_it():
    assert float(oc.act(np.float64(0.0))) == 0.0
    assert float(oc.act(np.float64(64.0))) == 1.0 and float(oc.act(np.float64(-64.0))) == -1.0
    with np.errstate(over="ignore"):
        assert float(oc.act(np.float64(-37.0))) != -1.0  # why the fixtures use 64


@pytest.mark.parametrize("key", list(oc.stop_cases()))
def test_stop_fixture_gives_the_expected_words(key):
    c, exp = oc.stop_cases()[key]
    for o in oc.ORDERS[:3]:
        r = oc.run_case(c, o)
        assert dict(iters=r.iters, ok=r.ok, first_ok=r.first_ok) == exp
        assert float(r.dEp) == 0.0
    if c.net == "SNN":
        r = oc.run_case(c)
        assert r.out[1] == 0.0 and r.out[3] == 0.0 and c.t[1] == 1.0 and float(r.init_err) > 0


# ----------------------------------------------------------------------------- mutants
def _differs(name, **kw):
    """the mutant leaves the tolerance of at least one compared quantity of the named case"""
    nat, tol, _, _, _ = oc.reference(name)
    m = oc.run_case(oc.case(name), **kw)
    if (m.iters, m.ok, m.first_ok) != (nat.iters, nat.ok, nat.first_ok):
        return True
    ref, got = oc.compared(nat), oc.compared(m)
    return any(float(np.abs(got[k] - ref[k]).max()) > tol[k] for k in ref)


def _words(r):
    return (r.iters, r.ok, r.first_ok)


def _stop_differs(key, mutant):
    c, _ = oc.stop_cases()[key]
    a, b = oc.run_case(c), oc.run_case(c, mutant=mutant)
    return _words(a) != _words(b) or float(a.init_err) != float(b.init_err)


def _exact_differs(name, mutant, grid=0):
    c, r = oc.exact_reference(name)
    m = oc.run_case(c, mutant=mutant, grid=grid)
    return any(not np.array_equal(a, b) for a, b in zip(r.W + r.dW, m.W + m.dW))


MUTANT_FIXTURES = {
    # exact fixtures: BPM only (under BP an update touches only columns whose f' is 0)
    "deltas_after_update": lambda: _differs("A-ANN-BPM", mutant="deltas_after_update") and _differs(
        "c-SNN-BP", mutant="deltas_after_update") and _exact_differs("A-ANN-BPM", "deltas_after_update"),
    "momentum_scaled_first": lambda: _differs("a63-ANN-BPM", mutant="momentum_scaled_first") and _exact_differs(
        "c-ANN-BPM", "momentum_scaled_first"),
    "first_target": lambda: _stop_differs("5-two-ones-last", "first_target") and _stop_differs(
        "5-two-ones-hit", "first_target"),
    "last_max": lambda: _stop_differs("4-tie-second", "last_max") and _stop_differs("4-tie-first", "last_max"),
    "min_ge": lambda: _stop_differs("1-correct", "min_ge"),
    "max_ge": lambda: _stop_differs("2-wrong", "max_ge"),
    "snn_no_guard": lambda: _stop_differs("9-snn-underflow", "snn_no_guard"),
    "skip_col_1024": lambda: (_differs("b1025-ANN-BPM", mutant="skip_col_1024")
                              and _differs("b1025-SNN-BP", mutant="skip_col_1024")
                              and _differs("c-SNN-BP", mutant="skip_col_1024")
                              and _exact_differs("b1025-ANN-BPM", "skip_col_1024")
                              and _exact_differs("c-LNN-BP", "skip_col_1024")),
    "drop_partial": lambda: all(_differs("A-SNN-BP", mutant="drop_partial", grid=g) for g in (3, 50, 128))
    and _exact_differs("A-ANN-BPM", "drop_partial", grid=65),
}


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_mutant_is_told_apart(mutant):
    assert MUTANT_FIXTURES[mutant](), mutant


def test_true_rule_is_not_told_apart_from_itself():
    assert not _differs("A-ANN-BPM") and not _differs("A-ANN-BPM", order="strided")
    assert not _exact_differs("A-ANN-BPM", None)


# ----------------------------------------------------------------------------- grid helpers
def _native():
    from hpnn_amd._lib import native
    return native()


def test_coop_grid_thresholds():
    n = _native()
    assert n.online_coop_grid([10, 28, 5]) == 0 and n.online_coop_grid([10, 29, 5]) == 8
    assert n.online_coop_grid([10, 32, 5]) == 8 and n.online_coop_grid([10, 33, 5]) == 9
    assert n.online_coop_grid([10, 511, 5]) == 128 and n.online_coop_grid([10, 512, 5]) == 128
    assert n.online_coop_grid([10, 4000, 5]) == 128
    # the vectors (x, t, three per row) above 150 KB: 19200 doubles
    assert n.online_coop_grid([19000, 40, 4]) == 10
    assert (19064 + 4 + 3 * 44) * 8 == 150 * 1024 and n.online_coop_grid([19064, 40, 4]) == 10
    assert n.online_coop_grid([19065, 40, 4]) == 0
    assert n.online_coop_grid([4] * 18) == 0  # 17 layers
    for s in oc.COOP_SHAPES.values():
        assert n.online_coop_grid(s) >= (8 if max(s[1:]) >= 29 else 0)
    assert n.online_coop_grid(oc.COOP_SHAPES["A"]) == 50 and n.online_coop_grid(oc.SINGLE_SHAPES["c"]) == 0


def test_coop_grid_env_switch():
    """HPNN_ONLINE_COOP=0 is read once per process"""
    code = "from hpnn_amd._lib import native; print(native().online_coop_grid([10, 300, 5]))"
    for val, want in (("0", "0"), ("1", "75")):
        env = dict(os.environ, HPNN_ONLINE_COOP=val, PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == want, p.stdout + p.stderr


def test_coop_grid_slots_respects_its_cap():
    n = _native()
    s = [10, 4000, 5]
    assert n.online_coop_grid_slots(s, 1, 16) == n.online_coop_grid(s) == 128
    assert n.online_coop_grid_slots(s, 2, 16) == 16 and n.online_coop_grid_slots(s, 2, 64) == 64
    assert n.online_coop_grid_slots(s, 2, 500) == 128
    assert n.online_coop_grid_slots([10, 40, 5], 2, 64) == 5 and n.online_coop_grid_slots([10, 3, 2], 4, 64) == 1


def test_vec_and_xch_bytes():
    n = _native()
    A = oc.COOP_SHAPES["A"]  # 70-48-200-33-7
    assert n.online_vec_bytes(A) == (70 + 3 * (48 + 200 + 33 + 7)) * 8
    # two generations of every layer's outputs, then [G][M_l] delta partials of layers 1..L-1
    for G in (1, 3, 50, 128):
        assert n.online_coop_xch_bytes(A, G) == (2 * (48 + 200 + 33 + 7) + G * (48 + 200 + 33)) * 8
    assert n.online_vec_bytes(oc.SINGLE_SHAPES["h"]) == 49888 and n.online_vec_bytes(oc.SINGLE_SHAPES["i"]) == 152288
    assert n.online_vec_bytes(oc.SINGLE_SHAPES["j"]) > 150 * 1024
    assert n.online_coop_xch_bytes([130, 40], 10) == 2 * 40 * 8  # L = 1: no partials


def test_design_names_the_threshold_the_code_has():
    with open(os.path.join(ROOT, "docs", "DESIGN.md")) as f:
        text = f.read()
    assert "widest layer of >= 29 rows" in text and "layers of >= 32 rows" not in text
