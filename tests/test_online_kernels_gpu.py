"""The online FP64 kernels of csrc/gpu/online.hip, one launch at a time (ops.online_sample):
online_kernel<true> ("lds"), online_kernel<false> ("global") and online_coop_kernel<false>
("coop") against the numpy reference of tests/online_common.py.

Toleranced comparisons use the reference's own spread (16 x the largest deviation among its
summation orders and its long-double run, + 4 ulp); the first-iteration tests on integer data,
the stop-rule tests (lr = 0) and the determinism test are bit for bit.  Measured deviations:
profiles/online_unit/README.md."""
import numpy as np
import pytest
import torch

from hpnn_amd import ops
from tests import online_common as oc

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _grid(sizes, grid=None):
    """the grid the engine picks; 8 (the smallest it ever picks) where it would not go cooperative"""
    if grid is not None:
        return grid
    return ops.online_coop_grid(sizes) or 8


def _launch(c, variant, dev, grid=None, forward_only=False, check=True):
    W = [torch.tensor(w, dtype=F64, device=dev) for w in c.W]
    dW = [torch.tensor(v, dtype=F64, device=dev) for v in c.dW]
    x, t = torch.tensor(c.x, dtype=F64, device=dev), torch.tensor(c.t, dtype=F64, device=dev)
    res = ops.online_sample(W, dW, x, t, oc.TYPES[c.net], variant=variant, momentum=c.momentum, lr=c.lr,
                            alpha=c.alpha, delta=c.delta, min_iter=c.min_iter, max_iter=c.max_iter,
                            forward_only=forward_only, grid=_grid(c.sizes, grid) if variant == "coop" else None,
                            check=check)
    return W, dW, res


def _got(W, dW, res, forward_only=False):
    d = {"out": res[0].cpu().numpy(), "init_err": np.float64(res[2])}
    if not forward_only:
        d["dEp"] = np.float64(res[1])
        for l, (w, v) in enumerate(zip(W, dW)):
            d[f"W{l}"], d[f"dW{l}"] = w.cpu().numpy(), v.cpu().numpy()
    return d


def _compare(name, tag, W, dW, res, forward_only=False):
    """every compared quantity within the reference's tolerance, the integer words exact; prints
    (kernel deviation) / (reference spread) of the worst quantity"""
    nat, tol, spread, _, _ = oc.reference(name, forward_only)
    ref, got = oc.compared(nat, forward_only), _got(W, dW, res, forward_only)
    worst, bad = (0.0, ""), []
    for k, r in ref.items():
        dev = float(np.abs(got[k] - r).max())
        ratio = dev / spread[k] if spread[k] > 0 else (0.0 if dev == 0 else float("inf"))
        if np.isfinite(ratio) and ratio > worst[0]:
            worst = (ratio, k)
        if not dev <= tol[k]:
            bad.append((k, dev, tol[k], spread[k]))
    print(f"ONLINE_RATIO {name} {tag} worst {worst[0]:.3f} at {worst[1] or '-'}")
    assert not bad, (name, tag, bad)
    if not forward_only:
        assert res[3:] == (nat.iters, nat.ok, nat.first_ok), (name, tag, res[3:], (nat.iters, nat.ok, nat.first_ok))


def _unchanged(c, W, dW):
    return all(torch.equal(w.cpu(), torch.tensor(a, dtype=F64)) for w, a in zip(W, c.W)) and all(
        torch.equal(v.cpu(), torch.tensor(a, dtype=F64)) for v, a in zip(dW, c.dW))


# ----------------------------------------------------------------------------- three iterations
def _single_params():
    out = []
    for s in oc.SINGLE_SHAPES:
        for net, mom in oc.nets_of(s):
            for variant in ("lds", "global"):
                if (variant == "global" and s in oc.LDS_ONLY) or s == "j":
                    continue
                out.append((f"{s}-{net}-{'BPM' if mom else 'BP'}", variant))
    return out


@pytest.mark.parametrize("name,variant", _single_params())
def test_single_workgroup_matches_reference(gpu, name, variant):
    """three iterations (min_iter = max_iter = 2) of the single-workgroup kernel at the shapes of
    the case table: every weight, momentum, the output and the result words"""
    oc.check_precondition(name)
    c = oc.case(name)
    if name.startswith(("h-", "i-")):
        assert 48 * 1024 < ops.native().online_vec_bytes(c.sizes) <= 150 * 1024
    W, dW, res = _launch(c, variant, gpu)
    _compare(name, variant, W, dW, res)


@pytest.mark.parametrize("name", [n for n in oc.case_names() if n.startswith("j-")])
def test_lds_limit_refuses_and_global_runs(gpu, name):
    """19300-8-4 needs 154 688 B of vectors: the LDS form answers -2 and launches nothing, the
    global-scratch form runs"""
    c = oc.case(name)
    assert ops.native().online_vec_bytes(c.sizes) == 154688
    W, dW, rc = _launch(c, "lds", gpu, check=False)
    assert rc == -2 and _unchanged(c, W, dW)
    oc.check_precondition(name)
    W, dW, res = _launch(c, "global", gpu)
    _compare(name, "global", W, dW, res)


@pytest.mark.parametrize("variant", ("lds", "global", "coop"))
def test_seventeen_layers_are_refused(gpu, variant):
    c = oc.make_case("L17", [4] * 18, "ANN", False, 3)
    W, dW, rc = _launch(c, variant, gpu, grid=4, check=False)
    assert rc == -1 and _unchanged(c, W, dW)


def _coop_params():
    out = []
    for s, grids in oc.COOP_GRIDS.items():
        for net, mom in oc.nets_of(s):
            out += [(f"{s}-{net}-{'BPM' if mom else 'BP'}", g) for g in grids]
    return out


@pytest.mark.parametrize("name,grid", _coop_params())
def test_cooperative_matches_reference(gpu, name, grid):
    """the cooperative kernel at the engine's grid and at grids it never picks (1, one that divides
    nothing, more workgroups than rows)"""
    oc.check_precondition(name)
    c = oc.case(name)
    if grid is None:
        assert ops.online_coop_grid(c.sizes) >= 8, "the engine runs this net on the cooperative kernel"
    W, dW, res = _launch(c, "coop", gpu, grid=grid)
    _compare(name, f"coop{_grid(c.sizes, grid)}", W, dW, res)


@pytest.mark.parametrize("grid", [None, 128])
def test_cooperative_is_deterministic(gpu, grid):
    """the hidden deltas are summed in workgroup order: two launches from fresh copies agree bit
    for bit"""
    c = oc.case("A-ANN-BPM")
    a, b = _launch(c, "coop", gpu, grid=grid), _launch(c, "coop", gpu, grid=grid)
    for ta, tb in zip(a[0] + a[1] + [a[2][0]], b[0] + b[1] + [b[2][0]]):
        assert torch.equal(ta, tb)
    assert a[2][1:] == b[2][1:]


# ----------------------------------------------------------------------------- forward_only
FWD_NAMES = [n for n in oc.case_names() if n.split("-")[0] in ("b1023", "b1024", "b1025", "d", "g", "A")]


@pytest.mark.parametrize("variant", ("lds", "global", "coop"))
@pytest.mark.parametrize("name", FWD_NAMES)
def test_forward_only(gpu, name, variant):
    """run_nn's path: the output and result[1] within tolerance, W and dW bit-unchanged"""
    c = oc.case(name)
    W, dW, res = _launch(c, variant, gpu, forward_only=True)
    _compare(name, f"fwd-{variant}", W, dW, res, forward_only=True)
    assert _unchanged(c, W, dW)


# ----------------------------------------------------------------------------- bit-exact first iteration
def test_probe_device_activation(gpu):
    """2 / (1 + exp(-x)) - 1 in FP64 on the device: exactly 0 at 0 and exactly +-1 at +-64, what the
    bit-exact tests stand on (measured through a one-layer ANN forward)"""
    W = np.array([[0.0, 5.0], [64.0, 5.0], [-64.0, 5.0], [37.0, 5.0], [-37.0, 5.0]])
    c = oc.make_case("probe", [2, 5], "ANN", False, 0)
    c.W, c.dW, c.x = [W], [np.zeros_like(W)], np.array([1.0, 0.0])
    for variant in ("lds", "global", "coop"):
        _, _, res = _launch(c, variant, gpu, grid=2, forward_only=True)
        f = res[0].cpu().tolist()
        print("ONLINE_PROBE", variant, "f(0), f(64), f(-64), f(37), f(-37) =", [repr(v) for v in f])
        assert f[:3] == [0.0, 1.0, -1.0], (variant, f)


def _exact_params():
    out = []
    for name in oc.exact_names():
        shape = name.split("-")[0]
        out += [(name, "lds", None), (name, "global", None)]
        out += [(name, "coop", g) for g in (oc.COOP_GRIDS["A"] if shape == "A" else (None,))]
    return out


@pytest.mark.parametrize("name,variant,grid", _exact_params())
def test_first_iteration_bit_exact(gpu, name, variant, grid):
    """integer data on which every delta, product and sum of the first iteration is exact in any
    order: W and dW after one iteration equal the reference bit for bit -- no element skipped,
    written twice or updated with another row's coefficient"""
    c, r = oc.exact_reference(name)
    W, dW, res = _launch(c, variant, gpu, grid=grid)
    assert res[3] == 1
    for l in range(len(W)):
        assert torch.equal(W[l].cpu(), torch.tensor(r.W[l], dtype=F64)), (name, variant, grid, "W", l)
        assert torch.equal(dW[l].cpu(), torch.tensor(r.dW[l], dtype=F64)), (name, variant, grid, "dW", l)


# ----------------------------------------------------------------------------- stop rule
STOP = oc.stop_cases()


@pytest.mark.parametrize("variant", ("lds", "global", "coop"))
@pytest.mark.parametrize("key", list(STOP))
def test_stop_rule(gpu, key, variant):
    """lr = 0 on integer data: dEp is exactly 0 and the result words follow the rule alone"""
    c, exp = STOP[key]
    r = oc.run_case(c)
    assert dict(iters=r.iters, ok=r.ok, first_ok=r.first_ok) == exp  # the reference agrees with the table
    W, dW, res = _launch(c, variant, gpu, grid=None if c.sizes[-1] > 256 else 3)
    out, dEp, init_err, iters, ok, first_ok = res
    assert (iters, ok, first_ok) == (exp["iters"], exp["ok"], exp["first_ok"]), (key, variant, res[3:])
    assert dEp == 0.0 and _unchanged(c, W, dW)
    if c.net == "SNN":
        # long double does not underflow at e^-801, so the spread is that of the FP64 orders
        others = [oc.run_case(c, o) for o in ("reversed", "strided")]
        sp = max(abs(float(v.init_err) - float(r.init_err)) for v in others)
        tol = oc.MARGIN * sp + oc.FLOOR_ULP * oc.EPS * abs(float(r.init_err))
        assert abs(init_err - float(r.init_err)) <= tol, (init_err, float(r.init_err), tol)
        o = out.cpu().numpy()
        tol_o = oc.MARGIN * max(float(np.abs(v.out - r.out).max()) for v in others) + oc.FLOOR_ULP * oc.EPS * float(
            r.out.max())
        assert (o[[1, 3]] == 0.0).all() and np.abs(o - r.out).max() <= tol_o, (o, r.out, tol_o)
    else:
        assert torch.equal(out.cpu(), torch.tensor(r.out, dtype=F64)) and init_err == float(r.init_err)


# ----------------------------------------------------------------------------- run to convergence
@pytest.mark.parametrize("name,variant", [("conv70", "global"), ("conv1100", "lds"), ("conv130", "coop")])
def test_run_to_convergence(gpu, name, variant):
    """the project's default limits: the iteration count, ok and first_ok exact, the weights
    within tolerance after hundreds to thousands of iterations"""
    oc.check_converge_precondition(name)
    oc.check_precondition(name)
    c = oc.case(name)
    W, dW, res = _launch(c, variant, gpu)
    _compare(name, variant, W, dW, res)
