"""The integer-exact fixtures of the fused fronts on the CPU (tests/front_exact_common.py):
  - the FP64 reference meets its own exactness conditions for every parametrisation that
    tests/test_front_exact_gpu.py runs (the reference asserts them);
  - the PyTorch emulations of the fronts (ops.mlp3_tile / mlp3_eval / mlp3_fused / mlp3_mid /
    wide2_front on CPU tensors) give the reference's bits;
  - every small mutant of the REFERENCE (an extra valid row, a dropped k-step, swapped row
    groups, a neighbour's f', another tie rule, a missing split, swapped labels) changes at
    least one compared output, so the GPU comparison would notice the same slip in a kernel."""
import pytest
import torch

from hpnn_amd import ops
from tests import front_exact_common as fc

CUS = 256  # the MI355X's compute units: the default grid of the fused front's two-tile case


def _fused_fixture(case, cus=CUS):
    net, K0, d1_fm, Bp, grid = case
    if Bp == 0:
        Bp, grid = 32 * (cus + 44), cus
    fx = fc.make_mlp3(net, K0, Bp, 10, u8=False, seed=fc.SEED)
    return fx, min(Bp - 5 if grid != 1 else Bp, fx.n_good), grid, d1_fm


def _step_fixture(net):
    return fc.make_mlp3(net, 800, 4096, 10, u8=True, seed=fc.SEED, n_in=784)


# ------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("case", fc.TILE_CASES, ids=str)
def test_conditions_tile(case):
    fx, n_valid, _ = fc.tile_fixture(case)
    ref = fc.reference(fx, n_valid)  # asserts every condition
    print(case, n_valid, fc.describe(ref["stats"]))
    fc.reference(fx, fx.n_good)  # the populated back chain, whatever n_valid the case runs
    assert n_valid >= 1 and (case[0] != "SNN" or fx.n_good >= 0.9 * fx.Bp)
    if case[0] == "SNN":
        tied, below = fc.snn_hit_rule_exercised(fx, fx.n_good)
        assert tied > 0 and below > 0, (tied, below)


@pytest.mark.parametrize("case", fc.FUSED_CASES, ids=str)
def test_conditions_fused(case):
    fx, n_valid, _, _ = _fused_fixture(case)
    print(case, n_valid, fc.describe(fc.reference(fx, n_valid)["stats"]))


def test_cases_cover_what_the_kernels_take():
    assert sorted({c[1] for c in fc.FUSED_CASES}) == sorted(ops.MLP3F_K0)
    assert sorted({c[3] for c in fc.TILE_CASES}) == sorted(ops.MLP3T_K0)
    assert {c[7] for c in fc.TILE_CASES} == {"all", "m5", 200, 1} and {c[4] for c in fc.TILE_CASES} == {10, 24}
    assert {(c[5], c[6]) for c in fc.TILE_CASES} == {(512, 1), (512, 2), (768, 2)}
    assert {(c[0], c[2]) for c in fc.TILE_CASES} == {(n, u) for n in ("ANN", "LNN", "SNN") for u in (True, False)}


@pytest.mark.parametrize("case", fc.WIDE_CASES, ids=str)
def test_conditions_wide(case):
    net, n_out, n_valid, _ = case
    fx = fc.make_wide(net, 256, n_out, seed=fc.SEED)
    assert fx.n_good >= n_valid
    print(case, fc.describe(fc.reference_wide(fx, n_valid)["stats"]))


@pytest.mark.parametrize("net", ["LNN", "SNN"])
@pytest.mark.parametrize("momentum", [False, True])
def test_conditions_step(net, momentum):
    fx = _step_fixture(net)
    assert fx.n_good >= fc.STEP_NVALID
    ref = fc.reference(fx, fc.STEP_NVALID, splits=1)
    print(net, fc.describe(ref["stats"]))
    # asserts that FP32 holds every stepped value
    new = fc.reference_step(fx, ref, fc.STEP_NVALID, fc.STEP_LR, fc.STEP_ALPHA, momentum)
    assert all(not torch.equal(w, old.float()) for (w, _, _), old in zip(new, (fx.W0, fx.W1, fx.W2)))


# ------------------------------------------------------------------------------- emulations
@pytest.mark.parametrize("case", fc.TILE_CASES, ids=str)
def test_tile_and_eval_emulations_give_the_reference(case):
    fx, n_valid, grid = fc.tile_fixture(case)
    ref = fc.reference(fx, n_valid)
    op = fc.operands(fx, "cpu")
    got = fc.run_tile(op, n_valid, grid)
    fc.compare(got, ref, ("delta1", "gslab", "loss", "hits"), fx.net, n_valid, fx.n_out)
    ev = fc.run_eval(op, n_valid, grid)
    fc.compare(ev, ref, ("guess", "loss", "hits"), fx.net, n_valid, fx.n_out)
    assert torch.equal(ev["stats"], got["stats"])


@pytest.mark.parametrize("case", fc.FUSED_CASES[:5], ids=str)
def test_fused_emulation_gives_the_reference(case):
    fx, n_valid, grid, d1_fm = _fused_fixture(case)
    ref = fc.reference(fx, n_valid)
    got = fc.run_fused(fc.operands(fx, "cpu"), n_valid, grid, d1_fm)
    fc.compare(got, ref, ("delta1", "gslab", "loss", "hits"), fx.net, n_valid, fx.n_out)


@pytest.mark.parametrize("case", fc.MID_CASES, ids=str)
def test_mid_emulation_gives_the_reference(case):
    net, grid = case
    fx = fc.make_mlp3(net, 256, 128, 10, u8=False, seed=fc.SEED)
    n_valid = min(123, fx.n_good)
    ref = fc.reference(fx, n_valid)
    got = fc.run_mid(fc.operands(fx, "cpu"), ref["H1"].to(torch.bfloat16), n_valid, grid)
    fc.compare(got, ref, ("delta1", "gslab", "loss", "hits"), net, n_valid, 10)


@pytest.mark.parametrize("case", fc.WIDE_CASES, ids=str)
def test_wide_emulation_gives_the_reference(case):
    net, n_out, n_valid, ksplit = case
    fx = fc.make_wide(net, 256, n_out, seed=fc.SEED)
    ref = fc.reference_wide(fx, n_valid)
    got = fc.run_wide(fc.operands(fx, "cpu", u8=False), n_valid, ksplit)
    fc.compare(got, ref, ("H0", "delta2", "delta1", "loss", "hits"), net, n_valid, n_out)


def test_g0_emulation_gives_the_reference_per_split():
    fx, n_valid, _ = fc.tile_fixture(fc.TILE_CASES[0])
    ref = fc.reference(fx, n_valid)
    D1g = ops.to_fragment_major(ref["delta1"].to(torch.bfloat16))
    Xg = ops.to_fragment_major(fx.X.to(torch.uint8))
    slab = ops.gemm_fm_direct(D1g, Xg, 128, fx.K0, splits=1, hscale=0.5)
    assert torch.equal(slab[0].double(), 0.5 * ref["G0"])


# ------------------------------------------------------------------------------- sensitivity
_KEYS = ("delta1", "gslab", "G0", "guess")


def _differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in _KEYS) or a["loss"] != b["loss"] or a["hits"] != b["hits"]


@pytest.mark.parametrize("net", ["LNN", "ANN", "SNN"])
@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_reference_mutants_are_detected(net, mutant):
    """the compared outputs (delta1, [G1 | G2], G0 over 4 splits, loss, hits, guess) tell every
    mutant from the true reference, for every output type"""
    fx = fc.make_mlp3(net, 800, 512, 10, u8=True, seed=fc.SEED)
    n_valid = min(fx.Bp - 5, fx.n_good)
    true = fc.reference(fx, n_valid, splits=4)
    assert not _differs(true, fc.reference(fx, n_valid, splits=4, check=False))
    assert _differs(true, fc.reference(fx, n_valid, mutant=mutant, splits=4))
