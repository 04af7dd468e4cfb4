"""The check functions of test_tn8_gpu.py and test_bf16_helpers_gpu.py (tests/tn8_common.py) run on
CPU tensors through the emulations of hpnn_amd.ops: the float64 references, the guards, the protocol
checks and the claim that the recipe's arithmetic is exact in FP32 are themselves right, and every
listed shape meets the launchers' divisibility rules -- so a later change of a parameter or a
case cannot make the GPU tests vacuous without a test failing here."""
import pytest
import torch

from tests import tn8_common as tc

CPU = torch.device("cpu")


def test_recipe_is_exact_at_the_bound():
    """three steps with every gradient element on the bound +-9 Bt stay exact; one step more in
    range would not be claimed: exact() does fail outside FP32"""
    g = torch.full((4, 8), 9.0 * tc.BT_MAX, dtype=torch.float64)
    g[1::2] *= -1
    for momentum in (False, True):
        W, V = tc.start_state(4, 8, tc._gen(0), CPU)
        for _ in range(tc.LAUNCHES):
            W, V = tc.ref_step(W, V, g, momentum)
    with pytest.raises(AssertionError):
        tc.exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    assert 9 * tc.BT_MAX < 2 ** 24 and max(c[3] for c in tc.MODE2_CASES) <= tc.BT_MAX


def test_shapes_meet_the_rules():
    for N, M, Bt in tc.MODE1_SHAPES:
        assert tc.mode1_ok(N, M, Bt, N, M) and tc.mode1_ok(N, M, Bt, N + 32, M + 64)
    assert not tc.mode1_ok(288, 256, 128, 288, 256) and not tc.mode1_ok(256, 256, 192, 256, 256)
    want = [(1, 128), (1, 192), (8, 20), (16, 9), (16, 16), (32, 5), (32, 7)]
    for (N, M, splits, Bt), (tiles, sp) in zip(tc.MODE2_CASES, want):
        assert tc.mode2_plan(N, M, Bt, splits) == (256, tiles, sp)
        assert tc.mode2_plan(N, M, Bt, splits, N + 32, M + 64) == (256, tiles, sp)
        assert (Bt // 64 // splits == 2) != ((N, M, splits, Bt) == tc.MODE2_CASES[4])  # one iteration but for one case
    for N, M, splits, Bt in tc.MODE2_REFUSED:
        assert tc.mode2_plan(N, M, Bt, splits) is None
    # each refusal has the one cause it is listed for
    assert tc.mode2_plan(2048, 1024, 1152, 9, cus=512) == (256, 32, 9)
    assert tc.mode2_plan(256, 256, 256, 2, cus=4) == (256, 1, 2)
    assert tc.mode2_plan(1024, 1024, 2048, 16) == (256, 16, 16)
    assert tc.mode2_plan(256, 32 * 256, 512, 4) == (256, 32, 4)
    for (N, M, splits, Bt), N1, M1, S, fits in tc.SIDE_CASES:
        assert tc.side_fits(splits * (N // 256) * (M // 256), Bt, N1, M1, S) == fits
    assert [tc.mode2_plan(N, M, Bt, sp, tm128=True) for N, M, sp, Bt in tc.TM128_CASES] == [(128, 2, 64),
                                                                                          (128, 32, 8)]
    # an odd split count keeps the 256-wide tile
    assert tc.mode2_plan(1024, 1024, 1152, 9, tm128=True) == (256, 16, 9)


def test_guards_notice_a_stray_write():
    g = tc.Guarded(8, torch.bfloat16, CPU, offset=1)
    assert g.untouched() and g.intact() and g.sentinel(g.t)
    g.t[0] = 1.0
    assert g.intact() and not g.untouched() and not g.sentinel(g.t)
    g.buf[g.hi] = 1.0
    assert not g.intact()
    f = tc.Guarded(8, torch.float32, CPU)
    f.buf[f.lo - 1] = float("nan")  # the sentinel itself: a NaN store is not a change
    assert f.intact()
    f.buf[f.lo - 1] = 0.0
    assert not f.intact()


@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("shape", tc.MODE1_SHAPES)
def test_mode1(shape, momentum):
    tc.check_mode1(CPU, *shape, momentum)


def test_mode1_padded_and_random():
    for shape in tc.MODE1_PADDED:
        tc.check_mode1(CPU, *shape, True, padded=True)
    tc.check_mode1_random(CPU, False)
    tc.check_mode1_random(CPU, True)


def test_a_wrong_step_fails_the_check():
    """the check functions are not vacuous: the emulation with another alpha, and a transposed
    operand, are caught"""
    with pytest.raises(AssertionError):
        alpha, tc.ALPHA = tc.ALPHA, 0.25
        try:
            L = tc.Layer(256, 256, CPU)
            W, V = tc.start_state(256, 256, tc._gen(1), CPU)
            L.start(W, V, True)
            D, H = tc.int_operands(128, 256, 256, tc._gen(2), CPU)
            tc.ops.gemm_tn_update(D, H, *L.args(True), tc.LR, alpha, tc.SCALE, True)
            W, V = tc.ref_step(W, V, tc.partials(D, H, 1)[0], True)
            L.check(W, V, True, "alpha")
        finally:
            tc.ALPHA = alpha
    L = tc.Layer(256, 256, CPU)
    W, V = tc.start_state(256, 256, tc._gen(1), CPU)
    L.start(W, V, False)
    D, H = tc.int_operands(128, 256, 256, tc._gen(2), CPU)
    tc.ops.gemm_tn_update(H, D, *L.args(False), tc.LR, tc.ALPHA, tc.SCALE, False)
    W, V = tc.ref_step(W, V, tc.partials(D, H, 1)[0], False)
    with pytest.raises(AssertionError):
        L.check(W, V, False, "swapped")


@pytest.mark.parametrize("case", tc.MODE3_CASES)
def test_mode3(case):
    tc.check_mode3(CPU, *case)


def test_mode3_random_and_ok():
    tc.check_mode3_random(CPU)
    tc.check_mode3_ok_agrees(CPU)


@pytest.mark.parametrize("case", tc.MODE2_CASES)
def test_mode2(case):
    tc.check_mode2(CPU, *case, True)


def test_mode2_variants():
    tc.check_mode2(CPU, *tc.MODE2_CASES[2], False, padded=True)
    tc.check_mode2(CPU, *tc.MODE2_CASES[3], True, wt_offset=1)
    tc.check_mode2_random(CPU, True, case=tc.MODE2_CASES[3])


@pytest.mark.parametrize("i", range(4))
def test_side(i):
    case, N1, M1, S, fits = tc.SIDE_CASES[i]
    assert fits
    tc.check_mode2(CPU, *case, i % 2 == 0, side=(N1, M1, S), side_padded=i == 1)


def test_side_random():
    case, N1, M1, S, _ = tc.SIDE_CASES[3]
    tc.check_mode2_random(CPU, False, case=case, side=(N1, M1, S))


@pytest.mark.parametrize("n", tc.HELPER_SIZES[:2])
def test_helpers(n):
    tc.check_cast(CPU, n)
    tc.check_dact(CPU, n)
    for momentum in (False, True):
        tc.check_sgd_rows(CPU, n, momentum)


def test_helpers_other():
    tc.check_cast_refused(CPU)
    tc.check_sgd_rows_refused(CPU)
    for momentum in (False, True):
        tc.check_sgd_rows_random(CPU, momentum)
    for N, K in tc.TRANSPOSE_SHAPES:
        tc.check_transpose(CPU, N, K)
    tc.check_transpose_refused(CPU)
    for P, rows, n in tc.PERMUTE_CASES[:-1]:
        tc.check_block_permute(CPU, P, rows, n)


@pytest.mark.parametrize("n", tc.HASH_SIZES)
def test_hash(n):
    tc.check_hash(CPU, n)
