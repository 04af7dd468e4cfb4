"""The check functions of test_gemm_exact_gpu.py (tests/gemm_exact_common.py) run on CPU tensors through
the emulations of hpnn_amd.ops, and the case tables checked against the dispatcher itself
(ops.gemm_nt_plan / ops.gemm_tn_plan, pure host arithmetic): every case lands on the arm and the
KT-to-ST relation it is listed for, the cases reach every exported arm, the references are exact in
FP32, the EPI_ACT scales leave the sigmoid unsaturated, and a wrong result or a stray write fails the
checks.  A later arm without a case, or a changed rule that moves a case to another arm, fails here."""
import math

import pytest
import torch

from hpnn_amd import ops
from tests import gemm_exact_common as gc
from tests.test_tn8_cpu import test_guards_notice_a_stray_write  # noqa: F401  (the same Guarded class)

CPU = torch.device("cpu")
NT_SMALL = [c for c in gc.NT_CASES if not c.big]
TN_SMALL = [c for c in gc.TN_CASES if not c.big]


# ---------------------------------------------------------------------------- the tables against the dispatcher
def test_every_case_lands_on_its_arm():
    for c in gc.NT_CASES:
        gc.assert_nt_plan(c)
    for c in gc.TN_CASES:
        gc.assert_tn_plan(c)
    for N, K in gc.WS_PAIRS:
        for M in gc.ws_rows(gc.CPU_CUS):
            assert gc.native().gemm_nt_ws_plan(M, N, K, K + 64, K, N + gc.LDC_PAD, ops.EPI_ACT) == gc.WS_ST[K]
    # the ring depths the tables list are the dispatcher's
    assert {a: st for a, (_, st) in gc.NT_ARM.items() if a != "ws"} == {
        c.arm: gc.nt_plan_of(c, ops.EPI_NONE)[1] for c in gc.NT_CASES}
    assert gc.TN_ST == {c.arm: gc.tn_plan_of(c)[1] for c in gc.TN_CASES}


def test_cases_reach_every_arm(capsys):
    """the arms the case tables reach == the exported arm lists minus the pairs no shape can reach;
    prints the cases per arm"""
    nt, tn = gc.coverage()
    with capsys.disabled():
        for name, cov in (("NT", nt), ("TN", tn)):
            for arm, ids in cov.items():
                print("%s %-12s %2d: %s" % (name, arm, len(ids), ", ".join(ids)))
    assert set(nt) == set(ops.gemm_nt_arms()) == set(gc.NT_ARM)
    assert all(nt[a] for a in nt), [a for a in nt if not nt[a]]
    assert set(tn) == set(ops.gemm_tn_arms()) == set(gc.TN_ST)
    assert {a for a in tn if not tn[a]} == gc.TN_UNREACHABLE


def test_kt_relations_per_arm():
    """every arm runs at KT = 1 (NT) / 2 (TN), ST - 1, ST, ST + 1 and 2 ST + 1 (TN: 2 ST + 2) as far as its K
    rule admits: BK = 32 arms take odd KT only (K % 64 != 0), TN arms even KT only (two 32-row stages per
    64-row unit), the 256 x 256 and 8-phase arms start at 256 tiles with K >= 512"""
    for arm, (bk, st) in gc.NT_ARM.items():
        if arm in ("ws", "8ph", "256x256"):
            continue
        want = {k for k in (1, st - 1, st, st + 1, 2 * st + 1) if k >= 1 and (bk == 64 or k % 2 == 1)}
        got = {c.K // bk for c in gc.NT_CASES if c.arm == arm}
        assert want <= got, (arm, want, got)
    for arm, st in gc.TN_ST.items():
        if arm in ("8ph", "256x256"):
            continue
        want = {2, 2 * st + 2} | {k for k in (st - 1, st, st + 1) if k % 2 == 0}
        got = {k for c in gc.TN_CASES if c.arm == arm and c.rel != "uneven" for k in gc.tn_kts(c)}
        assert want <= got, (arm, want, got)
        assert any(c.rel == "uneven" for c in gc.TN_CASES if c.arm == arm), arm
    # both sides of the xcd_map rule (splits % 8 == 0 with more than one tile)
    on = [c for c in gc.TN_CASES if c.splits % 8 == 0 and (c.N > 64 or c.M > 128)]
    assert {c.splits for c in on} >= {8, 16} and any(c.splits == 8 and (c.N, c.M) == (64, 32) for c in gc.TN_CASES)


def test_tn_sweep_of_the_dispatcher():
    """N, M <= 640 in steps of 32, splits in {1, 2, 8}: the arms the dispatcher chooses there are all
    but TN_SWEEP_UNREACHED (the four pairs that need (M / 128)(N / 128) splits >= 256 with M, N % 64 == 0,
    and the two 256-tile arms); the case tables reach those at larger split counts and sizes"""
    seen = set()
    for N in range(32, 641, 32):
        for M in range(32, 641, 32):
            for splits in (1, 2, 8):
                arm, st = ops.gemm_tn_plan(N, M, 64 * splits * 2, splits, N, M, M)
                assert st == gc.TN_ST[arm]
                seen.add(arm)
    assert set(ops.gemm_tn_arms()) - seen == gc.TN_SWEEP_UNREACHED
    for arm in gc.TN_SWEEP_UNREACHED:
        assert any(c.arm == arm for c in gc.TN_CASES), arm


def test_toggles_are_honoured_and_restored():
    c = next(c for c in gc.NT_CASES if c.arm == "w8_128")
    assert gc.nt_plan_of(c, ops.EPI_NONE)[0] == "w8_128"
    assert gc.nt_plan_of(c._replace(off=()), ops.EPI_NONE)[0] == "pp128"
    c = next(c for c in gc.NT_CASES if c.arm == "256x256" and c.off)
    assert gc.nt_plan_of(c._replace(off=()), ops.EPI_NONE)[0] == "8ph"
    c = next(c for c in gc.TN_CASES if c.arm == "256x256" and c.off)
    assert gc.tn_plan_of(c._replace(off=()))[0] == "8ph"
    with pytest.raises(ZeroDivisionError):
        with gc.toggled(gemm_nt_set_pp=0):
            1 // 0
    assert gc.nt_plan_of(next(c for c in gc.NT_CASES if c.arm == "pp128"), ops.EPI_NONE)[0] == "pp128"


def test_act_scales():
    """the scale of every case is a power of two that keeps 4 sqrt(K) scale <= 8 (check_nt asserts on
    the reference itself that at least half of the pre-activations lie in [-8, 8])"""
    for c in gc.NT_CASES:
        assert c.scale == gc.act_scale(c.K) and 4.0 * c.K ** 0.5 * c.scale <= 8.0
        assert c.scale == 1.0 or 8.0 * c.K ** 0.5 * c.scale > 8.0  # the largest such power of two
        assert math.frexp(c.scale)[0] == 0.5


def test_exactness_bound():
    for c in gc.NT_CASES:
        assert 9 * c.K < 2 ** 24
    for c in gc.TN_CASES:
        assert 9 * c.Bt < 2 ** 24
    with pytest.raises(AssertionError):
        gc.exact(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64))


# ---------------------------------------------------------------------------- the checks on CPU tensors
@pytest.mark.parametrize("c", NT_SMALL, ids=gc.nt_id)
def test_nt(c):
    gc.check_nt(CPU, c)


@pytest.mark.parametrize("c", [c for c in gc.NT_CASES if c.big], ids=gc.nt_id)
def test_nt_big_reference(c):
    """the workload-size cases: plan, exactness of the reference and one emulated launch"""
    gc.check_nt(CPU, c, epis=(ops.EPI_DACT,), types=(False,))


@pytest.mark.parametrize("c", TN_SMALL, ids=gc.tn_id)
def test_tn(c):
    gc.check_tn(CPU, c)


@pytest.mark.parametrize("c", [c for c in gc.TN_CASES if c.big], ids=gc.tn_id)
def test_tn_big(c):
    gc.check_tn(CPU, c)


@pytest.mark.parametrize("N,K", gc.WS_PAIRS)
def test_ws(N, K):
    for M in gc.ws_rows(gc.CPU_CUS)[:2]:
        gc.check_ws(CPU, N, K, M)


def test_ws_other():
    gc.check_ws(CPU, 128, 512, gc.ws_rows(gc.CPU_CUS)[2])
    gc.check_ws_refused(CPU)
    gc.check_ws_dispatched(CPU)


@pytest.mark.parametrize("epi", gc.EPIS)
def test_nn(epi):
    gc.check_nn(CPU, epi)


@pytest.mark.parametrize("i", range(len(gc.TAIL_LAUNCHES)))
def test_tn_tail(i):
    S, groups = gc.TAIL_SG[i]
    gc.check_tn_tail(CPU, gc.TAIL_LAUNCHES[i], S, groups, gc.TAIL_N[i % len(gc.TAIL_N)])


def test_tn_tail_every_grouping():
    for S, groups in gc.TAIL_SG:
        for n in gc.TAIL_N:
            gc.check_tn_tail(CPU, gc.TAIL_LAUNCHES[0], S, groups, n)
    assert float(gc.group_sums(torch.ones(9, 4), 8)[5:].abs().sum()) == 0.0  # (9, 8): groups 5..7 are empty


def test_refusal_codes():
    for row in gc.NT_REFUSED:
        gc.check_nt_refused(CPU, row)
    for row in gc.TN_REFUSED:
        gc.check_tn_refused(CPU, row)


@pytest.mark.parametrize("N,K", gc.CAST_SHAPES)
def test_cast_weights(N, K):
    gc.check_cast_weights(CPU, N, K, False)
    gc.check_cast_weights(CPU, N, K, True)


def test_reduce_slabs2():
    for S in gc.REDUCE_S:
        for n in gc.REDUCE_N:
            gc.check_reduce_slabs2(CPU, S, n, S % 2 == 0)


# ---------------------------------------------------------------------------- the checks are not vacuous
def test_a_swapped_index_fails_the_checks():
    """a seeded swap of two elements in a copy of the reference, a transposed tile, an unwritten element
    and a write into the padding are each caught"""
    gen = gc._gen(7)
    c = NT_SMALL[0]
    A, B, aux = gc.nt_operands(c.M, c.N, c.K, c.padded, gen, CPU)
    R = gc.nt_product(A, B)
    g, C = gc.out_buffer(c.M, c.N, True, CPU)
    ops.gemm_nt(A, B, ops.EPI_NONE, out_f32=True, out=C)
    gc.check_out(g, C, "ok")
    gc.compare_epi({True: C}, R, ops.EPI_NONE, "ok")
    bad = R.clone()
    i, j = (int(v) for v in torch.randint(0, c.N // 2, (2,), generator=gen))
    k = next(k for k in range(j + 1, c.N) if float(R[i, k]) != float(R[i, j]))
    bad[i, j], bad[i, k] = R[i, k], R[i, j]
    with pytest.raises(AssertionError):
        gc.compare_epi({True: C}, bad, ops.EPI_NONE, "swapped")
    blk = R.clone()
    blk[:16, :16] = R[:16, :16].t()
    with pytest.raises(AssertionError):
        gc.compare_epi({True: C}, blk, ops.EPI_NONE, "transposed fragment")
    full = g.view(c.M, c.N + gc.LDC_PAD)
    full[3, c.N] = 0.0
    with pytest.raises(AssertionError):
        gc.check_out(g, C, "padding")
    g, C = gc.out_buffer(c.M, c.N, False, CPU)
    ops.gemm_nt(A, B, ops.EPI_NONE, out_f32=False, out=C)
    g.view(c.M, c.N + gc.LDC_PAD)[5, 7:8].view(torch.int16).fill_(gc.Guarded(1, torch.bfloat16, CPU).sent)
    with pytest.raises(AssertionError):
        gc.check_out(g, C, "unwritten")
    # TN: the slab of one split given the rows of another
    t = next(c for c in TN_SMALL if c.splits == 3)
    D, H = gc.tn_operands(t, gen, CPU)
    g, out = gc.slab_buffer(t, CPU)
    ops.gemm_tn(D, H, t.splits, out=out)
    P = gc.tn_reference(D, H, t.splits)
    gc.check_slab(g, out, P, "ok")
    with pytest.raises(AssertionError):
        gc.check_slab(g, out, P[[1, 0, 2]], "splits swapped")
    # a double rounding on the BF16 store: through FP32 -> BF16 of a value already rounded to 9 bits
    x = torch.tensor([257.0 + 2.0 ** -10], dtype=torch.float64)  # rounds to 258 once, 256 if first cut to 257
    assert float(x.float().bfloat16()) == 258.0 and float(torch.tensor([257.0]).bfloat16()) == 256.0
