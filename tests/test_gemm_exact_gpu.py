"""Every arm of the BF16 NT / TN GEMM dispatch (csrc/gpu/kernels_mfma.hip, kernels_ws.hip, and the
hand-over to kernels_8ph.hip) on integer-exact operands against float64 references, bit for bit; the
tail reduction riding each TN launch shape; the launchers' refusals; cast_weights and reduce_slabs2.

Cases, references and check functions: tests/gemm_exact_common.py (run on CPU tensors, and checked
against the dispatcher, by test_gemm_exact_cpu.py).  Every case asks ops.gemm_nt_plan / ops.gemm_tn_plan
which arm and ring depth it runs before it launches, so a case cannot silently land on another arm;
every output is sentinel-guarded with a padded row stride."""
import pytest
import torch

from tests import gemm_exact_common as gc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------- NT
@pytest.mark.parametrize("c", gc.NT_CASES, ids=gc.nt_id)
def test_nt_exact(gpu, c):
    """three epilogues x two output types per case: EPI_NONE / EPI_DACT bitwise, EPI_ACT within the
    project's tolerance and its BF16 output bitwise the rounded FP32 output"""
    gc.check_nt(gpu, c)


@pytest.mark.parametrize("N,K", gc.WS_PAIRS, ids=lambda v: str(v))
def test_ws_direct(gpu, N, K):
    """the weight-stationary kernel below its dispatch threshold: one tile; one workgroup with two tiles
    beside CUs - 1 with one; nloc 4 and 5, above every ring depth"""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for M in gc.ws_rows(cus):
        gc.check_ws(gpu, N, K, M)


def test_ws_refusals_write_nothing(gpu):
    gc.check_ws_refused(gpu)


def test_ws_through_the_dispatcher(gpu):
    gc.check_ws_dispatched(gpu)


@pytest.mark.parametrize("epi", gc.EPIS, ids=lambda e: gc.EPI_NAME[e])
def test_nn_exact(gpu, epi):
    gc.check_nn(gpu, epi)


# ---------------------------------------------------------------------------- TN
@pytest.mark.parametrize("c", gc.TN_CASES, ids=gc.tn_id)
def test_tn_exact(gpu, c):
    """every split's slab against the float64 product of its own rows"""
    gc.check_tn(gpu, c)


@pytest.mark.parametrize("i", range(len(gc.TAIL_LAUNCHES)), ids=lambda i: gc.TAIL_LAUNCHES[i].arm)
def test_tn_tail_on_each_launch_shape(gpu, i):
    """TM x TN, 64 x 64, xcd_map on, 256 x 256 4-stage, 8-phase: each carries one (S, groups, n)"""
    S, groups = gc.TAIL_SG[i]
    gc.check_tn_tail(gpu, gc.TAIL_LAUNCHES[i], S, groups, gc.TAIL_N[i % len(gc.TAIL_N)])


@pytest.mark.parametrize("sg", gc.TAIL_SG, ids=lambda v: "S%d_g%d" % v)
def test_tn_tail_groupings(gpu, sg):
    for n in gc.TAIL_N:
        gc.check_tn_tail(gpu, gc.TAIL_LAUNCHES[0], sg[0], sg[1], n)


# ---------------------------------------------------------------------------- refusals, small kernels
def test_nt_refusals_write_nothing(gpu):
    for row in gc.NT_REFUSED:
        gc.check_nt_refused(gpu, row)


def test_tn_refusals_write_nothing(gpu):
    for row in gc.TN_REFUSED:
        gc.check_tn_refused(gpu, row)
    gc.check_tn_tail_refused(gpu)


@pytest.mark.parametrize("with_wf", [False, True], ids=["plain", "wf"])
@pytest.mark.parametrize("N,K", gc.CAST_SHAPES)
def test_cast_weights(gpu, N, K, with_wf):
    gc.check_cast_weights(gpu, N, K, with_wf)


@pytest.mark.parametrize("with_tmp", [False, True], ids=["one_pass", "tmp"])
@pytest.mark.parametrize("S", gc.REDUCE_S)
def test_reduce_slabs2(gpu, S, with_tmp):
    for n in gc.REDUCE_N:
        gc.check_reduce_slabs2(gpu, S, n, with_tmp)


def test_reduce_slabs2_refusals_write_nothing(gpu):
    gc.check_reduce_slabs2_refused(gpu)
