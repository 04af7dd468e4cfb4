"""The small BF16 kernels behind the data- and tensor-parallel exchanges, and the replica digest
(csrc/gpu/kernels_misc.hip), each against a plain PyTorch / float64 / integer expression: bitwise
where the operation is a rounding or a move.  Sizes: one item, a few blocks, and the first size
that enters the launchers' grid-stride loop (their grids are capped at 4096 blocks).
Check functions: tests/tn8_common.py (run on CPU tensors by test_tn8_cpu.py)."""
import pytest

from tests import tn8_common as tc

pytestmark = pytest.mark.gpu

SIZES = pytest.mark.parametrize("n", tc.HELPER_SIZES)


@SIZES
def test_cast_f32_bf16(gpu, n):
    """vs .bfloat16() on the CPU: ties, subnormals, +-0, +-inf, NaN stays NaN, rounding up to inf"""
    tc.check_cast(gpu, n)


@SIZES
@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
def test_sgd_update_rows_bf16g_exact(gpu, n, momentum):
    tc.check_sgd_rows(gpu, n, momentum)


@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
def test_sgd_update_rows_bf16g_random(gpu, momentum):
    tc.check_sgd_rows_random(gpu, momentum)


@pytest.mark.parametrize("N,K", tc.TRANSPOSE_SHAPES)
def test_transpose_bf16(gpu, N, K):
    tc.check_transpose(gpu, N, K)


@pytest.mark.parametrize("P,rows,n", tc.PERMUTE_CASES)
def test_block_permute(gpu, P, rows, n):
    tc.check_block_permute(gpu, P, rows, n)


@SIZES
def test_dact_cast(gpu, n):
    tc.check_dact(gpu, n)


@pytest.mark.parametrize("n", tc.HASH_SIZES)
def test_hash_words(gpu, n):
    """the device digest equals the numpy emulation (and, at the small sizes, plain integers):
    a base, accumulation with wrap-around, two pieces == the whole, one flipped bit, nbytes 0 and
    nbytes % 4"""
    tc.check_hash(gpu, n)


def test_refusals_write_nothing(gpu):
    """misaligned pointers, n % 4 (n % 8 for block_permute), N or K % 32 for the transpose: the
    documented -2 and no write"""
    tc.check_cast_refused(gpu)
    tc.check_sgd_rows_refused(gpu)
    tc.check_transpose_refused(gpu)
    tc.check_block_permute_refused(gpu)
    tc.check_dact_refused(gpu)
