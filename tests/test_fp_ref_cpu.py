"""The error bounds that test_fp_kernels_gpu.py applies to the FP64 / FP32 GEMM (tests/fp_ref.py),
checked on the CPU: correct products in either summation order stay inside the bound, and a
dot product that lost one of its K terms falls outside it."""
import pytest
import torch

from tests.fp_ref import U, gemm_none_bound, int_operands

SHAPES = [(65, 63, 17), (40, 90, 1000)]


def _operands(M, N, K, dt):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, dtype=torch.float64).to(dt)
    b = torch.randn(K, N, generator=g, dtype=torch.float64).to(dt)
    return a, b


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_correct_products_are_inside_the_bound(M, N, K, dt):
    a, b = _operands(M, N, K, dt)
    ref = a.double() @ b.double()
    bound = gemm_none_bound(a.double(), b.double(), U[dt])
    assert ((a @ b).double() - ref).abs().le(bound).all()
    rev = torch.zeros(M, N, dtype=dt)  # k-reversed sequential sum, rounded after every step
    for k in range(K - 1, -1, -1):
        rev = rev + a[:, k:k + 1] * b[k:k + 1, :]
    assert (rev.double() - ref).abs().le(bound).all()
    assert bound.gt(0).all()


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_dropped_product_is_outside_the_bound(M, N, K, dt):
    a, b = _operands(M, N, K, dt)
    ref = a.double() @ b.double()
    bound = gemm_none_bound(a.double(), b.double(), U[dt])
    for m, n in [(0, 0), (M - 1, N - 1), (M // 2, N // 3)]:
        prod = a[m].double() * b[:, n].double()
        k = prod.abs().argsort()[K // 2]  # a product of median magnitude, not the largest
        got = (a @ b).double()
        got[m, n] -= prod[k]
        bad = (got - ref).abs() > bound
        assert bad[m, n] and bad.sum() == 1, (m, n, float(prod[k]), float(bound[m, n]))


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_integer_operands_are_exact_and_asymmetric(M, N, K):
    a, b, ref = int_operands(M, N, K, 1)
    assert a.abs().max() <= 3 and b.abs().max() <= 3 and 9 * K < 2 ** 24
    assert torch.equal((a.float() @ b.float()).long(), ref)
    assert not torch.equal(b[:min(K, N), :min(K, N)], b[:min(K, N), :min(K, N)].t())
