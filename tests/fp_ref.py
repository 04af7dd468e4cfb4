"""Float64 references and element-wise error bounds for the FP64 / FP32 engine kernels
(csrc/gpu/kernels_fp.hip), shared by test_fp_kernels_gpu.py (which applies them to the
kernels) and test_fp_ref_cpu.py (which checks on the CPU that they are neither so loose
that a wrong result passes nor so tight that a correct one fails).

All references are float64 tensors on the CPU; operands are given as float64 tensors whose
values are representable in the kernel's type."""
import torch

U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}  # unit roundoff


def bip(x):
    """the bipolar sigmoid f(x) = 2 / (1 + e^-x) - 1"""
    return 2.0 / (1.0 + torch.exp(-x)) - 1.0


def dbip(y):
    """f' expressed in the activation: -0.5 (y^2 - 1)"""
    return -0.5 * (y * y - 1.0)


def gemm_none_bound(a, b, u):
    """|got - ref|[m, n] <= 2 (K + 2) u (|a| |b|)[m, n] for a [M x K] . b [K x N]: the standard
    bound gamma_K |a| |b| on a K-term dot product in any summation order (fused or not), the
    factor 2 covering the float64 reference's own rounding and the higher-order terms"""
    K = a.shape[1]
    return 2.0 * (K + 2) * u * (a.abs().double() @ b.abs().double())


def gemm_bound(epi, none_bound, ref, aux, u):
    """bound of an epilogue's result from the bound of its accumulator: none; bipolar f
    (1/2-Lipschitz, plus 8 u for exp, the division and the subtraction on values <= 2);
    * f'(aux) (plus 4 u |ref| for f' and the product)"""
    if epi == 0:
        return none_bound
    if epi == 1:
        return 0.5 * none_bound + 8.0 * u
    return none_bound * dbip(aux).abs() + 4.0 * u * ref.abs()


def gemm_ref(epi, acc, aux):
    """the epilogue applied to a float64 accumulator"""
    if epi == 0:
        return acc
    if epi == 1:
        return bip(acc)
    return acc * dbip(aux)


def int_operands(M, N, K, seed):
    """integer operands in [-3, 3] as int64: a [M x K], b [K x N] with b row-dependent in n
    (so a transposed or permuted store cannot pass), and their exact product"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g)
    b = (torch.randint(0, 7, (K, N), generator=g) + torch.arange(N)[None, :]) % 7 - 3
    return a, b, a @ b


def output_ref(z, t, net, n_valid):
    """the output layer in float64: (o, d, loss per row); net 0 = bipolar (ANN), 1 = linear
    (LNN), 2 = softmax (SNN) in its max-shifted form
    exp(z - zmax) / (sum exp(z - zmax) + TINY * exp(1 - zmax)), which is the reference's
    e^{z-1} / (TINY + sum e^{z-1}) without the overflow.  Rows >= n_valid have d = 0 and no
    loss."""
    TINY = 1e-14
    n_out = z.shape[1]
    if net == 2:
        zmax = z.max(1, keepdim=True).values
        e = torch.exp(z - zmax)
        o = e / (e.sum(1, keepdim=True) + TINY * torch.exp(1.0 - zmax))
        d = t - o
        loss = -(torch.where(o > 0, t * torch.log(o + TINY), torch.zeros_like(o))).sum(1) / n_out
    elif net == 0:
        o = bip(z)
        d = (t - o) * dbip(o)
        loss = 0.5 * ((t - o) ** 2).sum(1)
    else:
        o = z.clone()
        d = t - o
        loss = 0.5 * ((t - o) ** 2).sum(1)
    d[n_valid:] = 0
    loss[n_valid:] = 0
    return o, d, loss


def first_argmax(x):
    """index of the first maximum of each row (the reference's evaluation rule)"""
    m = x.max(1, keepdim=True).values
    idx = torch.arange(x.shape[1])[None, :].expand_as(x)
    return torch.where(x == m, idx, torch.full_like(idx, x.shape[1])).min(1).values


def update_ref(w, v, g, lr, alpha, scale, momentum):
    """BP: W += lr * scale * sum_s G[s]; BPM: V += lr * g, W += V, V *= alpha (float64).
    Returns (W, V, bound / ((S + 4) u)) with the bound's magnitude term
    lr |scale| sum_s |G| + |V| + |W|"""
    gs = scale * g.sum(0)
    mag = lr * abs(scale) * g.abs().sum(0) + w.abs()
    if momentum:
        vn = v + lr * gs
        return w + vn, vn * alpha, mag + v.abs()
    return w + lr * gs, None, mag
