"""The fused front kernels bit for bit on integer-exact inputs (tests/front_exact_common.py):
hpnn_mlp3_tile / hpnn_mlp3_eval (kernels_mlp3t.hip), hpnn_mlp3_fused (kernels_mlp3x.hip),
hpnn_mlp3_mid (kernels_mlp3.hip), hpnn_wide2_front (kernels_wide.hip) with the shared output
layer of mlp3_common.h, the first-layer gradient hpnn_gemm_fm_direct on the fixture's delta1,
and one whole plan step.  Every comparison with the FP64 reference is torch.equal / ==; the
SNN loss alone goes through __logf and is held to the bound derived in
front_exact_common.snn_loss_bound.  The metamorphic tests at the end run on ordinary random
data and need no assumption.  Measured values: profiles/front_exact/README.md."""
import functools

import pytest
import torch

from hpnn_amd import ops
from hpnn_amd.models import MLP
from tests import front_exact_common as fc

pytestmark = pytest.mark.gpu
PROBE_X = (0.0, 32.0, -32.0, 64.0, -64.0, 4096.0, -4096.0)
_probe = {}


def _device_bipolar(gpu):
    """f on the device at PROBE_X through the GEMM epilogue (A = the values on a diagonal
    times an identity B: integer operands, exact sums)"""
    if not _probe:
        A = torch.zeros(128, 32)
        A[torch.arange(len(PROBE_X)), torch.arange(len(PROBE_X))] = torch.tensor(PROBE_X)
        C = ops.gemm_nt(A.bfloat16().cuda(), torch.eye(32).bfloat16().cuda(), epi=ops.EPI_ACT, out_f32=True)
        torch.cuda.synchronize()
        C = C.cpu()
        _probe["f"] = [float(C[i, i]) for i in range(len(PROBE_X))]
        _probe["off"] = float(C[8:, :].abs().max())  # f(0) everywhere else
    return _probe


def _need_exact_zero(gpu):
    p = _device_bipolar(gpu)
    if p["f"][0] != 0.0 or p["off"] != 0.0:
        pytest.skip(f"the device's bipolar(0) is {p['f'][0]!r}, not 0: the backward-exact cases need f(0) = 0")


def test_probe_device_bipolar_is_exact(gpu):
    """2 rcp(1 + __expf(-x)) - 1 on gfx950: exactly 0 at 0 (so rcp(2) is exactly 0.5) and
    exactly +-1 at +-32, +-64 and +-4096 -- what every exact comparison below stands on"""
    p = _device_bipolar(gpu)
    print("device bipolar:", {x: repr(v) for x, v in zip(PROBE_X, p["f"])}, "off-diagonal max", p["off"])
    assert p["f"][0] == 0.0 and p["off"] == 0.0, p
    assert p["f"][1:] == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0], p


@functools.lru_cache(maxsize=None)
def _tile(case):
    fx, n_valid, grid = fc.tile_fixture(case)
    return fx, n_valid, grid, fc.reference(fx, n_valid)


# ------------------------------------------------------------------------------- tile + eval
@pytest.mark.parametrize("case", fc.TILE_CASES, ids=str)
def test_tile_exact(gpu, case):
    _need_exact_zero(gpu)
    fx, n_valid, grid, ref = _tile(case)
    got = fc.run_tile(fc.operands(fx, "cuda"), n_valid, grid)
    fc.compare(got, ref, ("delta1", "gslab", "loss", "hits"), fx.net, n_valid, fx.n_out)


@pytest.mark.parametrize("case", fc.TILE_CASES, ids=str)
def test_eval_exact_and_equal_to_tile(gpu, case):
    """loss, hits and guess against the reference (forward only: needs f(+-32 k) = +-1 and
    f(0) = 0), and the stat slots bit-equal to those of the training front on the same batch
    and grid -- hpnn_mlp3_eval's documented contract"""
    _need_exact_zero(gpu)
    fx, n_valid, grid, ref = _tile(case)
    op = fc.operands(fx, "cuda")
    ev = fc.run_eval(op, n_valid, grid)
    fc.compare(ev, ref, ("guess", "loss", "hits"), fx.net, n_valid, fx.n_out)
    tr = fc.run_tile(op, n_valid, grid)
    assert torch.equal(ev["stats"][:, :2], tr["stats"][:, :2])


# ------------------------------------------------------------------------------- fused, mid
@pytest.mark.parametrize("case", fc.FUSED_CASES, ids=str)
def test_fused_exact(gpu, case):
    _need_exact_zero(gpu)
    net, K0, d1_fm, Bp, grid = case
    assert K0 in ops.MLP3F_K0
    if Bp == 0:  # the default grid with 44 tiles more than workgroups: some take two tiles
        grid = ops.mlp3_fused_grid(1 << 20)
        Bp = 32 * (grid + 44)
        assert ops.mlp3_fused_grid(Bp) == grid
    fx = fc.make_mlp3(net, K0, Bp, 10, u8=False, seed=fc.SEED)
    n_valid = min(Bp - 5 if grid != 1 else Bp, fx.n_good)
    ref = fc.reference(fx, n_valid)
    got = fc.run_fused(fc.operands(fx, "cuda"), n_valid, grid, d1_fm)
    fc.compare(got, ref, ("delta1", "gslab", "loss", "hits"), net, n_valid, 10)


@pytest.mark.parametrize("case", fc.MID_CASES, ids=str)
def test_mid_exact(gpu, case):
    _need_exact_zero(gpu)
    net, grid = case
    fx = fc.make_mlp3(net, 256, 128, 10, u8=False, seed=fc.SEED)
    n_valid = min(123, fx.n_good)
    ref = fc.reference(fx, n_valid)
    got = fc.run_mid(fc.operands(fx, "cuda"), ref["H1"].to(torch.bfloat16).cuda(), n_valid, grid)
    fc.compare(got, ref, ("delta1", "gslab", "loss", "hits"), net, n_valid, 10)


# ------------------------------------------------------------------------------- wide front
@pytest.mark.parametrize("case", fc.WIDE_CASES, ids=str)
def test_wide_exact(gpu, case):
    _need_exact_zero(gpu)
    net, n_out, n_valid, ksplit = case
    fx = fc.make_wide(net, 256, n_out, seed=fc.SEED)
    ref = fc.reference_wide(fx, n_valid)
    got = fc.run_wide(fc.operands(fx, "cuda", u8=False), n_valid, ksplit)
    got["ws"].check()
    fc.compare(got, ref, ("H0", "delta2", "delta1", "loss", "hits"), net, n_valid, n_out)


# ------------------------------------------------------------------------------- G0
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("S", [1, 5, 7, 8])
def test_gemm_fm_direct_exact_per_split(gpu, S, u8):
    """every split's slab is the product over that split's rows (the 32-row units of
    test_gemm_fm_direct_matches_fp32; 8 splits take the XCD-mapped block order)"""
    fx, n_valid, _, ref = _tile(fc.TILE_CASES[0])
    Bt, N, M = fx.Bp, 128, fx.K0
    Dg = ops.to_fragment_major(ref["delta1"].to(torch.bfloat16).cuda())
    Hg = ops.to_fragment_major((fx.X.to(torch.uint8) if u8 else fx.X.to(torch.bfloat16)).cuda())
    hscale = 0.5 if u8 else 1.0
    slab = ops.gemm_fm_direct(Dg, Hg, N, M, splits=S, hscale=hscale)
    torch.cuda.synchronize()
    slab = slab.cpu().double()
    U = Bt // 32
    for s in range(S):
        a, b = 32 * (s * U // S), 32 * ((s + 1) * U // S)
        assert torch.equal(slab[s], hscale * (ref["delta1"][a:b].t() @ fx.X[a:b])), s


# ------------------------------------------------------------------------------- one plan step
@functools.lru_cache(maxsize=None)
def _step(net):
    fx = fc.make_mlp3(net, 800, 4096, 10, u8=True, seed=fc.SEED, n_in=784)
    return fx, fc.reference(fx, fc.STEP_NVALID)


@pytest.mark.parametrize("net", ["LNN", "SNN"])
@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
def test_plan_step_exact(gpu, net, momentum):
    """front + fused (or separate) first-layer gradient + every layer's step: with n_valid, lr and
    alpha powers of two every product, sum and stepped weight is an FP32 number, so the split-K
    tickets, the fixed-order reduction and the tail workgroups' layer 1 / 2 steps must give the
    reference's bits in both forms"""
    _need_exact_zero(gpu)
    fx, ref = _step(net)
    new = fc.reference_step(fx, ref, fc.STEP_NVALID, fc.STEP_LR, fc.STEP_ALPHA, momentum)
    stream = torch.cuda.current_stream().cuda_stream
    for g0_fused in (True, False):
        m = MLP([784, 128, 64, 10], net, batch=4096, momentum=momentum, fused="t")
        assert m.fused_mode == "t" and tuple(m.W32[0].shape) == (128, 800)
        for l, W in enumerate((fx.W0, fx.W1, fx.W2)):
            m.W32[l].copy_(W.float())
        m.refresh_bf16()
        m.plan.g0_fused = g0_fused
        Xg = m.prepare_input(fx.X[:, :784].to(torch.uint8), pixel_scale=1.0)
        m.train_step(Xg, labels=fx.labels.cuda(), n_valid=fc.STEP_NVALID, lr=fc.STEP_LR, alpha=fc.STEP_ALPHA)
        torch.cuda.synchronize()
        assert m.plan.health(stream) == 0
        for l, (W32, V32, Wb) in enumerate(new):
            assert torch.equal(m.W32[l].cpu(), W32), (g0_fused, l)
            if momentum:
                assert torch.equal(m.V32[l].cpu(), V32), (g0_fused, l)
            assert torch.equal(m.Wb[l].cpu(), Wb) and torch.equal(m.Wt[l].cpu(), Wb.t()), (g0_fused, l)
        assert torch.equal(m.W0f.cpu().view(-1), ops.frag_major(new[0][2]).reshape(-1)), g0_fused
        loss, hits = m.read_stats()
        assert hits == ref["hits"]
        if net == "LNN":
            assert loss == ref["loss"]


# ------------------------------------------------------------------------------- metamorphic
def _random_op(kind, net="SNN", seed=7):
    g = torch.Generator().manual_seed(seed)
    K0, Bp, H = (4096, 256, 256) if kind == "wide" else (800, 512 if kind == "tile" else 96, 128)
    n_out = 230 if kind == "wide" else 10
    r = lambda *s: torch.rand(*s, generator=g) - 0.5  # noqa: E731
    op = dict(net=net, n_out=n_out, K0=K0, Bp=Bp, T=None)
    op["X"] = torch.randint(0, 256, (Bp, K0), generator=g, dtype=torch.uint8) if kind == "tile" else r(Bp, K0).bfloat16()
    op["W0"] = (r(H, K0) * (0.02 if kind == "tile" else 2.0) / K0 ** 0.5).bfloat16()
    if kind == "wide":
        op["W1"] = torch.zeros(256, H).bfloat16()
        op["W1"][:n_out] = (r(n_out, H) / 8).bfloat16()
    else:
        op["W1"] = (r(64, 128) / 4).bfloat16()
        op["W2"] = torch.zeros(32, 64).bfloat16()
        op["W2"][:n_out] = (r(n_out, 64) / 2).bfloat16()
    op["labels"] = torch.randint(0, n_out, (Bp,), generator=g, dtype=torch.int32)
    return op, g


def _run(kind, op, n_valid):
    op = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in op.items()}
    if kind == "tile":
        out = fc.run_tile(op, n_valid, 2)
        out["guess"] = fc.run_eval(op, n_valid, 2)["guess"]
        return out
    if kind == "fused":
        return fc.run_fused(op, n_valid, 2, False)
    out = fc.run_wide(op, n_valid, 2)
    out["ws"].check()
    return out


_META_KEYS = {"tile": ("delta1", "gslab", "guess"), "fused": ("delta1", "gslab"), "wide": ("delta2", "delta1")}


@pytest.mark.parametrize("kind", ["tile", "fused", "wide"])
def test_rows_past_n_valid_do_not_count(gpu, kind):
    """finite garbage in the samples from n_valid up leaves every output bit-equal to the run
    with those rows zeroed"""
    op, g = _random_op(kind)
    n_valid = op["Bp"] - 37
    zeroed, garbage = dict(op), dict(op)
    zeroed["X"] = op["X"].clone()
    zeroed["X"][n_valid:] = 0
    garbage["X"] = op["X"].clone()
    junk = torch.randint(0, 256, (op["Bp"] - n_valid, op["K0"]), generator=g)
    garbage["X"][n_valid:] = junk.to(torch.uint8) if kind == "tile" else (junk.float() - 100.0).bfloat16()
    garbage["labels"] = op["labels"].clone()
    garbage["labels"][n_valid:] = (op["labels"][n_valid:] + 3) % op["n_out"]
    a, b = _run(kind, zeroed, n_valid), _run(kind, garbage, n_valid)
    for k in _META_KEYS[kind]:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["stats"][:, :2], b["stats"][:, :2])
    if kind == "wide":
        assert torch.equal(a["H0"][:n_valid], b["H0"][:n_valid])


@pytest.mark.parametrize("kind", ["tile", "fused", "wide"])
def test_rows_permute_across_tiles(gpu, kind):
    """the samples and their labels permuted over the whole batch: the rows of delta1 (delta2,
    the guess) permute bit for bit and the hits are equal"""
    op, g = _random_op(kind)
    perm = torch.randperm(op["Bp"], generator=g)
    moved = dict(op)
    moved["X"], moved["labels"] = op["X"][perm].contiguous(), op["labels"][perm].contiguous()
    a, b = _run(kind, op, op["Bp"]), _run(kind, moved, op["Bp"])
    for k in _META_KEYS[kind]:
        if k != "gslab":
            assert torch.equal(a[k][perm], b[k]), k
    assert a["hits"] == b["hits"]
