"""The end of the fused first-layer-gradient launch (kernels_g0.hip), bit for bit.

Lazy copies: a fused G0 step of the tile path stores neither W0 / W0^T nor W1^T in BF16 (no
kernel of that step, nor hpnn_mlp3_eval, reads them); BPlan::sync_copies re-derives them for
every reader.  k-group meet: the four k-groups of a G0 workgroup hand their partial tiles over
in an LDS area each behind one barrier (grids of at most one workgroup per CU) or in rounds
through one area; same order of additions.  Every comparison is torch.equal on integer-exact
data (tests/front_exact_common.py) or between two forms of the same arithmetic."""
import functools

import pytest
import torch

from hpnn_amd import ops
from hpnn_amd.models import MLP
from tests import front_exact_common as fc

pytestmark = pytest.mark.gpu
STALE = 0x10001 | 0x20000  # Wb[0], Wt[0], Wt[1]


# ------------------------------------------------------------------------------- lazy copies
def _mnist(B, lazy=True, seed=3, splits=2):
    m = MLP([784, 128, 64, 10], "SNN", batch=B, momentum=True, fused="t", seed=seed, splits=[splits, 0, 0])
    assert m.fused_mode == "t" and m.S[0] == splits
    m.plan.lazy_copies = lazy
    return m


def _batches(m, n, seed=17):
    g = torch.Generator().manual_seed(seed)
    xs = [m.prepare_input(torch.randint(0, 256, (m.Bp, 784), generator=g, dtype=torch.uint8)) for _ in range(n)]
    labs = [torch.randint(0, 10, (m.Bp,), generator=g, dtype=torch.int32).cuda() for _ in range(n)]
    return xs, labs


def _steps(m, xs, labs):
    for X, lab in zip(xs, labs):
        m.train_step(X, labels=lab, lr=0.05, alpha=0.2)


def _assert_copies_current(m):
    for l in range(m.L):
        wb = m.W32[l].bfloat16()
        assert torch.equal(m.Wb[l], wb), l
        assert torch.equal(m.Wt[l], wb.t()), l
    assert torch.equal(m.W0f, ops.frag_major(m.W32[0].bfloat16()))


@functools.lru_cache(maxsize=None)
def _trained(lazy):
    """three momentum steps at 512 samples (two tiles, two splits): the smallest batch with more
    than one workgroup in both launches"""
    m = _mnist(512, lazy)
    xs, labs = _batches(m, 3)
    _steps(m, xs, labs)
    torch.cuda.synchronize()
    assert m.healthy()
    # the fused G0 launch ran, in its lazy form or not: only that launch marks copies stale
    assert m.plan.stale_copies == (STALE if lazy else 0)
    raw = m.buf[("Wb", 0)].clone()  # no accessor: W0 in BF16 as the steps left it
    return m, xs, labs, raw


def test_lazy_copies_stale_then_current(gpu):
    m, _, _, raw = _trained(True)
    assert not torch.equal(raw, m.W32[0].bfloat16()), "the steps stored W0 after all"
    assert torch.equal(_trained(False)[3], m.W32[0].bfloat16())
    _assert_copies_current(m)
    assert m.plan.stale_copies == 0  # eager steps: synced once


def test_lazy_steps_equal_eager_stores(gpu):
    a, b = _trained(True)[0], _trained(False)[0]
    assert a.weights_digest(3) == b.weights_digest(3)
    for l in range(3):
        assert torch.equal(a.W32[l], b.W32[l]) and torch.equal(a.V32[l], b.V32[l]), l
        assert torch.equal(a.Wb[l], b.Wb[l]) and torch.equal(a.Wt[l], b.Wt[l]), l
    assert torch.equal(a.W0f, b.W0f)


def test_lazy_state_round_trip(gpu):
    """the FP32 state of a lazily stepped model loaded into a fresh one: every copy equal, and the
    next step too"""
    a, xs, labs, _ = _trained(True)
    b = _mnist(512, True, seed=99)
    for l in range(3):
        b.W32[l].copy_(a.W32[l])
        b.V32[l].copy_(a.V32[l])
    b.refresh_bf16()
    for l in range(3):
        assert torch.equal(a.Wb[l], b.Wb[l]) and torch.equal(a.Wt[l], b.Wt[l]), l
    assert torch.equal(a.W0f, b.W0f)
    ca = _mnist(512, True, seed=99)  # a copy of a: the cached model stays as the other tests expect it
    for l in range(3):
        ca.W32[l].copy_(a.W32[l])
        ca.V32[l].copy_(a.V32[l])
    ca.refresh_bf16()
    _steps(ca, xs[:1], labs[:1])
    _steps(b, xs[:1], labs[:1])
    torch.cuda.synchronize()
    for l in range(3):
        assert torch.equal(ca.W32[l], b.W32[l]) and torch.equal(ca.V32[l], b.V32[l]), l


def test_lazy_copies_feed_per_layer_forward(gpu):
    """predict() runs the per-layer path on W0: after lazy steps it sees what a freshly refreshed
    plan sees"""
    m = _mnist(512, True)
    xs, labs = _batches(m, 3)
    _steps(m, xs, labs)
    assert m.plan.stale_copies == STALE
    out = m.predict(xs[0])  # straight after the steps, the copies still stale
    b = _mnist(512, False, seed=99)
    for l in range(3):
        b.W32[l].copy_(m.W32[l])
    b.refresh_bf16()
    want = b.predict(xs[0])
    torch.cuda.synchronize()
    assert torch.equal(out, want) and bool(out.abs().sum() > 0)


def test_lazy_steps_in_a_graph(gpu):
    """one captured step replayed twice after an eager one == three eager steps; the copies read
    after the replays are current, and again after one more replay"""
    e = _mnist(512, True)
    xs, labs = _batches(e, 1)
    _steps(e, xs * 3, labs * 3)
    g = _mnist(512, True)
    _steps(g, xs, labs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.train_step(xs[0], labels=labs[0], lr=0.05, alpha=0.2)
    w_before = g.W32[0].clone()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(w_before, g.W32[0])
    for l in range(3):
        assert torch.equal(e.W32[l], g.W32[l]) and torch.equal(e.V32[l], g.V32[l]), l
        assert torch.equal(e.Wb[l], g.Wb[l]) and torch.equal(e.Wt[l], g.Wt[l]), l
    graph.replay()  # the plan does not see a replay: the copies must count as stale still
    torch.cuda.synchronize()
    _assert_copies_current(g)
    assert g.healthy()


# ------------------------------------------------------------------------------- k-group meet
# (32-row k-steps, splits): k-steps per split 1 (groups 1..3 idle), 2, 3, 5, 6, uneven 2 / 3 over
# 12 splits (not a multiple of 8, XCD-mapped first 8), and 270 workgroups, more than the 256 CUs of
# an MI355X (the form with one LDS area)
MEET_CASES = [(12, 12), (12, 6), (12, 4), (10, 2), (12, 2), (30, 12), (54, 27)]


@pytest.mark.parametrize("u8", [False, True], ids=["bf16", "u8"])
@pytest.mark.parametrize("ksteps,S", MEET_CASES)
def test_gemm_fm_direct_meet_exact(gpu, ksteps, S, u8):
    """80 x 128 tiles (four k-groups): every split's slab is the exact integer product"""
    g = torch.Generator().manual_seed(100 * ksteps + S)
    Bt, N, M = 32 * ksteps, 128, 800
    D = torch.randint(-3, 4, (Bt, N), generator=g).double()
    H = torch.randint(0, 4, (Bt, M), generator=g).double()
    Dg = ops.to_fragment_major(D.to(torch.bfloat16).cuda())
    Hg = ops.to_fragment_major((H.to(torch.uint8) if u8 else H.to(torch.bfloat16)).cuda())
    hscale = 0.5 if u8 else 1.0
    slab = ops.gemm_fm_direct(Dg, Hg, N, M, splits=S, hscale=hscale)
    torch.cuda.synchronize()
    slab = slab.cpu().double()
    sizes = set()
    for s in range(S):
        a, b = 32 * (s * ksteps // S), 32 * ((s + 1) * ksteps // S)
        sizes.add((b - a) // 32)
        assert torch.equal(slab[s], hscale * (D[a:b].t() @ H[a:b])), s
    assert sizes <= {1, 2, 3, 5, 6}, sizes


@functools.lru_cache(maxsize=None)
def _exact_step():
    fx = fc.make_mlp3("LNN", 800, 512, 10, u8=True, seed=fc.SEED, n_in=784)
    ref = fc.reference(fx, 256)
    return fx, ref, fc.reference_step(fx, ref, 256, fc.STEP_LR, fc.STEP_ALPHA, True)


@pytest.mark.parametrize("u8", [False, True], ids=["bf16", "u8"])
@pytest.mark.parametrize("S", [16, 8, 5, 3])
def test_fused_update_equals_slab_form_exact(gpu, S, u8):
    """one whole step at 16 k-steps over S splits (1, 2, 3 or 4 and 5 or 6 k-steps each): the
    fused launch, the slab form and the FP64 reference agree bit for bit"""
    fx, ref, new = _exact_step()
    for g0_fused in (True, False):
        m = MLP([784, 128, 64, 10], "LNN", batch=512, momentum=True, fused="t", splits=[S, 0, 0])
        assert m.fused_mode == "t" and m.S[0] == S
        for l, W in enumerate((fx.W0, fx.W1, fx.W2)):
            m.W32[l].copy_(W.float())
        m.refresh_bf16()
        m.plan.g0_fused = g0_fused
        X = fx.X[:, :784]
        Xg = m.prepare_input(X.to(torch.uint8), pixel_scale=1.0) if u8 else m.prepare_input(X.float())
        assert Xg.dtype == (torch.uint8 if u8 else torch.bfloat16)
        m.train_step(Xg, labels=fx.labels.cuda(), n_valid=256, lr=fc.STEP_LR, alpha=fc.STEP_ALPHA)
        torch.cuda.synchronize()
        assert m.healthy()
        assert m.plan.stale_copies == (STALE if g0_fused else 0)
        for l, (W32, V32, Wb) in enumerate(new):
            assert torch.equal(m.W32[l].cpu(), W32) and torch.equal(m.V32[l].cpu(), V32), (g0_fused, l)
            assert torch.equal(m.Wb[l].cpu(), Wb) and torch.equal(m.Wt[l].cpu(), Wb.t()), (g0_fused, l)
        assert torch.equal(m.W0f.cpu().view(-1), ops.frag_major(new[0][2]).reshape(-1)), g0_fused
