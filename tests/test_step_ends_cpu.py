"""The host side of the lazy BF16 copies (BPlan::lazy_copies / stale_copies / sync_copies,
MLP.Wb / Wt): a plan that never ran the fused G0 launch has nothing stale, and the accessors of
the CPU emulation hand out the plan's buffers themselves."""
import torch

from hpnn_amd.models import MLP


def test_cpu_plan_has_no_stale_copies():
    m = MLP([784, 128, 64, 10], "SNN", batch=256, device="cpu", momentum=True, fused="t", seed=5)
    assert m.plan.lazy_copies is True and m.plan.stale_copies == 0
    m.plan.lazy_copies = False
    assert m.plan.lazy_copies is False
    m.sync_copies()  # nothing to launch
    for l in range(m.L):
        assert m.Wb[l] is m.buf[("Wb", l)] and m.Wt[l] is m.buf[("Wt", l)]
        assert torch.equal(m.Wb[l], m.W32[l].bfloat16()) and torch.equal(m.Wt[l], m.W32[l].bfloat16().t())
    X = m.prepare_input(torch.randint(0, 256, (256, 784), dtype=torch.uint8))
    m.train_step(X, labels=torch.randint(0, 10, (256,), dtype=torch.int32), lr=0.05, alpha=0.2)
    assert m.plan.stale_copies == 0
    for l in range(m.L):
        assert torch.equal(m.Wb[l], m.W32[l].bfloat16()) and torch.equal(m.Wt[l], m.W32[l].bfloat16().t())
