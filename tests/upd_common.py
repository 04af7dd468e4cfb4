"""Helpers of the GPU tests of the update kernels (tests/test_adam_gpu.py, tests/test_lrsched_gpu.py):
segments inside sentinel-filled buffers, their device copies, and the BF16 plan's layer tuples."""
import torch


def ibits(t):
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype])


def window(values, off, tail=3):
    """values inside a NaN-filled buffer, `off` elements from its start"""
    base = torch.full((off + values.numel() + tail,), float("nan"), dtype=values.dtype)
    base[off:off + values.numel()] = values
    return base, base[off:off + values.numel()]


def slab_window(sl, goff):
    """the slabs sl [S, n] inside a NaN-filled buffer, `goff` elements from its start, rows n + 3
    apart (NaN between)"""
    S, n = sl.shape
    gs = n + 3
    base = torch.full((goff + S * gs + 1,), float("nan"), dtype=sl.dtype)
    slab = base[goff:goff + S * gs].view(S, gs)[:, :n]
    slab.copy_(sl)
    return base, slab


def to_cuda(seg, bases):
    """device copies of the buffers and the same windows into them"""
    dev, dbase = {}, {}
    for k, t in seg.items():
        dbase[k] = bases[k].cuda()
        dev[k] = dbase[k].as_strided(t.shape, t.stride(), t.storage_offset())
    return dev, dbase


def multi_dev(c, state):
    """the device tuple of one layer for adam_update_multi / sgd_sched_multi: W, the FP32 state
    arrays named in `state`, G, and BF16 W, W^T and (c["frag"]) Wf filled with 7"""
    N, K = c["W"].shape
    return (c["W"].cuda(),) + tuple(c[k].cuda() for k in state) + (
        c["G"].cuda(), torch.full((N, K), 7.0, dtype=torch.bfloat16, device="cuda"),
        torch.full((K, N), 7.0, dtype=torch.bfloat16, device="cuda"),
        torch.full((N * K,), 7.0, dtype=torch.bfloat16, device="cuda") if c["frag"] else None)
