"""[shuffle] epoch on the CPU: the permutation of include/libhpnn/shuffle.h (against a
pure-Python transcription of its definition and fixed vectors), the conf key, train_nn -R on
the FP64 CPU batched engine against an independent FP64 PyTorch reference stepped over
X[order][perm_e], and exact resume across the epoch sequence."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi
from hpnn_amd.models import reference
from hpnn_amd.utils import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")

M32 = 0xFFFFFFFF
SIZES = [1, 2, 3, 5, 31, 32, 33, 255, 256, 257, 300, 600, 768, 1000, 4097]
SEEDS = [1, 9, 10958]
EPOCHS = range(8)


def _mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def py_perm(n, seed, epoch):
    """the definition, transcribed (32-bit unsigned arithmetic)"""
    if n <= 1:
        return list(range(n))
    bits = max(2, (n - 1).bit_length())
    hb = (bits + 1) // 2
    mask = (1 << hb) - 1
    key = [_mix(seed ^ _mix((epoch + 0x9E3779B9 * (r + 1)) & M32)) for r in range(4)]
    out = []
    for i in range(n):
        x = i
        while True:
            L, R = x >> hb, x & mask
            for r in range(4):
                L, R = R, L ^ (_mix(R ^ key[r]) & mask)
            x = (L << hb) | R
            if x < n:
                break
        out.append(x)
    return out


def test_epoch_perm_vectors_and_transcription():
    vec = {(10, 7, 0): [8, 0, 1, 2, 4, 7, 3, 9, 6, 5],
           (10, 7, 1): [7, 8, 5, 9, 3, 1, 4, 0, 6, 2],
           (10, 8, 0): [8, 1, 3, 4, 9, 7, 2, 5, 0, 6]}
    for (n, seed, ep), want in vec.items():
        assert py_perm(n, seed, ep) == want
        assert capi.hpnn_epoch_perm(n, seed, ep).tolist() == want
    for n in (1, 2, 3, 33, 257, 1000):
        for ep in (0, 5):
            assert capi.hpnn_epoch_perm(n, 10958, ep).tolist() == py_perm(n, 10958, ep)


@pytest.mark.parametrize("n", SIZES)
def test_epoch_perm_is_a_bijection_that_moves(n):
    for seed in SEEDS:
        perms = [capi.hpnn_epoch_perm(n, seed, e) for e in EPOCHS]
        for p in perms:
            assert np.array_equal(np.sort(p), np.arange(n, dtype=np.uint32)), (n, seed)
        if n < 255:
            continue
        ident = np.arange(n, dtype=np.uint32)
        for e, p in enumerate(perms):
            assert int((p == ident).sum()) <= 8, (n, seed, e)
            if e:
                assert int((p == perms[e - 1]).sum()) <= 8, (n, seed, e)


def test_conf_shuffle_round_trip(tmp_path):
    d = str(tmp_path)
    kw = dict(name="s", type="SNN", seed=3, inputs=6, hiddens=[4], outputs=3, train="BP", sample_dir="./s",
              test_dir="./s", mode="batched")
    capi.init(0)
    formats.write_conf(os.path.join(d, "a.conf"), shuffle="Epoch", **kw)
    net = capi.Network(os.path.join(d, "a.conf"))
    assert net.shuffle == "epoch"
    net.dump_conf(os.path.join(d, "a2.conf"))
    net.close()
    assert "[shuffle] epoch\n" in open(os.path.join(d, "a2.conf")).read()
    net = capi.Network(os.path.join(d, "a2.conf"))
    assert net.shuffle == "epoch"
    net.set(shuffle="once")
    assert net.shuffle == "once"
    net.close()
    formats.write_conf(os.path.join(d, "b.conf"), **kw)
    net = capi.Network(os.path.join(d, "b.conf"))
    assert net.shuffle == "once"
    net.dump_conf(os.path.join(d, "b2.conf"))
    net.set(shuffle="epoch")
    assert net.shuffle == "epoch"
    net.close()
    assert "shuffle" not in open(os.path.join(d, "b2.conf")).read()
    formats.write_conf(os.path.join(d, "c.conf"), shuffle="bogus", **kw)
    with pytest.raises(RuntimeError):
        capi.Network(os.path.join(d, "c.conf"))


def _order(n, seed):
    """nn_train_kernel's seeded sample order (the helper of tests/test_bplan_gpu.py)"""
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.random.restype = ctypes.c_long
    libc.srandom(ctypes.c_uint(seed))
    used, order = set(), []
    while len(order) < n:
        idx = int(float(libc.random()) * n / 2147483647.0)
        if idx >= n or idx in used:
            continue
        used.add(idx)
        order.append(idx)
    return order


N, N_IN, HID, N_OUT, B, SEED, LR = 70, 20, [12], 5, 32, 11, 0.05


def _dataset(d):
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (N, N_IN))
    T = np.zeros((N, N_OUT))
    T[np.arange(N), rng.integers(0, N_OUT, N)] = 1.0
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    return X, T


def _conf(d, epochs, **extra):
    formats.write_conf(os.path.join(d, "nn.conf"), name="s", type="SNN", seed=SEED, inputs=N_IN, hiddens=HID,
                       outputs=N_OUT, train="BPM", sample_dir="./train.hpnb", test_dir="./train.hpnb",
                       mode="batched", batch=B, epochs=epochs, lr=LR, dtype="f64", **extra)


def _train(d, *flags):
    env = dict(os.environ, HPNN_KERNEL_EXACT="1")
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-c", "-vv", *flags, "nn.conf"], cwd=d, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _weights(d, name):
    return formats.read_kernel(os.path.join(d, name))["weights"]


def test_train_nn_reshuffle_matches_reference(tmp_path):
    epochs = 3
    runs = {}
    for tag, flags, extra in (("flag", ("-R",), {}), ("conf", (), {"shuffle": "epoch"}), ("once", (), {})):
        d = str(tmp_path / tag)
        os.makedirs(d)
        X, T = _dataset(d)
        _conf(d, epochs, **extra)
        out = _train(d, *flags)
        assert ("reshuffled every epoch" in out) == (tag != "once"), out[-2000:]
        runs[tag] = (_weights(d, "kernel.tmp"), _weights(d, "kernel.opt"))
    w0 = runs["flag"][0]
    for a, b in zip(runs["flag"][1], runs["conf"][1]):
        assert np.array_equal(a, b)
    assert any(not np.array_equal(a, b) for a, b in zip(runs["flag"][1], runs["once"][1]))

    # independent reference: FP64 PyTorch steps over X[order][perm_e]
    order = _order(N, SEED)
    Xo, To = torch.tensor(X[order]), torch.tensor(T[order])
    W = [torch.tensor(w) for w in w0]
    V = [torch.zeros_like(w) for w in W]
    for e in range(epochs):
        perm = torch.tensor(py_perm(N, SEED, e))
        Xe, Te = Xo[perm], To[perm]
        for s in range(0, N, B):
            reference.batched_step(W, Xe[s:s + B], Te[s:s + B], "SNN", LR, momentum=V, alpha=0.2)
    for a, got, ref in zip(w0, runs["flag"][1], W):
        dc, dg = ref.numpy() - a, got - a
        rel = np.linalg.norm(dc - dg) / (np.linalg.norm(dc) + 1e-300)
        print("relative error of the weight change:", rel)
        assert rel <= 1e-12, rel


def test_reshuffle_resume_continues_the_sequence(tmp_path):
    d4, d22 = str(tmp_path / "four"), str(tmp_path / "two_two")
    for d in (d4, d22):
        os.makedirs(d)
        _dataset(d)
    _conf(d4, 4)
    _train(d4, "-R")
    _conf(d22, 2)
    _train(d22, "-R", "-r", "state.bin")
    _train(d22, "-R", "-r", "state.bin")
    assert open(os.path.join(d4, "kernel.opt")).read() == open(os.path.join(d22, "kernel.opt")).read()


def test_ops_cpu_emulation():
    """the CPU forms of the ops (torch indexing + to_fragment_major), as every op has"""
    from hpnn_amd import ops
    perm = ops.epoch_perm(10, 7, 1, "cpu")
    assert perm.dtype == torch.int32 and perm.tolist() == [7, 8, 5, 9, 3, 1, 4, 0, 6, 2]
    src = torch.arange(10 * 32, dtype=torch.float32).view(10, 32)
    out = torch.full((32, 32), -1.0)
    ops.gather_rows(src, perm, out)
    assert torch.equal(out[:10], src[perm.long()]) and int(out[10:].count_nonzero()) == 0
    b = (src % 251).to(torch.uint8)
    fm = torch.full((1, 2, 64, 8), 255, dtype=torch.uint8)
    ops.gather_fragment_major(b, perm, fm)
    pad = torch.zeros(32, 32, dtype=torch.uint8)
    pad[:10] = b[perm.long()]
    assert torch.equal(ops.from_fragment_major(fm, 32, 32), pad)
