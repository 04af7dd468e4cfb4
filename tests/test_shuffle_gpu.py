"""[shuffle] epoch on the GPU (csrc/gpu/kernels_shuffle.hip and the single-device batched
engines): the gather kernels against torch indexing (bitwise), the device permutation against
the host's with the in-graph epoch word, train_nn's FP64 / FP32 engines against the CPU oracle,
the BF16 engine against the Python plan stepped over host-indexed batches (bitwise, every plan
mode), MLP.gather_input, and the refusal of the multi-replica engines."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP
from hpnn_amd.utils import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")

SIZES = [1, 2, 3, 5, 31, 32, 33, 255, 256, 257, 300, 600, 768, 1000, 4097]


def _bits(t):
    """a tensor's bytes (bitwise comparisons of any dtype, NaN patterns included)"""
    return t.contiguous().view(-1).view(torch.uint8)


def _rand(shape, dtype, gen):
    """random bit patterns of the dtype"""
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen)
    return raw.view(dtype).view(*shape).cuda()


def _pad(v, m):
    return (v + m - 1) // m * m


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,cols", [(torch.int32, 1), (torch.float32, 10), (torch.bfloat16, 32),
                                        (torch.bfloat16, 4096), (torch.float64, 784)])
def test_gather_rows_matches_index_select(gpu, dtype, cols):
    gen = torch.Generator().manual_seed(cols)
    for n in (1, 33, 257):
        rows_p = _pad(n, 128)
        src = _rand((n, cols), dtype, gen)
        perm = torch.randperm(n, generator=gen).to(torch.int32).cuda()
        out = torch.full((rows_p * cols * src.element_size(),), 0xFF, dtype=torch.uint8, device="cuda")
        out = out.view(dtype).view(rows_p, cols)
        ops.gather_rows(src, perm, out)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[:n]), _bits(src.index_select(0, perm.long()))), (n, cols)
        assert int(_bits(out[n:]).count_nonzero()) == 0, (n, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,Kp", [(torch.uint8, 32), (torch.uint8, 256), (torch.uint8, 800),
                                      (torch.bfloat16, 32), (torch.bfloat16, 256), (torch.bfloat16, 800),
                                      (torch.bfloat16, 4096)])
def test_gather_fragment_major_matches_torch(gpu, dtype, Kp):
    gen = torch.Generator().manual_seed(Kp)
    for n in (1, 31, 32, 33, 300):
        src = _rand((n, Kp), dtype, gen)
        perm = torch.randperm(n, generator=gen).to(torch.int32).cuda()
        for rows_p in sorted({_pad(n, 32), _pad(n, 256)}):
            out = torch.full((rows_p * Kp * src.element_size(),), 0xFF, dtype=torch.uint8, device="cuda")
            out = out.view(dtype).view(rows_p // 32, Kp // 16, 64, 8)
            ops.gather_fragment_major(src, perm, out)
            torch.cuda.synchronize()
            padded = torch.zeros(rows_p, Kp, dtype=dtype, device="cuda")
            padded[:n] = src[perm.long()]
            assert torch.equal(_bits(out), _bits(ops.to_fragment_major(padded))), (n, rows_p, Kp)


@pytest.mark.gpu
def test_device_permutation_and_epoch_word(gpu):
    seed, e0 = 10958, 5
    warm = torch.tensor([0], dtype=torch.int32, device="cuda")
    ops.epoch_perm(4, seed, warm, "cuda", advance=True)  # code object loaded before any capture
    torch.cuda.synchronize()
    assert int(warm.item()) == 1
    for n in SIZES:
        word = torch.tensor([e0], dtype=torch.int32, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        P = torch.full((2, n), -1, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # two epochs' launches on the one capture stream
            for i in range(2):
                ops.epoch_perm(n, seed, word, "cuda", out=P[i], err=err, advance=True)
        for rep in range(2):
            g.replay()
            torch.cuda.synchronize()
            for i in range(2):
                want = capi.hpnn_epoch_perm(n, seed, e0 + 2 * rep + i).astype(np.int32)
                assert np.array_equal(P[i].cpu().numpy(), want), (n, rep, i)
        assert int(word.item()) == e0 + 4 and int(err.item()) == 0, n
        # an integer epoch (no word) gives the same permutation
        assert np.array_equal(ops.epoch_perm(n, seed, e0, "cuda").cpu().numpy(),
                              capi.hpnn_epoch_perm(n, seed, e0).astype(np.int32))


def _run(cmd, cwd, cpu=False, extra_env=None, check=True):
    env = dict(os.environ)
    env.pop("HPNN_FORCE_CPU", None)
    if cpu:
        env["HPNN_FORCE_CPU"] = "1"
    env.update(extra_env or {})
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def _fp_case(d, net, dims, dtype):
    n_in, hid, n_out = dims
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, (300, n_in))
    T = np.full((300, n_out), 0.0 if net == "SNN" else -1.0)
    T[np.arange(300), rng.integers(0, n_out, 300)] = 1.0
    os.makedirs(d, exist_ok=True)
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    formats.write_conf(os.path.join(d, "nn.conf"), name="fp", type=net, seed=9, inputs=n_in, hiddens=hid,
                       outputs=n_out, train="BPM", sample_dir="./train.hpnb", test_dir="./train.hpnb",
                       mode="batched", batch=128, epochs=2, lr=0.05, dtype=dtype, shuffle="epoch")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-12), ("f32", 1e-4)])
@pytest.mark.parametrize("net,dims", [("SNN", (784, [128, 64], 10)), ("LNN", (33, [17], 5))])
def test_train_nn_fp_reshuffle_matches_cpu_oracle(tmp_path, gpu, dtype, tol, net, dims):
    res = {}
    runs = [("cpu", True, {}), ("gpu", False, {})] + ([("eager", False, {"HPNN_GRAPH": "0"})] if dtype == "f64" else [])
    for tag, cpu, env in runs:
        d = str(tmp_path / tag)
        _fp_case(d, net, dims, dtype)
        out = _run([os.path.join(BIN, "train_nn"), "-vv", "nn.conf"], d, cpu=cpu,
                   extra_env={"HPNN_KERNEL_EXACT": "1", **env}).stdout
        assert "reshuffled every epoch" in out, out[-2000:]
        if not cpu:
            assert f"batched GPU training: {dtype}" in out, out[-2000:]
        res[tag] = (formats.read_kernel(os.path.join(d, "kernel.tmp"))["weights"],
                    formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"],
                    open(os.path.join(d, "kernel.opt")).read())
    for w0, wc, wg in zip(res["cpu"][0], res["cpu"][1], res["gpu"][1]):
        dc, dg = wc - w0, wg - w0
        rel = np.linalg.norm(dc - dg) / (np.linalg.norm(dc) + 1e-300)
        print(f"{net} {dtype}: relative error of the weight change {rel:.3e}")
        assert rel <= tol, rel
    if dtype == "f64":
        assert res["eager"][2] == res["gpu"][2]


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


@pytest.mark.gpu
@pytest.mark.parametrize("net,train,dims,B,pixels,mode", [
    ("SNN", "BPM", (784, [128, 64], 10), 256, True, "t"),     # tile front, 8-bit input
    ("SNN", "BPM", (784, [128, 64], 10), 384, True, "x"),     # pipelined front + byte copy for G0
    ("SNN", "BPM", (4096, [230], 230), 256, False, "w"),      # wide front
    ("ANN", "BP", (100, [64, 48], 7), 128, False, None),      # per-layer kernels
    ("SNN", "BPM", (784, [128, 64], 10), 256, False, "t"),    # tile front, BF16 fragment-major input
])
def test_train_nn_bf16_reshuffle_equals_python_plan(tmp_path, gpu, net, train, dims, B, pixels, mode):
    n_in, hid, n_out = dims
    n, seed, epochs = 3 * B, 11, 2
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (n, n_in)).astype(np.float64) if pixels else rng.uniform(-1, 1, (n, n_in))
    lab = rng.integers(0, n_out, n)
    T = np.full((n, n_out), 0.0 if net == "SNN" else -1.0)
    T[np.arange(n), lab] = 1.0
    d = str(tmp_path)
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    formats.write_conf(os.path.join(d, "nn.conf"), name="t", type=net, seed=seed, inputs=n_in, hiddens=hid,
                       outputs=n_out, train=train, sample_dir="./train.hpnb", test_dir="./train.hpnb",
                       mode="batched", batch=B, epochs=epochs, dtype="bf16", lr=0.01, shuffle="epoch")
    r = _run([os.path.join(BIN, "train_nn"), "-vvv", "nn.conf"], d)
    assert f"batched plan: mode {mode or '-'}" in r.stdout, r.stdout[-3000:]
    assert "reshuffled every epoch" in r.stdout, r.stdout[-3000:]
    got = formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"]

    m = MLP([n_in] + hid + [n_out], net, batch=B, momentum=train == "BPM", seed=seed)
    assert m.fused_mode == mode
    order = _order(n, seed)
    Xo, To = X[order], T[order]
    for e in range(epochs):
        perm = capi.hpnn_epoch_perm(n, seed, e).astype(np.int64)
        Xe, Te = Xo[perm], To[perm]  # host indexing: independent of the gather kernels
        for s in range(3):
            xb = torch.tensor(Xe[s * B:(s + 1) * B])
            xb = xb.to(torch.uint8) if pixels else xb
            Xp = m.prepare_input(xb, pixel_scale=1.0)
            Tt = torch.tensor(Te[s * B:(s + 1) * B], dtype=torch.float32, device="cuda")
            Tt = torch.cat([Tt, torch.zeros(m.Bp - B, n_out, device="cuda")]) if m.Bp > B else Tt
            m.train_step(Xp, T=Tt.contiguous(), n_valid=B, lr=0.01, alpha=0.2 if train == "BPM" else 0.0)
    torch.cuda.synchronize()
    for a, w in zip(got, m.W32):
        ref = w[:a.shape[0], :a.shape[1]].double().cpu().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), ref), np.abs(a - ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("dims,mode,u8", [((784, [128, 64], 10), "t", True), ((4096, [230], 230), "w", False)])
def test_mlp_gather_input_equals_prepare_input(gpu, dims, mode, u8):
    n_in, hid, n_out = dims
    m = MLP([n_in] + hid + [n_out], "SNN", batch=256, momentum=True, seed=3)
    assert m.fused_mode == mode
    gen = torch.Generator().manual_seed(7)
    n = 300
    X = (torch.randint(0, 256, (n, n_in), dtype=torch.uint8, generator=gen) if u8
         else torch.rand(n, n_in, generator=gen) * 2 - 1).cuda()
    perm = torch.randperm(n, generator=gen).to(torch.int32).cuda()
    want = m.prepare_input(X[perm.long()])
    rows = m.canonical_rows(X)
    for src in (rows, X):  # the resident canonical set, or the raw rows
        got = m.gather_input(src, perm)
        torch.cuda.synchronize()
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(_bits(got), _bits(want))
        assert getattr(got, "hpnn_fm_scale", None) == getattr(want, "hpnn_fm_scale", None)


@pytest.mark.gpu
def test_multi_replica_engines_refuse_reshuffle(tmp_path, gpu):
    d = str(tmp_path)
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, (256, 20))
    T = np.zeros((256, 4))
    T[np.arange(256), rng.integers(0, 4, 256)] = 1.0
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    formats.write_conf(os.path.join(d, "nn.conf"), name="r", type="SNN", seed=3, inputs=20, hiddens=[16], outputs=4,
                       train="BP", sample_dir="./train.hpnb", test_dir="./train.hpnb", mode="batched", batch=128,
                       epochs=2, dtype="f32", shuffle="epoch")
    r = _run([os.path.join(BIN, "train_nn"), "-v", "nn.conf"], d, extra_env={"HPNN_LOOPBACK_RANKS": "2"}, check=False)
    assert r.returncode != 0
    assert "[shuffle] epoch is not supported" in r.stdout + r.stderr
