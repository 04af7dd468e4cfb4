"""[train] ADAM on the CPU: the rule of include/libhpnn/adam.h (host form and the PyTorch
reference) against torch.optim.Adam / AdamW, the advance, the rounding bounds of
tests/adam_common.py, the FP64 CPU engine against the reference, the conf keys and the C API, the
state file, [keep_best] and the CPU emulation of the BF16 plan."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP, reference
from hpnn_amd.utils import formats
from tests import adam_common as A

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]


def _ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _host_run(w0, grads, dtype, decay, lr=0.01):
    """the host form (ops on CPU tensors): advance + update per step"""
    w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    st = ops.adam_state(lr=lr, decay=decay)
    for g in grads:
        tb = ops.AdamTable([dict(w=w, m=m, v=v, slab=g.view(1, -1))])
        ops.adam_advance(st)
        ops.adam_update_fp(tb, st, 1.0)
    return w, m, v, st


def _ref_run(w0, grads, dtype, decay, lr=0.01):
    w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    st = reference.adam_new_state(lr=lr, decay=decay)
    for g in grads:
        reference.adam_step(w, m, v, g, st)
    return w, m, v, st


def _torch_run(w0, grads, decay, lr=0.01):
    p = torch.nn.Parameter(w0.clone())
    opt = (torch.optim.AdamW([p], lr=lr, weight_decay=decay, maximize=True) if decay else
           torch.optim.Adam([p], lr=lr, maximize=True))
    for g in grads:
        p.grad = g.clone()
        opt.step()
    return p.detach()


# ------------------------------------------------------------------ 1. the rule against torch
@pytest.mark.parametrize("decay", [0.0, 0.01])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rule_matches_torch_adam(dtype, decay):
    n, steps, zeros = 1000, 50, 17
    grads = A.gradients(n, steps, 3, dtype, zeros=zeros)
    w0 = torch.randn(n, generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(dtype)
    want = _torch_run(w0, grads, decay)
    eps_t = torch.finfo(dtype).eps
    bound = steps * 4 * eps_t * max(1.0, float(want.abs().max()))
    for name, run in (("host form", _host_run), ("reference.adam_step", _ref_run)):
        w, m, v, _ = run(w0, grads, dtype, decay)
        err = float((w.double() - want.double()).abs().max())
        print(f"{name} {dtype} decay {decay}: |w - torch| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound, name
        if decay == 0.0:  # a gradient that is always 0 changes nothing, bit for bit
            assert torch.equal(_ibits(w[-zeros:]), _ibits(w0[-zeros:])), name
            assert not m[-zeros:].any() and not v[-zeros:].any()
        assert not torch.equal(w[:-zeros], w0[:-zeros])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_host_form_and_reference_agree_to_rounding(dtype):
    grads = A.gradients(257, 5, 8, dtype)
    w0 = torch.randn(257, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype)
    a, b = _host_run(w0, grads, dtype, 0.01), _ref_run(w0, grads, dtype, 0.01)
    # the same operations in the same order and type: the same bits
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(_ibits(x), _ibits(y))


# ------------------------------------------------------------------ 2. advance
@pytest.mark.parametrize("calls", [1, 2, 1000])
def test_advance_is_the_written_out_products(calls):
    lr, b1, b2, eps, decay = 0.003, 0.9, 0.999, 1e-8, 0.01
    st = ops.adam_state(lr, b1, b2, eps, decay)
    p1 = p2 = 1.0
    for _ in range(calls):
        ops.adam_advance(st)
        p1 *= b1
        p2 *= b2
    r = ops.read_adam_state(st)
    assert r["t"] == calls
    pk = lambda x: struct.pack("<d", x)  # noqa: E731
    assert pk(r["p1"]) == pk(p1) and pk(r["p2"]) == pk(p2)
    assert pk(r["c1"]) == pk(lr / (1.0 - p1)) and pk(r["s2"]) == pk(math.sqrt(1.0 - p2)) and pk(r["wd"]) == pk(lr * decay)
    assert (r["lr"], r["beta1"], r["beta2"], r["eps"], r["decay"]) == (lr, b1, b2, eps, decay)


def test_adam_state_refuses_bad_coefficients():
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(eps=0.0), dict(decay=-1.0)):
        with pytest.raises(ValueError):
            ops.adam_state(**kw)


# ------------------------------------------------------------------ the bounds of adam_common
def _one_step(dtype, S, t, decay, seed, big=False):
    g = torch.Generator().manual_seed(seed)
    n = 1000
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    m = (0.1 * torch.randn(n, generator=g, dtype=torch.float64)).to(dtype)
    v = (0.01 * torch.rand(n, generator=g, dtype=torch.float64)).to(dtype)
    scale = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 6.0 - 4.0)
    slabs = (scale * torch.randn(S, n, generator=g, dtype=torch.float64)).to(dtype)
    slabs[:, :5] = 0.0
    m[:5] = 0.0
    v[:5] = 0.0
    if big:
        slabs[0, 5:9] = 1e30
    st = ops.adam_state(lr=0.01, decay=decay)
    for _ in range(t):
        ops.adam_advance(st)
    return w, m, v, slabs, st


@pytest.mark.parametrize("decay", [0.0, 0.01])
@pytest.mark.parametrize("S,t", [(1, 1), (3, 1000)])
def test_bounds_hold_for_the_fp32_host_form_and_catch_a_perturbation(S, t, decay):
    dtype = torch.float32
    w, m, v, slabs, st = _one_step(dtype, S, t, decay, 11 + S, big=True)
    w1, m1, v1 = w.clone(), m.clone(), v.clone()
    ops.adam_update_fp(ops.AdamTable([dict(w=w1, m=m1, v=v1, slab=slabs)]), st, 1.0 / 7)
    sd = ops.read_adam_state(st)
    ratios = A.check_update(w, m, v, slabs, 1.0 / 7, sd, w1, m1, v1, dtype, "host f32")
    print(f"S {S} t {t} decay {decay}: error / bound of m, v, w = {ratios}")
    assert torch.isinf(v1[5:9]).all() and torch.equal(_ibits(w1[:5]), _ibits(w[:5])) is (decay == 0.0)
    # a value 100 bounds away fails each check
    m_ref, mb, v_ref, vb = A.bounds(w, m, v, slabs, 1.0 / 7, sd, dtype)
    _, step = A.w_ref(w, m1, v1, sd)
    wb = A.w_bound(w, step, dtype)
    i = 100
    for which, bd in (("m", mb), ("v", vb), ("w", wb)):
        bad = dict(m=m1.clone(), v=v1.clone(), w=w1.clone())
        bad[which][i] = (bad[which][i].double() + 100.0 * bd[i] + 2.0 ** -140).to(dtype)
        if which != "w":  # keep w consistent with the perturbed moment: only that moment is wrong
            bad["w"] = A.w_ref(w, bad["m"], bad["v"], sd)[0].to(dtype)
        with pytest.raises(AssertionError):
            A.check_update(w, m, v, slabs, 1.0 / 7, sd, bad["w"], bad["m"], bad["v"], dtype)


# ------------------------------------------------------------------ 3. the CPU engine against the reference
@pytest.mark.parametrize("net,net_type", A.CASES)
def test_cpu_engine_matches_the_reference(tmp_path, net, net_type):
    d = str(tmp_path)
    X, T, _, _ = A.make_data(d, net, net_type)
    A.write_conf(d, net, net_type)
    B = A.NETS[net]["B"]
    got = A.train(d, "cpu")
    assert got["ok"] and got["epochs_done"] == A.EPOCHS
    W, M, V = A.reference_run(got["w0"], X, T, net_type, B)
    tol = 100.0 * A.order_spread(got["w0"], X, T, net_type, B)
    err = A.spread(got["w"], W)
    print(f"{net} {net_type}: order spread {tol / 100:.3g}, engine - reference {err:.3g}")
    assert tol > 0.0 and err <= tol
    assert A.spread(got["w"], got["w0"]) > 10 * A.LR  # it trained: every step moves a weight by about lr
    st = got["state"]
    steps = A.EPOCHS * math.ceil(A.NETS[net]["n"] / B)
    assert st["has_adam"] == 1 and st["t"] == steps
    assert A.spread(st["dW"], M) <= tol and A.spread(st["V"], V) <= tol


# ------------------------------------------------------------------ 4. conf and API
def _conf(d, **extra):
    A.make_data(d, "8-6-4", "SNN")
    A.write_conf(d, "8-6-4", "SNN", **extra)
    capi.init(0)
    return capi.Network(os.path.join(d, "nn.conf"))


def test_conf_keys_round_trip(tmp_path):
    d = str(tmp_path)
    net = _conf(d, beta1=0.8, beta2=0.99, epsilon=1e-6, decay=0.02)
    assert net.L.nn_return_train(net.ptr) == capi.NN_TRAIN["ADAM"] == 4
    assert net.adam == dict(beta1=0.8, beta2=0.99, epsilon=1e-6, decay=0.02)
    net.dump_conf(os.path.join(d, "out.conf"))
    c = formats.read_conf(os.path.join(d, "out.conf"))
    assert c["train"] == "ADAM"
    assert (float(c["beta1"]), float(c["beta2"]), float(c["epsilon"]), float(c["decay"])) == (0.8, 0.99, 1e-6, 0.02)
    assert float(c["lr"]) == A.LR
    net.close()
    # the dumped file parses to the same values; [batch] is still [batch]
    net = capi.Network(os.path.join(d, "out.conf"))
    assert net.adam == dict(beta1=0.8, beta2=0.99, epsilon=1e-6, decay=0.02)
    assert net.L.nn_return_batch(net.ptr) == 32
    net.close()


def test_defaults_and_keys_dumped_only_when_set(tmp_path):
    d = str(tmp_path)
    net = _conf(d)
    assert net.adam == dict(beta1=0.9, beta2=0.999, epsilon=1e-8, decay=0.0)
    net.dump_conf(os.path.join(d, "out.conf"))
    txt = open(os.path.join(d, "out.conf")).read()
    assert not any(k in txt for k in ("[beta1]", "[beta2]", "[epsilon]", "[decay]"))
    net.set(adam=dict(decay=0.5))
    assert net.adam == dict(beta1=0.9, beta2=0.999, epsilon=1e-8, decay=0.5)
    net.close()


@pytest.mark.parametrize("key,val", [("beta1", "1.0"), ("beta1", "-0.5"), ("beta2", "1.5"), ("epsilon", "0"),
                                     ("epsilon", "-1e-8"), ("decay", "-0.1"), ("beta2", "x")])
def test_conf_range_errors(tmp_path, capfd, key, val):
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "SNN")
    A.write_conf(d, "8-6-4", "SNN", **{key: val})
    capi.init(0)
    with pytest.raises(RuntimeError):
        capi.Network(os.path.join(d, "nn.conf"))
    assert f"[{key}] value" in capfd.readouterr().err


@pytest.mark.parametrize("bad", [dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(epsilon=0.0),
                                 dict(decay=-0.5)])
def test_api_range_errors_at_train(tmp_path, capfd, bad):
    d = str(tmp_path)
    net = _conf(d)
    net.set(device="cpu", adam=bad)
    w0 = A.weights_of(net, d, "a.opt")
    assert not net.train()
    assert "out of range" in capfd.readouterr().err
    assert all(np.array_equal(a, b) for a, b in zip(w0, A.weights_of(net, d, "b.opt")))
    net.close()


def test_lr_default_and_momentum_message(tmp_path, capfd):
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "SNN")
    f = A.NETS["8-6-4"]
    formats.write_conf(os.path.join(d, "nn.conf"), name="adam", type="SNN", seed=A.SEED, inputs=8, hiddens=[6],
                       outputs=4, train="ADAM", sample_dir=os.path.join(d, "train.hpnb"),
                       test_dir=os.path.join(d, "val.hpnb"), mode="batched", batch=f["B"], epochs=1, momentum=0.3)
    capi.init(2)  # NN_OUT lines are printed from verbosity 2
    try:
        net = capi.Network(os.path.join(d, "nn.conf"))
        net.set(device="cpu")
        assert net.train()
        net.dump_state(os.path.join(d, "s.bin"))
        net.close()
    finally:
        capi.init(0)
    capi._LIBC.fflush(None)  # the library prints through C stdio
    out = capfd.readouterr()
    assert (out.out + out.err).count("[momentum] is unused") == 1
    # one step of the first minibatch with lr = 0.001 moves every weight with a gradient by ~0.001
    st = A.read_state(os.path.join(d, "s.bin"))
    assert st["t"] == math.ceil(f["n"] / f["B"])
    X, T, _, _ = A.make_data(d, "8-6-4", "SNN")
    capi.init(0)
    net = capi.Network(os.path.join(d, "nn.conf"))
    w0 = A.weights_of(net, d, "a.opt")
    net.close()
    W, _, _ = A.reference_run(w0, X, T, "SNN", f["B"], epochs=1, lr=0.001)
    assert A.spread(st["W"], W) <= 1e-12


def test_online_mode_is_refused(tmp_path, capfd):
    d = str(tmp_path)
    net = _conf(d, mode="online")
    net.set(device="cpu")
    w0 = A.weights_of(net, d, "a.opt")
    assert not net.train()
    assert "[train] ADAM needs [mode] batched" in capfd.readouterr().err
    assert all(np.array_equal(a, b) for a, b in zip(w0, A.weights_of(net, d, "b.opt")))
    net.close()


# ------------------------------------------------------------------ 5. the state file
def test_resume_through_the_state_file_is_exact(tmp_path):
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "ANN")
    A.write_conf(d, "8-6-4", "ANN", epochs=7, decay=0.01, shuffle="epoch")
    whole = A.train(d, "cpu")
    A.write_conf(d, "8-6-4", "ANN", epochs=3, decay=0.01, shuffle="epoch")
    A.train(d, "cpu", dump="three.bin")
    A.write_conf(d, "8-6-4", "ANN", epochs=4, decay=0.01, shuffle="epoch")
    rest = A.train(d, "cpu", load="three.bin")
    assert whole["ok"] and rest["ok"] and rest["epochs_done"] == 7
    assert A.state_bits(rest["state"]) == A.state_bits(whole["state"])
    assert whole["state"]["t"] == 7 * 4 and whole["state"]["p1"] == _pow(0.9, 28) and whole["state"]["p2"] == _pow(0.999, 28)


def _pow(b, k):
    p = 1.0
    for _ in range(k):
        p *= b
    return p


def test_bpm_state_file_keeps_the_parents_layout(tmp_path):
    """magic, u32 type train L has_momentum, dims, u32 seed epochs_done 0 0, u64 samples_seen, W, dW,
    checksum -- byte for byte, also when an ADAM run left its moments in the kernel before"""
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "SNN")
    A.write_conf(d, "8-6-4", "SNN", train="BPM", epochs=2)
    capi.init(0)
    net = capi.Network(os.path.join(d, "nn.conf"))
    net.set(device="cpu")
    net.L.nn_set_train(net.ptr, capi.NN_TRAIN["ADAM"])
    assert net.train()
    net.L.nn_set_train(net.ptr, capi.NN_TRAIN["BPM"])
    assert net.train()
    p = os.path.join(d, "bpm.bin")
    net.dump_state(p)
    w = A.weights_of(net, d, "w.opt")
    net.close()
    b = open(p, "rb").read()
    st = A.read_state(p)
    assert st["has_adam"] == 0 and st["has_momentum"] == 1 and st["V"] is None
    head = b"HPNNSTA1" + struct.pack("<4I", 2, 1, 2, 1) + struct.pack("<3I", 8, 6, 4) + \
        struct.pack("<4I", A.SEED, 4, 0, 0) + struct.pack("<Q", 400)
    body = b"".join(x.tobytes() for x in w) + b"".join(x.tobytes() for x in st["dW"])
    assert b[:-8] == head + body and len(b) == len(head) + 2 * 8 * (48 + 24) + 8


def test_state_mismatches_warn(tmp_path, capfd):
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "SNN")
    A.write_conf(d, "8-6-4", "SNN", train="BPM", epochs=1)
    A.train(d, "cpu", dump="bpm.bin")
    A.write_conf(d, "8-6-4", "SNN", epochs=1)
    fresh = A.train(d, "cpu", dump="adam.bin")
    capfd.readouterr()
    capi.init(1)
    try:
        # a BPM state into an ADAM conf: the moments start at zero
        net = capi.Network(os.path.join(d, "nn.conf"))
        net.load_state(os.path.join(d, "bpm.bin"))
        assert "the moments start at zero" in capfd.readouterr().err
        net.set(device="cpu")
        assert net.train()
        net.dump_state(os.path.join(d, "x.bin"))
        net.close()
        assert A.read_state(os.path.join(d, "x.bin"))["t"] == fresh["state"]["t"]
        # an ADAM state into a BPM conf: the moments are ignored
        A.write_conf(d, "8-6-4", "SNN", train="BPM", epochs=1)
        net = capi.Network(os.path.join(d, "nn.conf"))
        net.load_state(os.path.join(d, "adam.bin"))
        assert "the moments are ignored" in capfd.readouterr().err
        net.set(device="cpu")
        assert net.train()
        net.dump_state(os.path.join(d, "y.bin"))
        net.close()
        assert A.read_state(os.path.join(d, "y.bin"))["has_adam"] == 0
    finally:
        capi.init(0)


def test_truncated_adam_block_is_a_load_error(tmp_path, capfd):
    d = str(tmp_path)
    A.make_data(d, "8-6-4", "SNN")
    A.write_conf(d, "8-6-4", "SNN", epochs=1)
    A.train(d, "cpu", dump="adam.bin")
    b = open(os.path.join(d, "adam.bin"), "rb").read()
    cut = b[:-8 - 16]  # t stays, p1 and p2 are gone; the checksum is recomputed so that only the size is wrong
    h = _fnv1a(cut)
    open(os.path.join(d, "cut.bin"), "wb").write(cut + struct.pack("<Q", h))
    open(os.path.join(d, "short.bin"), "wb").write(b[:-40])
    net = capi.Network(os.path.join(d, "nn.conf"))
    for name in ("cut.bin", "short.bin"):
        with pytest.raises(OSError):
            net.load_state(os.path.join(d, name))
    net.close()


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


# ------------------------------------------------------------------ 6. keep-best
def test_keep_best_returns_the_state_of_the_best_epoch(tmp_path):
    d = str(tmp_path)
    A.make_data(d, A.KEEP["net"], A.KEEP["net_type"])
    A.write_keep_conf(d)
    kept = A.train(d, "cpu", dump="kept.bin")
    assert kept["ok"]
    b = A.check_keep_fixture(kept)
    assert kept["epochs_done"] == b
    A.write_keep_conf(d, epochs=b, validate=None, keep_best=None, patience=None)
    plain = A.train(d, "cpu", dump="plain.bin")
    assert A.state_bits(kept["state"]) == A.state_bits(plain["state"])
    # two more epochs from each: the snapshot carried m, v and t, p1, p2
    A.write_keep_conf(d, epochs=2, validate=None, keep_best=None, patience=None)
    a = A.train(d, "cpu", load="kept.bin")
    c = A.train(d, "cpu", load="plain.bin")
    assert a["epochs_done"] == b + 2 and A.state_bits(a["state"]) == A.state_bits(c["state"])
    assert A.state_bits(a["state"]) != A.state_bits(kept["state"])


# ------------------------------------------------------------------ 7. the CPU emulation of the BF16 plan
def test_cpu_emulation_takes_adam_steps(tmp_path):
    sizes, B = [40, 64, 8], 128
    g = torch.Generator().manual_seed(2)
    m = MLP(sizes, "LNN", batch=B, device="cpu", optimizer="adam", lr=0.01, decay=0.01, seed=5)
    assert m.adam and m.A32[0].shape == m.W32[0].shape and ops.read_adam_state(m.adam_state)["t"] == 0
    for step in range(3):
        X = m.prepare_input(torch.rand(B, sizes[0], generator=g) * 2 - 1)
        T = torch.zeros(m.Bp, sizes[-1])
        T[torch.arange(B), torch.randint(0, sizes[-1], (B,), generator=g)] = 1.0
        w0 = [w.clone() for w in m.W32]
        m0 = [w.clone() for w in m.V32]
        v0 = [w.clone() for w in m.A32]
        m.train_step(X, T=T, n_valid=B - 3, lr=123.0, alpha=9.0)  # both ignored under Adam
        st = ops.read_adam_state(m.adam_state)
        assert st["t"] == step + 1
        for l in range(m.L):
            n = m.W32[l].numel()
            slabs = m.slab[l].reshape(m.S[l], n)
            A.check_update(w0[l].view(-1), m0[l].view(-1), v0[l].view(-1), slabs, 1.0 / (B - 3), st,
                           m.W32[l].view(-1), m.V32[l].view(-1), m.A32[l].view(-1), torch.float32, f"layer {l}")
            # against the independent PyTorch form on the emulation's own gradient
            w, mm, vv = w0[l].clone(), m0[l].clone(), v0[l].clone()
            gsum = ops.adam_slab_sum(m.slab[l]) * torch.tensor(1.0 / (B - 3), dtype=torch.float32)
            reference.adam_step(w, mm, vv, gsum, dict(st), advance=False)
            assert torch.equal(w, m.W32[l]) and torch.equal(mm, m.V32[l]) and torch.equal(vv, m.A32[l])
            N, K = sizes[l + 1], sizes[l]
            for t in (m.W32[l], m.V32[l], m.A32[l]):
                assert not t[N:].any() and not t[:, K:].any()  # the zero padding stays zero
            assert torch.equal(m.Wb[l], m.W32[l].bfloat16()) and torch.equal(m.Wt[l], m.Wb[l].t())
        assert not torch.equal(m.W32[0], w0[0])
    with pytest.raises(RuntimeError):
        m.update_layer(0, 0.1, 0.0, 1.0)


def test_data_parallel_refuses_an_adam_model():
    from hpnn_amd.parallel import DataParallel
    m = MLP([40, 64, 8], "LNN", batch=128, device="cpu", optimizer="adam")
    with pytest.raises(ValueError, match="one device"):
        DataParallel(m)
