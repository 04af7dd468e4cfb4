"""[clip] without a GPU: the host forms of include/libhpnn/clip.h (csrc/cpu/cpu_clip.cpp,
csrc/cpu/upd_host.h) bit for bit against the restatement of tests/clip_common.py and against
Python integers, the finalize's edges, the clipped host updates, the FP64 CPU oracle against the
independent PyTorch form, the conf key, the C API, the CLI, exact resume and [keep_best].

Every case prints what it measured."""
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from tests import clip_common as Q
from tests import upd_common as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]


def host_partials(slabs, scale, interleaved, extra=2):
    t = ops.GnormTable(slabs, interleaved=interleaved)
    p = torch.full((t.count + extra,), float("nan"), dtype=torch.float64)
    ops.gnorm_partials(t, p, scale)
    return t, p


# ------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("interleaved", [False, True], ids=["sequential", "8-way"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_host_sumsq_and_finalize_equal_the_restatement(dtype, interleaved):
    cases = [([n], S) for n in Q.SIZES for S in Q.SLABS] + [([4099, 3, 5], 2), ([5, 1025, 1], 9)]
    worst = 0.0
    for i, (sizes, S) in enumerate(cases):
        slabs = [Q.random_slabs(n, S, dtype, 50 + 7 * i + k) for k, n in enumerate(sizes)]
        t, p = host_partials(slabs, 1.0 / 7, interleaved)
        want = np.concatenate([Q.block_sums(s.numpy(), 1.0 / 7, interleaved) for s in slabs])
        assert t.count == len(want) == sum((n + 1023) // 1024 for n in sizes)
        assert p[:t.count].numpy().tobytes() == want.tobytes(), (sizes, S)
        assert bool(torch.isnan(p[t.count:]).all()), "partials past count were written"
        st, ref = ops.clip_state(0.5), Q.Clip(0.5)
        ops.clip_finalize(p, t.count, st)
        ref.finalize(Q.total(want))
        assert Q.same_state(ops.read_clip_state(st), ref.as_dict()), (sizes, S)
        # the order matters: a plain float64 sum differs somewhere, or the test shows nothing
        worst = max(worst, abs(float(np.sum(want)) - ref.sumsq) / ref.sumsq)
    print(f"host sumsq {dtype} interleaved {interleaved}: {len(cases)} cases bit-equal to the restatement; "
          f"largest relative distance to numpy's own sum {worst:.3g}")


def test_the_two_slab_orders_differ_somewhere():
    """S = 17 in float32: the sequential and the 8-way sum round differently, so a kernel that
    took the wrong order would be caught"""
    sl = Q.random_slabs(4099, 17, torch.float32, 3)
    a = Q.block_sums(sl.numpy(), 1.0, False)
    b = Q.block_sums(sl.numpy(), 1.0, True)
    assert a.tobytes() != b.tobytes()
    _, pa = host_partials([sl], 1.0, False)
    _, pb = host_partials([sl], 1.0, True)
    assert pa[:5].numpy().tobytes() == a.tobytes() and pb[:5].numpy().tobytes() == b.tobytes()


def test_more_than_256_partials():
    """n = 256 * 1024 + 5: 257 partials, the finalize's strided loop"""
    n = 256 * 1024 + 5
    sl = Q.random_slabs(n, 1, torch.float32, 9)
    t, p = host_partials([sl], 0.25, False)
    want = Q.block_sums(sl.numpy(), 0.25, False)
    assert t.count == 257 and p[:257].numpy().tobytes() == want.tobytes()
    st, ref = ops.clip_state(1.0), Q.Clip(1.0)
    ops.clip_finalize(p, 257, st)
    ref.finalize(Q.total(want))
    assert Q.same_state(ops.read_clip_state(st), ref.as_dict())


# ------------------------------------------------------------------ 2. integers: exact whatever the order
@pytest.mark.parametrize("interleaved", [False, True], ids=["sequential", "8-way"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_gradients_are_exact(dtype, interleaved):
    for n, S, j in ((4099, 1, 20), (4099, 9, 8), (1025, 17, 3), (3 * 1024, 2, 30)):
        sl, sumsq = Q.integer_set(n, S, j, dtype, 11 + S)
        sl = sl * 2  # with scale 0.5: the element the rule sees is the integer itself
        t, p = host_partials([sl], 0.5, interleaved)
        assert sum(int(x) for x in p[:t.count].tolist()) == sumsq and all(float(x).is_integer() for x in p[:t.count])
        for max_norm, factor, clipped in ((2.5 * j, 0.5, 1), (5.0 * j, 1.0, 0), (10.0 * j, 1.0, 0)):
            st = ops.clip_state(max_norm)
            ops.clip_finalize(p, t.count, st)
            r = ops.read_clip_state(st)
            assert (r["sumsq"], r["norm"], r["factor"], r["clipped"], r["steps"]) == \
                (float(sumsq), 5.0 * j, factor, clipped, 1), (n, S, j, max_norm, r)
    print(f"integer sets {dtype} interleaved {interleaved}: sums of squares equal Python's integers")


# ------------------------------------------------------------------ 3. the finalize's edges
def _finalize(max_norm, sumsq, st=None):
    st = ops.clip_state(max_norm) if st is None else st
    ops.clip_finalize(torch.tensor([sumsq], dtype=torch.float64), 1, st)
    return st, ops.read_clip_state(st)


def test_finalize_edges():
    # norm == max_norm: factor exactly 1, not counted
    _, r = _finalize(3.0, 9.0)
    assert (r["norm"], r["factor"], r["clipped"], r["steps"]) == (3.0, 1.0, 0, 1)
    assert (r["norm_max"], r["norm_last"]) == (3.0, 3.0)
    # the next double above it is clipped
    x = math.nextafter(3.0, math.inf)
    _, r = _finalize(3.0, x * x)
    assert r["norm"] == x and r["factor"] == 3.0 / x and r["factor"] < 1.0 and r["clipped"] == 1
    # an all-zero gradient
    _, r = _finalize(3.0, 0.0)
    assert (r["norm"], r["factor"], r["clipped"], r["norm_max"]) == (0.0, 1.0, 0, 0.0)
    # an infinite norm: factor 0
    _, r = _finalize(3.0, math.inf)
    assert (r["norm"], r["factor"], r["clipped"], r["norm_max"]) == (math.inf, 0.0, 1, math.inf)
    # a NaN: factor 1, never into norm_max
    st, r = _finalize(3.0, 16.0)
    assert r["norm_max"] == 4.0 and r["clipped"] == 1 and r["factor"] == 0.75
    st, r = _finalize(3.0, math.nan, st)
    assert math.isnan(r["norm"]) and math.isnan(r["norm_last"]) and r["factor"] == 1.0
    assert r["norm_max"] == 4.0 and r["clipped"] == 1 and r["steps"] == 2
    # the counters run over the epoch; commit files them and zeroes them; a full history drops
    st, r = _finalize(3.0, 1.0, st)
    assert (r["steps"], r["clipped"], r["norm_max"], r["norm_last"]) == (3, 1, 4.0, 1.0)
    hist, cur = ops.clip_history(1)
    ops.clip_commit(st, hist, cur)
    assert ops.read_clip_history(hist, cur) == [dict(steps=3, clipped=1, norm_max=4.0, norm_last=1.0)]
    r = ops.read_clip_state(st)
    assert (r["steps"], r["clipped"], r["norm_max"], r["norm_last"], r["max_norm"]) == (0, 0, 0.0, 0.0, 3.0)
    _finalize(3.0, 100.0, st)
    before = hist.clone()
    ops.clip_commit(st, hist, cur)
    assert int(cur[0]) == 1 and torch.equal(U.ibits(hist), U.ibits(before))
    assert ops.read_clip_state(st)["steps"] == 0


def test_state_layout_and_validity():
    assert ops.native().CLIP_STATE_BYTES == 64 and ops.native().CLIP_RECORD_BYTES == 24
    assert ops.native().GNORM_SEG_BYTES == 32
    s = ops.clip_state(0.75)
    assert s.tolist()[:6] == [0.75, 0.0, 0.0, 1.0, 0.0, 0.0] and s.view(torch.int32)[12:].tolist() == [0, 0, 0, 0]
    ops.write_clip_state(s, steps=7, clipped=2, norm_max=1.5)
    r = ops.read_clip_state(s)
    assert (r["steps"], r["clipped"], r["norm_max"]) == (7, 2, 1.5)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            ops.clip_state(bad)
    with pytest.raises(ValueError):
        ops.GnormTable([torch.ones(4)] * 17)
    with pytest.raises(ValueError):
        ops.GnormTable([torch.ones(0)])


# ------------------------------------------------------------------ 4. the clipped host updates
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_host_updates_take_one_product_in_t(dtype):
    """the rule receives gs * (T)factor: BP w + lr * (gs * f), restated in numpy; a factor of 1 and
    clip=None give the same bits; g = 0 keeps w's bits; Adam on pre-scaled slabs at factor 0.5"""
    T = Q.NP[dtype]
    n, S = 1031, 3
    g = torch.Generator().manual_seed(4)
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    sl = Q.random_slabs(n, S, dtype, 5)
    sl[:, :3] = 0.0
    lrs = ops.lr_state("constant", lr0=0.3)
    for factor in (0.3, 1.0, 0.0):
        cs = ops.write_clip_state(ops.clip_state(1.0), factor=factor)
        w1 = w.clone()
        ops.sgd_sched_fp(ops.SgdSchedTable([dict(w=w1, slab=sl)]), lrs, scale=1.0 / 7, clip=cs)
        gs = Q.slab_sum(sl.numpy(), False) * T(1.0 / 7)
        want = w.numpy() + T(0.3) * (gs * T(factor))
        assert w1.numpy().tobytes() == want.tobytes(), factor
        assert torch.equal(U.ibits(w1[:3]), U.ibits(w[:3]))
    plain, one = w.clone(), w.clone()
    ops.sgd_sched_fp(ops.SgdSchedTable([dict(w=plain, slab=sl)]), lrs, scale=1.0 / 7)
    ops.sgd_sched_fp(ops.SgdSchedTable([dict(w=one, slab=sl)]), lrs, scale=1.0 / 7,
                     clip=ops.clip_state(1.0))
    assert torch.equal(U.ibits(plain), U.ibits(one))
    # Adam: factor 0.5 on the slabs == factor-free on slabs halved beforehand (a halving is exact)
    ast = ops.adam_advance(ops.adam_state(lr=0.01))
    half = ops.write_clip_state(ops.clip_state(1.0), factor=0.5)
    a = dict(w=w.clone(), m=torch.zeros_like(w), v=torch.zeros_like(w), slab=sl)
    b = dict(w=w.clone(), m=torch.zeros_like(w), v=torch.zeros_like(w), slab=sl * 0.5)
    ops.adam_update_fp(ops.AdamTable([a]), ast, scale=2.0, clip=half)
    ops.adam_update_fp(ops.AdamTable([b]), ast, scale=2.0)
    for k in ("w", "m", "v"):
        assert torch.equal(U.ibits(a[k]), U.ibits(b[k])), k
    assert not torch.equal(a["w"], w)


# ------------------------------------------------------------------ 5. the FP64 CPU oracle
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("clip"))
    return (d,) + tuple(Q.make_data(d))


EPOCHS = 6


@pytest.mark.parametrize("tr", ["BP", "BPM", "ADAM"])
def test_oracle_matches_the_reference_and_clips_some_steps(data, tr):
    """max_norm = the median of the per-step norms of the unclipped run of the same configuration:
    the clipped run must clip, and not always.  The oracle against the independent PyTorch form at
    100 x the order spread of the same run (the tolerance of tests/test_adam_cpu.py)."""
    d, X, T = data[:3]
    lr = 0.01 if tr == "ADAM" else 1.0
    Q.write_conf(d, train=tr, epochs=EPOCHS, lr=lr)
    plain = Q.train(d)
    assert plain["ok"] and plain["clip"] == []
    c, norms = Q.median_norm(plain["w0"], X, T, "SNN", Q.NET["B"], EPOCHS, tr, lr=lr)
    # the unclipped oracle reports the same norms (a bound nothing reaches): per epoch the largest and the last
    huge = Q.train(d, clip=1e300)
    assert huge["raw"] == plain["raw"] and [r["clipped"] for r in huge["clip"]] == [0] * EPOCHS
    for e, r in enumerate(huge["clip"]):
        ep = norms[3 * e:3 * e + 3]
        assert r["steps"] == 3 and abs(r["norm_max"] - max(ep)) <= 1e-9 * max(ep)
        assert abs(r["norm_last"] - ep[-1]) <= 1e-9 * ep[-1]
    got = Q.train(d, clip=c)
    assert got["ok"] and len(got["clip"]) == EPOCHS
    steps, clipped = sum(r["steps"] for r in got["clip"]), sum(r["clipped"] for r in got["clip"])
    W, cn = Q.reference_run(plain["w0"], X, T, "SNN", Q.NET["B"], EPOCHS, tr, lr=lr, clip=c)
    tol = 100.0 * Q.order_spread(plain["w0"], X, T, "SNN", Q.NET["B"], EPOCHS, tr, lr=lr, clip=c)
    err = Q.A.spread(got["w"], W)
    moved = Q.A.spread(got["w"], plain["w"])
    print(f"{tr}: max_norm {c:.6g} (norms {min(norms):.4g} .. {max(norms):.4g}), clipped {clipped}/{steps}, "
          f"order spread {tol / 100:.3g}, oracle - reference {err:.3g}, clipped - unclipped {moved:.3g}")
    assert steps == 3 * EPOCHS and 0 < clipped < steps
    assert clipped == sum(1 for x in cn if x > c)
    assert tol > 0.0 and err <= tol
    assert moved > 1e3 * tol, "the fixture is at fault: clipping changed nothing"


@pytest.mark.parametrize("tr", ["BP", "BPM", "ADAM"])
def test_resume_is_exact_and_the_state_file_does_not_change(data, tr):
    d, X, T = data[:3]
    lr = 0.01 if tr == "ADAM" else 1.0
    Q.write_conf(d, train=tr, epochs=4, lr=lr)
    plain = Q.train(d)
    c = Q.median_norm(plain["w0"], X, T, "SNN", Q.NET["B"], 4, tr, lr=lr)[0]
    full = Q.train(d, clip=c)
    Q.write_conf(d, train=tr, epochs=2, lr=lr)
    h1 = Q.train(d, dump="h1.bin", clip=c)
    h2 = Q.train(d, load="h1.bin", dump="h2.bin", clip=c)
    assert full["ok"] and h1["ok"] and h2["ok"]
    assert Q.K.wbytes(h2["w"]) == Q.K.wbytes(full["w"]) and h2["raw"] == full["raw"]
    assert h1["clip"] + h2["clip"] == full["clip"] and 0 < sum(r["clipped"] for r in full["clip"]) < 12
    assert len(full["raw"]) == len(plain["raw"]) and full["raw"] != plain["raw"]  # no new block in the file


def test_keep_best_returns_the_best_epochs_kernel(data):
    d, X, T = data[:3]
    Q.write_conf(d, train="BPM", epochs=10, validate=1, lr=2.0)
    plain = Q.train(d)
    c = Q.median_norm(plain["w0"], X, T, "SNN", Q.NET["B"], 10, "BPM", lr=2.0)[0]
    kb = Q.train(d, clip=c, keep_best="loss", patience=3)
    b = kb["best"]["epoch"]
    print(f"keep_best under clip {c:.4g}: best epoch {b}, {len(kb['val'])} passes, {len(kb['clip'])} clip records")
    assert 1 <= b < 10 and kb["epochs_done"] == b
    assert len(kb["clip"]) == len(kb["val"])  # reported up to the stopping pass's epoch
    Q.write_conf(d, train="BPM", epochs=b, validate=1, lr=2.0)
    e = Q.train(d, clip=c)
    assert e["raw"] == kb["raw"] and Q.K.wbytes(e["w"]) == Q.K.wbytes(kb["w"])
    assert e["clip"] == kb["clip"][:b]


# ------------------------------------------------------------------ 6. the interface
def test_conf_round_trip(data, tmp_path):
    d = data[0]
    Q.write_conf(d, clip=0.375)
    net = capi.Network(os.path.join(d, "nn.conf"))
    assert net.clip == 0.375
    p = str(tmp_path / "out.conf")
    net.dump_conf(p)
    assert "[clip] 0.375" in open(p).read()
    net.close()
    net2 = capi.Network(p)
    assert net2.clip == 0.375
    net2.set(clip=0)
    net2.dump_conf(p)
    assert net2.clip == 0.0 and "[clip]" not in open(p).read()
    with pytest.raises(ValueError):
        net2.set(clip=-1.0)
    with pytest.raises(ValueError):
        net2.set(clip=float("nan"))
    net2.close()
    Q.write_conf(d)
    net = capi.Network(os.path.join(d, "nn.conf"))
    assert net.clip == 0.0 and net.clip_history() == []
    net.close()


@pytest.mark.parametrize("val", ["-1", "inf", "nan", "x", ""])
def test_conf_value_errors(data, capfd, val):
    Q.write_conf(data[0], clip=val)
    with pytest.raises(RuntimeError):
        capi.Network(os.path.join(data[0], "nn.conf"))
    assert "[clip]" in capfd.readouterr().err


def test_refusals(data, capfd):
    d = data[0]
    Q.write_conf(d, train="CG", epochs=2)
    capi.init(0)
    net = capi.Network(os.path.join(d, "nn.conf"))
    w0 = Q.K.C.weights_of(net, d, "r0.opt")
    net.set(device="cpu", clip=0.5)
    assert not net.train()
    capi._LIBC.fflush(None)
    err = capfd.readouterr().err
    assert "[clip] is not supported by [train] CG" in err and "BP, BPM or ADAM" in err
    assert Q.K.wbytes(Q.K.C.weights_of(net, d, "r1.opt")) == Q.K.wbytes(w0)  # weights untouched
    # a bound set through the C API is checked by nn_train_kernel too
    Q.write_conf(d, train="BP", epochs=2)
    net2 = capi.Network(os.path.join(d, "nn.conf"))
    net2.set(device="cpu")
    net2.L.nn_set_clip(net2.ptr, -2.0)
    assert not net2.train()
    capi._LIBC.fflush(None)
    assert "[clip] -2 is out of range" in capfd.readouterr().err
    net.close(), net2.close()


def test_python_multi_device_refusal_and_update_layer():
    from hpnn_amd.models import MLP
    from hpnn_amd.parallel.dp import DataParallel
    m = MLP([32, 32, 32], "SNN", batch=32, device="cpu", clip=0.5, lr=0.1)
    with pytest.raises(ValueError, match="one device only"):
        DataParallel(m)
    with pytest.raises(RuntimeError, match="one launch"):
        m.update_layer(0, 0.1, 0.0, 1.0)
    with pytest.raises(ValueError):
        MLP([32, 32, 32], "SNN", batch=32, device="cpu", clip=-1.0)
    plain = MLP([32, 32, 32], "SNN", batch=32, device="cpu")
    assert not plain.clip and ("clip", -1) not in plain.buf and ("lrs", -1) not in plain.buf
    with pytest.raises(RuntimeError):
        plain.commit_clip()


def test_online_mode_warns_once(data, capfd):
    Q.write_conf(data[0], train="BP", mode="online", batch=None, epochs=None)
    capi.init(1)
    try:
        net = capi.Network(os.path.join(data[0], "nn.conf"))
        net.set(device="cpu", clip=0.5)
        assert net.train() and net.clip_history() == []
        net.close()
    finally:
        capi.init(0)
        capi._LIBC.fflush(None)
    assert capfd.readouterr().err.count("[clip] has no effect in online mode") == 1


def test_cli_lines_and_metrics(data):
    """train_nn -C c: the clipping line, one CLIP line per epoch at -vv, one "clip" event per epoch;
    without -C none of them, and no schedule line either way"""
    d = data[0]
    Q.write_conf(d, train="BPM", epochs=3, lr=1.0)
    m = os.path.join(d, "m.jsonl")
    if os.path.exists(m):
        os.remove(m)
    r = subprocess.run([os.path.join(BIN, "train_nn"), "-vv", "-c", "-C", "0.05", "-M", "m.jsonl", "nn.conf"], cwd=d,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("gradient clipping: max norm 0.05") == 1
    lines = [ln.split("CLIP: ")[1] for ln in r.stdout.splitlines() if "CLIP: epoch" in ln]
    ev = [e for e in (json.loads(ln) for ln in open(m)) if e.get("event") == "clip"]
    assert len(lines) == 3 and [e["epoch"] for e in ev] == [1, 2, 3] and all(e["engine"] == "cpu" for e in ev)
    for ln, e in zip(lines, ev):
        assert ln == (f"epoch {e['epoch']} steps={e['steps']} clipped={e['clipped']} max_norm={e['max_norm']:.17g} "
                      f"last_norm={e['last_norm']:.17g}")
        assert e["steps"] == 3 and 0 <= e["clipped"] <= 3 and e["max_norm"] >= e["last_norm"] > 0.0
    assert "LR:" not in r.stdout and "learning rate schedule" not in r.stdout
    assert not [e for e in (json.loads(ln) for ln in open(m)) if e.get("event") == "lr"]
    os.remove(m)
    r2 = subprocess.run([os.path.join(BIN, "train_nn"), "-vv", "-c", "-M", "m.jsonl", "nn.conf"], cwd=d,
                        capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0 and "CLIP:" not in r2.stdout and "gradient clipping" not in r2.stdout
    assert not [ln for ln in open(m) if '"clip"' in ln.split(",")[0]]
    for bad in ("-1", "nan", "x"):
        b = subprocess.run([os.path.join(BIN, "train_nn"), "-C", bad, "nn.conf"], cwd=d, capture_output=True, text=True,
                           timeout=60)
        assert b.returncode != 0 and "-C" in b.stderr
    h = subprocess.run([os.path.join(BIN, "train_nn"), "-h"], capture_output=True, text=True, timeout=60)
    assert "-C c" in h.stdout


# ------------------------------------------------------------------ 7. the Python plan's emulation
@pytest.mark.parametrize("opt", ["BP", "BPM", "adam"])
def test_mlp_emulation_clips_by_the_padded_slabs_norm(opt):
    """the CPU emulation of the clipping plan: a bound nothing reaches is the unclipped plan bit
    for bit (one slab per layer at this batch); under a low bound the state holds norm and factor
    of the independent form, the step shrinks by the factor, and the zero padding stays zero"""
    from hpnn_amd.models import MLP
    torch.manual_seed(1)
    sizes, B = [40, 64, 8], 32
    X = torch.rand(B, sizes[0]) * 2 - 1
    T = torch.full((B, sizes[-1]), -1.0)
    T[torch.arange(B), torch.randint(0, sizes[-1], (B,))] = 1.0
    kw = dict(optimizer="adam", lr=0.01) if opt == "adam" else dict(momentum=opt == "BPM", lr=0.125)

    def run(clip, steps=1):
        m = MLP(sizes, "ANN", batch=B, device="cpu", seed=5, clip=clip, **kw)
        assert all(s == 1 for s in m.S)
        Tp = torch.zeros(m.Bp, sizes[-1])
        Tp[:B] = T
        for _ in range(steps):
            m.train_step(m.prepare_input(X), T=Tp, n_valid=B, lr=0.125, alpha=0.25)
        return m

    plain, far = run(None, 3), run(1e30, 3)
    for l in range(2):
        assert torch.equal(plain.W32[l], far.W32[l]) and torch.equal(plain.Wb[l], far.Wb[l])
        assert torch.equal(plain.Wt[l], far.Wt[l])
    r = ops.read_clip_state(far.clip_state)
    assert (r["steps"], r["clipped"], r["factor"]) == (3, 0, 1.0) and r["norm_max"] > 0.0
    one = run(1e30)
    norm = ops.read_clip_state(one.clip_state)["norm"]
    G = [one.slab[l][0].double() / B for l in range(2)]
    ref = float(torch.linalg.vector_norm(torch.cat([g.reshape(-1) for g in G])))
    assert abs(norm - ref) <= 1e-6 * ref
    low = run(norm / 4)
    r = ops.read_clip_state(low.clip_state)
    assert r["clipped"] == 1 and r["factor"] == (norm / 4) / norm == 0.25
    w0 = MLP(sizes, "ANN", batch=B, device="cpu", seed=5, **kw).W32
    if opt != "adam":  # BP / BPM: the first step is lr * g * factor; a factor of 1/4 is exact
        for l in range(2):
            assert torch.allclose((low.W32[l] - w0[l]) * 4, one.W32[l] - w0[l], rtol=1e-5, atol=1e-7)
    for l in range(2):
        assert not low.W32[l][sizes[l + 1]:].any() and not low.W32[l][:, sizes[l]:].any()
    hist, cur = ops.clip_history(2)
    low.commit_clip(hist, cur)
    assert ops.read_clip_history(hist, cur)[0]["clipped"] == 1 and ops.read_clip_state(low.clip_state)["steps"] == 0
    print(f"{opt}: norm {norm:.6g} (independent {ref:.6g}), factor at norm / 4: {r['factor']}")
