"""[confusion] on the GPU: hpnn_confusion_add at its edges against the numpy reference (guard words
on both sides of M), hpnn_confusion_commit against its emulation, a captured sequence of
evaluation, tally and the two commits, and the engines: the Python plan (fused and per-layer
evaluation) and the FP32 / FP64 batched engines against their own guesses, the FP64 engine against
the FP64 CPU oracle, the kept pass under -K acc -P 2, and the key off.

Every expected value is an integer count: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd._lib import native
from hpnn_amd.models import MLP
from hpnn_amd.utils import formats
from tests import confusion_common as cc
from tests import keep_best_common as kb

GUARD = 16  # int32 words on either side of M
SENTINEL = 0x5a5a5a5a
ROWS = [1, 255, 256, 257, 1000]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """a zeroed matrix inside a sentinel-filled buffer"""

    def __init__(self, n_out):
        self.cells = n_out * (n_out + 1)
        self.buf = torch.full((2 * GUARD + self.cells,), SENTINEL, dtype=torch.int32, device="cuda")
        self.M = self.buf[GUARD:GUARD + self.cells].view(n_out, n_out + 1)
        self.M.zero_()

    def get(self):
        """the matrix as numpy uint32, after checking both guards"""
        b = self.buf.cpu()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.cells:] == SENTINEL).all(), "a guard word changed"
        return b[GUARD:GUARD + self.cells].numpy().view(np.uint32).reshape(self.M.shape)


def _fast_matrix(guess, target, n_out):
    """cc.matrix for large inputs (numpy scatter-add; the same rule)"""
    g, t = np.asarray(guess, dtype=np.int64), np.asarray(target, dtype=np.int64)
    ok = (g >= 0) & (t >= 0) & (t < n_out)
    M = np.zeros((n_out, n_out + 1), dtype=np.uint32)
    np.add.at(M, (t[ok], np.minimum(g[ok], n_out)), 1)
    return M


def _data(n_out, kind, rows):
    """guesses with a sprinkle of "none" and pad rows; targets with ties (dense values from a set of
    four), an out-of-range label among the labels; dense rows ldt = n_out + 3 apart"""
    rng = np.random.default_rng(1000 * n_out + rows)
    guess = rng.integers(0, n_out, rows).astype(np.int32)
    guess[rng.random(rows) < 0.05] = cc.GUESS_NONE
    guess[rng.random(rows) < 0.05] = cc.GUESS_PAD
    if kind == "labels":
        lab = rng.integers(0, n_out, rows).astype(np.int32)
        if rows > 4:
            lab[3], lab[rows - 1] = n_out, -2  # caller bugs: skipped, nothing written
        return guess, lab, torch.tensor(lab).cuda(), lab.astype(np.int64)
    dt = np.float32 if kind == "f32" else np.float64
    T = rng.integers(0, 4, (rows, n_out + 3)).astype(dt) * dt(0.25)
    T[:, n_out:] = 9.0  # past n_out: never read
    tgt = np.argmax(T[:, :n_out], axis=1)  # numpy's argmax is the first maximum too
    if rows <= 257 and n_out <= 33:
        assert np.array_equal(tgt, cc.target_class(T[:, :n_out]))
    return guess, T, torch.tensor(T).cuda(), tgt


# ------------------------------------------------------------------ confusion_add
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["labels", "f32", "f64"])
@pytest.mark.parametrize("n_out", [1, 2, 10, 32, 33, 64, 65, 230])
def test_confusion_add_at_its_edges(gpu, n_out, kind):
    """the kernel has one form and no threshold between two; 32 | 33 and 64 | 65 are the sizes at
    which the lanes per dense row change (32 -> 64) and a lane starts to load a second value"""
    for rows in ROWS:
        guess, _, tdev, tgt = _data(n_out, kind, rows)
        for n_valid in sorted({0, 1, rows - 1, rows}):
            g = guess.copy()
            g[n_valid:] = cc.GUESS_PAD  # what an evaluation kernel leaves from n_valid up
            want = _fast_matrix(g, tgt, n_out)
            if rows <= 257:
                assert np.array_equal(want, cc.matrix(g, tgt, n_out))
            G = _Guarded(n_out)
            kw = dict(labels=tdev) if kind == "labels" else dict(T=tdev)
            ops.confusion_add(torch.tensor(g).cuda(), G.M, **kw)
            got = G.get()
            assert np.array_equal(got, want), (n_out, kind, rows, n_valid)
            assert int(got.sum()) == int(((g >= 0) & (tgt >= 0) & (tgt < n_out)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n_out", [10, 230])
def test_all_rows_in_one_cell_count_exactly(gpu, n_out):
    rows = 4096
    G = _Guarded(n_out)
    guess = torch.full((rows,), n_out - 1, dtype=torch.int32, device="cuda")
    lab = torch.full((rows,), 1 % n_out, dtype=torch.int32, device="cuda")
    ops.confusion_add(guess, G.M, labels=lab)
    got = G.get()
    assert int(got[1 % n_out, n_out - 1]) == rows and int(got.sum()) == rows
    # two launches accumulate before a commit; the dense form of the same rows agrees
    T = torch.zeros(rows, n_out, dtype=torch.float64, device="cuda")
    T[:, 1 % n_out] = 1.0
    ops.confusion_add(guess, G.M, T=T)
    got = G.get()
    assert int(got[1 % n_out, n_out - 1]) == 2 * rows and int(got.sum()) == 2 * rows


@pytest.mark.gpu
def test_confusion_add_refuses_bad_arguments_and_launches_nothing(gpu):
    G = _Guarded(4)
    g = torch.zeros(8, dtype=torch.int32, device="cuda")
    T = torch.zeros(8, 4, dtype=torch.float32, device="cuda")
    nat = native()
    assert nat.confusion_add(0, T.data_ptr(), 4, 1, 8, 4, G.M.data_ptr(), _stream()) == -1
    assert nat.confusion_add(g.data_ptr(), 0, 4, 1, 8, 4, G.M.data_ptr(), _stream()) == -1
    assert nat.confusion_add(g.data_ptr(), T.data_ptr(), 3, 1, 8, 4, G.M.data_ptr(), _stream()) == -1  # ldt < n_out
    assert nat.confusion_add(g.data_ptr(), T.data_ptr(), 4, 3, 8, 4, G.M.data_ptr(), _stream()) == -1  # t_kind
    assert nat.confusion_add(g.data_ptr(), T.data_ptr(), 4, 1, 8, 0, G.M.data_ptr(), _stream()) == -1
    assert nat.confusion_add(g.data_ptr(), T.data_ptr(), 4, 1, -1, 4, G.M.data_ptr(), _stream()) == -1
    assert nat.confusion_add(g.data_ptr(), T.data_ptr() + 4, 4, 2, 8, 4, G.M.data_ptr(), _stream()) == -1
    assert nat.confusion_add(g.data_ptr(), T.data_ptr(), 4, 1, 0, 4, G.M.data_ptr(), _stream()) == 0  # no rows
    assert nat.confusion_commit(0, 4, 0, 0, g.data_ptr(), 0, _stream()) == -1
    assert nat.confusion_commit(G.M.data_ptr(), 4, 0, 0, 0, 0, _stream()) == -1
    assert int(G.get().sum()) == 0


# ------------------------------------------------------------------ confusion_commit
@pytest.mark.gpu
@pytest.mark.parametrize("n_out", [1, 10, 230])
def test_confusion_commit_equals_the_emulation(gpu, n_out):
    rng = np.random.default_rng(n_out)
    res = {}
    for dev in ("cpu", "cuda"):
        M = ops.confusion_matrix(n_out, dev)
        cells = n_out * (n_out + 1)
        buf = torch.full((2 * GUARD + 2 * 3 * n_out,), SENTINEL, dtype=torch.int32, device=dev)
        hist = buf[GUARD:GUARD + 6 * n_out].view(2, 3 * n_out)
        hist.zero_()
        last, cur = ops.confusion_matrix(n_out, dev), torch.zeros(1, dtype=torch.int32, device=dev)
        out = []
        for p in range(3):  # two records filed at the cursor's indices, the third dropped
            rows = 300 + 50 * p
            g = torch.tensor(rng.integers(0, n_out + 1, rows).astype(np.int32)).to(dev)
            lab = torch.tensor(rng.integers(0, n_out, rows).astype(np.int32)).to(dev)
            ops.confusion_add(g, M, labels=lab)
            before = M.cpu().clone()
            ops.confusion_commit(M, hist, last, cur)
            assert int(M.cpu().abs().sum()) == 0 and torch.equal(last.cpu(), before)
            cur += 1  # what validate_commit does behind it
            out.append((buf.cpu().clone(), last.cpu().clone()))
        assert cells == M.numel()
        res[dev] = out
        rng = np.random.default_rng(n_out)
    for p, ((hc, lc), (hg, lg)) in enumerate(zip(res["cpu"], res["cuda"])):
        assert torch.equal(hc, hg) and torch.equal(lc, lg), p
    final = res["cuda"][-1][0]
    assert (final[:GUARD] == SENTINEL).all() and (final[GUARD + 6 * n_out:] == SENTINEL).all()
    assert torch.equal(res["cuda"][1][0], res["cuda"][2][0]), "a cursor at the capacity wrote a record"
    rec = cc.class_record(res["cuda"][0][1].numpy().view(np.uint32))
    got = final[GUARD:GUARD + 3 * n_out].numpy().view(np.uint32)
    assert np.array_equal(got, np.concatenate([rec["support"], rec["hit"], rec["predicted"]]))


# ------------------------------------------------------------------ the Python plan: graph, fused and per-layer
def _plan(monkeypatch, fused, dense):
    if fused:
        monkeypatch.delenv("HPNN_EVAL_FUSED", raising=False)
    else:
        monkeypatch.setenv("HPNN_EVAL_FUSED", "0")
    n, n_out = 1000, 10
    g = torch.Generator().manual_seed(12)
    X = torch.randint(0, 256, (n, 784), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, n_out, (n,), dtype=torch.int32, generator=g)
    m = MLP([784, 128, 64, n_out], "SNN", batch=256, momentum=True, seed=6, fused="t")
    assert m.plan.eval_is_fused() == fused
    kw = dict(labels=lab.cuda())
    if dense:  # soft targets with ties: the first maximum is the class
        T = torch.zeros(n, n_out)
        T[torch.arange(n), lab.long()] = 0.5
        T[torch.arange(n), (lab.long() + 3) % n_out] = 0.5
        kw = dict(T=T.cuda())
        lab = torch.minimum(lab, (lab + 3) % n_out)
    return m, m.prepare_input(X.cuda()), kw, lab.numpy(), n, n_out


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True], ids=["labels", "dense"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
def test_plan_matrix_equals_the_tally_of_its_own_guesses(gpu, monkeypatch, fused, dense):
    m, Xg, kw, target, n, n_out = _plan(monkeypatch, fused, dense)
    guess = m.evaluate(Xg, n_valid=n, guess=True, **kw).cpu().numpy()
    hits = m.read_eval_stats()[1]
    m.confusion(True, passes=2)
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")
    m.evaluate(Xg, n_valid=n, **kw)
    m.commit_confusion(cur)
    want = cc.matrix(guess[:n], target, n_out)
    got = m.confusion_matrix("last").numpy().astype(np.uint32)
    assert np.array_equal(got, want) and int(got.sum()) == n and int(np.trace(got[:, :-1])) == hits
    rec = cc.class_record(want)
    assert all(m.class_history(1)[0][k] == rec[k].tolist() for k in rec)
    assert m.confusion_matrix("best") is None
    m.confusion(False)
    assert m.confusion_matrix("last") is None and m.evaluate(Xg, n_valid=n, **kw) is None


@pytest.mark.gpu
def test_captured_pass_replayed_twice_gives_the_eager_result(gpu, monkeypatch):
    m, Xg, kw, target, n, n_out = _plan(monkeypatch, True, False)
    m.confusion(True, passes=4)
    m.keep_best("acc", 0)
    vst = m.buf[("vstats", -1)]
    hist = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_pass():
        m.evaluate(Xg, n_valid=n, **kw)
        m.commit_confusion(cur)
        ops.validate_commit(vst, hist, cur)
        m.commit_best(hist, cur)
    one_pass()  # eager: record 0 (and every code object loaded before the capture)
    torch.cuda.synchronize()
    eager = m.confusion_matrix("last")
    assert int(eager.sum()) == n and torch.equal(m.confusion_matrix("best"), eager)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        one_pass()
    for i in (1, 2):
        m._cm_last.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert int(cur.item()) == i + 1
        assert torch.equal(m.confusion_matrix("last"), eager), f"replay {i}: M was not zeroed, or a tally was lost"
    recs = m.class_history(3)
    assert recs[0] == recs[1] == recs[2] and sum(recs[0]["support"]) == n
    assert int(m._cm.abs().sum()) == 0
    assert torch.equal(m.confusion_matrix("best"), eager) and m.best_state()["index"] == 0  # ties do not improve


# ------------------------------------------------------------------ the batched engines through train_nn
def _fp_guesses(d, name, Xv, Tv, f64):
    """the FP engine's own evaluation of the held-out set with the weights of d/kernel.opt: the
    same GEMM and output launches in the same chunks of [batch] rows; returns the guesses"""
    f = cc.NETS[name]
    dt = torch.float64 if f64 else torch.float32
    W = [torch.tensor(np.asarray(w), dtype=dt).cuda().contiguous()
         for w in formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"]]
    X, T = torch.tensor(Xv, dtype=dt).cuda(), torch.tensor(Tv, dtype=dt).cuda()
    nv, n_out, nat = X.shape[0], T.shape[1], native()
    guess = torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    slots = torch.zeros(64, 16, device="cuda")
    for r0 in range(0, nv, f["B"]):
        rows = min(f["B"], nv - r0)
        A = X[r0:r0 + rows]
        for l, w in enumerate(W):
            N, K = w.shape
            out = torch.empty(rows, N, dtype=dt, device="cuda")
            nat.gemm_fp(int(f64), A.data_ptr(), K, 0, w.data_ptr(), K, 0, out.data_ptr(), N, 0, 0, rows, N, K,
                        ops.EPI_NONE if l == len(W) - 1 else ops.EPI_ACT, 1, 0, _stream())
            A = out
        nat.output_fp_eval(int(f64), A.data_ptr(), n_out, T[r0:].data_ptr(), n_out, guess[r0:].data_ptr(),
                           slots.data_ptr(), rows, rows, n_out, {"ANN": 0, "LNN": 1, "SNN": 2}[f["type"]], _stream())
    torch.cuda.synchronize()
    return guess.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["S", "L"])
def test_fp_engine_matrix_equals_the_tally_of_its_own_guesses(tmp_path, gpu, name, dtype):
    d = str(tmp_path)
    f, Xv, Tv = cc.make_net(d, name)
    cc.write_conf(d, name, dtype=dtype, epochs=3)
    out = cc.run(d, "-V", "1", "-X", "m.txt", cpu=False).stdout
    assert f"batched GPU training: {dtype}" in out and "per-class metrics of every validation pass" in out
    got = cc.read_matrix_file(os.path.join(d, "m.txt"))
    guess = _fp_guesses(d, name, Xv, Tv, dtype == "f64")
    assert np.array_equal(got, cc.matrix(guess, cc.target_class(Tv), f["sizes"][-1]))
    recs, lines = kb.records(out), cc.CLASSES_RE.findall(out)
    assert len(recs) == len(lines) == 3 and int(got.sum()) == f["nv"] and int(np.trace(got[:, :-1])) == recs[-1][2]


@pytest.mark.gpu
@pytest.mark.parametrize("fx,mode,env", [("D", "t", None), ("D", "t", {"HPNN_EVAL_FUSED": "0"}), ("B", "-", None)],
                         ids=["tile-fused", "tile-per-layer-eval", "per-layer-plan"])
def test_bf16_engine_matrix_agrees_with_its_validation_records(tmp_path, gpu, fx, mode, env):
    d = str(tmp_path)
    f = kb.make_fixture(d, fx)
    kb.write_conf(d, fx, dtype="bf16", epochs=3)
    out = kb.run(d, "-v", "-V", "1", "-X", "m.txt", "-M", "m.jsonl", cpu=False, env=env).stdout
    assert f"batched plan: mode {mode}" in out, out[-3000:]
    got = cc.read_matrix_file(os.path.join(d, "m.txt"))
    recs, events = kb.records(out), cc.classes_events(os.path.join(d, "m.jsonl"))
    assert len(recs) == len(events) == 3 and int(got.sum()) == f["nv"]
    assert int(np.trace(got[:, :-1])) == recs[-1][2]
    for r, ev in zip(recs, events):
        assert ev["engine"] == "gpu" and ev["epoch"] == r[0]
        assert sum(ev["hit"]) == r[2] and sum(ev["support"]) == f["nv"] and sum(ev["predicted"]) <= f["nv"]
    rec = cc.class_record(got)
    assert all(events[-1][k] == rec[k].tolist() for k in rec)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused-eval", "per-layer-eval"])
def test_bf16_engine_matrix_equals_the_tally_of_independent_guesses(tmp_path, gpu, monkeypatch, fused):
    """train_nn's bf16 engine on the tile plan against guesses it did not make itself: its dumped
    weights loaded into the Python plan, which evaluates the held-out set through the same kernels"""
    d = str(tmp_path)
    f = kb.make_fixture(d, "D")
    kb.write_conf(d, "D", dtype="bf16", epochs=3)
    env = None if fused else {"HPNN_EVAL_FUSED": "0"}
    out = kb.run(d, "-v", "-V", "1", "-X", "m.txt", cpu=False, env=env).stdout
    assert "batched plan: mode t" in out, out[-3000:]
    got = cc.read_matrix_file(os.path.join(d, "m.txt"))
    Xv, lab = cc.keep_best_held_out("D")
    assert Xv.shape == (f["nv"], 784)
    if fused:
        monkeypatch.delenv("HPNN_EVAL_FUSED", raising=False)
    else:
        monkeypatch.setenv("HPNN_EVAL_FUSED", "0")
    W = [torch.tensor(np.asarray(w)) for w in formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"]]
    m = MLP(f["sizes"], "SNN", batch=f["B"], momentum=True, weights=W, fused="t")
    assert m.plan.eval_is_fused() == fused
    labels = torch.tensor(lab, dtype=torch.int32).cuda()
    guess = m.evaluate(m.prepare_input(torch.tensor(Xv, dtype=torch.float32)), labels=labels, n_valid=f["nv"],
                       guess=True).cpu().numpy()
    want = cc.matrix(guess[:f["nv"]], lab, f["sizes"][-1])
    assert int(np.trace(want[:, :-1])) == kb.records(out)[-1][2], "the plan does not reproduce the engine's last pass"
    assert np.array_equal(got, want), (got, want)
    # a transposed tally would differ: the fixture's matrix is not symmetric
    assert not np.array_equal(want[:, :-1], want[:, :-1].T)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "L"])
def test_f64_engine_matrices_equal_the_cpu_oracles(tmp_path, gpu, name):
    d = str(tmp_path)
    f, Xv, Tv = cc.make_net(d, name)
    cc.write_conf(d, name, dtype="f64")
    for e in range(1, 5):
        cc.run(d, "-e", str(e), "-V", "1", "-X", "cpu.txt")
        # a property of the fixture: no held-out sample near a tie, so the engines cannot disagree
        gap = cc.top2_gap(cc.oracle_outputs(d, name, Xv))
        assert gap > 1e-6, f"fixture {name}, not the kernel, is at fault: the two largest outputs differ by {gap}"
        out = cc.run(d, "-e", str(e), "-V", "1", "-X", "gpu.txt", cpu=False).stdout
        assert "batched GPU training: f64" in out
        want, got = cc.read_matrix_file(os.path.join(d, "cpu.txt")), cc.read_matrix_file(os.path.join(d, "gpu.txt"))
        assert np.array_equal(got, want), (e, got, want)
    # and the per-class record of every pass of one call
    capi.init(0)
    hist = {}
    for dev in ("cpu", "gpu"):
        net = capi.Network(os.path.join(d, "nn.conf")).set(device=dev, validate=1, confusion=True)
        assert net.train()
        hist[dev] = net.class_history()
        assert (net.confusion_launches > 0) == (dev == "gpu")
        net.close()
    assert len(hist["cpu"]) == len(hist["gpu"]) == 4
    for c, g in zip(hist["cpu"], hist["gpu"]):
        assert all(np.array_equal(c[k], g[k]) for k in ("support", "hit", "predicted"))
        assert c["balanced_accuracy"] == g["balanced_accuracy"]


@pytest.mark.gpu
@pytest.mark.parametrize("fx,dtype", [("D", "bf16"), ("A", "f64")])
def test_best_matrix_is_the_kept_pass_after_an_early_stop(tmp_path, gpu, fx, dtype):
    d = str(tmp_path)
    f = kb.make_fixture(d, fx)
    kb.write_conf(d, fx, dtype=dtype)
    out = kb.run(d, "-V", "1", "-K", "acc", "-P", "2", "-X", "best.txt", cpu=False).stdout
    recs, stop, best = kb.records(out), kb.STOP_RE.findall(out), kb.BEST_RE.findall(out)
    assert len(stop) == 1 and len(recs) < f["epochs"], \
        f"fixture {fx}, not the feature, is at fault: -K acc -P 2 does not stop before the last epoch: {recs}"
    b, s = kb.rule(recs, "acc", 2)
    assert int(best[0][0]) == recs[b][0] and int(stop[0][0]) == recs[s][0] and len(recs) == s + 1
    got = cc.read_matrix_file(os.path.join(d, "best.txt"))
    assert int(got.sum()) == f["nv"] and int(np.trace(got[:, :-1])) == recs[b][2]
    # the same engine given the best pass's epochs: its last matrix is the kept one
    kb.run(d, "-e", str(recs[b][0]), "-V", "1", "-X", "short.txt", cpu=False)
    assert np.array_equal(got, cc.read_matrix_file(os.path.join(d, "short.txt")))
    assert len(cc.CLASSES_RE.findall(out)) == len(recs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f64"])
def test_key_off_launches_nothing_and_on_changes_no_weight(tmp_path, gpu, monkeypatch, dtype):
    monkeypatch.delenv("HPNN_FORCE_CPU", raising=False)
    d = str(tmp_path)
    cc.make_net(d, "S")
    cc.write_conf(d, "S", dtype=dtype, epochs=3)
    capi.init(0)
    kernels = {}
    for on in (False, True):
        net = capi.Network(os.path.join(d, "nn.conf")).set(device="gpu", validate=1, confusion=on)
        assert net.train()
        assert (net.confusion_launches == 0) == (not on)
        assert (net.confusion_matrix() is None) == (not on) and (net.class_history() == []) == (not on)
        path = os.path.join(d, f"k{int(on)}.opt")
        net.dump_kernel(path, exact=True)
        kernels[on] = open(path, "rb").read()
        net.close()
    assert kernels[False] == kernels[True]
