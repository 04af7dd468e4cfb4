"""[keep_best] / [patience] on the GPU: the snapshot kernel at its edges (guards, flag read at
run time, captured replays), the decision kernel against its PyTorch emulation bit for bit,
train_nn -K / -P on the BF16 (tile and per-layer plans), FP32 and FP64 engines against the same
engine's run of -e <best epoch>, the FP64 engine against the FP64 CPU oracle, and the Python
plan's keep_best / commit_best / restore_best.

Fixtures: tests/keep_best_common.py.  One graph replay holds 10 epochs of fixture D, 6 of B and
all 32 of C, so the best pass lies inside a replay whose later epochs overwrite its weights.
Observed on an MI355X ([seed] 11, -V 1; best pass b, 0-based, and the pass -P 3 stops at; each
case prints its own): D bf16 (tile plan) b = 4 of 16, stop 7; B bf16 (per-layer) b = 8 of 24,
stop 11; C f32 b = 13 of 32, stop 16; A f64 b = 9 of 24, stop 12 (the CPU oracle's too)."""
import json
import os

import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd._lib import native
from hpnn_amd.models import MLP
from tests import keep_best_common as kb

NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ snapshot_if
GUARD = 16  # bytes on either side of every dst: keeps dst 16-byte aligned


class _Seg:
    """src: random words; dst: a window of a NaN-filled buffer with guard words on both sides"""

    def __init__(self, nbytes, g, f64=False):
        assert nbytes % (8 if f64 else 4) == 0
        words = nbytes // 4
        self.src = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int32, generator=g).cuda()
        if f64:  # a float64 payload: the same bytes seen as doubles
            self.src = self.src.view(torch.float64) if words else torch.zeros(0, dtype=torch.float64, device="cuda")
        total = (2 * GUARD + (nbytes + 15) // 16 * 16) // 4
        self.buf = torch.full((total,), NAN, dtype=torch.float32, device="cuda")
        self.before = self.buf.view(torch.int32).clone()
        win = self.buf.view(torch.int32)[GUARD // 4:GUARD // 4 + words]
        self.dst = win.view(torch.float64) if f64 and words else win
        self.words = words

    def pair(self):
        return self.src, self.dst

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before)

    def copied(self):
        now, lo, hi = self.buf.view(torch.int32), GUARD // 4, GUARD // 4 + self.words
        src = self.src.view(torch.int32) if self.words else self.src.new_zeros(0, dtype=torch.int32)
        return torch.equal(now[lo:hi], src) and torch.equal(now[:lo], self.before[:lo]) and \
            torch.equal(now[hi:], self.before[hi:])


SIZES = [4, 12, 16, 20, 4096 + 4, (1 << 20) + 8, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["each-size-alone", "all-sizes", "32-segments", "f64"])
def test_snapshot_if_at_its_edges(gpu, case):
    g = torch.Generator().manual_seed(len(case))
    if case == "each-size-alone":
        groups = [[_Seg(n, g)] for n in SIZES]
    elif case == "all-sizes":
        groups = [[_Seg(n, g) for n in SIZES]]
    elif case == "32-segments":
        groups = [[_Seg([4, 12, 16, 20, 36, 4096 + 4, 0, 65536 + 8][i % 8], g) for i in range(32)]]
    else:
        groups = [[_Seg(n, g, f64=True) for n in (8, 16, 24, 4096 + 8, (1 << 20) + 8, 0)]]
    take = torch.zeros(1, dtype=torch.int32, device="cuda")
    for segs in groups:
        table = ops.snapshot_table([s.pair() for s in segs])
        assert table.shape == (len(segs), 3)
        take.zero_()
        ops.snapshot_if(table, take)
        torch.cuda.synchronize()
        assert all(s.untouched() for s in segs), "take = 0 wrote something"
        take.fill_(1)
        ops.snapshot_if(table, take)
        torch.cuda.synchronize()
        for s in segs:
            assert s.copied(), f"{s.words * 4} bytes: dst differs from src or a guard word changed"


@pytest.mark.gpu
def test_snapshot_if_refuses_misaligned_pointers_and_launches_nothing(gpu):
    g = torch.Generator().manual_seed(3)
    s = _Seg(64, g)
    take = torch.ones(1, dtype=torch.int32, device="cuda")
    off = s.buf.view(torch.int32)[GUARD // 4 + 1:GUARD // 4 + 1 + 16]  # 4 bytes past a 16-byte boundary
    with pytest.raises(ValueError):
        ops.snapshot_table([(s.src, off)])
    with pytest.raises(ValueError):
        ops.snapshot_table([(s.src[1:], s.dst[1:])])
    nat, table = native(), torch.zeros(2, 3, dtype=torch.int64, device="cuda")
    n = s.src.numel() * 4
    assert nat.snapshot_table(table.data_ptr(), [(s.src.data_ptr(), s.dst.data_ptr() + 4, n - 4)], _stream()) == -1
    assert nat.snapshot_table(table.data_ptr(), [(s.src.data_ptr(), s.dst.data_ptr(), n - 2)], _stream()) == -1
    assert nat.snapshot_table(table.data_ptr() + 8, [(s.src.data_ptr(), s.dst.data_ptr(), n)], _stream()) == -1
    assert nat.snapshot_table(table.data_ptr(), [(s.src.data_ptr(), s.dst.data_ptr(), 4)] * 33, _stream()) == -1
    assert int(table.count_nonzero()) == 0  # a refused table is not written
    good = ops.snapshot_table([s.pair()])
    assert nat.snapshot_if(good.data_ptr() + 8, 1, take.data_ptr(), _stream()) == -1
    assert nat.snapshot_if(good.data_ptr(), 1, take.data_ptr() + 2, _stream()) == -1
    assert nat.snapshot_if(good.data_ptr(), 33, take.data_ptr(), _stream()) == -1
    assert nat.snapshot_if(good.data_ptr(), -1, take.data_ptr(), _stream()) == -1
    assert nat.snapshot_if(0, 1, take.data_ptr(), _stream()) == -1
    # a table filled in by hand with a misaligned dst (inside the buffer): the segment is skipped
    table[0] = torch.tensor([s.src.data_ptr(), s.dst.data_ptr() + 4, 16], dtype=torch.int64)
    assert nat.snapshot_if(table.data_ptr(), 1, take.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert s.untouched()
    assert nat.snapshot_if(0, 0, take.data_ptr(), _stream()) == 0  # no segment: nothing to launch


@pytest.mark.gpu
def test_snapshot_if_reads_the_flag_at_every_replay(gpu):
    g = torch.Generator().manual_seed(5)
    segs = [_Seg(n, g) for n in (20, 4096 + 4, 1 << 16)]
    table = ops.snapshot_table([s.pair() for s in segs])
    take = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.snapshot_if(table, take)  # the code object is loaded before the capture
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        ops.snapshot_if(table, take)
    assert all(s.untouched() for s in segs)  # a capture runs nothing
    take.fill_(1)
    gr.replay()
    torch.cuda.synchronize()
    assert all(s.copied() for s in segs)
    first = [s.src.clone() for s in segs]
    for s in segs:
        s.src.add_(1)
    take.zero_()  # a device write between the replays
    gr.replay()
    torch.cuda.synchronize()
    for s, f in zip(segs, first):
        assert torch.equal(s.dst, f) and not torch.equal(s.dst, s.src), "the second replay copied"


# ------------------------------------------------------------------ best_commit
HISTORIES = [
    ("loss", 0, [(NAN, 9), (NAN, 9), (5.0, 1), (5.0, 7), (NAN, 8), (4.5, 0), (6.0, 9)]),
    ("acc", 0, [(NAN, 3), (2.0, 3), (2.0, 3), (1.5, 3), (9.0, 4), (0.1, 2)]),
    ("acc", 0, [(3.0, 3), (3.0, 3), (2.5, 3), (2.5, 2)]),
    ("loss", 1, [(3.0, 1), (2.0, 1), (2.5, 1), (0.1, 9), (0.0, 9)]),
    ("loss", 3, [(3.0, 1), (2.0, 1), (2.5, 1), (1.9, 1), (2.5, 1), (2.6, 1), (2.7, 1), (0.1, 9), (0.0, 9)]),
    ("acc", 2, [(NAN, 0), (NAN, 0), (NAN, 0), (1.0, 5)]),
    ("loss", 2, [(NAN, 0), (NAN, 0), (1.0, 5)]),  # stops with nothing taken
]


def _hist(recs, dev):
    h = torch.zeros(len(recs) + 1, 2, dtype=torch.float64)
    for i, (loss, hits) in enumerate(recs):
        h[i, 0] = loss
        h[i, 1:2].view(torch.int32)[0] = hits
    return h.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,patience,recs", HISTORIES)
def test_best_commit_kernel_equals_the_emulation_bit_for_bit(gpu, metric, patience, recs):
    states = {}
    for dev in ("cpu", "cuda"):
        hist, cur, st = _hist(recs, dev), torch.zeros(1, dtype=torch.int32, device=dev), ops.best_state(dev)
        st[7] = 1
        ops.best_commit(hist, cur, st, metric, patience)  # an empty history: only the take word is cleared
        out = [st.cpu().clone()]
        for i in range(len(recs)):
            cur.fill_(i + 1)
            ops.best_commit(hist, cur, st, metric, patience)
            out.append(st.cpu().clone())
        states[dev] = out
    assert states["cpu"][0].tolist() == [0] * 8
    for i, (c, d) in enumerate(zip(states["cpu"], states["cuda"])):
        assert torch.equal(c, d), (i, c.tolist(), d.tolist())
    b, s = kb.rule([(i, l, h, 1) for i, (l, h) in enumerate(recs)], metric, patience)
    last = ops.read_best_state(states["cuda"][-1])
    assert (last["index"] if last["valid"] else None) == b and bool(last["stop"]) == (s is not None)
    assert native().best_commit(0, 0, 0, 1, 0, _stream()) == -1
    hist, cur, st = _hist(recs, "cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), ops.best_state("cuda")
    assert native().best_commit(hist.data_ptr(), cur.data_ptr(), st.data_ptr(), 3, 0, _stream()) == -1
    assert native().best_commit(hist.data_ptr(), cur.data_ptr(), st.data_ptr() + 4, 1, 0, _stream()) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("metric,patience", [("loss", 2), ("acc", 0)])
def test_best_commit_captured_behind_validate_commit(gpu, metric, patience):
    passes = [(3.0, 4), (2.0, 4), (2.5, 6), (2.25, 6), (2.75, 1), (0.5, 9)]
    res = {}
    for dev in ("cpu", "cuda"):
        slots = torch.zeros(64, 16, device=dev)
        hist = torch.zeros(len(passes), 2, dtype=torch.float64, device=dev)
        cur, st = torch.zeros(1, dtype=torch.int32, device=dev), ops.best_state(dev)
        if dev == "cuda":
            ops.validate_commit(slots, hist, cur)  # load both code objects, then start over
            ops.best_commit(hist, cur, st, metric, patience)
            torch.cuda.synchronize()
            hist.zero_(), cur.zero_(), st.zero_()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                ops.validate_commit(slots, hist, cur)
                ops.best_commit(hist, cur, st, metric, patience)
        out = []
        for loss, hits in passes:  # the pass's statistics, spread over the slots as a kernel leaves them
            slots[:, 0] = loss / 64
            slots[:, 1:2].view(torch.int32)[:] = 0
            slots[5, 1:2].view(torch.int32)[0] = hits
            if dev == "cuda":
                gr.replay()
            else:
                ops.validate_commit(slots, hist, cur)
                ops.best_commit(hist, cur, st, metric, patience)
            out.append(st.cpu().clone())
        res[dev] = (out, hist.cpu(), int(cur.cpu()[0]))
    assert res["cpu"][2] == res["cuda"][2] == len(passes) and torch.equal(res["cpu"][1], res["cuda"][1])
    for i, (c, d) in enumerate(zip(res["cpu"][0], res["cuda"][0])):
        assert torch.equal(c, d), (i, c.tolist(), d.tolist())
    b, s = kb.rule([(i, l, h, 1) for i, (l, h) in enumerate(passes)], metric, patience)
    last = ops.read_best_state(res["cuda"][0][-1])
    assert last["index"] == b and bool(last["stop"]) == (s is not None)


# ------------------------------------------------------------------ train_nn end to end
CASES = [("D", "bf16", "t"), ("B", "bf16", "-"), ("C", "f32", None), ("A", "f64", None)]
_REF = {}


def _dir(data, tag, fx, dtype):
    d = os.path.join(data, tag)
    os.makedirs(d)
    kb.write_conf(d, fx, dtype=dtype, data=data)
    return d


def _same_records(got, want, dtype):
    """epoch, hits and n exactly; the loss to the ten printed decimals in FP64, and in BF16 /
    FP32 to 1e-4: their loss slots are summed by FP32 atomic adds whose order is not fixed (the
    bound test_validate_gpu.py uses between two runs of one engine)"""
    assert [(r[0], r[2], r[3]) for r in got] == [(r[0], r[2], r[3]) for r in want], (got, want)
    for g, w in zip(got, want):
        assert abs(g[1] - w[1]) <= (1e-12 * abs(w[1]) + 1e-10 if dtype == "f64" else 1e-4 * abs(w[1])), (g, w)


def _ref(tmp_path_factory, fx, dtype, mode):
    """once per case: the plain -V 1 run, the expected best and stop pass from its records, and
    the kernel of the same engine's -e <best epoch> run"""
    if (fx, dtype) not in _REF:
        data = str(tmp_path_factory.mktemp(f"kb_{fx}_{dtype}"))
        kb.make_fixture(data, fx)
        out = kb.run(_dir(data, "plain", fx, dtype), "-v", "-V", "1", cpu=False).stdout
        assert f"batched GPU training: {dtype}" in out, out[-2000:]
        if mode:
            assert f"batched plan: mode {mode}" in out, out[-3000:]
        recs = kb.records(out)
        assert len(recs) == kb.FIXTURES[fx]["epochs"]
        b, s = kb.check_interior(fx, recs, "loss", 3, need_stop=True)
        if dtype != "f64":  # clear of the summation-order noise of _same_records as well
            assert min(r[1] for i, r in enumerate(recs) if i != b) > recs[b][1] * (1 + 2e-4), \
                f"fixture {fx} is at fault: the best loss is within the noise of the runner-up: {recs}"
        de = _dir(data, "short", fx, dtype)
        kb.run(de, "-e", str(b + 1), cpu=False)
        print(f"fixture {fx} {dtype}: best pass {b} (epoch {b + 1}), -P 3 stops at pass {s}; losses "
              f"{[round(r[1], 4) for r in recs]}")
        _REF[(fx, dtype)] = dict(data=data, recs=recs, b=b, s=s, kernel=kb.kernel(de), n=0)
    ref = _REF[(fx, dtype)]
    ref["n"] += 1
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["graph", "eager", "metrics", "patience", "patience-eager"])
@pytest.mark.parametrize("fx,dtype,mode", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_train_nn_keep_best_equals_a_run_of_best_epochs(tmp_path_factory, gpu, fx, dtype, mode, variant):
    ref = _ref(tmp_path_factory, fx, dtype, mode)
    recs, b, s = ref["recs"], ref["b"], ref["s"]
    d = _dir(ref["data"], f"{variant}{ref['n']}", fx, dtype)
    flags = ["-V", "1", "-K", "loss"]
    flags += ["-P", "3"] if variant.startswith("patience") else []
    flags += ["-M", "m.jsonl"] if variant == "metrics" else []  # one replay and one sync per epoch
    env = {"HPNN_GRAPH": "0"} if variant.endswith("eager") else None
    out = kb.run(d, *flags, cpu=False, env=env).stdout
    assert "the best validation pass (loss) is kept" in out
    got = kb.records(out)
    print(f"{fx} {dtype} {variant}: {len(got)} records, {kb.BEST_RE.findall(out)}, {kb.STOP_RE.findall(out)}")
    _same_records(got, recs[:s + 1] if variant.startswith("patience") else recs, dtype)
    best = kb.BEST_RE.findall(out)
    assert len(best) == 1 and (int(best[0][0]), int(best[0][2]), int(best[0][3])) == (b + 1, recs[b][2], recs[b][3])
    if variant.startswith("patience"):
        assert kb.STOP_RE.findall(out) == [(str(recs[s][0]), "3")], out[-1500:]
    else:
        assert "EARLY STOP" not in out
    assert kb.kernel(d) == ref["kernel"], "kernel.opt differs from the -e <best epoch> run's"
    if variant == "metrics":
        names = [json.loads(l)["event"] for l in open(os.path.join(d, "m.jsonl"))]
        assert names.count("validation") == len(recs) and names.count("best") == 1
        assert max(i for i, n in enumerate(names) if n == "validation") < names.index("best")


@pytest.mark.gpu
def test_train_nn_keep_best_resumes_like_the_short_run(tmp_path_factory, gpu):
    """momentum and epoch numbering on the tile plan: two more epochs from either state file"""
    ref = _ref(tmp_path_factory, "D", "bf16", "t")
    b = ref["b"]
    kernels = []
    for tag, flags in (("rk", ["-V", "1", "-K", "loss"]), ("re", ["-V", "1", "-e", str(b + 1)])):
        d = _dir(ref["data"], f"{tag}{ref['n']}", "D", "bf16")
        kb.run(d, *flags, "-r", "state.bin", cpu=False)
        more = kb.records(kb.run(d, "-V", "1", "-e", "2", "-r", "state.bin", cpu=False).stdout)
        assert [r[0] for r in more] == [b + 2, b + 3], more
        kernels.append(kb.kernel(d))
    assert kernels[0] == kernels[1]


@pytest.mark.gpu
def test_f64_engine_agrees_with_the_cpu_oracle(tmp_path, gpu, monkeypatch):
    monkeypatch.delenv("HPNN_FORCE_CPU", raising=False)
    d = str(tmp_path)
    kb.make_fixture(d, "A")
    kb.write_conf(d, "A", dtype="f64")
    capi.init(0)
    res = {}
    for dev in ("cpu", "gpu"):
        for patience in (0, 3):
            net = capi.Network(os.path.join(d, "nn.conf")).set(device=dev, validate=1, keep_best="loss",
                                                                patience=patience)
            assert net.train()
            res[dev, patience] = (net.best(), net.validation(), net.epochs_done)
            net.close()
    full = res["cpu", 0][1]
    order = sorted(r["loss"] for r in full)
    assert order[1] - order[0] > 1e-9 * order[0], "fixture A is at fault: the oracle's best loss is not clear"
    rl = [(r["epoch"], r["loss"], r["correct"], r["n"]) for r in full]
    b, s = kb.check_interior("A", rl, "loss", 3, need_stop=True)
    for patience in (0, 3):
        (cb, cr, cd), (gb, gr, gd) = res["cpu", patience], res["gpu", patience]
        print(f"patience {patience}: cpu best {cb} of {len(cr)}; gpu best {gb} of {len(gr)}")
        assert cb["epoch"] == gb["epoch"] == b + 1 == cd == gd
        assert len(cr) == len(gr) == (s + 1 if patience else 24)  # the same stop epoch
        for g, c in zip(gr, cr):
            assert g["epoch"] == c["epoch"] and g["correct"] == c["correct"]
            assert abs(g["loss"] - c["loss"]) <= 1e-12 * abs(c["loss"]), (g, c)
        assert gb["correct"] == cb["correct"] and abs(gb["loss"] - cb["loss"]) <= 1e-12 * abs(cb["loss"])


# ------------------------------------------------------------------ the Python plan
@pytest.mark.gpu
@pytest.mark.parametrize("sizes,Bp,fused", [([784, 128, 64, 10], 256, "t"), ([20, 16, 8, 5], 128, False)])
def test_mlp_restore_best_gives_the_middle_pass(gpu, sizes, Bp, fused):
    g = torch.Generator().manual_seed(8)
    m = MLP(sizes, "SNN", batch=Bp, momentum=True, seed=3, fused=fused)
    assert m.fused_mode == (fused or None)
    X = m.prepare_input((torch.rand(Bp, sizes[0], generator=g) - 0.5).cuda())
    lab = torch.randint(0, sizes[-1], (Bp,), dtype=torch.int32, generator=g).cuda()
    m.keep_best("loss", 0)
    hist = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")
    vst = m.buf[("vstats", -1)]
    digests, V, W = [], [], []
    # two steps down the gradient of the batch that is also evaluated, then one far up it
    for lr in (0.5, 0.5, -4.0):
        m.train_step(X, labels=lab, lr=lr, alpha=0.2)
        m.evaluate(X, labels=lab, n_valid=Bp)
        ops.validate_commit(vst, hist, cur)
        m.commit_best(hist, cur)
        digests.append(m.weights_digest())
        V.append([v.clone() for v in m.V32])
        W.append([w.clone() for w in m.W32])
    losses = hist[:3, 0].tolist()
    print("losses", losses, "digests", digests)
    assert losses[1] < losses[0] and losses[1] < losses[2], f"the schedule, not the feature, is at fault: {losses}"
    st = m.best_state()
    assert (st["valid"], st["index"], st["stale"], st["stop"], st["take"]) == (1, 1, 1, 0, 0)
    assert st["loss_sum"] == losses[1]
    assert m.weights_digest() == digests[2] != digests[1]
    assert m.restore_best() is True
    assert m.weights_digest() == digests[1]
    for l in range(len(sizes) - 1):
        assert torch.equal(m.V32[l], V[1][l]) and torch.equal(m.W32[l], W[1][l])
    assert m.healthy()
    m2 = MLP(sizes, "SNN", batch=Bp, momentum=True, seed=3, fused=fused)
    m2.keep_best("acc", 2)
    before = m2.weights_digest()
    assert m2.restore_best() is False and m2.weights_digest() == before and m2.best_state()["valid"] == 0
