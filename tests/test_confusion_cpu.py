"""[confusion] on the CPU: the rule (numpy reference, the PyTorch emulations of ops.confusion_add /
confusion_commit / balanced_accuracy, the C header), the FP64 CPU batched engine -- the oracle --
against an independent FP64 PyTorch forward of the dumped weights, the -X file, run_nn, the
"classes" metrics event, the conf key and its preconditions.

Every expected value is an integer count: every comparison is exact."""
import os
import re

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd._lib import native
from hpnn_amd.utils import formats
from tests import confusion_common as cc
from tests import keep_best_common as kb


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("case", cc.RULE_CASES, ids=[c[0] for c in cc.RULE_CASES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rule_cases_numpy_and_emulation(case, dtype):
    _, n_out, guess, T, want = case
    want = np.array(want, dtype=np.uint32)
    T = np.array(T, dtype=np.float64)
    assert np.array_equal(cc.matrix(guess, cc.target_class(T), n_out), want)
    M = ops.confusion_matrix(n_out)
    ops.confusion_add(torch.tensor(guess, dtype=torch.int32), M, T=torch.tensor(T, dtype=dtype))
    assert np.array_equal(M.numpy().view(np.uint32), want)
    # labels in place of the dense rows: the same cells
    M2 = ops.confusion_matrix(n_out)
    ops.confusion_add(torch.tensor(guess, dtype=torch.int32), M2,
                      labels=torch.tensor(cc.target_class(T), dtype=torch.int32))
    assert torch.equal(M, M2)


def test_emulation_edges_accumulate_and_commit():
    n_out = 3
    M = ops.confusion_matrix(n_out)
    g = torch.tensor([0, 1, 2, 1, -1, cc.GUESS_NONE], dtype=torch.int32)
    lab = torch.tensor([0, 1, 1, 7, 2, 2], dtype=torch.int32)  # 7: out of range, skipped
    ops.confusion_add(g, M, labels=lab, rows=0)  # n_valid = 0: nothing
    assert int(M.abs().sum()) == 0
    ops.confusion_add(g, M, labels=lab, rows=3)
    ops.confusion_add(g[3:], M, labels=lab[3:])  # a second chunk accumulates
    want = cc.matrix(g.tolist(), lab.tolist(), n_out)
    assert np.array_equal(M.numpy().view(np.uint32), want) and int(want.sum()) == 4
    # ldt > n_out: the columns past n_out are not read
    T = torch.tensor([[0.0, 1.0, 0.0, 9.0], [1.0, 0.0, 0.0, 9.0]], dtype=torch.float64)
    M3 = ops.confusion_matrix(n_out)
    ops.confusion_add(torch.tensor([1, 1], dtype=torch.int32), M3, T=T)
    assert M3[1, 1] == 1 and M3[0, 1] == 1 and int(M3.sum()) == 2
    # two passes file two records at the indices the cursor walks; a full history drops the third
    hist, last, cur = torch.full((2, 3 * n_out), -1, dtype=torch.int32), ops.confusion_matrix(n_out), \
        torch.zeros(1, dtype=torch.int32)
    ops.confusion_commit(M, hist, last, cur)
    assert int(M.abs().sum()) == 0 and np.array_equal(last.numpy().view(np.uint32), want)
    rec = cc.class_record(want)
    got = ops.class_record(hist, 0)
    assert all(got[k] == rec[k].tolist() for k in rec)
    cur[0] = 1
    ops.confusion_add(g, M, labels=lab, rows=2)
    ops.confusion_commit(M, hist, last, cur)
    assert ops.class_record(hist, 1)["hit"] == [1, 1, 0] and int(last.sum()) == 2
    cur[0] = 2
    before = hist.clone()
    ops.confusion_add(g, M, labels=lab, rows=1)
    ops.confusion_commit(M, hist, last, cur)
    assert torch.equal(hist, before) and int(last.sum()) == 1 and int(M.abs().sum()) == 0


def test_balanced_accuracy_python_numpy_and_c_agree_bitwise():
    rng = np.random.default_rng(5)
    cases = [([0, 0, 0], [0, 0, 0]), ([3, 0, 7], [1, 0, 7]), ([1], [1]), ([10, 3, 3, 0, 9], [9, 1, 2, 0, 0])]
    for _ in range(20):
        s = rng.integers(0, 50, 11)
        cases.append((s.tolist(), (rng.integers(0, 51, 11) % (s + 1)).tolist()))
    for s, h in cases:
        a, b, c = ops.balanced_accuracy(s, h), cc.balanced_accuracy(s, h), native().balanced_accuracy(s, h)
        assert np.float64(a).tobytes() == np.float64(b).tobytes() == np.float64(c).tobytes(), (s, h, a, b, c)
        assert native().worst_class(s, h) == cc.worst_class(s, h)
    assert ops.balanced_accuracy([0, 0], [0, 0]) == 0.0
    assert ops.balanced_accuracy([3, 0, 7], [1, 0, 7]) == (0.0 + 1.0 / 3.0 + 1.0) / 2.0
    assert cc.worst_class([4, 0, 2, 8], [2, 0, 1, 4]) == 0  # 2/4 = 1/2 = 4/8: the lowest index


# ------------------------------------------------------------------ the CPU engine, the oracle
@pytest.fixture(scope="module", params=["S", "L"])
def trained(request, tmp_path_factory):
    """-V 1 -X over 4 epochs, and the same run cut at every epoch: the weights of every pass"""
    name = request.param
    d = str(tmp_path_factory.mktemp("cf" + name))
    f, Xv, Tv = cc.make_net(d, name)
    cc.write_conf(d, name)
    per_epoch = []
    for e in range(1, 5):
        r = cc.run(d, "-e", str(e), "-V", "1", "-X", "m.txt")
        per_epoch.append((cc.read_matrix_file(os.path.join(d, "m.txt")), cc.oracle_matrix(d, name, Xv, Tv), r.stdout))
    r = cc.run(d, "-V", "1", "-X", "m.txt", "-M", "metrics.jsonl")
    return dict(d=d, name=name, f=f, Xv=Xv, Tv=Tv, per_epoch=per_epoch, out=r.stdout,
                events=cc.classes_events(os.path.join(d, "metrics.jsonl")))


def test_cpu_engine_matrix_of_every_pass_equals_the_independent_forward(trained):
    nv = trained["f"]["nv"]
    for e, (got, want, out) in enumerate(trained["per_epoch"], 1):
        assert np.array_equal(got, want), (e, got, want)
        assert int(got.sum()) == nv
        recs = kb.records(out)
        assert len(recs) == e and int(np.trace(got[:, :-1])) == recs[-1][2]


def test_cpu_engine_classes_lines_and_events(trained):
    recs = kb.records(trained["out"])
    lines = cc.CLASSES_RE.findall(trained["out"])
    events = trained["events"]
    assert len(recs) == len(lines) == len(events) == 4
    # every VALIDATION line is followed by its CLASSES line
    assert re.findall(r"NN: (VALIDATION|CLASSES):", trained["out"]) == ["VALIDATION", "CLASSES"] * 4
    for i, (_, want, _) in enumerate(trained["per_epoch"]):
        rec = cc.class_record(want)
        ev = events[i]
        assert ev["epoch"] == recs[i][0] == int(lines[i][0]) and ev["engine"] == "cpu"
        assert all(ev[k] == rec[k].tolist() for k in rec)
        assert sum(ev["hit"]) == recs[i][2] and sum(ev["support"]) == trained["f"]["nv"]
        bacc = cc.balanced_accuracy(rec["support"], rec["hit"])
        assert ev["balanced_accuracy"] == bacc and lines[i][1] == f"{bacc:.10f}"
        w = cc.worst_class(rec["support"], rec["hit"])
        assert (int(lines[i][2]), int(lines[i][3]), int(lines[i][4])) == (w, rec["hit"][w], rec["support"][w])


def test_keep_best_matrix_is_the_kept_pass_and_the_file_round_trips(trained):
    d, name = trained["d"], trained["name"]
    capi.init(0)
    net = capi.Network(os.path.join(d, "nn.conf"))
    net.set(device="cpu", validate=1, keep_best="loss", confusion=True)
    assert net.confusion and net.train()
    b = [r["epoch"] for r in net.validation()].index(net.best()["epoch"])
    best, last = net.confusion_matrix("best"), net.confusion_matrix("last")
    assert np.array_equal(best, trained["per_epoch"][b][1]) and np.array_equal(last, trained["per_epoch"][3][1])
    hist = net.class_history()
    assert len(hist) == 4 and net.confusion_launches == 0
    for i, h in enumerate(hist):
        rec = cc.class_record(trained["per_epoch"][i][1])
        assert all(np.array_equal(h[k], rec[k]) for k in rec)
        assert h["balanced_accuracy"] == cc.balanced_accuracy(rec["support"], rec["hit"])
    # at most max_cells cells are copied
    part = np.full(7, 0xffffffff, dtype=np.uint32)
    assert net.L.nn_get_confusion_matrix(net.ptr, 0, 3, part.ctypes.data) == last.shape[0]
    assert part[:3].tolist() == last.reshape(-1)[:3].tolist() and (part[3:] == 0xffffffff).all()
    path = os.path.join(d, "best.txt")
    net.dump_confusion_matrix(path, "best")
    assert np.array_equal(cc.read_matrix_file(path), best)
    net.close()
    # train_nn -K loss -X writes the best pass's matrix and names the same pass
    r = cc.run(d, "-V", "1", "-K", "loss", "-X", "k.txt")
    e = int(kb.BEST_RE.search(r.stdout).group(1))
    assert e == b + 1 and np.array_equal(cc.read_matrix_file(os.path.join(d, "k.txt")), best)


def test_run_nn_matrix_is_the_tally_of_its_pass_fail_lines(trained):
    d = trained["d"]
    n_out = trained["f"]["sizes"][-1]
    cc.run(d, "-e", "2")
    formats.write_conf(os.path.join(d, "run.conf"), name="cf", type=trained["f"]["type"], init="kernel.opt",
                       seed=cc.SEED, train="BPM", sample_dir=os.path.join(d, "train.hpnb"),
                       test_dir=os.path.join(d, "val.hpnb"))
    e = dict(os.environ)
    import subprocess
    r = subprocess.run([os.path.join(kb.BIN, "run_nn"), "-c", "-vv", "-X", "r.txt", "run.conf"], cwd=d, env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plain = subprocess.run([os.path.join(kb.BIN, "run_nn"), "-c", "-vv", "run.conf"], cwd=d, env=e,
                           capture_output=True, text=True, timeout=300)
    assert plain.stdout == r.stdout  # the PASS / FAIL lines do not change
    want = np.zeros((n_out, n_out + 1), dtype=np.uint32)
    lines = [ln for ln in r.stdout.split("\n") if "TESTING FILE" in ln]
    assert len(lines) == trained["f"]["nv"]
    for ln in lines:
        g = int(cc.BESTCLASS_RE.search(ln).group(1)) - 1
        m = cc.RUN_RE.search(ln)
        t = g if m.group(1) else int(m.group(2)) - 1
        want[t, g] += 1
    assert np.array_equal(cc.read_matrix_file(os.path.join(d, "r.txt")), want)


# ------------------------------------------------------------------ the key and its preconditions
KW = dict(name="s", type="SNN", seed=3, inputs=6, hiddens=[4], outputs=3, train="BP", sample_dir="./s",
          test_dir="./s", mode="batched")


def test_conf_key_is_dumped_only_when_on_and_bad_values_fail(tmp_path, capfd):
    d = str(tmp_path)
    capi.init(0)
    for value, on in (("on", True), ("ON", True), ("off", False), (None, False)):
        extra = {} if value is None else dict(confusion=value)
        formats.write_conf(os.path.join(d, "a.conf"), **extra, **KW)
        net = capi.Network(os.path.join(d, "a.conf"))
        assert net.confusion is on
        net.dump_conf(os.path.join(d, "a2.conf"))
        txt = open(os.path.join(d, "a2.conf")).read()
        assert ("[confusion] on\n" in txt) is on and ("confusion" in txt) is on
        assert net.confusion_matrix() is None and net.class_history() == []
        net.set(confusion=not on)
        assert net.confusion is (not on)
        net.close()
    capfd.readouterr()
    for bad in ("yes", "", "1"):
        formats.write_conf(os.path.join(d, "c.conf"), confusion=bad, **KW)
        with pytest.raises(RuntimeError):
            capi.Network(os.path.join(d, "c.conf"))
        err = capfd.readouterr().err
        assert "NN(ERR): Malformed NN configuration file!\n" in err
        assert f"NN(ERR): [confusion] unknown: {bad} (on | off)\n" in err


def test_confusion_without_validate_is_refused_with_status_1(tmp_path):
    d = str(tmp_path)
    cc.make_net(d, "S")
    cc.write_conf(d, "S", epochs=2)
    r = cc.run(d, "-X", "m.txt", check=False)
    assert r.returncode == 1 and "[confusion] needs [validate]" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(d, "m.txt")) and "CLASSES:" not in r.stdout
    assert "-X F" in cc.run(d, "-h").stdout


def test_online_mode_warns_once(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(2)
    os.makedirs(os.path.join(d, "samples"))
    for i in range(3):
        t = np.zeros(3)
        t[i] = 1.0
        formats.write_sample(os.path.join(d, "samples", f"s{i}"), rng.uniform(-1, 1, 4), t)
    formats.write_conf(os.path.join(d, "nn.conf"), name="o", type="SNN", seed=3, inputs=4, hiddens=[5], outputs=3,
                       train="BP", sample_dir="./samples", test_dir="./samples", confusion="on")
    r = cc.run(d)
    assert r.stderr.count("[confusion] has no effect in online mode (ignored)") == 1
    assert "TRAINING FILE" in r.stdout and "CLASSES:" not in r.stdout
    # -X there: the training goes well, there is no matrix and no file, and that is said, not failed
    formats.write_conf(os.path.join(d, "nn.conf"), name="o", type="SNN", seed=3, inputs=4, hiddens=[5], outputs=3,
                       train="BP", sample_dir="./samples", test_dir="./samples")
    r = cc.run(d, "-X", "m.txt")
    assert r.returncode == 0 and "tallied no confusion matrix" in r.stderr and "FAILED" not in r.stderr
    assert not os.path.exists(os.path.join(d, "m.txt"))
