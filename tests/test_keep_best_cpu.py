"""[keep_best] loss | acc and [patience] P on the CPU: the conf keys and the -K / -P flags, the
preconditions, the PyTorch emulations of the two device launches (ops.best_commit,
ops.snapshot_if), and the FP64 CPU batched engine -- the oracle -- on fixture A
(tests/keep_best_common.py): a keep-best run returns, bit for bit and for an exact resume, what a
run given -e <best epoch> returns.

Observed with the CPU engine ([seed] 11; pass index b, 0-based, of 24 passes with -V 1):
fixture A -K loss b = 9 (epoch 10), with -R b = 10; -K acc b = 14 (hits tie with pass 3, the
loss breaks it); -P 3 stops at pass 12 (-V 1) and at pass 7 = epoch 16 (-V 2, best pass 4)."""
import json
import os

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.utils import formats
from tests import keep_best_common as kb


# ------------------------------------------------------------------ conf and CLI
KW = dict(name="s", type="SNN", seed=3, inputs=6, hiddens=[4], outputs=3, train="BP", sample_dir="./s",
          test_dir="./s", mode="batched")


def test_conf_round_trip_defaults_and_bad_values(tmp_path):
    d = str(tmp_path)
    capi.init(0)
    formats.write_conf(os.path.join(d, "a.conf"), validate=2, keep_best="acc", patience=4, **KW)
    net = capi.Network(os.path.join(d, "a.conf"))
    assert net.keep_best == "acc" and net.patience == 4
    net.dump_conf(os.path.join(d, "a2.conf"))
    net.close()
    txt = open(os.path.join(d, "a2.conf")).read()
    assert "[keep_best] acc\n" in txt and "[patience] 4\n" in txt
    net = capi.Network(os.path.join(d, "a2.conf"))
    assert net.keep_best == "acc" and net.patience == 4
    net.set(keep_best="loss", patience=0)
    assert net.keep_best == "loss" and net.patience == 0 and net.best() is None
    net.set(keep_best="off")
    assert net.keep_best == "off"
    net.close()
    formats.write_conf(os.path.join(d, "b.conf"), **KW)
    net = capi.Network(os.path.join(d, "b.conf"))
    assert net.keep_best == "off" and net.patience == 0
    net.dump_conf(os.path.join(d, "b2.conf"))
    net.close()
    txt = open(os.path.join(d, "b2.conf")).read()
    assert "keep_best" not in txt and "patience" not in txt
    for bad in (dict(keep_best="best"), dict(keep_best=""), dict(keep_best="1"), dict(patience="0"),
                dict(patience="x")):
        formats.write_conf(os.path.join(d, "c.conf"), **bad, **KW)
        with pytest.raises(RuntimeError):
            capi.Network(os.path.join(d, "c.conf"))


def test_cli_flags(tmp_path):
    d = str(tmp_path)
    kb.make_fixture(d, "A")
    kb.write_conf(d, "A")
    for flags in (("-K",), ("-K", "x"), ("-K", "1"), ("-P",), ("-P", "x"), ("-P", "0"), ("-P", "-2")):
        r = kb.run(d, *flags, check=False)
        assert r.returncode != 0 and "syntax error" in r.stderr, (flags, r.stdout, r.stderr)
    for flags in (("-K", "loss"), ("-P", "2")):
        r = kb.run(d, *flags, tool="run_nn", check=False)
        assert r.returncode != 0 and "syntax error" in r.stderr, (flags, r.stdout + r.stderr)
    r = kb.run(d, "-h")
    assert "-K M" in r.stdout and "-P P" in r.stdout and "loss | acc" in r.stdout


def test_preconditions_fail_the_call(tmp_path):
    d = str(tmp_path)
    kb.make_fixture(d, "A")
    kb.write_conf(d, "A", epochs=2)
    r = kb.run(d, "-K", "loss", check=False)
    assert r.returncode != 0 and "[keep_best]" in r.stderr and "[validate]" in r.stderr, r.stdout + r.stderr
    assert "BEST:" not in r.stdout
    r = kb.run(d, "-V", "1", "-P", "2", check=False)
    assert r.returncode != 0 and "[patience]" in r.stderr and "[keep_best]" in r.stderr, r.stdout + r.stderr
    assert "VALIDATION:" not in r.stdout


def test_online_mode_warns_once_each_and_trains(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(2)
    os.makedirs(os.path.join(d, "samples"))
    for i in range(3):
        t = np.zeros(3)
        t[i] = 1.0
        formats.write_sample(os.path.join(d, "samples", f"s{i}"), rng.uniform(-1, 1, 4), t)
    formats.write_conf(os.path.join(d, "nn.conf"), name="o", type="SNN", seed=3, inputs=4, hiddens=[5], outputs=3,
                       train="BP", sample_dir="./samples", test_dir="./samples", keep_best="loss", patience=2)
    r = kb.run(d)
    assert r.stderr.count("[keep_best] has no effect in online mode (ignored)") == 1
    assert r.stderr.count("[patience] has no effect in online mode (ignored)") == 1
    assert "TRAINING FILE" in r.stdout and "BEST:" not in r.stdout


# ------------------------------------------------------------------ rule emulation
def _hist(recs):
    h = torch.zeros(len(recs) + 1, 2, dtype=torch.float64)
    for i, (loss, hits) in enumerate(recs):
        h[i, 0] = loss
        h[i, 1:2].view(torch.int32)[0] = hits
    return h


def _walk(recs, metric, patience=0):
    """best_commit after each record: the states [(index, stale, stop, valid, take, hits, loss)]"""
    hist, cur, st = _hist(recs), torch.zeros(1, dtype=torch.int32), ops.best_state()
    out = []
    for i in range(len(recs)):
        cur[0] = i + 1
        ops.best_commit(hist, cur, st, metric, patience)
        s = ops.read_best_state(st)
        out.append((s["index"], s["stale"], s["stop"], s["valid"], s["take"], s["hits"], s["loss_sum"]))
    return out


NAN = float("nan")


def test_rule_first_pass_ties_and_nan_under_loss():
    w = _walk([(NAN, 9), (NAN, 9), (5.0, 1), (5.0, 7), (NAN, 8), (4.5, 0), (6.0, 9)], "loss")
    assert [x[:5] for x in w] == [(0, 1, 0, 0, 0), (0, 2, 0, 0, 0),  # a NaN is not taken, even first
                                  (2, 0, 0, 1, 1),                   # the first pass with a number
                                  (2, 1, 0, 1, 0),                   # a tie does not improve
                                  (2, 2, 0, 1, 0),                   # a NaN does not improve
                                  (5, 0, 0, 1, 1), (5, 1, 0, 1, 0)]
    assert w[-1][5:] == (0, 4.5)


def test_rule_acc_takes_the_first_pass_and_breaks_ties_by_loss():
    w = _walk([(NAN, 3), (2.0, 3), (2.0, 3), (1.5, 3), (9.0, 4), (0.1, 2)], "acc")
    assert [x[:5] for x in w] == [(0, 0, 0, 1, 1),   # the first pass at all, NaN or not
                                  (0, 1, 0, 1, 0),   # same hits, 2.0 < NaN is false
                                  (0, 2, 0, 1, 0), (0, 3, 0, 1, 0),
                                  (4, 0, 0, 1, 1),   # more hits win whatever the loss
                                  (4, 1, 0, 1, 0)]
    w = _walk([(3.0, 3), (3.0, 3), (2.5, 3), (2.5, 2)], "acc")
    assert [x[:5] for x in w] == [(0, 0, 0, 1, 1), (0, 1, 0, 1, 0), (2, 0, 0, 1, 1), (2, 1, 0, 1, 0)]


@pytest.mark.parametrize("patience,recs,stop_at", [
    (1, [(3.0, 1), (2.0, 1), (2.5, 1), (0.1, 9), (0.0, 9)], 2),
    # an improvement at pass 3 resets the count; passes 4, 5, 6 are stale
    (3, [(3.0, 1), (2.0, 1), (2.5, 1), (1.9, 1), (2.5, 1), (2.6, 1), (2.7, 1), (0.1, 9), (0.0, 9)], 6),
])
def test_rule_patience_stops_and_freezes(patience, recs, stop_at):
    w = _walk(recs, "loss", patience)
    assert [x[2] for x in w] == [0] * stop_at + [1] * (len(recs) - stop_at)
    assert w[stop_at][1] == patience and w[stop_at - 1][1] == patience - 1 and w[stop_at][4] == 0
    # frozen: the better passes behind the stop change nothing and are not taken
    assert all(x == w[stop_at] for x in w[stop_at:])
    assert kb.rule([(i, l, h, 1) for i, (l, h) in enumerate(recs)], "loss", patience) == (w[-1][0], stop_at)


def test_rule_empty_history_is_a_no_op():
    st = ops.best_state()
    st[7] = 1  # a stale take word is cleared, nothing else moves
    ops.best_commit(_hist([(1.0, 1)]), torch.zeros(1, dtype=torch.int32), st, "loss", 1)
    assert st.tolist() == [0] * 8
    with pytest.raises((ValueError, KeyError)):
        ops.best_commit(_hist([(1.0, 1)]), torch.ones(1, dtype=torch.int32), st, "best")


def test_rule_emulation_agrees_with_the_written_out_rule():
    rng = np.random.default_rng(7)
    for metric in ("loss", "acc"):
        for patience in (0, 1, 2, 4):
            recs = [(float(rng.integers(0, 6)) if rng.random() > 0.15 else NAN, int(rng.integers(0, 4)))
                    for _ in range(40)]
            w = _walk(recs, metric, patience)
            b, s = kb.rule([(i, l, h, 1) for i, (l, h) in enumerate(recs)], metric, patience)
            assert (w[-1][0] if w[-1][3] else None) == b
            assert ([x[2] for x in w].index(1) if w[-1][2] else None) == s


# ------------------------------------------------------------------ snapshot emulation
def test_snapshot_emulation_copies_only_when_the_flag_is_set():
    g = torch.Generator().manual_seed(1)
    src = [torch.rand(3, 5, generator=g), torch.rand(7, generator=g).double(), torch.zeros(0)]
    dst = [torch.full_like(t, 7.0) for t in src]
    table = ops.snapshot_table(list(zip(src, dst)))
    take = torch.zeros(1, dtype=torch.int32)
    ops.snapshot_if(table, take)
    assert all(bool((d == 7.0).all()) for d in dst)
    take[0] = 1
    ops.snapshot_if(table, take)
    assert all(torch.equal(s, d) for s, d in zip(src, dst))
    with pytest.raises(ValueError):
        ops.snapshot_table([(torch.zeros(4), torch.zeros(5))])
    with pytest.raises(ValueError):
        ops.snapshot_table([(torch.zeros(1), torch.zeros(1))] * 33)


# ------------------------------------------------------------------ CPU engine, fixture A
def _dir(tmp_path, tag, data, **extra):
    d = str(tmp_path / tag)
    os.makedirs(d)
    kb.write_conf(d, "A", data=data, **extra)
    return d


@pytest.mark.parametrize("metric", ["loss", "acc"])
@pytest.mark.parametrize("flags", [(), ("-R",)], ids=["once", "R"])
def test_cpu_engine_keep_best_equals_a_run_of_best_epochs(tmp_path, metric, flags):
    data = str(tmp_path)
    kb.make_fixture(data, "A")
    plain = kb.records(kb.run(_dir(tmp_path, "plain", data), "-V", "1", *flags).stdout)
    assert len(plain) == 24
    b, _ = kb.check_interior("A", plain, metric)
    dk = _dir(tmp_path, "keep", data)
    out = kb.run(dk, "-V", "1", "-K", metric, "-r", "state.bin", *flags).stdout
    assert kb.records(out) == plain
    assert kb.BEST_RE.findall(out) == [(str(b + 1), f"{plain[b][1]:.10f}", str(plain[b][2]), "23")], out[-1500:]
    assert "EARLY STOP" not in out
    de = _dir(tmp_path, "short", data)
    kb.run(de, "-V", "1", "-e", str(b + 1), "-r", "state.bin", *flags)
    assert kb.kernel(dk) == kb.kernel(de)
    # momentum and epoch numbering: two more epochs from either state file
    for d in (dk, de):
        more = kb.records(kb.run(d, "-V", "1", "-e", "2", "-r", "state.bin", *flags).stdout)
        assert [r[0] for r in more] == [b + 2, b + 3], more
    assert kb.kernel(dk) == kb.kernel(de)


@pytest.mark.parametrize("every", [1, 2])
def test_cpu_engine_patience_counts_passes(tmp_path, every):
    data = str(tmp_path)
    kb.make_fixture(data, "A")
    plain = kb.records(kb.run(_dir(tmp_path, "plain", data), "-V", str(every)).stdout)
    b, s = kb.check_interior("A", plain, "loss", 3, need_stop=True)
    assert s == b + 3  # the loss rises monotonically behind the minimum: three passes, not epochs
    dk = _dir(tmp_path, "keep", data)
    out = kb.run(dk, "-V", str(every), "-K", "loss", "-P", "3").stdout
    assert kb.records(out) == plain[:s + 1]
    assert kb.BEST_RE.findall(out)[0][0] == str(plain[b][0])
    assert kb.STOP_RE.findall(out) == [(str(plain[s][0]), "3")], out[-1500:]
    assert out.index("VALIDATION: epoch %d " % plain[s][0]) < out.index("BEST:") < out.index("EARLY STOP:")
    de = _dir(tmp_path, "short", data)
    kb.run(de, "-e", str(plain[b][0]))
    assert kb.kernel(dk) == kb.kernel(de)


def test_conf_keys_act_like_the_flags(tmp_path):
    data = str(tmp_path)
    kb.make_fixture(data, "A")
    a = kb.run(_dir(tmp_path, "flags", data), "-V", "1", "-K", "loss", "-P", "3").stdout
    b = kb.run(_dir(tmp_path, "keys", data, validate=1, keep_best="loss", patience=3)).stdout
    assert kb.records(a) == kb.records(b) and kb.BEST_RE.findall(a) == kb.BEST_RE.findall(b)
    assert kb.STOP_RE.findall(a) == kb.STOP_RE.findall(b) != []
    assert kb.kernel(str(tmp_path / "flags")) == kb.kernel(str(tmp_path / "keys"))


def test_metrics_hold_best_and_early_stop_after_the_last_validation(tmp_path):
    data = str(tmp_path)
    kb.make_fixture(data, "A")
    d = _dir(tmp_path, "m", data)
    out = kb.run(d, "-V", "1", "-K", "loss", "-P", "3", "-M", "m.jsonl").stdout
    recs = kb.records(out)
    ev = [json.loads(l) for l in open(os.path.join(d, "m.jsonl"))]
    names = [e["event"] for e in ev]
    last_val = max(i for i, n in enumerate(names) if n == "validation")
    assert names.count("validation") == len(recs) and names.count("best") == 1 and names.count("early_stop") == 1
    assert last_val < names.index("best") < names.index("early_stop")
    be, es = ev[names.index("best")], ev[names.index("early_stop")]
    b, s = kb.rule(recs, "loss", 3)
    assert s == len(recs) - 1
    assert (be["epoch"], be["correct"], be["n"], be["metric"]) == (recs[b][0], recs[b][2], 23, "loss")
    assert abs(be["loss"] - recs[b][1]) <= 1e-9 and (es["epoch"], es["patience"]) == (recs[s][0], 3)
    # without a stop there is no early_stop event
    d2 = _dir(tmp_path, "m2", data)
    kb.run(d2, "-V", "1", "-K", "loss", "-M", "m.jsonl")
    names = [json.loads(l)["event"] for l in open(os.path.join(d2, "m.jsonl"))]
    assert names.count("best") == 1 and "early_stop" not in names


def test_network_api_best_equals_the_printed_line(tmp_path, capfd):
    data = str(tmp_path)
    kb.make_fixture(data, "A")
    d = _dir(tmp_path, "api", data, device="cpu")
    capi.init(2)
    try:
        net = capi.Network(os.path.join(d, "nn.conf")).set(validate=1, keep_best="loss", patience=3)
        assert net.best() is None
        assert net.train()
        best, recs, done = net.best(), net.validation(), net.epochs_done
        # the best is per call: a call without keep_best clears it
        net.set(keep_best="off", patience=0, epochs=1)
        assert net.train() and net.best() is None and net.epochs_done == done + 1
        net.close()
    finally:
        capi._LIBC.fflush(None)
        capi.init(0)
    out = capfd.readouterr().out
    b, s = kb.rule([(r["epoch"], r["loss"], r["correct"], r["n"]) for r in recs], "loss", 3)
    assert 1 <= b < s == len(recs) - 1 < 23
    assert best == recs[b] and done == best["epoch"] == b + 1
    assert kb.BEST_RE.findall(out) == [(str(best["epoch"]), f"{best['loss']:.10f}", str(best["correct"]), "23")]
    assert kb.STOP_RE.findall(out) == [(str(recs[s]["epoch"]), "3")]
