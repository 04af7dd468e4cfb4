"""nn_load_conf / nn_dump_conf and the output of nn_train_kernel against a record.

capi_record_cpu.json was written by a build of the commit before the conf-key table and the
stepwise nn_train_kernel (see capi_record_common.py): every case here must give, byte for byte,
what that build gave.  Only the wall-clock fields are masked (seconds and samples/s on stdout;
time, seconds and samples_per_s in the metrics lines); the CPU engine on one thread is
deterministic, so every other number is compared exactly."""
import json

import pytest

from tests import capi_record_common as crc


@pytest.fixture(scope="module")
def record():
    with open(crc.RECORD_CPU) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("capi_record"))
    crc.make_workdir(d)
    return d


def _differences(got, want):
    assert sorted(got) == sorted(want), "the corpus and the record list different cases"
    return {cid: {f: (got[cid][f], want[cid][f]) for f in want[cid] if got[cid][f] != want[cid][f]}
            for cid in want if got[cid] != want[cid]}


@pytest.mark.parametrize("group", sorted(crc.CONF_GROUPS))
def test_conf_corpus(record, group):
    """every conf of the group: exit status, the dumped conf on stdout and the error lines on stderr"""
    want = record["conf"][group]
    assert len(want) >= 10
    assert not _differences(crc.run_conf_group(group), want)


def test_malformed_values_are_refused(record):
    """every malformed value of an extension key: nn_load_conf returned NULL (train_nn gave up
    before it dumped a conf) behind the two error lines"""
    for cid, r in record["conf"]["malformed"].items():
        err = r["stderr"].splitlines()
        assert r["rc"] == 255 and "# NN configuration" not in r["stdout"], cid
        assert err[0] == "NN(ERR): Malformed NN configuration file!", cid
        assert err[1].startswith("NN(ERR): [") and (" value: " in err[1] or " unknown: " in err[1]), cid
        assert err[2:] == ["FAILED to read NN configuration file! (ABORTING)"], cid


def test_getters(record):
    assert crc.read_getters() == record["getters"]


@pytest.mark.parametrize("run", sorted(crc.TRAIN_RUNS))
def test_training_output(record, workdir, run):
    conf, flags = crc.TRAIN_RUNS[run]
    assert not _differences({run: crc.run_train(workdir, conf, flags)}, {run: record["train"][run]})


def test_online_warnings_once_each_in_order(record):
    keys = ["[validate]", "[keep_best]", "[patience]", "[lr_schedule]", "[clip]", "[shuffle] epoch"]
    assert record["train"]["online"]["stderr"].splitlines() == [
        f"NN(WARN): {key} has no effect in online mode (ignored)" for key in keys]


def test_refusals(record, workdir):
    """every refusal of nn_train_kernel: exit status 1, its line on stderr (stdout for the train
    type, as before), nothing trained; where two causes coincide the earlier check reports"""
    got = {rid: crc.run_train(workdir, c, f) for rid, (c, f) in crc.REFUSALS.items()}
    assert not _differences(got, record["refusals"])
    for rid, r in record["refusals"].items():
        assert r["rc"] == 1 and "BATCHED TRAINING" not in r["stdout"] and "TRAINING FILE" not in r["stdout"], rid
        assert r["stderr"].endswith("Training FAILED!\n"), rid


def test_refusals_through_the_setters(record, workdir):
    got = {rid: crc.run_api_refusal(workdir, w) for rid, w in crc.API_REFUSALS.items()}
    assert not _differences(got, record["api_refusals"])
    assert all(r["rc"] == 3 and "out of range" in r["stderr"] for r in record["api_refusals"].values())
