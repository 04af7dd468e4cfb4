"""The conf-key corpus and the training runs whose output is compared with a record.

The record files beside this module (capi_record_cpu.json, capi_record_gpu.json) hold what a
build of the commit BEFORE the conf-key table wrote for every case below: they are the
reference, the code under test never writes them.  To make them again, check that commit out,
build it, and run

    python tests/capi_record_common.py cpu      (any machine)
    python tests/capi_record_common.py gpu      (a machine with the GPU)

Every case is one train_nn process (-c -x -O 1 -vv: the CPU engine on one thread is
deterministic, -vv prints the conf that nn_load_conf produced through nn_dump_conf), or, for
the two refusals that no conf and no flag can reach, one small ctypes process (api_child).
"""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_NN = os.path.join(ROOT, "bin", "train_nn")
LIBHPNN = os.path.join(ROOT, "hpnn_amd", "lib", "libhpnn.so")
HERE = os.path.dirname(os.path.abspath(__file__))
RECORD_CPU = os.path.join(HERE, "capi_record_cpu.json")
RECORD_GPU = os.path.join(HERE, "capi_record_gpu.json")

# a 6-5-4-3 net
BASE = ["[name] t", "[type] SNN", "[init] generate", "[seed] 7", "[input] 6", "[hidden] 5 4", "[output] 3",
        "[train] BP"]
BATCHED = ["[mode] batched"]  # [batch], [epochs], [dtype] and [parallel] are dumped in batched mode only

# ---------------------------------------------------------------------------------------------
# conf corpus: {group: {case id: the lines that follow BASE}}
# ---------------------------------------------------------------------------------------------
VALID = {
    "name": ["[name] abc"], "type": ["[type] LNN"], "seed": ["[seed] 123"], "train": ["[train] BPM"],
    "train_adam": ["[train] ADAM"], "train_cg": ["[train] CG"], "train_splx": ["[train] SPLX"],
    "input_hidden_output": ["[input] 9", "[hidden] 8 7 6", "[output] 2"],
    "sample_dir": ["[sample_dir] ./s"], "test_dir": ["[test_dir] ./t"], "mode": ["[mode] batched"],
    "device": ["[device] gpu"], "batch": BATCHED + ["[batch] 32"], "epochs": BATCHED + ["[epochs] 5"],
    "parallel": BATCHED + ["[parallel] tp"], "lr": ["[lr] 0.05"], "momentum": ["[momentum] 0.3"],
    "dtype": BATCHED + ["[dtype] bf16"], "dtype_fp32": BATCHED + ["[dtype] fp32"],
    "dtype_float": BATCHED + ["[dtype] float"], "dtype_F32": BATCHED + ["[dtype] F32"],
    "dtype_f64": BATCHED + ["[dtype] f64"], "dtype_fp64": BATCHED + ["[dtype] fp64"],
    "dtype_double": BATCHED + ["[dtype] Double"],
    "shuffle": ["[shuffle] epoch"], "shuffle_once": ["[shuffle] ONCE"], "validate": ["[validate] 3"],
    "validate_max": ["[validate] 4294967295"], "keep_best": ["[keep_best] acc"], "keep_best_loss": ["[keep_best] Loss"],
    "patience": ["[patience] 2"], "clip": ["[clip] 0.5"], "clip_off": ["[clip] 0"],
    "lr_schedule": ["[lr_schedule] step"], "lr_schedule_constant": ["[lr_schedule] constant"],
    "lr_schedule_linear": ["[lr_schedule] Linear"], "lr_schedule_plateau": ["[lr_schedule] PLATEAU"],
    "lr_gamma": ["[lr_gamma] 0.25"], "lr_gamma_one": ["[lr_gamma] 1"], "lr_end": ["[lr_end] -0.001"],
    "lr_min": ["[lr_min] 1e-5"], "lr_min_zero": ["[lr_min] 0"], "lr_period": ["[lr_period] 4"],
    "lr_span": ["[lr_span] 9"], "lr_patience": ["[lr_patience] 3"], "warmup": ["[warmup] 2"],
    "warmup_zero": ["[warmup] 0"], "beta1": ["[beta1] 0.8"], "beta1_zero": ["[beta1] 0"], "beta2": ["[beta2] 0.95"],
    "epsilon": ["[epsilon] 1e-6"], "decay": ["[decay] 0.01"], "decay_zero": ["[decay] 0"],
    "all": ["[sample_dir] ./s", "[test_dir] ./t", "[mode] batched", "[batch] 8", "[epochs] 3", "[dtype] f32",
            "[parallel] tp", "[shuffle] epoch", "[validate] 2", "[keep_best] loss", "[patience] 4", "[lr] 0.02",
            "[momentum] 0.1", "[beta1] 0.7", "[beta2] 0.9", "[epsilon] 1e-7", "[decay] 0.5", "[lr_schedule] plateau",
            "[lr_gamma] 0.3", "[lr_period] 2", "[lr_span] 6", "[lr_end] 0.004", "[lr_min] 0.0001", "[lr_patience] 5",
            "[warmup] 1", "[clip] 2.5"],
}

# the reference's keys stay lenient: whatever they make of these values is part of the record
LENIENT = {
    "type_unknown_word": ["[type] xyz"], "type_empty": ["[type]"], "type_lower": ["[type] snn"],
    "init_upper": ["[init] GENERATE"], "init_empty": ["[init]"], "init_missing_file": ["[init] ./no_such_kernel"],
    "seed_word": ["[seed] x"], "seed_empty": ["[seed]"], "seed_trailing": ["[seed] 12abc"],
    "input_word": ["[input] x"], "input_zero": ["[input] 0"], "output_word": ["[output] -3"],
    "hidden_word": ["[hidden] 5 x"], "hidden_zero": ["[hidden] 5 0"], "hidden_empty": ["[hidden]"],
    "train_lower": ["[train] bpm"], "train_bp_long": ["[train] BPx"], "train_unknown": ["[train] zz"],
    "train_empty": ["[train]"], "mode_first_letter": ["[mode] Bxyz"], "mode_unknown": ["[mode] zz"],
    "device_unknown": ["[device] zz"], "batch_zero": BATCHED + ["[batch] 0"], "batch_word": BATCHED + ["[batch] x"],
    "epochs_zero": BATCHED + ["[epochs] 0"], "parallel_unknown": BATCHED + ["[parallel] zz"],
    "parallel_upper": BATCHED + ["[parallel] TP"], "lr_word": ["[lr] abc"], "lr_negative": ["[lr] -2"],
    "lr_trailing": ["[lr] 0.5abc"], "momentum_word": ["[momentum] abc"], "momentum_negative": ["[momentum] -1"],
    "no_type": ["[type] "], "unknown_key": ["[nothing] 3"], "sample_dir_empty": ["[sample_dir]"],
    "epsilon_inf": ["[epsilon] inf"], "decay_inf": ["[decay] inf"], "count_trailing": ["[validate] 3abc"],
    "real_trailing": ["[clip] 0.5abc"], "count_signed": ["[lr_period] +3"],
}

_COUNTS_MIN1 = ["validate", "patience", "lr_period", "lr_span", "lr_patience"]
_BAD_COUNT = {"empty": "", "word": "abc", "negative": "-3", "big": "4294967296", "huge": "99999999999999999999999"}
_BAD_REAL = {
    "clip": {"empty": "", "word": "abc", "nan": "nan", "inf": "inf", "negative": "-1"},
    "lr_gamma": {"empty": "", "word": "abc", "nan": "nan", "inf": "inf", "zero": "0", "above": "1.5",
                 "negative": "-0.1"},
    "lr_end": {"empty": "", "word": "abc", "nan": "nan", "inf": "inf", "neg_inf": "-inf"},
    "lr_min": {"empty": "", "word": "abc", "nan": "nan", "inf": "inf", "negative": "-1"},
    "beta1": {"empty": "", "word": "abc", "nan": "nan", "inf": "inf", "negative": "-0.1", "one": "1"},
    "beta2": {"empty": "", "word": "abc", "nan": "nan", "inf": "inf", "negative": "-0.1", "one": "1"},
    "epsilon": {"empty": "", "word": "abc", "nan": "nan", "zero": "0", "negative": "-1"},
    "decay": {"empty": "", "word": "abc", "nan": "nan", "negative": "-1", "neg_inf": "-inf"},
}
_BAD_WORD = {"dtype": ["", "f16", "bf61"], "shuffle": ["", "never"], "keep_best": ["", "best", "off"],
             "lr_schedule": ["", "cosine", "none"]}


def _malformed():
    out = {}
    for key in _COUNTS_MIN1 + ["warmup"]:
        for tag, val in _BAD_COUNT.items():
            out[f"{key}_{tag}"] = [f"[{key}] {val}"]
        if key != "warmup":
            out[f"{key}_zero"] = [f"[{key}] 0"]
    for key, bad in _BAD_REAL.items():
        for tag, val in bad.items():
            out[f"{key}_{tag}"] = [f"[{key}] {val}"]
    for key, bad in _BAD_WORD.items():
        for i, val in enumerate(bad):
            out[f"{key}_{i}_{val or 'empty'}"] = [f"[{key}] {val}"]
    # a longer spelling of the key: some messages name the key as it was typed, some as it is defined
    for line in ("[validates] x", "[patiences] 0", "[clipping] -1", "[dtypes] zz", "[shuffled] zz", "[keep_bests] zz",
                 "[lr_schedules] zz", "[lr_gamma_x] x", "[lr_ends] x", "[lr_minimum] -1", "[lr_periods] 0",
                 "[lr_spans] 0", "[lr_patiences] 0", "[warmups] x", "[beta1x] 7", "[beta2x] 7", "[epsilons] 0",
                 "[decays] -1"):
        out["typed_" + line[1:line.index("]")]] = [line]
    return out


MALFORMED = _malformed()

# every spelling resolves to the handler it resolved to before (first name that is a prefix)
RESOLUTION = {
    "inputs_hiddens_outputs": ["[inputs] 9", "[hiddens] 8 7", "[outputs] 2"], "samples": ["[samples] ./s"],
    "tests": ["[tests] ./t"], "sample_dir": ["[sample_dir] ./s2"], "test_dir": ["[test_dir] ./t2"],
    "sample_directory": ["[sample_directory] ./s3"], "lr_gamma": ["[lr_gamma] 0.3"], "lr_gamma_x": ["[lr_gamma_x] 0.3"],
    "lr_end": ["[lr_end] 0.002"], "lr_min": ["[lr_min] 0.003"], "lr_period": ["[lr_period] 6"],
    "lr_span": ["[lr_span] 7"], "lr_patience": ["[lr_patience] 8"], "lr": ["[lr] 0.04"], "lr_unknown": ["[lr_zzz] 0.06"],
    "lrate": ["[lrate] 0.07"], "lr_schedule_x": ["[lr_schedules] step"], "batch": BATCHED + ["[batch] 17"],
    "batches": BATCHED + ["[batches] 18"], "beta1": ["[beta1] 0.6"], "beta2": ["[beta2] 0.7"], "beta": ["[beta] 0.5"],
    "epochs": BATCHED + ["[epochs] 9"], "epoch": BATCHED + ["[epoch] 9"], "epsilon": ["[epsilon] 0.001"],
    "decay": ["[decay] 0.25"], "device": ["[device] cpu"], "mode": ["[mode] batched"], "momentum": ["[momentum] 0.4"],
    "patience": ["[patience] 6"], "parallel": BATCHED + ["[parallel] tp"], "clipping": ["[clipping] 0.75"],
    "validates": ["[validates] 4"], "warmups": ["[warmups] 3"], "keep_best_x": ["[keep_best_pass] acc"],
    "upper_case_key": ["[LR] 0.09", "[Validate] 4"], "names": ["[names] nnn"], "seeds": ["[seeds] 99"],
    "lr_then_lr_star": ["[lr] 0.01", "[lr_gamma] 0.2", "[lr_end] 0.3", "[lr_min] 0.4", "[lr_period] 5", "[lr_span] 6",
                        "[lr_patience] 7", "[lr_schedule] linear"],
}

COMMENTS = {
    "count": ["[validate]   3   # every third epoch"], "real": ["[clip]\t0.5\t# the bound"],
    "word": ["[shuffle]   epoch  # a new order every epoch"], "reference_real": ["[lr]  0.05 # the rate"],
    "reference_count": BATCHED + ["[batch]  16   # samples"], "reference_word": ["[train]  BPM # momentum"],
    "reference_name": ["[name]  abc  # the name"], "lead_text": ["the rate [lr] 0.05"],
    "malformed_count": ["[validate]  # nothing"], "malformed_word": ["[dtype]  f16 # no such type"],
}

CONF_GROUPS = {"valid": VALID, "lenient": LENIENT, "malformed": MALFORMED, "resolution": RESOLUTION,
               "comments": COMMENTS}

# what the getters return for a conf whose keys the dump does not all show
GETTER_CONF = ["[device] gpu", "[mode] batched", "[batch] 17", "[epochs] 9", "[dtype] f32", "[lr] 0.04",
               "[momentum] 0.4", "[parallel] tp", "[validate] 4", "[patience] 6", "[shuffle] epoch", "[keep_best] acc",
               "[clip] 0.75", "[beta1] 0.6", "[epsilon] 0.001", "[lr_schedule] step", "[lr_period] 6", "[warmup] 3"]
GETTERS_INT = ["mode", "dtype", "device", "batch", "epochs", "shuffle", "validate", "keep_best", "patience", "seed",
               "type", "train"]
GETTERS_REAL = ["learning_rate", "momentum"]


def _cpu_env():
    e = dict(os.environ)
    e["HPNN_FORCE_CPU"] = "1"
    for k in ("HPNN_METRICS", "HPNN_TRACE", "HPNN_PARALLEL", "HPNN_DEBUG", "HPNN_LOOPBACK_RANKS", "HPNN_FORCE_RCCL"):
        e.pop(k, None)
    return e


def _gpu_env():
    e = _cpu_env()
    e.pop("HPNN_FORCE_CPU")
    return e


def _result(r):
    return {"rc": r.returncode, "stdout": r.stdout, "stderr": r.stderr}


def run_conf_case(workdir, lines):
    """train_nn -c -x -vv on BASE + lines: stdout holds the dumped conf, stderr the parse errors"""
    path = os.path.join(workdir, "nn.conf")
    with open(path, "w") as f:
        f.write("\n".join(BASE + lines) + "\n")
    r = subprocess.run([TRAIN_NN, "-c", "-x", "-O", "1", "-vv", "nn.conf"], cwd=workdir, env=_cpu_env(),
                       capture_output=True, text=True, timeout=120)
    return _result(r)


def run_conf_group(group):
    with tempfile.TemporaryDirectory() as d:
        return {cid: run_conf_case(d, lines) for cid, lines in CONF_GROUPS[group].items()}


def read_getters():
    """in this process, through libhpnn directly: the values of the plain getters for GETTER_CONF"""
    L = ctypes.CDLL(LIBHPNN)
    L.nn_load_conf.restype = ctypes.c_void_p
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "nn.conf")
        with open(path, "w") as f:
            f.write("\n".join(BASE + GETTER_CONF) + "\n")
        conf = ctypes.c_void_p(L.nn_load_conf(path.encode()))
    assert conf
    out = {}
    for g in GETTERS_INT:
        out[g] = int(getattr(L, "nn_return_" + g)(conf))
    for g in GETTERS_REAL:
        fn = getattr(L, "nn_return_" + g)
        fn.restype = ctypes.c_double
        out[g] = float(fn(conf))
    L.nn_get_clip.restype = ctypes.c_double
    out["clip"] = float(L.nn_get_clip(conf))
    L.nn_deinit_conf(conf)
    return out


# ---------------------------------------------------------------------------------------------
# training runs: 12 training and 6 validation samples, batch 4, 4 epochs, seed 7
# ---------------------------------------------------------------------------------------------
def _write_samples(d, n, shift, nan=False):
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        c = (i + shift) % 3
        x = [((i * 37 + j * 11 + shift * 5) % 23) / 11.0 - 1.0 for j in range(6)]
        x[c] += 0.5
        t = [1.0 if j == c else 0.0 for j in range(3)]
        with open(os.path.join(d, f"s{i:03d}.txt"), "w") as f:
            f.write("[input] 6\n" + " ".join("nan" if nan else f"{v:7.5f}" for v in x) + "\n")
            f.write("[output] 3\n" + " ".join(f"{v:.1f}" for v in t) + "\n")


def make_workdir(d):
    _write_samples(os.path.join(d, "train"), 12, 0)
    _write_samples(os.path.join(d, "val"), 6, 1)
    _write_samples(os.path.join(d, "two"), 2, 2)
    _write_samples(os.path.join(d, "valnan"), 2, 1, nan=True)  # every validation loss a NaN
    os.makedirs(os.path.join(d, "empty"), exist_ok=True)
    with open(os.path.join(d, "empty", "readme"), "w") as f:
        f.write("no sample here\n")


def _conf(train, extra=(), samples="./train", tests="./val"):
    return [x for x in BASE if not x.startswith("[train]")] + [f"[train] {train}", f"[sample_dir] {samples}",
                                                               f"[test_dir] {tests}", "[lr] 0.05"] + list(extra)


B = ["-b", "4", "-e", "4"]
BPM_FLAGS = B + ["-V", "1", "-K", "loss", "-P", "1", "-L", "plateau", "-C", "0.5"]
ONLINE_KEYS = ["[shuffle] epoch", "[validate] 1", "[keep_best] loss", "[patience] 1", "[lr_schedule] step",
               "[clip] 0.5"]

# {run id: (conf lines, train_nn flags)}
TRAIN_RUNS = {
    "bpm": (_conf("BPM"), BPM_FLAGS),
    "adam": (_conf("ADAM", ["[decay] 0.01"]), B + ["-V", "2", "-K", "acc"]),
    "cg": (_conf("CG"), B + ["-d", "f64"]),
    "bp_step_warmup": (_conf("BP", ["[lr_schedule] step", "[lr_period] 2", "[warmup] 2", "[shuffle] epoch"]), B),
    "bpm_early_stop": (_conf("BPM", ["[lr] 1e300"]), B + ["-V", "1", "-K", "loss", "-P", "1"]),
    "bpm_nan_validation": (_conf("BPM", tests="./valnan"), B + ["-V", "1", "-K", "loss"]),
    "online": (_conf("BP", ONLINE_KEYS, samples="./two"), []),
    "online_bpm_plain": (_conf("BPM", samples="./two"), []),
}

# the refusals of nn_train_kernel in the order of their checks; where two causes coincide the first
# one is reported
REFUSALS = {
    "train_type": (_conf("SPLX"), B),
    "train_unknown": (_conf("zz"), B),
    "cg_online": (_conf("CG"), []),
    "cg_bf16": (_conf("CG"), B + ["-d", "bf16"]),
    "adam_online": (_conf("ADAM"), []),
    "schedule_cg": (_conf("CG"), B + ["-L", "step"]),
    "plateau_no_validate": (_conf("BPM"), B + ["-L", "plateau"]),
    "clip_cg": (_conf("CG"), B + ["-C", "0.5"]),
    "no_sample_dir": (_conf("BPM", samples="./missing"), B),
    "keep_best_no_validate": (_conf("BPM"), B + ["-K", "loss"]),
    "patience_no_keep_best": (_conf("BPM"), B + ["-V", "1", "-P", "1"]),
    "test_dir_missing": (_conf("BPM", tests="./missing"), B + ["-V", "1"]),
    "test_dir_empty": (_conf("BPM", tests="./empty"), B + ["-V", "1"]),
    "schedule_invalid": (_conf("BPM"), B + ["-L", "linear"]),
    "both_cg_online_and_schedule": (_conf("CG", ["[lr_schedule] step", "[clip] 0.5"]), []),
    "both_schedule_cg_and_clip_cg": (_conf("CG"), B + ["-L", "step", "-C", "0.5", "-K", "loss"]),
    "both_plateau_and_keep_best": (_conf("BPM"), B + ["-L", "plateau", "-K", "loss", "-P", "1"]),
    "both_clip_cg_and_missing_samples": (_conf("CG", samples="./missing"), B + ["-C", "0.5"]),
    "both_keep_best_and_patience": (_conf("BPM", tests="./missing"), B + ["-K", "loss", "-P", "1"]),
    "both_patience_and_test_dir": (_conf("BPM", tests="./missing"), B + ["-V", "1", "-P", "1"]),
}
# the two that only the setters reach (the conf and the flags refuse these values themselves)
API_REFUSALS = {"adam_range": "adam", "clip_range": "clip", "both_adam_range_and_clip_range": "adam+clip"}

_TIMES = [(re.compile(r"in [0-9.]+ s \([0-9.]+ samples/s\)"), "in <T> s (<R> samples/s)")]
_METRIC_TIMES = re.compile(r'"(time|seconds|samples_per_s)": [-+0-9.eE]+')
_FLOAT = re.compile(r"(?<![\w.])[-+]?(?:\d+\.\d*(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+|nan|inf)(?![\w.])")


def mask_times(stdout, metrics):
    """the wall-clock fields alone: seconds and samples/s on stdout; time, seconds and samples_per_s
    in the metrics lines"""
    for rx, to in _TIMES:
        stdout = rx.sub(to, stdout)
    return stdout, _METRIC_TIMES.sub(lambda m: f'"{m.group(1)}": 0', metrics)


def mask_floats(stdout, metrics):
    """every floating-point field (the GPU engines add their loss slots with atomics): the kinds of
    line and their order, the epoch numbers and every integer field stay; of the metrics the event
    and field names, the field order, the strings and the integers"""
    stdout = _FLOAT.sub("<F>", mask_times(stdout, "")[0])
    events = []
    for ln in metrics.splitlines():
        pairs = json.loads(ln, object_pairs_hook=list)
        events.append([[k, "<F>" if isinstance(v, float) else v] for k, v in pairs])
    return stdout, events


def run_train(workdir, conf_lines, flags, gpu=False):
    with open(os.path.join(workdir, "nn.conf"), "w") as f:
        f.write("\n".join(conf_lines) + "\n")
    mpath = os.path.join(workdir, "m.jsonl")
    if os.path.exists(mpath):
        os.remove(mpath)
    cmd = [TRAIN_NN] + ([] if gpu else ["-c"]) + ["-x", "-O", "1", "-vv", "-M", "m.jsonl"] + flags + ["nn.conf"]
    r = subprocess.run(cmd, cwd=workdir, env=_gpu_env() if gpu else _cpu_env(), capture_output=True, text=True,
                       timeout=300)
    out = _result(r)
    out["metrics"] = open(mpath).read() if os.path.exists(mpath) else ""
    if not gpu:
        out["stdout"], out["metrics"] = mask_times(out["stdout"], out["metrics"])
    return out


def run_api_refusal(workdir, what):
    with open(os.path.join(workdir, "nn.conf"), "w") as f:
        f.write("\n".join(_conf("ADAM", ["[mode] batched", "[batch] 4"])) + "\n")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "api_child", what], cwd=workdir, env=_cpu_env(),
                       capture_output=True, text=True, timeout=120)
    return _result(r)


def api_child(what):
    """load ./nn.conf, set values that only the setters let through, train: exit status 3 on a refusal"""
    L = ctypes.CDLL(LIBHPNN)
    L.nn_load_conf.restype = ctypes.c_void_p
    L.nn_init_all(0)
    conf = ctypes.c_void_p(L.nn_load_conf(b"nn.conf"))
    d = ctypes.c_double
    L.nn_set_adam.argtypes = [ctypes.c_void_p, d, d, d, d]
    L.nn_set_clip.argtypes = [ctypes.c_void_p, d]
    L.nn_set_device(conf, 1)
    if "adam" in what:
        L.nn_set_adam(conf, 1.5, 0.999, 1e-8, 0.0)
    if "clip" in what:
        L.nn_set_clip(conf, -1.0)
    ok = L.nn_train_kernel(conf)
    L.nn_deinit_conf(conf)
    L.nn_deinit_all()
    sys.exit(0 if ok else 3)


GPU_BPM = (_conf("BPM", ["[dtype] f32"]), BPM_FLAGS)


def run_gpu_bpm(workdir):
    make_workdir(workdir)
    out = run_train(workdir, GPU_BPM[0], GPU_BPM[1], gpu=True)
    out["stdout"], out["metrics"] = mask_floats(out["stdout"], out["metrics"])
    return out


def record_cpu():
    rec = {"conf": {g: run_conf_group(g) for g in CONF_GROUPS}, "getters": read_getters()}
    with tempfile.TemporaryDirectory() as d:
        make_workdir(d)
        rec["train"] = {rid: run_train(d, c, f) for rid, (c, f) in TRAIN_RUNS.items()}
        rec["refusals"] = {rid: run_train(d, c, f) for rid, (c, f) in REFUSALS.items()}
        rec["api_refusals"] = {rid: run_api_refusal(d, w) for rid, w in API_REFUSALS.items()}
    return rec


def _write(path, rec):
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "api_child":
        api_child(sys.argv[2])
    elif sys.argv[1] == "cpu":
        _write(sys.argv[2] if len(sys.argv) > 2 else RECORD_CPU, record_cpu())
    elif sys.argv[1] == "gpu":
        with tempfile.TemporaryDirectory() as d:
            _write(sys.argv[2] if len(sys.argv) > 2 else RECORD_GPU, run_gpu_bpm(d))
