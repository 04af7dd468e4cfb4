"""ctypes binding of the native libhpnn C API (hpnn_amd/lib/libhpnn.so).

Gives Python users the reference workflow (include/libhpnn.h of ovhpa/hpnn): load a conf,
generate/load a kernel, train (online reference semantics or batched), run, dump
kernel.opt -- executed by the C++/HIP engines, not by Python.
"""
import ctypes
import os
import tempfile

import torch  # noqa: F401  (shares torch's HIP runtime with libhpnn)

from ._lib import lib_path

_LIB = None
_LIBC = None

NN_TYPE = {"ANN": 0, "LNN": 1, "SNN": 2}
NN_TRAIN = {"BP": 0, "BPM": 1, "CG": 2, "SPLX": 3, "ADAM": 4}
NN_MODE = {"online": 0, "batched": 1}
NN_DTYPE = {"f64": 0, "f32": 1, "bf16": 2}
NN_DEVICE = {"auto": 0, "cpu": 1, "gpu": 2}
NN_LR_SCHEDULE = {None: -1, "constant": 0, "step": 1, "linear": 2, "plateau": 3}
NN_SHUFFLE = {"once": 0, "epoch": 1}
NN_KEEP_BEST = {"off": 0, "loss": 1, "acc": 2}
NN_CONFUSION = {"last": 0, "best": 1}
CG_FAILED, CG_RESTART, CG_VERTEX, CG_TOOK7 = 1, 2, 4, 8  # flags of a CG record (include/libhpnn/cg.h)


class CgRecord(ctypes.Structure):
    """hpnn_cg_record"""
    _fields_ = [("f0", ctypes.c_double), ("f1", ctypes.c_double), ("beta", ctypes.c_double),
                ("alpha", ctypes.c_double), ("trial", ctypes.c_uint), ("flags", ctypes.c_uint)]


class ClipRecord(ctypes.Structure):
    """nn_clip_record (= hpnn_clip_record)"""
    _fields_ = [("steps", ctypes.c_uint), ("clipped", ctypes.c_uint), ("norm_max", ctypes.c_double),
                ("norm_last", ctypes.c_double)]


def lib():
    global _LIB, _LIBC
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: build with `make`")
        L = ctypes.CDLL(path)
        vp, u, i, d, cp = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_double, ctypes.c_char_p
        sig = {
            "nn_init_all": (i, [u]), "nn_deinit_all": (i, []),
            "nn_set_verbose": (None, [ctypes.c_short]), "nn_return_verbose": (ctypes.c_short, []),
            "nn_return_capabilities": (i, []), "nn_set_cuda_streams": (i, [u]),
            "nn_set_n_gpu": (i, [u]), "nn_get_n_gpu": (i, [ctypes.POINTER(u)]),
            "nn_set_omp_threads": (i, [u]),
            "nn_load_conf": (vp, [cp]), "nn_deinit_conf": (None, [vp]),
            "nn_dump_conf": (None, [vp, vp]), "nn_dump_kernel": (None, [vp, vp]),
            "nn_dump_kernel_exact": (None, [vp, vp]),
            "nn_train_kernel": (i, [vp]), "nn_run_kernel": (None, [vp]),
            "nn_get_n_inputs": (u, [vp]), "nn_get_n_hiddens": (u, [vp]), "nn_get_n_outputs": (u, [vp]),
            "nn_get_h_neurons": (u, [vp, u]),
            "nn_set_mode": (None, [vp, i]), "nn_set_dtype": (None, [vp, i]), "nn_set_device": (None, [vp, i]),
            "nn_set_shuffle": (None, [vp, i]), "nn_return_shuffle": (i, [vp]),
            "hpnn_epoch_perm": (None, [u, u, u, vp]),
            "nn_set_validate": (None, [vp, u]), "nn_return_validate": (u, [vp]),
            "nn_get_validation": (u, [vp, u, vp, vp, vp, vp]),
            "nn_set_keep_best": (None, [vp, i]), "nn_return_keep_best": (i, [vp]),
            "nn_set_patience": (None, [vp, u]), "nn_return_patience": (u, [vp]),
            "nn_get_best": (i, [vp, ctypes.POINTER(u), ctypes.POINTER(d), ctypes.POINTER(u), ctypes.POINTER(u)]),
            "nn_get_cg_history": (ctypes.POINTER(CgRecord), [vp, ctypes.POINTER(u)]),
            "nn_set_batch": (None, [vp, u]), "nn_set_epochs": (None, [vp, u]),
            "nn_set_learning_rate": (None, [vp, d]), "nn_set_momentum": (None, [vp, d]),
            "nn_set_seed": (None, [vp, u]), "nn_return_seed": (u, [vp]),
            "nn_set_train": (None, [vp, i]), "nn_return_batch": (u, [vp]),
            "nn_set_adam": (None, [vp, d, d, d, d]),
            "nn_get_adam": (None, [vp, ctypes.POINTER(d), ctypes.POINTER(d), ctypes.POINTER(d), ctypes.POINTER(d)]),
            "nn_set_lr_schedule": (None, [vp, i, d, u, u, d, d, u, u]),
            "nn_get_lr_schedule": (None, [vp, ctypes.POINTER(i), ctypes.POINTER(d), ctypes.POINTER(u),
                                          ctypes.POINTER(u), ctypes.POINTER(d), ctypes.POINTER(d), ctypes.POINTER(u),
                                          ctypes.POINTER(u)]),
            "nn_get_lr_history": (ctypes.POINTER(d), [vp, ctypes.POINTER(u)]),
            "nn_set_clip": (None, [vp, d]), "nn_get_clip": (d, [vp]),
            "nn_get_clip_history": (ctypes.POINTER(ClipRecord), [vp, ctypes.POINTER(u)]),
            "nn_set_confusion": (None, [vp, i]), "nn_return_confusion": (i, [vp]),
            "nn_get_confusion_matrix": (u, [vp, i, u, vp]), "nn_get_class_history": (u, [vp, u, vp, vp, vp]),
            "nn_return_confusion_launches": (u, [vp]), "nn_dump_confusion_matrix": (i, [vp, i, cp]),
            "nn_return_last_pass": (u, []), "nn_return_last_total": (u, []),
            "nn_return_version": (cp, []), "nn_return_type": (i, [vp]), "nn_return_train": (i, [vp]),
            "nn_dump_state": (i, [vp, cp]), "nn_load_state": (i, [vp, cp]), "nn_return_epochs_done": (u, [vp]),
            "nn_pack_samples": (i, [cp, cp]),
            "nn_pack_arrays": (i, [cp, vp, vp, u, u, u]),
            "hpnn_trace_enable": (None, [i]), "hpnn_trace_enabled": (i, []), "hpnn_trace_push": (None, [cp]),
            "hpnn_trace_pop": (None, []), "hpnn_trace_add": (None, [cp, d]), "hpnn_trace_reset": (None, []),
            "hpnn_trace_calls": (ctypes.c_uint64, [cp]), "hpnn_trace_seconds": (d, [cp]),
            "hpnn_metrics_open": (i, [cp]), "hpnn_metrics_emit": (None, [cp, cp]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
        _LIBC = ctypes.CDLL(None)
        _LIBC.fopen.restype = vp
        _LIBC.fopen.argtypes = [cp, cp]
        _LIBC.fclose.argtypes = [vp]
    return _LIB


def init(verbose=0, streams=1):
    L = lib()
    L.nn_init_all(0)
    L.nn_set_verbose(verbose)
    L.nn_set_cuda_streams(streams)
    return L


def deinit():
    lib().nn_deinit_all()


class Network:
    """A libhpnn nn_def: conf + kernel, driven by the native engines."""

    def __init__(self, conf_path):
        self.L = lib()
        self.ptr = self.L.nn_load_conf(conf_path.encode())
        if not self.ptr:
            raise RuntimeError(f"nn_load_conf failed for {conf_path}")

    def close(self):
        if self.ptr:
            self.L.nn_deinit_conf(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # configuration
    def set(self, mode=None, dtype=None, device=None, batch=None, epochs=None, lr=None, momentum=None, seed=None,
            shuffle=None, validate=None, keep_best=None, patience=None, adam=None, lr_schedule=None, clip=None,
            confusion=None):
        if mode is not None:
            self.L.nn_set_mode(self.ptr, NN_MODE[mode])
        if dtype is not None:
            self.L.nn_set_dtype(self.ptr, NN_DTYPE[dtype])
        if device is not None:
            self.L.nn_set_device(self.ptr, NN_DEVICE[device])
        if batch is not None:
            self.L.nn_set_batch(self.ptr, batch)
        if epochs is not None:
            self.L.nn_set_epochs(self.ptr, epochs)
        if lr is not None:
            self.L.nn_set_learning_rate(self.ptr, lr)
        if momentum is not None:
            self.L.nn_set_momentum(self.ptr, momentum)
        if seed is not None:
            self.L.nn_set_seed(self.ptr, seed)
        if shuffle is not None:  # "once" | "epoch" (or a bool: True = "epoch")
            self.L.nn_set_shuffle(self.ptr, NN_SHUFFLE[shuffle] if isinstance(shuffle, str) else int(bool(shuffle)))
        if validate is not None:  # N: batched training validates on [test_dir] every N epochs (0 = off)
            self.L.nn_set_validate(self.ptr, int(validate))
        if keep_best is not None:  # "loss" | "acc": return the state of the best validation pass ("off" / False)
            self.L.nn_set_keep_best(self.ptr, NN_KEEP_BEST[keep_best or "off"])
        if patience is not None:  # P: stop after P validation passes without improvement (0 = never)
            self.L.nn_set_patience(self.ptr, int(patience))
        if adam is not None:  # dict(beta1=, beta2=, epsilon=, decay=) of [train] ADAM; a missing key keeps its value
            cur = self.adam
            unknown = set(adam) - set(cur)
            if unknown:
                raise ValueError(f"adam: unknown keys {sorted(unknown)} (beta1, beta2, epsilon, decay)")
            cur.update({k: float(v) for k, v in adam.items()})
            self.L.nn_set_adam(self.ptr, cur["beta1"], cur["beta2"], cur["epsilon"], cur["decay"])
        if lr_schedule is not None:  # dict(kind=, gamma=, period=, span=, lr_end=, lr_min=, patience=, warmup=)
            cur = self.lr_schedule   # of [lr_schedule]; a missing key keeps its value, kind=None turns it off
            unknown = set(lr_schedule) - set(cur)
            if unknown:
                raise ValueError(f"lr_schedule: unknown keys {sorted(unknown)} ({', '.join(cur)})")
            cur.update(lr_schedule)
            if cur["kind"] not in NN_LR_SCHEDULE:
                raise ValueError(f"lr_schedule: kind {cur['kind']!r} (constant | step | linear | plateau)")
            self.L.nn_set_lr_schedule(self.ptr, NN_LR_SCHEDULE[cur["kind"]], float(cur["gamma"]), int(cur["period"]),
                                      int(cur["span"]), float(cur["lr_end"]), float(cur["lr_min"]),
                                      int(cur["patience"]), int(cur["warmup"]))
        if clip is not None:  # c: batched training rescales a gradient whose global L2 norm exceeds c (0 = off)
            c = float(clip)
            if not (c >= 0.0 and c != float("inf")):
                raise ValueError(f"clip: {clip!r} (a finite norm > 0; 0 turns it off)")
            self.L.nn_set_clip(self.ptr, c)
        if confusion is not None:  # per-class metrics of every validation pass / of run() ([confusion] on | off)
            self.L.nn_set_confusion(self.ptr, int(bool(confusion)))
        return self

    @property
    def confusion(self):
        return bool(self.L.nn_return_confusion(self.ptr))

    def confusion_matrix(self, which="last"):
        """the confusion matrix of the last train() or run() call as a [n_out, n_out + 1] numpy uint32
        array (row = target class, column = guess, the last column "none"): which "last" = the last
        validation pass reported (or the run), "best" = the pass keep_best kept; None when there is
        nothing to report"""
        import numpy as np
        w = NN_CONFUSION[which]
        n = self.L.nn_get_confusion_matrix(self.ptr, w, 0, None)
        if not n:
            return None
        m = np.zeros((n, n + 1), dtype=np.uint32)
        self.L.nn_get_confusion_matrix(self.ptr, w, m.size, m.ctypes.data)
        return m

    def class_history(self):
        """one dict per validation pass of the last train() call under [confusion]: numpy uint32
        arrays support, hit and predicted (one entry per class) and balanced_accuracy"""
        import numpy as np
        from . import ops
        out = []
        while True:
            n = self.L.nn_get_class_history(self.ptr, len(out), None, None, None)
            if not n:
                return out
            a = [np.zeros(n, dtype=np.uint32) for _ in range(3)]
            self.L.nn_get_class_history(self.ptr, len(out), *[x.ctypes.data for x in a])
            out.append({"support": a[0], "hit": a[1], "predicted": a[2],
                        "balanced_accuracy": ops.balanced_accuracy(a[0], a[1])})

    @property
    def confusion_launches(self):
        """the tally launches the last train() call issued on the GPU, a captured launch counted once
        however often its graph is replayed (0 with the key off)"""
        return self.L.nn_return_confusion_launches(self.ptr)

    def dump_confusion_matrix(self, path, which="last"):
        if not self.L.nn_dump_confusion_matrix(self.ptr, NN_CONFUSION[which], path.encode()):
            raise OSError(f"nn_dump_confusion_matrix({path}) failed: nothing to report, or the file cannot be written")

    @property
    def clip(self):
        """the [clip] bound a training call would use (0.0: off)"""
        return float(self.L.nn_get_clip(self.ptr))

    def clip_history(self):
        """one dict per epoch of the last train() call under [clip]: steps, clipped (the steps whose
        gradient was rescaled), norm_max, norm_last; empty without [clip]"""
        m = ctypes.c_uint()
        r = self.L.nn_get_clip_history(self.ptr, ctypes.byref(m))
        return [{"steps": r[i].steps, "clipped": r[i].clipped, "norm_max": r[i].norm_max, "norm_last": r[i].norm_last}
                for i in range(m.value)]

    @property
    def lr_schedule(self):
        """the [lr_schedule] keys a training call would use: kind (None: no schedule), gamma, period,
        span, lr_end, lr_min, patience, warmup"""
        k = ctypes.c_int()
        g, e, m = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        p, sp, pa, w = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
        self.L.nn_get_lr_schedule(self.ptr, *[ctypes.byref(x) for x in (k, g, p, sp, e, m, pa, w)])
        return {"kind": {v: n for n, v in NN_LR_SCHEDULE.items()}[k.value], "gamma": g.value, "period": p.value,
                "span": sp.value, "lr_end": e.value, "lr_min": m.value, "patience": pa.value, "warmup": w.value}

    def lr_history(self):
        """the learning rate of every epoch of the last train() call under [lr_schedule] (a list of
        floats, empty without a schedule)"""
        m = ctypes.c_uint()
        r = self.L.nn_get_lr_history(self.ptr, ctypes.byref(m))
        return [float(r[i]) for i in range(m.value)]

    @property
    def adam(self):
        """the [train] ADAM coefficients a training call would use: beta1, beta2, epsilon, decay"""
        v = [ctypes.c_double() for _ in range(4)]
        self.L.nn_get_adam(self.ptr, *[ctypes.byref(x) for x in v])
        return dict(zip(("beta1", "beta2", "epsilon", "decay"), (x.value for x in v)))

    @property
    def keep_best(self):
        return {v: k for k, v in NN_KEEP_BEST.items()}[self.L.nn_return_keep_best(self.ptr)]

    @property
    def patience(self):
        return self.L.nn_return_patience(self.ptr)

    def best(self):
        """the best validation record of the last train() call with keep_best on: a dict with
        epoch, loss (mean per sample), correct, n and accuracy; None when there is none"""
        ep, co, nn, lo = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint(), ctypes.c_double()
        if not self.L.nn_get_best(self.ptr, ctypes.byref(ep), ctypes.byref(lo), ctypes.byref(co), ctypes.byref(nn)):
            return None
        return {"epoch": ep.value, "loss": lo.value, "correct": co.value, "n": nn.value,
                "accuracy": co.value / nn.value if nn.value else 0.0}

    def cg_history(self):
        """the [train] CG records of the last train() call, one dict per iteration (= epoch): f0 and
        f1 (mean loss before / after), beta, alpha (the step taken), trial (j*, None when every
        trial loss was a NaN), flags (CG_FAILED | CG_RESTART | CG_VERTEX | CG_TOOK7)"""
        m = ctypes.c_uint()
        r = self.L.nn_get_cg_history(self.ptr, ctypes.byref(m))
        return [{"f0": r[i].f0, "f1": r[i].f1, "beta": r[i].beta, "alpha": r[i].alpha,
                 "trial": None if r[i].trial == 0xffffffff else int(r[i].trial), "flags": int(r[i].flags)}
                for i in range(m.value)]

    @property
    def validate(self):
        return self.L.nn_return_validate(self.ptr)

    def validation(self):
        """the validation records of the last train() call: a list of dicts with epoch, loss
        (mean per sample), correct, n and accuracy, in epoch order"""
        import numpy as np
        m = self.L.nn_get_validation(self.ptr, 0, None, None, None, None)
        ep, co, nn = (np.zeros(m, dtype=np.uint32) for _ in range(3))
        lo = np.zeros(m, dtype=np.float64)
        if m:
            self.L.nn_get_validation(self.ptr, m, ep.ctypes.data, lo.ctypes.data, co.ctypes.data, nn.ctypes.data)
        return [{"epoch": int(ep[i]), "loss": float(lo[i]), "correct": int(co[i]), "n": int(nn[i]),
                 "accuracy": float(co[i]) / float(nn[i]) if nn[i] else 0.0} for i in range(m)]

    @property
    def shuffle(self):
        return {v: k for k, v in NN_SHUFFLE.items()}[self.L.nn_return_shuffle(self.ptr)]

    @property
    def dims(self):
        h = [self.L.nn_get_h_neurons(self.ptr, i) for i in range(self.L.nn_get_n_hiddens(self.ptr))]
        return [self.L.nn_get_n_inputs(self.ptr)] + h + [self.L.nn_get_n_outputs(self.ptr)]

    def train(self):
        return bool(self.L.nn_train_kernel(self.ptr))

    def run(self):
        self.L.nn_run_kernel(self.ptr)
        return self.L.nn_return_last_pass(), self.L.nn_return_last_total()

    def _dump(self, fn, path):
        f = _LIBC.fopen(path.encode(), b"w")
        if not f:
            raise OSError(path)
        try:
            fn(self.ptr, f)
        finally:
            _LIBC.fclose(f)

    def dump_kernel(self, path, exact=False):
        self._dump(self.L.nn_dump_kernel_exact if exact else self.L.nn_dump_kernel, path)

    def dump_conf(self, path):
        self._dump(self.L.nn_dump_conf, path)

    # exact checkpoint / resume (csrc/core/state.cpp)
    def dump_state(self, path):
        if not self.L.nn_dump_state(self.ptr, path.encode()):
            raise OSError(f"nn_dump_state({path}) failed")

    def load_state(self, path):
        if not self.L.nn_load_state(self.ptr, path.encode()):
            raise OSError(f"nn_load_state({path}) failed (missing, corrupted or mismatched)")

    @property
    def epochs_done(self):
        return self.L.nn_return_epochs_done(self.ptr)


def hpnn_epoch_perm(n, seed, epoch):
    """the [shuffle] epoch permutation (include/libhpnn/shuffle.h) as a numpy uint32 array:
    out[i] = index, in the order drawn once from [seed], of the sample at position i of `epoch`"""
    import numpy as np
    out = np.empty(int(n), dtype=np.uint32)
    lib().hpnn_epoch_perm(int(n), int(seed) & 0xffffffff, int(epoch) & 0xffffffff, out.ctypes.data)
    return out


def pack_samples(sample_dir, out_path):
    """pack a directory of sample files into one binary file (csrc/core/dataset.cpp)"""
    if not lib().nn_pack_samples(sample_dir.encode(), out_path.encode()):
        raise OSError(f"nn_pack_samples({sample_dir}) failed")


def pack_arrays(out_path, X, T):
    """write n records (X [n, n_in], T [n, n_out], anything numpy turns into float64) as a pack
    file train_nn / run_nn accept in place of a sample directory"""
    import numpy as np
    X = np.ascontiguousarray(X, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    n, n_in = X.shape
    if T.shape[0] != n:
        raise ValueError("X and T need the same number of rows")
    if not lib().nn_pack_arrays(out_path.encode(), X.ctypes.data, T.ctypes.data, n, n_in, T.shape[1]):
        raise OSError(f"nn_pack_arrays({out_path}) failed")


def smoke_online():
    """One MNIST-shaped SNN sample trained online (reference semantics) by the native
    engine (GPU when present), then a kernel dump + reload round trip."""
    from .utils import formats
    import numpy as np
    init(0)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "s"))
        rng = np.random.default_rng(0)
        x = rng.random(784)
        t = np.zeros(10)
        t[3] = 1.0
        formats.write_sample(os.path.join(d, "s", "s00001.txt"), x, t)
        conf = os.path.join(d, "nn.conf")
        formats.write_conf(conf, name="smoke", type="SNN", init="generate", seed=10958, inputs=784,
                           hiddens=[128, 64], outputs=10, train="BP", sample_dir=os.path.join(d, "s"),
                           test_dir=os.path.join(d, "s"))
        net = Network(conf)
        assert net.dims == [784, 128, 64, 10]
        assert net.train()
        kpath = os.path.join(d, "kernel.opt")
        net.dump_kernel(kpath)
        net.close()
        k = formats.read_kernel(kpath)
        assert [w.shape for w in k["weights"]] == [(128, 784), (64, 128), (10, 64)]
