"""Bias-free MLP (libhpnn ANN / SNN / LNN) on the gfx950 kernels.

Math (reference SURVEY 2.4; ann.c / snn.c):
  h_l = f(W_l h_{l-1}),  f(x) = 2/(1+e^-x) - 1   (every hidden layer; ANN output too)
  SNN output  o = e^{z-1} / (TINY + sum e^{z-1}),  delta_L = t - o
  ANN output  o = f(z),                             delta_L = (t - o) f'(o)
  hidden      delta_l = (W_{l+1}^T delta_{l+1}) * f'(h_l),  f'(y) = -0.5 (y^2 - 1)
  update      BP : W += lr * G ;  BPM: dW += lr * G; W += dW; dW *= alpha
              Adam (optimizer="adam"): include/libhpnn/adam.h on W32 / V32 (= m) / A32 (= v)
  with G = mean over the minibatch of delta_l (x) h_{l-1} (batched mode, see
  csrc/cpu/cpu_batched.cpp for the FP64 oracle of exactly these semantics).

This class is a thin binding over the library's batched plan (csrc/gpu/bplan.h, the same
object train_nn's batched engine runs): the plan picks the step structure, the split-K
factors and the grids, declares the device buffers, and launches every kernel.  Python
allocates those buffers as torch tensors (so W32, G, ... are views the tests and the
data-parallel driver use) and passes the current HIP stream, so steps are captured by
torch.cuda.graph.  On CPU tensors (tests without a GPU) the same configuration runs the
per-layer step in the PyTorch emulation of the kernels (hpnn_amd.ops), whatever the mode.
"""
import ctypes
import ctypes.util
import hashlib
import math
import os

import torch

from .. import ops
from .._lib import native

# the value a uint8 input means (1/255: MNIST pixels normalised to [0, 1])
PIXEL_SCALE = float(torch.tensor(float(os.environ.get("HPNN_PIXEL_SCALE", str(1.0 / 255.0))),
                                 dtype=torch.float32).item())

TYPES = {"ANN": ops.TYPE_ANN, "LNN": ops.TYPE_LNN, "SNN": ops.TYPE_SNN}
_MODES = {"": None, "t": "t", "x": "x", "m": "mid", "w": "w"}
_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.uint8, 3: torch.int32}


def reference_init(sizes, seed):
    """Bit-identical to libhpnn ann_generate (ann.c:632-766): glibc srandom(seed),
    w = 2 (random()/RAND_MAX - 0.5) / sqrt(M), hidden layers first, row-major."""
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.random.restype = ctypes.c_long
    libc.srandom(ctypes.c_uint(seed))
    rand_max = 2147483647.0
    out = []
    for l in range(len(sizes) - 1):
        M, N = sizes[l], sizes[l + 1]
        n = N * M
        if n > 4_000_000:
            raise ValueError("reference_init is meant for small nets; use init='fast'")
        w = torch.tensor([libc.random() for _ in range(n)], dtype=torch.float64)
        w = 2.0 * (w / rand_max - 0.5) / math.sqrt(M)
        out.append(w.view(N, M))
    return out


def fast_init(sizes, seed):
    """Same distribution U(-1,1)/sqrt(M) from torch's generator (large benchmark nets)."""
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(sizes[l + 1], sizes[l], generator=g, dtype=torch.float64) - 0.5) * 2.0
             / math.sqrt(sizes[l])) for l in range(len(sizes) - 1)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


class MLP:
    """Network + device state for batched BF16 MFMA training on one GPU.

    sizes: [n_in, h_1, ..., n_out]; net_type: 'ANN' | 'SNN' | 'LNN'.
    batch: per-step (per-GPU) minibatch (padded by the plan: to 128, 256 on the tile path).
    fused: None / True = the fastest structure the plan finds (True: error if none),
    False = per-layer kernels, or one of "t", "x", "mid", "w" (bplan.h).
    optimizer: "sgd" (BP, or BPM with momentum=True) | "adam" with lr, betas, eps, decay (AdamW when
    decay > 0): the plan then keeps the moments V32 (first) and A32 (second) and the state
    `adam_state` ([11] float64, ops.read_adam_state), and train_step ignores its lr / alpha.
    lr_schedule: None | dict(kind="constant" | "step" | "linear" | "plateau", lr=, gamma=, period=,
    span=, lr_end=, lr_min=, patience=, warmup=, epoch=) (include/libhpnn/lrsched.h; lr defaults to
    the `lr` argument): the plan keeps the state `lr_state` ([12] float64, ops.read_lr_state), every
    step reads its rate from it and ignores train_step's lr, and the caller runs advance_schedule()
    before the first step of every epoch (and ops.lr_plateau behind a validation pass).
    clip: None | c > 0 (include/libhpnn/clip.h): every optimizer step is the global norm of the
    gradient as the update sees it (ops.gnorm_partials over the padded slabs, in the plan's 8-way
    slab order), ops.clip_finalize into `clip_state` ([8] float64, ops.read_clip_state) and the
    update with the factor.  Plain BP / BPM then steps at the constructor's `lr` (train_step's lr is
    ignored, as under a schedule).  commit_clip() closes an epoch.
    """

    def __init__(self, sizes, net_type="SNN", batch=256, device="cuda", momentum=False, weights=None, seed=10958,
                 init="reference", splits=None, fused=None, mid_grid=512, optimizer="sgd", lr=0.001,
                 betas=(0.9, 0.999), eps=1e-8, decay=0.0, lr_schedule=None, clip=None):
        self.sizes = list(sizes)
        self.L = len(sizes) - 1
        self.type = TYPES[net_type] if isinstance(net_type, str) else int(net_type)
        self.type_name = net_type if isinstance(net_type, str) else {v: k for k, v in TYPES.items()}[net_type]
        self.device = torch.device(device)
        self.batch = batch
        self.momentum = momentum
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer {optimizer!r} (sgd | adam)")
        self.adam = optimizer == "adam"
        adam_cfg = (float(lr), float(betas[0]), float(betas[1]), float(eps), float(decay)) if self.adam else None
        self._best = None  # keep_best(): the best state
        self._cm = self._cm_last = self._cm_best = self._pc_hist = None  # confusion(True): the tally's tensors
        self.sched = lr_schedule is not None
        sched_cfg = None
        if self.sched:
            d = dict(kind="constant", lr=lr, gamma=0.5, period=10, span=0, lr_end=0.0, lr_min=0.0, patience=2,
                     warmup=0, epoch=0)
            unknown = set(lr_schedule) - set(d)
            if unknown:
                raise ValueError(f"lr_schedule: unknown keys {sorted(unknown)} ({', '.join(d)})")
            d.update(lr_schedule)
            kind = ops.LR_KIND[d["kind"]] if isinstance(d["kind"], str) else int(d["kind"])
            sched_cfg = (kind, float(d["lr"]), float(d["gamma"]), int(d["period"]), int(d["span"]), float(d["lr_end"]),
                         float(d["lr_min"]), int(d["patience"]), int(d["warmup"]), int(d["epoch"]))
        self.clip = clip is not None and float(clip) != 0.0
        clip_cfg = None
        if self.clip:
            if not (float(clip) > 0.0 and float(clip) != float("inf")):
                raise ValueError(f"clip: {clip!r} (a finite norm > 0)")
            clip_cfg = (float(clip), float(lr))
        on_gpu = self.device.type == "cuda"
        req = -1 if fused is None or fused is True else (0 if fused is False else ord({"mid": "m"}.get(fused, fused)))
        try:
            self.plan = native().BPlan(self.sizes, self.type, int(batch), bool(momentum), req, list(splits or []),
                                       int(mid_grid), on_gpu, adam_cfg, sched_cfg, clip_cfg)
        except ValueError as e:
            raise ValueError(f"fused={fused!r}: {e}") from None
        cfg = self.plan.config()
        self.cfg = cfg
        self.Bp, self.Kp, self.Np, self.S = cfg["Bp"], cfg["Kp"], cfg["Np"], cfg["S"]
        self.fused_mode = _MODES[cfg["mode"]]
        if fused is True and self.fused_mode is None:
            raise ValueError(f"no fused path for padded dims {self.Kp[0]}-{self.Np}")
        self.fused = self.fused_mode is not None
        self.n_out = sizes[-1]
        self.mid_groups = cfg["mid_groups"]
        # the plan's buffer table -> torch tensors (views), bound to the plan in table order
        self.buf = {}
        for name, layer, dt, shape, zero in self.plan.buffers():
            mk = torch.zeros if zero else torch.empty
            self.buf[(name, layer)] = mk(tuple(shape), dtype=_DT[dt], device=self.device)
        if on_gpu:
            self.plan.bind([t.data_ptr() for t in self.buf.values()])
        b = self.buf
        self.W32 = [b[("W32", l)] for l in range(self.L)]
        self.V32 = [b.get(("V32", l)) for l in range(self.L)]
        self.A32 = [b.get(("A32", l)) for l in range(self.L)]
        self.adam_state = None
        if self.adam:  # the plan's "adam" buffer is the hpnn_adam_state itself
            self.adam_state = b[("adam", -1)].view(torch.float64)
            self.adam_state.copy_(ops.adam_state(*adam_cfg))
        self.lr_state = None
        if self.sched:  # the plan's "lrs" buffer is the hpnn_lr_state itself
            self.lr_state = b[("lrs", -1)].view(torch.float64)
            self.lr_state.copy_(ops.lr_state(sched_cfg[0], *sched_cfg[1:]))
        self.clip_state = self.clip_part = None
        if self.clip:  # the plan's "clip" buffer is the hpnn_clip_state itself
            self.clip_state = b[("clip", -1)].view(torch.float64)
            self.clip_state.copy_(ops.clip_state(clip_cfg[0]))
            self.clip_part = b[("clip_part", -1)].view(torch.float64)
            if not (self.sched or self.adam):  # plain BP / BPM: the scheduled launch at a constant rate
                self.lr_state = b[("lrs", -1)].view(torch.float64)
                self.lr_state.copy_(ops.lr_state("constant", clip_cfg[1]))
            if on_gpu:
                self.plan.prepare_clip(_stream())
        self._Wb = [b[("Wb", l)] for l in range(self.L)]
        self._Wt = [b[("Wt", l)] for l in range(self.L)]
        self.slab = [b[("slab", l)] for l in range(self.L)]
        self.H = [b[("H", l)] for l in range(self.L - 1)]
        self.D = [b[("D", l)] for l in range(self.L)]
        self.Z, self.stats, self.grad_flat = b[("Z", -1)], b[("stats", -1)], b[("gflat", -1)]
        self.G, off = [], 0
        for l in range(self.L):
            n = self.Np[l] * self.Kp[l]
            self.G.append(self.grad_flat[off:off + n].view(self.Np[l], self.Kp[l]))
            off += n
        self.midslab, self.midtmp = b.get(("midslab", -1)), b.get(("midtmp", -1))
        self.W0f = b.get(("W0f", -1))
        if weights is None:
            weights = reference_init(sizes, seed) if init == "reference" else fast_init(sizes, seed)
        for l in range(self.L):
            self.W32[l][:sizes[l + 1], :sizes[l]].copy_(weights[l].to(torch.float32))
        self.refresh_bf16()

    # ------------------------------------------------------------------ helpers
    @property
    def _gpu(self):
        return self.device.type == "cuda"

    def sync_copies(self):
        """the BF16 copies a fused step of the tile path leaves stale (W0, W0^T, W1^T: no kernel of
        that step reads them) brought up to date from the FP32 masters, on the current stream;
        nothing is launched when none is stale (plan.stale_copies)"""
        if self._gpu and self.plan.stale_copies:
            self.plan.sync_copies(_stream())

    @property
    def Wb(self):
        """BF16 weights [Np, Kp] per layer, current (sync_copies)"""
        self.sync_copies()
        return self._Wb

    @property
    def Wt(self):
        """their transposes [Kp, Np], current (sync_copies)"""
        self.sync_copies()
        return self._Wt

    @property
    def tn_update(self):
        """the optimizer step in the 8-phase TN gradient's epilogue where it applies (plan)"""
        return self.plan.tn_update

    @tn_update.setter
    def tn_update(self, on):
        self.plan.tn_update = bool(on)

    def _tn_update_ok(self, l):
        return self.plan.tn_update_ok(int(l))

    @staticmethod
    def _pick_splits(N, K, Bp):
        """the plan's split-K rule (bplan.cpp BPlan::pick_splits)"""
        return native().BPlan.pick_splits(N, K, Bp)

    def refresh_bf16(self):
        """BF16 compute copies (and the fragment-major W0) from the FP32 masters"""
        if self._gpu:
            self.plan.cast_weights(_stream())
            return
        for l in range(self.L):
            ops.cast_weights(self.W32[l], self.Wb[l], self.Wt[l], self.W0f if l == 0 else None)

    def host_weights(self):
        """FP64 [N, M] weights (unpadded), for kernel.opt dumps / parity checks."""
        return [self.W32[l][:self.sizes[l + 1], :self.sizes[l]].double().cpu() for l in range(self.L)]

    def prepare_input(self, X, pixel_scale=None):
        """[n, n_in] -> the plan's input layout on the device, >= Bp rows (zero padding).

        X float/double: the values as given (BF16).  X uint8 (8-bit pixel data, e.g. MNIST
        images): the network sees bf16(X * PIXEL_SCALE) (1/255; HPNN_PIXEL_SCALE overrides, 1 =
        the raw 0..255 values the reference's pmnist writes).  Layouts (BPlan.input_layout):
        the tile path ("t") takes the batch fragment-major ([Bp/32, Kp0/16, 64, 8],
        ops.to_fragment_major; 8-bit pixels kept as bytes, exact integers in the MFMAs with
        the scale on the accumulators); "x" takes row-major BF16 plus, for 8-bit data, a
        fragment-major copy of the bytes (attribute `hpnn_fm`) for the first-layer gradient;
        every other mode row-major BF16.  pixel_scale overrides PIXEL_SCALE for this batch
        (1.0: the bytes are the values, as train_nn takes integer 0..255 data)."""
        ps = PIXEL_SCALE if pixel_scale is None else float(pixel_scale)
        Xd = X.to(self.device)
        n = Xd.shape[0]
        layout = self.cfg["input_layout"] if self._gpu else 0
        rows = max(self.Bp, ops.pad_to(n, 256 if layout == 1 else 128))
        u8 = Xd.dtype == torch.uint8
        if layout == 1:
            src = torch.zeros(rows, self.Kp[0], dtype=torch.uint8 if u8 else torch.bfloat16, device=self.device)
            if u8:
                src[:n, :Xd.shape[1]] = Xd
            else:
                ops.pack_bf16(Xd.contiguous(), src)
            out = ops.to_fragment_major(src).view(rows // 32, self.Kp[0] // 16, 64, 8)
            out.hpnn_fm_scale = ps if u8 else 1.0
            return out
        out = torch.empty(rows, self.Kp[0], dtype=torch.bfloat16, device=self.device)
        if u8:
            b = torch.zeros(rows, self.Kp[0], dtype=torch.uint8, device=self.device)
            b[:n, :Xd.shape[1]] = Xd
            out.copy_((b.float() * ps).bfloat16())  # the same rounding as the kernels'
            if layout == 2:
                out.hpnn_fm = ops.to_fragment_major(b)
                out.hpnn_fm_scale = ps
            return out
        ops.pack_bf16(Xd.contiguous(), out)
        return out

    def canonical_rows(self, X, pixel_scale=None):
        """[n, n_in] -> the device-resident row-major set MLP.gather_input reads: a dict with
        "x" = [n, Kp0] rows in the element type of the plan's input layout (uint8 for 8-bit data
        on the tile path, else BF16; the values prepare_input gives) and, for 8-bit data in
        mode "x", "xg" = the [n, Kp0] bytes of the first-layer gradient's copy."""
        ps = PIXEL_SCALE if pixel_scale is None else float(pixel_scale)
        Xd = X.to(self.device)
        n = Xd.shape[0]
        layout = self.cfg["input_layout"] if self._gpu else 0
        u8 = Xd.dtype == torch.uint8
        rows = {"n": n, "scale": ps if u8 else 1.0}
        if u8:
            b = torch.zeros(n, self.Kp[0], dtype=torch.uint8, device=self.device)
            b[:, :Xd.shape[1]] = Xd
            if layout == 1:
                rows["x"] = b
                return rows
            if layout == 2:
                rows["xg"] = b
            rows["x"] = (b.float() * ps).bfloat16()
            return rows
        rows["x"] = ops.pack_bf16(Xd.contiguous(), torch.empty(n, self.Kp[0], dtype=torch.bfloat16,
                                                               device=self.device))
        return rows

    def gather_input(self, X_rows, perm, pixel_scale=None):
        """what prepare_input(X[perm]) returns, gathered on the device (ops.gather_rows /
        ops.gather_fragment_major) from a resident row-major set: X_rows is canonical_rows(X),
        or X itself (converted first); perm an int32 device tensor of row indices."""
        if not isinstance(X_rows, dict):
            X_rows = self.canonical_rows(X_rows, pixel_scale)
        perm = perm.to(device=self.device, dtype=torch.int32).contiguous()
        n = perm.numel()
        layout = self.cfg["input_layout"] if self._gpu else 0
        rows = max(self.Bp, ops.pad_to(n, 256 if layout == 1 else 128))
        x = X_rows["x"]
        if layout == 1:
            out = torch.empty(rows // 32, self.Kp[0] // 16, 64, 8, dtype=x.dtype, device=self.device)
            ops.gather_fragment_major(x, perm, out)
            out.hpnn_fm_scale = X_rows["scale"]
            return out
        out = ops.gather_rows(x, perm, torch.empty(rows, self.Kp[0], dtype=torch.bfloat16, device=self.device))
        if "xg" in X_rows:
            out.hpnn_fm = ops.gather_fragment_major(
                X_rows["xg"], perm, torch.empty(rows // 32, self.Kp[0] // 16, 4, 16, 8, dtype=torch.uint8,
                                                device=self.device))
            out.hpnn_fm_scale = X_rows["scale"]
        return out

    @staticmethod
    def _is_fm(X):
        return X.dim() >= 4

    def _rowmajor(self, X):
        """row-major BF16 [rows, Kp0] view of a prepared batch (fragment-major input of the
        tile path is converted; the per-layer kernels need rows)"""
        if not self._is_fm(X):
            return X
        rows = X.shape[0] * 32
        R = ops.from_fragment_major(X, rows, X.shape[1] * 16)
        if X.dtype == torch.uint8:
            return (R.float() * getattr(X, "hpnn_fm_scale", PIXEL_SCALE)).bfloat16()
        return R.contiguous()

    def _fm_input(self, X):
        """the fragment-major copy of a prepared batch X the first-layer gradient streams, or None"""
        if self._is_fm(X):
            return X if X.shape[0] * 32 >= self.Bp else None
        Xg = getattr(X, "hpnn_fm", None)
        if Xg is None or X.shape[0] < self.Bp or Xg.numel() != X.shape[0] * self.Kp[0]:
            return None
        return Xg

    def _x(self, X):
        """(x, xg, u8, scale) plan arguments of a prepared batch; checks it has >= Bp rows"""
        if self._is_fm(X):
            if self.fused_mode != "t" or X.shape[0] * 32 < self.Bp or X.shape[1] * 16 != self.Kp[0]:
                raise ValueError(f"fragment-major batch {tuple(X.shape)} does not fit this plan "
                                 f"(mode {self.fused_mode}, Bp {self.Bp}, Kp0 {self.Kp[0]})")
            u8 = X.dtype == torch.uint8
            return X.data_ptr(), 0, int(u8), float(getattr(X, "hpnn_fm_scale", 1.0))
        if self.fused_mode == "t":
            raise ValueError("the tile path takes fragment-major batches (MLP.prepare_input)")
        if X.shape[0] < self.Bp or X.shape[1] != self.Kp[0] or X.stride(0) != self.Kp[0]:
            raise ValueError(f"batch {tuple(X.shape)} does not fit this plan (Bp {self.Bp}, Kp0 {self.Kp[0]})")
        xg = self._fm_input(X) if self.fused_mode == "x" else None
        # mode x: the u8 flag describes the fragment-major copy (8-bit pixels or BF16)
        return (X.data_ptr(), _p(xg), int(xg is not None and xg.dtype == torch.uint8),
                float(getattr(X, "hpnn_fm_scale", 1.0)))

    @staticmethod
    def _tgt(labels, T):
        return _p(labels), _p(T), (T.stride(0) if T is not None else 0)

    def _t_hilo(self):
        return (1.0, 0.0) if self.type == ops.TYPE_SNN else (1.0, -1.0)

    # ------------------------------------------------------------------ phases
    def forward(self, X):
        X = self._rowmajor(X)
        if self._gpu:
            self.plan.forward(X.data_ptr(), _stream())
            return self.Z
        for l in range(self.L):
            A = X if l == 0 else self.H[l - 1]
            if l == self.L - 1:
                ops.gemm_nt(A, self.Wb[l], ops.EPI_NONE, out_f32=True, out=self.Z)
            else:
                ops.gemm_nt(A, self.Wb[l], ops.EPI_ACT, out=self.H[l])
        return self.Z

    def output(self, labels=None, T=None, n_valid=None):
        n_valid = self.Bp if n_valid is None else int(n_valid)
        if self._gpu:
            self.plan.output(*self._tgt(labels, T), n_valid, 0, 0, True, _stream())
            return
        t_hi, t_lo = self._t_hilo()
        ops.output_delta(self.Z, self.n_out, self.type, self.D[-1], labels=labels, T=T, t_hi=t_hi, t_lo=t_lo,
                         n_valid=n_valid, loss_acc=self.stats[0, 0:1], correct=self.stats[0, 1:2])

    def backward_layer(self, l):
        """D[l-1] = (D[l] @ W_l) * f'(H[l-1]) (uses pre-update W_l^T)."""
        if self._gpu:
            self.plan.backward_layer(l, _stream())
            return
        ops.gemm_nt(self.D[l], self.Wt[l], ops.EPI_DACT, aux=self.H[l - 1], out=self.D[l - 1])

    def grad_layer(self, l, X, reduce=False):
        if self._gpu:
            self.plan.grad_layer(l, *self._x(X), bool(reduce), _stream())
            return
        Hin = X if l == 0 else self.H[l - 1]
        if reduce and self.S[l] == 1:
            ops.gemm_tn(self.D[l], Hin, splits=1, out=self.G[l].unsqueeze(0))
            return
        ops.gemm_tn(self.D[l], Hin, splits=self.S[l], out=self.slab[l])
        if reduce:
            ops.reduce_slabs(self.slab[l], self.G[l])

    def update_layer(self, l, lr, alpha, scale, from_G=False):
        if self.adam:
            raise RuntimeError("update_layer: Adam advances once per step and updates every layer in one launch "
                               "(train_step / update_all)")
        if self.sched:
            raise RuntimeError("update_layer: a scheduled plan updates every layer in one launch that reads the "
                               "device rate (train_step / update_all)")
        if self.clip:
            raise RuntimeError("update_layer: a clipping plan needs every layer's gradient for the norm and updates "
                               "them in one launch (train_step / update_all)")
        if self._gpu:
            self.plan.update_layer(l, float(lr), float(alpha), float(scale), bool(from_G), _stream())
            return
        G = self.G[l] if from_G else self.slab[l]
        ops.sgd_update(self.W32[l], self.V32[l], G, self.Wb[l], self.Wt[l], lr, alpha, scale, self.momentum)

    def update_all(self, lr, alpha, scale, grads=None):
        """every layer's optimizer step from the flat gradient buffer (the data-parallel
        all-reduce result), one launch"""
        if self._gpu:
            self.plan.update_flat(self.grad_flat.data_ptr(), float(lr), float(alpha), float(scale), _stream())
            return
        if self.adam:
            self._adam_update(scale, from_G=True)
            return
        if self.sched or self.clip:
            self._sched_update(alpha, scale, from_G=True)
            return
        for l in range(self.L):
            self.update_layer(l, lr, alpha, scale, from_G=True)

    def _adam_update(self, scale, from_G=False):
        """CPU emulation of the plan's optimizer under Adam: the advance, then every layer"""
        self._clip_factor(scale, from_G)
        ops.adam_advance(self.adam_state)
        ops.adam_update_multi([(self.W32[l], self.V32[l], self.A32[l], self.G[l] if from_G else self.slab[l],
                                self.Wb[l], self.Wt[l], self.W0f if l == 0 else None) for l in range(self.L)],
                              self.adam_state, scale, clip=self.clip_state)

    def _sched_update(self, alpha, scale, from_G=False):
        """CPU emulation of the plan's BP / BPM step under a schedule or [clip]: every layer, the
        state's rate"""
        self._clip_factor(scale, from_G)
        ops.sgd_sched_multi([(self.W32[l], self.V32[l], self.G[l] if from_G else self.slab[l], self.Wb[l], self.Wt[l],
                              self.W0f if l == 0 else None) for l in range(self.L)],
                            self.lr_state, alpha=alpha, scale=scale, momentum=self.momentum, clip=self.clip_state)

    def _clip_factor(self, scale, from_G=False):
        """CPU emulation of the plan's norm launches: the partials of every layer's padded gradient in
        the plan's slab order, then the finalize into clip_state"""
        if not self.clip:
            return
        t = ops.GnormTable([(self.G[l] if from_G else self.slab[l]).reshape(-1, self.Np[l] * self.Kp[l])
                            for l in range(self.L)], interleaved=True)
        ops.gnorm_partials(t, self.clip_part, scale)
        ops.clip_finalize(self.clip_part, t.count, self.clip_state)

    def commit_clip(self, hist=None, cursor=None):
        """the last launch of an epoch: the epoch's clip record appended to hist at cursor when given
        (ops.clip_history), the counters of clip_state zeroed (ops.clip_commit)"""
        if not self.clip:
            raise RuntimeError("commit_clip: the model does not clip")
        if self._gpu:
            self.plan.commit_clip(_p(hist), _p(cursor), hist.shape[0] if hist is not None else 0, _stream())
        else:
            ops.clip_commit(self.clip_state, hist, cursor)

    def advance_schedule(self, hist=None, cursor=None):
        """the first launch of an epoch: the rate of the next epoch into lr_state (and, under Adam,
        into adam_state), appended to hist at cursor when given (ops.lr_advance)"""
        if not self.sched:  # [clip] alone keeps a constant-rate state that nothing advances
            raise RuntimeError("advance_schedule: the model has no lr_schedule")
        if self._gpu:
            self.plan.advance_schedule(_p(hist), _p(cursor), hist.shape[0] if hist is not None else 0, _stream())
        else:
            ops.lr_advance(self.lr_state, self.adam_state, hist, cursor)

    def front(self, X, labels=None, T=None, n_valid=None):
        """fused modes: X -> the deltas (+ the [G1 | G2] block slabs), one launch"""
        n_valid = self.Bp if n_valid is None else int(n_valid)
        if not (self._gpu and self.fused):
            raise RuntimeError("front() needs a fused plan on a GPU")
        self.plan.front(*self._x(X), *self._tgt(labels, T), n_valid, _stream())

    _fused_front = front

    def backward_grads(self, X, labels=None, T=None, n_valid=None, reduce=True, on_ready=None):
        """forward + backward of one minibatch, the weight gradients summed into self.G[l]
        (the all-reduce buckets); on_ready(l) is called as soon as layer l's gradient is final
        (layers become ready from the last to the first)."""
        n_valid = self.Bp if n_valid is None else int(n_valid)
        if self._gpu:
            def ready(lo, hi):
                if on_ready:
                    for l in range(hi, lo - 1, -1):
                        on_ready(l)
                return True
            self.plan.grads(*self._x(X), *self._tgt(labels, T), n_valid, ready, _stream())
            return
        self.forward(X)
        self.output(labels=labels, T=T, n_valid=n_valid)
        for l in range(self.L - 1, -1, -1):
            if l > 0:
                self.backward_layer(l)
            self.grad_layer(l, X, reduce=True)
            if on_ready:
                on_ready(l)

    def grads_slabs(self, X, labels=None, T=None, n_valid=None, dst=None):
        """fused modes: front + first-layer gradient with the gradient left unreduced; returns
        [(address, slab stride, slabs, floats)] segments for the xGMI all-reduce's copy-in.
        dst = (address, selector address, half stride in floats) -- the all-reduce's own
        buffer (NativeComm.xar_local): when G0 reduces in-kernel the gradient goes there and
        the result is [] (nothing to copy in)"""
        n_valid = self.Bp if n_valid is None else int(n_valid)
        d, sel, alt = dst if dst is not None else (0, 0, 0)
        return self.plan.grads_slabs(*self._x(X), *self._tgt(labels, T), n_valid, _stream(), d, sel, alt)

    def train_step(self, X, labels=None, T=None, n_valid=None, lr=0.01, alpha=0.2):
        """One minibatch fwd + bwd + update on the current stream (no host sync).  Under Adam lr
        and alpha are ignored: the step size is the state's lr."""
        n_valid = self.Bp if n_valid is None else int(n_valid)
        if self._gpu:
            self.plan.step(*self._x(X), *self._tgt(labels, T), n_valid, float(lr), float(alpha), _stream())
            return
        scale = 1.0 / n_valid
        self.forward(X)
        self.output(labels=labels, T=T, n_valid=n_valid)
        for l in range(self.L - 1, -1, -1):
            if l > 0:
                self.backward_layer(l)  # pre-update W_l^T, before layer l's step below
            self.grad_layer(l, X)
            if not (self.adam or self.sched or self.clip):
                self.update_layer(l, lr, alpha, scale)
        if self.adam:
            self._adam_update(scale)
        elif self.sched or self.clip:
            self._sched_update(alpha, scale)

    def predict(self, X, n_valid=None):
        """network outputs [n_valid, n_out] (fp32)."""
        n_valid = (X.shape[0] * 32 if self._is_fm(X) else X.shape[0]) if n_valid is None else n_valid
        n_valid = min(int(n_valid), self.Bp)
        O = torch.empty(self.Bp, self.Np[-1], dtype=torch.float32, device=self.device)
        if self._gpu:
            self.plan.predict(self._rowmajor(X).data_ptr(), n_valid, O.data_ptr(), O.stride(0), _stream())
            return O[:n_valid, :self.n_out]
        self.forward(X)
        Tz = torch.zeros(self.Bp, self.n_out, dtype=torch.float32, device=self.device)
        ops.output_delta(self.Z, self.n_out, self.type, self.D[-1], T=Tz, n_valid=n_valid, O=O)
        return O[:n_valid, :self.n_out]

    def evaluate(self, X, labels=None, T=None, n_valid=None, guess=False):
        """Forward only (validation) on the current stream, no host sync: the loss and the
        argmax hits of the first n_valid rows of a prepared input X (any number of rows >=
        n_valid) are added into the validation stat slots (read_eval_stats), apart from the
        training statistics.  guess=True returns the int32 guesses (lowest index of the largest
        output, -1 from n_valid up).  The tile path makes one launch over the whole set
        (hpnn_mlp3_eval: the training front's numbers for the same batch and weights); every
        other plan -- and the tile path under HPNN_EVAL_FUSED=0 -- runs forward + the output
        kernel in chunks of Bp rows.  Weights, momenta, gradients and the training statistics
        are not touched; H, Z and the last D are scratch.  On CPU tensors: the emulation."""
        rows = X.shape[0] * 32 if self._is_fm(X) else X.shape[0]
        n_valid = rows if n_valid is None else int(n_valid)
        if n_valid < 1 or n_valid > rows:
            raise ValueError(f"n_valid {n_valid} outside the prepared input's {rows} rows")
        if labels is None and T is None:
            raise ValueError("evaluate needs labels or dense targets T")
        vst = self.buf[("vstats", -1)]
        ldt = T.stride(0) if T is not None else 0
        tally = self._cm is not None  # confusion(True): every chunk is tallied, which needs its guesses
        asked, guess = guess, guess or tally

        def tallied(g, r0=0, n=n_valid):
            """the caller's return value: the guesses only when asked for"""
            if tally:
                ops.confusion_add(g[r0:], self._cm, labels=None if labels is None else labels[r0:],
                                  T=None if labels is not None else T[r0:], rows=n)
            return g if asked else None
        if not self._gpu:
            A = self._rowmajor(X)[:n_valid]
            for l in range(self.L - 1):
                A = ops.gemm_nt(A, self.Wb[l], ops.EPI_ACT) if A.shape[0] % 128 == 0 else \
                    ops.ref_gemm_nt(A, self.Wb[l], ops.EPI_ACT).bfloat16()
            Z = A.float() @ self.Wb[-1].float().t()
            t_hi, t_lo = self._t_hilo()
            D = torch.empty(n_valid, self.Np[-1], dtype=torch.bfloat16)
            ops.output_delta(Z, self.n_out, self.type, D, labels=None if labels is None else labels[:n_valid],
                             T=None if T is None else T[:n_valid], t_hi=t_hi, t_lo=t_lo, n_valid=n_valid,
                             loss_acc=vst[0, 0:1], correct=vst[0, 1:2])
            if not guess:
                return None
            g = torch.full((rows,), -1, dtype=torch.int32)
            g[:n_valid] = Z[:, :self.n_out].argmax(1).to(torch.int32)
            return tallied(g)
        if self.plan.eval_is_fused() and self._is_fm(X):
            if X.shape[1] * 16 != self.Kp[0]:
                raise ValueError(f"fragment-major input {tuple(X.shape)} does not fit Kp0 {self.Kp[0]}")
            if ops.pad_to(n_valid, 256) > rows:
                raise ValueError("the tile path evaluates whole 256-row tiles: pad the prepared input")
            g = torch.empty(ops.pad_to(n_valid, 256), dtype=torch.int32, device=self.device) if guess else None
            self.plan.evaluate(X.data_ptr(), int(X.dtype == torch.uint8), float(getattr(X, "hpnn_fm_scale", 1.0)),
                               False, _p(labels), _p(T), ldt, n_valid, vst.data_ptr(), _p(g), _stream())
            return tallied(g)
        Xr = self._rowmajor(X)
        chunks = (n_valid + self.Bp - 1) // self.Bp
        if Xr.shape[0] < chunks * self.Bp:  # the per-layer kernels read whole Bp-row chunks
            Xr = torch.cat([Xr, Xr.new_zeros(chunks * self.Bp - Xr.shape[0], Xr.shape[1])])
        g = torch.full((chunks * self.Bp,), -1, dtype=torch.int32, device=self.device) if guess else None
        for c in range(chunks):
            r0 = c * self.Bp
            self.plan.evaluate(Xr[r0:].data_ptr(), 0, 1.0, True, _p(None if labels is None else labels[r0:]),
                               _p(None if T is None else T[r0:]), ldt, min(self.Bp, n_valid - r0), vst.data_ptr(),
                               _p(None if g is None else g[r0:]), _stream())
            tallied(g, r0, min(self.Bp, n_valid - r0))
        return g if asked else None

    # ------------------------------------------------------------------ keep the best pass
    def _masters(self):
        m = [t for l in range(self.L) for t in (self.W32[l], self.V32[l], self.A32[l]) if t is not None]
        m += [self.adam_state.view(torch.float32)] if self.adam else []
        return m + ([self.lr_state.view(torch.float32)] if self.sched else [])

    # ------------------------------------------------------------------ per-class metrics
    def confusion(self, enable=True, passes=64):
        """[confusion] (docs/DESIGN.md 3.2l): with enable, every evaluate() call also adds its rows
        into a device confusion matrix [n_out, n_out + 1] (ops.confusion_add per chunk), and
        commit_confusion files a pass: the per-class record into a history of `passes` records,
        the matrix kept as "last" and zeroed.  Under keep_best the kept pass's matrix survives as
        "best" (one more segment of the snapshot).  enable=False frees everything: evaluate()
        launches nothing more."""
        if not enable:
            self._cm = self._cm_last = self._cm_best = self._pc_hist = None
        else:
            self._cm = ops.confusion_matrix(self.n_out, self.device)
            self._cm_last, self._cm_best = torch.zeros_like(self._cm), torch.zeros_like(self._cm)
            self._pc_hist = torch.zeros(int(passes), 3 * self.n_out, dtype=torch.int32, device=self.device)
        if self._best is not None:
            self._snapshot_table()

    def commit_confusion(self, cursor):
        """in front of ops.validate_commit(vstats, hist, cursor) on the current stream: file the
        matrix the evaluate() calls since the last commit tallied, at the record index `cursor`
        holds (one launch, no host sync; capturable)"""
        ops.confusion_commit(self._cm, self._pc_hist, self._cm_last, cursor)

    def confusion_matrix(self, which="last"):
        """the matrix of the last pass filed ("last") or of the pass keep_best kept ("best") as a
        [n_out, n_out + 1] int64 CPU tensor; None when there is none (synchronises)"""
        if which not in ("last", "best"):
            raise ValueError(f"confusion_matrix: which {which!r} (last | best)")
        if self._cm is None:
            return None
        if which == "best" and (self._best is None or not self.best_state()["valid"]):
            return None
        return (self._cm_last if which == "last" else self._cm_best).cpu().long() & 0xffffffff

    def class_history(self, n):
        """the first n per-class records filed: dicts of support, hit, predicted (synchronises)"""
        return [ops.class_record(self._pc_hist, i) for i in range(n)]

    def _snapshot_table(self):
        pairs = list(zip(self._masters(), self._snap))
        if self._cm is not None:
            pairs.append((self._cm_last, self._cm_best))
        self._snap_table = ops.snapshot_table(pairs)

    def keep_best(self, metric="loss", patience=0):
        """allocate the best state and the snapshot of the FP32 masters (and the momentum) for
        commit_best (docs/DESIGN.md 3.2g); metric "loss" | "acc", patience 0 = never stop"""
        if metric not in ops.BEST_METRIC:
            raise ValueError(f"keep_best: metric {metric!r} (loss | acc)")
        self._best_metric, self._best_patience = metric, int(patience)
        self._best = ops.best_state(self.device)
        self._snap = [torch.zeros_like(t) for t in self._masters()]
        self._snapshot_table()

    def commit_best(self, hist, cursor):
        """behind ops.validate_commit(vstats, hist, cursor) on the current stream: judge the
        record just filed and copy the masters into the snapshot when it is the best so far
        (two launches, no host sync; capturable)"""
        ops.best_commit(hist, cursor, self._best, self._best_metric, self._best_patience)
        ops.snapshot_if(self._snap_table, self._best[7:8])

    def best_state(self):
        """the best state as a dict: loss_sum, hits, index (of the best record in the history),
        stale, stop, valid, take (synchronises)"""
        return ops.read_best_state(self._best)

    def restore_best(self):
        """the snapshot of the best pass back into W32 / V32 and the BF16 copies re-derived;
        False (nothing changed) when no pass was taken"""
        if not self.best_state()["valid"]:
            return False
        for t, s in zip(self._masters(), self._snap):
            t.copy_(s)
        self.refresh_bf16()
        return True

    def reset_eval_stats(self):
        self.buf[("vstats", -1)].zero_()

    def read_eval_stats(self):
        """(loss sum, hits) of the evaluate() calls since the last reset (synchronises)"""
        s = self.buf[("vstats", -1)].cpu()
        return float(s[:, 0].double().sum()), int(s[:, 1].contiguous().view(torch.int32).long().sum())

    def healthy(self):
        """False when an in-kernel hand-off (the fused G0's split-K tickets, a fused TN
        gradient's tickets, the wide front's tile pair) timed out since the model was made:
        that step used partial sums (synchronises the current stream)."""
        if not self._gpu:
            return True
        return self.plan.health(_stream()) == 0

    def weights_digest(self, which=3):
        """64-bit digest of the weights (1: BF16 copies, 2: FP32 masters, 3: both); data-
        parallel replicas hold bitwise-identical weights, so equal digests (synchronises)."""
        if self._gpu:
            return int(self.plan.weights_digest(int(which), _stream()))
        # a keyless, process-independent hash (Python's hash() of bytes is salted per process,
        # so replicas in different processes would never agree)
        h = hashlib.blake2b(digest_size=8)
        for l in range(self.L):
            ts = ([self.Wb[l], self.Wt[l]] if which & 1 else []) + ([self.W32[l]] if which & 2 else [])
            for t in ts:
                h.update(t.contiguous().view(-1).view(torch.int16 if t.element_size() == 2
                                                      else torch.int32).cpu().numpy().tobytes())
        return int.from_bytes(h.digest(), "little")

    def reset_stats(self):
        self.stats.zero_()

    def read_stats(self):
        s = self.stats.cpu()
        return float(s[:, 0].double().sum()), int(s[:, 1].contiguous().view(torch.int32).long().sum())
