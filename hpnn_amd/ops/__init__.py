"""gfx950 kernel wrappers (torch tensors in, raw pointers to libhpnn launchers).

Every function launches on torch's current HIP stream, so it composes with torch
streams/events and is captured by torch.cuda.graph.  `ref_*` functions are the plain
PyTorch FP32 references used by the numerics tests (and by the CPU path of the
distributed tests, which exercise the orchestration, not the kernels).
"""
import torch

from .._lib import native

EPI_NONE, EPI_ACT, EPI_DACT = 0, 1, 2
TYPE_ANN, TYPE_LNN, TYPE_SNN = 0, 1, 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cpu(t):
    """CPU tensors run the PyTorch emulation of the kernel (same rounding points);
    device tensors always run the native gfx950 kernel -- never a silent fallback."""
    return t.device.type == "cpu"


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def pad_to(v, m):
    return (v + m - 1) // m * m


# --------------------------------------------------------------------------- kernels
def gemm_nt(A, B, epi=EPI_NONE, aux=None, out_f32=False, out=None):
    """C[M,N] = epi(A[M,K] @ B[N,K]^T); A, B bf16 row-major (row strides may exceed K).

    epi: EPI_NONE, EPI_ACT (bipolar sigmoid), EPI_DACT (C *= -0.5(aux^2-1)).
    Shapes: M % 128 == 0, N % 32 == 0, K % 32 == 0."""
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=A.device)
    if _cpu(A):
        out.copy_(ref_gemm_nt(A, B, epi, aux))
        return out
    native().gemm_nt_bf16(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), out.stride(0),
                          _ptr(aux), aux.stride(0) if aux is not None else 0, M, N, K, epi, int(out_f32), _stream())
    return out


def _plan(arm, stages, names):
    return (names[arm] if arm >= 0 else arm), stages


def gemm_nt_arms():
    """names of the kernels hpnn_gemm_nt_bf16 chooses between (csrc/gpu/kernels_mfma.hip)"""
    return list(native().gemm_nt_arms())


def gemm_tn_arms():
    return list(native().gemm_tn_arms())


def gemm_nt_plan(M, N, K, lda, ldb, ldc, epi=EPI_NONE, has_aux=False, ldaux=0):
    """what gemm_nt launches for these arguments under the current toggles: (arm name, ring depth of
    its instantiation; 0 for the 8-phase schedule), or (refusal code < 0, 0).  Pure host arithmetic."""
    arm, st = native().gemm_nt_plan(int(M), int(N), int(K), int(lda), int(ldb), int(ldc), int(epi), int(has_aux),
                                    int(ldaux))
    return _plan(arm, st, gemm_nt_arms())


def gemm_tn_plan(N, M, Bt, splits, ldd, ldh, ldg):
    """the same for gemm_tn / gemm_tn_reduce"""
    arm, st = native().gemm_tn_plan(int(N), int(M), int(Bt), int(splits), int(ldd), int(ldh), int(ldg))
    return _plan(arm, st, gemm_tn_arms())


def gemm_nt_ws(X, W, epi, out):
    """out[M,N] = epi(X[M,K] @ W[N,K]^T) on the weight-stationary kernel (csrc/gpu/kernels_ws.hip) called
    directly, at any M % 32 == 0.  Returns 0, or 1 with nothing launched where the kernel has no instance
    (EPI_DACT, an (N, K) pair not instantiated, a row stride % 8); the CPU emulation refuses the same."""
    M, K = X.shape
    N = W.shape[0]
    if _cpu(X):
        if not native().gemm_nt_ws_plan(M, N, K, X.stride(0), W.stride(0), out.stride(0), epi):
            return 1
        out.copy_(ref_gemm_nt(X, W, epi, None))
        return 0
    return native().gemm_nt_ws_bf16(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(),
                                    out.stride(0), M, N, K, epi, int(out.dtype == torch.float32), _stream())


def gemm_nn(A, W, epi=EPI_NONE, aux=None, out_f32=False, out=None):
    """C[M,N] = epi(A[M,K] @ W[K,N]), W row-major [K][N]: the NT product on W^T without the transposed
    copy (M, N % 128, K % 64)."""
    M, K = A.shape
    N = W.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=A.device)
    if _cpu(A):
        out.copy_(ref_gemm_nt(A, W.t(), epi, aux))
        return out
    native().gemm_nn_bf16(A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), out.stride(0),
                          _ptr(aux), aux.stride(0) if aux is not None else 0, M, N, K, epi,
                          int(out.dtype == torch.float32), _stream())
    return out


def split_rows(Bt, splits):
    """batch rows of each split-K slice of gemm_tn: 64-row units, uneven when S does not
    divide them (csrc/gpu/kernels.h)"""
    if Bt % 64 == 0:
        U = Bt // 64
        return [(s * U // splits * 64, (s + 1) * U // splits * 64) for s in range(splits)]
    c = Bt // splits  # CPU emulation of tiny batches only
    return [(s * c, (s + 1) * c) for s in range(splits)]


def gemm_tn(D, H, splits=1, out=None):
    """slab[s, N, M] = sum over batch slice s of D[b, n] * H[b, m]  (FP32)."""
    Bt, N = D.shape
    M = H.shape[1]
    if out is None:
        out = torch.empty(splits, N, M, dtype=torch.float32, device=D.device)
    if _cpu(D):
        for s_, (a, b) in enumerate(split_rows(Bt, splits)):
            out[s_].copy_(ref_gemm_tn(D[a:b], H[a:b]))
        return out
    native().gemm_tn_bf16(D.data_ptr(), D.stride(0), H.data_ptr(), H.stride(0), out.data_ptr(), out.stride(1), N, M,
                          Bt, splits, _stream())
    return out


def gemm_tn_update(D, H, W32, V32, Wbf, Wt, lr, alpha=0.0, scale=1.0, momentum=False):
    """G = D^T H over the whole batch with the optimizer step of sgd_update (one slab) fused
    into the 8-phase TN kernel's epilogue (csrc/gpu/kernels_8ph.hip): the gradient never
    reaches memory.  Returns False (nothing launched) when the shape is not supported
    (N, M % 256, batch % 128); the CPU emulation always applies."""
    Bt, N = D.shape
    M = H.shape[1]
    if _cpu(D):
        G = ref_gemm_tn(D, H)
        sgd_update(W32, V32, G, Wbf, Wt, lr, alpha, scale, momentum)
        return True
    return bool(native().gemm_tn8_update(D.data_ptr(), D.stride(0), H.data_ptr(), H.stride(0), N, M, Bt,
                                         W32.data_ptr(), _ptr(V32) if momentum else 0, Wbf.data_ptr(), Wt.data_ptr(),
                                         float(lr), float(alpha), float(scale), int(bool(momentum)), _stream()))


class TnSide:
    """the side job of gemm_tn_fused_update: the next layer's gradient D^T H ([Bt, N] x [Bt, M],
    S splits into slab [S, N, M]) and its step on W32 / V32 / Wb [N, M] and Wt [M, N]; cnt: one
    int64 arrival counter, zeroed once and kept for this launch shape."""

    def __init__(self, D, H, S, slab, W32, V32, Wb, Wt, cnt):
        self.D, self.H, self.S, self.slab = D, H, int(S), slab
        self.W32, self.V32, self.Wb, self.Wt, self.cnt = W32, V32, Wb, Wt, cnt


def _sum_groups_of_8(slab):
    """the split-K sum of the fused TN update: batches of 16 partials, each group of 8 summed
    first (csrc/gpu/kernels_8ph.hip, MODE 2)"""
    g = torch.zeros_like(slab[0])
    for s0 in range(0, slab.shape[0], 8):
        t = slab[s0].clone()
        for s_ in range(s0 + 1, min(s0 + 8, slab.shape[0])):
            t += slab[s_]
        g += t
    return g


def _sum_sgd_tile(slab):
    """the slab sum of sgd_tile (csrc/gpu/kernels_misc.hip): slab 0, then slabs 1.. in four
    interleaved chains while four remain, the rest into chain 0, chain 0 + ((1 + 2) + 3)"""
    S = slab.shape[0]
    if S == 1:  # one slab is taken as it is (a -0.0 stays -0.0)
        return slab[0].clone()
    gend = 1 + 4 * ((S - 1) // 4)
    c = [slab[0].clone()] + [torch.zeros_like(slab[0]) for _ in range(3)]
    for k in range(1, S):
        c[0 if k >= gend else (k - 1) & 3] += slab[k]
    return c[0] + ((c[1] + c[2]) + c[3])


def gemm_tn_fused_update(D, H, splits, slab, W32, V32, Wbf, Wt, lr, alpha=0.0, scale=1.0, momentum=False, cnt=None,
                         err=None, side=None):
    """gemm_tn_update for a gradient over `splits` (>= 2) split-K slices, reduced inside the
    launch (csrc/gpu/kernels_8ph.hip, MODE 2): every split publishes its partial tile into slab
    [splits, N, M], the splits of a tile meet through the tile's 64-bit ticket in cnt (int64
    [512], zeroed once and kept for this GEMM shape: word 16 * tile gains `splits` per launch), then
    each reduces 1 / splits of the tile and steps it.  err (int32 [1]) is set when a wait timed
    out.  side (TnSide): the next layer's gradient and step carried by the same launch.
    Returns the launcher's code: 0, -1 (shape or grid not covered: nothing launched), -2 (the
    side job does not fit this grid).  The CPU emulation always applies."""
    Bt, N = D.shape
    M = H.shape[1]
    if _cpu(D):
        for s_, (a, b) in enumerate(split_rows(Bt, splits)):
            slab[s_].copy_(ref_gemm_tn(D[a:b], H[a:b]))
        sgd_update(W32, V32, _sum_groups_of_8(slab[:splits]), Wbf, Wt, lr, alpha, scale, momentum)
        ntiles = (N // 256) * (M // 256)
        cnt[0:16 * ntiles:16] += splits
        if side is not None:
            for s_, (a, b) in enumerate(split_rows(Bt, side.S)):
                side.slab[s_].copy_(ref_gemm_tn(side.D[a:b], side.H[a:b]))
            sgd_update(side.W32, side.V32, _sum_sgd_tile(side.slab[:side.S]), side.Wb, side.Wt, lr, alpha, scale,
                       momentum)
            side.cnt[0] += ntiles * splits
        return 0
    sd = None
    if side is not None:
        sd = (side.D.data_ptr(), side.D.stride(0), side.H.data_ptr(), side.H.stride(0), side.slab.data_ptr(),
              side.D.shape[1], side.H.shape[1], side.S, side.W32.data_ptr(), _ptr(side.V32) if momentum else 0,
              side.Wb.data_ptr(), side.Wt.data_ptr(), side.cnt.data_ptr())
    return native().gemm_tn8_fused_update(D.data_ptr(), D.stride(0), H.data_ptr(), H.stride(0), N, M, Bt, int(splits),
                                          slab.data_ptr(), W32.data_ptr(), _ptr(V32) if momentum else 0,
                                          Wbf.data_ptr(), Wt.data_ptr(), float(lr), float(alpha), float(scale),
                                          int(bool(momentum)), cnt.data_ptr(), err.data_ptr(), sd, _stream())


def gemm_tn_bf16out_ok(N, M, Bt, ldd, ldh):
    """whether gemm_tn_bf16out covers the shape (N, M % 256, an even number of 64-row units,
    operand strides % 8); pure host arithmetic"""
    return bool(native().gemm_tn8_bf16out_ok(int(N), int(M), int(Bt), int(ldd), int(ldh)))


def gemm_tn_bf16out(D, H, G16):
    """G16[:, :M] (BF16, row stride >= M) = bf16(D^T H) over the whole batch, one rounding of the
    FP32 sum (csrc/gpu/kernels_8ph.hip, MODE 3: the send buffer of the data-parallel BF16
    exchange).  Returns the launcher's code: 0, or -1 (shape not covered: nothing launched); the
    CPU emulation always applies."""
    Bt, N = D.shape
    M = H.shape[1]
    if _cpu(D):
        G16[:, :M] = ref_gemm_tn(D, H).bfloat16()
        return 0
    return native().gemm_tn8_bf16out(D.data_ptr(), D.stride(0), H.data_ptr(), H.stride(0), G16.data_ptr(),
                                     G16.stride(0), N, M, Bt, _stream())


def gemm_tn_reduce(D, H, splits, out, rslab, groups, rout):
    """gemm_tn(D, H, splits, out) and reduce_groups(rslab, groups, rout) in ONE launch:
    the reduction runs on workgroups appended to the GEMM grid (csrc/gpu/kernels.h)."""
    if _cpu(D):
        gemm_tn(D, H, splits=splits, out=out)
        return reduce_groups(rslab, groups, rout)
    Bt, N = D.shape
    M = H.shape[1]
    native().gemm_tn_bf16_reduce(D.data_ptr(), D.stride(0), H.data_ptr(), H.stride(0), out.data_ptr(), out.stride(1),
                                 N, M, Bt, splits, rslab.data_ptr(), rslab.shape[0], rslab.stride(0), rslab[0].numel(),
                                 groups, rout.data_ptr(), _stream())
    return rout


def to_fragment_major(A):
    """[Bt, M] (batch rows) -> fragment-major [Bt/32, M/16, 64, 8]: lane l = 16 g + r of
    fragment (t, rb) holds A[t*32 + 8g + j, rb*16 + r], j < 8 (the MFMA operand layout of a
    k = batch product, one contiguous 1 KiB per 16 x 32 fragment)"""
    Bt, M = A.shape
    return A.reshape(Bt // 32, 4, 8, M // 16, 16).permute(0, 3, 1, 4, 2).contiguous()


def from_fragment_major(Ag, rows, cols):
    """inverse of to_fragment_major"""
    return Ag.view(rows // 32, cols // 16, 4, 16, 8).permute(0, 2, 4, 1, 3).reshape(rows, cols)


def gemm_fm_direct(Dg, Hg, N, M, splits=1, out=None, hscale=1.0):
    """slab[s, N, M] = sum over batch slice s of D[b, n] * H[b, m] (gemm_tn) with D, H
    given fragment-major (to_fragment_major), direct-to-register loads
    (csrc/gpu/kernels_g0.hip).  Hg may be uint8 (pixel data): multiplied as exact integers,
    the result scaled by hscale."""
    Bt = Dg.numel() // N
    u8 = Hg.dtype == torch.uint8
    if out is None:
        out = torch.empty(splits, N, M, dtype=torch.float32, device=Dg.device)
    if _cpu(Dg):
        # u8: the exact integers (BF16 holds 0..255 exactly), hscale on the FP32 result
        H = from_fragment_major(Hg, Bt, M)
        gemm_tn(from_fragment_major(Dg, Bt, N), H.bfloat16() if u8 else H, splits=splits, out=out)
        if u8:
            out *= hscale
        return out
    native().gemm_fm_direct(Dg.data_ptr(), Hg.data_ptr(), int(u8), float(hscale), out.data_ptr(), out.stride(1), N, M,
                            Bt, splits, _stream())
    return out


def gemm_fm_direct_reduce(Dg, Hg, N, M, splits, out, rslab, groups, rout, hscale=1.0):
    """gemm_fm_direct and reduce_groups(rslab, groups, rout) in ONE launch"""
    if _cpu(Dg):
        gemm_fm_direct(Dg, Hg, N, M, splits=splits, out=out, hscale=hscale)
        return reduce_groups(rslab, groups, rout)
    Bt = Dg.numel() // N
    native().gemm_fm_direct_reduce(Dg.data_ptr(), Hg.data_ptr(), int(Hg.dtype == torch.uint8), float(hscale),
                                   out.data_ptr(), out.stride(1), N, M, Bt, splits, rslab.data_ptr(), rslab.shape[0],
                                   rslab.stride(0), rslab[0].numel(), groups, rout.data_ptr(), _stream())
    return rout


def output_delta(Z, n_out, net_type, D, labels=None, T=None, t_hi=1.0, t_lo=0.0, n_valid=None, O=None,
                 loss_acc=None, correct=None):
    """Output layer: activation/softmax, loss sum, delta (bf16) and argmax hits."""
    B = Z.shape[0]
    if _cpu(Z):
        return _cpu_output_delta(Z, n_out, net_type, D, labels, T, t_hi, t_lo, B if n_valid is None else int(n_valid),
                                 O, loss_acc, correct)
    native().output_delta(Z.data_ptr(), Z.stride(0), _ptr(T), T.stride(0) if T is not None else 0, _ptr(labels),
                          float(t_hi), float(t_lo), D.data_ptr(), D.stride(0), _ptr(O),
                          O.stride(0) if O is not None else 0, _ptr(loss_acc), _ptr(correct), B,
                          B if n_valid is None else int(n_valid), n_out, net_type, _stream())
    return D


def reduce_slabs(slab, out):
    S = slab.shape[0]
    n = slab[0].numel()
    if _cpu(slab):
        out.view(-1).copy_(slab.reshape(S, -1).sum(0))
        return out
    native().reduce_slabs(slab.data_ptr(), S, slab.stride(0), n, out.data_ptr(), _stream())
    return out


def reduce_slabs2(slab, out, tmp=None):
    """out = slab.sum(0), deterministic two-pass reduction (tmp: >= 16 * slab[0].numel()
    floats of scratch; None = single pass)."""
    S = slab.shape[0]
    n = slab[0].numel()
    if _cpu(slab):
        out.view(-1).copy_(slab.reshape(S, -1).sum(0))
        return out
    native().reduce_slabs2(slab.data_ptr(), S, slab.stride(0), n, _ptr(tmp), out.data_ptr(), _stream())
    return out


UPD_MAX = 8  # HPNN_UPD_MAX (csrc/gpu/kernels.h): layers per sgd_update_multi launch
MLP3_DIMS = (128, 64, 32)


def mlp3_mid(H1, W1, W1t, W2, W2t, D1, gslab, n_out, net_type, labels=None, T=None, t_hi=1.0, t_lo=0.0,
             n_valid=None, loss_acc=None, correct=None):
    """Fused middle of the n_in-128-64-(<=32) MLP step (csrc/gpu/kernels_mlp3.hip):
    H1 -> H2 -> output/loss -> delta3 -> delta2 -> delta1 (into D1), per-block
    [G1 | G2] FP32 slabs into gslab [grid, 64*128 + 32*64]."""
    Bp = H1.shape[0]
    grid = gslab.shape[0]
    n_valid = Bp if n_valid is None else int(n_valid)
    if _cpu(H1):
        return _cpu_mlp3_mid(H1, W1, W1t, W2, W2t, D1, gslab, n_out, net_type, labels, T, t_hi, t_lo, n_valid,
                             loss_acc, correct)
    native().mlp3_mid(H1.data_ptr(), W1.data_ptr(), W1t.data_ptr(), W2.data_ptr(), W2t.data_ptr(), _ptr(labels),
                      _ptr(T), T.stride(0) if T is not None else 0, float(t_hi), float(t_lo), D1.data_ptr(),
                      gslab.data_ptr(), _ptr(loss_acc), _ptr(correct), Bp, n_valid, n_out, net_type, *MLP3_DIMS,
                      grid, _stream())
    return D1


MLP3F_K0 = (256, 512, 800, 832, 896)  # first-layer input widths of hpnn_mlp3_fused
MLP3_SLAB = 128 * 64 + 64 * 32


def mlp3_fused_grid(Bp, device=None):
    """workgroups (= gradient slab rows) hpnn_mlp3_fused uses for Bp samples."""
    if device is not None and torch.device(device).type == "cpu":
        return 1
    g = native().mlp3_fused_grid(int(Bp), 0)
    if g <= 0:
        raise ValueError(f"mlp3_fused: batch {Bp} not a multiple of 32")
    return g


def mlp3_fused(X, W0, W0f, W1, W2, D1, gslab, n_out, net_type, labels=None, T=None, t_hi=1.0, t_lo=0.0,
               n_valid=None, loss_acc=None, correct=None, d1_fm=False):
    """Whole n_in-128-64-(<=32) step up to delta1 in one persistent kernel
    (csrc/gpu/kernels_mlp3.hip, mlp3_fused_kernel): X [Bp, K0] -> delta1 into D1
    [Bp, 128], per-block [G1 | G2] slabs into gslab [grid, MLP3_SLAB], loss/hits.
    W0f: fragment-major BF16 copy of W0 (frag_major); W0 (row-major) is only used by
    the CPU emulation.  d1_fm: D1 receives delta1 fragment-major (to_fragment_major
    layout, the operand of gemm_fm_direct) instead of row-major."""
    Bp, K0 = X.shape[0], W0.shape[1]
    n_valid = Bp if n_valid is None else int(n_valid)
    if _cpu(X):
        H1 = bipolar(X[:, :K0].float() @ W0.float().t()).bfloat16()
        out = _cpu_mlp3_mid(H1, W1, None, W2, None, D1, gslab, n_out, net_type, labels, T, t_hi, t_lo, n_valid,
                            loss_acc, correct)
        if d1_fm:
            D1.view(-1).copy_(to_fragment_major(D1.clone()).view(-1))
        return out
    native().mlp3_fused(X.data_ptr(), X.stride(0), K0, W0f.data_ptr(), W1.data_ptr(), W2.data_ptr(), _ptr(labels),
                        _ptr(T), T.stride(0) if T is not None else 0, float(t_hi), float(t_lo), D1.data_ptr(),
                        gslab.data_ptr(), _ptr(loss_acc), _ptr(correct), Bp, n_valid, n_out, net_type,
                        gslab.shape[0], int(bool(d1_fm)), _stream())
    return D1


MLP3T_K0 = (256, 800)  # first-layer input widths of hpnn_mlp3_tile
MLP3T_TILE = 256  # samples per tile (the batch must be a multiple)


def mlp3_tile_grid(Bp, device=None):
    """workgroups (= gradient slab rows) hpnn_mlp3_tile uses for Bp samples."""
    if device is not None and torch.device(device).type == "cpu":
        return 1
    g = native().mlp3_tile_grid(int(Bp), 0)
    if g <= 0:
        raise ValueError(f"mlp3_tile: batch {Bp} not a multiple of {MLP3T_TILE}")
    return g


def mlp3_tile(Xg, K0, W0, W0f, W1, W2, W2t, D1g, gslab, n_out, net_type, labels=None, T=None, t_hi=1.0, t_lo=0.0,
              n_valid=None, loss_acc=None, correct=None, xscale=1.0):
    """The n_in-128-64-(<=32) step up to delta1 with 256-sample tiles
    (csrc/gpu/kernels_mlp3t.hip): Xg fragment-major [Bp/32, K0/16, 64, 8] (to_fragment_major)
    uint8 (exact integers, H1 = f(xscale * X W0^T)) or bf16 -> delta1 fragment-major into D1g
    [Bp/32, 8, 64, 8] bf16, per-block [G1 | G2] slabs into gslab [grid, MLP3_SLAB],
    loss / hits.  W0f: fragment-major BF16 W0 (frag_major); W0 (row-major) is used by the
    CPU emulation only; W2t: W2^T [64, 32] BF16."""
    Bp = Xg.shape[0] * 32
    n_valid = Bp if n_valid is None else int(n_valid)
    u8 = Xg.dtype == torch.uint8
    if _cpu(Xg):
        X = from_fragment_major(Xg, Bp, K0)
        H1 = bipolar((X.float() @ W0.float().t()) * xscale).bfloat16()
        D1 = torch.empty(Bp, 128, dtype=torch.bfloat16)
        _cpu_mlp3_mid(H1, W1, None, W2, None, D1, gslab, n_out, net_type, labels, T, t_hi, t_lo, n_valid, loss_acc,
                      correct)
        D1g.view(-1).copy_(to_fragment_major(D1).view(-1))
        return D1g
    native().mlp3_tile(Xg.data_ptr(), int(u8), float(xscale), K0, W0f.data_ptr(), W1.data_ptr(), W2.data_ptr(),
                       W2t.data_ptr(), _ptr(labels), _ptr(T), T.stride(0) if T is not None else 0, float(t_hi),
                       float(t_lo), D1g.data_ptr(), gslab.data_ptr(), _ptr(loss_acc), _ptr(correct), Bp, n_valid,
                       n_out, net_type, gslab.shape[0], _stream())
    return D1g


def mlp3_eval(Xg, K0, W0, W0f, W1, W2, n_out, net_type, labels=None, T=None, t_hi=1.0, t_lo=0.0, n_valid=None,
              loss_acc=None, correct=None, guess=None, xscale=1.0, grid=0):
    """Forward-only form of mlp3_tile (validation; csrc/gpu/kernels_mlp3t.hip, EVAL): the same
    fragment-major input and weights, the same rounding points, so the loss and the argmax hits
    of the first n_valid rows (added into loss_acc / correct, stat-slot layout) are the numbers
    the training front reports for the batch.  guess (optional int32 [Bp]): the lowest index of
    the largest logit, -1 from n_valid up.  No deltas, no slabs.  grid: workgroups (0 = one per
    CU, capped at the tiles).  W0 (row-major) is used by the CPU emulation only."""
    Bp = Xg.shape[0] * 32
    n_valid = Bp if n_valid is None else int(n_valid)
    u8 = Xg.dtype == torch.uint8
    if _cpu(Xg):
        X = from_fragment_major(Xg, Bp, K0)
        H1 = bipolar((X.float() @ W0.float().t()) * xscale).bfloat16()
        H2 = bipolar(H1.float() @ W1.float().t()).bfloat16()
        Z = H2.float() @ W2.float().t()
        D3 = torch.empty(Bp, W2.shape[0], dtype=torch.bfloat16)
        _cpu_output_delta(Z, n_out, net_type, D3, labels, T, t_hi, t_lo, n_valid, None, loss_acc, correct,
                          front=True)
        if guess is not None:  # the lowest index of the largest logit
            z = Z[:n_valid, :n_out]
            col = torch.arange(n_out).expand_as(z)
            low = torch.where(z == z.max(1, keepdim=True).values, col, torch.full_like(col, n_out)).min(1).values
            guess.fill_(-1)
            guess[:n_valid] = low.to(torch.int32)
        return guess
    native().mlp3_eval(Xg.data_ptr(), int(u8), float(xscale), K0, W0f.data_ptr(), W1.data_ptr(), W2.data_ptr(),
                       _ptr(labels), _ptr(T), T.stride(0) if T is not None else 0, float(t_hi), float(t_lo),
                       _ptr(loss_acc), _ptr(correct), _ptr(guess), Bp, n_valid, n_out, net_type, int(grid), _stream())
    return guess


def validate_commit(slots, hist, cursor):
    """file one validation pass: the 64 stat slots summed in slot order (the float loss at [0]
    plus the double the FP64 / FP32 engines keep in floats 2..3) -> hist[cursor] = (float64 loss
    sum, uint32 hits, pad), the slots zeroed, cursor += 1 (a full history drops the record).  hist: [cap, 2] float64 (row = 16 bytes), cursor: [1] int32; one capturable launch."""
    cap = hist.shape[0]
    if _cpu(slots):
        c = int(cursor[0])
        if c < cap:
            hist[c, 0] = slots[:, 0].double().sum() + slots[:, 2:4].contiguous().view(torch.float64).sum()
            hist[c, 1:2].view(torch.int32)[0] = int(slots[:, 1].contiguous().view(torch.int32).long().sum())
            hist[c, 1:2].view(torch.int32)[1] = 0
            cursor[0] = c + 1
        slots[:, :4] = 0
        return hist
    native().validate_commit(slots.data_ptr(), hist.data_ptr(), cursor.data_ptr(), cap, _stream())
    return hist


BEST_METRIC = {"loss": 1, "acc": 2}  # HPNN_BEST_LOSS / HPNN_BEST_ACC (= nn_keep_best)
BEST_WORDS = ("hits", "index", "stale", "stop", "valid", "take")  # int32 words 2..7 of a best state


def best_state(device="cpu"):
    """a zeroed hpnn_best_state as [8] int32: the float64 loss sum in words 0..1, then hits,
    index, stale, stop, valid, take"""
    return torch.zeros(8, dtype=torch.int32, device=device)


def read_best_state(state):
    """the best state as a dict (synchronises)"""
    s = state.cpu()
    d = {k: int(s[2 + i]) & 0xffffffff for i, k in enumerate(BEST_WORDS)}
    d["loss_sum"] = float(s[0:2].view(torch.float64)[0])
    return d


def best_commit(hist, cursor, state, metric="loss", patience=0):
    """judge the record validate_commit has just filed (hist[cursor - 1]) against the best so far
    (csrc/gpu/kernels_best.hip; docs/DESIGN.md 3.2g) and set the take word of `state`
    (best_state()).  metric "loss": a smaller loss sum; "acc": more hits, the loss breaking
    ties; nothing is best before the first pass (loss: the first pass whose loss is not a NaN is
    taken), ties do not improve.  An improving pass zeroes stale, any other adds one; patience >
    0: the pass at which stale == patience sets stop, and the state is frozen from then on.
    cursor == 0: a no-op.  One capturable one-thread launch; on CPU tensors the same rule in
    PyTorch, bit for bit."""
    m = BEST_METRIC[metric] if isinstance(metric, str) else int(metric)
    if m not in (1, 2):
        raise ValueError(f"best_commit: metric {metric!r}")
    if _cpu(hist):
        c = int(cursor[0])
        if c == 0 or int(state[5]):
            state[7] = 0
            return state
        loss = float(hist[c - 1, 0])
        hits = int(hist[c - 1, 1:2].view(torch.int32)[0]) & 0xffffffff
        b_loss = float(state[0:2].view(torch.float64)[0])
        b_hits = int(state[2]) & 0xffffffff
        if not int(state[6]):
            better = m == 2 or loss == loss
        elif m == 2:
            better = hits > b_hits or (hits == b_hits and loss < b_loss)
        else:
            better = loss < b_loss
        if better:
            state[0:2].copy_(hist[c - 1, 0:1].view(torch.int32))
            state[2] = hist[c - 1, 1:2].view(torch.int32)[0]
            state[3], state[4], state[6], state[7] = c - 1, 0, 1, 1
        else:
            state[4] += 1
            state[7] = 0
        if patience and (int(state[4]) & 0xffffffff) == int(patience):
            state[5] = 1
        return state
    rc = native().best_commit(hist.data_ptr(), cursor.data_ptr(), state.data_ptr(), m, int(patience), _stream())
    if rc:
        raise RuntimeError(f"best_commit failed (rc={rc})")
    return state


def snapshot_table(pairs):
    """the segment table of snapshot_if for (src, dst) tensor pairs of equal byte size (at most
    32; any multiple of 4 bytes; both 16-byte aligned, else ValueError and nothing is written).
    Device tensors: a [n, 3] int64 device tensor {src, dst, bytes} (it keeps the pairs alive);
    CPU tensors: the list itself."""
    pairs = [(s, d) for s, d in pairs]
    for s, d in pairs:
        if s.numel() * s.element_size() != d.numel() * d.element_size():
            raise ValueError("snapshot_table: src and dst differ in size")
        if not (s.is_contiguous() and d.is_contiguous()):
            raise ValueError("snapshot_table: contiguous tensors only")
    if not pairs or _cpu(pairs[0][0]):
        if len(pairs) > 32:
            raise ValueError("snapshot_table: more than 32 segments")
        return pairs
    segs = torch.zeros(len(pairs), 3, dtype=torch.int64, device=pairs[0][0].device)
    rc = native().snapshot_table(segs.data_ptr(), [(s.data_ptr(), d.data_ptr(), s.numel() * s.element_size())
                                                   for s, d in pairs], _stream())
    if rc:
        raise ValueError(f"snapshot_table refused the segments (rc={rc}): 16-byte aligned pointers, sizes a "
                         "multiple of 4, at most 32 segments")
    segs.hpnn_pairs = pairs
    return segs


def snapshot_if(segs, take):
    """copy every segment of a snapshot_table when the word take[0] is not 0 -- read from memory
    when the launch runs, so a captured launch follows the flag of each replay -- and do nothing
    when it is 0.  One capturable launch (16-byte vector copies, a 4-byte tail); on CPU tensors
    the same in PyTorch."""
    if isinstance(segs, list):
        if int(take[0]) != 0:
            for s, d in segs:
                d.view(-1).view(torch.uint8).copy_(s.view(-1).view(torch.uint8))
        return
    rc = native().snapshot_if(segs.data_ptr(), segs.shape[0], take.data_ptr(), _stream())
    if rc:
        raise RuntimeError(f"snapshot_if failed (rc={rc})")


# --------------------------------------------------------------------------- [confusion]
GUESS_PAD, GUESS_NONE = -1, 1 << 30  # HPNN_GUESS_PAD / HPNN_GUESS_NONE (include/libhpnn/confusion.h)
_CONFUSION_KIND = {torch.int32: 0, torch.float32: 1, torch.float64: 2}


def confusion_matrix(n_out, device="cpu"):
    """a zeroed confusion matrix [n_out, n_out + 1] int32 (uint32 counts; the last column is "none")"""
    return torch.zeros(n_out, n_out + 1, dtype=torch.int32, device=device)


def confusion_add(guess, M, labels=None, T=None, rows=None):
    """add the first `rows` rows (default: all of guess) of one evaluation chunk into the confusion
    matrix M [n_out, n_out + 1] int32 (csrc/gpu/kernels_confusion.hip; the rule is
    include/libhpnn/confusion.h): M[t, g] += 1 for every row of target class t guessed g.  guess:
    int32 as the evaluation kernels write it (-1: not a sample; >= n_out: the "none" column).
    Targets: int32 labels (a label outside [0, n_out) skips its row) or dense float32 / float64 rows
    T (row stride >= n_out; the lowest index of the largest value).  Integer atomics only, so the
    result is the same bits whatever the grid.  One capturable launch; on CPU tensors the same counts in PyTorch integers."""
    if (labels is None) == (T is None):
        raise ValueError("confusion_add needs labels or dense targets T, not both")
    n_out = M.shape[0]
    if M.dtype != torch.int32 or M.shape[1] != n_out + 1 or not M.is_contiguous():
        raise ValueError("confusion_add: M is a contiguous [n_out, n_out + 1] int32 tensor")
    tgt = labels if T is None else T
    rows = guess.shape[0] if rows is None else int(rows)
    if tgt.dtype not in _CONFUSION_KIND or (T is None) != (tgt.dtype == torch.int32):
        raise ValueError(f"confusion_add: targets of dtype {tgt.dtype}")
    if guess.dtype != torch.int32 or rows > guess.shape[0] or rows > tgt.shape[0] or rows < 0:
        raise ValueError("confusion_add: guess is int32 with at least `rows` entries, as the targets")
    if T is not None and (T.shape[1] < n_out or T.stride(1) != 1):
        raise ValueError("confusion_add: T has at least n_out columns of stride 1")
    if _cpu(guess):
        g = guess[:rows].long()
        if T is None:
            t = labels[:rows].long()
        else:  # the lowest index of the largest value; NaNs never compare, a NaN at [0] gives 0
            x = T[:rows, :n_out]
            clean = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
            col = torch.arange(n_out).expand_as(clean)
            t = torch.where(clean == clean.max(1, keepdim=True).values, col, torch.full_like(col, n_out)).min(1).values
            t = torch.where(torch.isnan(x[:, 0]), torch.zeros_like(t), t)
        ok = (g >= 0) & (t >= 0) & (t < n_out)
        cell = t[ok] * (n_out + 1) + g[ok].clamp(max=n_out)
        counts = torch.bincount(cell, minlength=n_out * (n_out + 1))
        M.view(-1).copy_(_u32((M.view(-1).long() & 0xffffffff) + counts))
        return M
    rc = native().confusion_add(guess.data_ptr(), tgt.data_ptr(), T.stride(0) if T is not None else 0,
                                _CONFUSION_KIND[tgt.dtype], rows, n_out, M.data_ptr(), _stream())
    if rc:
        raise RuntimeError(f"confusion_add failed (rc={rc})")
    return M


def _u32(x):
    """int64 values mod 2^32 as the int32 tensor with those bits"""
    x = x & 0xffffffff
    return torch.where(x >= 1 << 31, x - (1 << 32), x).to(torch.int32)


def confusion_commit(M, pc_hist, last, cursor):
    """file one pass, in front of validate_commit: the per-class record -- support (row sums), hit
    (diagonal), predicted (column sums), n_out words each -- into pc_hist[cursor] (pc_hist: [cap,
    3 * n_out] int32; a cursor at cap drops the record), M copied to `last` (may be None), M zeroed.
    The cursor ([1] int32) is read, not advanced: validate_commit does that.  One capturable
    one-workgroup launch; on CPU tensors the same in PyTorch integers."""
    n_out = M.shape[0]
    if pc_hist is not None and (pc_hist.dtype != torch.int32 or pc_hist.shape[1] != 3 * n_out or
                                not pc_hist.is_contiguous()):
        raise ValueError("confusion_commit: pc_hist is a contiguous [cap, 3 * n_out] int32 tensor")
    if last is not None and (last.shape != M.shape or last.dtype != torch.int32 or not last.is_contiguous()):
        raise ValueError("confusion_commit: last has the shape and dtype of M")
    cap = 0 if pc_hist is None else pc_hist.shape[0]
    if _cpu(M):
        c = int(cursor[0]) & 0xffffffff
        if c < cap:
            m = M.long() & 0xffffffff
            pc_hist[c, :n_out] = _u32(m.sum(1))
            pc_hist[c, n_out:2 * n_out] = M.diagonal()
            pc_hist[c, 2 * n_out:] = _u32(m[:, :n_out].sum(0))
        if last is not None:
            last.copy_(M)
        M.zero_()
        return pc_hist
    rc = native().confusion_commit(M.data_ptr(), n_out, _ptr(pc_hist), _ptr(last), cursor.data_ptr(), cap, _stream())
    if rc:
        raise RuntimeError(f"confusion_commit failed (rc={rc})")
    return pc_hist


def class_record(pc_hist, index):
    """record `index` of a per-class history as a dict of int lists: support, hit, predicted
    (synchronises)"""
    r = (pc_hist[index].cpu().long() & 0xffffffff).tolist()
    n = len(r) // 3
    return {"support": r[:n], "hit": r[n:2 * n], "predicted": r[2 * n:]}


def balanced_accuracy(support, hit):
    """the mean of hit[c] / support[c] over the classes with support, in float64, in class order,
    additions and divisions only (hpnn_balanced_accuracy: the same bits as the C rule); 0.0 when no
    class has support"""
    total, classes = 0.0, 0.0
    for s, h in zip([int(v) for v in support], [int(v) for v in hit]):
        if s:
            total = total + float(h) / float(s)
            classes = classes + 1.0
    return total / classes if classes > 0.0 else 0.0


# --------------------------------------------------------------------------- [train] CG
CG_TRIALS, CG_PARABOLA, CG_FINAL = 6, 6, 7  # HPNN_CG_TRIALS / _PARABOLA / _FINAL (include/libhpnn/cg.h)
CG_NONE = 0xffffffff
CG_FAILED, CG_RESTART, CG_VERTEX, CG_TOOK7 = 1, 2, 4, 8
_CG_D = ("gg", "gp", "gd", "gg_prev", "beta", "a_init")  # float64 words 0..5 of a CG state
_CG_U = ("hits0", "first", "jstar", "flags", "cursor", "cap", "n")  # int32 words 44..50


def cg_state(a_init, n, cap, device="cpu"):
    """a fresh hpnn_cg_state as [26] float64: gg, gp, gd, gg_prev, beta, a_init, a[8], phi[8]
    (phi[7] = f0), then the int32 words hits0, first, jstar, flags, cursor, cap, n, pad"""
    st = torch.zeros(26, dtype=torch.float64)
    native().cg_host_init(st.data_ptr(), float(a_init), int(n), int(cap))
    return st.to(device)


def read_cg_state(state):
    """the CG state as a dict (synchronises)"""
    s = state.cpu()
    u = s.view(torch.int32)
    out = {k: float(s[i]) for i, k in enumerate(_CG_D)}
    out["a"] = [float(x) for x in s[6:14]]
    out["phi"] = [float(x) for x in s[14:22]]
    out.update({k: int(u[44 + i]) & 0xffffffff for i, k in enumerate(_CG_U)})
    return out


def write_cg_state(state, **kw):
    """set fields of a CG state (names of read_cg_state; a / phi as 8-lists); returns the state"""
    s = state.cpu().clone()
    u = s.view(torch.int32)
    for k, v in kw.items():
        if k in _CG_D:
            s[_CG_D.index(k)] = v
        elif k in ("a", "phi"):
            o = 6 if k == "a" else 14
            s[o:o + 8] = torch.tensor(v, dtype=torch.float64)
        else:
            v = int(v) & 0xffffffff
            u[44 + _CG_U.index(k)] = v - (1 << 32) if v >= 1 << 31 else v
    state.copy_(s)
    return state


def cg_history(cap, device="cpu"):
    """a zeroed history of cap hpnn_cg_record rows as [cap, 5] float64: f0, f1, beta, alpha, then
    the int32 words trial and flags"""
    return torch.zeros(max(int(cap), 1), 5, dtype=torch.float64, device=device)


def read_cg_history(hist, count):
    h = hist.cpu()
    out = []
    for i in range(int(count)):
        w = h[i, 4:5].view(torch.int32)
        t = int(w[0]) & 0xffffffff
        out.append({"f0": float(h[i, 0]), "f1": float(h[i, 1]), "beta": float(h[i, 2]), "alpha": float(h[i, 3]),
                    "trial": None if t == CG_NONE else t, "flags": int(w[1]) & 0xffffffff})
    return out


class CgTable:
    """the segment table of the cg_* ops: one segment per layer, a dict of flat (element stride 1)
    tensors of one dtype (float64 / float32) under the keys w, w0, g, gprev, d -- only those the
    ops called need be given -- and slab: [S, n] with any row stride.  At most 16 segments.
    Device tensors: uploaded once (a [n, 9] int64 device tensor that keeps the tensors alive)."""

    def __init__(self, segs):
        self.segs = [dict(s) for s in segs]
        if not 1 <= len(self.segs) <= 16:
            raise ValueError("CgTable: 1..16 segments")
        any_t = next(t for t in self.segs[0].values() if t is not None)
        self.dtype, self.device = any_t.dtype, any_t.device
        if self.dtype not in (torch.float64, torch.float32):
            raise ValueError("CgTable: float64 or float32 tensors")
        self.f64 = int(self.dtype == torch.float64)
        rows = []
        for s in self.segs:
            n = next(t.numel() for k, t in s.items() if t is not None and k != "slab")
            slab = s.get("slab")
            for k, t in s.items():
                if t is None:
                    continue
                if t.dtype != self.dtype or t.device != self.device or t.stride(-1) != 1:
                    raise ValueError("CgTable: one dtype, one device, element stride 1")
                if (k == "slab" and t.shape[-1] != n) or (k != "slab" and t.numel() != n):
                    raise ValueError("CgTable: every tensor of a segment has its n elements")
            s["n"] = n
            rows.append(tuple(_ptr(s.get(k)) for k in ("w", "w0", "g", "gprev", "d", "slab")) +
                        (slab.shape[0] if slab is not None else 0,
                         (slab.stride(0) if slab.shape[0] > 1 else n) if slab is not None else 0, n))
        self.dev = None
        if self.device.type != "cpu":
            self.dev = torch.zeros(len(rows), 9, dtype=torch.int64, device=self.device)
            rc = native().cg_table(self.f64, self.dev.data_ptr(), rows, _stream())
            if rc:
                raise ValueError(f"cg_table refused the segments (rc={rc})")
        self.rows = rows

    def __len__(self):
        return len(self.segs)


def _cg_rc(rc, what):
    if rc:
        raise RuntimeError(f"{what} failed (rc={rc})")


def cg_accumulate(table, first, scale=1.0):
    """g = ((0 if first else g) + slab[0] + slab[1] + ...) * scale per segment, in slab order
    (csrc/gpu/kernels_cg.hip); one capturable launch for the whole table.  CPU tensors: the host
    entry point of include/libhpnn/cg.h."""
    if table.dev is None:
        for r in table.rows:
            native().cg_host_accumulate(table.f64, r[2], r[5], r[6], r[7], r[8], int(bool(first)), float(scale))
        return
    _cg_rc(native().cg_accumulate(table.f64, table.dev.data_ptr(), len(table), int(bool(first)), float(scale),
                                  _stream()), "cg_accumulate")


def cg_dots(table, state, partials=None):
    """state.gg, gp, gd = <g,g>, <g,g_prev>, <g,d> over every segment: FP64 sums of FP64 products
    in a fixed order (bitwise reproducible); two capturable launches.  partials: [3 * 64] float64
    scratch (allocated when not given)."""
    if table.dev is None:
        out = torch.zeros(3, dtype=torch.float64)
        for r in table.rows:
            native().cg_host_dots(table.f64, r[2], r[3], r[4], r[8], out.data_ptr())
        state[0:3] = out
        return state
    if partials is None:
        partials = torch.zeros(3 * native().CG_DOT_WGS, dtype=torch.float64, device=table.device)
    _cg_rc(native().cg_dots(table.f64, table.dev.data_ptr(), len(table), partials.data_ptr(), state.data_ptr(),
                            _stream()), "cg_dots")
    return state


def cg_direction(state):
    """beta (Polak-Ribiere+, 0 on a restart), the restart flag and the six trial steps
    a_init 2^(j-2) from the state's dot products: one capturable one-thread launch"""
    if _cpu(state):
        native().cg_host_direction(state.data_ptr())
        return state
    _cg_rc(native().cg_direction(state.data_ptr(), _stream()), "cg_direction")
    return state


def cg_begin(table, state):
    """d = fma(beta, d, g) (beta = 0: d = g), g_prev = g, W0 = W per segment, beta read from the state"""
    if table.dev is None:
        beta = float(state[4])
        for r in table.rows:
            native().cg_host_begin(table.f64, r[0], r[1], r[2], r[3], r[4], r[8], beta)
        return
    _cg_rc(native().cg_begin(table.f64, table.dev.data_ptr(), len(table), state.data_ptr(), _stream()), "cg_begin")


def cg_trial(table, state, j):
    """W = fma(a[j], d, W0) per segment, one fma in the tensors' dtype, a[j] read from the state when
    the launch runs; a[j] = 0 gives W0 bit for bit.  j = 6: the parabola point, j = 7: the final step."""
    if not 0 <= int(j) <= CG_FINAL:
        raise ValueError(f"cg_trial: j = {j}")
    if table.dev is None:
        a = float(state[6 + int(j)])
        for r in table.rows:
            native().cg_host_trial(table.f64, r[0], r[1], r[4], r[8], a)
        return
    _cg_rc(native().cg_trial(table.f64, table.dev.data_ptr(), len(table), state.data_ptr(), int(j), _stream()),
           "cg_trial")


def cg_loss(Z, T, slots, net_type, n_valid=None):
    """the output layer forward only over the first n_valid rows of the logits Z [B, n_out]
    (float64 / float32; net_type TYPE_ANN / TYPE_LNN / TYPE_SNN): the loss sum (float64, floats
    2..3 of a slot) and the argmax hits (word 1) ADDED into the 64 stat slots [64, 16] float32,
    bitwise reproducible (64 workgroups, one writer per slot, no atomics).  Device tensors only."""
    if _cpu(Z):
        raise NotImplementedError("cg_loss: device tensors only (the CPU oracle is csrc/cpu/cpu_cg.cpp)")
    n_valid = Z.shape[0] if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= Z.shape[0] or T.shape[0] < n_valid or Z.dtype != T.dtype:
        raise ValueError("cg_loss: n_valid rows of Z and T, one dtype")
    _cg_rc(native().cg_loss(int(Z.dtype == torch.float64), Z.data_ptr(), Z.stride(0), T.data_ptr(), T.stride(0),
                            slots.data_ptr(), n_valid, Z.shape[1], int(net_type), _stream()), "cg_loss")
    return slots


def cg_file(slots, state, hist, j):
    """file the loss of trial j: the 64 stat slots summed in slot order (layout of validate_commit)
    and zeroed, phi[j] = sum / n (j = 7: f0 and its hits); behind j = 5 the choice of j* and of the
    seventh point, behind j = 6 the step a* and a record appended to hist (cg_history; may be
    None).  One capturable 64-lane launch; CPU tensors: the same rule through cg.h."""
    if not 0 <= int(j) <= CG_FINAL:
        raise ValueError(f"cg_file: j = {j}")
    if _cpu(slots):
        loss, hits = 0.0, 0
        dbl = slots[:, 2:4].contiguous().view(torch.float64).view(-1)
        word = slots[:, 1].contiguous().view(torch.int32)
        for i in range(slots.shape[0]):
            loss += float(slots[i, 0].double()) + float(dbl[i])
            hits += int(word[i]) & 0xffffffff
        slots[:, :4] = 0
        native().cg_host_file(state.data_ptr(), _ptr(hist), int(j), loss, hits & 0xffffffff)
        return state
    _cg_rc(native().cg_file(slots.data_ptr(), state.data_ptr(), _ptr(hist), int(j), _stream()), "cg_file")
    return state


WIDE2_K0 = (4096,)  # first-layer input widths of hpnn_wide2_front
WIDE2_TILE = 128  # samples per tile (the batch must be a multiple)


class Wide2Workspace:
    """exchange state of hpnn_wide2_front with two workgroups per tile: the FP32 partial
    buffer and the per-tile ticket counters (zeroed once, monotonic: two tickets per tile and
    launch; the flag words are unused) plus an error word (set if an exchange ever timed out)."""

    def __init__(self, Bp, K0, device, ksplit=None):
        if torch.device(device).type != "cuda":
            self.ksplit = 1
        else:
            self.ksplit = int(ksplit) if ksplit else native().wide2_ksplit(int(Bp), int(K0))
        n_tiles = Bp // WIDE2_TILE
        nb = native().wide2_pbuf_bytes(int(Bp)) if self.ksplit == 2 else 16
        self.pbuf = torch.empty(nb // 4, dtype=torch.float32, device=device)
        self.words = torch.zeros(2 * n_tiles + 4, dtype=torch.int32, device=device)
        self.cnt, self.flag = self.words[:n_tiles], self.words[n_tiles:2 * n_tiles]
        self.err = self.words[2 * n_tiles:2 * n_tiles + 1]

    def check(self):
        if int(self.err.item()) != 0:
            raise RuntimeError("wide2_front: a partial-sum hand-over timed out")


def wide2_front(X, W0, W1, W1t, H0, D2, D1, ws, n_out, net_type, labels=None, T=None, t_hi=1.0, t_lo=0.0,
                n_valid=None, loss_acc=None, correct=None):
    """The K0 (4096) -> 256 -> 256 step up to the deltas in one launch
    (csrc/gpu/kernels_wide.hip): X [Bp, K0] bf16 -> H0 = f(X W0^T), delta2 (output layer)
    and delta1 = (delta2 W1) f'(H0), all [Bp, 256] bf16, plus loss / hits.  ws: a
    Wide2Workspace.  CPU tensors: the same rounding points in PyTorch."""
    Bp, K0 = X.shape[0], W0.shape[1]
    n_valid = Bp if n_valid is None else int(n_valid)
    if _cpu(X):
        h = bipolar(X[:, :K0].float() @ W0.float().t()).bfloat16()
        H0.copy_(h)
        Z = h.float() @ W1.float().t()
        _cpu_output_delta(Z, n_out, net_type, D2, labels, T, t_hi, t_lo, n_valid, None, loss_acc, correct,
                          front=True)
        D1.copy_(((D2.float() @ W1.float()) * dbipolar(h.float())).bfloat16())
        return D1
    native().wide2_front(X.data_ptr(), X.stride(0), K0, W0.data_ptr(), W1.data_ptr(), W1t.data_ptr(), _ptr(labels),
                         _ptr(T), T.stride(0) if T is not None else 0, float(t_hi), float(t_lo), H0.data_ptr(),
                         D2.data_ptr(), D1.data_ptr(), ws.pbuf.data_ptr(), ws.cnt.data_ptr(), ws.flag.data_ptr(),
                         ws.err.data_ptr(), _ptr(loss_acc), _ptr(correct), Bp, n_valid, n_out, net_type, ws.ksplit,
                         _stream())
    return D1


def frag_major(W):
    """[N, K] -> flat MFMA-fragment-major copy (layout of hpnn_sgd_update_multi's Wf):
    element (n, k) at (((n//16)*(K//32) + k//32)*64 + n%16 + 16*((k//8)%4))*8 + k%8."""
    N, K = W.shape
    return W.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def reduce_groups(slab, groups, out):
    """out[g, :] = sum of slab rows [g*ceil(S/groups), ...) (first reduction pass)."""
    S = slab.shape[0]
    n = slab[0].numel()
    if _cpu(slab):
        sg = -(-S // groups)
        for g in range(groups):
            out[g].copy_(slab[g * sg:min(S, (g + 1) * sg)].reshape(-1, n).sum(0).view_as(out[g]))
        return out
    native().reduce_groups(slab.data_ptr(), S, slab.stride(0), n, groups, out.data_ptr(), _stream())
    return out


def sgd_update_multi(layers, lr, alpha=0.0, scale=1.0, momentum=False):
    """All layers' optimizer steps in one launch.  layers: list of
    (W32, V32, G, Wbf, Wt, Wf) with G [S, N, K] (or a strided view) or [N, K]; Wf may be None."""
    if _cpu(layers[0][0]):
        for W32, V32, G, Wbf, Wt, Wf in layers:
            sgd_update(W32, V32, G, Wbf, Wt, lr, alpha, scale, momentum)
            if Wf is not None:
                Wf.copy_(frag_major(W32.bfloat16()))
        return
    desc = []
    for W32, V32, G, Wbf, Wt, Wf in layers:
        N, K = W32.shape
        S = G.shape[0] if G.dim() == 3 else 1
        gstride = G.stride(0) if G.dim() == 3 else 0
        desc.append((W32.data_ptr(), _ptr(V32), G.data_ptr(), gstride, Wbf.data_ptr(), Wt.data_ptr(), _ptr(Wf), S,
                     N, K))
    native().sgd_update_multi(desc, float(lr), float(alpha), float(scale), int(momentum), _stream())


def sgd_update(W32, V32, G, Wbf, Wt, lr, alpha=0.0, scale=1.0, momentum=False):
    """W32[N,K] FP32 master; G: [S,N,K] or [N,K] FP32 gradient sum(s)."""
    N, K = W32.shape
    S = G.shape[0] if G.dim() == 3 else 1
    gstride = G.stride(0) if G.dim() == 3 else 0
    if _cpu(W32):
        g = (G.sum(0) if G.dim() == 3 else G) * scale
        if momentum:
            V32 += lr * g
            W32 += V32
            V32 *= alpha
        else:
            W32 += lr * g
        Wbf.copy_(W32.bfloat16())
        Wt.copy_(W32.bfloat16().t())
        return
    native().sgd_update(W32.data_ptr(), _ptr(V32), G.data_ptr(), S, gstride, Wbf.data_ptr(), Wt.data_ptr(), N, K,
                        float(lr), float(alpha), float(scale), int(momentum), _stream())


def cast_weights(W32, Wbf, Wt, Wf=None):
    N, K = W32.shape
    if _cpu(W32):
        Wbf.copy_(W32.bfloat16())
        Wt.copy_(W32.bfloat16().t())
        if Wf is not None:
            Wf.copy_(frag_major(Wbf))
        return
    if Wf is not None:  # an lr = 0 update is exactly a cast (same kernel writes Wf)
        sgd_update_multi([(W32, None, W32, Wbf, Wt, Wf)], 0.0, 0.0, 0.0, False)
        return
    native().cast_weights(W32.data_ptr(), Wbf.data_ptr(), Wt.data_ptr(), N, K, _stream())


def block_permute(src, dst):
    """dst [rows, P*n] <- src [P, rows, n] (BF16): rank-major all-gather output -> feature-
    concatenated activations (the tensor-parallel forward)."""
    Pn, rows, n = src.shape
    assert dst.shape == (rows, Pn * n) and src.is_contiguous() and dst.is_contiguous()
    if _cpu(src):
        dst.copy_(src.permute(1, 0, 2).reshape(rows, Pn * n))
        return dst
    native().block_permute_bf16(src.data_ptr(), dst.data_ptr(), Pn, rows, n, _stream())
    return dst


def dact_cast(out, x, H):
    """out (BF16) = bf16(x * f'(H)), x FP32 (the reduced partial deltas), H BF16 activations."""
    assert out.shape == x.shape == H.shape and out.is_contiguous() and x.is_contiguous() and H.is_contiguous()
    if _cpu(x):
        out.copy_((x * dbipolar(H.float())).bfloat16())
        return out
    native().dact_f32_bf16(out.data_ptr(), x.data_ptr(), H.data_ptr(), x.numel(), _stream())
    return out


def _misaligned(t, b):
    return t.data_ptr() % b != 0


def cast_f32_bf16(src, dst):
    """dst (BF16) = bf16(src) (FP32), flat contiguous tensors of n % 4 == 0 elements (the FP32
    gradient into the send buffer of the BF16 exchange).  Returns the launcher's code: 0, or -2
    (n, or a pointer not 16- / 8-byte aligned: nothing written)."""
    n = src.numel()
    assert dst.numel() == n and src.is_contiguous() and dst.is_contiguous()
    if _cpu(src):
        if n <= 0 or n % 4 or _misaligned(src, 16) or _misaligned(dst, 8):
            return -2
        dst.copy_(src.bfloat16())
        return 0
    return native().cast_f32_bf16(src.data_ptr(), dst.data_ptr(), n, _stream())


def sgd_update_rows_bf16g(W32, V32, G16, Wbf, lr, alpha=0.0, scale=1.0, momentum=False):
    """the step of sgd_update on n % 4 == 0 contiguous elements from their BF16 gradient sum
    G16: W32 / V32 FP32 masters, Wbf = bf16(W32) (a rank's rows in the sharded data-parallel
    step).  Returns the launcher's code: 0, or -2 (n, alignment, momentum without V32: nothing
    written)."""
    n = W32.numel()
    assert G16.numel() == n and Wbf.numel() == n and W32.is_contiguous() and G16.is_contiguous()
    if _cpu(W32):
        if n <= 0 or n % 4 or (momentum and V32 is None) or _misaligned(W32, 16) or \
                (momentum and _misaligned(V32, 16)) or _misaligned(G16, 8) or _misaligned(Wbf, 8):
            return -2
        g = G16.float() * scale
        if momentum:
            V32 += lr * g
            W32 += V32
            V32 *= alpha
        else:
            W32 += lr * g
        Wbf.copy_(W32.bfloat16())
        return 0
    return native().sgd_update_rows_bf16g(W32.data_ptr(), _ptr(V32) if momentum else 0, G16.data_ptr(), n, float(lr),
                                          float(alpha), float(scale), int(bool(momentum)), Wbf.data_ptr(), _stream())


def transpose_bf16(Wb, Wt):
    """Wt [K, N] = Wb^T for a contiguous BF16 [N, K] matrix, N % 32 == 0, K % 32 == 0."""
    N, K = Wb.shape
    assert Wt.shape == (K, N) and Wb.is_contiguous() and Wt.is_contiguous()
    if _cpu(Wb):
        if N % 32 or K % 32:
            raise RuntimeError("transpose_bf16 failed (rc=-2)")
        Wt.copy_(Wb.t())
        return Wt
    native().transpose_bf16(Wb.data_ptr(), Wt.data_ptr(), N, K, _stream())
    return Wt


_HASH_GOLD, _HASH_M1, _HASH_M2 = 0x9e3779b97f4a7c15, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53


def hash_words(t, out, base=0, nbytes=None):
    """out[0] (int64 [1]) += the order-independent digest of the first nbytes (default: all) of
    the contiguous tensor t: the wrapping 64-bit sum over its 4-byte words w_i of
    mix64((w_i << 32) ^ (i + base) ^ 0x9e3779b97f4a7c15), mix64 the murmur3 finalizer
    (csrc/gpu/kernels_misc.hip).  Returns the launcher's code: 0, or -1 (nbytes % 4)."""
    assert t.is_contiguous() and out.dtype == torch.int64 and out.numel() == 1
    nbytes = t.numel() * t.element_size() if nbytes is None else int(nbytes)
    if _cpu(t):
        import numpy as np
        if nbytes < 0 or nbytes % 4:
            return -1
        if nbytes == 0:
            return 0
        w = t.view(-1).view(torch.uint8)[:nbytes].numpy().view("<u4").astype(np.uint64)
        x = (w << np.uint64(32)) ^ (np.arange(w.size, dtype=np.uint64) + np.uint64(base)) ^ np.uint64(_HASH_GOLD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(_HASH_M1)
        x ^= x >> np.uint64(33)
        x *= np.uint64(_HASH_M2)
        x ^= x >> np.uint64(33)
        h = (int(np.add.reduce(x, dtype=np.uint64)) + int(out[0])) & 0xffffffffffffffff
        out[0] = h - (1 << 64) if h >> 63 else h
        return 0
    return native().hash_words(t.data_ptr(), nbytes, int(base), out.data_ptr(), _stream())


def pack_bf16(src, dst):
    """dst (bf16, padded) <- src (float32/float64 [rows, cols]); padding zero-filled."""
    rows, cols = src.shape
    if _cpu(dst):
        dst.zero_()
        dst[:rows, :cols] = src.float().bfloat16()
        return dst
    native().pack_bf16(src.data_ptr(), int(src.dtype == torch.float64), rows, cols, src.stride(0), dst.data_ptr(),
                       dst.shape[0], dst.shape[1], dst.stride(0), _stream())
    return dst


def epoch_perm(n, seed, epoch, device, out=None, err=None, advance=False):
    """int32 [n] permutation of epoch `epoch` ([shuffle] epoch, include/libhpnn/shuffle.h):
    out[i] = the sample at position i.  `epoch` is an int, or a 1-element int32 device tensor
    (the epoch word: read by the kernel, so a captured launch follows it); advance=True adds
    one to that word in a launch of its own behind the kernel.  err (1-element int32 tensor)
    is set when the bounded walk did not terminate; without it that raises."""
    device = torch.device(device)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=device)
    if device.type == "cpu":
        from .. import capi
        e = int(epoch.item()) if torch.is_tensor(epoch) else int(epoch)
        out.copy_(torch.from_numpy(capi.hpnn_epoch_perm(n, seed, e).astype("int32")))
        if advance and torch.is_tensor(epoch):
            epoch += 1
        return out
    word = epoch if torch.is_tensor(epoch) else torch.tensor([int(epoch) & 0xffffffff], dtype=torch.int64,
                                                              device=device).to(torch.int32)
    assert word.dtype == torch.int32 and word.numel() == 1 and out.dtype == torch.int32 and out.numel() >= n
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=device)
    native().epoch_perm(out.data_ptr(), n, int(seed) & 0xffffffff, word.data_ptr(), err.data_ptr(), _stream())
    if advance:
        native().epoch_advance(word.data_ptr(), _stream())
    if own_err and not torch.cuda.is_current_stream_capturing() and int(err.item()):
        raise RuntimeError("epoch_perm: the permutation walk did not terminate within its bound")
    return out


def gather_rows(src, perm, out, n=None):
    """row-major gather: out[i] = src[perm[i]] for i < n (default len(perm)), zero rows from n
    up.  Rows of any dtype whose byte size is a multiple of 4; src, out contiguous."""
    n = perm.numel() if n is None else int(n)
    rb = src[0].numel() * src.element_size()
    assert src.is_contiguous() and out.is_contiguous() and perm.dtype == torch.int32 and perm.is_contiguous()
    assert out.dtype == src.dtype and out[0].numel() == src[0].numel() and rb % 4 == 0
    assert n <= perm.numel() and n <= out.shape[0] and n <= src.shape[0]
    if _cpu(src):
        out.zero_()
        out[:n] = src[perm[:n].long()]
        return out
    native().gather_rows(out.data_ptr(), src.data_ptr(), perm.data_ptr(), n, out.shape[0], rb, _stream())
    return out


def gather_fragment_major(src, perm, out, n=None):
    """out = to_fragment_major(zero-padded src[perm[:n]]): src row-major [rows, Kp] uint8 or
    bfloat16 (Kp % 16 == 0), out fragment-major [rows_p/32, Kp/16, 64, 8] of the same dtype."""
    n = perm.numel() if n is None else int(n)
    Kp = src.shape[1]
    rows_p = out.numel() // Kp
    assert src.is_contiguous() and out.is_contiguous() and perm.dtype == torch.int32 and perm.is_contiguous()
    assert src.dtype in (torch.uint8, torch.bfloat16) and out.dtype == src.dtype
    assert Kp % 16 == 0 and rows_p % 32 == 0 and out.numel() == rows_p * Kp
    assert n <= perm.numel() and n <= rows_p and n <= src.shape[0]
    if _cpu(src):
        pad = torch.zeros(rows_p, Kp, dtype=src.dtype)
        pad[:n] = src[perm[:n].long()]
        out.view(-1).copy_(to_fragment_major(pad).reshape(-1))
        return out
    native().gather_fm(out.data_ptr(), src.data_ptr(), perm.data_ptr(), n, rows_p, Kp, src.element_size(), _stream())
    return out


# --------------------------------------------------------------------------- references
def bipolar(x):
    return 2.0 / (1.0 + torch.exp(-x)) - 1.0


def dbipolar(y):
    return -0.5 * (y * y - 1.0)


def ref_gemm_nt(A, B, epi=EPI_NONE, aux=None):
    C = A.float() @ B.float().t()
    if epi == EPI_ACT:
        C = bipolar(C)
    elif epi == EPI_DACT:
        C = C * dbipolar(aux.float())
    return C


def ref_gemm_tn(D, H):
    return D.float().t() @ H.float()


def ref_output(Z, n_out, net_type, T):
    """returns (O, delta, per-sample loss) in fp32 following the reference formulas."""
    z = Z[:, :n_out].float()
    if net_type == TYPE_SNN:
        m = z.max(dim=1, keepdim=True).values
        e = torch.exp(z - m)
        tiny = torch.exp(torch.clamp(torch.log(torch.tensor(1e-14)) + 1.0 - m, max=80.0))
        o = e / (e.sum(1, keepdim=True) + tiny)
        d = T - o
        loss = -(T * torch.log(o + 1e-14) * (o > 0)).sum(1) / n_out
    elif net_type == TYPE_ANN:
        o = bipolar(z)
        d = (T - o) * dbipolar(o)
        loss = 0.5 * ((T - o) ** 2).sum(1)
    else:
        o = z
        d = T - o
        loss = 0.5 * ((T - o) ** 2).sum(1)
    return o, d, loss


def _cpu_output_delta(Z, n_out, net_type, D, labels, T, t_hi, t_lo, n_valid, O, loss_acc, correct, front=False):
    """front: the hit rule of the fused fronts (csrc/gpu/mlp3_common.h, kernels_mlp3.hip,
    kernels_wide.hip): a row is a hit when the logit of its label -- dense targets: of its first
    largest target -- is >= the row's largest logit, so a tie counts.  Otherwise the rule of
    hpnn_output_delta: the argmax of the outputs is the argmax of the targets."""
    B = Z.shape[0]
    if T is None:
        T = torch.full((B, n_out), t_lo, dtype=torch.float32)
        T[torch.arange(B), labels.long()] = t_hi
    o, d, loss = ref_output(Z, n_out, net_type, T[:, :n_out].float())
    D.zero_()
    D[:n_valid, :n_out] = d[:n_valid].bfloat16()
    if O is not None:
        O[:, :n_out] = o
    if loss_acc is not None:
        loss_acc += loss[:n_valid].sum()
    if correct is not None and front:
        Tv, z = T[:n_valid, :n_out].float(), Z[:n_valid, :n_out].float()
        col = torch.arange(n_out).expand_as(Tv)
        tcol = torch.where(Tv == Tv.max(1, keepdim=True).values, col, torch.full_like(col, n_out)).min(1).values
        hits = (z.gather(1, tcol[:, None])[:, 0] >= z.max(1).values).sum().to(torch.int32)
        correct.view(torch.int32).add_(hits)
    elif correct is not None:
        hits = (o[:n_valid].argmax(1) == T[:n_valid, :n_out].argmax(1)).sum().to(torch.int32)
        correct.view(torch.int32).add_(hits)
    # (GPU kernels spread these over 64 slots of 16 floats; slot 0 is used here)
    return D


def _cpu_mlp3_mid(H1, W1, W1t, W2, W2t, D1, gslab, n_out, net_type, labels, T, t_hi, t_lo, n_valid, loss_acc,
                  correct):
    """PyTorch emulation with the kernel's rounding points (bf16 H2 / deltas)."""
    Bp = H1.shape[0]
    H2 = bipolar(H1.float() @ W1.float().t()).bfloat16()
    D1 = D1 if D1 is not None else torch.empty_like(H1)
    Z = (H2.float() @ W2.float().t())
    D3 = torch.zeros(Bp, W2.shape[0], dtype=torch.bfloat16)
    _cpu_output_delta(Z, n_out, net_type, D3, labels, T, t_hi, t_lo, n_valid, None, loss_acc, correct, front=True)
    D2 = ((D3.float() @ W2.float()) * dbipolar(H2.float())).bfloat16()
    D1.copy_(((D2.float() @ W1.float()) * dbipolar(H1.float())).bfloat16())
    G1 = D2.float().t() @ H1.float()
    G2 = D3.float().t() @ H2.float()
    gslab.zero_()
    gslab[0, :G1.numel()] = G1.reshape(-1)
    gslab[0, G1.numel():] = G2.reshape(-1)
    return D1


# --------------------------------------------------------------------------- [train] ADAM
_ADAM_D = ("lr", "beta1", "beta2", "eps", "decay", "t", "p1", "p2", "c1", "s2", "wd")  # words of hpnn_adam_state


def adam_state(lr=0.001, beta1=0.9, beta2=0.999, eps=1e-8, decay=0.0, device="cpu"):
    """a fresh hpnn_adam_state (include/libhpnn/adam.h) as [11] float64: lr, beta1, beta2, eps,
    decay, t (a uint64 word, 0), p1 = p2 = 1, then c1, s2, wd as the last advance derived them"""
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0 and eps > 0.0 and decay >= 0.0):
        raise ValueError("adam_state: 0 <= beta < 1, eps > 0, decay >= 0")
    st = torch.zeros(11, dtype=torch.float64)
    native().adam_host_init(st.data_ptr(), float(lr), float(beta1), float(beta2), float(eps), float(decay))
    return st.to(device)


def read_adam_state(state):
    """the Adam state as a dict (synchronises); t is an int"""
    s = state.cpu()
    out = {k: float(s[i]) for i, k in enumerate(_ADAM_D)}
    out["t"] = int(s[5:6].view(torch.int64)[0])
    return out


def write_adam_state(state, **kw):
    """set fields of an Adam state (names of read_adam_state); returns the state"""
    s = state.cpu().clone()
    for k, v in kw.items():
        if k == "t":
            s[5:6].view(torch.int64)[0] = int(v)
        else:
            s[_ADAM_D.index(k)] = float(v)
    state.copy_(s)
    return state


def adam_advance(state):
    """t += 1, p1 *= beta1, p2 *= beta2, then c1 = lr / (1 - p1), s2 = sqrt(1 - p2), wd = lr decay:
    one capturable one-thread launch (csrc/gpu/kernels_adam.hip); CPU tensors: the host form"""
    if _cpu(state):
        native().adam_host_advance(state.data_ptr())
        return state
    _cg_rc(native().adam_advance(state.data_ptr(), _stream()), "adam_advance")
    return state


class _SegTable:
    """a segment table of the update kernels (csrc/gpu/upd_common.h): one segment per layer, a dict
    of flat (element stride 1) tensors w and the state arrays `keys` of one dtype (float64 /
    float32) with n elements each and slab: [S, n] with any row stride >= n.  At most 16 segments.
    A row is (w, the state pointers, slab, S, slab row stride, n); a state array outside `_used()`
    is not looked at and its pointer is 0.  Device tensors: uploaded once by the native `entry` (a
    [n, width] int64 device tensor; the table keeps the tensors alive)."""

    name, keys, width, entry = None, (), 0, None

    def _used(self):
        """the state arrays this table's launches use"""
        return self.keys

    def _extra(self):
        """what the native `entry` takes between the rows and the stream"""
        return ()

    def __init__(self, segs):
        name, used = self.name, self._used()
        self.segs = [dict(s) for s in segs]
        if not 1 <= len(self.segs) <= 16:
            raise ValueError(f"{name}: 1..16 segments")
        w0 = self.segs[0]["w"]
        self.dtype, self.device = w0.dtype, w0.device
        if self.dtype not in (torch.float64, torch.float32):
            raise ValueError(f"{name}: float64 or float32 tensors")
        self.f64 = int(self.dtype == torch.float64)
        rows = []
        for s in self.segs:
            n, slab = s["w"].numel(), s["slab"]
            for k in ("w",) + used + ("slab",):
                t = s[k]
                if t.dtype != self.dtype or t.device != self.device or t.stride(-1) != 1:
                    raise ValueError(f"{name}: one dtype, one device, element stride 1")
                if (k == "slab" and (t.dim() != 2 or t.shape[1] != n)) or (k != "slab" and t.numel() != n):
                    raise ValueError(f"{name}: every tensor of a segment has its n elements")
            if n == 0 or slab.shape[0] < 1 or (slab.shape[0] > 1 and slab.stride(0) < n):
                raise ValueError(f"{name}: n >= 1, S >= 1, slab row stride >= n")
            rows.append((_ptr(s["w"]),) + tuple(_ptr(s.get(k)) if k in used else 0 for k in self.keys) +
                        (_ptr(slab), slab.shape[0], slab.stride(0) if slab.shape[0] > 1 else n, n))
        self.dev = None
        if self.device.type != "cpu":
            self.dev = torch.zeros(len(rows), self.width, dtype=torch.int64, device=self.device)
            rc = getattr(native(), self.entry)(self.f64, self.dev.data_ptr(), rows, *self._extra(), _stream())
            if rc:
                raise ValueError(f"{self.entry} refused the segments (rc={rc})")
        self.rows = rows

    def __len__(self):
        return len(self.segs)


class AdamTable(_SegTable):
    """the segment table of adam_update_fp: per segment w, m, v and slab; on a device a [n, 8]
    int64 tensor"""

    name, keys, width, entry = "AdamTable", ("m", "v"), 8, "adam_table"


def adam_update_fp(table, state, scale=1.0, clip=None):
    """per segment g = (slab[0] + ... + slab[S-1]) * scale in slab order, then the Adam rule of
    include/libhpnn/adam.h on w, m, v in the tensors' dtype with the coefficients the last
    adam_advance left in the state, read when the launch runs: one capturable launch for the whole
    table (csrc/gpu/kernels_adam.hip).  clip: a clip state (clip_state) -- the rule then sees
    g * factor, the factor of the last clip_finalize read when the launch runs.  CPU tensors: the
    host entry point."""
    if table.dev is None:
        for r in table.rows:
            native().adam_host_update_clip(table.f64, r[0], r[1], r[2], r[3], r[4], r[5], r[6], float(scale),
                                           state.data_ptr(), _ptr(clip))
        return
    _cg_rc(native().adam_fp_clip(table.f64, table.dev.data_ptr(), len(table), float(scale), state.data_ptr(),
                                 _ptr(clip), _stream()), "adam_update_fp")


def adam_slab_sum(G):
    """the slab sum of adam_update_multi in the kernel's one fixed order (csrc/gpu/upd_common.h):
    p_w = the slabs w, w + 8, ... added in that order to 0, then ((p_0 + p_1) + ...) + p_7; FP32"""
    if G.dim() == 2:
        G = G.unsqueeze(0)
    parts = []
    for w in range(8):
        p = torch.zeros_like(G[0])
        for s in range(w, G.shape[0], 8):
            p = p + G[s]
        parts.append(p)
    g = parts[0]
    for w in range(1, 8):
        g = g + parts[w]
    return g


def adam_update_multi(layers, state, scale=1.0, clip=None):
    """All layers' Adam steps in one launch (the BF16 plan's update, csrc/gpu/kernels_adam.hip).
    layers: list of (W32, V32, A32, G, Wbf, Wt, Wf) with the FP32 masters W32, first moment V32 and
    second moment A32 [N, K], G [S, N, K] (or a strided view) or [N, K]; Wf may be None.  The
    coefficients are those the last adam_advance left in the state, read when the launch runs.
    clip: a clip state -- the rule sees g * factor.  CPU tensors: the slabs summed in the kernel's
    order, then the host entry point of include/libhpnn/adam.h and the BF16 copies of the
    emulation."""
    if _cpu(layers[0][0]):
        for W32, V32, A32, G, Wbf, Wt, Wf in layers:
            g = adam_slab_sum(G.float()).contiguous()
            if not (W32.is_contiguous() and V32.is_contiguous() and A32.is_contiguous()):
                raise ValueError("adam_update_multi: contiguous W32, V32, A32")
            native().adam_host_update_clip(0, W32.data_ptr(), V32.data_ptr(), A32.data_ptr(), g.data_ptr(), 1, 0,
                                           W32.numel(), float(scale), state.data_ptr(), _ptr(clip))
            cast_weights(W32, Wbf, Wt, Wf)
        return
    desc = []
    for W32, V32, A32, G, Wbf, Wt, Wf in layers:
        N, K = W32.shape
        S = G.shape[0] if G.dim() == 3 else 1
        gstride = G.stride(0) if G.dim() == 3 else 0
        desc.append((W32.data_ptr(), V32.data_ptr(), A32.data_ptr(), G.data_ptr(), gstride, Wbf.data_ptr(),
                     Wt.data_ptr(), _ptr(Wf), S, N, K))
    native().adam_update_multi(desc, float(scale), state.data_ptr(), _stream(), _ptr(clip))


# --------------------------------------------------------------------------- [lr_schedule]
LR_KIND = {"constant": 0, "step": 1, "linear": 2, "plateau": 3}  # HPNN_LR_* (= nn_lr_schedule)
_LR_D = ("lr0", "gamma", "lr_end", "lr_min", "scale", "best", "lr")  # float64 words 0..6 of hpnn_lr_state
_LR_U = ("kind", "period", "span", "patience", "warmup", "epoch", "stale", "cuts", "valid")  # uint32 words 14..22


def lr_state(kind="constant", lr0=0.01, gamma=0.5, period=10, span=0, lr_end=0.0, lr_min=0.0, patience=2, warmup=0,
             epoch=0, device="cpu"):
    """a fresh hpnn_lr_state (include/libhpnn/lrsched.h) as [12] float64 (96 bytes): lr0, gamma,
    lr_end, lr_min, scale (1), best, lr, then the uint32 words kind, period, span, patience, warmup,
    epoch (the absolute 0-based index of the next epoch), stale, cuts, valid, pad.  Raises when
    hpnn_lr_valid refuses the keys."""
    k = LR_KIND[kind] if isinstance(kind, str) else int(kind)
    st = torch.zeros(12, dtype=torch.float64)
    ok = native().lr_host_init(st.data_ptr(), k, float(lr0), float(gamma), int(period), int(span), float(lr_end),
                               float(lr_min), int(patience), int(warmup), int(epoch))
    if not ok:
        raise ValueError("lr_state: lr0 and lr_end finite, 0 < gamma <= 1, period >= 1, lr_min >= 0, span >= 1 for "
                         "linear, patience >= 1 for plateau")
    return st.to(device)


def lr_valid(state):
    """hpnn_lr_valid on a state (synchronises)"""
    return bool(native().lr_host_valid(state.cpu().contiguous().data_ptr()))


def read_lr_state(state):
    """the schedule state as a dict (synchronises); the counters are ints"""
    s = state.cpu().contiguous()
    out = {k: float(s[i]) for i, k in enumerate(_LR_D)}
    u = s.view(torch.int32)
    out.update({k: int(u[14 + i]) & 0xffffffff for i, k in enumerate(_LR_U)})
    return out


def write_lr_state(state, **kw):
    """set fields of a schedule state (names of read_lr_state); returns the state"""
    s = state.cpu().clone()
    u = s.view(torch.int32)
    for k, v in kw.items():
        if k in _LR_U:
            v = int(v) & 0xffffffff
            u[14 + _LR_U.index(k)] = v - (1 << 32) if v >= 1 << 31 else v
        else:
            s[_LR_D.index(k)] = float(v)
    state.copy_(s)
    return state


def lr_advance(state, adam=None, hist=None, cursor=None):
    """the first launch of an epoch: hpnn_lr_advance on the state -- the rate of epoch `epoch` into
    lr, epoch += 1 -- then, when given, lr appended to hist ([cap] float64) at cursor ([1] int32; a
    full history drops the record) and stored into the lr word of an Adam state.  One capturable
    one-thread launch (csrc/gpu/kernels_lrsched.hip); CPU tensors: the host form."""
    if (hist is None) != (cursor is None):
        raise ValueError("lr_advance: hist and cursor come together")
    if _cpu(state):
        native().lr_host_advance(state.data_ptr())
        if adam is not None:
            adam[0] = state[6]
        if hist is not None:
            c = int(cursor[0])
            if c < hist.shape[0]:
                hist[c] = state[6]
                cursor[0] = c + 1
        return state
    _cg_rc(native().lr_advance(state.data_ptr(), _ptr(adam), _ptr(hist), _ptr(cursor),
                               hist.shape[0] if hist is not None else 0, _stream()), "lr_advance")
    return state


def lr_plateau(vhist, vcursor, state):
    """behind validate_commit: hpnn_lr_plateau on the loss sum of the pass just filed
    (vhist[vcursor - 1]; vcursor == 0: a no-op).  A loss that is not a NaN and < best sets best and
    zeroes stale, anything else adds one; stale == patience: scale *= gamma, stale = 0, cuts += 1.
    One capturable one-thread launch; CPU tensors: the host form."""
    if _cpu(state):
        c = int(vcursor[0])
        if c:
            native().lr_host_plateau(state.data_ptr(), float(vhist[c - 1, 0]))
        return state
    _cg_rc(native().lr_plateau(vhist.data_ptr(), vcursor.data_ptr(), state.data_ptr(), _stream()), "lr_plateau")
    return state


class SgdSchedTable(_SegTable):
    """the segment table of sgd_sched_fp: per segment w, (BPM) v and slab; on a device a [n, 7]
    int64 tensor"""

    name, keys, width, entry = "SgdSchedTable", ("v",), 7, "sgd_sched_table"

    def __init__(self, segs, momentum=False):
        self.momentum = bool(momentum)
        super().__init__(segs)

    def _used(self):
        return self.keys if self.momentum else ()

    def _extra(self):
        return (int(self.momentum),)


def sgd_sched_fp(table, state, scale=1.0, alpha=0.0, clip=None):
    """per segment g = (slab[0] + ... + slab[S-1]) * scale in slab order, then the scheduled BP
    (w += lr g) or BPM (v += lr g; w += v; v *= alpha) step of include/libhpnn/lrsched.h in the
    tensors' dtype with lr = the state's rate, read when the launch runs: one capturable launch for
    the whole table (csrc/gpu/kernels_lrsched.hip).  clip: a clip state (clip_state) -- the rule
    then sees g * factor, the factor of the last clip_finalize read when the launch runs.  CPU
    tensors: the host entry point."""
    if table.dev is None:
        for r in table.rows:
            native().sgd_sched_host_update_clip(table.f64, r[0], r[1], r[2], r[3], r[4], r[5], float(scale),
                                                float(alpha), int(table.momentum), state.data_ptr(), _ptr(clip))
        return
    _cg_rc(native().sgd_sched_fp_clip(table.f64, table.dev.data_ptr(), len(table), float(scale), float(alpha),
                                      int(table.momentum), state.data_ptr(), _ptr(clip), _stream()), "sgd_sched_fp")


def sgd_sched_multi(layers, state, alpha=0.0, scale=1.0, momentum=False, clip=None):
    """All layers' BP / BPM steps in one launch with the rate read from the schedule state (the
    BF16 plan's scheduled update, csrc/gpu/kernels_lrsched.hip).  layers: list of (W32, V32, G, Wbf,
    Wt, Wf) with the FP32 masters W32 and momentum V32 [N, K] (V32 may be None under BP), G [S, N,
    K] (or a strided view) or [N, K]; Wf may be None.  More than 8 layers go in groups of 8.  The
    slabs are summed in the order of adam_slab_sum.  clip: a clip state -- the rule sees
    g * factor.  CPU tensors: that sum, then the host entry point of include/libhpnn/lrsched.h and
    the BF16 copies of the emulation."""
    if _cpu(layers[0][0]):
        for W32, V32, G, Wbf, Wt, Wf in layers:
            g = adam_slab_sum(G.float()).contiguous()
            if not (W32.is_contiguous() and (V32 is None or V32.is_contiguous())):
                raise ValueError("sgd_sched_multi: contiguous W32, V32")
            native().sgd_sched_host_update_clip(0, W32.data_ptr(), _ptr(V32), g.data_ptr(), 1, 0, W32.numel(),
                                                float(scale), float(alpha), int(bool(momentum)), state.data_ptr(),
                                                _ptr(clip))
            cast_weights(W32, Wbf, Wt, Wf)
        return
    desc = []
    for W32, V32, G, Wbf, Wt, Wf in layers:
        N, K = W32.shape
        S = G.shape[0] if G.dim() == 3 else 1
        gstride = G.stride(0) if G.dim() == 3 else 0
        desc.append((W32.data_ptr(), _ptr(V32), G.data_ptr(), gstride, Wbf.data_ptr(), Wt.data_ptr(), _ptr(Wf), S,
                     N, K))
    native().sgd_sched_multi(desc, float(alpha), float(scale), int(bool(momentum)), state.data_ptr(), _stream(),
                             _ptr(clip))


# --------------------------------------------------------------------------- [clip]
_CLIP_D = ("max_norm", "sumsq", "norm", "factor", "norm_max", "norm_last")  # float64 words 0..5 of hpnn_clip_state
_CLIP_U = ("steps", "clipped")  # uint32 words 12..13
CLIP_BLOCK = 1024  # elements of one partial (HPNN_CLIP_BLOCK)


def clip_state(max_norm, device="cpu"):
    """a fresh hpnn_clip_state (include/libhpnn/clip.h) as [8] float64 (64 bytes): max_norm, sumsq,
    norm, factor (1), norm_max, norm_last, then the uint32 words steps, clipped and two of padding.
    Raises unless max_norm is finite and >= 0."""
    st = torch.zeros(8, dtype=torch.float64)
    if not native().clip_host_init(st.data_ptr(), float(max_norm)):
        raise ValueError("clip_state: a finite max_norm >= 0")
    return st.to(device)


def read_clip_state(state):
    """the clip state as a dict (synchronises); the counters are ints"""
    s = state.cpu().contiguous()
    out = {k: float(s[i]) for i, k in enumerate(_CLIP_D)}
    u = s.view(torch.int32)
    out.update({k: int(u[12 + i]) & 0xffffffff for i, k in enumerate(_CLIP_U)})
    return out


def write_clip_state(state, **kw):
    """set fields of a clip state (names of read_clip_state); returns the state"""
    s = state.cpu().clone()
    u = s.view(torch.int32)
    for k, v in kw.items():
        if k in _CLIP_U:
            v = int(v) & 0xffffffff
            u[12 + _CLIP_U.index(k)] = v - (1 << 32) if v >= 1 << 31 else v
        else:
            s[_CLIP_D.index(k)] = float(v)
    state.copy_(s)
    return state


def clip_history(cap, device="cpu"):
    """an empty epoch history for clip_commit: (hist [cap, 3] float64 -- per record the uint32 words
    steps, clipped, then norm_max, norm_last -- and cursor [1] int32)"""
    return torch.zeros(cap, 3, dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.int32, device=device)


def read_clip_history(hist, cursor):
    """the records filed so far as dicts (synchronises)"""
    h, c = hist.cpu().contiguous(), int(cursor.cpu()[0])
    u = h.view(torch.int32).reshape(-1, 6)
    return [{"steps": int(u[i, 0]) & 0xffffffff, "clipped": int(u[i, 1]) & 0xffffffff, "norm_max": float(h[i, 1]),
             "norm_last": float(h[i, 2])} for i in range(c)]


class GnormTable:
    """the segment table of gnorm_partials (csrc/gpu/kernels_clip.hip): one segment per layer, each
    a slab tensor [S, n] (element stride 1, any row stride >= n) or [n], float64 or float32, all of
    one dtype and device; at most 16.  `interleaved` selects the slab order: False the FP64 / FP32
    engines' (slabs 0 .. S-1 in order), True the BF16 plan's 8-way order (adam_slab_sum).  Segment
    y owns the entries [first[y], first[y] + ceil(n / 1024)) of the partials; `count` is their
    total.  Device tensors: uploaded once (a [n, 4] int64 device tensor; the table keeps the slabs
    alive)."""

    def __init__(self, slabs, interleaved=False):
        self.slabs = [s if s.dim() == 2 else s.unsqueeze(0) for s in slabs]
        if not 1 <= len(self.slabs) <= 16:
            raise ValueError("GnormTable: 1..16 segments")
        s0 = self.slabs[0]
        self.dtype, self.device, self.interleaved = s0.dtype, s0.device, bool(interleaved)
        if self.dtype not in (torch.float64, torch.float32):
            raise ValueError("GnormTable: float64 or float32 tensors")
        self.f64 = int(self.dtype == torch.float64)
        self.rows, self.first, count = [], [], 0
        for s in self.slabs:
            if s.dtype != self.dtype or s.device != self.device or s.dim() != 2 or s.stride(-1) != 1:
                raise ValueError("GnormTable: one dtype, one device, [S, n] with element stride 1")
            S, n = s.shape
            if n == 0 or S < 1 or (S > 1 and s.stride(0) < n):
                raise ValueError("GnormTable: n >= 1, S >= 1, slab row stride >= n")
            self.rows.append((_ptr(s), S, s.stride(0) if S > 1 else n, n))
            self.first.append(count)
            count += (n + CLIP_BLOCK - 1) // CLIP_BLOCK
        self.count, self.dev = count, None
        if self.device.type != "cpu":
            self.dev = torch.zeros(len(self.rows), 4, dtype=torch.int64, device=self.device)
            rc, dev_count = native().gnorm_table(self.f64, self.dev.data_ptr(), self.rows, _stream())
            if rc or dev_count != count:
                raise ValueError(f"gnorm_table refused the segments (rc={rc})")

    def __len__(self):
        return len(self.slabs)


def gnorm_partials(table, partials, scale=1.0):
    """per block of 1024 elements of every segment the sum of gs^2 in FP64, gs = (the slab sum in
    the table's order) * scale in the tensors' dtype, in the fixed order of include/libhpnn/clip.h,
    into partials[0 .. table.count) (float64; the rest is left alone): one capturable launch with
    one workgroup per block (csrc/gpu/kernels_clip.hip).  CPU tensors: the host entry point."""
    if partials.dtype != torch.float64 or partials.dim() != 1 or partials.stride(0) != 1 or \
            partials.numel() < table.count or partials.device != table.device:
        raise ValueError("gnorm_partials: partials is float64 [>= table.count] on the table's device")
    if table.dev is None:
        for r, first in zip(table.rows, table.first):
            native().clip_host_sumsq(table.f64, int(table.interleaved), r[0], r[1], r[2], r[3], float(scale),
                                     partials.data_ptr() + 8 * first)
        return partials
    _cg_rc(native().gnorm_partials(table.f64, int(table.interleaved), table.dev.data_ptr(), len(table), table.count,
                                   float(scale), partials.data_ptr(), _stream()), "gnorm_partials")
    return partials


def clip_finalize(partials, count, state):
    """partials[0 .. count) summed in the finalize's order, norm = sqrt(sum), factor = max_norm /
    norm when norm > max_norm, else 1, and the epoch's counters (steps, clipped, norm_max,
    norm_last): one capturable launch of one workgroup; CPU tensors: the host form."""
    if not 1 <= count <= partials.numel():
        raise ValueError("clip_finalize: 1 <= count <= len(partials)")
    if _cpu(state):
        native().clip_host_finalize(state.data_ptr(), partials.data_ptr(), int(count))
        return state
    _cg_rc(native().clip_finalize(partials.data_ptr(), int(count), state.data_ptr(), _stream()), "clip_finalize")
    return state


def clip_commit(state, hist=None, cursor=None):
    """the last launch of an epoch: the record (steps, clipped, norm_max, norm_last) appended to hist
    at cursor (clip_history; a full history drops the record), then the four zeroed.  One capturable
    one-thread launch; CPU tensors: the host form."""
    if (hist is None) != (cursor is None):
        raise ValueError("clip_commit: hist and cursor come together")
    cap = hist.shape[0] if hist is not None else 0
    if _cpu(state):
        native().clip_host_commit(state.data_ptr(), _ptr(hist), _ptr(cursor), cap)
        return state
    _cg_rc(native().clip_commit(state.data_ptr(), _ptr(hist), _ptr(cursor), cap, _stream()), "clip_commit")
    return state


# --------------------------------------------------------------------------- online FP64 engine
ONLINE_VARIANTS = ("lds", "global", "coop")


def online_sizes(W):
    """[n_in, N_0, ..] of a list of [N, M] weight tensors"""
    return [int(W[0].shape[1])] + [int(w.shape[0]) for w in W]


def online_coop_grid(sizes):
    """the grid the engine gives the cooperative online kernel for this net (0: single workgroup)"""
    return native().online_coop_grid([int(s) for s in sizes])


def online_sample(W, dW, x, t, net_type, variant="lds", momentum=False, lr=0.0, alpha=0.0, delta=1e-6, min_iter=0,
                  max_iter=0, forward_only=False, grid=None, check=True):
    """One sample through ONE launch of an online kernel of csrc/gpu/online.hip: the reference's
    "iterate this sample until it converges" loop on the device.  W / dW: lists of FP64 device
    tensors [N, M], updated in place (dW: the momenta of BPM; read and written only when momentum).
    variant: "lds" / "global" (the single-workgroup kernel with its vectors in LDS / in global
    scratch) or "coop" (the cooperative kernel on `grid` workgroups; None: the engine's choice).
    Launches on the current stream and synchronises.  Returns (out, dEp, init_err, iters, ok,
    first_ok); forward_only: (out, None, init_err, None, None, None).  check=False returns the
    launcher's code instead of raising when it refuses (then nothing was launched)."""
    n = native()
    sizes = online_sizes(W)
    dev = x.device
    for a, b, m in zip(W, dW, sizes):
        if not (a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.float64 and a.is_contiguous()
                and b.is_contiguous() and a.shape == b.shape and a.shape[1] == m):
            raise ValueError("online_sample: W / dW are contiguous FP64 device tensors [N, M], chained")
    if not (x.dtype == t.dtype == torch.float64 and x.numel() == sizes[0] and t.numel() == sizes[-1]):
        raise ValueError("online_sample: x [n_in], t [n_out] FP64")
    if variant not in ONLINE_VARIANTS:
        raise ValueError("online_sample: variant is one of %s" % (ONLINE_VARIANTS,))
    x, t = x.contiguous(), t.contiguous()
    out = torch.zeros(sizes[-1], dtype=torch.float64, device=dev)
    result = torch.zeros(8, dtype=torch.float64, device=dev)
    fits = len(W) <= 16
    scratch = torch.zeros(max(n.online_vec_bytes(sizes) // 8, 1) if fits else 1, dtype=torch.float64, device=dev)
    xch = ctl = None
    if variant == "coop":
        if grid is None:
            grid = n.online_coop_grid(sizes)
        xb = n.online_coop_xch_bytes(sizes, max(int(grid), 1)) if fits else 8
        xch = torch.zeros(max(xb // 8, 1), dtype=torch.float64, device=dev)
        ctl = torch.zeros(n.ONLINE_CTL_BYTES // 4, dtype=torch.int32, device=dev)
    rc = n.online_sample(sizes, [w.data_ptr() for w in W], [v.data_ptr() for v in dW], x.data_ptr(), t.data_ptr(),
                         out.data_ptr(), result.data_ptr(), scratch.data_ptr(), int(net_type), int(bool(momentum)),
                         float(lr), float(alpha), float(delta), int(min_iter), int(max_iter), int(bool(forward_only)),
                         variant, int(grid or 0), _ptr(xch), _ptr(ctl), 1, _stream())
    torch.cuda.current_stream().synchronize()
    if rc != 0:
        if check:
            raise RuntimeError("online_sample: the %s launcher refused (rc=%d)" % (variant, rc))
        return rc
    if variant == "coop" and n.online_coop_status(ctl.data_ptr()) != 0:
        raise RuntimeError("online_sample: a grid barrier of the cooperative kernel timed out")
    r = result.cpu()
    if forward_only:
        return out, None, float(r[1]), None, None, None
    return out, float(r[0]), float(r[1]), int(r[2]), int(r[3]), int(r[4])
