"""Cases, exact references and check functions for the 8-phase TN update kernels
(csrc/gpu/kernels_8ph.hip, gemm_tn8_kernel MODE 1 / 2 / 2 + side / 3), shared by test_tn8_gpu.py
(which runs them on the kernels) and test_tn8_cpu.py (which runs them on CPU tensors through the
emulations of hpnn_amd.ops, so the references, the guards and the exactness claim are themselves
checked where there is no GPU).

The oracle: with small-integer operands and power-of-two step parameters every product, partial
sum, total and step of the FP32 kernel is exact, so its result does not depend on the summation
order, on fma contraction or on how the splits are reduced, and the float64 reference is the
answer bit for bit.  exact() asserts that claim on every intermediate of the reference.

Shapes are written (N, M, Bt): the gradient is N x M over Bt batch rows, D [Bt, N], H [Bt, M]."""
import torch

from hpnn_amd import ops

# ---------------------------------------------------------------------------- the recipe
LR, SCALE, ALPHA = 2.0 ** -3, 2.0 ** -10, 0.5
BT_MAX = 24576  # |g| <= 9 Bt = 221184 < 2^24
LAUNCHES = 3

# ---------------------------------------------------------------------------- the cases
MODE1_SHAPES = [(256, 256, 128), (512, 256, 384), (256, 768, 256), (768, 768, 256), (512, 1280, 128)]
MODE1_PADDED = [MODE1_SHAPES[0], MODE1_SHAPES[-1]]  # again with ldd = N + 32, ldh = M + 64
MODE3_CASES = [(256, 256, 128, 256), (512, 768, 640, 768 + 64), (768, 512, 256, 512)]  # (N, M, Bt, ldg)
# (N, M, Bt, ldd, ldh) that hpnn_gemm_tn8_bf16out refuses
MODE3_REFUSED = [(288, 256, 128, 288, 256), (256, 256, 192, 256, 256), (256, 256, 128, 256 + 4, 256)]
CUS = 256  # the MODE 2 cases are laid out for 256 CUs, one resident workgroup each
# (N, M, splits, Bt)
MODE2_CASES = [(256, 256, 128, 16384), (256, 256, 192, 24576), (512, 1024, 20, 2560), (1024, 1024, 9, 1152),
               (1024, 1024, 16, 4096), (2048, 1024, 5, 640), (1024, 2048, 7, 896)]
# refused with -1: one split; above the capacity; below the minimum grid; units / splits odd; 33 tiles
MODE2_REFUSED = [(256, 256, 1, 128), (2048, 1024, 9, 1152), (256, 256, 2, 256), (1024, 1024, 16, 1024),
                 (256, 33 * 256, 4, 512)]
# (main case, N1, M1, S, fits)
SIDE_CASES = [(MODE2_CASES[0], 128, 64, 128, True), (MODE2_CASES[2], 128, 256, 40, True),
              (MODE2_CASES[4], 256, 256, 32, True), (MODE2_CASES[3], 256, 256, 18, True),
              (MODE2_CASES[3], 256, 256, 9, False)]
TM128_CASES = [MODE2_CASES[0], MODE2_CASES[4]]


# ---------------------------------------------------------------------------- shape arithmetic
def _strides_ok(ldd, ldh):
    return ldd % 8 == 0 and ldh % 8 == 0 and ldd * 2 * 64 < 2 ** 31 and ldh * 2 * 64 < 2 ** 31


def mode1_ok(N, M, Bt, ldd, ldh):
    """the shape rule of hpnn_gemm_tn8_update"""
    return N % 256 == 0 and M % 256 == 0 and Bt % 128 == 0 and _strides_ok(ldd, ldh)


def mode3_ok(N, M, Bt, ldd, ldh):
    """the shape rule of hpnn_gemm_tn8_bf16out_ok"""
    return mode1_ok(N, M, Bt, ldd, ldh) and (Bt // 64) % 2 == 0


def mode2_plan(N, M, Bt, splits, ldd=None, ldh=None, tm128=False, cus=CUS):
    """what hpnn_gemm_tn8_fused_update launches: (tile width, tiles, splits after the TM = 128
    halving), or None where it returns -1.  The capacity is one workgroup per CU (the kernel's
    LDS is 160 KiB), the minimum grid half the CUs."""
    if splits < 2 or not mode1_ok(N, M, Bt, ldd or N, ldh or M):
        return None
    units = Bt // 64
    if units % splits or (units // splits) % 2:
        return None
    tm = 256
    if tm128 and splits % 2 == 0 and (units // (splits // 2)) % 2 == 0:
        tm, splits = 128, splits // 2
    ntiles = (N // 256) * (M // tm)
    if ntiles > 32 or ntiles * splits > cus or ntiles * splits < cus // 2:
        return None
    return tm, ntiles, splits


def side_fits(G, Bt, N1, M1, S):
    """whether the side job splits evenly over the 2 G half-workgroups of a grid of G"""
    if N1 % 64 or M1 % 64 or S < 1 or (Bt // 64) % S:
        return False
    return G % 8 == 0 and ((N1 // 64) * (M1 // 64) * S) % (2 * G) == 0


# ---------------------------------------------------------------------------- guarded buffers
SENT16 = 0x7fc1  # BF16 sentinel bit pattern (a NaN no kernel here produces)
SENT32 = 0x7fc00000  # FP32 sentinel: the quiet NaN
PAD = 256  # guard elements on either side (keeps the inner buffer 16-byte aligned)


class Guarded:
    """n elements of float32 / bfloat16 inside a larger sentinel-filled tensor.  `t` is the inner
    flat view (offset: its start moved by that many elements, for the misaligned cases)."""

    def __init__(self, n, dtype, device, offset=0):
        assert dtype in (torch.float32, torch.bfloat16)
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        self.sent = SENT32 if dtype == torch.float32 else SENT16
        self.raw = torch.full((n + 2 * PAD,), self.sent, dtype=self.bits, device=device)
        self.buf = self.raw.view(dtype)
        self.lo, self.hi = PAD + offset, PAD + offset + n
        self.t = self.buf[self.lo:self.hi]

    def view(self, *shape):
        return self.t.view(*shape)

    def intact(self):
        """the surroundings still hold the sentinel"""
        return bool((self.raw[:self.lo] == self.sent).all()) and bool((self.raw[self.hi:] == self.sent).all())

    def untouched(self):
        """nothing at all was written"""
        return bool((self.raw == self.sent).all())

    def sentinel(self, t):
        """whether every element of t (a view of the inner buffer) still holds the sentinel"""
        return bool((t.contiguous().view(self.bits) == self.sent).all())


class Layer:
    """guarded W32 / V32 / Wb [N, M] and Wt [M, N] of one layer"""

    def __init__(self, N, M, device, w32_offset=0, wt_offset=0):
        self.N, self.M = N, M
        self.W32 = Guarded(N * M, torch.float32, device, offset=w32_offset)
        self.V32 = Guarded(N * M, torch.float32, device)
        self.Wb = Guarded(N * M, torch.bfloat16, device)
        self.Wt = Guarded(N * M, torch.bfloat16, device, offset=wt_offset)
        self.all = (self.W32, self.V32, self.Wb, self.Wt)

    def start(self, W0, V0, momentum):
        """the start state; without momentum V32 keeps its sentinel (the kernels must not touch it)"""
        self.W32.view(self.N, self.M).copy_(W0)
        if momentum:
            self.V32.view(self.N, self.M).copy_(V0)

    def args(self, momentum=True):
        """(W32, V32, Wb, Wt) as the ops wrappers take them"""
        return (self.W32.view(self.N, self.M), self.V32.view(self.N, self.M) if momentum else None,
                self.Wb.view(self.N, self.M), self.Wt.view(self.M, self.N))

    def check(self, W, V, momentum, what):
        """bitwise against the float64 reference state (W, V), every copy, every guard"""
        W32, _, Wb, Wt = self.args()
        assert torch.equal(W32.double(), W), (what, "W32", _diff(W32.double(), W))
        if momentum:
            assert torch.equal(self.V32.view(self.N, self.M).double(), V), (what, "V32")
            assert self.V32.intact(), (what, "V32 guard")
        else:
            assert self.V32.untouched(), (what, "V32 written without momentum")
        assert torch.equal(Wb, W32.bfloat16()), (what, "Wb")
        assert torch.equal(Wt, Wb.t()), (what, "Wt")
        assert self.W32.intact() and self.Wb.intact() and self.Wt.intact(), (what, "guards")

    def untouched(self):
        return all(g.untouched() for g in self.all)


def _diff(a, b):
    d = torch.nan_to_num((a - b).abs(), nan=float("inf"))
    return "max |diff| %g at %s, %d elements differ" % (d.max().item(), tuple(
        int(i) for i in torch.nonzero(d == d.max())[0]), int((d != 0).sum()))


# ---------------------------------------------------------------------------- exact data and reference
def exact(x):
    """x (float64) is representable in FP32"""
    assert torch.equal(x.float().double(), x), "the reference left the exactly representable range"
    return x


def int_operands(Bt, N, M, gen, device, ldd=None, ldh=None, bound=True):
    """D [Bt, N], H [Bt, M]: integers in [-3, 3] as BF16 (column slices of wider tensors when
    ldd / ldh are given); bound: columns 0 / 1 of D and column 0 of H forced to +3 / -3 / +3 so that
    G[0, 0] = 9 Bt and G[1, 0] = -9 Bt sit on the bound of the recipe, and column 1 of H to +3 but
    for one 2, so that G[0, 1] = 9 Bt - 3 is odd and above 256: it rounds when converted to BF16"""
    assert Bt <= BT_MAX
    D = torch.randint(-3, 4, (Bt, ldd or N), generator=gen).to(device).bfloat16()[:, :N]
    H = torch.randint(-3, 4, (Bt, ldh or M), generator=gen).to(device).bfloat16()[:, :M]
    if bound:
        D[:, 0], D[:, 1], H[:, 0], H[:, 1] = 3, -3, 3, 3
        H[0, 1] = 2
    return D, H


def start_state(N, M, gen, device):
    """W0, V0 (float64): multiples of 2^-13 in [-0.5, 0.5]"""
    W0 = torch.randint(-4096, 4097, (N, M), generator=gen).double() * 2.0 ** -13
    V0 = torch.randint(-4096, 4097, (N, M), generator=gen).double() * 2.0 ** -13
    return W0.to(device), V0.to(device)


def partials(D, H, splits):
    """float64 [splits, N, M]: the exact partial gradient of each split's batch rows"""
    rows = ops.split_rows(D.shape[0], splits)
    assert len({b - a for a, b in rows}) == 1
    Dd, Hd = D.double().reshape(splits, -1, D.shape[1]), H.double().reshape(splits, -1, H.shape[1])
    P = torch.bmm(Dd.transpose(1, 2), Hd)
    assert float(P.abs().max()) <= 9 * D.shape[0]
    return exact(P)


def ref_step(W, V, G, momentum):
    """one step of the recipe in float64, every intermediate asserted exact in FP32:
    v += lr * (g * scale); w += v; v *= alpha   (without momentum: w += lr * (g * scale))"""
    exact(G)
    u = exact(LR * exact(G * SCALE))
    if momentum:
        V = exact(V + u)
        W = exact(W + V)
        V = exact(V * ALPHA)
    else:
        W = exact(W + u)
    return W, V


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(*shape, gen, device, scale=1.0):
    return ((torch.rand(*shape, generator=gen) * 2 - 1) * scale).to(device)


# ---------------------------------------------------------------------------- MODE 1
def check_mode1(device, N, M, Bt, momentum, padded=False, seed=1):
    """LAUNCHES launches of ops.gemm_tn_update on one weight state, fresh exact operands each"""
    gen = _gen(seed)
    ldd, ldh = (N + 32, M + 64) if padded else (N, M)
    assert mode1_ok(N, M, Bt, ldd, ldh)
    L = Layer(N, M, device)
    W, V = start_state(N, M, gen, device)
    L.start(W, V, momentum)
    for k in range(LAUNCHES):
        D, H = int_operands(Bt, N, M, gen, device, ldd, ldh)
        assert D.stride(0) == ldd and H.stride(0) == ldh
        W32, V32, Wb, Wt = L.args(momentum)
        ok = ops.gemm_tn_update(D, H, W32, V32, Wb, Wt, LR, ALPHA, SCALE, momentum)
        assert ok is True, "launch %d refused" % k
        W, V = ref_step(W, V, partials(D, H, 1)[0], momentum)
        L.check(W, V, momentum, "launch %d" % k)
    return L


def check_mode1_refused(device):
    """every shape / pointer hpnn_gemm_tn8_update refuses returns False with nothing written"""
    gen = _gen(2)
    for N, M, Bt, w_off, wt_off, no_v in [(288, 256, 128, 0, 0, False), (256, 256, 192, 0, 0, False),
                                          (256, 256, 128, 1, 0, False), (256, 256, 128, 0, 4, False),
                                          (256, 256, 128, 0, 0, True)]:
        what = (N, M, Bt, w_off, wt_off, no_v)
        if not (w_off or wt_off or no_v):
            assert not mode1_ok(N, M, Bt, N, M), what
        L = Layer(N, M, device, w32_offset=w_off, wt_offset=wt_off)
        D, H = int_operands(Bt, N, M, gen, device)
        W32, V32, Wb, Wt = L.args(True)
        ok = ops.gemm_tn_update(D, H, W32, None if no_v else V32, Wb, Wt, LR, ALPHA, SCALE, True)
        assert ok is False, what
        assert L.untouched(), what


def grad_tol(G):
    """the project's tolerance for this GEMM on random BF16 operands (test_gemm_tn)"""
    return 1e-3 * float(G.abs().max()) + 1e-4


RLR, RSCALE, RALPHA = 0.05, 1.0 / 7, 0.2  # the ordinary step of the random-data cases


def check_random_step(L, W0, V0, G, momentum, what):
    """W32 / V32 after one RLR / RSCALE / RALPHA step from (W0, V0) hold the gradient G (float64)
    within grad_tol: BP  (W - W0) / (lr scale);  BPM  (V / alpha - V0) / (lr scale), and W = W0 + V / alpha
    within the FP32 rounding of the three operations on values below 4 (1e-6).  Wb / Wt bitwise."""
    W32, V32, Wb, Wt = L.args()
    tol = grad_tol(G)
    if momentum:
        v = V32.double() / RALPHA
        err = float(((v - V0) / (RLR * RSCALE) - G).abs().max())
        werr = float((W32.double() - (W0 + v)).abs().max())
        print("%s: W error %.3g (bound 1e-6)" % (what, werr))
        assert werr < 1e-6, (what, werr)
        assert L.V32.intact()
    else:
        err = float(((W32.double() - W0) / (RLR * RSCALE) - G).abs().max())
        assert L.V32.untouched()
    print("%s: gradient error %.3g (bound %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)
    assert torch.equal(Wb, W32.bfloat16()) and torch.equal(Wt, Wb.t()), what
    assert L.W32.intact() and L.Wb.intact() and L.Wt.intact(), what


def check_mode1_random(device, momentum, N=512, M=256, Bt=384, seed=3):
    gen = _gen(seed)
    L = Layer(N, M, device)
    W0, V0 = _rand(N, M, gen=gen, device=device), _rand(N, M, gen=gen, device=device, scale=0.1)
    L.start(W0, V0, momentum)
    D, H = _rand(Bt, N, gen=gen, device=device).bfloat16(), _rand(Bt, M, gen=gen, device=device).bfloat16()
    W32, V32, Wb, Wt = L.args(momentum)
    assert ops.gemm_tn_update(D, H, W32, V32, Wb, Wt, RLR, RALPHA, RSCALE, momentum) is True
    check_random_step(L, W0.double(), V0.double(), D.double().t() @ H.double(), momentum, "mode 1 random")
    return L


# ---------------------------------------------------------------------------- MODE 3
def check_mode3(device, N, M, Bt, ldg, seed=4):
    """LAUNCHES launches of ops.gemm_tn_bf16out into one guarded [N, ldg] buffer: bitwise the
    exact sum rounded once to BF16 (sums in the thousands do round), padding columns untouched"""
    gen = _gen(seed)
    assert mode3_ok(N, M, Bt, N + 32, M + 64) and ldg % 4 == 0 and ldg >= M
    Gd = Guarded(N * ldg, torch.bfloat16, device)
    G16 = Gd.view(N, ldg)
    rounded = False
    for k in range(LAUNCHES):
        D, H = int_operands(Bt, N, M, gen, device, N + 32, M + 64)
        assert ops.gemm_tn_bf16out(D, H, G16) == 0, "launch %d refused" % k
        G = partials(D, H, 1)[0]
        want = G.float().bfloat16()
        rounded = rounded or not torch.equal(want.double(), G)
        assert torch.equal(G16[:, :M], want), ("launch %d" % k, _diff(G16[:, :M].double(), want.double()))
        assert Gd.intact() and (ldg == M or Gd.sentinel(G16[:, M:])), "launch %d wrote outside G" % k
    assert rounded, "no sum needed rounding: the case does not test the conversion"


def check_mode3_random(device, N=512, M=256, Bt=384, seed=5):
    """random BF16 operands: |G16 - G| <= grad_tol + 2^-8 |G| (the FP32 result within the GEMM's
    tolerance, then one rounding to BF16's 8 significant bits: half an ulp is at most 2^-8 |x|)"""
    gen = _gen(seed)
    Gd = Guarded(N * M, torch.bfloat16, device)
    D, H = _rand(Bt, N, gen=gen, device=device).bfloat16(), _rand(Bt, M, gen=gen, device=device).bfloat16()
    assert ops.gemm_tn_bf16out(D, H, Gd.view(N, M)) == 0
    G = D.double().t() @ H.double()
    over = float(((Gd.view(N, M).double() - G).abs() - 2.0 ** -8 * G.abs()).max())
    print("mode 3 random: error beyond the BF16 rounding %.3g (bound %.3g)" % (over, grad_tol(G)))
    assert over <= grad_tol(G) and Gd.intact()


def check_mode3_ok_agrees(device, native_ok=None):
    """_ok and the launcher accept and refuse the same shapes"""
    ok = native_ok or mode3_ok
    gen = _gen(6)
    for N, M, Bt, ldg in MODE3_CASES:
        assert ok(N, M, Bt, N + 32, M + 64) and mode3_ok(N, M, Bt, N + 32, M + 64)
    for N, M, Bt, ldd, ldh in MODE3_REFUSED:
        assert not ok(N, M, Bt, ldd, ldh) and not mode3_ok(N, M, Bt, ldd, ldh), (N, M, Bt, ldd, ldh)
        if device.type == "cpu":
            continue  # the emulation applies to every shape
        Gd = Guarded(N * M, torch.bfloat16, device)
        D, H = int_operands(Bt, N, M, gen, device, ldd, ldh, bound=False)
        assert ops.gemm_tn_bf16out(D, H, Gd.view(N, M)) == -1, (N, M, Bt, ldd, ldh)
        assert Gd.untouched()


# ---------------------------------------------------------------------------- MODE 2 (+ side)
class Fused:
    """the buffers of one fused-update GEMM shape: guarded layer and slab, ticket block, error
    word; with a side job (N1, M1, S) the same for the next layer"""

    def __init__(self, device, N, M, Bt, splits, side=None, wt_offset=0, w32_offset=0):
        self.device, self.N, self.M, self.Bt, self.splits = device, N, M, Bt, splits
        self.L = Layer(N, M, device, w32_offset=w32_offset, wt_offset=wt_offset)
        self.slab = Guarded(splits * N * M, torch.float32, device)
        self.cnt = torch.zeros(512, dtype=torch.int64, device=device)
        self.err = torch.zeros(4, dtype=torch.int32, device=device)
        self.side = side
        if side:
            N1, M1, S = side
            self.L1 = Layer(N1, M1, device)
            self.slab1 = Guarded(S * N1 * M1, torch.float32, device)
            self.cnt1 = torch.zeros(8, dtype=torch.int64, device=device)

    def launch(self, D, H, momentum, D1=None, H1=None, lr=LR, alpha=ALPHA, scale=SCALE):
        W32, V32, Wb, Wt = self.L.args(momentum)
        sd = None
        if self.side:
            N1, M1, S = self.side
            a = self.L1.args(momentum)
            sd = ops.TnSide(D1, H1, S, self.slab1.view(S, N1, M1), a[0], a[1], a[2], a[3], self.cnt1[:1])
        return ops.gemm_tn_fused_update(D, H, self.splits, self.slab.view(self.splits, self.N, self.M), W32, V32,
                                        Wb, Wt, lr, alpha, scale, momentum, self.cnt, self.err[:1], sd)

    def check_protocol(self, launches, ntiles, eff, what):
        """err == 0; the 64-bit counter of every tile == launches * splits, 0 beyond the tiles"""
        assert int(self.err.abs().sum()) == 0, (what, "a ticket wait timed out")
        want = torch.zeros(512, dtype=torch.int64)
        want[0:16 * ntiles:16] = launches * eff
        assert torch.equal(self.cnt.cpu(), want), (what, "tickets", self.cnt.cpu()[::16].tolist())
        if self.side:
            want1 = torch.zeros(8, dtype=torch.int64)
            want1[0] = launches * ntiles * eff
            assert torch.equal(self.cnt1.cpu(), want1), (what, "side tickets", self.cnt1.tolist())

    def untouched(self):
        ok = self.L.untouched() and self.slab.untouched() and int(self.cnt.abs().sum()) == 0
        ok = ok and int(self.err.abs().sum()) == 0
        if self.side:
            ok = ok and self.L1.untouched() and self.slab1.untouched() and int(self.cnt1.abs().sum()) == 0
        return ok


def check_mode2(device, N, M, splits, Bt, momentum, padded=False, side=None, side_padded=False, tm128=False,
                wt_offset=0, seed=7):
    """LAUNCHES launches of ops.gemm_tn_fused_update on one weight state / slab / ticket block,
    fresh exact operands before each (a partial left over from the launch before is a different
    integer).  side: (N1, M1, S).  tm128: the process runs with HPNN_TN8_TM=128.  After each
    launch: both layers bitwise, the slabs (the first `eff` hold each split's exact partial, the
    rest the sentinel), the guards, the protocol words.  Returns the Fused state."""
    gen = _gen(seed)
    ldd, ldh = (N + 32, M + 64) if padded else (N, M)
    plan = mode2_plan(N, M, Bt, splits, ldd, ldh, tm128=tm128)
    assert plan is not None, "the case does not fit the launcher's rules"
    tm, ntiles, eff = plan
    assert (tm == 128) == tm128
    if side:
        assert side_fits(ntiles * eff, Bt, *side)
    F = Fused(device, N, M, Bt, splits, side, wt_offset=wt_offset)
    W, V = start_state(N, M, gen, device)
    F.L.start(W, V, momentum)
    if side:
        N1, M1, S = side
        W1, V1 = start_state(N1, M1, gen, device)
        F.L1.start(W1, V1, momentum)
    for k in range(LAUNCHES):
        what = "launch %d" % k
        D, H = int_operands(Bt, N, M, gen, device, ldd, ldh)
        D1 = H1 = None
        if side:
            D1, H1 = int_operands(Bt, N1, M1, gen, device, N1 + 64 if side_padded else N1,
                                  M1 + 8 if side_padded else M1)
        rc = F.launch(D, H, momentum, D1, H1)
        assert rc == 0, (what, "the launcher returned", rc)
        P = partials(D, H, eff)
        W, V = ref_step(W, V, exact(P.sum(0)), momentum)
        F.L.check(W, V, momentum, what)
        sl = F.slab.view(splits, N, M)
        assert torch.equal(sl[:eff].double(), P), (what, "published partials")
        assert F.slab.intact() and (eff == splits or F.slab.sentinel(sl[eff:])), (what, "slab guard")
        if side:
            P1 = partials(D1, H1, S)
            W1, V1 = ref_step(W1, V1, exact(P1.sum(0)), momentum)
            F.L1.check(W1, V1, momentum, what + " side")
            assert torch.equal(F.slab1.view(S, N1, M1).double(), P1), (what, "side partials")
            assert F.slab1.intact(), (what, "side slab guard")
        F.check_protocol(k + 1, ntiles, eff, what)
    return F


def check_mode2_refused(device, case, rc_want=-1, side=None):
    """a refused launch returns rc_want and writes nothing: no buffer, no ticket, no slab"""
    N, M, splits, Bt = case
    gen = _gen(8)
    F = Fused(device, N, M, Bt, splits, side)
    D, H = int_operands(Bt, N, M, gen, device, bound=False)
    D1 = H1 = None
    if side:
        D1, H1 = int_operands(Bt, side[0], side[1], gen, device, bound=False)
    rc = F.launch(D, H, True, D1, H1)
    assert rc == rc_want, (case, side, rc)
    assert F.untouched(), (case, side)


def check_mode2_random(device, momentum, case=MODE2_CASES[4], side=None, seed=9):
    """random BF16 operands, an ordinary step, twice from the same start state: the gradient
    within grad_tol and the two runs bitwise equal"""
    N, M, splits, Bt = case
    runs = []
    for _ in range(2):
        gen = _gen(seed)
        F = Fused(device, N, M, Bt, splits, side)
        W0, V0 = _rand(N, M, gen=gen, device=device), _rand(N, M, gen=gen, device=device, scale=0.1)
        F.L.start(W0, V0, momentum)
        D, H = _rand(Bt, N, gen=gen, device=device).bfloat16(), _rand(Bt, M, gen=gen, device=device).bfloat16()
        D1 = H1 = None
        if side:
            N1, M1, S = side
            W1, V1 = _rand(N1, M1, gen=gen, device=device), _rand(N1, M1, gen=gen, device=device, scale=0.1)
            F.L1.start(W1, V1, momentum)
            D1 = _rand(Bt, N1, gen=gen, device=device).bfloat16()
            H1 = _rand(Bt, M1, gen=gen, device=device).bfloat16()
        rc = F.launch(D, H, momentum, D1, H1, RLR, RALPHA, RSCALE)
        assert rc == 0, rc
        check_random_step(F.L, W0.double(), V0.double(), D.double().t() @ H.double(), momentum, "mode 2 random")
        if side:
            check_random_step(F.L1, W1.double(), V1.double(), D1.double().t() @ H1.double(), momentum,
                              "side random")
        runs.append(F)
    a, b = runs
    assert torch.equal(a.L.W32.raw, b.L.W32.raw) and torch.equal(a.L.V32.raw, b.L.V32.raw)
    assert torch.equal(a.L.Wb.raw, b.L.Wb.raw) and torch.equal(a.L.Wt.raw, b.L.Wt.raw)
    assert torch.equal(a.slab.raw, b.slab.raw)
    if side:
        assert torch.equal(a.L1.W32.raw, b.L1.W32.raw) and torch.equal(a.L1.Wt.raw, b.L1.Wt.raw)


def check_tm128(device):
    """the body of the HPNN_TN8_TM=128 child process: the 256 x 128 tile instantiation on two
    MODE 2 cases (the slab shows that it ran: exactly the first splits / 2 slabs are written)"""
    for N, M, splits, Bt in TM128_CASES:
        for momentum in (False, True):
            check_mode2(device, N, M, splits, Bt, momentum, tm128=True)


# ---------------------------------------------------------------------------- the BF16 helpers
# (csrc/gpu/kernels_misc.hip: the pieces of the BF16 data-/tensor-parallel exchanges, and the digest)
GRID_CAP = 4096 * 256  # work items one launch covers without its grid-stride loop
BIG = GRID_CAP * 4 + 4  # the first element count that enters the loop (4 elements per item)
HELPER_SIZES = [4, 1028, BIG]


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


# FP32 bit patterns whose conversion to BF16 goes wrong first: ties to even (down and up), just
# above / below a tie, FP32 and BF16 subnormals, +-0, +-inf, the largest finite values (they round up
# to inf), the largest value that does not, and NaN (first: every size gets one)
CAST_SPECIALS = [0x7fc00000, 0x3f808000, 0x3f818000, 0x3f808001, 0x3f817fff, 0x00000001, 0x00008000, 0x00018000,
                 0x007fffff, 0x80000000, 0x00000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000,
                 0x7f7f7fff, 0xbf808000, 0xffc00001]


def _same_bf16(got, want):
    """bitwise equal, a NaN matching any NaN"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn])


def check_cast(device, n, seed=20):
    gen = _gen(seed)
    src = torch.randn(n, generator=gen) * 100.0
    sp = _f32([b - (1 << 32) if b >> 31 else b for b in CAST_SPECIALS])
    k = min(n, sp.numel())
    src[:k] = sp[:k]
    if n >= 2 * sp.numel():
        src[-sp.numel():] = sp
    want = src.bfloat16()
    dst = Guarded(n, torch.bfloat16, device)
    assert ops.cast_f32_bf16(src.to(device), dst.t) == 0
    got = dst.t.cpu()
    assert _same_bf16(got, want), torch.nonzero(got.view(torch.int16) != want.view(torch.int16))[:8].tolist()
    assert bool(torch.isnan(got[0])) and dst.intact()
    if n >= 2 * sp.numel():
        assert bool(torch.isinf(got[-6])) and not bool(torch.isinf(got[-3]))  # 0x7f7fffff -> inf, 0x7f7f7fff not


def check_cast_refused(device):
    for n, so, do in [(6, 0, 0), (8, 1, 0), (8, 0, 1)]:
        src = torch.zeros(n + 4, device=device)[so:so + n]
        dst = Guarded(n, torch.bfloat16, device, offset=do)
        assert ops.cast_f32_bf16(src, dst.t) == -2, (n, so, do)
        assert dst.untouched()


def check_sgd_rows(device, n, momentum, seed=21):
    """the exact recipe with an integer-valued BF16 gradient, LAUNCHES steps: bitwise"""
    gen = _gen(seed)
    W0, V0 = start_state(1, n, gen, device)
    W, V = W0[0], V0[0]
    W32, V32, Wb = (Guarded(n, torch.float32, device), Guarded(n, torch.float32, device),
                    Guarded(n, torch.bfloat16, device))
    W32.t.copy_(W)
    if momentum:
        V32.t.copy_(V)
    for k in range(LAUNCHES):
        G = torch.randint(-256, 257, (n,), generator=gen).to(device).bfloat16()
        G[0], G[-1] = 256, -256
        assert torch.equal(G.double().round(), G.double())
        rc = ops.sgd_update_rows_bf16g(W32.t, V32.t if momentum else None, G, Wb.t, LR, ALPHA, SCALE, momentum)
        assert rc == 0, rc
        W, V = ref_step(W, V, G.double(), momentum)
        assert torch.equal(W32.t.double(), W), ("launch %d" % k, _diff(W32.t.double(), W))
        assert torch.equal(V32.t.double(), V) if momentum else V32.untouched(), "launch %d V32" % k
        assert torch.equal(Wb.t, W32.t.bfloat16()), "launch %d Wb" % k
        assert W32.intact() and V32.intact() and Wb.intact()


def check_sgd_rows_random(device, momentum, n=1028, seed=22):
    """random data against float64 at the absolute bound of test_sgd_update (1e-6)"""
    gen = _gen(seed)
    W0, V0 = _rand(n, gen=gen, device=device), _rand(n, gen=gen, device=device, scale=0.1)
    G = _rand(n, gen=gen, device=device).bfloat16()
    W, V, Wb = W0.clone(), V0.clone(), torch.empty(n, dtype=torch.bfloat16, device=device)
    assert ops.sgd_update_rows_bf16g(W, V if momentum else None, G, Wb, RLR, RALPHA, RSCALE, momentum) == 0
    g = G.double() * RSCALE
    if momentum:
        v = V0.double() + RLR * g
        w = W0.double() + v
        assert float((V.double() - v * RALPHA).abs().max()) < 1e-6
    else:
        w = W0.double() + RLR * g
        assert torch.equal(V, V0)
    assert float((W.double() - w).abs().max()) < 1e-6
    assert torch.equal(Wb, W.bfloat16())


def check_sgd_rows_refused(device):
    for n, wo, go, no_v in [(6, 0, 0, False), (8, 1, 0, False), (8, 0, 1, False), (8, 0, 0, True)]:
        W32, V32, Wb = (Guarded(n, torch.float32, device, offset=wo), Guarded(n, torch.float32, device),
                        Guarded(n, torch.bfloat16, device))
        G = torch.ones(n + 4, dtype=torch.bfloat16, device=device)[go:go + n]
        rc = ops.sgd_update_rows_bf16g(W32.t, None if no_v else V32.t, G, Wb.t, LR, ALPHA, SCALE, True)
        assert rc == -2, (n, wo, go, no_v, rc)
        assert W32.untouched() and V32.untouched() and Wb.untouched()


def _patterns(*shape, device):
    """distinct BF16 bit patterns: arange (mod 2^16) viewed as BF16"""
    n = 1
    for s in shape:
        n *= s
    return torch.arange(n, dtype=torch.int32).to(torch.int16).to(device).view(torch.bfloat16).view(*shape)


TRANSPOSE_SHAPES = [(32, 32), (32, 96), (96, 32), (256, 800)]


def check_transpose(device, N, K):
    Wb = _patterns(N, K, device=device)
    Wt = Guarded(N * K, torch.bfloat16, device)
    ops.transpose_bf16(Wb, Wt.view(K, N))
    assert torch.equal(Wt.view(K, N).view(torch.int16), Wb.view(torch.int16).t())
    assert Wt.intact()


def check_transpose_refused(device):
    import pytest
    for N, K in [(48, 32), (32, 40)]:
        Wt = Guarded(N * K, torch.bfloat16, device)
        with pytest.raises(RuntimeError, match="rc=-2"):
            ops.transpose_bf16(_patterns(N, K, device=device), Wt.view(K, N))
        assert Wt.untouched()


# (P, rows, n); the last: P rows n / 8 = 1049088 items, above the grid cap
PERMUTE_CASES = [(P, rows, n) for P in (1, 2, 3, 8) for n in (8, 24, 256) for rows in (1, 130)] + [(2, 2049, 2048)]
assert 2 * 2049 * (2048 // 8) > GRID_CAP


def check_block_permute(device, P, rows, n):
    src = _patterns(P, rows, n, device=device)
    dst = Guarded(P * rows * n, torch.bfloat16, device)
    ops.block_permute(src, dst.view(rows, P * n))
    want = src.view(torch.int16).permute(1, 0, 2).reshape(rows, P * n)
    assert torch.equal(dst.view(rows, P * n).view(torch.int16), want)
    assert dst.intact()


def check_block_permute_refused(device):
    """device tensors only (the CPU emulation takes any n): n % 8, a misaligned destination"""
    import pytest
    for n, off in [(12, 0), (16, 4)]:
        dst = Guarded(2 * 4 * n, torch.bfloat16, device, offset=off)
        with pytest.raises(RuntimeError, match="rc=-2"):
            ops.block_permute(_patterns(2, 4, n, device=device), dst.view(4, 2 * n))
        assert dst.untouched()


def _bf16_key(t):
    """BF16 values as integers ordered like the values (adjacent values differ by one)"""
    b = t.view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7fff))


def check_dact(device, n, seed=23):
    """out = bf16(x * f'(H)) against the float64 product rounded to BF16, within one BF16 ulp (the
    kernel rounds the product to FP32 first); f'(+-1) = 0 exactly"""
    gen = _gen(seed)
    x = (torch.randn(n, generator=gen) * 4.0).to(device)
    H = _rand(n, gen=gen, device=device).bfloat16()
    H[0], H[1], H[-1] = 1.0, -1.0, -1.0
    H[2] = 0.0
    out = Guarded(n, torch.bfloat16, device)
    ops.dact_cast(out.t, x, H)
    ref = x.double() * (-0.5 * (H.double() ** 2 - 1.0))
    assert int((_bf16_key(out.t) - _bf16_key(ref.float().bfloat16())).abs().max()) <= 1
    for i in (0, 1, -1):
        assert float(out.t[i]) == 0.0
    assert float(out.t[2]) == float((x[2] * 0.5).bfloat16())
    assert out.intact()


def check_dact_refused(device):
    """device tensors only: n % 4, a misaligned output"""
    import pytest
    for n, off in [(6, 0), (8, 2)]:
        out = Guarded(n, torch.bfloat16, device, offset=off)
        with pytest.raises(RuntimeError, match="rc=-2"):
            ops.dact_cast(out.t, torch.ones(n, device=device), torch.ones(n, dtype=torch.bfloat16, device=device))
        assert out.untouched()


M64 = (1 << 64) - 1


def digest_py(words, base=0, start=0):
    """the digest of hpnn_hash_words in plain Python integers (kernels_misc.hip: the wrapping sum
    over i of the murmur3 finalizer of (word_i << 32) ^ (i + base) ^ 0x9e3779b97f4a7c15)"""
    h = start & M64
    for i, w in enumerate(words):
        x = ((w & 0xffffffff) << 32) ^ ((i + base) & M64) ^ 0x9e3779b97f4a7c15
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & M64
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 & M64
        x ^= x >> 33
        h = (h + x) & M64
    return h - (1 << 64) if h >> 63 else h


def digest(t, base=0, start=0, nbytes=None):
    """the numpy emulation (ops.hash_words on a CPU copy)"""
    out = torch.tensor([start], dtype=torch.int64)
    assert ops.hash_words(t.cpu().contiguous(), out, base, nbytes) == 0
    return int(out[0])


HASH_SIZES = [1, 255, 257, 1024 * 256 + 1]  # words; the last needs more than the 1024-block cap


def check_hash(device, n, seed=24):
    gen = _gen(seed + n)
    w = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    want = digest(w)
    if n <= 257:  # the emulation itself against plain integers
        assert want == digest_py(w.tolist()) and digest(w, 12345, -5) == digest_py(w.tolist(), 12345, -5)
    wd = w.to(device)
    out = torch.zeros(3, dtype=torch.int64, device=device)

    def run(t, base=0, start=0, nbytes=None):
        out.zero_()
        out[1] = start
        rc = ops.hash_words(t, out[1:2], base, nbytes)
        assert int(out[0]) == 0 and int(out[2]) == 0
        return rc, int(out[1])

    assert run(wd) == (0, want)
    assert run(wd, base=12345) == (0, digest(w, 12345)) and digest(w, 12345) != want
    assert run(wd, start=-5) == (0, digest(w, 0, -5))  # accumulates, wrapping
    k = n // 3
    if k:  # two pieces with their offsets == the whole
        assert ops.hash_words(wd[:k].contiguous(), out[1:2].zero_(), 0) == 0
        assert ops.hash_words(wd[k:].contiguous(), out[1:2], k) == 0
        assert int(out[1]) == want
    w2 = wd.clone()
    w2[n // 2] ^= 1 << 17
    rc, h2 = run(w2)
    assert rc == 0 and h2 != want and h2 == digest(w2)
    assert run(wd, start=77, nbytes=0) == (0, 77)
    if n >= 2:
        assert run(wd, start=77, nbytes=6) == (-1, 77)
        assert run(wd, nbytes=4 * (n - 1)) == (0, digest(w[:n - 1]))
    # a BF16 buffer, as the engine hashes its weights
    b = w.view(torch.bfloat16)
    assert run(b.to(device)) == (0, want)
