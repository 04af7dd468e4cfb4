"""Cases, exact references and check functions for every arm of the BF16 NT / TN GEMM dispatch
(csrc/gpu/kernels_mfma.hip, kernels_ws.hip and the hand-over to kernels_8ph.hip), for the tail
reduction riding a TN launch, the launchers' refusals, cast_weights and reduce_slabs2.  Shared by
test_gemm_exact_gpu.py (which runs them on the kernels) and test_gemm_exact_cpu.py (which runs them on
CPU tensors through the emulations of hpnn_amd.ops and checks the case tables against the dispatcher).

The oracle: operands are integers in [-3, 3] stored as BF16 (B times a power of two for EPI_ACT), so
every product and partial sum is an integer of magnitude at most 9 * depth (depth: K for NT, the rows of
one split for TN).  With 9 * depth < 2^24 the FP32 result is exact in any summation order and the
float64 product is the answer bit for bit.  Every output is a Guarded region (tests/tn8_common.py) with
a padded row stride: padding and surroundings keep the sentinel, every in-range element leaves it.

Which arm a case runs is asked of the dispatcher itself (ops.gemm_nt_plan / ops.gemm_tn_plan): a case
lists its arm and how its K-step count KT relates to the ring depth ST of that arm's instantiation,
and every check asserts both before it launches."""
import contextlib
import os
from collections import namedtuple

import torch

from hpnn_amd import ops
from hpnn_amd._lib import native
from tests.tn8_common import Guarded, _diff, _gen, exact

EPIS = (ops.EPI_NONE, ops.EPI_ACT, ops.EPI_DACT)
EPI_NAME = {ops.EPI_NONE: "none", ops.EPI_ACT: "act", ops.EPI_DACT: "dact"}
ACT_TOL = {True: 2e-3, False: 2e-2}  # FP32 / BF16 output, absolute on outputs in [-1, 1] (test_gemm_nt)
LDC_PAD = 64  # every output row stride is N + LDC_PAD


# ---------------------------------------------------------------------------- run-time toggles
_TOGGLE_ENV = {"gemm_nt_set_8ph": "HPNN_NT_8PH", "gemm_tn_set_8ph": "HPNN_TN_8PH", "gemm_nt_set_pp": "HPNN_NT_PP"}


@contextlib.contextmanager
def toggled(**off):
    """toggled(gemm_nt_set_pp=0): the launcher toggle set for the block, its start-up value (on, unless
    its HPNN_* switch says 0) put back in a finally"""
    try:
        for name, v in off.items():
            getattr(native(), name)(v)
        yield
    finally:
        for name in off:
            getattr(native(), name)(0 if os.environ.get(_TOGGLE_ENV[name], "1")[:1] == "0" else 1)


# ---------------------------------------------------------------------------- KT relative to ST
def rel_kt(rel, st, kt=None):
    """the K-step count a relation stands for at ring depth st ("deep": any count above 2 st + 1)"""
    if rel == "deep":
        assert kt is not None and kt > 2 * st + 1
        return kt
    return {"1": 1, "2": 2, "ST-1": st - 1, "ST": st, "ST+1": st + 1, "2ST+1": 2 * st + 1, "2ST+2": 2 * st + 2}[rel]


def act_scale(K):
    """the power of two B is scaled by for EPI_ACT: a sum of K products of two uniform integers in
    [-3, 3] has standard deviation 4 sqrt(K); scaled to at most 8, so about two thirds of the
    pre-activations lie in [-8, 8] where the bipolar sigmoid is not saturated"""
    s = 1.0
    while 4.0 * K ** 0.5 * s > 8.0:
        s /= 2
    return s


# ---------------------------------------------------------------------------- NT cases
# arm -> (BK, ST) of its instantiation (ST is asserted against the dispatcher's answer)
NT_ARM = {"bn128_bk64": (64, 2), "bn128_bk32": (32, 4), "bn64_bk64": (64, 2), "bn64_bk32": (32, 5),
          "bn32_bk64": (64, 3), "bn32_bk32": (32, 5), "pp128": (64, 5), "w8_128": (64, 3), "256x256": (64, 2),
          "8ph": (128, 0), "ws": (32, None)}

# padded: lda = K + 64, ldb = K + 32, ldaux = N + 32.  off: toggles switched off for the case.
# scale: the EPI_ACT scale of B (= act_scale(K)).  big: a workload-size case (one per arm rule).
NtCase = namedtuple("NtCase", "arm M N K rel padded off scale big")


def _nt(arm, M, N, rel, padded, off=(), big=False, K=None):
    bk, st = NT_ARM[arm]
    K = K if K is not None else bk * rel_kt(rel, st)
    return NtCase(arm, M, N, K, rel, padded, tuple(off), act_scale(K), big)


def _nt_cases():
    cases = []
    # the 4-wave 128 x BN tile with BK = 32 (K % 64 != 0: odd KT only) and BK = 64, BN in {64, 32}:
    # 2 x 3 tiles with padded operands at every admitted KT, one tile dense at the first and last
    for bn in (128, 64, 32):
        for bk in (32, 64):
            arm = "bn%d_bk%d" % (bn, bk)
            if arm == "bn128_bk64":
                continue
            st = NT_ARM[arm][1]
            rels = [r for r in ("1", "ST-1", "ST", "ST+1", "2ST+1") if bk == 64 or rel_kt(r, st) % 2 == 1]
            rels = [r for i, r in enumerate(rels) if rel_kt(r, st) >= 1 and rel_kt(r, st) not in
                    [rel_kt(q, st) for q in rels[:i]]]
            for r in rels:
                cases.append(_nt(arm, 256, 3 * bn, r, True))
            m1 = 256 if bn == 128 else 128  # M != N
            cases.append(_nt(arm, m1, bn, rels[0], False))
            cases.append(_nt(arm, m1, bn, rels[-1], False))
    # the 4-wave 128 x 128 x 64 tile: from 512 tiles of 128 x 128 (ST = 2: KT 1, 2, 3, 5)
    for r, padded in (("ST-1", False), ("ST", True), ("ST+1", False), ("2ST+1", False)):
        cases.append(_nt("bn128_bk64", 8192, 1024, r, padded, big=True))
    # under 512 tiles: the software-pipelined 128 x 128 kernel, and the 8-wave kernel it replaced
    for arm, off in (("pp128", ()), ("w8_128", ("gemm_nt_set_pp",))):
        st = NT_ARM[arm][1]
        for r in ("1", "ST-1", "ST", "ST+1", "2ST+1"):
            if r == "ST-1" and st - 1 == 1:
                continue
            cases.append(_nt(arm, 256, 384, r, True, off))
        cases.append(_nt(arm, 128, 256, "1", False, off))
        cases.append(_nt(arm, 384, 256, "ST+1", False, off))
    # 256 tiles of 256 x 256: the 1-phase kernel where K % 128 != 0 or the 8-phase kernel is off, else
    # the 8-phase kernel (exact in test_gemm_nt8_integer_exact; here the hand-over from the dispatcher)
    cases.append(_nt("256x256", 4096, 4096, "deep", True, big=True, K=576))
    cases.append(_nt("256x256", 4096, 4096, "deep", False, ("gemm_nt_set_8ph",), big=True, K=512))
    cases.append(_nt("8ph", 4096, 4096, "deep", False, big=True, K=512))
    return cases


NT_CASES = _nt_cases()


def nt_id(c):
    return "%s-%dx%dx%d-%s%s" % (c.arm, c.M, c.N, c.K, c.rel, "-pad" if c.padded else "")


def nt_plan_of(c, epi):
    """the dispatcher's answer for the case with this epilogue (under the case's toggles)"""
    lda, ldb, ldaux = (c.K + 64, c.K + 32, c.N + 32) if c.padded else (c.K, c.K, c.N)
    with toggled(**{t: 0 for t in c.off}):
        return ops.gemm_nt_plan(c.M, c.N, c.K, lda, ldb, c.N + LDC_PAD, epi, epi == ops.EPI_DACT, ldaux)


def assert_nt_plan(c):
    """the case lands on the arm it is listed for, at the listed KT-to-ST relation, for every epilogue"""
    bk, st = NT_ARM[c.arm]
    for epi in EPIS:
        assert nt_plan_of(c, epi) == (c.arm, st), (nt_id(c), EPI_NAME[epi], nt_plan_of(c, epi))
    assert c.K % bk == 0 and c.K // bk == rel_kt(c.rel, st, c.K // bk), nt_id(c)
    assert c.M != c.N or c.big  # the square cases are the 4096-wide ones
    assert 9 * c.K < 2 ** 24 and c.scale == act_scale(c.K)


def int_mat(rows, cols, ld, gen, device, scale=1.0):
    """[rows, cols] integers in [-3, 3] (times scale) as BF16, a column slice of a [rows, ld] tensor"""
    return (torch.randint(-3, 4, (rows, ld), generator=gen).to(device) * scale).bfloat16()[:, :cols]


def nt_operands(M, N, K, padded, gen, device):
    """A [M, K], B [N, K] integer-valued, aux [M, N] from {0, +-0.5, +-1} (f'(aux) = 0.5, 0.375, 0)"""
    lda, ldb, ldaux = (K + 64, K + 32, N + 32) if padded else (K, K, N)
    A = int_mat(M, K, lda, gen, device)
    B = int_mat(N, K, ldb, gen, device)
    aux = (torch.randint(-2, 3, (M, ldaux), generator=gen).to(device) * 0.5).bfloat16()[:, :N]
    assert A.stride(0) == lda and B.stride(0) == ldb and aux.stride(0) == ldaux
    return A, B, aux


def nt_product(A, B):
    """float64: the exact product, asserted exact in FP32 and within 9 K"""
    R = exact(A.double() @ B.double().t())
    assert float(R.abs().max()) <= 9 * A.shape[1]
    return R


def nt_epilogue(R, aux, epi, scale):
    """float64: the epilogue on the exact product R.  EPI_ACT: of the product with scale * B"""
    if epi == ops.EPI_ACT:
        P = exact(R * scale)
        frac = float((P.abs() <= 8.0).double().mean())
        assert frac >= 0.5, ("the scale leaves %.2f of the pre-activations in [-8, 8]" % frac)
        return ops.bipolar(P)
    if epi == ops.EPI_DACT:
        return exact(R * (-0.5 * (aux.double() ** 2 - 1.0)))
    return R


def scaled_copy(B, scale):
    """scale * B (exact: a power of two) with B's row stride"""
    Bs = torch.zeros(B.shape[0], B.stride(0), dtype=torch.bfloat16, device=B.device)[:, :B.shape[1]]
    Bs.copy_(B * scale)
    assert torch.equal(Bs.double(), B.double() * scale) and Bs.stride(0) == B.stride(0)
    return Bs


def out_buffer(rows, cols, f32, device):
    """a Guarded [rows, cols + LDC_PAD] buffer and its [rows, cols] in-range view"""
    g = Guarded(rows * (cols + LDC_PAD), torch.float32 if f32 else torch.bfloat16, device)
    return g, g.view(rows, cols + LDC_PAD)[:, :cols]


def check_out(g, C, what):
    """guards and padding columns keep the sentinel; every in-range element has left it"""
    full = g.view(C.shape[0], -1)
    assert g.intact(), (what, "wrote outside the buffer")
    assert g.sentinel(full[:, C.shape[1]:]), (what, "wrote into the padding columns")
    left = int((C.contiguous().view(g.bits) == g.sent).sum())
    assert left == 0, (what, "%d in-range elements not written" % left)


def compare_epi(outs, R, epi, what):
    """outs: {f32: C}.  EPI_NONE / EPI_DACT: the FP32 output equals R, the BF16 output R rounded once.
    EPI_ACT: each within the project's tolerance of R, and the BF16 output == bfloat16(FP32 output)."""
    if epi == ops.EPI_ACT:
        for f32, C in outs.items():
            err = float((C.double() - R).abs().max())
            assert err <= ACT_TOL[f32], (what, "f32" if f32 else "bf16", err)
        if len(outs) == 2:
            assert torch.equal(outs[False], outs[True].bfloat16()), (what, "BF16 output != bfloat16(FP32 output)")
        return
    for f32, C in outs.items():
        want = R.float() if f32 else R.float().bfloat16()
        assert torch.equal(C, want), (what, "f32" if f32 else "bf16", _diff(C.double(), want.double()))


def check_nt(device, c, launch=None, epis=EPIS, types=(True, False), seed=31):
    """one NT case through ops.gemm_nt (or launch(A, B, epi, aux, C)): the plan, then every epilogue
    and both output types against the float64 reference"""
    assert_nt_plan(c)
    gen = _gen(seed + c.M + 3 * c.N + c.K)
    A, B, aux = nt_operands(c.M, c.N, c.K, c.padded, gen, device)
    Bs = scaled_copy(B, c.scale)
    R0 = nt_product(A, B)
    with toggled(**{t: 0 for t in c.off}):
        for epi in epis:
            R = nt_epilogue(R0, aux, epi, c.scale)
            outs = {}
            for f32 in types:
                what = (nt_id(c), EPI_NAME[epi], "f32" if f32 else "bf16")
                g, C = out_buffer(c.M, c.N, f32, device)
                a = aux if epi == ops.EPI_DACT else None
                b = Bs if epi == ops.EPI_ACT else B
                if launch is None:
                    ops.gemm_nt(A, b, epi, aux=a, out_f32=f32, out=C)
                else:
                    launch(A, b, epi, a, C)
                check_out(g, C, what)
                outs[f32] = C
            compare_epi(outs, R, epi, nt_id(c))


# ---------------------------------------------------------------------------- weight-stationary
WS_PAIRS = [(128, 800), (64, 800), (128, 512), (128, 1024)]  # the instantiated (N, K)
WS_ST = {800: 3, 512: 4, 1024: 2}  # ring depth by K
CPU_CUS = 256  # the CPU companion lays the persistent grid out for 256 CUs


def ws_rows(cus):
    """M: one tile (one workgroup, nloc = 1); one workgroup with two tiles beside cus - 1 with one; nloc 4
    and 5, above every ring depth"""
    return [32, 32 * (cus + 1), 32 * (4 * cus + 3)]


def check_ws(device, N, K, M, seed=41):
    """the kernel called directly (ops.gemm_nt_ws), EPI_NONE / EPI_ACT, both output types, X with a padded
    row stride"""
    assert native().gemm_nt_ws_plan(M, N, K, K + 64, K, N + LDC_PAD, ops.EPI_NONE) == WS_ST[K]
    assert 9 * K < 2 ** 24 and M != N
    gen = _gen(seed + M + N + K)
    X, W = int_mat(M, K, K + 64, gen, device), int_mat(N, K, K, gen, device)
    scale = act_scale(K)
    Ws = scaled_copy(W, scale)
    R0 = nt_product(X, W)
    for epi in (ops.EPI_NONE, ops.EPI_ACT):
        R = nt_epilogue(R0, None, epi, scale)
        outs = {}
        for f32 in (True, False):
            g, C = out_buffer(M, N, f32, device)
            rc = ops.gemm_nt_ws(X, Ws if epi == ops.EPI_ACT else W, epi, C)
            assert rc == 0, (N, K, M, rc)
            check_out(g, C, ("ws", N, K, M, EPI_NAME[epi], f32))
            outs[f32] = C
        compare_epi(outs, R, epi, ("ws", N, K, M))


def check_ws_refused(device):
    """EPI_DACT, a K or an N without an instance, ldx % 8 != 0: 1, the output untouched"""
    gen = _gen(42)
    for N, K, ldx, epi in [(128, 800, 800, ops.EPI_DACT), (128, 768, 768, ops.EPI_NONE), (32, 800, 800, ops.EPI_NONE),
                           (128, 800, 804, ops.EPI_NONE)]:
        X = int_mat(64, K, ldx, gen, device)
        W = int_mat(N, K, K, gen, device)
        g, C = out_buffer(64, N, True, device)
        assert ops.gemm_nt_ws(X, W, epi, C) == 1, (N, K, ldx, epi)
        assert g.untouched(), (N, K, ldx, epi)
        assert native().gemm_nt_ws_plan(64, N, K, ldx, K, N + LDC_PAD, epi) == 0


WS_DISPATCH_CASE = NtCase("ws", 16384, 128, 512, "deep", True, (), act_scale(512), True)


def check_ws_dispatched(device):
    """M = 16384 through ops.gemm_nt: the plan says weight-stationary"""
    c = WS_DISPATCH_CASE
    for epi in (ops.EPI_NONE, ops.EPI_ACT):
        assert ops.gemm_nt_plan(c.M, c.N, c.K, c.K + 64, c.K + 32, c.N + LDC_PAD, epi) == ("ws", WS_ST[c.K])
    gen = _gen(43)
    A, B, _ = nt_operands(c.M, c.N, c.K, True, gen, device)
    for f32 in (True, False):
        g, C = out_buffer(c.M, c.N, f32, device)
        ops.gemm_nt(A, B, ops.EPI_NONE, out_f32=f32, out=C)
        check_out(g, C, ("ws dispatched", f32))
        compare_epi({f32: C}, nt_product(A, B), ops.EPI_NONE, "ws dispatched")


# ---------------------------------------------------------------------------- NN form
NN_SHAPE = (256, 384, 320)  # M, N, K


def check_nn(device, epi, seed=44):
    """gemm_nn (W row-major [K][N]) against the float64 reference of A . W, both output types; padded
    strides on every operand"""
    M, N, K = NN_SHAPE
    gen = _gen(seed + epi)
    A, Wt, aux = nt_operands(M, N, K, True, gen, device)
    scale = act_scale(K)
    W = torch.zeros(K, N + 32, dtype=torch.bfloat16, device=device)[:, :N]
    W.copy_(Wt.t() * (scale if epi == ops.EPI_ACT else 1.0))
    assert W.stride(0) == N + 32
    R = nt_epilogue(nt_product(A, Wt), aux, epi, scale)
    outs = {}
    for f32 in (True, False):
        g, C = out_buffer(M, N, f32, device)
        ops.gemm_nn(A, W, epi, aux=aux if epi == ops.EPI_DACT else None, out_f32=f32, out=C)
        check_out(g, C, ("nn", EPI_NAME[epi], f32))
        outs[f32] = C
    compare_epi(outs, R, epi, ("nn", EPI_NAME[epi]))


# ---------------------------------------------------------------------------- TN cases
# arm -> ring depth ST; KT = 2 * (64-row units of the split) is even
TN_ST = {"8ph": 0, "256x256": 4, "t64": 6,
         "tm128_tn128": 4, "tm128_tn64": 6, "tm128_tn32": 6, "tm160_tn128": 4, "tm160_tn64": 5, "tm160_tn32": 6,
         "tm96_tn128": 5, "tm96_tn64": 6, "tm96_tn32": 6, "tm64_tn128": 6, "tm64_tn64": 6, "tm64_tn32": 6,
         "tm32_tn128": 6, "tm32_tn64": 6, "tm32_tn32": 6}
# (N, M, fewest splits at which the arm is chosen).  2 tile rows x 3 tile columns where the arm's rule
# allows it; where the 64 x 64 rule would capture that shape M is taken off a multiple of 64 (3 or 7
# tile rows).  The four pairs with M, N % 64 == 0 are chosen only once (M / 128)(N / 128) splits >= 256,
# which no N, M <= 640 with splits <= 8 reaches (TN_SWEEP_UNREACHED, proven by the CPU test's sweep of
# the dispatcher); they are reached here at 29 to 128 splits.
TN_SHAPES = {"t64": (192, 128, 1),
             "tm128_tn128": (384, 256, 43), "tm128_tn64": (192, 256, 128), "tm128_tn32": (96, 256, 1),
             "tm160_tn128": (384, 480, 1), "tm160_tn64": (192, 480, 1), "tm160_tn32": (96, 320, 1),
             "tm96_tn128": (384, 288, 1), "tm96_tn64": (192, 288, 1), "tm96_tn32": (96, 192, 1),
             "tm64_tn128": (384, 448, 29), "tm64_tn64": (192, 448, 86), "tm64_tn32": (96, 448, 1),
             "tm32_tn128": (384, 224, 1), "tm32_tn64": (192, 224, 1), "tm32_tn32": (96, 224, 1)}
TN_SWEEP_UNREACHED = {"tm128_tn128", "tm128_tn64", "tm64_tn128", "tm64_tn64", "8ph", "256x256"}
TN_UNREACHABLE = set()  # pairs no shape can reach: none

# kts: the set of K-step counts over the splits, as relations to ST ("uneven": more than one count).
# padded: ldd = N + 32, ldh = M + 64.  ldg: the slab row stride (M + 4 or M + 64).
TnCase = namedtuple("TnCase", "arm N M Bt splits rel padded ldg off big")


def _tn(arm, N, M, units, splits, rel, padded, pad_g=64, off=(), big=False):
    return TnCase(arm, N, M, 64 * units, splits, rel, padded, M + pad_g, tuple(off), big)


def _tn_cases():
    cases = []
    for arm, (N, M, s0) in TN_SHAPES.items():
        st = TN_ST[arm]
        s = max(s0, 3)
        cases.append(_tn(arm, N, M, s, s, "2", True))  # one unit per split
        sp = max(s0, 2)
        rels = [r for r in ("ST-1", "ST", "ST+1", "2ST+1", "2ST+2") if rel_kt(r, st) % 2 == 0]
        for i, r in enumerate(rels):
            cases.append(_tn(arm, N, M, sp * rel_kt(r, st) // 2, sp, r, i % 2 == 1, 4 if i % 2 else 64))
        if s0 == 1:
            cases.append(_tn(arm, N, M, 7, 3, "uneven", False, 4))
            cases.append(_tn(arm, N, M, 12, 8, "uneven", True))  # splits % 8 == 0, > 1 tile: xcd_map on
        else:
            cases.append(_tn(arm, N, M, s0 + s0 // 2, s0, "uneven", True, 4))
    # xcd_map: 16 splits with uneven units; 8 splits on one tile (the map is off)
    cases.append(_tn("tm128_tn32", 96, 256, 27, 16, "uneven", True))
    cases.append(_tn("tm32_tn64", 64, 32, 12, 8, "uneven", False, 4))
    cases.append(_tn("t64", 64, 128, 12, 8, "uneven", True))
    # 256 tiles of 256 x 256: the 4-stage kernel where the 8-phase launcher declines (Bt = 64: KT = 2; an
    # odd unit count; uneven splits; one unit per split with xcd_map on) or is switched off
    cases.append(_tn("256x256", 4096, 4096, 1, 1, "2", False, 64, big=True))
    cases.append(_tn("256x256", 4096, 4096, 3, 1, "ST+2", True, 4, big=True))
    cases.append(_tn("256x256", 4096, 4096, 4, 1, "2ST", False, 64, ("gemm_tn_set_8ph",), big=True))
    cases.append(_tn("256x256", 2048, 2048, 6, 4, "uneven", True, 64, big=True))
    cases.append(_tn("256x256", 2048, 2048, 8, 8, "2", False, 4, big=True))
    cases.append(_tn("8ph", 4096, 4096, 2, 1, "any", True, 64, big=True))
    cases.append(_tn("8ph", 4096, 4096, 4, 1, "any", False, 4, big=True))
    return cases


def tn_kts(c):
    return sorted({(b - a) // 32 for a, b in ops.split_rows(c.Bt, c.splits)})


def tn_rel_kts(rel, st):
    return {"ST+2": [st + 2], "2ST": [2 * st]}.get(rel) or [rel_kt(rel, st)]


TN_CASES = _tn_cases()


def tn_id(c):
    return "%s-%dx%d-b%d-s%d-%s%s" % (c.arm, c.N, c.M, c.Bt, c.splits, c.rel, "-pad" if c.padded else "")


def tn_plan_of(c):
    ldd, ldh = (c.N + 32, c.M + 64) if c.padded else (c.N, c.M)
    with toggled(**{t: 0 for t in c.off}):
        return ops.gemm_tn_plan(c.N, c.M, c.Bt, c.splits, ldd, ldh, c.ldg)


def assert_tn_plan(c):
    st = TN_ST[c.arm]
    assert tn_plan_of(c) == (c.arm, st), (tn_id(c), tn_plan_of(c))
    kts = tn_kts(c)
    if c.rel == "uneven":
        assert len(kts) > 1, tn_id(c)
    elif c.rel != "any":
        assert kts == tn_rel_kts(c.rel, st), (tn_id(c), kts)
    assert c.M != c.N or c.big  # the square cases are the 4096- and 2048-wide ones the issue names
    assert 9 * max(b - a for a, b in ops.split_rows(c.Bt, c.splits)) < 2 ** 24


def tn_operands(c, gen, device):
    ldd, ldh = (c.N + 32, c.M + 64) if c.padded else (c.N, c.M)
    D, H = int_mat(c.Bt, c.N, ldd, gen, device), int_mat(c.Bt, c.M, ldh, gen, device)
    assert D.stride(0) == ldd and H.stride(0) == ldh
    return D, H


def tn_reference(D, H, splits):
    """float64 [splits, N, M]: each split's product over its own row range, asserted exact in FP32"""
    P = torch.stack([D[a:b].double().t() @ H[a:b].double() for a, b in ops.split_rows(D.shape[0], splits)])
    return exact(P)


def slab_buffer(c, device):
    g = Guarded(c.splits * c.N * c.ldg, torch.float32, device)
    return g, g.view(c.splits, c.N, c.ldg)[:, :, :c.M]


def check_slab(g, out, P, what):
    full = g.view(out.shape[0], out.shape[1], -1)
    assert g.intact(), (what, "wrote outside the slab")
    assert g.sentinel(full[:, :, out.shape[2]:]), (what, "wrote into the padding columns")
    for s in range(out.shape[0]):
        assert torch.equal(out[s].double(), P[s]), (what, "split %d" % s, _diff(out[s].double(), P[s]))


def check_tn(device, c, seed=51):
    """one TN case through ops.gemm_tn: the plan, then every split's slab against the float64 product
    of its own rows"""
    assert_tn_plan(c)
    gen = _gen(seed + c.N + 3 * c.M + c.Bt + c.splits)
    D, H = tn_operands(c, gen, device)
    g, out = slab_buffer(c, device)
    with toggled(**{t: 0 for t in c.off}):
        ops.gemm_tn(D, H, c.splits, out=out)
    check_slab(g, out, tn_reference(D, H, c.splits), tn_id(c))
    return g


# ---------------------------------------------------------------------------- the tail reduction
TAIL_SG = [(1, 1), (5, 5), (9, 8), (100, 7), (37, 4)]  # (S, groups); (9, 8) leaves three groups empty
TAIL_N = [4, 1020, 1024, 10240]


def _first(arm, pred=lambda c: True):
    return next(c for c in TN_CASES if c.arm == arm and pred(c))


# one case of each launch shape: TM x TN, 64 x 64, xcd_map on, 256 x 256 4-stage, 8-phase
TAIL_LAUNCHES = [_first("tm96_tn32", lambda c: c.splits == 3), _first("t64", lambda c: c.splits == 3),
                 _first("tm128_tn32", lambda c: c.splits == 16), _first("256x256", lambda c: c.splits == 4),
                 _first("8ph")]


def group_sums(rslab, groups):
    """float64 [groups, n]: rows [g * ceil(S / groups), ...) summed, an empty group zero"""
    S = rslab.shape[0]
    sg = -(-S // groups)
    return exact(torch.stack([rslab[g * sg:min(S, (g + 1) * sg)].double().sum(0) for g in range(groups)]))


def check_tn_tail(device, c, S, groups, n, seed=61):
    """ops.gemm_tn_reduce: rout (Guarded) == the float64 group sums of the integer-valued rslab bit for
    bit, and the GEMM's own slab is bit-identical to the launch without a tail"""
    assert_tn_plan(c)
    gen = _gen(seed + S + groups + n)
    D, H = tn_operands(c, gen, device)
    rfull = torch.randint(-1000, 1001, (S, n + 4), generator=gen).float().to(device)
    rslab = rfull[:, :n]
    assert rslab.stride(0) == n + 4
    g, out = slab_buffer(c, device)
    g0, out0 = slab_buffer(c, device)
    rg = Guarded(groups * n, torch.float32, device)
    with toggled(**{t: 0 for t in c.off}):
        ops.gemm_tn(D, H, c.splits, out=out0)
        ops.gemm_tn_reduce(D, H, c.splits, out, rslab, groups, rg.view(groups, n))
    what = (tn_id(c), S, groups, n)
    assert rg.intact(), (what, "rout guard")
    assert torch.equal(rg.view(groups, n).double(), group_sums(rslab, groups)), (what, "group sums")
    assert torch.equal(g.raw, g0.raw), (what, "the slab differs from the launch without a tail")
    check_slab(g, out, tn_reference(D, H, c.splits), what)


# ---------------------------------------------------------------------------- refusals
# (what, M, N, K, lda, ldb, ldc, epi, aux, ldaux, code) for hpnn_gemm_nt_bf16
NT_REFUSED = [("M % 128", 192, 64, 64, 64, 64, 64, ops.EPI_NONE, False, 0, -2),
              ("N % 32", 128, 48, 64, 64, 64, 48, ops.EPI_NONE, False, 0, -2),
              ("K % 32", 128, 64, 48, 48, 48, 64, ops.EPI_NONE, False, 0, -2),
              ("lda % 8", 128, 64, 64, 68, 64, 64, ops.EPI_NONE, False, 0, -3),
              ("ldb % 8", 128, 64, 64, 64, 68, 64, ops.EPI_NONE, False, 0, -3),
              ("ldc % 8", 128, 64, 64, 64, 64, 68, ops.EPI_NONE, False, 0, -3),
              ("DACT without aux", 128, 64, 64, 64, 64, 64, ops.EPI_DACT, False, 0, -3),
              ("ldaux % 4", 128, 64, 64, 64, 64, 64, ops.EPI_DACT, True, 66, -3),
              ("M = 0", 0, 64, 64, 64, 64, 64, ops.EPI_NONE, False, 0, -1),
              ("N = 0", 128, 0, 64, 64, 64, 64, ops.EPI_NONE, False, 0, -1),
              ("K = 0", 128, 64, 0, 64, 64, 64, ops.EPI_NONE, False, 0, -1)]
# (what, N, M, Bt, splits, ldd, ldh, ldg, code) for hpnn_gemm_tn_bf16
TN_REFUSED = [("N % 32", 48, 64, 128, 1, 48, 64, 64, -2), ("M % 32", 64, 48, 128, 1, 64, 48, 48, -2),
              ("Bt % 64", 64, 96, 96, 1, 64, 96, 96, -2), ("splits > Bt / 64", 64, 96, 128, 3, 64, 96, 96, -2),
              ("ldg < M", 64, 96, 128, 1, 64, 96, 64, -3), ("ldg % 4", 64, 96, 128, 1, 64, 96, 98, -3),
              ("ldd % 8", 64, 96, 128, 1, 68, 96, 96, -3)]


def _strided(rows, cols, ld, dtype, device):
    """a [rows, cols] tensor of row stride ld (possibly below cols: the launcher must refuse before use)"""
    return torch.zeros(max(rows, 1) * max(ld, cols) + 8, dtype=dtype, device=device).as_strided((rows, cols), (ld, 1))


def check_nt_refused(device, row):
    """the plan reports the code; on a device the launch raises with it and writes nothing"""
    what, M, N, K, lda, ldb, ldc, epi, has_aux, ldaux, code = row
    assert ops.gemm_nt_plan(M, N, K, lda, ldb, ldc, epi, has_aux, ldaux) == (code, 0), what
    if device.type == "cpu":
        return  # the emulation applies to every shape
    import pytest
    A, B = _strided(M, K, lda, torch.bfloat16, device), _strided(N, K, ldb, torch.bfloat16, device)
    aux = _strided(M, N, ldaux, torch.bfloat16, device) if has_aux else None
    g = Guarded(max(M, 1) * max(ldc, N) + 8, torch.bfloat16, device)
    C = g.t.as_strided((M, N), (ldc, 1))
    with pytest.raises(RuntimeError, match="rc=%d" % code):
        ops.gemm_nt(A, B, epi, aux=aux, out_f32=False, out=C)
    assert g.untouched(), what


def check_tn_refused(device, row):
    what, N, M, Bt, splits, ldd, ldh, ldg, code = row
    assert ops.gemm_tn_plan(N, M, Bt, splits, ldd, ldh, ldg) == (code, 0), what
    if device.type == "cpu":
        return
    import pytest
    D, H = _strided(Bt, N, ldd, torch.bfloat16, device), _strided(Bt, M, ldh, torch.bfloat16, device)
    g = Guarded(splits * N * max(ldg, M) + 8, torch.float32, device)
    out = g.t.as_strided((splits, N, M), (N * ldg, ldg, 1))
    with pytest.raises(RuntimeError, match="rc=%d" % code):
        ops.gemm_tn(D, H, splits, out=out)
    assert g.untouched(), what


def check_tn_tail_refused(device):
    """device tensors only: rn % 4, groups > S, null pointers: -2, neither the slab nor rout written"""
    import pytest
    c = TAIL_LAUNCHES[0]
    D, H = tn_operands(c, _gen(62), device)
    for S, groups, n, null in [(4, 2, 6, None), (4, 5, 8, None), (4, 2, 8, "rslab"), (4, 2, 8, "rout")]:
        g, out = slab_buffer(c, device)
        rslab = torch.ones(S, n, device=device)
        rg = Guarded(groups * n, torch.float32, device)
        with pytest.raises(RuntimeError, match="rc=-2"):
            native().gemm_tn_bf16_reduce(D.data_ptr(), D.stride(0), H.data_ptr(), H.stride(0), out.data_ptr(),
                                         out.stride(1), c.N, c.M, c.Bt, c.splits,
                                         0 if null == "rslab" else rslab.data_ptr(), S, rslab.stride(0), n, groups,
                                         0 if null == "rout" else rg.t.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        assert g.untouched() and rg.untouched(), (S, groups, n, null)


# ---------------------------------------------------------------------------- cast_weights
CAST_SHAPES = [(32, 32), (96, 160), (128, 800)]
# FP32 bit patterns: -0.0, +0.0, FP32 and BF16 subnormals, BF16 rounding ties (to even down and up, and
# negative), just above / below a tie, the largest value that does not round to inf
CAST_BITS = [0x80000000, 0x00000000, 0x00000001, 0x00008000, 0x00018000, 0x007fffff, 0x80008000, 0x3f808000,
             0x3f818000, 0xbf808000, 0xbf818000, 0x3f808001, 0x3f817fff, 0x7f7f7fff]


def cast_input(N, K, gen):
    W = torch.randn(N, K, generator=gen)
    sp = torch.tensor([b - (1 << 32) if b >> 31 else b for b in CAST_BITS], dtype=torch.int64).to(torch.int32)
    flat = W.view(-1).view(torch.int32)
    flat[:sp.numel()] = sp
    flat[-sp.numel():] = sp
    idx = torch.randperm(N * K, generator=gen)[:4 * sp.numel()]
    flat[idx] = sp.repeat(4)
    return W


def _bit_diff(want, got):
    """the first differing bit patterns as (flat index, wanted, got) in hex"""
    w, g = want.reshape(-1).cpu(), got.reshape(-1).cpu()
    mask = (1 << (8 * w.element_size())) - 1
    return [(int(i), hex(int(w[i]) & mask), hex(int(g[i]) & mask)) for i in torch.nonzero(w != g).view(-1)[:8]]


def check_cast_weights(device, N, K, with_wf, seed=71):
    """Wbf == W32.bfloat16(), Wt == Wbf.t(), Wf == frag_major(Wbf), W32 bit-identical afterwards"""
    W = cast_input(N, K, _gen(seed + N + K)).to(device)
    W32 = Guarded(N * K, torch.float32, device)
    W32.view(N, K).copy_(W)
    before = W32.raw.clone()
    Wbf, Wt = Guarded(N * K, torch.bfloat16, device), Guarded(N * K, torch.bfloat16, device)
    Wf = Guarded(N * K, torch.bfloat16, device) if with_wf else None
    ops.cast_weights(W32.view(N, K), Wbf.view(N, K), Wt.view(K, N), Wf.t if with_wf else None)
    want = W.bfloat16()
    bits = torch.int16
    assert torch.equal(W32.raw, before), ("W32 changed", _bit_diff(before, W32.raw))
    assert torch.equal(Wbf.view(N, K).view(bits), want.view(bits)), ("Wbf", _bit_diff(want.view(bits), Wbf.view(N, K).view(bits)))
    assert torch.equal(Wt.view(K, N).view(bits), want.view(bits).t()), "Wt"
    assert Wbf.intact() and Wt.intact()
    if with_wf:
        assert torch.equal(Wf.t.view(bits), ops.frag_major(want).view(bits)), "Wf"
        assert Wf.intact()
    assert int((want.view(bits) == -32768).sum()) >= 2, "-0.0 must survive the cast"


# ---------------------------------------------------------------------------- reduce_slabs2
REDUCE_S = [1, 15, 16, 17, 63, 64, 65]  # 1 / 4 / 16 groups with tmp: S < 16, 16 <= S < 64, S >= 64
REDUCE_N = [4, 1020, 10240]


def check_reduce_slabs2(device, S, n, with_tmp, seed=81):
    gen = _gen(seed + S + n)
    full = torch.randint(-1000, 1001, (S, n + 4), generator=gen).float().to(device)
    slab = full[:, :n]
    out = Guarded(n, torch.float32, device)
    tmp = Guarded(16 * n, torch.float32, device) if with_tmp else None
    ops.reduce_slabs2(slab, out.t, tmp.t if with_tmp else None)
    assert torch.equal(out.t.double(), exact(slab.double().sum(0))), (S, n, with_tmp)
    assert out.intact() and (tmp is None or tmp.intact())


def check_reduce_slabs2_refused(device):
    """device tensors only: n % 4, stride % 4, S < 1 write nothing"""
    import pytest
    for S, n, stride in [(4, 6, 8), (4, 8, 10), (0, 8, 8)]:
        slab = torch.ones(max(S, 1) * stride + 8, device=device).as_strided((S, n), (stride, 1))
        out, tmp = Guarded(n, torch.float32, device), Guarded(16 * n, torch.float32, device)
        with pytest.raises(RuntimeError, match="rc=-2"):
            native().reduce_slabs2(slab.data_ptr(), S, stride, n, tmp.t.data_ptr(), out.t.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        assert out.untouched() and tmp.untouched(), (S, n, stride)


# ---------------------------------------------------------------------------- coverage
def coverage():
    """arm -> ids of the cases that reach it (as the case tables list them; the CPU test asserts that
    the dispatcher agrees)"""
    nt = {a: [] for a in ops.gemm_nt_arms()}
    for c in NT_CASES:
        nt[c.arm].append(nt_id(c))
    nt["ws"] = ["direct %dx%d, M in 32 x {1, CUs + 1, 4 CUs + 3}" % p for p in WS_PAIRS] + ["gemm_nt 16384x128x512"]
    tn = {a: [] for a in ops.gemm_tn_arms()}
    for c in TN_CASES:
        tn[c.arm].append(tn_id(c))
    return nt, tn
