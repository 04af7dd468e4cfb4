"""Every FP64 / FP32 engine kernel variant (csrc/gpu/kernels_fp.hip) at its edges, directly.

gemm_fp: every (ta, tb, epilogue, type) instantiation of the 64 x 64 and of the 128 x 128 kernel,
with operands inside larger buffers (lda / ldb / ldc / ldaux beyond the logical width) whose
padding is NaN: an over-read turns the result into NaN, and the padding of C, the rows beyond
M and the slabs beyond the returned count must come back bit-identical.  Every case runs with
integer operands (exact: torch.equal against an int64 matmul) and with random operands against
a float64 CPU reference under the element-wise bounds of tests/fp_ref.py (checked on their own
in test_fp_ref_cpu.py).

output_fp / output_fp_eval: O, D, guess, hits and the LOSS, padded strides, argmax ties,
softmax extremes.  update_fp / reduce_fp / dact_fp: slab strides, in-place calls, the
grid-stride loop, error returns."""
import functools
import os

import pytest
import torch

from hpnn_amd import capi
from hpnn_amd._lib import native
from tests.fp_ref import (U, dbip, first_argmax, gemm_bound, gemm_none_bound, gemm_ref, int_operands, output_ref,
                          update_ref)

pytestmark = pytest.mark.gpu

DTS = [torch.float64, torch.float32]
ITY = {torch.float64: torch.int64, torch.float32: torch.int32}
# quiet NaNs with distinct payloads: operand padding (an over-read) and output sentinels (a
# stray store) stay distinguishable from each other and from a computed NaN
PAD_BITS = {torch.float64: 0x7FF8000000000A11, torch.float32: 0x7FC00A11}
SENT_BITS = {torch.float64: 0x7FF8000000000BAD, torch.float32: 0x7FC00BAD}
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
VARIANTS = [(ta, tb, epi) for epi in (0, 1, 2) for ta, tb in LAYOUTS]
FORMS = ["vec", "odd_ld", "offset"]
big_kernel = pytest.mark.skipif(os.environ.get("HPNN_FP_BIG", "")[:1] == "0",
                                reason="HPNN_FP_BIG=0 disables the 128 x 128 kernel")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _filled(n, dt, bits):
    return torch.full((n,), bits[dt], dtype=ITY[dt], device="cuda").view(dt)


def _same_bits(x, y):
    return torch.equal(x.view(ITY[x.dtype]), y.view(ITY[y.dtype]))


def _embed(R, W, dt, bits, form="offset", slabs=1, x=None):
    """slabs logical [R x W] matrices inside one larger buffer filled with the NaN `bits`:
    returns (whole buffer, [slabs x R x W] view of the logical parts, ld, slab stride).
    form "vec": 16-byte aligned base, ld a multiple of 16 bytes; "odd_ld": an odd ld;
    "offset": the aligned ld with the base one element further."""
    ld = (W + 4) // 4 * 4 + 4
    off = 16
    if form == "odd_ld":
        ld += 1
    elif form == "offset":
        off += 1
    stride = (R + 2) * ld + 3
    flat = _filled(off + slabs * stride + 5, dt, bits)
    view = flat.as_strided((slabs, R, W), (stride, ld, 1), off)
    if x is not None:
        view[0] = x.to(dt)
    aligned = view.data_ptr() % 16 == 0 and (ld * flat.element_size()) % 16 == 0
    assert aligned == (form == "vec") and ld > W
    return flat, view, ld, stride


# ---- gemm_fp --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _operands(M, N, K, dt, kind):
    """logical a [M x K], b [K x N], aux [M x N] as float64 (values representable in dt), the
    float64 accumulator a . b and its bound (zero for the exact integer operands)"""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    aux = (torch.rand(M, N, generator=g, dtype=torch.float64) * 1.8 - 0.9).to(dt).double()
    if kind == "int":
        a, b, acc = int_operands(M, N, K, M + N + K)
        # every partial sum is an integer of magnitude <= 9 K: exact in either type
        assert a.abs().max() <= 3 and b.abs().max() <= 3 and 9 * K <= (2 ** 53 if dt == torch.float64 else 2 ** 24)
        return a.double(), b.double(), aux, acc.double(), torch.zeros(M, N, dtype=torch.float64)
    a = torch.randn(M, K, generator=g, dtype=torch.float64).to(dt).double()
    b = (torch.randn(K, N, generator=g, dtype=torch.float64) + torch.arange(N)[None, :] * 0.01).to(dt).double()
    return a, b, aux, a @ b, gemm_none_bound(a, b, U[dt])


@functools.lru_cache(maxsize=4)
def _expected(M, N, K, dt, kind, epi):
    """(reference, bound) of one epilogue, on the GPU"""
    a, b, aux, acc, nb = _operands(M, N, K, dt, kind)
    ref = gemm_ref(epi, acc, aux)
    return ref.cuda(), gemm_bound(epi, nb, ref, aux, U[dt]).cuda()


def _kchunk(K, splits):
    return ((K + splits - 1) // splits + 15) // 16 * 16


def _launch(dt, M, N, K, ta, tb, epi, splits, kind, form):
    """one gemm_fp call on padded NaN-guarded buffers: (slab count, [S x M x N] result)"""
    a, b, aux, _, _ = _operands(M, N, K, dt, kind)
    A = a.t() if ta else a
    Bm = b if tb else b.t()
    _, va, lda, _ = _embed(A.shape[0], A.shape[1], dt, PAD_BITS, form, x=A)
    _, vb, ldb, _ = _embed(Bm.shape[0], Bm.shape[1], dt, PAD_BITS, form, x=Bm)
    _, vx, ldx, _ = _embed(M, N, dt, PAD_BITS, form, x=aux)
    fc, vc, ldc, sst = _embed(M, N, dt, SENT_BITS, form, slabs=splits)
    before = fc.clone()
    S = native().gemm_fp(int(dt == torch.float64), va.data_ptr(), lda, ta, vb.data_ptr(), ldb, tb, vc.data_ptr(), ldc,
                         vx.data_ptr() if epi == 2 else 0, ldx, M, N, K, epi, splits, sst, _stream())
    torch.cuda.synchronize()
    assert 1 <= S <= splits
    got = vc[:S].clone()
    # the padding of C, the rows beyond M and the slabs beyond S: put the sentinel back into
    # the S logical regions and the whole buffer must be what it was, bit for bit
    vc[:S] = before.as_strided(vc.shape, vc.stride(), vc.storage_offset())[:S]
    assert _same_bits(fc, before), "gemm_fp stored outside the logical C of its slabs"
    assert not got.isnan().any(), "NaN in C: an operand or aux was read outside its logical region, or C left unwritten"
    return S, got


def _check_gemm(dt, M, N, K, ta, tb, epi, splits, big, form="offset"):
    assert epi == 0 or splits == 1
    for kind in ("int", "rand"):
        S, got = _launch(dt, M, N, K, ta, tb, epi, splits, kind, form)
        kc = _kchunk(K, splits)
        assert S == (K + kc - 1) // kc == capi.lib().hpnn_gemm_fp_splits(K, splits)
        # the documented rule: 128 x 128 tiles once they, times the slabs, fill 256 workgroups
        assert (((M + 127) // 128) * ((N + 127) // 128) * S >= 256) == big
        ref, bound = _expected(M, N, K, dt, kind, epi)
        tot = got.double().sum(0)
        if kind == "int" and epi == 0:
            assert torch.equal(got.sum(0), ref.to(dt)) and torch.equal(tot, ref)
            a, b = _operands(M, N, K, dt, kind)[:2]
            for s in range(S):  # and every slab is its own k-chunk
                assert torch.equal(got[s].double().cpu(), a[:, s * kc:(s + 1) * kc] @ b[s * kc:(s + 1) * kc]), s
        err = (tot - ref).abs()
        bad = err > bound
        assert not bad.any(), (kind, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
        if form != "vec" and big:  # scalar loads give the bits of the 16-byte vector loads
            Sv, gv = _launch(dt, M, N, K, ta, tb, epi, splits, kind, "vec")
            assert Sv == S and _same_bits(got, gv)


SMALL_SHAPES = [(65, 63, 17), (1, 1, 1), (1, 130, 16), (130, 1, 33), (64, 64, 16), (40, 90, 1000)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ta,tb,epi", VARIANTS)
@pytest.mark.parametrize("M,N,K", SMALL_SHAPES)
def test_gemm_fp_small_kernel(gpu, M, N, K, ta, tb, epi, dt):
    """gemm_fp_kernel (64 x 64 tiles): all 12 variants at one tile plus one row / column, a
    single element, one row, one column, an exact tile, a long K"""
    _check_gemm(dt, M, N, K, ta, tb, epi, 1, big=False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("K,splits,slabs", [(100, 3, 3), (100, 50, 7), (1, 5, 1), (48, 3, 3)])
def test_gemm_fp_small_kernel_split_k(gpu, K, splits, slabs, ta, tb, dt):
    """split-K of the 64 x 64 kernel: a ragged last chunk, more splits than 16-wide chunks
    (fewer slabs returned, the others untouched), K = 1, exact chunks"""
    M, N = 65, 63
    assert (K + _kchunk(K, splits) - 1) // _kchunk(K, splits) == slabs
    _check_gemm(dt, M, N, K, ta, tb, 0, splits, big=False)


@big_kernel
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_fp_big_kernel_split_k(gpu, ta, tb, form, dt):
    """gemm_fp_big_kernel (128 x 128 tiles) reached through the splits: 4 tiles x 65 slabs of
    one 16-wide stage, the last with 5 k; 16-byte vector loads with scalar edge chunks, and
    the scalar loads of an odd ld and of an unaligned base (same bits)"""
    _check_gemm(dt, 130, 130, 1029, ta, tb, 0, 65, big=True, form=form)


@big_kernel
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ta,tb,epi", VARIANTS)
def test_gemm_fp_big_kernel(gpu, ta, tb, epi, form, dt):
    """gemm_fp_big_kernel, all 12 variants: 16 x 16 tiles with ragged edges on both axes,
    K = 2 stages + 5; both load paths"""
    _check_gemm(dt, 1925, 1930, 37, ta, tb, epi, 1, big=True, form=form)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,splits,big", [(65, 63, 100, 3, False),
                                              pytest.param(130, 130, 1029, 65, True, marks=big_kernel)])
def test_gemm_fp_is_deterministic(gpu, M, N, K, splits, big, dt):
    S0, g0 = _launch(dt, M, N, K, 1, 1, 0, splits, "rand", "vec")
    S1, g1 = _launch(dt, M, N, K, 1, 1, 0, splits, "rand", "vec")
    assert (((M + 127) // 128) * ((N + 127) // 128) * S0 >= 256) == big
    assert S0 == S1 and _same_bits(g0, g1)


# ---- output_fp / output_fp_eval -------------------------------------------------------------

OUT_B = 333
# largest |O - o|, |D - d| of the f32 kernel against the float64 reference over all cases of
# test_output_fp below, measured on an MI355X: 4.768e-07 (= 8 * 2^-24: the linear delta t - z at
# |z| ~ 12; bipolar 3.49e-07, softmax 1.94e-07); the tolerance is 4 x that (exp / log differ by
# an ulp between shapes) and never beyond 64 * 2^-24
OUT_TOL = {torch.float64: 1e-14, torch.float32: 4 * 4.768e-07}
assert OUT_TOL[torch.float32] <= 64 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _output_case(dt, n_out, net):
    """Z, T (float64 values representable in dt) with planted argmax ties and, for the softmax,
    extreme rows; all planted rows lie below every non-zero n_valid"""
    g = torch.Generator().manual_seed(100 * n_out + net)
    B, lo = OUT_B, (0.0 if net == 2 else -1.0)
    z = (torch.randn(B, n_out, generator=g, dtype=torch.float64) * 3).to(dt).double()
    t = torch.full((B, n_out), lo, dtype=torch.float64)
    t[torch.arange(B), torch.randint(0, n_out, (B,), generator=g)] = 1.0

    def plant(row, zcols, tcols):
        z[row, zcols] = 20.0
        t[row] = lo
        t[row, tcols] = 1.0

    if n_out > 67:  # equal maxima in different lanes and different iterations of the c += 64 loop
        plant(0, [3, 67], [3])      # output tie: guess 3, a hit
        plant(1, [3], [3, 67])      # target tie: target 3, a hit
        plant(2, [67], [3, 67])     # target 3, guess 67: no hit
    if n_out > 6:   # equal maxima in neighbouring lanes
        plant(3, [5, 6], [5])       # guess 5, a hit
        plant(4, [5, 6], [6])       # guess 5: no hit
        plant(5, [6], [5, 6])       # target 5, guess 6: no hit
    if net == 2:
        big = 700.0 if dt == torch.float64 else 80.0
        r = torch.rand(n_out, generator=g, dtype=torch.float64)
        z[6] = torch.where(torch.arange(n_out) % 2 == 0, big - r, -big + r).to(dt).double()
        z[7] = -big  # all equal at the far end: TINY e^{1 - zmax} dominates the denominator
        z[8] = 0.5   # all equal: the first index wins
        for row in (6, 7, 8):
            # target on the (first) maximum: a target on an output that underflows to 0 in dt
            # but not in float64 would make the reference's `if (o > 0)` differ by type
            t[row] = lo
            t[row, first_argmax(z[row:row + 1])] = 1.0
    return z, t


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("net", [0, 1, 2])
@pytest.mark.parametrize("n_out", [1, 37, 64, 65, 230])
@pytest.mark.parametrize("n_valid", [0, 328, 333])
def test_output_fp(gpu, n_valid, n_out, net, dt):
    B, u, tol = OUT_B, U[dt], OUT_TOL[dt]
    z, t = _output_case(dt, n_out, net)
    o, d, loss = output_ref(z, t, net, n_valid)
    guess_ref = first_argmax(o)
    hits_ref = int((guess_ref == first_argmax(t))[:n_valid].sum())
    assert o.isfinite().all() and d.isfinite().all() and loss.isfinite().all()
    _, vz, ldz, _ = _embed(B, n_out, dt, PAD_BITS, x=z)
    _, vt, ldt, _ = _embed(B, n_out, dt, PAD_BITS, "odd_ld", x=t)
    fd, vd, ldd, _ = _embed(B, n_out, dt, SENT_BITS)
    fo, vo, ldo, _ = _embed(B, n_out, dt, SENT_BITS, "odd_ld")
    fd0, fo0 = fd.clone(), fo.clone()
    guess = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    stats = torch.zeros(64, 16, device="cuda")
    f64 = int(dt == torch.float64)
    native().output_fp(f64, vz.data_ptr(), ldz, vt.data_ptr(), ldt, vd.data_ptr(), ldd, vo.data_ptr(), ldo,
                       guess.data_ptr(), stats.data_ptr(), stats[0, 1:].data_ptr(), B, n_valid, n_out, net, _stream())
    torch.cuda.synchronize()
    O, D = vo[0].double().cpu(), vd[0].double().cpu()
    vo[0], vd[0] = fo0.as_strided(vo.shape, vo.stride(), vo.storage_offset())[0], \
        fd0.as_strided(vd.shape, vd.stride(), vd.storage_offset())[0]
    assert _same_bits(fo, fo0) and _same_bits(fd, fd0), "store outside the logical O / D"
    assert O.isfinite().all() and D.isfinite().all()
    eo, ed = (O - o).abs().max().item(), (D - d).abs().max().item()
    print(f"output_fp {dt} net {net} n_out {n_out} n_valid {n_valid}: max|O-o| {eo:.3e} max|D-d| {ed:.3e}")
    assert eo <= tol and ed <= tol
    assert torch.count_nonzero(D[n_valid:]) == 0
    assert torch.equal(guess[:B].long().cpu(), guess_ref) and guess[B] == -7
    st = stats.cpu()
    assert int(st[:, 1].contiguous().view(torch.int32).sum()) == hits_ref
    assert torch.count_nonzero(st[:, 2:]) == 0
    # the float path adds float(l_row) into float slots
    el = abs(st[:, 0].double().sum().item() - loss.sum().item())
    print(f"  loss {loss.sum().item():.9e} float-slot error {el:.3e}")
    assert el <= B * 2.0 ** -24 * loss.abs().sum().item()

    # the forward-only form: hits at word 1, the loss as a double at floats 2..3, word 0 untouched
    slots = torch.zeros(64, 16, device="cuda")
    guess2 = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    native().output_fp_eval(f64, vz.data_ptr(), ldz, vt.data_ptr(), ldt, guess2.data_ptr(), slots.data_ptr(), B,
                            n_valid, n_out, net, _stream())
    torch.cuda.synchronize()
    sl = slots.cpu()
    assert torch.equal(guess2, guess)
    assert torch.count_nonzero(sl[:, 0].contiguous().view(torch.int32)) == 0
    assert torch.equal(sl[:, 1].contiguous().view(torch.int32), st[:, 1].contiguous().view(torch.int32))
    assert torch.count_nonzero(sl[:, 4:]) == 0
    el = abs(sl.view(torch.float64)[:, 1].sum().item() - loss.sum().item())
    print(f"  double-slot error {el:.3e}")
    assert el <= B * u * loss.abs().sum().item()


def test_output_fp_eval_rejects_missing_arguments(gpu):
    x = torch.zeros(64, 16, device="cuda")
    p = x.data_ptr()
    # (Z, ldz, T, ldt, guess, slots, B, n_valid, n_out, type): no T, no slots, B = 0
    for args in [(p, 4, 0, 4, 0, p, 4, 4, 4, 2), (p, 4, p, 4, 0, 0, 4, 4, 4, 2), (p, 4, p, 4, 0, p, 0, 0, 4, 2)]:
        with pytest.raises(RuntimeError):
            native().output_fp_eval(0, *args, _stream())
    torch.cuda.synchronize()
    assert torch.count_nonzero(x) == 0


# ---- update_fp / reduce_fp / dact_fp --------------------------------------------------------

NS = [1, 255, 257, 4096 * 256 + 257]  # the last: more than the 4096-workgroup grid covers at once
SLABS = [(1, True), (3, True), (1, False)]  # (S, gstride > n with NaN between the slabs | gstride = 0)


def _slabs(vals, dt, gapped):
    """[S x n] values as slabs gstride apart: (buffer, [S x n] view, gstride)"""
    S, n = vals.shape
    gstride = n + 13 if gapped else 0
    flat = _filled(S * (n + 13) + 3, dt, PAD_BITS)
    view = flat.as_strided((S, n), (n + 13, 1), 0)
    view.copy_(vals.to(dt))
    return flat, view, gstride


def _guarded(vals, dt):
    """n values followed by sentinels: (buffer, [n] view)"""
    flat = _filled(vals.numel() + 9, dt, SENT_BITS)
    flat[:vals.numel()] = vals.to(dt)
    return flat, flat[:vals.numel()]


def _tail_kept(flat, n, dt):
    return _same_bits(flat[n:], _filled(flat.numel() - n, dt, SENT_BITS))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("momentum", [0, 1])
@pytest.mark.parametrize("S,gapped", SLABS)
@pytest.mark.parametrize("n", NS)
def test_update_fp(gpu, n, S, gapped, momentum, dt):
    g = torch.Generator().manual_seed(n + S)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dt).double()
    G, w, v = r(S, n), r(n), r(n)
    # lr, alpha, scale exactly representable in float: the f32 kernel takes them as floats
    lr, alpha, scale = float(torch.tensor(0.05, dtype=torch.float32)), 0.25, 1.0 / 128
    fg, vg, gstride = _slabs(G, dt, gapped)
    fw, vw = _guarded(w, dt)
    fv, vv = _guarded(v, dt)
    fg0 = fg.clone()
    native().update_fp(int(dt == torch.float64), vw.data_ptr(), vv.data_ptr() if momentum else 0, vg.data_ptr(), S,
                       gstride, n, lr, alpha, scale, momentum, _stream())
    torch.cuda.synchronize()
    wr, vr, mag = update_ref(w, v, G, lr, alpha, scale, momentum)
    bound = (S + 4) * U[dt] * mag
    assert ((vw.double().cpu() - wr).abs() <= bound).all()
    if momentum:
        assert ((vv.double().cpu() - vr).abs() <= bound).all()
    else:
        assert torch.equal(vv.double().cpu(), v)
    assert _tail_kept(fw, n, dt) and _tail_kept(fv, n, dt) and _same_bits(fg, fg0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("S,gapped", SLABS)
@pytest.mark.parametrize("n", NS)
def test_reduce_fp(gpu, n, S, gapped, inplace, dt):
    """integer slabs sum exactly; in place: out is slab 0, as the data-parallel engine calls it"""
    g = torch.Generator().manual_seed(n + S)
    G = torch.randint(-1000, 1001, (S, n), generator=g)
    fg, vg, gstride = _slabs(G.double(), dt, gapped)
    fg0 = fg.clone()
    fo, vo = _guarded(torch.zeros(n), dt)
    out = vg if inplace else vo
    native().reduce_fp(int(dt == torch.float64), out.data_ptr(), vg.data_ptr(), S, gstride, n, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(-1)[:n].cpu(), G.sum(0).to(dt))
    if inplace:
        vg[0] = fg0[:n]
    assert _same_bits(fg, fg0) and _tail_kept(fo, n, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("n", NS)
def test_dact_fp(gpu, n, inplace, dt):
    """out = in * f'(aux), in place as the tensor-parallel engine calls it.  |aux| <= 0.7: there
    the rounding of aux^2 (<= u aux^2 / (1 - aux^2) <= 0.96 u of f'), of the subtraction and of
    the product stay under 4 u |ref| whether or not the compiler fuses aux * aux - 1"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g, dtype=torch.float64).to(dt).double()
    aux = (torch.rand(n, generator=g, dtype=torch.float64) * 1.4 - 0.7).to(dt).double()
    fx, vx = _guarded(x, dt)
    fa, va = _guarded(aux, dt)
    fo, vo = _guarded(torch.zeros(n), dt)
    out = vx if inplace else vo
    native().dact_fp(int(dt == torch.float64), out.data_ptr(), vx.data_ptr(), va.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    ref = x * dbip(aux)
    assert ((out.double().cpu() - ref).abs() <= 4 * U[dt] * ref.abs()).all()
    assert _tail_kept(fx, n, dt) and _tail_kept(fa, n, dt) and _tail_kept(fo, n, dt)
    assert torch.equal(va.double().cpu(), aux) and (inplace or torch.equal(vx.double().cpu(), x))


@pytest.mark.parametrize("dt", DTS)
def test_fp_elementwise_error_returns(gpu, dt):
    f64, s = int(dt == torch.float64), _stream()
    x = torch.zeros(64, dtype=dt, device="cuda")
    p = x.data_ptr()
    with pytest.raises(RuntimeError):
        native().update_fp(f64, p, p, p, 1, 0, 0, 0.1, 0.2, 1.0, 1, s)   # n = 0
    with pytest.raises(RuntimeError):
        native().update_fp(f64, p, p, p, 0, 0, 8, 0.1, 0.2, 1.0, 1, s)   # S = 0
    with pytest.raises(RuntimeError):
        native().update_fp(f64, p, 0, p, 1, 0, 8, 0.1, 0.2, 1.0, 1, s)   # momentum without V
    with pytest.raises(RuntimeError):
        native().reduce_fp(f64, p, p, 1, 0, 0, s)
    with pytest.raises(RuntimeError):
        native().reduce_fp(f64, p, p, 0, 0, 8, s)
    with pytest.raises(RuntimeError):
        native().dact_fp(f64, p, p, p, 0, s)
    torch.cuda.synchronize()
    assert torch.count_nonzero(x) == 0
