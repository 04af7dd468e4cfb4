"""[clip] on the GPU: the kernels of csrc/gpu/kernels_clip.hip bit for bit against the host entry
points of include/libhpnn/clip.h, the integer-exact sets and the finalize's edges on the device,
the refusals, the four update kernels with a clip state, the factor read from device memory inside
a captured graph, the whole BF16 plan on the integer-exact fixture, the f64 / f32 engines against
the FP64 CPU oracle, train_nn -d bf16 -C against the Python plan, exact resume, [keep_best], and an
unclipped plan untouched.

Every case prints what it measured."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from hpnn_amd import capi, ops
from hpnn_amd.models import MLP
from hpnn_amd.utils import formats
from tests import adam_common as A
from tests import clip_common as Q
from tests import front_exact_common as fc
from tests import lrsched_common as K
from tests import upd_common as U

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
NAN = float("nan")


def _windows(slabs, goff):
    """every [S, n] slab inside a NaN-filled buffer (rows n + 3 apart, goff elements from the
    start); returns the CPU windows, their buffers and the device copies of both"""
    cpu, bases, dev, dbases = [], [], [], []
    for sl in slabs:
        base, win = U.slab_window(sl, goff)
        d, db = U.to_cuda(dict(slab=win), dict(slab=base))
        cpu.append(win), bases.append(base), dev.append(d["slab"]), dbases.append(db["slab"])
    return cpu, bases, dev, dbases


def _run_partials(slabs, goff, interleaved, scale, max_norm=0.5, extra=3):
    """gnorm_partials + clip_finalize on the device against the host entry points: every bit of
    the partials and of the state, partials[count ..] and the slabs' buffers untouched"""
    cpu, bases, dev, dbases = _windows(slabs, goff)
    th, td = ops.GnormTable(cpu, interleaved=interleaved), ops.GnormTable(dev, interleaved=interleaved)
    assert td.count == th.count and td.first == th.first
    ph = torch.full((th.count + extra,), NAN, dtype=torch.float64)
    pd = ph.clone().cuda()
    sh = ops.clip_state(max_norm)
    sd = sh.clone().cuda()
    ops.gnorm_partials(th, ph, scale), ops.clip_finalize(ph, th.count, sh)
    ops.gnorm_partials(td, pd, scale), ops.clip_finalize(pd, td.count, sd)
    torch.cuda.synchronize()
    who = f"n {[s.shape[1] for s in slabs]} S {slabs[0].shape[0]} goff {goff} {slabs[0].dtype} 8-way {interleaved}"
    assert torch.equal(U.ibits(pd.cpu()), U.ibits(ph)), who  # the NaN tail included: untouched
    assert torch.equal(U.ibits(sd.cpu()), U.ibits(sh)), who
    for b, db in zip(bases, dbases):
        assert torch.equal(U.ibits(db.cpu()), U.ibits(b)), f"{who}: the slabs are read only"
    return ops.read_clip_state(sd), ph[:th.count]


# ------------------------------------------------------------------ 1. partials + finalize
@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True], ids=["sequential", "8-way"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_partials_and_finalize_equal_the_host_form(gpu, dtype, interleaved):
    # goff 0: the slabs on a 16-byte boundary; 1: one element off it (element by element).  Rows are
    # n + 3 apart: a stride that keeps the 16-byte alignment for some n (1025 in float, 1023 in
    # double) and breaks it for the others
    cases = [([n], S, goff) for n in Q.SIZES for S in Q.SLABS for goff in (0, 1)]
    cases += [([4099, 3, 5], 2, 1), ([4099, 3, 5], 9, 0), ([5, 1025, 1], 17, 0)]  # three segments in one table
    for i, (sizes, S, goff) in enumerate(cases):
        _run_partials([Q.random_slabs(n, S, dtype, 300 + 5 * i + k) for k, n in enumerate(sizes)], goff, interleaved,
                      1.0 / 7)
    # contiguous slabs (row stride n): the 16-byte loads with S > 1
    for n, S in ((1024, 3), (4100, 9)):
        sl = Q.random_slabs(n, S, dtype, n + S)
        h, d = ops.GnormTable([sl], interleaved=interleaved), ops.GnormTable([sl.cuda()], interleaved=interleaved)
        ph, pd = torch.zeros(h.count, dtype=torch.float64), torch.zeros(h.count, dtype=torch.float64, device="cuda")
        ops.gnorm_partials(h, ph, 0.5), ops.gnorm_partials(d, pd, 0.5)
        assert torch.equal(U.ibits(pd.cpu()), U.ibits(ph)), (n, S)
    print(f"gnorm_partials + finalize {dtype} 8-way {interleaved}: {len(cases) + 2} cases bit-equal to the host form")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_more_than_256_partials(gpu, dtype):
    """n = 256 * 1024 + 5: 257 partials, the finalize's strided loop"""
    r, p = _run_partials([Q.random_slabs(256 * 1024 + 5, 2, dtype, 8)], 1, False, 0.25)
    assert p.numel() == 257 and r["clipped"] == 1 and abs(float(p.sum()) - r["sumsq"]) <= 1e-12 * r["sumsq"]
    print(f"{dtype}: 257 partials, sumsq {r['sumsq']:.17g}, numpy-order sum {float(p.sum()):.17g}")


# ------------------------------------------------------------------ 2. integers and the finalize's edges
@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True], ids=["sequential", "8-way"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_gradients_are_exact_on_the_device(gpu, dtype, interleaved):
    for n, S, j in ((4099, 1, 20), (4099, 9, 8), (1025, 17, 3), (3 * 1024, 2, 30)):
        sl, sumsq = Q.integer_set(n, S, j, dtype, 11 + S)
        for max_norm, factor, clipped in ((2.5 * j, 0.5, 1), (5.0 * j, 1.0, 0), (10.0 * j, 1.0, 0)):
            r, p = _run_partials([sl * 2], 0, interleaved, 0.5, max_norm=max_norm)
            assert sum(int(x) for x in p.tolist()) == sumsq
            assert (r["sumsq"], r["norm"], r["factor"], r["clipped"], r["steps"]) == \
                (float(sumsq), 5.0 * j, factor, clipped, 1), (n, S, j, max_norm, r)
    print(f"integer sets {dtype} 8-way {interleaved}: the device's sums of squares equal Python's integers")


@pytest.mark.gpu
def test_finalize_edges_on_the_device(gpu):
    x = math.nextafter(3.0, math.inf)
    seq = [9.0, x * x, 0.0, math.inf, 16.0, math.nan, 1.0]
    sd, sh = ops.clip_state(3.0).cuda(), ops.clip_state(3.0)
    ref = Q.Clip(3.0)
    want = [(3.0, 1.0), (x, 3.0 / x), (0.0, 1.0), (math.inf, 0.0), (4.0, 0.75), (math.nan, 1.0), (1.0, 1.0)]
    for sumsq, (norm, factor) in zip(seq, want):
        p = torch.tensor([sumsq], dtype=torch.float64)
        ops.clip_finalize(p.cuda(), 1, sd), ops.clip_finalize(p, 1, sh)
        ref.finalize(sumsq)
        r = ops.read_clip_state(sd)
        assert torch.equal(U.ibits(sd.cpu()), U.ibits(sh)) and Q.same_state(r, ref.as_dict()), sumsq
        assert K.bits(r["norm"]) == K.bits(norm) and r["factor"] == factor, (sumsq, r)
    r = ops.read_clip_state(sd)
    assert (r["steps"], r["clipped"], r["norm_max"], r["norm_last"]) == (7, 3, math.inf, 1.0)
    # a NaN never enters norm_max
    s2 = ops.clip_state(3.0).cuda()
    for sumsq in (16.0, math.nan):
        ops.clip_finalize(torch.tensor([sumsq], dtype=torch.float64, device="cuda"), 1, s2)
    r = ops.read_clip_state(s2)
    assert r["norm_max"] == 4.0 and math.isnan(r["norm_last"]) and (r["steps"], r["clipped"]) == (2, 1)


# ------------------------------------------------------------------ 3. refusals
@pytest.mark.gpu
def test_table_and_launch_refusals_write_nothing(gpu):
    nat = ops.native()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.ones(2, 16, device="cuda")
    g64 = torch.ones(2, 16, dtype=torch.float64, device="cuda")
    ops.GnormTable([g])
    with pytest.raises(ValueError):
        ops.GnormTable([g] * 17)
    tb = torch.full((17, 4), -7, dtype=torch.int64, device="cuda")
    row = (g.data_ptr(), 2, 16, 16)  # (g, S, gstride, n)
    assert nat.gnorm_table(0, tb.data_ptr(), [row] * 17, s)[0] == -1           # 17 segments
    assert nat.gnorm_table(0, tb.data_ptr(), [(0,) + row[1:]], s)[0] == -1      # a null pointer
    assert nat.gnorm_table(1, tb.data_ptr(), [(g64.data_ptr() + 4, 2, 16, 16)], s)[0] == -1  # a misaligned double
    assert nat.gnorm_table(0, tb.data_ptr(), [(row[0], 2, 8, 16)], s)[0] == -1  # overlapping slabs
    assert nat.gnorm_table(0, tb.data_ptr(), [row[:3] + (0,)], s)[0] == -1      # n = 0
    assert nat.gnorm_table(0, tb.data_ptr(), [(row[0], 0, 16, 16)], s)[0] == -1  # S = 0
    assert nat.gnorm_table(0, 0, [row], s)[0] == -1                             # no table
    torch.cuda.synchronize()
    assert bool((tb == -7).all()), "a refused table wrote something"
    ok, count = nat.gnorm_table(0, tb.data_ptr(), [row], s)
    assert (ok, count) == (0, 1)
    part = torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
    st = ops.clip_state(1.0).cuda()
    st0 = st.clone()
    assert nat.gnorm_partials(0, 0, tb.data_ptr(), 17, 1, 1.0, part.data_ptr(), s) == -1
    assert nat.gnorm_partials(0, 0, tb.data_ptr(), 1, 0, 1.0, part.data_ptr(), s) == -1
    assert nat.gnorm_partials(0, 0, 0, 1, 1, 1.0, part.data_ptr(), s) == -1
    assert nat.gnorm_partials(0, 0, tb.data_ptr(), 1, 1, 1.0, 0, s) == -1
    assert nat.gnorm_partials(0, 0, tb.data_ptr(), 1, 1, 1.0, part.data_ptr() + 4, s) == -1
    assert nat.clip_finalize(part.data_ptr(), 1, 0, s) == -1                    # a null state
    assert nat.clip_finalize(part.data_ptr(), 1, st.data_ptr() + 4, s) == -1    # a misaligned state
    assert nat.clip_finalize(0, 1, st.data_ptr(), s) == -1
    assert nat.clip_finalize(part.data_ptr(), 0, st.data_ptr(), s) == -1
    assert nat.clip_commit(0, 0, 0, 0, s) == -1
    assert nat.clip_commit(st.data_ptr(), part.data_ptr(), 0, 4, s) == -1       # a history without a cursor
    # the update launches refuse a misaligned clip state
    w = torch.ones(16, device="cuda")
    tab = ops.SgdSchedTable([dict(w=w, slab=g)])
    lrs = ops.lr_state("constant", lr0=0.5).cuda()
    assert nat.sgd_sched_fp_clip(0, tab.dev.data_ptr(), 1, 1.0, 0.0, 0, lrs.data_ptr(), st.data_ptr() + 4, s) == -1
    torch.cuda.synchronize()
    assert bool((part == -3.0).all()) and torch.equal(U.ibits(st.cpu()), U.ibits(st0.cpu())) and bool((w == 1).all())


# ------------------------------------------------------------------ 4. the update kernels with a clip state
def _clip(factor, device="cpu"):
    return ops.write_clip_state(ops.clip_state(1.0), factor=factor).to(device)


def _walker_case(n, S, off, goff, dtype, seed, adam):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    sl = Q.random_slabs(n, S, dtype, seed + 1)
    keys = ("m", "v") if adam else ("v",)
    state = {k: (0.01 * torch.rand(n, generator=g, dtype=torch.float64)).to(dtype) for k in keys}
    if n > 3:
        sl[:, :3] = 0.0
        for k in keys:
            state[k][:3] = 0.0
    seg, bases = {}, {}
    bases["slab"], seg["slab"] = U.slab_window(sl, goff)
    for k, t in [("w", w)] + list(state.items()):
        bases[k], seg[k] = U.window(t, off)
    return seg, bases


def _rule_state(adam):
    """an advanced Adam state, or a schedule state one epoch in"""
    if adam:
        return ops.adam_advance(ops.adam_state(lr=0.01))
    return ops.lr_advance(ops.lr_state("step", lr0=0.3, gamma=0.9, period=1))


def _walk(segs, st, clip, adam, scale):
    if adam:
        ops.adam_update_fp(ops.AdamTable(segs), st, scale=scale, clip=clip)
    else:
        ops.sgd_sched_fp(ops.SgdSchedTable(segs, momentum=True), st, scale=scale, alpha=0.25, clip=clip)


@pytest.mark.gpu
@pytest.mark.parametrize("adam", [False, True], ids=["sched", "adam"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_walker_with_a_clip_state(gpu, dtype, adam):
    """hpnn_sgd_sched_fp / hpnn_adam_fp: bit-equal to the host entry point at a factor that is no
    power of two; at factor 0.5 bit-equal to an unclipped launch on slabs halved beforehand; with
    clip=None bit-equal to today's entry point; g = 0 rows keep w's bits"""
    st = _rule_state(adam)
    keys = ("w", "m", "v") if adam else ("w", "v")
    cases = [(n, S, off, goff) for n in (1, 3, 5, 4099) for S in (1, 3) for off, goff in ((0, 0), (1, 1), (0, 1))]
    for i, (n, S, off, goff) in enumerate(cases):
        seg, bases = _walker_case(n, S, off, goff, dtype, 500 + i, adam)
        for factor in (0.3, 0.5, None):
            clip = None if factor is None else _clip(factor)
            host = {k: (v.clone() if k != "slab" else v) for k, v in seg.items()}
            _walk([host], st, clip, adam, 1.0 / 7)
            dev, dbase = U.to_cuda(seg, bases)
            _walk([dev], st.cuda(), None if clip is None else clip.cuda(), adam, 1.0 / 7)
            torch.cuda.synchronize()
            who = f"n {n} S {S} off {off} goff {goff} {dtype} adam {adam} factor {factor}"
            for k in keys:
                assert torch.equal(U.ibits(dev[k].cpu()), U.ibits(host[k])), f"{who}: {k}"
                mask = torch.ones_like(bases[k], dtype=torch.bool)
                mask.as_strided(seg[k].shape, seg[k].stride(), seg[k].storage_offset()).fill_(False)
                assert torch.equal(U.ibits(dbase[k].cpu())[mask], U.ibits(bases[k])[mask]), f"{who}: {k} sentinels"
            assert torch.equal(U.ibits(dbase["slab"].cpu()), U.ibits(bases["slab"])), "the slabs are read only"
            if n > 3:
                assert torch.equal(U.ibits(dev["w"].cpu()[:3]), U.ibits(seg["w"][:3])), who
                assert not torch.equal(dev["w"].cpu(), seg["w"]), who
            if factor == 0.5:  # one product in T by 0.5 is exact: the same as halving the slabs first
                pre = {k: v.clone() for k, v in seg.items()}
                pre["slab"] = (seg["slab"] * 0.5).contiguous()
                pd = {k: v.cuda() for k, v in pre.items()}
                _walk([pd], st.cuda(), None, adam, 1.0 / 7)
                for k in keys:
                    assert torch.equal(U.ibits(pd[k].cpu()), U.ibits(dev[k].cpu())), f"{who}: pre-halved {k}"
            if factor is None:  # today's entry point: the native call without a clip argument
                td = {k: v.cuda() if k != "slab" else v.contiguous().cuda() for k, v in seg.items()}
                nat, s = ops.native(), torch.cuda.current_stream().cuda_stream
                if adam:
                    t = ops.AdamTable([td])
                    assert nat.adam_fp(t.f64, t.dev.data_ptr(), 1, 1.0 / 7, st.cuda().data_ptr(), s) == 0
                else:
                    t = ops.SgdSchedTable([td], momentum=True)
                    std = st.cuda()
                    assert nat.sgd_sched_fp(t.f64, t.dev.data_ptr(), 1, 1.0 / 7, 0.25, 1, std.data_ptr(), s) == 0
                torch.cuda.synchronize()
                for k in keys:
                    assert torch.equal(U.ibits(td[k].cpu()), U.ibits(dev[k].cpu())), f"{who}: today's {k}"
    print(f"walker {dtype} adam {adam}: {len(cases)} segments x factors (0.3, 0.5, none) bit-equal")


LAYERS = {"32x32": (32, 32, False), "64x96": (64, 96, False), "128x800": (128, 800, True)}


def _check_copies(W1, Wb, Wt, Wf):
    assert torch.equal(Wb, W1.bfloat16()) and torch.equal(Wt, Wb.t())
    if Wf is not None:
        assert torch.equal(Wf, ops.frag_major(Wb).reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("adam", [False, True], ids=["sched", "adam"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_sub_tile_update_with_a_clip_state(gpu, name, adam):
    """hpnn_sgd_sched_multi / hpnn_adam_update_multi with a clip state, the checks of the walker"""
    N, Kk, frag = LAYERS[name]
    st = _rule_state(adam)
    state = ("V", "A") if adam else ("V",)

    def launch(layers, state_t, clip):
        if adam:
            ops.adam_update_multi(layers, state_t, scale=1.0 / 5, clip=clip)
        else:
            ops.sgd_sched_multi(layers, state_t, alpha=0.2, scale=1.0 / 5, momentum=True, clip=clip)

    for S in (1, 2, 24):
        g = torch.Generator().manual_seed(S)
        c = dict(W=torch.randn(N, Kk, generator=g) / math.sqrt(Kk), V=0.01 * torch.rand(N, Kk, generator=g),
                 A=0.01 * torch.rand(N, Kk, generator=g), G=torch.randn(S, N, Kk, generator=g), frag=frag)
        c["G"][:, -3:, :] = 0.0  # rows that behave like the plan's zero padding
        c["W"][-3:], c["V"][-3:], c["A"][-3:] = 0.0, 0.0, 0.0
        seen = {}
        for factor in (0.3, 0.5, None):
            clip = None if factor is None else _clip(factor)
            d = U.multi_dev(c, state)
            launch([d], st.cuda(), None if clip is None else clip.cuda())
            torch.cuda.synchronize()
            out = [None if t is None else t.cpu() for t in d]
            W1, Wb, Wt, Wf = out[0], out[-3], out[-2], out[-1]
            host = [c["W"].clone()] + [c[k].clone() for k in state]
            launch([tuple(host) + (c["G"], torch.empty_like(Wb), torch.empty_like(Wt), None)], st, clip)
            for i, h in enumerate(host):
                assert torch.equal(U.ibits(out[i]), U.ibits(h)), (name, S, factor, i)
            assert torch.equal(out[len(host)], c["G"])  # the slabs are read only
            assert not W1[-3:].any() and not torch.equal(W1, c["W"])  # g = 0 with zero state keeps w
            _check_copies(W1, Wb, Wt, Wf)
            seen[factor] = out[:len(host)]
        # factor 0.5 == unclipped on slabs halved beforehand; clip=None == today's native entry point
        pre = U.multi_dev(dict(c, G=c["G"] * 0.5), state)
        launch([pre], st.cuda(), None)
        today = U.multi_dev(c, state)
        desc = [tuple(t.data_ptr() for t in today[:len(state) + 2]) + (c["G"].stride(0),) +
                (today[-3].data_ptr(), today[-2].data_ptr(), 0 if today[-1] is None else today[-1].data_ptr(), S, N,
                 Kk)]
        s = torch.cuda.current_stream().cuda_stream
        if adam:
            ops.native().adam_update_multi(desc, 1.0 / 5, st.cuda().data_ptr(), s)
        else:
            ops.native().sgd_sched_multi(desc, 0.2, 1.0 / 5, 1, st.cuda().data_ptr(), s)
        torch.cuda.synchronize()
        for i in range(len(state) + 1):
            assert torch.equal(U.ibits(pre[i].cpu()), U.ibits(seen[0.5][i])), (name, S, "pre-halved", i)
            assert torch.equal(U.ibits(today[i].cpu()), U.ibits(seen[None][i])), (name, S, "today", i)
        assert not torch.equal(seen[0.3][0], seen[None][0])
    print(f"sub-tile {name} adam {adam}: S (1, 2, 24) x factors (0.3, 0.5, none) bit-equal")


# ------------------------------------------------------------------ 5. the factor is read when the launch runs
@pytest.mark.gpu
@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_a_captured_step_reads_its_factor_when_it_runs(gpu, adam):
    """ONE captured graph [partials, finalize, update] replayed with a gradient under the bound,
    then one over it: each replay equals the host, so the factor is not the captured one.  Then
    commit appends and zeroes, and a full history drops the record."""
    n, S = 4099, 3
    g = torch.Generator().manual_seed(2)
    w0 = torch.randn(n, generator=g, dtype=torch.float64)
    small = 1e-3 * torch.randn(S, n, generator=g, dtype=torch.float64)
    big = 10.0 * torch.randn(S, n, generator=g, dtype=torch.float64)
    st = ops.adam_advance(ops.adam_state(lr=0.01)) if adam else ops.lr_advance(ops.lr_state("constant", lr0=0.1))
    keys = ("w", "m", "v") if adam else ("w",)
    hseg = dict(w=w0.clone(), m=torch.zeros(n, dtype=torch.float64), v=torch.zeros(n, dtype=torch.float64),
                slab=small.clone())
    dseg = {k: v.clone().cuda() for k, v in hseg.items()}
    Tab = ops.AdamTable if adam else ops.SgdSchedTable
    th, td = Tab([hseg]), Tab([dseg])
    gh, gd = ops.GnormTable([hseg["slab"]]), ops.GnormTable([dseg["slab"]])
    ph, pd = torch.zeros(gh.count, dtype=torch.float64), torch.zeros(gh.count, dtype=torch.float64, device="cuda")
    ch = ops.clip_state(1.0)
    cd, std = ch.clone().cuda(), st.cuda()

    def step(gt, p, c, tab, state):
        ops.gnorm_partials(gt, p, 0.5)
        ops.clip_finalize(p, gt.count, c)
        if adam:
            ops.adam_update_fp(tab, state, scale=0.5, clip=c)
        else:
            ops.sgd_sched_fp(tab, state, scale=0.5, clip=c)

    # load the code objects before the capture
    warm = {k: v.clone() for k, v in dseg.items()}
    step(ops.GnormTable([warm["slab"]]), pd.clone(), cd.clone(), Tab([warm]), std)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(gd, pd, cd, td, std)
    factors = []
    for grad in (small, big, small):
        hseg["slab"].copy_(grad), dseg["slab"].copy_(grad.cuda())
        graph.replay()
        torch.cuda.synchronize()
        step(gh, ph, ch, th, st)
        assert torch.equal(U.ibits(cd.cpu()), U.ibits(ch))
        for k in keys:
            assert torch.equal(U.ibits(dseg[k].cpu()), U.ibits(hseg[k])), k
        factors.append(ops.read_clip_state(cd)["factor"])
    print(f"adam {adam}: factors of the three replays {factors}")
    assert factors[0] == 1.0 and factors[2] == 1.0 and 0.0 < factors[1] < 0.01
    r = ops.read_clip_state(cd)
    assert (r["steps"], r["clipped"]) == (3, 1) and r["norm_max"] > 1.0 > r["norm_last"]
    hist, cur = ops.clip_history(1, "cuda")
    ops.clip_commit(cd, hist, cur)
    rec = ops.read_clip_history(hist, cur)
    assert rec == [dict(steps=3, clipped=1, norm_max=r["norm_max"], norm_last=r["norm_last"])]
    z = ops.read_clip_state(cd)
    assert (z["steps"], z["clipped"], z["norm_max"], z["norm_last"], z["max_norm"]) == (0, 0, 0.0, 0.0, 1.0)
    graph.replay()
    before = hist.clone()
    ops.clip_commit(cd, hist, cur)  # a full history drops the record and still zeroes
    torch.cuda.synchronize()
    assert int(cur[0]) == 1 and torch.equal(U.ibits(hist), U.ibits(before)) and ops.read_clip_state(cd)["steps"] == 0
    ops.clip_commit(cd)  # no history at all


# ------------------------------------------------------------------ 6. the whole BF16 plan, exact
def _exact_clipped_step(fx, ref, n_valid, lr, alpha, momentum, max_norm):
    """the clipping plan's step restated: the FP64 norm of g = G / n_valid over the three layers
    (every square and every partial sum is exact in FP64 on this fixture, whatever the order), the
    factor, then per element ONE FP32 product g * (float)factor and the FP32 rule"""
    gs = [(G / n_valid) for G in (ref["G0"], ref["G1"], ref["G2"])]
    sumsq = sum(float((g * g).sum()) for g in gs)
    assert all(torch.equal(g.float().double(), g) for g in gs) and sumsq < 2.0 ** 40
    c = Q.Clip(max_norm)
    c.finalize(sumsq)
    f = torch.tensor(c.factor, dtype=torch.float64).float()
    out = []
    for W, g in zip((fx.W0, fx.W1, fx.W2), gs):
        x = g.float() * f if c.factor != 1.0 else g.float()
        d = torch.tensor(lr, dtype=torch.float32) * x
        Wn = W.float() + d
        Vn = d * torch.tensor(alpha, dtype=torch.float32) if momentum else None
        out.append((Wn, Vn, Wn.bfloat16()))
    return out, c


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["t", False], ids=["mode-t", "mode-0"])
@pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])
def test_clipping_plan_steps_exact(gpu, fused, momentum):
    """three steps on the integer-exact fixture (784-128-64-10, batch 256) with 64, 128 and 256
    valid rows, each from the fixture's weights: three different gradients, max_norm = the median
    of their norms, so exactly the largest is clipped"""
    fx = fc.make_mlp3("LNN", 800, 256, 10, u8=True, seed=fc.SEED, n_in=784)
    valid = (64, 128, 256)
    refs = {nv: fc.reference(fx, nv, check=nv >= 128) for nv in valid}
    norms = {nv: math.sqrt(sum(float(((G / nv) ** 2).sum()) for G in (refs[nv]["G0"], refs[nv]["G1"], refs[nv]["G2"])))
             for nv in valid}
    c = float(np.median(list(norms.values())))
    m = MLP([784, 128, 64, 10], "LNN", batch=256, momentum=momentum, fused=fused, clip=c, lr=fc.STEP_LR)
    assert m.fused_mode == (fused or None) and m.plan.clip and not m.plan.sched and not m.plan.g0_fused
    assert not m.plan.tn_update and not m.plan.tn8_side
    Xg = m.prepare_input(fx.X[:, :784].to(torch.uint8), pixel_scale=1.0)
    host = Q.Clip(c)
    for nv in valid:
        for l, W in enumerate((fx.W0, fx.W1, fx.W2)):
            m.W32[l].copy_(W.float())
            if momentum:
                m.V32[l].zero_()
        m.refresh_bf16()
        m.train_step(Xg, labels=fx.labels.cuda(), n_valid=nv, lr=77.0, alpha=fc.STEP_ALPHA)  # lr: ignored
        torch.cuda.synchronize()
        new, one = _exact_clipped_step(fx, refs[nv], nv, fc.STEP_LR, fc.STEP_ALPHA, momentum, c)
        host.finalize(one.sumsq)
        r = ops.read_clip_state(m.clip_state)
        assert Q.same_state(r, host.as_dict()), (nv, r, host.as_dict())
        for l, (W32, V32, Wb) in enumerate(new):
            assert torch.equal(m.W32[l].cpu(), W32), (nv, l)
            if momentum:
                assert torch.equal(m.V32[l].cpu(), V32), (nv, l)
            assert torch.equal(m.Wb[l].cpu(), Wb) and torch.equal(m.Wt[l].cpu(), Wb.t()), (nv, l)
        assert not m.W32[2][10:].any()  # the zero padding of the output layer stays zero
        if m.W0f is not None:
            assert torch.equal(m.W0f.cpu().view(-1), ops.frag_major(new[0][2]).reshape(-1)), nv
    r = ops.read_clip_state(m.clip_state)
    print(f"mode {fused} momentum {momentum}: norms {norms}, max_norm {c}, clipped {r['clipped']}/{r['steps']}")
    assert r["steps"] == 3 and 0 < r["clipped"] < 3
    assert m.plan.clip_launches == 6 and m.plan.sched_launches == 3 and m.plan.side_launches == 0
    hist, cur = ops.clip_history(2, "cuda")
    m.commit_clip(hist, cur)
    assert ops.read_clip_history(hist, cur) == [host.commit()] and m.plan.clip_launches == 7


# ------------------------------------------------------------------ 7. f64 / f32 engines against the CPU oracle
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("clip"))
    return (d,) + tuple(Q.make_data(d))


ENGINE_CASES = [("BPM", None), ("BP", dict(kind="step", gamma=0.5, period=2)), ("ADAM", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tr,sched", ENGINE_CASES, ids=["BPM", "BP-step", "ADAM"])
def test_engine_matches_the_oracle(gpu, data, tr, sched, dtype):
    d, X, T = data[:3]
    lr = 0.01 if tr == "ADAM" else 1.0
    kw = dict(lr_schedule=sched) if sched else {}
    Q.write_conf(d, train=tr, dtype=dtype, epochs=6, lr=lr)
    plain = Q.train(d, "cpu", **kw)
    c, norms = Q.median_norm(plain["w0"], X, T, "SNN", Q.NET["B"], 6, tr, lr=lr) if not sched else (None, None)
    if sched:  # the schedule changes the run: the norms of the unclipped oracle's own records
        huge = Q.train(d, "cpu", clip=1e300, **kw)
        c = float(np.median([r["norm_last"] for r in huge["clip"]] + [r["norm_max"] for r in huge["clip"]]))
    cpu = Q.train(d, "cpu", clip=c, **kw)
    got = Q.train(d, "gpu", clip=c, **kw)
    assert cpu["ok"] and got["ok"]
    steps, clipped = sum(r["steps"] for r in cpu["clip"]), sum(r["clipped"] for r in cpu["clip"])
    tdt = torch.float64 if dtype == "f64" else torch.float32
    tol = 100.0 * A.order_spread(cpu["w0"], X, T, "SNN", Q.NET["B"], dtype=tdt, epochs=6)
    err = A.spread(got["w"], cpu["w"])
    print(f"{tr} {dtype}: max_norm {c:.6g}, clipped {clipped}/{steps}, order spread {tol / 100:.3g}, "
          f"engine - oracle {err:.3g}")
    assert steps == 18 and 0 < clipped < steps
    assert [(r["steps"], r["clipped"]) for r in got["clip"]] == [(r["steps"], r["clipped"]) for r in cpu["clip"]]
    for a, b in zip(got["clip"], cpu["clip"]):
        assert abs(a["norm_max"] - b["norm_max"]) <= 1e-3 * b["norm_max"]
    assert tol > 0.0 and err <= tol
    assert A.spread(cpu["w"], plain["w"]) > 1e-3, "the fixture is at fault: clipping changed nothing"
    assert got["lr"] == cpu["lr"] and (bool(got["lr"]) == bool(sched))
    # the captured replays, the eager launches and a second run: the same bits
    eager = Q.train(d, "gpu", env={"HPNN_GRAPH": "0"}, clip=c, **kw)
    assert eager["raw"] == got["raw"] and eager["clip"] == got["clip"]
    assert Q.train(d, "gpu", clip=c, **kw)["raw"] == got["raw"]


# ------------------------------------------------------------------ 8. the BF16 engine
@pytest.mark.gpu
@pytest.mark.parametrize("net,dims,B,pixels,mode,tr", [
    ("SNN", (784, [128, 64], 10), 256, True, "t", "BPM"),
    ("SNN", (4096, [230], 230), 256, False, "w", "BP"),
    ("ANN", (100, [64, 48], 7), 128, False, None, "ADAM"),
])
def test_train_nn_bf16_equals_python_plan(tmp_path, gpu, net, dims, B, pixels, mode, tr):
    """three clipped epochs of one minibatch each through train_nn -d bf16 -C against the Python
    plan; max_norm = the median of the Python plan's own unclipped norms"""
    n_in, hid, n_out = dims
    n, seed, lr = B - 7, 11, (0.01 if tr == "ADAM" else 0.05)
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (n, n_in)).astype(np.float64) if pixels else rng.uniform(-1, 1, (n, n_in))
    lab = rng.integers(0, n_out, n)
    T = np.full((n, n_out), 0.0 if net == "SNN" else -1.0)
    T[np.arange(n), lab] = 1.0
    d = str(tmp_path)
    capi.pack_arrays(os.path.join(d, "train.hpnb"), X, T)
    formats.write_conf(os.path.join(d, "nn.conf"), name="t", type=net, seed=seed, inputs=n_in, hiddens=hid,
                       outputs=n_out, train=tr, sample_dir="./train.hpnb", test_dir="./train.hpnb",
                       mode="batched", batch=B, epochs=3, dtype="bf16", lr=lr, momentum=0.25)
    o = A.order(n, seed)
    xb = torch.tensor(X[o])
    kw = dict(optimizer="adam") if tr == "ADAM" else dict(momentum=tr == "BPM")

    def plan(clip):
        m = MLP([n_in] + hid + [n_out], net, batch=B, seed=seed, lr=lr, clip=clip, **kw)
        assert m.fused_mode == mode
        Xp = m.prepare_input(xb.to(torch.uint8) if pixels else xb, pixel_scale=1.0)
        Tt = torch.zeros(m.Bp, n_out, device="cuda")
        Tt[:n] = torch.tensor(T[o], dtype=torch.float32, device="cuda")
        norms = []
        for _ in range(3):
            m.train_step(Xp, T=Tt, n_valid=n, alpha=0.25)
            torch.cuda.synchronize()
            norms.append(ops.read_clip_state(m.clip_state)["norm"])
        return m, norms

    c = float(np.median(plan(1e30)[1]))
    m, norms = plan(c)
    r = ops.read_clip_state(m.clip_state)
    print(f"{net} {dims} {tr}: max_norm {c:.6g}, norms {norms}, clipped {r['clipped']}/{r['steps']}")
    assert r["steps"] == 3 and 0 < r["clipped"] < 3
    env = dict(os.environ)
    env.pop("HPNN_FORCE_CPU", None)
    run = subprocess.run([os.path.join(BIN, "train_nn"), "-vvv", "-C", repr(c), "nn.conf"], cwd=d, env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"batched plan: mode {mode or '-'}" in run.stdout, run.stdout[-3000:]
    assert run.stdout.count("gradient clipping: max norm") == 1 and "LR: epoch" not in run.stdout
    lines = [ln.split("CLIP: ")[1] for ln in run.stdout.splitlines() if "CLIP: epoch" in ln]
    assert lines == [f"epoch {e + 1} steps=1 clipped={int(norms[e] > c)} max_norm={norms[e]:.17g} "
                     f"last_norm={norms[e]:.17g}" for e in range(3)]
    got = formats.read_kernel(os.path.join(d, "kernel.opt"))["weights"]
    for a, w in zip(got, m.W32):
        ref = w[:a.shape[0], :a.shape[1]].double().cpu().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), ref), np.abs(a - ref).max()
        assert not w[a.shape[0]:].any() and not w[:, a.shape[1]:].any()


# ------------------------------------------------------------------ 9. resume, keep-best, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resume_through_the_state_file_is_exact(gpu, data, dtype):
    d, X, T = data[:3]
    kw = dict(train="BPM", dtype=dtype, lr=1.0)
    Q.write_conf(d, epochs=4, **kw)
    plain = Q.train(d, "gpu")
    c = Q.median_norm(plain["w0"], X, T, "SNN", Q.NET["B"], 4, "BPM", lr=1.0)[0]
    whole = Q.train(d, "gpu", clip=c)
    Q.write_conf(d, epochs=2, **kw)
    h1 = Q.train(d, "gpu", dump="two.bin", clip=c)
    rest = Q.train(d, "gpu", load="two.bin", clip=c)
    assert whole["ok"] and rest["ok"] and rest["epochs_done"] == 4
    clipped = sum(r["clipped"] for r in whole["clip"])
    print(f"{dtype}: max_norm {c:.6g}, clipped {clipped}/12")
    assert 0 < clipped < 12 and h1["clip"] + rest["clip"] == whole["clip"]
    assert rest["raw"] == whole["raw"] and len(whole["raw"]) == len(plain["raw"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_keep_best_equals_the_best_epochs_run(gpu, data, dtype):
    d, X, T = data[:3]
    kw = dict(train="BPM", dtype=dtype, validate=1, lr=2.0)
    Q.write_conf(d, epochs=10, **kw)
    plain = Q.train(d, "cpu")
    c = Q.median_norm(plain["w0"], X, T, "SNN", Q.NET["B"], 10, "BPM", lr=2.0)[0]
    kept = Q.train(d, "gpu", clip=c, keep_best="loss", patience=3)
    assert kept["ok"]
    b = kept["best"]["epoch"]
    clipped, steps = sum(r["clipped"] for r in kept["clip"]), sum(r["steps"] for r in kept["clip"])
    print(f"{dtype}: best epoch {b}, {len(kept['val'])} passes, clipped {clipped}/{steps}")
    assert 1 <= b < 10 and kept["epochs_done"] == b and len(kept["clip"]) == len(kept["val"])
    assert 0 < clipped < steps
    Q.write_conf(d, epochs=b, **kw)
    e = Q.train(d, "gpu", clip=c)
    assert e["raw"] == kept["raw"] and e["clip"] == kept["clip"][:b]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_keep_best_with_adam_plateau_and_clip_equals_the_best_epochs_run(gpu, data, dtype):
    """the one snapshot that carries both trailing segments, the Adam state and the schedule state,
    behind the three per layer; the rate and the epochs were chosen on the FP64 CPU engine: best
    pass 5, plateau cuts before epochs 7 and 8, the stop at pass 8 of 12, 11 of 24 steps clipped"""
    d = data[0]
    epochs, lr, sched = 12, 0.03, dict(kind="plateau", gamma=0.5, patience=1)
    kw = dict(train="ADAM", dtype=dtype, validate=1, lr=lr)
    Q.write_conf(d, epochs=epochs, **kw)
    huge = Q.train(d, "gpu", clip=1e300, lr_schedule=sched)  # unclipped: the norms of its own records
    assert huge["ok"]
    c = float(np.median([r["norm_last"] for r in huge["clip"]] + [r["norm_max"] for r in huge["clip"]]))
    kept = Q.train(d, "gpu", clip=c, lr_schedule=sched, keep_best="loss", patience=3)
    assert kept["ok"]
    b = kept["best"]["epoch"]
    clipped, steps = sum(r["clipped"] for r in kept["clip"]), sum(r["steps"] for r in kept["clip"])
    print(f"{dtype}: max_norm {c:.6g}, best epoch {b}, {len(kept['val'])} passes, clipped {clipped}/{steps}, "
          f"rates {kept['lr']}")
    assert 1 < b < epochs, "the fixture is at fault: the best pass is the first or the last"
    assert min(kept["lr"]) < lr, "the fixture is at fault: no plateau cut"
    assert 0 < clipped < steps, "the fixture is at fault: every step or no step clipped"
    assert kept["epochs_done"] == b and len(kept["clip"]) == len(kept["lr"]) == len(kept["val"])
    Q.write_conf(d, epochs=b, **kw)
    plain = Q.train(d, "gpu", clip=c, lr_schedule=sched)
    assert plain["raw"] == kept["raw"] and plain["clip"] == kept["clip"][:b]
    assert [Q.bits(x) for x in plain["lr"]] == [Q.bits(x) for x in kept["lr"][:b]]


@pytest.mark.gpu
@pytest.mark.parametrize("env,msg", [
    ({"HPNN_LOOPBACK_RANKS": "2"}, "[clip] is not supported by data-parallel batched training"),
    ({"HPNN_PARALLEL": "tp"}, "[clip] is not supported by tensor-parallel batched training"),
])
def test_engine_refusals(gpu, data, capfd, env, msg):
    d = data[0]
    Q.write_conf(d, train="BPM", dtype="f32", epochs=2)
    r = Q.train(d, "gpu", env=env, dump=None, clip=0.5)
    out = capfd.readouterr()
    assert not r["ok"] and (out.err + out.out).count(msg) == 1 and "BP, BPM and ADAM on one GPU" in out.err + out.out
    assert all(np.array_equal(a, b) for a, b in zip(r["w"], r["w0"]))
    m = MLP([784, 128, 64, 10], "SNN", batch=256, clip=0.5, lr=0.01)
    with pytest.raises(RuntimeError):
        m.update_layer(0, 0.1, 0.0, 1.0)


# ------------------------------------------------------------------ 10. an unclipped plan is untouched
@pytest.mark.gpu
def test_an_unclipped_plan_launches_no_clip_kernel(gpu):
    torch.manual_seed(0)
    B = 256
    X = torch.rand(B, 784)
    lab = torch.randint(0, 10, (B,), dtype=torch.int32, device="cuda")
    m = MLP([784, 128, 64, 10], "SNN", batch=B, momentum=True, seed=3)
    assert not m.clip and m.clip_state is None and not m.plan.clip and m.plan.clip_count == 0
    assert m.plan.g0_fused and m.plan.tn_update and m.plan.tn8_side  # the fused steps stay on
    assert not any(name in ("clip", "clip_part", "clip_tab", "lrs") for name, *_ in m.plan.buffers())
    Xd = m.prepare_input(X)
    c = MLP([784, 128, 64, 10], "SNN", batch=B, momentum=True, seed=3, clip=1e30, lr=0.01)
    assert [name for name, *_ in c.plan.buffers() if name.startswith("clip")] == ["clip", "clip_part", "clip_tab"]
    for _ in range(2):
        m.train_step(Xd, labels=lab, lr=0.01, alpha=0.2)
        c.train_step(Xd, labels=lab, alpha=0.2)
    torch.cuda.synchronize()
    assert m.plan.clip_launches == 0 and m.plan.sched_launches == 0
    assert c.plan.clip_launches == 4 and c.plan.sched_launches == 2
    with pytest.raises(RuntimeError):
        m.commit_clip()
    with pytest.raises(RuntimeError):
        c.advance_schedule()  # [clip] alone is no schedule
    r = ops.read_clip_state(c.clip_state)
    assert (r["steps"], r["clipped"], r["factor"]) == (2, 0, 1.0) and r["norm_max"] > 0.0
