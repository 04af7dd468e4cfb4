"""The 8-phase TN update kernels (csrc/gpu/kernels_8ph.hip: gemm_tn8_kernel MODE 1, 2, 2 + side
job, 3 and the 256 x 128 tile instantiation) against exact float64 references, bitwise.

Cases, references and check functions: tests/tn8_common.py (run on CPU tensors by
test_tn8_cpu.py).  Every case launches three times on one weight state / slab / ticket block
with fresh integer operands, and compares W32, V32, Wb, Wt (MODE 3: G16), the published partial
slabs, the sentinel-filled surroundings of every buffer and the protocol words after each launch."""
import os
import subprocess
import sys

import pytest
import torch

from tests import tn8_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BP_BPM = pytest.mark.parametrize("momentum", [False, True], ids=["BP", "BPM"])


# ---------------------------------------------------------------------------- MODE 1
@BP_BPM
@pytest.mark.parametrize("shape", tc.MODE1_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_mode1_exact(gpu, shape, momentum):
    """one split, the step in the epilogue, W^T through LDS: 1, 2, 3, 9 and 10 tiles (the XCD-aware
    tile map at counts below and not a multiple of 8), tiles_n != tiles_m, 1 to 3 iterations"""
    tc.check_mode1(gpu, *shape, momentum)


@BP_BPM
@pytest.mark.parametrize("shape", tc.MODE1_PADDED, ids=lambda s: "%dx%dx%d" % s)
def test_mode1_padded_operands(gpu, shape, momentum):
    """D, H as column slices of wider tensors (ldd = N + 32, ldh = M + 64)"""
    tc.check_mode1(gpu, *shape, momentum, padded=True)


def test_mode1_refusals_write_nothing(gpu):
    """N = 288, Bt = 192, W32 off by 4 bytes, Wt off by 8 bytes (its rows leave in 16-byte pieces),
    momentum without V32: False, every buffer still at its sentinel"""
    tc.check_mode1_refused(gpu)


@BP_BPM
def test_mode1_random(gpu, momentum):
    """random BF16 operands, an ordinary step: the FP32 rounding and BF16 conversion paths on
    values that are not exact, at the tolerance of test_gemm_tn"""
    tc.check_mode1_random(gpu, momentum)


# ---------------------------------------------------------------------------- MODE 3
@pytest.mark.parametrize("case", tc.MODE3_CASES, ids=lambda c: "%dx%dx%d_ldg%d" % c)
def test_mode3_exact(gpu, case):
    """the gradient rounded once to BF16; a padded ldg keeps its padding columns"""
    tc.check_mode3(gpu, *case)


def test_mode3_random(gpu):
    tc.check_mode3_random(gpu)


def test_mode3_ok_agrees_with_the_launcher(gpu):
    from hpnn_amd import ops
    tc.check_mode3_ok_agrees(gpu, ops.gemm_tn_bf16out_ok)


# ---------------------------------------------------------------------------- MODE 2
def _mode2_ready(gpu):
    """the MODE 2 cases are laid out for 256 CUs and the default launcher settings"""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if cus != tc.CUS:
        pytest.skip("the fused-update cases need %d CUs (grid between CUs / 2 and one workgroup per CU); "
                    "this device has %d" % (tc.CUS, cus))
    for k in ("HPNN_TN8_FUSED", "HPNN_TN8_MINWG", "HPNN_TN8_TM"):
        if k in os.environ:
            pytest.skip("%s is set: it changes what the fused-update launcher accepts (read once per process)" % k)
    assert cus == tc.CUS


@BP_BPM
@pytest.mark.parametrize("case", tc.MODE2_CASES, ids=lambda c: "%dx%d_s%d_b%d" % c)
def test_mode2_exact(gpu, case, momentum):
    """split-K partials published write-through, per-tile tickets, each split reduces and steps
    1 / splits of its tile: split counts 5, 7, 9, 20, 192 next to 16 and 128, 1 to 32 tiles, one and
    two iterations per split"""
    _mode2_ready(gpu)
    tc.check_mode2(gpu, *case, momentum)


@BP_BPM
def test_mode2_padded_operands(gpu, momentum):
    _mode2_ready(gpu)
    tc.check_mode2(gpu, *tc.MODE2_CASES[2], momentum, padded=True)


def test_mode2_wt_needs_no_alignment(gpu):
    """MODE 2 writes W^T one BF16 at a time (its reduction walks W row-wise), so unlike MODE 1 its
    launcher rightly does not ask for an aligned Wt: one 2 bytes off is accepted and correct"""
    _mode2_ready(gpu)
    tc.check_mode2(gpu, *tc.MODE2_CASES[3], True, wt_offset=1)


def test_mode2_misaligned_w32_refused(gpu):
    _mode2_ready(gpu)
    N, M, splits, Bt = tc.MODE2_CASES[3]
    F = tc.Fused(gpu, N, M, Bt, splits, w32_offset=1)
    D, H = tc.int_operands(Bt, N, M, tc._gen(0), gpu)
    assert F.launch(D, H, True) == -1 and F.untouched()


def test_mode2_repeatable(gpu):
    """the same start state twice: bitwise equal, and (exact data) equal to the reference"""
    _mode2_ready(gpu)
    a = tc.check_mode2(gpu, *tc.MODE2_CASES[4], True)
    b = tc.check_mode2(gpu, *tc.MODE2_CASES[4], True)
    for x, y in zip(a.L.all + (a.slab,), b.L.all + (b.slab,)):
        assert torch.equal(x.raw, y.raw)


@BP_BPM
def test_mode2_random(gpu, momentum):
    """random BF16 operands twice from one start state: the tolerance of test_gemm_tn, and the
    fixed reduction order makes the two runs bitwise equal"""
    _mode2_ready(gpu)
    tc.check_mode2_random(gpu, momentum)


@pytest.mark.parametrize("case", tc.MODE2_REFUSED, ids=lambda c: "%dx%d_s%d_b%d" % c)
def test_mode2_refusals_write_nothing(gpu, case):
    """one split; above the capacity; below the minimum grid; an odd number of units per split;
    33 tiles: -1, no buffer, slab or ticket written"""
    _mode2_ready(gpu)
    tc.check_mode2_refused(gpu, case)


# ---------------------------------------------------------------------------- MODE 2 + side job
@BP_BPM
@pytest.mark.parametrize("i", range(4))
def test_side_job_exact(gpu, i, momentum):
    """the next layer's gradient and step on half-workgroups of the same launch: both layers, both
    slabs and both ticket words; case 1 with padded strides of the side operands"""
    _mode2_ready(gpu)
    case, N1, M1, S, fits = tc.SIDE_CASES[i]
    assert fits
    tc.check_mode2(gpu, *case, momentum, side=(N1, M1, S), side_padded=i == 1)


def test_side_job_that_does_not_fit(gpu):
    """144 pieces over 288 half-workgroups: -2 and nothing written, neither layer"""
    _mode2_ready(gpu)
    case, N1, M1, S, fits = tc.SIDE_CASES[4]
    assert not fits
    tc.check_mode2_refused(gpu, case, rc_want=-2, side=(N1, M1, S))


@BP_BPM
def test_side_job_random(gpu, momentum):
    _mode2_ready(gpu)
    case, N1, M1, S, _ = tc.SIDE_CASES[2]
    tc.check_mode2_random(gpu, momentum, case=case, side=(N1, M1, S))


# ---------------------------------------------------------------------------- TM = 128
def test_tm128_in_a_child_process(gpu):
    """HPNN_TN8_TM=128 is read once per process: a fresh child runs two MODE 2 cases on the 256 x 128
    tile instantiation through the same check (which also sees that exactly the first splits / 2
    slabs were written, i.e. that the variant ran)"""
    _mode2_ready(gpu)
    env = dict(os.environ)
    env["HPNN_TN8_TM"] = "128"
    code = ("import sys; sys.path.insert(0, %r); import torch; from tests import tn8_common as tc; "
            "tc.check_tm128(torch.device('cuda:0'))" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=170, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
