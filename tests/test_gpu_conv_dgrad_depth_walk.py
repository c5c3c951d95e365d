"""The depth-walk form of the 8^3 -> 16^3 LDS-halo input gradient: conv_dgrad_halo_dwalk_kernel (conv3d_halo.hip).  It does the work of
conv_dgrad_halo_kernel<0> on dy grids of depth 8 with another split of the work — a workgroup is (sample, 8 x 8 h/w tile, depth half,
output parity ph) and walks its two plane pairs x (pd, pw); a wave's two column tiles are the two depth planes of a pair — and does
not issue the tiles whose dy operand is the zero padding beyond the depth range (plane 0 with td 1 at pd 0, plane 7 with td 0 at
pd 1).  Bodies, patterns, references (float64 on the CPU) and tolerances are those of tests/conv_patterns.py, unchanged.

Case -> kernel, forced through conv_dgrad_halo_raw(impl = 129) = conv_dgrad_halo_dwalk_kernel + pack_dgrad_frag_kernel (mode 0); the
kernel table of tests/test_gpu_conv_grids.py stays as it is (a forced call WITHOUT bit 128 still runs the kernels named there):
    (1, 64, 32) on dy 8^3      two stages per pass, one sample
    (3, 72, 32) on dy 8^3      odd batch, rows 64 + 8 (two row tiles)
    (2, 40, 64) on dy 8^3      a cut row tile, four stages per pass
    (2, 64, 32) on dy 8x16x8   two h tiles
    (2, 64, 32) on dy 8x8x16   two w tiles
dispatch: ops.conv_dgrad_raw at 128 samples x 64 x 32 (512 workgroups) takes the new form, at 16 samples conv_dgrad_halo_kernel<0>;
ops.conv_dgrad_form (host code) names the kernel on both sides of the 512-workgroup boundary (also tests/test_conv_dgrad_form_host.py,
which needs no GPU).  The forced entries have no twin (the twin models no kernel forms), so nothing here is repeated on it.

"Counting" inputs (tests/test_gpu_conv_depth_skip.py): dy = 1 everywhere and weights (1 + tap index) * (1 + co % 3), so that every sum
is a small integer, exact in fp32 in any order: a tap wrongly dropped or wrongly kept is an error of at least 1 at a named position.
"""
import pytest
import torch
import torch.nn.functional as F

from shapegan_amd.lib import ACT_LEAKY, ACT_NONE

import conv_patterns as CP
import test_gpu_ops as OPS
import test_gpu_unwritten as UNW

pytestmark = pytest.mark.gpu

WALK = 128 + 1                       # impl of sg_conv3d_k4s2p1_dgrad_impl: forced, depth-walk form
G8 = (8, 8, 8)
CASES = [(1, 64, 32, G8), (3, 72, 32, G8), (2, 40, 64, G8), (2, 64, 32, (8, 16, 8)), (2, 64, 32, (8, 8, 16))]
FORM_ROWS64, FORM_DEPTH_WALK = 5, 6      # SG_DGRAD_FORM_ROWS64 / _DEPTH_WALK of include/shapegan_hip.h


def _first_bad(got, ref):
    bad = (got != ref).nonzero()
    return "first of %d wrong elements at (n, c, d, h, w) = %s: got %r, expected %r" % (
        bad.shape[0], tuple(int(v) for v in bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])])) if bad.numel() else "equal"


def _counting_weights(Co, Ci):
    tap = torch.arange(1, 65, dtype=torch.float32).view(1, 1, 4, 4, 4)
    return tap * (1 + torch.arange(Co) % 3).float().view(Co, 1, 1, 1, 1) * torch.ones(1, Ci, 1, 1, 1)


@pytest.mark.parametrize("pattern", CP.PATTERNS)
@pytest.mark.parametrize("N,Ci,Co,grid", CASES)
def test_by_position(N, Ci, Co, grid, pattern):
    """ConvTranspose3d forward: random (bias + LeakyReLU) and the by-position patterns (no bias, no activation, exact support)."""
    CP.body_dgrad_halo(N, Ci, Co, grid, pattern, (WALK,))


@pytest.mark.parametrize("act", [ACT_NONE, ACT_LEAKY])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,Ci,Co,grid", CASES)
def test_bias_and_activation(N, Ci, Co, grid, bias, act):
    """Without bias and activation this is the Conv3d input gradient (reference: float64 autograd of F.conv3d); with them the
    ConvTranspose3d forward (reference: F.conv_transpose3d)."""
    from shapegan_amd import ops
    dy, w, b, _ = CP.dgrad_inputs(N, Ci, Co, grid, "random", act)
    b = b if bias else None
    if b is None and act == ACT_NONE:
        ref = CP.conv_reference(torch.zeros(N, Ci, *(2 * e for e in grid)), w, None, dy)[1]
    else:
        ref = CP._act(F.conv_transpose3d(dy.double(), w.double(), None if b is None else b.double(), stride=2, padding=1), act).float()
    got = ops.conv_dgrad_halo_raw(OPS.dev(dy), OPS.dev(w), None if b is None else OPS.dev(b), Ci, act, 0.2, impl=WALK)
    CP.check(got, ref, "dgrad depth-walk", "%s bias %d act %d" % (CP._what(N, Ci, Co, *grid), bias, act))


@pytest.mark.parametrize("N,Ci,Co,grid", CASES)
def test_counting(N, Ci, Co, grid):
    from shapegan_amd import ops
    dy, w = torch.ones(N, Co, *grid), _counting_weights(Co, Ci)
    ref = F.conv_transpose3d(dy.double(), w.double(), None, stride=2, padding=1).float()
    assert float(ref.max()) < 2 ** 24 and len(set(ref[0, 0, :, 3, 3].tolist())) >= 4      # exact in fp32; the depth border shows
    got = ops.conv_dgrad_halo_raw(OPS.dev(dy), OPS.dev(w), None, Ci, ACT_NONE, 0.0, impl=WALK).cpu()
    planes = sorted(set(int(d) for d in (got != ref).nonzero()[:, 2]))
    print("[conv-grid] dgrad depth-walk | counting %s | %s | wrong depth planes %s" % (CP._what(N, Ci, Co, *grid), _first_bad(got, ref), planes))
    assert torch.equal(got, ref), "wrong depth planes %s: %s" % (planes, _first_bad(got, ref))


@pytest.mark.parametrize("N,Ci,Co,grid", CASES)
def test_new_against_present_form(N, Ci, Co, grid):
    """Same k order per accumulator, dropped products have B = 0: bit-equal for finite inputs (torch.equal: -0 == +0)."""
    from shapegan_amd import ops
    dy, w, b, ref = CP.dgrad_inputs(N, Ci, Co, grid, "random", ACT_LEAKY)
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    new = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=WALK)
    old = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=1)
    print("[conv-grid] dgrad depth-walk | against the present form %s | max |new - old| %.3g" % (
        CP._what(N, Ci, Co, *grid), float((new - old).abs().max())))
    assert torch.equal(new, old), _first_bad(new.cpu(), old.cpu())
    raw_new = ops.conv_dgrad_halo_raw(dyg, wg, None, Ci, ACT_NONE, 0.0, impl=WALK)      # the Conv3d input gradient
    assert torch.equal(raw_new, ops.conv_dgrad_halo_raw(dyg, wg, None, Ci, ACT_NONE, 0.0, impl=1))


def test_every_element_written():
    from shapegan_amd import ops
    for N, Ci, Co, grid in (CASES[1], CASES[3]):
        dy, w, b, ref = CP.dgrad_inputs(N, Ci, Co, grid, "random", ACT_LEAKY)
        dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
        what = "dgrad depth-walk %s" % CP._what(N, Ci, Co, *grid)
        UNW.run_form(lambda: ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=WALK),
                     lambda o: OPS.close(o[0], ref, what=what + " under poison"), what=what)


def test_infinite_weight_on_depth_padding_taps():
    """Output depth 0 (pd 0, q 0) reads kd 1 on dy depth 0 and kd 3 on depth -1; output depth 15 (pd 1, q 7) reads kd 2 on dy depth 7
    and kd 0 on depth 8.  With w[.., kd = 0 and 3, ..] = inf the depth-walk form returns the in-range sums in these two planes (the
    present form: NaN = 0 x inf); every other plane reads kd 0 or kd 3 on data and is not finite in either form."""
    from shapegan_amd import ops
    N, Ci, Co, grid = CASES[0]
    dy, w, _, _ = CP.dgrad_inputs(N, Ci, Co, grid, "random", ACT_NONE)
    w0, winf = w.clone(), w.clone()
    w0[:, :, 0] = 0
    w0[:, :, 3] = 0
    winf[:, :, 0] = float("inf")
    winf[:, :, 3] = float("inf")
    ref = F.conv_transpose3d(dy.double(), w0.double(), None, stride=2, padding=1).float()
    got = ops.conv_dgrad_halo_raw(dy.cuda(), winf.cuda(), None, Ci, ACT_NONE, 0.0, impl=WALK).cpu()
    assert bool(torch.isfinite(got[:, :, 0]).all()) and bool(torch.isfinite(got[:, :, 15]).all())
    assert not bool(torch.isfinite(got[:, :, 1:15]).any())
    CP.check(got[:, :, 0], ref[:, :, 0], "dgrad depth-walk", "output depth 0 under infinite kd = 0, 3 weights")
    CP.check(got[:, :, 15], ref[:, :, 15], "dgrad depth-walk", "output depth 15 under infinite kd = 0, 3 weights")


@pytest.mark.parametrize("N,Ci,Co,grid,impl", [
    (2, 64, 32, (4, 8, 8), WALK), (2, 64, 32, (16, 8, 8), WALK),      # dy depth 4 and 16
    (2, 64, 16, G8, WALK), (2, 64, 48, G8, WALK),                      # an odd stage count
    (2, 32, 32, G8, WALK),                                             # 32-row workgroups
    (2, 64, 32, G8, WALK + 8), (2, 64, 32, G8, WALK + 2), (2, 64, 32, G8, WALK + 64),      # with a ppw / one-parity / depth-skip bit
])
def test_refusals(N, Ci, Co, grid, impl):
    from shapegan_amd import ops
    dy, w = torch.randn(N, Co, *grid).cuda(), torch.randn(Co, Ci, 4, 4, 4).cuda()
    with pytest.raises(RuntimeError, match="not eligible"):
        ops.conv_dgrad_halo_raw(dy, w, None, Ci, ACT_NONE, 0.0, impl=impl)


def test_dispatch():
    """128 samples x 64 x 32 on 8^3 are 512 depth-walk workgroups: the plain entry, ConvTranspose3d forward and Conv3d backward are
    bit-equal to the forced new form.  16 samples stay on conv_dgrad_halo_kernel<0>."""
    from shapegan_amd import ops
    Ci, Co = 64, 32
    dy, w, b, ref = CP.dgrad_inputs(16, Ci, Co, G8, "random", ACT_LEAKY)
    dy128 = dy.repeat(8, 1, 1, 1, 1).cuda()
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    assert ops.conv_dgrad_form(128, Ci, Co, G8) == FORM_DEPTH_WALK and ops.conv_dgrad_form(127, Ci, Co, G8) == FORM_ROWS64
    assert ops.conv_dgrad_form(16, Ci, Co, G8) == FORM_ROWS64
    forced = ops.conv_dgrad_halo_raw(dy128, wg, bg, Ci, ACT_LEAKY, 0.2, impl=WALK)
    plain = ops.conv_dgrad_raw(dy128, wg, bg, Ci, ACT_LEAKY, 0.2)
    CP.check(plain[:16], ref, "dgrad dispatch", CP._what(128, Ci, Co) + ", samples 0-15")
    CP.check(plain[112:], ref, "dgrad dispatch", CP._what(128, Ci, Co) + ", samples 112-127")
    assert torch.equal(plain, forced)
    with torch.no_grad():                      # ConvTranspose3d(Co -> Ci) forward: weight [in = Co, out = Ci, 4, 4, 4]
        assert torch.equal(ops.conv_transpose3d_k4s2p1(dy128, wg, bg, ACT_LEAKY, 0.2), forced)
    xg = torch.zeros(128, Ci, 16, 16, 16, device="cuda", requires_grad=True)      # Conv3d(Ci -> Co) backward
    ops.conv3d_k4s2p1(xg, wg, None).backward(dy128)
    assert torch.equal(xg.grad, ops.conv_dgrad_halo_raw(dy128, wg, None, Ci, ACT_NONE, 0.0, impl=WALK))
    small = ops.conv_dgrad_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2)
    CP.check(small, ref, "dgrad dispatch", CP._what(16, Ci, Co))
    assert torch.equal(small, ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=1))
